// Teacher-forced decode (Tacotron2.forward in eval, layers/tacotron2.py:300-333): prenet layer 1 of
// every teacher frame in one launch, before the persistent decoder starts.
//
// Step t >= 1 of row m feeds the prenet the ground-truth frame mel[b][t r - 1] (_update_memory: the
// last frame of group t - 1), b = map[m] the caller's row of decode row m. The frames are known
// before the decode, so layer 1 for all steps and rows is one (S Bp x 80) . (80 x 256) GEMM:
//   teach[t - 1][m][n] = sum_k mel[b][t r - 1][k] W1[n][k] + b1'[n]     (b1': BN prenet, else none)
// written row-major [step][decode row][256], the order P1 of persist_decoder_kernel<.., V_TEACH>
// consumes (a lane's f32x4 at row m, columns 16 kc + 4 (lane >> 4) ..).
//
// Workgroup = one 16-row tile (one step, 16 decode rows) x 256 columns: 4 waves x 4 column tiles,
// K = 80 as 5 chunks of 16 on the fp32 16x16x4 MFMA (exact f32 products, k-ordered). W1 is the
// stepwise path's swizzled layer-1 weight (TacoModel::pre1, [16 tiles][5][64][4]). A row past the
// batch, or at a step the row does not take (t >= max_steps[m]: never read for a live row, and the
// caller's padding must not reach the range check of the split-f16 GEMMs), gets a zero frame.
#include "common.h"
#include "decoder.h"

namespace {

__global__ __launch_bounds__(256) void teacher_prenet_kernel(TeachArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int MT = a.Bp >> 4;
  const int step = blockIdx.x / MT, mt = blockIdx.x - step * MT;  // teach[step] feeds decoder step t = step + 1
  const int t = step + 1;
  const int m = mt * 16 + (lane & 15);
  const bool live = m < a.B && t < a.max_steps[min(m, a.B - 1)];
  f32x4 x[5];
#pragma unroll
  for (int kc = 0; kc < 5; ++kc) x[kc] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (live) {
    // (t r - 1) < M_max: t <= S_m - 1 and (S_m - 1) r - 1 < M_m <= M_max
    const float* fr = a.mel + (long)a.map[m] * a.mel_b + (long)(t * a.r - 1) * 80 + 4 * (lane >> 4);
#pragma unroll
    for (int kc = 0; kc < 5; ++kc) x[kc] = *reinterpret_cast<const f32x4*>(fr + kc * 16);
  }
  f32x4 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4* W = reinterpret_cast<const f32x4*>(a.W1) + lane;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int tile = 4 * wave + c;
#pragma unroll
    for (int kc = 0; kc < 5; ++kc) {
      const f32x4 w = W[(tile * 5 + kc) * 64];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[c] = MFMA16(x[kc][q], w[q], acc[c]);
    }
  }
  // D: column lane & 15, rows 4 (lane >> 4) + j
  float* out = a.teach + ((long)step * a.Bp + mt * 16 + 4 * (lane >> 4)) * 256 + (lane & 15);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int n = (4 * wave + c) * 16;
    const float b = a.b1 ? a.b1[n + (lane & 15)] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(long)j * 256 + n] = acc[c][j] + b;
  }
}

}  // namespace

void launch_teacher_prenet(const TeachArgs& a, hipStream_t s) {
  TTS_CHECK(a.B >= 1 && a.B <= a.Bp && a.Bp % 16 == 0 && a.Bp <= BMAX && a.r >= 1 && a.steps >= 1,
            "teacher prenet: sizes");
  TTS_CHECK(reinterpret_cast<uintptr_t>(a.mel) % 16 == 0 && a.mel_b % 4 == 0, "teacher prenet: mel_specs must be 16-byte aligned");
  teacher_prenet_kernel<<<dim3((unsigned)(a.steps * (a.Bp / 16))), 256, 0, s>>>(a);
  HIP_OK(hipGetLastError());
}
