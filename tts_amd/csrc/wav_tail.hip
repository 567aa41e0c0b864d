// The waveform tail: normalised linear spectrogram -> Griffin-Lim magnitudes (audio.py:232-239),
// de-emphasis (scipy.signal.lfilter([1], [1, -a], x), audio.py:204-207) and the end of
// Synthesizer.tts (server/synthesizer.py:179-193 with audio.py:302-309, 335-337): endpoint per row,
// rows joined with gaps, one peak, 16-bit samples. fp32; every kernel is an ordinary launch, every
// loop runs to a length the host has checked, every output has one fixed order of operations that
// depends on its own row alone.
#include "common.h"
#include "launch.h"

namespace {

// S = (10 ^ ((clip(x) scale + offset) / gain)) ^ power per element: grid (ceil(M_max F / 256), B)
__global__ void __launch_bounds__(256)
    spec_to_mag_kernel(const float* __restrict__ x, RowInts lens, int M_max, int F, const float* __restrict__ scale,
                       const float* __restrict__ offset, float clip_lo, float clip_hi, int use_clip, float gain,
                       float power, float* __restrict__ S) {
  const int b = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M_max * F) return;
  const int t = (int)(i / F), k = (int)(i - (long)t * F);
  float v = 0.f;
  if (t < lens.v[b]) {
    float a = x[(size_t)b * M_max * F + i];
    if (use_clip) a = fminf(fmaxf(a, clip_lo), clip_hi);
    v = powf(powf(10.f, (a * scale[k] + offset[k]) / gain), power);
  }
  S[(size_t)b * M_max * F + i] = v;
}

// y[n] = x[n] + a y[n-1] as a scan over the affine maps y -> a^len y + e of DE_C-sample chunks.
// One workgroup per row walks the row in tiles of DE_T chunks: thread j runs chunk j from zero
// (thread 0 from the previous tile's last output), the chunk ends e_j are combined by a
// Hillis-Steele scan in a fixed order (at distance 2^s the multiplier is a^(DE_C 2^s), from the
// host's table), and every thread adds a^(i+1) times the output before its chunk. Only the last
// chunk of a row can be short, and nothing is combined after it. The tile goes through LDS, so
// out may be in.
__global__ void __launch_bounds__(DE_T)
    deemphasis_kernel(const float* in, float* out, RowInts ns, int L_max, DeemphTable tab) {
  __shared__ float x[DE_T * (DE_C + 1)];  // sample p at p + p / DE_C: chunk rows one bank apart
  __shared__ float e[2][DE_T];
  const int b = blockIdx.x, j = threadIdx.x, n = ns.v[b];
  const float* src = in + (size_t)b * L_max;
  float* dst = out + (size_t)b * L_max;
  float carry = 0.f;
  for (int base = 0; base < n; base += DE_T * DE_C) {
    const int cnt = min(DE_T * DE_C, n - base);
    for (int p = j; p < cnt; p += DE_T) x[p + p / DE_C] = src[base + p];
    __syncthreads();
    const int m = min(DE_C, max(0, cnt - j * DE_C));
    float* mine = x + j * (DE_C + 1);
    float loc[DE_C];
    float y = j == 0 ? carry : 0.f;
#pragma unroll
    for (int i = 0; i < DE_C; ++i) {
      if (i < m) y = fmaf(tab.pw[1], y, mine[i]);
      loc[i] = y;
    }
    e[0][j] = y;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int s = 0; s < DE_LOG; ++s) {
      float v = e[cur][j];
      if (j >= (1 << s)) v = fmaf(tab.pwc[s], e[cur][j - (1 << s)], v);
      e[cur ^ 1][j] = v;
      __syncthreads();
      cur ^= 1;
    }
    const float before = j == 0 ? 0.f : e[cur][j - 1];  // thread 0 started from the carry itself
    carry = e[cur][DE_T - 1];
#pragma unroll
    for (int i = 0; i < DE_C; ++i)
      if (i < m) mine[i] = fmaf(tab.pw[i + 1], before, loc[i]);
    __syncthreads();
    for (int p = j; p < cnt; p += DE_T) dst[base + p] = x[p + p / DE_C];
    __syncthreads();
  }
  for (int p = n + j; p < L_max; p += DE_T) dst[p] = 0.f;
}

// maximum over the workgroup's 256 threads, in every thread
__device__ __forceinline__ float block_max256(float v, float* red) {
  const int j = threadIdx.x;
  red[j] = v;
  __syncthreads();
#pragma unroll
  for (int d = 128; d >= 1; d >>= 1) {
    if (j < d) red[j] = fmaxf(red[j], red[j + d]);
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// per hop block k of row b (samples [k hop, min((k + 1) hop, n))): the maximum of the signed
// samples (a NaN counts as +inf: np.max would return it, and it is not below any threshold) and
// of their magnitudes. grid (nblk, B); blocks at or past the row's end write nothing and are never read.
__global__ void __launch_bounds__(256)
    wt_hop_max_kernel(const float* __restrict__ wav, RowInts ns, int L_max, int hop, int nblk,
                      float* __restrict__ smax, float* __restrict__ amax) {
  __shared__ float red[256];
  const int b = blockIdx.y, k = blockIdx.x, n = ns.v[b];
  const long lo = (long)k * hop;
  if (lo >= n) return;
  const int cnt = (int)min((long)hop, n - lo);
  const float* src = wav + (size_t)b * L_max + lo;
  float s = -INFINITY, a = 0.f;
  for (int p = threadIdx.x; p < cnt; p += 256) {
    const float v = src[p];
    s = fmaxf(s, v != v ? INFINITY : v);
    a = fmaxf(a, fabsf(v));
  }
  s = block_max256(s, red);
  a = block_max256(a, red);
  if (threadIdx.x == 0) {
    smax[(size_t)b * nblk + k] = s;
    amax[(size_t)b * nblk + k] = a;
  }
}

// AudioProcessor.find_endpoint per row: candidate i (x = i hop, 1 <= i <= nc) hits when the maximum
// of hop blocks i .. i + q - 1 and of the rem samples after them is below thr; the first hit gives
// (i + 1) hop, none gives n. One workgroup per row.
__global__ void __launch_bounds__(256)
    wt_endpoint_kernel(const float* __restrict__ wav, RowInts ns, int L_max, int hop, int window, int nblk,
                       const float* __restrict__ smax, double thr, int* __restrict__ ends) {
  __shared__ int first[256];
  const int b = blockIdx.x, j = threadIdx.x, n = ns.v[b];
  const int q = window / hop, rem = window - q * hop;
  // x in range(hop, n - window, hop)
  const int nc = n - window > hop ? (n - window - 1) / hop : 0;
  const float* row = wav + (size_t)b * L_max;
  const float* bm = smax + (size_t)b * nblk;
  int hit = nc + 1;
  for (int i = 1 + j; i <= nc && hit > nc; i += 256) {
    float m = -INFINITY;
    for (int k = 0; k < q; ++k) m = fmaxf(m, bm[i + k]);
    const float* tail = row + (long)(i + q) * hop;
    for (int p = 0; p < rem; ++p) {
      const float v = tail[p];
      m = fmaxf(m, v != v ? INFINITY : v);
    }
    if ((double)m < thr) hit = i;
  }
  first[j] = hit;
  __syncthreads();
#pragma unroll
  for (int d = 128; d >= 1; d >>= 1) {
    if (j < d) first[j] = min(first[j], first[j + d]);
    __syncthreads();
  }
  if (j == 0) ends[b] = first[0] <= nc ? (first[0] + 1) * hop : n;
}

// offsets of the rows in the joined signal (a prefix over at most 64 rows), its length, and
// save_wav's factor from the peak of |x| over the kept samples: an endpoint is a multiple of hop or
// the row's end, so the hop blocks below it cover exactly the kept samples. One workgroup.
__global__ void __launch_bounds__(256)
    wt_plan_kernel(const int* __restrict__ ends, int B, int gap, int hop, int nblk, const float* __restrict__ amax,
                   int* __restrict__ offs, float* __restrict__ factor, int* __restrict__ total) {
  __shared__ float red[256];
  float a = 0.f;
  for (int b = 0; b < B; ++b) {
    const int kend = (ends[b] + hop - 1) / hop;
    for (int k = threadIdx.x; k < kend; k += 256) a = fmaxf(a, amax[(size_t)b * nblk + k]);
  }
  const float peak = block_max256(a, red);
  if (threadIdx.x == 0) {
    int off = 0;
    for (int b = 0; b < B; ++b) {
      offs[b] = off;
      off += ends[b] + gap;
    }
    *total = off;
    // numpy: 32767 / float32 peak is the correctly rounded float32 quotient; the double quotient of
    // two floats rounds to it
    *factor = peak > 0.01f ? (float)(32767.0 / (double)peak) : 3276700.f;
  }
}

// row b's kept samples times the factor (a float32 product), truncated toward zero, then gap zeros
__global__ void __launch_bounds__(256)
    wt_write_kernel(const float* __restrict__ wav, int L_max, int gap, const int* __restrict__ ends,
                    const int* __restrict__ offs, const float* __restrict__ factor, int16_t* __restrict__ pcm) {
  const int b = blockIdx.y, end = ends[b];
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)end + gap) return;
  int16_t v = 0;
  if (p < end) v = (int16_t)(int)(wav[(size_t)b * L_max + p] * *factor);
  pcm[offs[b] + p] = v;
}

}  // namespace

void launch_spec_to_mag(const float* x, const RowInts& lens, int B, int M_max, int F, const float* scale,
                        const float* offset, float clip_lo, float clip_hi, int use_clip, float spec_gain, float power,
                        float* S, hipStream_t s) {
  const long per_row = (long)M_max * F;
  spec_to_mag_kernel<<<dim3((unsigned)((per_row + 255) / 256), B), 256, 0, s>>>(
      x, lens, M_max, F, scale, offset, clip_lo, clip_hi, use_clip, spec_gain, power, S);
  HIP_OK(hipGetLastError());
}

void launch_deemphasis(const float* in, float* out, const RowInts& ns, int B, int L_max, const DeemphTable& tab,
                       hipStream_t s) {
  deemphasis_kernel<<<B, DE_T, 0, s>>>(in, out, ns, L_max, tab);
  HIP_OK(hipGetLastError());
}

void launch_wav_finish(const float* wav, const RowInts& ns, int B, int L_max, int window, int hop, double thr, int gap,
                       float* smax, float* amax, int nblk, int* offs, float* factor, int16_t* pcm, int* ends,
                       int* total, hipStream_t s) {
  wt_hop_max_kernel<<<dim3(nblk, B), 256, 0, s>>>(wav, ns, L_max, hop, nblk, smax, amax);
  HIP_OK(hipGetLastError());
  wt_endpoint_kernel<<<B, 256, 0, s>>>(wav, ns, L_max, hop, window, nblk, smax, thr, ends);
  HIP_OK(hipGetLastError());
  wt_plan_kernel<<<1, 256, 0, s>>>(ends, B, gap, hop, nblk, amax, offs, factor, total);
  HIP_OK(hipGetLastError());
  const long span = (long)L_max + gap;
  wt_write_kernel<<<dim3((unsigned)((span + 255) / 256), B), 256, 0, s>>>(wav, L_max, gap, ends, offs, factor, pcm);
  HIP_OK(hipGetLastError());
}
