// Plumbing shared by the split-f16 tile kernels (conv_x3, resblock_x3, resstack_x3, the PWGAN
// layer): the buffer resource of their raw buffer loads, the weight (A-operand) fragment fetch, and
// the persistent kernels' table from tile index to (utterance, first position), with the host's
// tile count. Staging, weight rings and epilogues differ per kernel on purpose and stay there.
#pragma once
#include "common.h"
#include "split16.h"

// buffer resource over everything from p on (no bound to clip at): for raw buffer loads whose
// 32-bit offsets the kernel keeps inside the tensor itself
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x3_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

// one lane's A fragment of a pack_split_a block (64 lanes x [hi 8 | lo 8], 2048 bytes): the lane's
// 32 bytes at wlo = lane * 32 are the VGPR offset (computed once by the caller), the block's byte
// offset `blk` (wave-uniform) the SGPR one
__device__ __forceinline__ void x3_load_a(h8 (&r)[2], __amdgpu_buffer_rsrc_t w, int wlo, int blk) {
  r[0] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(w, wlo, blk, 0));
  r[1] = __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(w, wlo + 16, blk, 0));
}

// Tile of a persistent loop: utterance b, positions [q0, q0 + TQ) of its L = (lens + len_add) * mul
struct X3Tile {
  int b, q0, L;
};
// tile index -> (utterance, first position): per-utterance tile offsets as an exclusive scan over
// the <= 64 lengths, once per workgroup, in LDS (tcum[65], tlen[64]). Wave 0 calls this with L =
// lane's utterance length (0 for lanes past the batch); the caller's workgroup barrier follows
// before any x3_tile_of.
template <int TQ>
__device__ __forceinline__ void x3_tile_scan(int* tcum, int* tlen, int lane, int L) {
  const int n = (L + TQ - 1) / TQ;
  int v = n;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(v, o, 64);
    if (lane >= o) v += y;
  }
  tcum[lane] = v - n;
  tlen[lane] = L;
  if (lane == 63) tcum[64] = v;
}
// a lookup is one LDS read per lane and a ballot; the result is wave-uniform (SGPRs)
template <int TQ>
__device__ __forceinline__ X3Tile x3_tile_of(const int* tcum, const int* tlen, int B, int lane, int i) {
  const bool hit = lane < B && tcum[lane] <= i && i < tcum[lane + 1];
  const unsigned long long m = __ballot(hit);
  const int b = __builtin_amdgcn_readfirstlane(m ? __ffsll((long long)m) - 1 : 0);
  X3Tile r;
  r.b = b;
  r.q0 = __builtin_amdgcn_readfirstlane((i - tcum[b]) * TQ);
  r.L = __builtin_amdgcn_readfirstlane(tlen[b]);
  return r;
}

// host: the tile count x3_tile_scan arrives at, sum over utterances of ceil((lens + len_add) * mul / TQ)
inline long x3_tile_count(const int* h_lens, int B, int len_add, int mul, int TQ, const char* who) {
  long ntiles = 0;
  for (int b = 0; b < B; ++b) ntiles += ((long)(h_lens[b] + len_add) * mul + TQ - 1) / TQ;
  TTS_CHECK(ntiles < (1L << 30), std::string(who) + ": too many tiles");
  return ntiles;
}
