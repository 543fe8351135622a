// trtlab_amd — pieces shared by the row-sampling kernels (gfx950).
// elementwise.hip (argmax_rows / gumbel_argmax_rows) and sampling.hip
// (topk_topp_sample_rows) draw the SAME Gumbel noise and reduce with the
// SAME lowest-index tie rule; both include this header so the two cannot
// drift: a row with no filter active must sample the identical token from
// either kernel.
#pragma once

#include "../common.h"

namespace trtlab {

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// Per-row noise key: (seed[row], device pos[row], row). Null arrays read 0.
__device__ __forceinline__ uint64_t gumbel_row_key(const int* seeds,
                                                   const int* pos, int row) {
  return ((uint64_t)(uint32_t)(seeds ? seeds[row] : 0) << 32) ^
         (uint64_t)(uint32_t)(pos ? pos[row] : 0) ^
         ((uint64_t)(uint32_t)row << 20);
}

// v/T + G_c, G_c = -log(-log(u_c)), u_c from splitmix64(key ^ c).
__device__ __forceinline__ float gumbel_perturb(float v, float invT,
                                                uint64_t key, int c) {
  uint64_t h = splitmix64(key ^ (uint64_t)c);
  // u in (0, 1): top 24 bits, never exactly 0
  float u = ((float)(uint32_t)(h >> 40) + 0.5f) * (1.0f / 16777216.f);
  return v * invT - __logf(-__logf(u));
}

// Running argmax, ties to the LOWEST index (numpy argmax). Order-free: the
// winner does not depend on the order candidates are offered in.
__device__ __forceinline__ void argmax_take(float v, int c, float& best,
                                            int& bi) {
  if (v > best || (v == best && c < bi)) {
    best = v;
    bi = c;
  }
}

// 256-thread block argmax over per-thread (best, bi). wb/wi are 4-entry
// __shared__ arrays of the caller; on return thread 0 holds the block
// winner in wb[0]/wi[0] (other threads must __syncthreads() before
// reading them).
__device__ __forceinline__ void block_argmax_256(float best, int bi,
                                                 float* wb, int* wi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    float ob = __shfl_xor(best, off, 64);
    int oi = __shfl_xor(bi, off, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) {
    wb[wave] = best;
    wi[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (wb[w] > wb[0] || (wb[w] == wb[0] && wi[w] < wi[0])) {
        wb[0] = wb[w];
        wi[0] = wi[w];
      }
  }
}

}  // namespace trtlab
