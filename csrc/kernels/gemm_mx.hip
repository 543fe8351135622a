// trtlab_amd — MX-format GEMM on the CDNA4 scaled MFMA
// (mfma_scale_f32_16x16x128_f8f6f4): OCP Microscaling fp8-e4m3 or fp4-e2m1
// elements with one e8m0 shared scale per 32-element K-block. This
// instruction is gfx950's headline-throughput path (K=128 per issue, 4x
// the K-depth of the 16x16x32 fp8 MFMA) and has no equivalent in the CUDA
// reference.
//
// C[M,N] = sum_k (a[m,k] * 2^(sa[m,k/32]-127)) * (b[n,k] * 2^(sb[n,k/32]-127))
//
// B is prepacked transposed [N][K] like every other "bt" GEMM here; scales
// are row-major u8 [M][K/32] / [N][K/32]. Rows stage through the shared
// 128-byte-row XOR-swizzled LDS tiles. Everything that depends on the
// element format lives in the MxFp8 / MxFp4 policies below; the kernels,
// quantizers and probes are written once over a policy F. A further format
// of the same instruction (fp6) is one more policy.
#include <string>

#include "gemm_common.h"
#include "mx_common.h"

namespace trtlab {

typedef __attribute__((ext_vector_type(8))) int i32x8v;

__device__ __forceinline__ void glds4(const void* gsrc, uint32_t lds_byte) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) uint32_t*)gsrc,
      (__attribute__((address_space(3))) uint32_t*)(uintptr_t)lds_byte, 4, 0,
      0);
}

// ------------------------------------------------------------ format policy
// Operand layout of the scaled MFMA, pinned down empirically with
// tools/probe_mx.py (fp8; experiment E1 = 48 is the split-half signature)
// and tools/probe_mx4.py (fp4). One instruction consumes a 128-k window of
// a row; lane l = 16*g + r carries row r, and with opsel 0 lane-group g's
// scale byte applies to MX block g of the window, k [g*32, g*32+32).
//   fp8: the lane's 32-byte register holds k [g*16, +16) in its low half
//        and k [64+g*16, +16) in its high half.
//   fp4: the lane's low 16 bytes hold k [g*32, +32) contiguously (two
//        elements per byte, low nibble first); the upper 16 bytes are zero.
// A 128-byte LDS row therefore holds kWindows windows: one for fp8, two for
// fp4. A policy states this as chunk(g, w, c): the byte offset in the row of
// the c-th 16-byte chunk of lane-group g's register for window w.
template <typename F>
struct MxFormat {
  // logical k per staged LDS tile; also the K multiple the launcher enforces
  static __host__ __device__ constexpr int tile_k() { return 128 * F::kWindows; }

  // Fragment for window w of swizzled LDS tile row `row`.
  static __device__ __forceinline__ i32x8v frag(const char* lds, int row,
                                                int w, int lane) {
    i32x8v f = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < F::kChunks; ++c) {
      uint32_t cb = F::chunk((uint32_t)(lane >> 4), (uint32_t)w, c);
      i32x4 v = *(const i32x4*)(lds + (uint32_t)row * 128 +
                                (cb ^ (((uint32_t)row & 7) << 4)));
      f[4 * c] = v[0]; f[4 * c + 1] = v[1];
      f[4 * c + 2] = v[2]; f[4 * c + 3] = v[3];
    }
    return f;
  }

  // The same map straight from unswizzled global memory: window 0 of row
  // `row` of a [rows][128 k] matrix (the layout probes).
  static __device__ __forceinline__ i32x8v frag_global(const uint8_t* p,
                                                       int row, int lane) {
    i32x8v f = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < F::kChunks; ++c) {
      i32x4 v = *(const i32x4*)(p + row * F::row_bytes(128) +
                                F::chunk((uint32_t)(lane >> 4), 0, c));
      f[4 * c] = v[0]; f[4 * c + 1] = v[1];
      f[4 * c + 2] = v[2]; f[4 * c + 3] = v[3];
    }
    return f;
  }

  static __device__ __forceinline__ f32x4 mfma(i32x8v a, i32x8v b, f32x4 c,
                                               int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
        a, b, c, F::kFmt /*cbsz*/, F::kFmt /*blgp*/, 0, sa, 0, sb);
  }
};

struct MxFp8 : MxFormat<MxFp8> {
  static constexpr const char* kName = "mxfp8";
  static constexpr int kFmt = 0;      // cbsz/blgp: e4m3
  static constexpr int kWindows = 1;  // 128-k windows per 128-byte LDS row
  static constexpr int kChunks = 2;
  static constexpr int kEmax = 8;     // 448 = 1.75 * 2^8
  static __host__ __device__ constexpr int row_bytes(int K) { return K; }
  static __device__ __forceinline__ uint32_t chunk(uint32_t g, uint32_t,
                                                   int c) {
    return c * 64 + g * 16;
  }
  // N scaled elements -> row_bytes(N) code bytes
  template <int N>
  static __device__ __forceinline__ void encode(const float* v, float inv,
                                                uint8_t* out) {
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = mx_encode_e4m3(v[j] * inv);
  }
};

struct MxFp4 : MxFormat<MxFp4> {
  static constexpr const char* kName = "mxfp4";
  static constexpr int kFmt = 4;  // cbsz/blgp: e2m1
  static constexpr int kWindows = 2;
  static constexpr int kChunks = 1;
  static constexpr int kEmax = 2;  // 6 = 1.5 * 2^2
  static __host__ __device__ constexpr int row_bytes(int K) { return K >> 1; }
  static __device__ __forceinline__ uint32_t chunk(uint32_t g, uint32_t w,
                                                   int) {
    return w * 64 + g * 16;
  }
  // low nibble = even element
  template <int N>
  static __device__ __forceinline__ void encode(const float* v, float inv,
                                                uint8_t* out) {
#pragma unroll
    for (int j = 0; j < N / 2; ++j)
      out[j] = (uint8_t)(mx_encode_e2m1(v[2 * j] * inv) |
                         (mx_encode_e2m1(v[2 * j + 1] * inv) << 4));
  }
};

// ----------------------------------------------------------------- epilogue
// Epilogue for accumulators in the row-run mapping (activation fragment
// first): col = lane&15 of fragment column f, rows 4*(lane>>4) + r of
// fragment row i. Scalar stores, predicated on both M and N.
template <Epi E, typename OT, int MF, int NF>
__device__ __forceinline__ void store_mx_tile(
    f32x4 (&acc)[MF][NF], OT* __restrict__ C, int row0, int col0, int M,
    int N, const float* __restrict__ scale, const float* __restrict__ bias,
    int lane) {
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int col = col0 + f * 16 + (lane & 15);
      if (col >= N) continue;
      float sc = 1.0f, bi = 0.0f;
      if constexpr (kEpiHasScale<E>) sc = scale[col];
      if constexpr (E != Epi::kNone) bi = bias[col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = row0 + i * 16 + ((lane >> 4) << 2) + r;
        if (row >= M) continue;
        C[(int64_t)row * N + col] =
            store_cast<OT>(apply_epi<E>(acc[i][f][r], sc, bi, 0.0f));
      }
    }
}

// ------------------------------------------------------------------ kernels
// BM = BN = 128, one workgroup = 4 waves; wave (wr, wc) = (w>>1, w&1)
// computes the [wr*64, +64) x [wc*64, +64) quadrant: per window 4x4
// fragment pairs, 16 scaled MFMAs from 8 fragment reads. 3 slots x (A tile
// + B tile + scale slabs): the counted-vmcnt pipeline keeps 2 tiles'
// staging in flight behind the MFMAs.
template <typename F, typename OT, Epi E>
__global__ __launch_bounds__(256) void gemm_mx_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
    const uint8_t* __restrict__ Sa, const uint8_t* __restrict__ Sb,
    OT* __restrict__ C, const float* __restrict__ scale,
    const float* __restrict__ bias, int M, int N, int K, int tiles_n) {
  constexpr int W = F::kWindows;
  constexpr int kABytes = 128 * 128;
  // scale slabs: 128 rows x u32 (4 block scales) = 512 B per window per
  // side, A's windows first
  constexpr int kSlot = 2 * kABytes + 2 * W * 512;
  __shared__ __attribute__((aligned(16))) char smem[3 * kSlot];

  uint32_t bid = xcd_swizzle(blockIdx.x, gridDim.x);
  int m0 = (int)(bid / tiles_n) * 128;
  int n0 = (int)(bid % tiles_n) * 128;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int pitch = F::row_bytes(K);
  const int ktiles = K >> __builtin_ctz(F::tile_k());
  const int kblocks = K >> 5;  // 32-elem MX blocks per row

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[i][f] = {0.f, 0.f, 0.f, 0.f};

  auto stage = [&](int t, int slot) {
    char* base = smem + slot * kSlot;
    stage_tile<uint8_t, 128>(A + (int64_t)m0 * pitch + t * 128, pitch, m0, M,
                             (uint32_t)(uintptr_t)base, tid);
    stage_tile<uint8_t, 128>(B + (int64_t)n0 * pitch + t * 128, pitch, n0, N,
                             (uint32_t)(uintptr_t)(base + kABytes), tid);
    // Scales go through glds too, so the per-thread glds count stays
    // uniform: 8 data + W scale loads (scattered 1-byte global loads per
    // MFMA were the v1 bottleneck: 402 -> 747 TF when staged).
    // global_load_lds packs lanes at consecutive 4-B slots from a uniform
    // base, so each 512-B slab gets its own call with a lane-natural
    // destination: threads 0-127 fetch A's rows, 128-255 B's.
    uint32_t sbase = (uint32_t)(uintptr_t)(base + 2 * kABytes);
    if (tid < 128) {
      int ar = m0 + tid;
      if (ar >= M) ar = M - 1;
#pragma unroll
      for (int w = 0; w < W; ++w)
        glds4(Sa + (int64_t)ar * kblocks + (t * W + w) * 4,
              sbase + w * 512 + (uint32_t)tid * 4);
    } else {
      int br = n0 + tid - 128;
      if (br >= N) br = N - 1;
#pragma unroll
      for (int w = 0; w < W; ++w)
        glds4(Sb + (int64_t)br * kblocks + (t * W + w) * 4,
              sbase + (W + w) * 512 + (uint32_t)(tid - 128) * 4);
    }
  };

  stage(0, 0);
  if (ktiles > 1) stage(1, 1);
  for (int t = 0; t < ktiles; ++t) {
    int ahead = ktiles - 1 - t;
    if (ahead > 1) ahead = 1;
    wait_tiles_inflight<8 + W>(ahead);
    __builtin_amdgcn_s_barrier();
    if (t + 2 < ktiles) stage(t + 2, (t + 2) % 3);
    const char* As = smem + (t % 3) * kSlot;
    const char* Bs = As + kABytes;
    const uint8_t* sas = (const uint8_t*)(As + 2 * kABytes);
    const uint8_t* sbs = sas + W * 512;
    int g = lane >> 4;  // lane's MX block within the window (scale byte)
#pragma unroll
    for (int w = 0; w < W; ++w) {
      i32x8v af[4];
      int sa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int arow = wr * 64 + i * 16 + (lane & 15);
        af[i] = F::frag(As, arow, w, lane);
        sa[i] = sas[w * 512 + arow * 4 + g];
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        int brow = wc * 64 + f * 16 + (lane & 15);
        i32x8v bf = F::frag(Bs, brow, w, lane);
        int sb = sbs[w * 512 + brow * 4 + g];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i][f] = F::mfma(af[i], bf, acc[i][f], sa[i], sb);
      }
    }
  }

  store_mx_tile<E>(acc, C, m0 + wr * 64, n0 + wc * 64, M, N, scale, bias,
                   lane);
}

// 64x64 small-tile variant for grid-starved serving shapes (e.g. BERT b8:
// M=1024 gives the 128-tile kernel only 48 workgroups on 256 CUs). 4 waves
// x [16 rows x 64 cols]; 2-phase staging with plain-load scale arrays
// (latency-bound shapes; the deep pipeline is the 128-tile's job).
template <typename F, typename OT, Epi E>
__global__ __launch_bounds__(256) void gemm_mx_small_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
    const uint8_t* __restrict__ Sa, const uint8_t* __restrict__ Sb,
    OT* __restrict__ C, const float* __restrict__ scale,
    const float* __restrict__ bias, int M, int N, int K, int tiles_n) {
  constexpr int W = F::kWindows;
  constexpr int kABytes = 64 * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * kABytes];
  // one u32 (4 block scales) per row per window
  __shared__ __attribute__((aligned(4))) uint32_t sa_s[2][W * 64],
      sb_s[2][W * 64];

  uint32_t bid = xcd_swizzle(blockIdx.x, gridDim.x);
  int m0 = (int)(bid / tiles_n) * 64;
  int n0 = (int)(bid % tiles_n) * 64;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int pitch = F::row_bytes(K);
  const int ktiles = K >> __builtin_ctz(F::tile_k());
  const int kblocks = K >> 5;

  f32x4 acc[1][4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc[0][f] = {0.f, 0.f, 0.f, 0.f};

  auto stage = [&](int t, int slot) {
    char* base = smem + slot * 2 * kABytes;
    stage_tile<uint8_t, 64>(A + (int64_t)m0 * pitch + t * 128, pitch, m0, M,
                            (uint32_t)(uintptr_t)base, tid);
    stage_tile<uint8_t, 64>(B + (int64_t)n0 * pitch + t * 128, pitch, n0, N,
                            (uint32_t)(uintptr_t)(base + kABytes), tid);
    if (tid < 64) {
      int ar = m0 + tid;
      if (ar >= M) ar = M - 1;
#pragma unroll
      for (int w = 0; w < W; ++w)
        sa_s[slot][w * 64 + tid] = *(const uint32_t*)(
            Sa + (int64_t)ar * kblocks + (t * W + w) * 4);
    } else if (tid < 128) {
      int br = n0 + tid - 64;
      if (br >= N) br = N - 1;
#pragma unroll
      for (int w = 0; w < W; ++w)
        sb_s[slot][w * 64 + tid - 64] = *(const uint32_t*)(
            Sb + (int64_t)br * kblocks + (t * W + w) * 4);
    }
  };

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < ktiles; ++t) {
    if (t + 1 < ktiles) stage(t + 1, cur ^ 1);
    const char* As = smem + cur * 2 * kABytes;
    const char* Bs = As + kABytes;
    int g = lane >> 4;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      int arow = wave * 16 + (lane & 15);
      i32x8v af = F::frag(As, arow, w, lane);
      int sa = ((const uint8_t*)&sa_s[cur][w * 64 + arow])[g];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        int brow = f * 16 + (lane & 15);
        i32x8v bf = F::frag(Bs, brow, w, lane);
        int sb = ((const uint8_t*)&sb_s[cur][w * 64 + brow])[g];
        acc[0][f] = F::mfma(af, bf, acc[0][f], sa, sb);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }

  store_mx_tile<E>(acc, C, m0 + wave * 16, n0, M, N, scale, bias, lane);
}

// ----------------------------------------------------------------- launchers
template <typename F, int TILE, typename OT, Epi E>
constexpr auto mx_kernel() {
  if constexpr (TILE == 128)
    return &gemm_mx_kernel<F, OT, E>;
  else
    return &gemm_mx_small_kernel<F, OT, E>;
}

template <typename F, int TILE>
void launch_gemm_mx_tile(const void* A, const void* B, const void* Sa,
                         const void* Sb, void* C, int M, int N, int K,
                         hipStream_t stream, int out_dtype, int epi,
                         const float* scale, const float* bias) {
  int tiles_n = (int)cdiv(N, TILE);
  dim3 grid((unsigned)(cdiv(M, TILE) * tiles_n));
  auto go = [&](auto kernel, auto* c, const float* sc, const float* bi) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, (const uint8_t*)A,
                       (const uint8_t*)B, (const uint8_t*)Sa,
                       (const uint8_t*)Sb, c, sc, bi, M, N, K, tiles_n);
  };
  if (out_dtype == 2) {
    go(mx_kernel<F, TILE, float, Epi::kNone>(), (float*)C, nullptr, nullptr);
    return;
  }
  epi_dispatch(epi, [&](auto e) {
    go(mx_kernel<F, TILE, _Float16, decltype(e)::value>(), (_Float16*)C,
       scale, bias);
  });
}

// out_dtype: 0 = fp16 (engine path, with epilogue), 2 = fp32 raw C.
template <typename F>
void launch_gemm_mx(const void* A, const void* B, const void* Sa,
                    const void* Sb, void* C, int M, int N, int K,
                    hipStream_t stream, int out_dtype, int epi,
                    const float* scale, const float* bias) {
  if (K % F::tile_k() != 0)
    throw std::runtime_error(std::string("gemm_") + F::kName +
                             ": K must be a multiple of " +
                             std::to_string(F::tile_k()));
  // grid-starved: 4x the workgroups at 64x64
  if ((long)cdiv(M, 128) * cdiv(N, 128) < 64)
    launch_gemm_mx_tile<F, 64>(A, B, Sa, Sb, C, M, N, K, stream, out_dtype,
                               epi, scale, bias);
  else
    launch_gemm_mx_tile<F, 128>(A, B, Sa, Sb, C, M, N, K, stream, out_dtype,
                                epi, scale, bias);
}

void launch_gemm_mxfp8(const void* A, const void* B, const void* Sa,
                       const void* Sb, void* C, int M, int N, int K,
                       hipStream_t stream, int out_dtype, int epi,
                       const float* scale, const float* bias) {
  launch_gemm_mx<MxFp8>(A, B, Sa, Sb, C, M, N, K, stream, out_dtype, epi,
                        scale, bias);
}

void launch_gemm_mxfp4(const void* A, const void* B, const void* Sa,
                       const void* Sb, void* C, int M, int N, int K,
                       hipStream_t stream, int out_dtype, int epi,
                       const float* scale, const float* bias) {
  launch_gemm_mx<MxFp4>(A, B, Sa, Sb, C, M, N, K, stream, out_dtype, epi,
                        scale, bias);
}

// ---------------------------------------------------------------- quantizers
// Row-wise dynamic MX quantization of fp16 activations: x [M, K] -> codes
// [M, row_bytes(K)] + e8m0 scales [M, K/32]. One thread per 32-element
// block: block amax -> shared exponent (mx_common.h) -> F::encode.
template <typename F>
__global__ __launch_bounds__(256) void quantize_mx_kernel(
    const _Float16* __restrict__ x, uint8_t* __restrict__ codes,
    uint8_t* __restrict__ scales, int64_t nblocks) {
  int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const _Float16* src = x + b * 32;
  float v[32];
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    half8v h = *(const half8v*)(src + c * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (float)((const _Float16*)&h)[j];
      v[c * 8 + j] = f;
      amax = fmaxf(amax, fabsf(f));
    }
  }
  int e = mx_block_exponent(amax, F::kEmax);
  scales[b] = (uint8_t)(e + 127);
  constexpr int kBytes = F::row_bytes(32);
  uint8_t out[kBytes];
  F::template encode<32>(v, exp2f((float)-e), out);
#pragma unroll
  for (int c = 0; c < kBytes; c += 16)
    *(f32x4*)(codes + b * kBytes + c) = *(const f32x4*)(out + c);
}

template <typename F>
void launch_quantize_mx(const void* x, void* codes, void* scales, int64_t m,
                        int64_t k, hipStream_t stream) {
  if (k % 32 != 0)
    throw std::runtime_error(std::string("quantize_") + F::kName +
                             ": K must be a multiple of 32");
  int64_t nblocks = m * (k / 32);
  int64_t blocks = (nblocks + 255) / 256;
  hipLaunchKernelGGL(quantize_mx_kernel<F>, dim3((unsigned)blocks), dim3(256),
                     0, stream, (const _Float16*)x, (uint8_t*)codes,
                     (uint8_t*)scales, nblocks);
}

void launch_quantize_mxfp8(const void* x, void* codes, void* scales,
                           int64_t m, int64_t k, hipStream_t stream) {
  launch_quantize_mx<MxFp8>(x, codes, scales, m, k, stream);
}

void launch_quantize_mxfp4(const void* x, void* codes, void* scales,
                           int64_t m, int64_t k, hipStream_t stream) {
  launch_quantize_mx<MxFp4>(x, codes, scales, m, k, stream);
}

// -------------------------------------------------------------------- probes
// Layout probe: one wave, direct global loads, no LDS. M = N = 16, one
// 128-k window; A and B are [16][row_bytes(128)], scales [16][4]. Dumps
// the accumulators for host-side hypothesis falsification
// (tools/probe_mx.py, tools/probe_mx4.py).
template <typename F>
__global__ __launch_bounds__(64) void mx_probe_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
    const uint8_t* __restrict__ Sa, const uint8_t* __restrict__ Sb,
    float* __restrict__ D) {
  int lane = threadIdx.x;
  int row = lane & 15, g = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = F::mfma(F::frag_global(A, row, lane), F::frag_global(B, row, lane),
                acc, Sa[row * 4 + g], Sb[row * 4 + g]);
#pragma unroll
  for (int r = 0; r < 4; ++r) D[((g << 2) + r) * 16 + row] = acc[r];
}

void launch_mx_probe(const void* A, const void* B, const void* Sa,
                     const void* Sb, void* D, hipStream_t stream) {
  hipLaunchKernelGGL(mx_probe_kernel<MxFp8>, dim3(1), dim3(64), 0, stream,
                     (const uint8_t*)A, (const uint8_t*)B, (const uint8_t*)Sa,
                     (const uint8_t*)Sb, (float*)D);
}

void launch_mx4_probe(const void* A, const void* B, const void* Sa,
                      const void* Sb, void* D, hipStream_t stream) {
  hipLaunchKernelGGL(mx_probe_kernel<MxFp4>, dim3(1), dim3(64), 0, stream,
                     (const uint8_t*)A, (const uint8_t*)B, (const uint8_t*)Sa,
                     (const uint8_t*)Sb, (float*)D);
}

// Stage 64 fp8 rows through the swizzled LDS tile exactly like the GEMM
// kernels, then dump the four waves' assembled fragments so the host can
// verify the LDS round trip byte-for-byte (tools/dbg_mx.py).
__global__ __launch_bounds__(256) void mx_frag_dump_kernel(
    const uint8_t* __restrict__ A, uint8_t* __restrict__ out, int K) {
  __shared__ __attribute__((aligned(16))) char smem[64 * 128];
  const int tid = threadIdx.x;
  stage_tile<uint8_t, 64>(A, K, 0, 64, (uint32_t)(uintptr_t)smem, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int lane = tid & 63, wave = tid >> 6;
  *(i32x8v*)(out + (wave * 64 + lane) * 32) =
      MxFp8::frag(smem, wave * 16 + (lane & 15), 0, lane);
}

void launch_mx_frag_dump(const void* A, void* out, int K, hipStream_t s) {
  hipLaunchKernelGGL(mx_frag_dump_kernel, dim3(1), dim3(256), 0, s,
                     (const uint8_t*)A, (uint8_t*)out, K);
}

}  // namespace trtlab
