// trtlab_amd — implicit-GEMM conv2d (NHWC, fp16/bf16) for gfx950 with fused
// BN(scale,bias) + ReLU + optional residual-add epilogue.
//
// out[n,oh,ow,co] = epi( sum_{kh,kw,ci} in[n,ih,iw,ci] * w[co, kh,kw,ci] )
//     ih = oh*sh - ph + kh, iw = ow*sw - pw + kw
//
// GEMM view: A[M=N*OH*OW][K=KH*KW*C] is generated on the fly — each
// global_load_lds lane computes its own source address ((row,k) -> NHWC
// address) and out-of-image taps read a 16-byte zero page instead
// (glds has per-lane SOURCE addressing, so implicit im2col costs no
// separate pass and padding costs no branches in the MFMA loop).
// Weights are prepacked [Cout][KH*KW*C] ("bt" layout) at engine build time.
// Requires C % 8 == 0 (host pads input channels, e.g. RGB 3 -> 8) and the
// weight K padded to % 64 (zero filled; A taps >= Kreal read the zero page).
//
// Tile size BMxBN is picked per shape (gemm_common.h pick_tile) so the small
// deep-layer shapes (ResNet stage 4/5 at batch 8) still fill 256 CUs.
// Replaces TensorRT's internal conv kernels.
#include "gemm_common.h"

namespace trtlab {

struct ConvParams {
  int Nb, H, W, C;        // input NHWC (C already padded to %8)
  int Cout, KH, KW;       // weights [Cout][K]
  int OH, OW;             // output spatial
  int sh, sw, ph, pw;     // stride / padding
  int M;                  // Nb*OH*OW
  int K;                  // KH*KW*C rounded up to the K-tile (64/128 elems)
  int Kreal;              // KH*KW*C
  float res_scale;        // int8 residual dequant ratio (s_res/s_out)
  FastDiv d_ohw, d_ow, d_c, d_kw;
};

// Stage a ROWS x 64-elem A-tile of the implicit im2col matrix.
template <typename T, int ROWS>
__device__ __forceinline__ void stage_conv_a(
    const T* __restrict__ in, const T* __restrict__ zero_page,
    const ConvParams p, int m0, int k0, uint32_t lds_base, int tid) {
#pragma unroll
  for (int c = 0; c < ROWS / 32; ++c) {
    uint32_t pbyte = c * 4096 + tid * 16;
    uint32_t row = pbyte >> 7;
    uint32_t kb = (pbyte & 127) ^ ((row & 7) << 4);  // source-side swizzle
    int m = m0 + (int)row;
    if (m >= p.M) m = p.M - 1;
    uint32_t n = fdiv((uint32_t)m, p.d_ohw);
    uint32_t rem = (uint32_t)m - n * (uint32_t)(p.OH * p.OW);
    uint32_t oh = fdiv(rem, p.d_ow);
    uint32_t ow = rem - oh * (uint32_t)p.OW;
    int k = k0 + (int)(kb / sizeof(T));  // element index along K
    const char* src;
    if (k >= p.Kreal) {
      src = (const char*)zero_page;
    } else {
      uint32_t pix = fdiv((uint32_t)k, p.d_c);
      uint32_t ci = (uint32_t)k - pix * (uint32_t)p.C;
      uint32_t kh = fdiv(pix, p.d_kw);
      uint32_t kw = pix - kh * (uint32_t)p.KW;
      int ih = (int)oh * p.sh - p.ph + (int)kh;
      int iw = (int)ow * p.sw - p.pw + (int)kw;
      if ((uint32_t)ih < (uint32_t)p.H && (uint32_t)iw < (uint32_t)p.W) {
        int64_t off = (((int64_t)n * p.H + ih) * p.W + iw) * p.C + ci;
        src = (const char*)(in + off);
      } else {
        src = (const char*)zero_page;
      }
    }
    glds16(src, lds_base + pbyte);
  }
}

void launch_splitk_reduce(int dtype, const float* scratch, void* C,
                          const float* scale, const float* bias,
                          const void* residual, float res_scale, int M, int N,
                          int64_t ldc, int tiles_m, int tiles_n, int splitk,
                          int bm, int bn, int epi, hipStream_t stream);

template <typename T, Epi E, int BM, int BN, bool SPLIT, int NBUF>
__global__ __launch_bounds__(256) void conv_igemm_kernel(
    const T* __restrict__ in, const T* __restrict__ Wt, T* __restrict__ out,
    const float* __restrict__ scale, const float* __restrict__ bias,
    const T* __restrict__ residual, const T* __restrict__ zero_page,
    const ConvParams p, int tiles_n, float* __restrict__ scratch, int splitk,
    int ktper) {
  constexpr int kABytes = BM * 128;
  constexpr int kBuf = (BM + BN) * 128;

  uint32_t bid = xcd_swizzle(blockIdx.x, gridDim.x);
  uint32_t tile = SPLIT ? bid / splitk : bid;
  int m0 = (int)(tile / tiles_n) * BM;
  int n0 = (int)(tile % tiles_n) * BN;

  __shared__ __attribute__((aligned(16))) char smem[NBUF * kBuf];
  uint32_t lds0 = (uint32_t)(uintptr_t)&smem[0];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;

  typename Mfma16x16x32<T>::accv acc[BM / 32][BN / 32];
#pragma unroll
  for (int i = 0; i < BM / 32; ++i)
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) acc[i][j] = {0, 0, 0, 0};

  constexpr int KT = kTileElems<T>;
  const int ktiles = p.K / KT;
  int kt0 = 0, kt1 = ktiles;
  if constexpr (SPLIT) {
    int slice = bid % splitk;
    kt0 = slice * ktper;
    kt1 = min(ktiles, kt0 + ktper);
  }

  auto stage = [&](int t, int slot) {
    uint32_t base = lds0 + slot * kBuf;
    stage_conv_a<T, BM>(in, zero_page, p, m0, t * KT, base, tid);
    stage_tile<T, BN, true>(Wt + (int64_t)n0 * p.K + (int64_t)t * KT, p.K, n0,
                            p.Cout, base + kABytes, tid);
  };

  if constexpr (NBUF == 4) {
    constexpr int G = BM / 32 + BN / 32;
    for (int i = 0; i < 3 && kt0 + i < kt1; ++i) stage(kt0 + i, i);
    for (int t = kt0; t < kt1; ++t) {
      int ahead = kt1 - 1 - t;
      if (ahead > 2) ahead = 2;
      wait_tiles_inflight<G>(ahead);
      __builtin_amdgcn_s_barrier();
      if (t + 3 < kt1) stage(t + 3, (t + 3 - kt0) & 3);
      const char* As = &smem[((t - kt0) & 3) * kBuf];
      mfma_tile<T, BM, BN, true>(As, As + kABytes, lane, wr, wc, acc);
    }
  } else {
    stage(kt0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int t = kt0; t < kt1; ++t) {
      if (t + 1 < kt1) stage(t + 1, cur ^ 1);
      const char* As = &smem[cur * kBuf];
      mfma_tile<T, BM, BN, true>(As, As + kABytes, lane, wr, wc, acc);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      cur ^= 1;
    }
  }

  if constexpr (SPLIT) {
    store_splitk<T, BM, BN>(acc, scratch + (int64_t)bid * BM * BN, lane, wr,
                            wc);
  } else {
    store_epilogue<T, E, BM, BN>(acc, out, p.Cout, m0, n0, p.M, p.Cout, scale,
                                 bias, residual, p.res_scale, lane, wr, wc);
  }
}

size_t conv_scratch_bytes(int Nb, int H, int W, int C, int Cout, int KH,
                          int KW, int sh, int sw, int ph, int pw) {
  int OH = (H + 2 * ph - KH) / sh + 1;
  int OW = (W + 2 * pw - KW) / sw + 1;
  int M = Nb * OH * OW;
  int K = (int)round_up(KH * KW * C, 64);
  TileCfg cfg = pick_tile(M, Cout);
  long tiles = cdiv(M, cfg.bm) * cdiv(Cout, cfg.bn);
  int splitk = pick_splitk(tiles, K >> 6);
  if (splitk == 1) return 0;
  return (size_t)tiles * splitk * cfg.bm * cfg.bn * 4;
}

// ---- direct-to-VGPR small-K fast path ----
// 1x1/s1/p0 convs with exactly one 128-byte K-tile (K == 64 fp16 elems,
// e.g. the 16 C=64 1x1 convs in ResNet-50) are pure GEMMs with a single
// MFMA K-pass. For those the staged kernel's LDS round-trip + barrier IS
// the ~5-8 us latency floor (profiles/README "known next levers"), so this
// variant reads A and B fragments straight from global memory — each A
// fragment row is one 128-B cacheline, B (the 64xK weight panel) stays
// L2-resident across all M-tiles — and needs no LDS and no barrier.
// MFMA A/B lane layout: lane holds 8 contiguous k at row lane&15,
// k = (lane>>4)*8; with the weight fragment first, D: row = lane&15,
// channel = (lane>>4)*4 + r (gemm_common.h chan_of_frag_row).
template <typename T, Epi E>
__global__ __launch_bounds__(256) void conv_smallk_kernel(
    const T* __restrict__ A, const T* __restrict__ Bw, T* __restrict__ C,
    const float* __restrict__ scale, const float* __restrict__ bias,
    const T* __restrict__ residual, int M, int N, int K, float res_scale,
    int tiles_n) {
  using MF = Mfma16x16x32<T>;
  uint32_t blk = xcd_swizzle(blockIdx.x, gridDim.x);
  int m0 = (int)(blk / tiles_n) * 64, n0 = (int)(blk % tiles_n) * 64;
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int arow = m0 + wave * 16 + (lane & 15);
  if (arow >= M) arow = M - 1;  // clamp loads; stores are predicated
  constexpr int kEps = MF::kStepBytes / (int)sizeof(T);    // 32 (fp16)
  constexpr int kFe = MF::kFragBytes / (int)sizeof(T);     // 8
  constexpr int kSteps = 128 / MF::kStepBytes;             // 2
  f32x4 acc[1][4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc[0][f] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    int kb = s * kEps + (lane >> 4) * kFe;
    typename MF::frag af =
        *(const typename MF::frag*)(A + (int64_t)arow * K + kb);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      // channel-run mapping over the wave's 64 columns: weight first
      int brow = n0 + (int)chan_of_frag_row<64>(f * 16 + (lane & 15));
      if (brow >= N) brow = N - 1;
      typename MF::frag bf =
          *(const typename MF::frag*)(Bw + (int64_t)brow * K + kb);
      acc[0][f] = MF::run(bf, af, acc[0][f]);
    }
  }
  // lane: row wave*16 + (lane&15), 16 contiguous channels from (lane>>4)*16
  store_chan_runs<E>(acc, C, (int64_t)N, m0 + wave * 16 + (lane & 15),
                     n0 + (lane >> 4) * 16, M, N, scale, bias, residual,
                     res_scale, 1.0f);
}

// ---- fused bottleneck tail: conv3x3+BN+ReLU -> conv1x1+BN+res+ReLU ----
// The ResNet bottleneck interior (3x3 s1 p1, width CM) immediately feeds a
// 1x1 expand (CM -> Co) whose only input is the 3x3 output. One workgroup
// computes the ENTIRE channel extent (BN1 = CM) of the 3x3 for a 64-row
// spatial tile, applies BN+ReLU, re-stages the tile T[64][CM] into LDS in
// the standard swizzled A-tile layout, and runs the 1x1 GEMM (K = CM) from
// LDS — the intermediate tensor never touches HBM and one kernel launch
// (~10-15 us at these latency-bound b8 shapes) disappears per pair.
// CM in {64, 128} (ResNet-50 stages 1-2; wider stages would overflow the
// 64 KB static-LDS T tile at full width). fp16 only (the headline dtype).
template <typename T, int CM, bool DEEP, int BM = 64>
__global__ __launch_bounds__(256) void bottleneck_tail_kernel(
    const T* __restrict__ in, const T* __restrict__ W1,
    const T* __restrict__ W2, T* __restrict__ out,
    const float* __restrict__ s1, const float* __restrict__ b1,
    const float* __restrict__ s2, const float* __restrict__ b2,
    const T* __restrict__ residual, const T* __restrict__ zero_page,
    const ConvParams p, int Co) {
  constexpr int BNC = 64;                      // GEMM1 column chunk
  constexpr int NB1 = CM / BNC;                // chunks across the 3x3 width
  constexpr int kABytes = BM * 128;
  constexpr int kBuf = (BM + BNC) * 128;       // one GEMM1 staging slot
  constexpr int NBUF = DEEP ? 4 : 2;
  constexpr int kT2 = CM / 64;                 // GEMM2 K-tiles
  constexpr int kTBlk = BM * 128;              // one T K-tile block
  constexpr int kTBytes = kT2 * kTBlk;         // T tile (BM x CM fp16)
  constexpr int kSmem =
      (NBUF * kBuf > kTBytes + 8192) ? NBUF * kBuf : kTBytes + 8192;
  __shared__ __attribute__((aligned(16))) char smem[kSmem];
  uint32_t lds0 = (uint32_t)(uintptr_t)&smem[0];

  uint32_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  int m0 = (int)tile * BM;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;

  // ---- GEMM1: T = relu(bn1(conv3x3(in))), 64-col chunks so the staging
  // slot stays 16 KB and the 4-deep counted pipeline fits 64 KB LDS (the
  // grid-starved stage-2 shape needs it; accumulators for every chunk
  // stay live in VGPRs until the shared T-write below) ----
  typename Mfma16x16x32<T>::accv acc1[NB1][BM / 32][BNC / 32];
#pragma unroll
  for (int c = 0; c < NB1; ++c)
#pragma unroll
    for (int i = 0; i < BM / 32; ++i)
#pragma unroll
      for (int j = 0; j < BNC / 32; ++j) acc1[c][i][j] = {0, 0, 0, 0};

  const int ktiles = p.K / kTileElems<T>;
  for (int nc = 0; nc < NB1; ++nc) {
    auto stage1 = [&](int t, int slot) {
      uint32_t base = lds0 + slot * kBuf;
      stage_conv_a<T, BM>(in, zero_page, p, m0, t * kTileElems<T>, base,
                          tid);
      stage_tile<T, BNC, true>(W1 + (int64_t)nc * BNC * p.K +
                             (int64_t)t * kTileElems<T>,
                         p.K, nc * BNC, CM, base + kABytes, tid);
    };
    if constexpr (DEEP) {
      constexpr int G = BM / 32 + BNC / 32;
      for (int i = 0; i < 3 && i < ktiles; ++i) stage1(i, i);
      for (int t = 0; t < ktiles; ++t) {
        int ahead = ktiles - 1 - t;
        if (ahead > 2) ahead = 2;
        wait_tiles_inflight<G>(ahead);
        __builtin_amdgcn_s_barrier();
        if (t + 3 < ktiles) stage1(t + 3, (t + 3) & 3);
        const char* As = &smem[(t & 3) * kBuf];
        mfma_tile<T, BM, BNC, true>(As, As + kABytes, lane, wr, wc, acc1[nc]);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    } else {
      stage1(0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      int cur = 0;
      for (int t = 0; t < ktiles; ++t) {
        if (t + 1 < ktiles) stage1(t + 1, cur ^ 1);
        const char* As = &smem[cur * kBuf];
        mfma_tile<T, BM, BNC, true>(As, As + kABytes, lane, wr, wc, acc1[nc]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
      }
    }
  }

  // ---- T -> LDS in swizzled A-tile layout (GEMM1 LDS slots are dead) ----
  // Channel-run mapping: a lane holds 8 consecutive channels (= GEMM2 k
  // elements) of one row, exactly one swizzled 16-byte chunk of the T tile.
  static_assert(BNC == 64 && sizeof(T) == 2, "one 16-B chunk per lane");
#pragma unroll
  for (int nc = 0; nc < NB1; ++nc) {
    const int col0 = nc * BNC + wc * (BNC / 2) + (lane >> 4) * 8;
    float sc[8], bi[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      sc[c] = s1[col0 + c];
      bi[c] = b1[col0 + c];
    }
#pragma unroll
    for (int i = 0; i < BM / 32; ++i) {
      uint32_t row = (uint32_t)(wr * (BM / 2) + i * 16 + (lane & 15));
      __attribute__((aligned(16))) T o[8];
#pragma unroll
      for (int j = 0; j < BNC / 32; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          o[4 * j + r] = (T)fmaxf(
              (float)acc1[nc][i][j][r] * sc[4 * j + r] + bi[4 * j + r], 0.0f);
      uint32_t kb = (uint32_t)(col0 & 63) * (uint32_t)sizeof(T);
      uint32_t off = (uint32_t)(col0 >> 6) * (uint32_t)kTBlk + (row << 7) +
                     (kb ^ ((row & 7) << 4));
      i32x4 t;
      __builtin_memcpy(&t, o, 16);
      *(i32x4*)(smem + off) = t;
    }
  }
  __syncthreads();

  // ---- GEMM2: out = relu(bn2(T @ W2^T) + residual), N2 chunks of 64 ----
  const char* Tlds = smem;
  char* B2s = smem + kTBytes;
  for (int c2 = 0; c2 < Co / 64; ++c2) {
#pragma unroll
    for (int t = 0; t < kT2; ++t)
      stage_tile<T, 64, true>(W2 + (int64_t)c2 * 64 * CM + t * kTileElems<T>, CM,
                        c2 * 64, Co, (uint32_t)(uintptr_t)(B2s + t * 8192),
                        tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    typename Mfma16x16x32<T>::accv acc2[BM / 32][2];
#pragma unroll
    for (int i = 0; i < BM / 32; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc2[i][j] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < kT2; ++t)
      mfma_tile<T, BM, 64, true>(Tlds + t * kTBlk, B2s + t * 8192, lane, wr, wc,
                           acc2);
    store_epilogue<T, Epi::kScaleBiasAddRelu, BM, 64>(
        acc2, out, Co, m0, c2 * 64, p.M, Co, s2, b2, residual, p.res_scale,
        lane, wr, wc);
    __syncthreads();  // before the next chunk overwrites B2s
  }
}

void launch_bottleneck_tail(int dtype, const void* in, const void* W1,
                            const void* W2, void* out, const float* s1,
                            const float* b1, const float* s2, const float* b2,
                            const void* residual, const void* zero_page,
                            int Nb, int H, int W, int Cm, int Co,
                            hipStream_t stream) {
  if (dtype != 0)
    throw std::runtime_error("bottleneck_tail: fp16 only");
  if (Cm != 64 && Cm != 128)
    throw std::runtime_error("bottleneck_tail: Cm must be 64 or 128");
  if (Co % 64 != 0) throw std::runtime_error("bottleneck_tail: Co % 64");
  ConvParams p;
  p.res_scale = 1.0f;
  p.Nb = Nb; p.H = H; p.W = W; p.C = Cm;
  p.Cout = Cm; p.KH = 3; p.KW = 3;
  p.sh = 1; p.sw = 1; p.ph = 1; p.pw = 1;
  p.OH = H; p.OW = W;
  p.M = Nb * H * W;
  p.Kreal = 9 * Cm;
  p.K = p.Kreal;  // 9*Cm is a multiple of 64 for Cm in {64,128}
  p.d_ohw = make_fastdiv((uint32_t)(p.OH * p.OW));
  p.d_ow = make_fastdiv((uint32_t)p.OW);
  p.d_c = make_fastdiv((uint32_t)Cm);
  p.d_kw = make_fastdiv((uint32_t)p.KW);
  // grid-starved shapes (stage 2: 98 WGs at BM=64) halve the M-tile to
  // double the workgroup count; the deep pipeline follows the same gate
  // as the standalone conv.
  int bm = (cdiv(p.M, 64) >= 256) ? 64 : 32;
  dim3 grid((unsigned)cdiv(p.M, bm));
  bool deep = want_deep_pipe(grid.x, p.K / 64);
  auto go = [&](auto cm, auto dp, auto bmv) {
    constexpr int CMv = decltype(cm)::value;
    constexpr bool DPv = decltype(dp)::value;
    constexpr int BMv = decltype(bmv)::value;
    hipLaunchKernelGGL((bottleneck_tail_kernel<_Float16, CMv, DPv, BMv>),
                       grid, dim3(256), 0, stream, (const _Float16*)in,
                       (const _Float16*)W1, (const _Float16*)W2,
                       (_Float16*)out, s1, b1, s2, b2,
                       (const _Float16*)residual, (const _Float16*)zero_page,
                       p, Co);
  };
  auto c64 = std::integral_constant<int, 64>{};
  auto c128 = std::integral_constant<int, 128>{};
  auto b64 = std::integral_constant<int, 64>{};
  auto b32 = std::integral_constant<int, 32>{};
  if (Cm == 64) {
    if (bm == 64) { deep ? go(c64, std::true_type{}, b64)
                         : go(c64, std::false_type{}, b64); }
    else { deep ? go(c64, std::true_type{}, b32)
                : go(c64, std::false_type{}, b32); }
  } else {
    if (bm == 64) { deep ? go(c128, std::true_type{}, b64)
                         : go(c128, std::false_type{}, b64); }
    else { deep ? go(c128, std::true_type{}, b32)
                : go(c128, std::false_type{}, b32); }
  }
}

template <typename T>
static void launch_conv2d_t(const void* in, const void* Wt, void* out,
                            const float* scale, const float* bias,
                            const void* residual, const void* zero_page,
                            const ConvParams& p, int epi, hipStream_t stream,
                            int tile, float* scratch) {
  // small-K fast path (2-byte dtypes; K fits one tile with no zero pad).
  // Taken regardless of the autotuned tile code: it has no tiling choice.
  // (constexpr guard keeps the kernel uninstantiated for 1-byte formats,
  // whose single K-tile would still need zero-fill past C.)
  if constexpr (sizeof(T) == 2) {
  // grid-starved gate: at large M these shapes are bandwidth-bound and the
  // staged kernel's LDS B-reuse wins (measured: -1.4% on rn50 b8 ungated);
  // under ~384 workgroups the LDS round-trip + barrier latency dominates.
  if (p.KH == 1 && p.KW == 1 && p.sh == 1 && p.sw == 1 &&
      p.ph == 0 && p.pw == 0 && p.Kreal == p.K && p.K == kTileElems<T> &&
      cdiv(p.M, 64) * cdiv(p.Cout, 64) <= 384) {
    dim3 grid((unsigned)(cdiv(p.M, 64) * cdiv(p.Cout, 64)));
    int tn = (int)cdiv(p.Cout, 64);
    epi_dispatch(epi, [&](auto e) {
      constexpr Epi EE = decltype(e)::value;
      hipLaunchKernelGGL((conv_smallk_kernel<T, EE>), grid, dim3(256), 0,
                         stream, (const T*)in, (const T*)Wt, (T*)out, scale,
                         bias, (const T*)residual, p.M, p.Cout, p.K,
                         p.res_scale, tn);
    });
    return;
  }
  }
  // code 5 (256-wide) is a GEMM-only tactic: LDS would overflow the deep
  // conv pipeline, so fall back to the heuristic
  TileCfg cfg = (tile && tile != 5) ? tile_from_code(tile)
                                    : pick_tile(p.M, p.Cout);
  int tiles_m = (int)cdiv(p.M, cfg.bm);
  int tiles_n = (int)cdiv(p.Cout, cfg.bn);
  long tiles = (long)tiles_m * tiles_n;
  int ktiles = p.K / kTileElems<T>;
  int splitk = (!tile && scratch) ? pick_splitk(tiles, ktiles) : 1;
  dim3 block(256);
  int dtype = std::is_same<T, _Float16>::value
                  ? 0
                  : (std::is_same<T, __bf16>::value
                         ? 1
                         : (std::is_same<T, int8_t>::value ? 2 : 3));
  if (splitk > 1) {
    int ktper = (int)cdiv(ktiles, splitk);
    dim3 grid((unsigned)(tiles * splitk));
    bool deep = want_deep_pipe(tiles * splitk, ktper);
    tile_dispatch(cfg, [&](auto bm, auto bn) {
      constexpr int BM = decltype(bm)::value;
      constexpr int BN = decltype(bn)::value;
      if (deep)
        hipLaunchKernelGGL((conv_igemm_kernel<T, Epi::kNone, BM, BN, true, 4>),
                           grid, block, 0, stream, (const T*)in, (const T*)Wt,
                           (T*)out, scale, bias, (const T*)residual,
                           (const T*)zero_page, p, tiles_n, scratch, splitk,
                           ktper);
      else
        hipLaunchKernelGGL((conv_igemm_kernel<T, Epi::kNone, BM, BN, true, 2>),
                           grid, block, 0, stream, (const T*)in, (const T*)Wt,
                           (T*)out, scale, bias, (const T*)residual,
                           (const T*)zero_page, p, tiles_n, scratch, splitk,
                           ktper);
    });
    launch_splitk_reduce(dtype, scratch, out, scale, bias, residual,
                         p.res_scale, p.M, p.Cout, p.Cout, tiles_m, tiles_n,
                         splitk, cfg.bm, cfg.bn, epi, stream);
    return;
  }
  dim3 grid((unsigned)tiles);
  bool deep = want_deep_pipe(tiles, ktiles);
  epi_dispatch(epi, [&](auto e) {
    constexpr Epi EE = decltype(e)::value;
    tile_dispatch(cfg, [&](auto bm, auto bn) {
      constexpr int BM = decltype(bm)::value;
      constexpr int BN = decltype(bn)::value;
      if (deep)
        hipLaunchKernelGGL((conv_igemm_kernel<T, EE, BM, BN, false, 4>), grid,
                           block, 0, stream, (const T*)in, (const T*)Wt,
                           (T*)out, scale, bias, (const T*)residual,
                           (const T*)zero_page, p, tiles_n, (float*)nullptr,
                           1, ktiles);
      else
        hipLaunchKernelGGL((conv_igemm_kernel<T, EE, BM, BN, false, 2>), grid,
                           block, 0, stream, (const T*)in, (const T*)Wt,
                           (T*)out, scale, bias, (const T*)residual,
                           (const T*)zero_page, p, tiles_n, (float*)nullptr,
                           1, ktiles);
    });
  });
}

void launch_conv2d(int dtype, const void* in, const void* Wt, void* out,
                   const float* scale, const float* bias, const void* residual,
                   const void* zero_page, int Nb, int H, int W, int C,
                   int Cout, int KH, int KW, int sh, int sw, int ph, int pw,
                   int epi, hipStream_t stream, int tile, void* scratch,
                   float res_scale) {
  ConvParams p;
  p.res_scale = res_scale;
  p.Nb = Nb; p.H = H; p.W = W; p.C = C;
  p.Cout = Cout; p.KH = KH; p.KW = KW;
  p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw;
  p.OH = (H + 2 * ph - KH) / sh + 1;
  p.OW = (W + 2 * pw - KW) / sw + 1;
  p.M = Nb * p.OH * p.OW;
  p.Kreal = KH * KW * C;
  int kt = dtype >= 2 ? 128 : 64;  // 1-byte formats: 128 elems per K-tile
  p.K = (int)round_up(p.Kreal, kt);
  int cmin = dtype >= 2 ? 16 : 8;  // one 16-B glds chunk per pixel minimum
  if (C % cmin != 0)
    throw std::runtime_error("conv2d: C must be a multiple of 16 B / elem "
                             "size (pad input channels)");
  p.d_ohw = make_fastdiv((uint32_t)(p.OH * p.OW));
  p.d_ow = make_fastdiv((uint32_t)p.OW);
  p.d_c = make_fastdiv((uint32_t)C);
  p.d_kw = make_fastdiv((uint32_t)KW);
  if (dtype == 0)
    launch_conv2d_t<_Float16>(in, Wt, out, scale, bias, residual, zero_page, p,
                              epi, stream, tile, (float*)scratch);
  else if (dtype == 1)
    launch_conv2d_t<__bf16>(in, Wt, out, scale, bias, residual, zero_page, p,
                            epi, stream, tile, (float*)scratch);
  else if (dtype == 2)
    launch_conv2d_t<int8_t>(in, Wt, out, scale, bias, residual, zero_page, p,
                            epi, stream, tile, (float*)scratch);
  else
    launch_conv2d_t<__hip_fp8_e4m3>(in, Wt, out, scale, bias, residual,
                                    zero_page, p, epi, stream, tile,
                                    (float*)scratch);
}

}  // namespace trtlab
