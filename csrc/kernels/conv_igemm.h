// trtlab_amd — implicit-GEMM conv2d kernels and their per-dtype launcher
// (see conv.hip for the structure notes). A header so that each element
// type is instantiated in a translation unit of its own (conv_f16.hip,
// conv_bf16.hip, conv_i8.hip, conv_fp8.hip): the general and tap-uniform
// staging variants double the kernel count, and one file per type keeps
// the build's critical path below what the single file took before.
#pragma once
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

// Stage a ROWS x 64-elem A-tile of the implicit im2col matrix: the general
// path. Every lane derives (kh, kw, ci) and the source address from k for
// each chunk on every K-tile. Serves C % K-tile != 0 (the stem, 1-byte
// formats at C = 64, odd channel counts), where a K-tile straddles taps
// or runs into the zero-padded K tail.
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

// ---- tap-uniform A staging (C % K-tile == 0) ----
// A K-tile then lies inside one filter tap: (kh, kw, ci0) is the same for
// the whole workgroup and lives in scalar registers (TapCursor), advanced
// incrementally once per staged tile. The row part (n, oh, ow) does not
// depend on k and is decomposed once per thread before the K-loop
// (TapRows). Per chunk per tile that leaves one add, two unsigned compares
// and the zero-page select; pointwise convs (one tap, always in the image)
// drop the compares and the select too. Same glds16 count, order, sources
// and LDS image as stage_conv_a. Offsets are 32-bit byte offsets modulo
// 2^32 (the host takes this path only for inputs under 2 GiB): a row whose
// (ih0, iw0) is outside the image holds a wrapped value, which becomes the
// true offset again once an in-image tap is added.
template <int ROWS>
struct TapRows {
  uint32_t off[ROWS / 32];  // byte offset of (n, ih0, iw0, channel 0) + kb
  int ih0[ROWS / 32];       // oh*sh - ph
  int iw0[ROWS / 32];       // ow*sw - pw
};

struct TapCursor {
  int kh, kw, ci0;  // tap and first channel of the next K-tile to stage
  uint32_t off;     // ((kh*W + kw)*C + ci0) * sizeof(T)
  bool pointwise;   // KH == KW == 1, no padding: every tap is in the image
};

template <typename T, int ROWS>
__device__ __forceinline__ TapRows<ROWS> tap_rows_init(const ConvParams& p,
                                                       int m0, int tid) {
  TapRows<ROWS> r;
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
    r.ih0[c] = (int)oh * p.sh - p.ph;
    r.iw0[c] = (int)ow * p.sw - p.pw;
    uint32_t pixel = (n * (uint32_t)p.H + (uint32_t)r.ih0[c]) * (uint32_t)p.W +
                     (uint32_t)r.iw0[c];
    r.off[c] = pixel * (uint32_t)p.C * (uint32_t)sizeof(T) + kb;
  }
  return r;
}

// Cursor at K-tile kt (a split-K slice may start in mid-tap).
template <typename T>
__device__ __forceinline__ TapCursor tap_cursor_init(const ConvParams& p,
                                                     int kt) {
  TapCursor cur;
  uint32_t k = (uint32_t)kt * (uint32_t)kTileElems<T>;
  uint32_t pix = fdiv(k, p.d_c);
  uint32_t kh = fdiv(pix, p.d_kw);
  cur.ci0 = (int)(k - pix * (uint32_t)p.C);
  cur.kh = (int)kh;
  cur.kw = (int)(pix - kh * (uint32_t)p.KW);
  cur.off = ((kh * (uint32_t)p.W + (uint32_t)cur.kw) * (uint32_t)p.C +
             (uint32_t)cur.ci0) * (uint32_t)sizeof(T);
  cur.pointwise = p.KH == 1 && p.KW == 1 && p.ph == 0 && p.pw == 0;
  return cur;
}

// Stage the A-tile under the cursor, then advance the cursor by one K-tile.
template <typename T, int ROWS>
__device__ __forceinline__ void stage_conv_a_tap(
    const T* __restrict__ in, const T* __restrict__ zero_page,
    const ConvParams& p, const TapRows<ROWS>& r, TapCursor& cur,
    uint32_t lds_base, int tid) {
  const char* inb = (const char*)in;
  if (cur.pointwise) {
#pragma unroll
    for (int c = 0; c < ROWS / 32; ++c)
      glds16(inb + (uint32_t)(r.off[c] + cur.off),
             lds_base + c * 4096 + tid * 16);
    cur.off += 128;  // the one tap: a plain pointer bump, as stage_tile
    return;
  }
#pragma unroll
  for (int c = 0; c < ROWS / 32; ++c) {
    bool ok = ((uint32_t)(r.ih0[c] + cur.kh) < (uint32_t)p.H) &
              ((uint32_t)(r.iw0[c] + cur.kw) < (uint32_t)p.W);
    const char* src = inb + (uint32_t)(r.off[c] + cur.off);
    glds16(ok ? src : (const char*)zero_page, lds_base + c * 4096 + tid * 16);
  }
  // next tile: 128 bytes on along the pixel's channels; running off the
  // pixel lands on the next kw, running off the filter row skips to kh+1
  cur.off += 128;
  cur.ci0 += kTileElems<T>;
  if (cur.ci0 == p.C) {
    cur.ci0 = 0;
    if (++cur.kw == p.KW) {
      cur.kw = 0;
      ++cur.kh;
      cur.off += (uint32_t)(p.W - p.KW) * (uint32_t)p.C * (uint32_t)sizeof(T);
    }
  }
}

void launch_splitk_reduce(int dtype, const float* scratch, void* C,
                          const float* scale, const float* bias,
                          const void* residual, float res_scale, int M, int N,
                          int64_t ldc, int tiles_m, int tiles_n, int splitk,
                          int bm, int bn, int epi, hipStream_t stream);

// TAP: tap-uniform A staging (host guarantees C % K-tile == 0 and an input
// under 2 GiB); otherwise the general per-lane path.
template <typename T, Epi E, int BM, int BN, bool SPLIT, int NBUF,
          bool TAP = false>
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

  // tap-uniform state; stage() is called for consecutive t from kt0 on,
  // so the cursor always sits on the tile being staged
  TapRows<TAP ? BM : 32> rows;
  TapCursor tap;
  if constexpr (TAP) {
    rows = tap_rows_init<T, BM>(p, m0, tid);
    tap = tap_cursor_init<T>(p, kt0);
  }

  auto stage = [&](int t, int slot) {
    uint32_t base = lds0 + slot * kBuf;
    if constexpr (TAP)
      stage_conv_a_tap<T, BM>(in, zero_page, p, rows, tap, base, tid);
    else
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

// The tap-uniform staging addresses the input with 32-bit byte offsets.
static inline bool tap_offsets_fit(int64_t input_bytes) {
  return input_bytes < ((int64_t)1 << 31);
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

template <typename T>
void launch_conv2d_t(const void* in, const void* Wt, void* out,
                            const float* scale, const float* bias,
                            const void* residual, const void* zero_page,
                            const ConvParams& p, int epi, hipStream_t stream,
                            int tile, float* scratch, int staging) {
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
  // A-tile staging path: tap-uniform whenever a K-tile lies inside one
  // filter tap (which also means Kreal == K, no zero-padded K-tile);
  // staging == 1 forces the general path (A/B runs and tests).
  const bool tap =
      staging != 1 && p.C % kTileElems<T> == 0 &&
      tap_offsets_fit((int64_t)p.Nb * p.H * p.W * p.C * (int64_t)sizeof(T));
  auto tap_dispatch = [&](auto&& f) {
    if (tap) f(std::true_type{});
    else f(std::false_type{});
  };
  if (splitk > 1) {
    int ktper = (int)cdiv(ktiles, splitk);
    dim3 grid((unsigned)(tiles * splitk));
    bool deep = want_deep_pipe(tiles * splitk, ktper);
    tile_dispatch(cfg, [&](auto bm, auto bn) {
      constexpr int BM = decltype(bm)::value;
      constexpr int BN = decltype(bn)::value;
      tap_dispatch([&](auto tp) {
        constexpr bool TAP = decltype(tp)::value;
        if (deep)
          hipLaunchKernelGGL(
              (conv_igemm_kernel<T, Epi::kNone, BM, BN, true, 4, TAP>), grid,
              block, 0, stream, (const T*)in, (const T*)Wt, (T*)out, scale,
              bias, (const T*)residual, (const T*)zero_page, p, tiles_n,
              scratch, splitk, ktper);
        else
          hipLaunchKernelGGL(
              (conv_igemm_kernel<T, Epi::kNone, BM, BN, true, 2, TAP>), grid,
              block, 0, stream, (const T*)in, (const T*)Wt, (T*)out, scale,
              bias, (const T*)residual, (const T*)zero_page, p, tiles_n,
              scratch, splitk, ktper);
      });
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
      tap_dispatch([&](auto tp) {
        constexpr bool TAP = decltype(tp)::value;
        if (deep)
          hipLaunchKernelGGL(
              (conv_igemm_kernel<T, EE, BM, BN, false, 4, TAP>), grid, block,
              0, stream, (const T*)in, (const T*)Wt, (T*)out, scale, bias,
              (const T*)residual, (const T*)zero_page, p, tiles_n,
              (float*)nullptr, 1, ktiles);
        else
          hipLaunchKernelGGL(
              (conv_igemm_kernel<T, EE, BM, BN, false, 2, TAP>), grid, block,
              0, stream, (const T*)in, (const T*)Wt, (T*)out, scale, bias,
              (const T*)residual, (const T*)zero_page, p, tiles_n,
              (float*)nullptr, 1, ktiles);
      });
    });
  });
}

}  // namespace trtlab
