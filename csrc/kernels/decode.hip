// trtlab_amd — incremental (KV-cache) decode kernels for GPT-family
// serving on gfx950. Beyond-reference capability: the CUDA reference
// served static TensorRT engines only.
//
// Design: the decode step is captured in a hipGraph once and replayed per
// token. All position dependence goes through a DEVICE-side PER-SEQUENCE
// counter array (`pos[B]`), so replays need no re-capture — and a slot
// can be reset to position 0 between replays (continuous batching in
// lockstep: a finished sequence's slot restarts a new request while the
// other slots keep decoding). advance_pos bumps every slot at the end of
// the captured step.
//
// One kernel body each for the K/V scatter, the single-query attention
// and the embedding. Two axes select the variant:
//   rows — query/source rows per slot, b-major then row: 1 for a decode
//          step, K for a speculative-verification chunk (row q of slot b
//          sits at position pos[b] + q), P for a prefill range (pos is
//          null: base position 0).
//   KV   — cache layout policy (DenseKV / PagedKV below), the only code
//          that knows how row t of (slot, head) is addressed.
// Grouped-query attention (Hq query heads over Hkv kv heads, G = Hq/Hkv)
// is not a third axis of the layouts: the caches simply hold Hkv heads
// (the policies are addressed with H := Hkv), the fused qkv row narrows to
// [q: Hq*D | k: Hkv*D | v: Hkv*D], and the attention workgroup grows to G
// waves (see decode_attention_kernel). Hkv = Hq is plain MHA, G = 1.
//
// Bounds rule (every kernel here, both layouts):
//   * pos[b] < 0 marks slot b IDLE: the block exits — no cache write, no
//     scan, no output, position stays parked — so empty slots in a
//     continuous batch cost ~nothing while the graph keeps its shape.
//     A null pos (range append) has no idle slots.
//   * a write position is clamped to smax-1; the attended length n is
//     clamped to smax (<= 4096, the LDS score buffer — launcher-checked).
//     Clamped rows pile up on position smax-1, which is rewritten by a
//     later step before it is ever attended.
//   * a paged row whose page is unmapped (table entry < 0, or logical
//     page >= max_pages) is skipped on append. Attention does not test
//     it: the host maps every page below pos[b] + rows before launch.
//   smax is the session's position bound for both layouts, NOT
//   max_pages*64: a shared pool may be larger than one session's window.
//
// A third, orthogonal axis is the cache ELEMENT format (Fp16Cache /
// Mx8Cache below): fp16 rows, or MXFP8 rows — D e4m3 code bytes plus D/32
// e8m0 scale bytes in a separate buffer. kv_append quantises, attention
// dequantises in registers; the layouts, the bounds rule and the work
// decomposition are the same for both.
#include "gemm_common.h"
#include "mx_common.h"

namespace trtlab {

// Dense cache, per layer: K and V as [B][H][smax][D] fp16 (a key's head
// row is contiguous — one 128-B cacheline at D = 64).
struct DenseKV {
  int smax;
  __device__ int64_t row(int b, int h, int H, int D, int t) const {
    return (((int64_t)b * H + h) * smax + t) * D;
  }
};

// Paged cache (vLLM-style block tables): many sessions share ONE fixed
// physical pool per layer; each slot maps logical 64-position pages to
// physical page ids through a device table [B][max_pages] (filled by the
// host as positions grow; reset/idle returns pages to the host free list,
// so parked slots hold no memory). Pool layout [page][64][H][D] — a
// position's per-head row stays contiguous. row() is negative when the
// page is unmapped: a negative page id makes the whole offset negative
// ((page*64 + t%64)*H + h < 0 for h < H), so the read path pays no test;
// the table index is clamped so the lookup itself stays in bounds.
struct PagedKV {
  const int* table;
  int max_pages;
  __device__ int64_t row(int b, int h, int H, int D, int t) const {
    int lp = t >> 6;
    int page = table[b * max_pages + min(lp, max_pages - 1)];
    if (lp >= max_pages) page = -1;
    return (((int64_t)page * 64 + (t & 63)) * H + h) * D;
  }
};

// Cache element format. Fp16Cache: the row is D fp16 values. Mx8Cache
// (MXFP8): the row is D e4m3 bytes in the cache buffer (same shape as the
// fp16 cache, 1-byte elements) plus D/32 e8m0 scale bytes, one per 32
// consecutive elements, in kscale / vscale. Row offsets are multiples of
// D, so the scale offset of a row is row / 32 for either layout and the
// layout policies need no second addressing rule. The quantisation rule
// is mx_common.h's (the one every MX producer shares): e = floor(log2
// amax) - 8, codes saturate to +-448 and round to nearest even, scale
// byte e + 127; an all-zero block stores byte 127.
struct Fp16Cache {
  using elem = _Float16;
  static constexpr bool kMx = false;
};
struct Mx8Cache {
  using elem = unsigned char;
  static constexpr bool kMx = true;
  unsigned char* kscale;
  unsigned char* vscale;
};

// Scatter K/V head rows from the fused qkv projection output (qkv
// [B*rows, (Hq + 2*Hkv)*D]) into the cache at position
// (pos ? pos[b] : 0) + q. One block per (b, kv head, q); H is Hkv.
// Mx8Cache (D = 64 or 128, launcher-checked): lane d owns element d (and
// d + 64), its 32-element block is the 32-lane half of the wave it sits
// in, so the block amax is five xor-shuffles; the lane with d % 32 == 0
// stores the block's scale byte.
template <class KV, class EF>
__global__ __launch_bounds__(64) void kv_append_kernel(
    const _Float16* __restrict__ qkv, typename EF::elem* __restrict__ kcache,
    typename EF::elem* __restrict__ vcache, const int* __restrict__ pos,
    KV kv, EF ef, int H, int Hq, int rows, int smax, int D) {
  int q = blockIdx.x % rows;
  int bh = blockIdx.x / rows;
  int b = bh / H, h = bh % H;
  int p = q;
  if (pos) {
    int p0 = pos[b];
    if (p0 < 0) return;  // idle slot
    p += p0;
  }
  if (p >= smax) p = smax - 1;
  int64_t dst = kv.row(b, h, H, D, p);
  if (dst < 0) return;  // unmapped page (host error) — fail soft, not wild
  int khid = H * D;
  int64_t src = ((int64_t)b * rows + q) * (Hq + 2 * H) * D + Hq * D + h * D;
  if constexpr (EF::kMx) {
    // D is a multiple of 64: every lane runs the same trip count, so the
    // shuffles below are wave-uniform.
    for (int d = threadIdx.x; d < D; d += 64) {
      float k = (float)qkv[src + d];
      float v = (float)qkv[src + khid + d];
      float ka = fabsf(k), va = fabsf(v);
#pragma unroll
      for (int off = 16; off; off >>= 1) {
        ka = fmaxf(ka, __shfl_xor(ka, off, 64));
        va = fmaxf(va, __shfl_xor(va, off, 64));
      }
      int ke = mx_block_exponent(ka, 8);
      int ve = mx_block_exponent(va, 8);
      kcache[dst + d] = mx_encode_e4m3(k * exp2f((float)-ke));
      vcache[dst + d] = mx_encode_e4m3(v * exp2f((float)-ve));
      if ((d & 31) == 0) {
        ef.kscale[(dst + d) >> 5] = (unsigned char)(ke + 127);
        ef.vscale[(dst + d) >> 5] = (unsigned char)(ve + 127);
      }
    }
  } else {
    for (int d = threadIdx.x; d < D; d += 64) {
      kcache[dst + d] = qkv[src + d];
      vcache[dst + d] = qkv[src + khid + d];
    }
  }
}

// kv_format of the launchers: 0 fp16, 1 mxfp8 (needs both scale buffers).
static bool kv_format_is_mx(const char* op, int kv_format, const void* kscale,
                            const void* vscale) {
  if (kv_format != 0 && kv_format != 1)
    throw std::runtime_error(std::string(op) + ": unknown kv_format " +
                             std::to_string(kv_format));
  if (kv_format == 1 && (!kscale || !vscale))
    throw std::runtime_error(std::string(op) +
                             ": mxfp8 cache needs kscale and vscale");
  return kv_format == 1;
}

// Hq query heads over Hkv kv heads: kv_heads = 0 means Hkv = Hq (MHA).
static int gqa_kv_heads(const char* op, int H, int kv_heads) {
  int Hkv = kv_heads > 0 ? kv_heads : H;
  if (Hkv > H || H % Hkv != 0)
    throw std::runtime_error(std::string(op) +
                             ": heads must be a multiple of kv_heads");
  return Hkv;
}

void launch_kv_append(const void* qkv, void* kcache, void* vcache,
                      const void* pos, const void* table, int max_pages,
                      int B, int H, int rows, int smax, hipStream_t stream,
                      int D, int kv_heads, void* kscale, void* vscale,
                      int kv_format) {
  if (rows < 1) throw std::runtime_error("kv_append: rows < 1");
  int Hkv = gqa_kv_heads("kv_append", H, kv_heads);
  bool mx = kv_format_is_mx("kv_append", kv_format, kscale, vscale);
  if (mx && D != 64 && D != 128)
    throw std::runtime_error("kv_append: mxfp8 head_dim must be 64 or 128");
  auto L = [&](auto kv, auto ef) {
    using E = typename decltype(ef)::elem;
    hipLaunchKernelGGL((kv_append_kernel<decltype(kv), decltype(ef)>),
                       dim3(B * Hkv * rows), dim3(64), 0, stream,
                       (const _Float16*)qkv, (E*)kcache, (E*)vcache,
                       (const int*)pos, kv, ef, Hkv, H, rows, smax, D);
  };
  auto LE = [&](auto kv) {
    if (mx) L(kv, Mx8Cache{(unsigned char*)kscale, (unsigned char*)vscale});
    else L(kv, Fp16Cache{});
  };
  if (table) LE(PagedKV{(const int*)table, max_pages});
  else LE(DenseKV{smax});
}

// Single-query attention against the cache: query row (b, q) attends keys
// 0 .. pos[b]+q (its own K already appended), out[(b*rows+q), h*D+d] =
// softmax(q . K) @ V. One wave per (b, h, q) — a chunk's queries are
// causal within the chunk by construction of their lengths. Each lane
// owns keys lane, lane+64, ... for the score pass (its K rows are whole
// cachelines), then output element d = lane (+64) for the PV pass with
// the probabilities broadcast through LDS.
//
// Grouped-query: one workgroup per (b, kv head, q) with G waves; wave g
// is query head hk*G + g and runs the per-wave body above against the kv
// head's rows with its own 4096-float slice of p_s. The G waves share a
// CU and walk the same K/V rows in step, so a row leaves HBM once per
// group (the other G-1 reads hit the CU's L1/L2) instead of once per
// query head. The __syncthreads() are workgroup-wide; idle exit and n
// depend on (b, q) only, so every wave of a group takes them alike.
// G = 1 is the MHA kernel: same grid, same 16 KiB of LDS, same
// arithmetic order. p_s is G * 16 KiB of static LDS (128 KiB at G = 8,
// within the 160 KiB a gfx950 workgroup may declare).
//
// Mx8Cache: the lane's K row is D code bytes (16-byte loads, half of
// fp16's) and D/32 scale bytes (one 2- or 4-byte load). Codes go through
// the hardware fp8 -> f32 convert; each 32-element block's partial dot
// product is scaled by 2^(byte - 127) with ldexp, which is exact, so the
// score equals the one computed on the dequantised row with block-wise
// accumulation. PV: lane d converts its V code byte and applies its
// block's scale the same way. Everything from the softmax on is shared.
template <int D, int G, class KV, class EF>  // D 64|128; G 1,2,4,8
__global__ __launch_bounds__(64 * G) void decode_attention_kernel(
    const _Float16* __restrict__ qkv,
    const typename EF::elem* __restrict__ kcache,
    const typename EF::elem* __restrict__ vcache, _Float16* __restrict__ out,
    const int* __restrict__ pos, KV kv, EF ef, int H, int rows, int smax,
    float scale) {
  __shared__ float p_all[G * 4096];
  int q = blockIdx.x % rows;
  int bh = blockIdx.x / rows;
  int b = bh / H, hk = bh % H;  // H = kv heads
  int lane = threadIdx.x & 63;
  // wave index, kept scalar so the K/V row addresses stay wave-uniform
  int g = G == 1 ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* p_s = p_all + g * 4096;
  int h = hk * G + g;           // query head
  int hid = H * G * D;          // q block / output row width
  int p0 = pos[b];
  if (p0 < 0) return;  // idle slot: stale output row unused
  int n = p0 + q + 1;
  if (n > smax) n = smax;

  // q for this head (fp16 registers: D=128 stays within budget)
  _Float16 qv[D];
  {
    const _Float16* qrow =
        qkv + ((int64_t)b * rows + q) * (G + 2) * H * D + h * D;
#pragma unroll
    for (int c = 0; c < D / 8; ++c)
      *(half8v*)(qv + c * 8) = *(const half8v*)(qrow + c * 8);
  }

  // scores for this lane's keys
  float m = -3.0e38f;
  for (int t = lane; t < n; t += 64) {
    float s = 0.f;
    if constexpr (EF::kMx) {
      int64_t r = kv.row(b, hk, H, D, t);
      const unsigned char* krow = kcache + r;
      using scales_t =
          std::conditional_t<D == 128, unsigned int, unsigned short>;
      unsigned int sb = *(const scales_t*)(ef.kscale + (r >> 5));
#pragma unroll
      for (int blk = 0; blk < D / 32; ++blk) {
        float bs = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          i32x4 w = *(const i32x4*)(krow + blk * 32 + c * 16);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[j], false);
            auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[j], true);
            const _Float16* qe = qv + blk * 32 + c * 16 + j * 4;
            bs += (float)qe[0] * lo[0];
            bs += (float)qe[1] * lo[1];
            bs += (float)qe[2] * hi[0];
            bs += (float)qe[3] * hi[1];
          }
        }
        s += ldexpf(bs, (int)((sb >> (8 * blk)) & 255u) - 127);
      }
    } else {
      const _Float16* krow = kcache + kv.row(b, hk, H, D, t);
#pragma unroll
      for (int c = 0; c < D / 8; ++c) {
        half8v v = *(const half8v*)(krow + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s += (float)qv[c * 8 + j] * (float)((const _Float16*)&v)[j];
      }
    }
    s *= scale;
    p_s[t] = s;
    m = fmaxf(m, s);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  __syncthreads();
  float l = 0.f;
  for (int t = lane; t < n; t += 64) {
    float e = __expf(p_s[t] - m);
    p_s[t] = e;
    l += e;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) l += __shfl_xor(l, off, 64);
  __syncthreads();

  // PV: output elements d = lane (+64 for D=128)
  float acc[D / 64];
#pragma unroll
  for (int j = 0; j < D / 64; ++j) acc[j] = 0.f;
  for (int t = 0; t < n; ++t) {
    float p = p_s[t];
    if constexpr (EF::kMx) {
      int64_t r = kv.row(b, hk, H, D, t);
      const unsigned char* vrow = vcache + r;
      const unsigned char* srow = ef.vscale + (r >> 5);
#pragma unroll
      for (int j = 0; j < D / 64; ++j) {
        int d = j * 64 + lane;
        float v = __builtin_amdgcn_cvt_f32_fp8((int)vrow[d], 0);
        acc[j] += p * ldexpf(v, (int)srow[d >> 5] - 127);
      }
    } else {
      const _Float16* vrow = vcache + kv.row(b, hk, H, D, t);
#pragma unroll
      for (int j = 0; j < D / 64; ++j)
        acc[j] += p * (float)vrow[j * 64 + lane];
    }
  }
#pragma unroll
  for (int j = 0; j < D / 64; ++j)
    out[((int64_t)b * rows + q) * hid + h * D + j * 64 + lane] =
        (_Float16)(acc[j] / l);
}

void launch_decode_attention(const void* qkv, const void* kcache,
                             const void* vcache, void* out, const void* pos,
                             const void* table, int max_pages, int B, int H,
                             int rows, int smax, float scale,
                             hipStream_t stream, int D, int kv_heads,
                             const void* kscale, const void* vscale,
                             int kv_format) {
  if (smax > 4096)
    throw std::runtime_error("decode_attention: smax > 4096 unsupported");
  if (D != 64 && D != 128)
    throw std::runtime_error("decode_attention: head_dim must be 64 or 128");
  if (rows < 1) throw std::runtime_error("decode_attention: rows < 1");
  int Hkv = gqa_kv_heads("decode_attention", H, kv_heads);
  int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8)
    throw std::runtime_error(
        "decode_attention: heads / kv_heads must be 1, 2, 4 or 8");
  bool mx = kv_format_is_mx("decode_attention", kv_format, kscale, vscale);
  auto L = [&](auto d_c, auto g_c, auto kv, auto ef) {
    using E = typename decltype(ef)::elem;
    hipLaunchKernelGGL(
        (decode_attention_kernel<decltype(d_c)::value, decltype(g_c)::value,
                                 decltype(kv), decltype(ef)>),
        dim3(B * Hkv * rows), dim3(64 * decltype(g_c)::value), 0, stream,
        (const _Float16*)qkv, (const E*)kcache, (const E*)vcache,
        (_Float16*)out, (const int*)pos, kv, ef, Hkv, rows, smax, scale);
  };
  auto LE = [&](auto d_c, auto g_c, auto kv) {
    if (mx)
      L(d_c, g_c, kv,
        Mx8Cache{(unsigned char*)kscale, (unsigned char*)vscale});
    else
      L(d_c, g_c, kv, Fp16Cache{});
  };
  auto LG = [&](auto d_c, auto kv) {
    if (G == 1) LE(d_c, std::integral_constant<int, 1>{}, kv);
    else if (G == 2) LE(d_c, std::integral_constant<int, 2>{}, kv);
    else if (G == 4) LE(d_c, std::integral_constant<int, 4>{}, kv);
    else LE(d_c, std::integral_constant<int, 8>{}, kv);
  };
  using D64 = std::integral_constant<int, 64>;
  using D128 = std::integral_constant<int, 128>;
  PagedKV paged{(const int*)table, max_pages};
  DenseKV dense{smax};
  if (table && D == 128) LG(D128{}, paged);
  else if (table) LG(D64{}, paged);
  else if (D == 128) LG(D128{}, dense);
  else LG(D64{}, dense);
}

// Token + position embedding: out[b*rows + q] = tok[ids[b*rows + q]] +
// posemb[pos[b] + q].
__global__ void decode_embed_kernel(const int* __restrict__ ids,
                                    const _Float16* __restrict__ tok,
                                    const _Float16* __restrict__ posemb,
                                    _Float16* __restrict__ out,
                                    const int* __restrict__ pos, int rows,
                                    int smax, int hidden) {
  int q = blockIdx.x % rows;
  int b = blockIdx.x / rows;
  int p0 = pos[b];
  if (p0 < 0) return;  // idle slot
  int p = p0 + q;
  if (p >= smax) p = smax - 1;
  int64_t r = (int64_t)b * rows + q;
  int64_t t = (int64_t)ids[r] * hidden;
  for (int i = threadIdx.x; i < hidden; i += blockDim.x)
    out[r * hidden + i] =
        (_Float16)((float)tok[t + i] +
                   (float)posemb[(int64_t)p * hidden + i]);
}

void launch_decode_embed(const void* ids, const void* tok, const void* posemb,
                         void* out, const void* pos, int B, int rows,
                         int smax, int hidden, hipStream_t stream) {
  if (rows < 1) throw std::runtime_error("decode_embed: rows < 1");
  hipLaunchKernelGGL(decode_embed_kernel, dim3(B * rows), dim3(256), 0,
                     stream, (const int*)ids, (const _Float16*)tok,
                     (const _Float16*)posemb, (_Float16*)out,
                     (const int*)pos, rows, smax, hidden);
}

// Advance every slot's position counter (last node of the captured
// decode step; clamped so replay past smax is safe).
__global__ void advance_pos_kernel(int* pos, int B, int smax) {
  int b = threadIdx.x;
  if (b < B && pos[b] >= 0) {  // idle slots stay parked at -1
    int p = pos[b] + 1;
    pos[b] = p >= smax ? smax - 1 : p;
  }
}

void launch_advance_pos(void* pos, int B, int smax, hipStream_t stream) {
  hipLaunchKernelGGL(advance_pos_kernel, dim3(1),
                     dim3((B + 63) / 64 * 64), 0, stream, (int*)pos, B,
                     smax);
}


// ---- fused decode GEMM (horizontal fusion for the latency-bound step) ----
// The decode step is kernel-COUNT bound (~4.6 us replay floor/kernel), so
// this kernel folds the surrounding elementwise work into the small-M
// (M = batch <= 64) GEMMs:
//   prologue PRO: 1 = LN(x), 2 = ADD_LN(x + r, also storing the new
//   residual stream h_out — blocks write identical values, benign),
//   3 = EMBED_LN(tok[ids[b]] + posemb[pos[b]])
//   epilogue EPI: 0 = +bias, 1 = gelu(+bias), 2 = +bias AND scatter the
//   K/V column ranges into the caches at pos[b] (replaces kv_append)
// One block per 64 output columns; rows are the whole batch. LN stats are
// computed in-block (4 lanes per row, shfl-combined) and the normalized
// A-tile is ds_written per K-step with the same XOR swizzle the MFMA
// fragment reads expect. Cuts the GPT-2 step from ~8 to 5 kernels/layer.
template <int PRO, int EPI>
__global__ __launch_bounds__(256) void decode_gemm_fused_kernel(
    const _Float16* __restrict__ x, const _Float16* __restrict__ r,
    _Float16* __restrict__ h_out, const float* __restrict__ gamma,
    const float* __restrict__ beta, const _Float16* __restrict__ Bw,
    const float* __restrict__ bias, _Float16* __restrict__ C,
    const int* __restrict__ ids, const _Float16* __restrict__ tok,
    const _Float16* __restrict__ posemb, const int* __restrict__ pos,
    _Float16* __restrict__ kcache, _Float16* __restrict__ vcache, int M,
    int N, int K, int heads, int smax, float eps) {
  constexpr int BM = 64, BN = 64;
  __shared__ __attribute__((aligned(16))) char smem[2 * (BM + BN) * 128];
  __shared__ float sm_mean[BM], sm_inv[BM];
  // gamma/beta staged once per block: the per-tile normalize would
  // otherwise expose a global-latency chain every iteration
  __shared__ float sm_gamma[2048], sm_beta[2048];
  uint32_t lds0 = (uint32_t)(uintptr_t)&smem[0];
  constexpr int kABytes = BM * 128;
  constexpr int kBuf = (BM + BN) * 128;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1;
  const int wc = wave & 1;
  const int n0 = (int)blockIdx.x * BN;
  int cur_kbase = 0;  // K-base of the tile currently being staged

  // source value of the pre-norm row (x + r / embed), 8 elems at kk
  auto load8 = [&](int row, int kk, _Float16* v8) {
    if (PRO == 3) {
      int p = pos[row];
      if (p < 0) p = 0;
      const _Float16* trow = tok + (int64_t)ids[row] * K + kk;
      const _Float16* prow = posemb + (int64_t)p * K + kk;
      half8v a = *(const half8v*)trow;
      half8v b = *(const half8v*)prow;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v8[j] = (_Float16)((float)((const _Float16*)&a)[j] +
                           (float)((const _Float16*)&b)[j]);
    } else if (PRO == 2) {
      half8v a = *(const half8v*)(x + (int64_t)row * K + kk);
      half8v b = *(const half8v*)(r + (int64_t)row * K + kk);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v8[j] = (_Float16)((float)((const _Float16*)&a)[j] +
                           (float)((const _Float16*)&b)[j]);
    } else {
      *(half8v*)v8 = *(const half8v*)(x + (int64_t)row * K + kk);
    }
  };

  // ---- stage gamma/beta + LN stats ----
  for (int i = tid; i < K; i += 256) {
    sm_gamma[i] = gamma ? gamma[i] : 1.0f;
    sm_beta[i] = beta ? beta[i] : 0.0f;
  }
  {
    int row = tid >> 2;
    int part = tid & 3;
    float s = 0.f, ss = 0.f;
    if (row < M) {
      for (int kk = part * 8; kk < K; kk += 32) {
        _Float16 v8[8];
        load8(row, kk, v8);
        // block 0 persists the new residual stream h_out = x + r. h_out
        // MUST be a different buffer than r (ping-pong in the session):
        // other blocks re-read r during their own staging, so an in-place
        // update would race. Every block computes identical values; the
        // n0 gate just avoids duplicate HBM traffic.
        if ((PRO == 2 || PRO == 3) && n0 == 0 && h_out)
          *(half8v*)(h_out + (int64_t)row * K + kk) = *(const half8v*)v8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = (float)v8[j];
          s += f;
          ss += f * f;
        }
      }
    }
    // combine the 4 partial lanes of this row (consecutive lanes)
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    if (part == 0 && row < M) {
      float mean = s / K;
      float var = ss / K - mean * mean;
      sm_mean[row] = mean;
      sm_inv[row] = rsqrtf(var + eps);
    }
  }
  __syncthreads();

  typename Mfma16x16x32<_Float16>::accv acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = {0, 0, 0, 0};

  const int ktiles = K / 64;
  // Register-prefetch pipeline (the attention kernel's proven pattern):
  // A and B tiles are prefetched into REGISTERS (not glds), so
  // __syncthreads() between ds_writes and the MFMAs only waits lgkmcnt —
  // the next tile's global loads stay in flight under the compute, and
  // the ds_writes' register dependencies are the only load waits.
  _Float16 a_reg[2][8];
  _Float16 b_reg[2][8];
  auto prefetch = [&](int t) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int idx = c * 256 + tid;      // 0..511
      int row = idx >> 3;           // 0..63
      int cb = (idx & 7) * 16;
      int kk = t * 64 + cb / 2;
      int ar = row < M ? row : M - 1;
      load8(ar, kk, a_reg[c]);
      int br = n0 + row;
      if (br >= N) br = N - 1;
      *(half8v*)b_reg[c] = *(const half8v*)(Bw + (int64_t)br * K + kk);
    }
  };
  auto stage_regs = [&](char* abase) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int idx = c * 256 + tid;
      int row = idx >> 3;
      int cb = (idx & 7) * 16;
      float mean = sm_mean[row < M ? row : M - 1];
      float inv = sm_inv[row < M ? row : M - 1];
      _Float16 o8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int kg = cur_kbase + cb / 2 + j;
        o8[j] = (_Float16)(((float)a_reg[c][j] - mean) * inv * sm_gamma[kg] +
                           sm_beta[kg]);
      }
      *(short8v*)(abase + row * 128 + (cb ^ ((row & 7) << 4))) =
          *(const short8v*)o8;
      *(short8v*)(abase + kABytes + row * 128 + (cb ^ ((row & 7) << 4))) =
          *(const short8v*)b_reg[c];
    }
  };

  char* abase = smem;  // single slot: barrier-write-barrier-compute
  cur_kbase = 0;
  prefetch(0);
  for (int t = 0; t < ktiles; ++t) {
    __syncthreads();   // prior tile's LDS reads complete before overwrite
    cur_kbase = t * 64;
    stage_regs(abase);             // waits only the prefetched registers
    if (t + 1 < ktiles) prefetch(t + 1);  // overlaps the MFMAs below
    __syncthreads();               // ds_writes visible (lgkmcnt)
    mfma_tile<_Float16, BM, BN>(abase, abase + kABytes, lane, wr, wc, acc);
  }

  // ---- epilogue: bias (+gelu) (+K/V scatter) ----
  const int hid = (EPI == 2) ? N / 3 : 0;  // qkv gemm: N = 3*H*64
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int col = n0 + wc * 32 + j * 16 + (lane & 15);
      if (col >= N) continue;
      float bi = bias ? bias[col] : 0.0f;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        int row = wr * 32 + i * 16 + ((lane >> 4) << 2) + rr;
        if (row >= M) continue;
        float v = (float)acc[i][j][rr] + bi;
        if (EPI == 1) v = gelu_tanh(v);
        _Float16 hv = (_Float16)v;
        C[(int64_t)row * N + col] = hv;
        if (EPI == 2) {
          int p = pos[row];
          if (p >= 0 && col >= hid) {  // K or V column range
            if (p >= smax) p = smax - 1;
            int rel = col - hid;
            bool is_v = rel >= hid;
            if (is_v) rel -= hid;
            int h_idx = rel >> 6, d = rel & 63;
            _Float16* cache = is_v ? vcache : kcache;
            cache[(((int64_t)row * heads + h_idx) * smax + p) * 64 + d] = hv;
          }
        }
      }
    }
  }
}

void launch_decode_gemm_fused(int pro, int epi, const void* x, const void* r,
                              void* h_out, const float* gamma,
                              const float* beta, const void* Bw,
                              const float* bias, void* C, const void* ids,
                              const void* tok, const void* posemb,
                              const void* pos, void* kcache, void* vcache,
                              int M, int N, int K, int heads, int smax,
                              float eps, hipStream_t stream) {
  if (M > 64) throw std::runtime_error("decode_gemm_fused: M > 64");
  if (K % 64 != 0) throw std::runtime_error("decode_gemm_fused: K % 64");
  if (K > 2048) throw std::runtime_error("decode_gemm_fused: K > 2048");
  dim3 grid((unsigned)cdiv(N, 64));
  dim3 block(256);
  auto L = [&](auto pro_c, auto epi_c) {
    hipLaunchKernelGGL(
        (decode_gemm_fused_kernel<decltype(pro_c)::value,
                                  decltype(epi_c)::value>),
        grid, block, 0, stream, (const _Float16*)x, (const _Float16*)r,
        (_Float16*)h_out, gamma, beta, (const _Float16*)Bw, bias,
        (_Float16*)C, (const int*)ids, (const _Float16*)tok,
        (const _Float16*)posemb, (const int*)pos, (_Float16*)kcache,
        (_Float16*)vcache, M, N, K, heads, smax, eps);
  };
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  using E0 = std::integral_constant<int, 0>;
  using E1 = std::integral_constant<int, 1>;
  using E2 = std::integral_constant<int, 2>;
  if (pro == 1 && epi == 0) L(I1{}, E0{});
  else if (pro == 1 && epi == 1) L(I1{}, E1{});
  else if (pro == 1 && epi == 2) L(I1{}, E2{});
  else if (pro == 2 && epi == 0) L(I2{}, E0{});
  else if (pro == 2 && epi == 1) L(I2{}, E1{});
  else if (pro == 2 && epi == 2) L(I2{}, E2{});
  else if (pro == 3 && epi == 2) L(I3{}, E2{});
  else if (pro == 3 && epi == 0) L(I3{}, E0{});
  else throw std::runtime_error("decode_gemm_fused: bad pro/epi combo");
}

}  // namespace trtlab
