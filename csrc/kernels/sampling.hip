// trtlab_amd — device-side top-k / nucleus (top-p) sampling (gfx950).
//
// topk_topp_sample_rows_kernel: fp16 logits [M, V] -> one sampled token id
// per row, restricted to the top-k / top-p candidate set. One 256-thread
// workgroup per row, like argmax_rows / gumbel_argmax_rows.
//
// The candidate set is defined on VALUE CLASSES (equal logits form one
// class, -0 == +0): walking classes from the highest value down, the cut
// is the first class at which the cumulative token count reaches top_k or
// the cumulative probability reaches top_p, whichever comes first; the
// whole class at the cut is kept. That makes the kept set a function of
// the values alone (trtlab_amd/engine/sampling.py is the reference). With a
// filter active, -inf logits (weight 0) are left out of the classes.
//
// Selection is an exact two-pass radix select over the 16-bit
// order-preserving key of the fp16 logit (high byte, then low byte among
// the elements of the selected high byte). Each pass fills a 256-bin LDS
// histogram of token counts (u32) and of probability mass. Mass is
// FIXED-POINT: w = (u64)(exp((x - rowmax)/T) * 2^40), accumulated with
// 64-bit integer LDS atomics — integer addition is order-free, so the kept
// set, and with it the token, is bit-reproducible from run to run. No
// floating-point atomics anywhere. V * 2^40 is far inside 64 bits.
//
// The draw is Gumbel-argmax over the kept elements with the noise of
// gumbel_argmax_rows (sampling_common.h): a row with no filter active
// returns exactly what that kernel returns, and skips the histogram
// passes; a row with T <= 0 is a plain argmax. Both branches are uniform
// per workgroup. A filtered row is read four times (row max, two
// histograms, draw); re-reads hit L2 (a 32k row is 64 KB).
//
// Deviation from the sketch in the design: the exponential is __expf (the
// hardware exp2 path, relative error ~|z| * 2^-24), not libm expf; the
// tests' mass band is sized for it.
#include "../common.h"
#include "launchers.h"
#include "sampling_common.h"

namespace trtlab {

namespace {

constexpr uint32_t kKeyNegInf = 0x03ffu;  // row_key(0xfc00)

// fp16 bits -> 16-bit key whose unsigned order is the order of the values;
// -0 is canonicalised to +0 first so both share one class.
__device__ __forceinline__ uint32_t row_key(uint32_t h) {
  if (h == 0x8000u) h = 0u;
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}

__device__ __forceinline__ float key_value(uint32_t key) {
  uint16_t h = (uint16_t)((key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu));
  return (float)__builtin_bit_cast(_Float16, h);
}

// Calls f(c, fp16 bits) once for every column c of the row, 16 B per lane
// where possible. A row base is only 2-byte aligned when V is not a
// multiple of 8 (GPT-2's 50257) or x is an offset view, so the 16-byte
// body starts at the first aligned element of THIS row; head and tail are
// scalar loads.
template <typename F>
__device__ __forceinline__ void for_each_in_row(const _Float16* r, int V,
                                                int tid, F&& f) {
  const uint16_t* rb = (const uint16_t*)r;
  int head = (int)(((16u - (uint32_t)((uintptr_t)r & 15u)) & 15u) >> 1);
  if (head > V) head = V;
  if (tid < head) f(tid, (uint32_t)rb[tid]);
  const int nv8 = (V - head) >> 3;
  for (int i = tid; i < nv8; i += 256) {
    const int c0 = head + i * 8;
    uint4v q = *(const uint4v*)(rb + c0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f(c0 + 2 * j, q[j] & 0xffffu);
      f(c0 + 2 * j + 1, q[j] >> 16);
    }
  }
  for (int c = head + (nv8 << 3) + tid; c < V; c += 256)
    f(c, (uint32_t)rb[c]);
}

struct Cut {
  uint32_t bin;   // selected histogram bin
  uint32_t cnt;   // tokens in the bins ABOVE it (plus the base)
  uint64_t mass;  // mass in the bins above it (plus the base)
  uint32_t kept;  // tokens down to and including the bin
};

// Walks the 256-bin histogram from the top bin down (thread t owns bin
// 255 - t) and selects the first bin whose inclusive running count
// reaches k or whose inclusive running mass reaches target; when neither
// is reached the last non-empty bin is selected. base_* carry what lies
// above this histogram (pass 2). Running sums are monotone, so exactly one
// thread sees the condition flip and writes *cut. All 256 threads call.
__device__ __forceinline__ void select_bin(const uint32_t* hcnt,
                                           const uint64_t* hmass,
                                           uint32_t base_cnt,
                                           uint64_t base_mass, uint32_t k,
                                           uint64_t target, uint32_t* wcnt,
                                           uint64_t* wmass, Cut* cut) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t own_c = hcnt[255 - tid];
  const uint64_t own_m = hmass[255 - tid];
  uint32_t c = own_c;
  uint64_t m = own_m;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    uint32_t oc = __shfl_up(c, off, 64);
    uint64_t om = __shfl_up((unsigned long long)m, off, 64);
    if (lane >= off) {
      c += oc;
      m += om;
    }
  }
  if (lane == 63) {
    wcnt[wave] = c;
    wmass[wave] = m;
  }
  __syncthreads();
  uint32_t total = base_cnt;
  c += base_cnt;
  m += base_mass;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    total += wcnt[w];
    if (w < wave) {
      c += wcnt[w];
      m += wmass[w];
    }
  }
  const uint32_t ec = c - own_c;
  const uint64_t em = m - own_m;
  const bool hit = c >= k || m >= target || c == total;
  const bool hit_above = tid > 0 && (ec >= k || em >= target || ec == total);
  if (hit && !hit_above) {
    cut->bin = 255u - (uint32_t)tid;
    cut->cnt = ec;
    cut->mass = em;
    cut->kept = c;
  }
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(256) void topk_topp_sample_rows_kernel(
    const _Float16* __restrict__ x, int* __restrict__ out,
    const float* __restrict__ temps, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const int* __restrict__ seeds,
    const int* __restrict__ pos, int* __restrict__ kept,
    float* __restrict__ thr, int M, int V) {
  const int row = blockIdx.x;
  if (row >= M) return;
  const int tid = threadIdx.x;
  const _Float16* r = x + (int64_t)row * V;
  const float T = temps ? temps[row] : 0.0f;
  const float invT = (T > 0.0f) ? 1.0f / T : 0.0f;
  const int tk = top_k ? top_k[row] : 0;
  const float tp = top_p ? top_p[row] : 0.0f;
  const bool use_k = tk > 0 && tk < V;
  const bool use_p = tp > 0.0f && tp < 1.0f;
  const bool filtered = T > 0.0f && (use_k || use_p);
  const uint64_t key = gumbel_row_key(seeds, pos, row);

  __shared__ float wb[4];
  __shared__ int wi[4];
  __shared__ uint32_t hcnt[256];
  __shared__ uint64_t hmass[256];
  __shared__ uint32_t wcnt[4];
  __shared__ uint64_t wmass[4];
  __shared__ Cut cut;

  float best = -1e30f;
  int bi = 0x7fffffff;

  // rows without a filter: one read, exactly gumbel_argmax_rows
  if (!filtered) {
    for_each_in_row(r, V, tid, [&](int c, uint32_t h) {
      float v = (float)__builtin_bit_cast(_Float16, (uint16_t)h);
      if (T > 0.0f) v = gumbel_perturb(v, invT, key, c);
      argmax_take(v, c, best, bi);
    });
    block_argmax_256(best, bi, wb, wi);
    if (tid == 0) {
      out[row] = wi[0];
      // greedy keeps its one token; unfiltered sampling keeps the row
      if (kept) kept[row] = (T > 0.0f) ? V : 1;
      if (thr) thr[row] = (T > 0.0f) ? -INFINITY : wb[0];
    }
    return;
  }

  // read 1: row max
  hcnt[tid] = 0u;
  hmass[tid] = 0ull;
  float mx = -INFINITY;
  for_each_in_row(r, V, tid, [&](int, uint32_t h) {
    mx = fmaxf(mx, (float)__builtin_bit_cast(_Float16, (uint16_t)h));
  });
  block_argmax_256(mx, 0, wb, wi);
  __syncthreads();  // wb[0] final; also orders the histogram clear
  const float rowmax = wb[0];
  // (a row of -inf only is out of scope: its histograms stay empty and it
  // ends with the same out-of-range index the unfiltered kernels give)

  // read 2: histogram of the key's high byte (-inf left out)
  for_each_in_row(r, V, tid, [&](int, uint32_t h) {
    const uint32_t k16 = row_key(h);
    if (k16 == kKeyNegInf) return;
    const float v = (float)__builtin_bit_cast(_Float16, (uint16_t)h);
    const uint64_t w = (uint64_t)(__expf((v - rowmax) * invT) * 1099511627776.f);
    atomicAdd(&hcnt[k16 >> 8], 1u);
    atomicAdd((unsigned long long*)&hmass[k16 >> 8], (unsigned long long)w);
  });
  __syncthreads();
  // Z = total mass; target = ceil(top_p * Z) in integer mass units
  uint64_t zpart = hmass[tid];
#pragma unroll
  for (int off = 32; off; off >>= 1)
    zpart += __shfl_xor((unsigned long long)zpart, off, 64);
  if ((tid & 63) == 0) wmass[tid >> 6] = zpart;
  __syncthreads();
  const uint64_t Z = wmass[0] + wmass[1] + wmass[2] + wmass[3];
  __syncthreads();  // wmass is reused by select_bin
  const uint32_t kk = use_k ? (uint32_t)tk : 0xffffffffu;
  uint64_t target = ~0ull;
  if (use_p) {
    const double t = (double)tp * (double)Z;
    target = (uint64_t)t;
    if ((double)target < t) ++target;
  }
  select_bin(hcnt, hmass, 0u, 0ull, kk, target, wcnt, wmass, &cut);
  const uint32_t hi = cut.bin;
  const uint32_t base_c = cut.cnt;
  const uint64_t base_m = cut.mass;

  // read 3: histogram of the low byte among elements with that high byte
  hcnt[tid] = 0u;
  hmass[tid] = 0ull;
  __syncthreads();  // also: everyone has read cut before it is rewritten
  for_each_in_row(r, V, tid, [&](int, uint32_t h) {
    const uint32_t k16 = row_key(h);
    if ((k16 >> 8) != hi || k16 == kKeyNegInf) return;
    const float v = (float)__builtin_bit_cast(_Float16, (uint16_t)h);
    const uint64_t w = (uint64_t)(__expf((v - rowmax) * invT) * 1099511627776.f);
    atomicAdd(&hcnt[k16 & 0xffu], 1u);
    atomicAdd((unsigned long long*)&hmass[k16 & 0xffu], (unsigned long long)w);
  });
  __syncthreads();
  select_bin(hcnt, hmass, base_c, base_m, kk, target, wcnt, wmass, &cut);
  const uint32_t thr_key = (hi << 8) | cut.bin;
  const uint32_t nkept = cut.kept;

  // read 4: Gumbel-argmax over the kept set
  for_each_in_row(r, V, tid, [&](int c, uint32_t h) {
    if (row_key(h) < thr_key) return;
    float v = (float)__builtin_bit_cast(_Float16, (uint16_t)h);
    v = gumbel_perturb(v, invT, key, c);
    argmax_take(v, c, best, bi);
  });
  block_argmax_256(best, bi, wb, wi);
  if (tid == 0) {
    out[row] = wi[0];
    if (kept) kept[row] = (int)nkept;
    if (thr) thr[row] = key_value(thr_key);
  }
}

void launch_topk_topp_sample_rows(const void* x, void* out, const void* temps,
                                  const void* top_k, const void* top_p,
                                  const void* seeds, const void* pos,
                                  void* kept, void* thr, int M, int V,
                                  hipStream_t stream) {
  hipLaunchKernelGGL(topk_topp_sample_rows_kernel, dim3((unsigned)M),
                     dim3(256), 0, stream, (const _Float16*)x, (int*)out,
                     (const float*)temps, (const int*)top_k,
                     (const float*)top_p, (const int*)seeds, (const int*)pos,
                     (int*)kept, (float*)thr, M, V);
}

}  // namespace trtlab
