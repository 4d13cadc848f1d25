// The k likeliest tokens of a bf16 logits row as log-probabilities: ids[r, j] / logp[r, j], j = 0 .. k-1 (k <= TOPK_MAX), a sibling launch
// of llx_logprob_rows_fwd (scoring) and of the sampler (generation) that leaves both untouched.
//
// Order.  Descending by value, equal values by ascending index - the tie rule of top1 (logprob.hip) and of the greedy sampler.  -0.0
// equals +0.0 (as the float compare of top1 has it).  -inf entries rank last, among themselves by index.  A NaN never wins over a
// number: it ranks as -inf does (a NaN and a -inf tie, by index), so ids[r, 0] is what llx_logprob_rows_fwd writes to top1 on every
// row, a row without any finite entry included (index 0 there).  The logp of a selected NaN entry is NaN, of a -inf entry -inf.
//
// Selection: ONE read of the row.  Every element becomes a key whose unsigned order is the rank order, ties included: the
// order-preserving 16-bit image of the bf16 value in the high bits, the complement of its place in the low ones.  Inside a thread the
// place is the running element count of the thread (16 bits: its chunks ascend, so that is index order; V <= 2^25), the key 32 bits,
// and the thread keeps its TOPK_MAX largest in a sorted register list by a branch-free insertion, one v_max_u32 / v_min_u32 pair per
// list slot (at 31 chunks a thread nearly every chunk holds a new entry for some lane of the wave, so a cheap insertion pays, a skip
// does not; a chunk whose float maximum does not exceed the 8th best of any lane is still skipped after 8 compares).  For the merges
// the place becomes the row index (64-bit keys): each wave extracts the 8 largest of its 64 lists by 8 rounds of (wave max of the
// list heads, the owner pops); wave 0 does the same over the 8 x 8 keys of the waves.  No atomics, one fixed order: repeat launches
// are bit-identical.
//
// lse: given (fp32 [R], the scoring head has it from llx_logprob_rows_fwd) logp = x - lse[r] in fp32.  Null (generation): the kernel
// forms it in the same read, logp = (x - max) - log(sum) as llx_logprob_rows_fwd has it, by the arithmetic of row_lse_pass (rowlse.h)
// in its order - the same bits wherever that pass yields a number - with one guard that pass lacks: while a thread's running maximum
// is still -inf, a chunk of -inf adds 0 (row_lse_pass forms exp(-inf - -inf) = NaN there, which poisons every row that holds a whole
// chunk of -inf in front of a thread's first number: a masked vocabulary, a row with fewer than k finite entries).  A NaN in the row
// still makes its lse NaN.  label_logp (nullable, scoring with lse): the alternative that is the row's label gets label_logp[r], the
// value llx_logprob_rows_fwd computed as (x - max) - log(sum), which x - lse[r] matches only to the rounding of lse.
#include "common.h"

#define TOPK_THREADS 512
#define TOPK_MAX 8
#define TOPK_WAVES (TOPK_THREADS / LLX_WAVE)

typedef unsigned long long topk_key_t;

// bf16 bits -> 16-bit image whose unsigned order is the rank order above (NaN -> the image of -inf, -0.0 -> that of +0.0)
__device__ __forceinline__ uint32_t topk_ord(uint32_t b) {
  if ((b & 0x7fffu) > 0x7f80u) b = 0xff80u;
  if (b == 0x8000u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float topk_ord_value(uint32_t o) {  // the float of an image (NaN comes back as -inf: callers read x itself)
  const uint32_t b = (o & 0x8000u) ? (o & 0x7fffu) : (~o & 0xffffu);
  return __uint_as_float(b << 16);
}

// key into the descending list l, its smallest entry dropped: branch-free, a no-op for a key below l[TOPK_MAX - 1]
__device__ __forceinline__ void topk_insert(uint32_t (&l)[TOPK_MAX], uint32_t key) {
  l[TOPK_MAX - 1] = max(l[TOPK_MAX - 1], key);
#pragma unroll
  for (int i = TOPK_MAX - 1; i > 0; --i) {
    const uint32_t a = l[i - 1], b = l[i];
    l[i - 1] = max(a, b);
    l[i] = min(a, b);
  }
}

__device__ __forceinline__ topk_key_t topk_wave_max(topk_key_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const topk_key_t u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// The TOPK_MAX largest keys over the sorted lists of a wave's lanes, descending, in every lane.  Keys are unique (or 0 = empty).
__device__ __forceinline__ void topk_wave_extract(topk_key_t (&l)[TOPK_MAX], topk_key_t (&out)[TOPK_MAX]) {
#pragma unroll
  for (int j = 0; j < TOPK_MAX; ++j) {
    const topk_key_t m = topk_wave_max(l[0]);
    out[j] = m;
    if (l[0] == m && m != 0) {
#pragma unroll
      for (int i = 0; i < TOPK_MAX - 1; ++i) l[i] = l[i + 1];
      l[TOPK_MAX - 1] = 0;
    }
  }
}

// One block per row.  Scoring (labels != null): rows with label -100 and rows at or past rows_dyn[0] rounded up to 256 are not read
// and get ids = -1, logp = 0; the results go to ids / logp + r * ld_out.  Generation (pos != null): row r writes at column
// h = pos[r] - hist_base of its [hist_cap, k] block when 0 <= h < hist_cap and finished[r] is not set, nothing otherwise; pos and
// finished are only read.  Neither: every row is ranked and written at r * ld_out.
template <bool OWN_LSE>
__global__ __launch_bounds__(TOPK_THREADS) void topk_logprobs_row_kernel(const bf16_t* __restrict__ logits, int64_t ld, int V, int k,
                                                                          const float* __restrict__ lse_in, const float* __restrict__ label_logp,
                                                                          const int64_t* __restrict__ labels, const int32_t* __restrict__ rows_dyn,
                                                                          const int64_t* __restrict__ pos, int64_t hist_base,
                                                                          const int32_t* __restrict__ finished, int32_t* __restrict__ ids,
                                                                          float* __restrict__ logp, int64_t ld_out, int64_t hist_cap) {
  __shared__ float red[16];
  __shared__ topk_key_t wtop[TOPK_WAVES * TOPK_MAX];
  const int64_t r = blockIdx.x;
  int64_t o = r * ld_out;
  int64_t label = -1;
  if (labels != nullptr) {
    const bool past = rows_dyn != nullptr && r >= ((rows_dyn[0] + 255) & ~255);
    if (!past) label = labels[r];
    if (past || label == -100) {
      if (threadIdx.x < k) {
        ids[o + threadIdx.x] = -1;
        logp[o + threadIdx.x] = 0.f;
      }
      return;
    }
  } else if (pos != nullptr) {
    if (finished != nullptr && finished[r]) return;
    const int64_t h = pos[r] - hist_base;
    if (h < 0 || h >= hist_cap) return;
    o += h * k;
  }
  const bf16_t* x = logits + r * ld;
  const int nchunk = V >> 3;

  // this thread's TOPK_MAX best keys (image << 16 | 0xffff - running element count), descending; 0 = empty: an image is >= 0x7f
  uint32_t t32[TOPK_MAX];
#pragma unroll
  for (int i = 0; i < TOPK_MAX; ++i) t32[i] = 0;
  float thr = -INFINITY;  // the value of l[TOPK_MAX - 1] once the list is full
  bool full = false;
  float m = -INFINITY, s = 0.f;  // OWN_LSE: the thread's running maximum and sum exp(x - m), as RowLse
  uint32_t sq = 0xffffu;  // 0xffff - the count of the chunk's first element (V <= 2^25: at most 8192 chunks a thread)
  for (int c = threadIdx.x; c < nchunk; c += TOPK_THREADS, sq -= 8) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(x + c * 8);
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[2 * e] = bflo(v[e]); f[2 * e + 1] = bfhi(v[e]); }
    float cm = f[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) cm = fmaxf(cm, f[e]);
    if constexpr (OWN_LSE) {
      const float mn = fmaxf(m, cm);
      float add = 0.f;
      if (mn == -INFINITY) {  // nothing but -inf (or NaN) so far: the chunk adds 0, a NaN in it itself
        float t = f[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) t += f[e];
        add = t != t ? t : 0.f;
        s += add;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) add += __expf(f[e] - mn);
        s = s * __expf(m - mn) + add;
      }
      m = mn;
    }
    // a thread's chunks ascend, so a value equal to its 8th best loses the tie: strictly larger, or the list still has room
    if (full && !(cm > thr)) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      topk_insert(t32, (topk_ord(v[e] & 0xffffu) << 16) | (sq - 2 * e));
      topk_insert(t32, (topk_ord(v[e] >> 16) << 16) | (sq - 2 * e - 1));
    }
    full = t32[TOPK_MAX - 1] != 0;
    thr = full ? topk_ord_value(t32[TOPK_MAX - 1] >> 16) : -INFINITY;
  }
  // the merges rank across threads: the place becomes the row index, index = (thread + 512 (count / 8)) 8 + count % 8
  topk_key_t l[TOPK_MAX];
#pragma unroll
  for (int i = 0; i < TOPK_MAX; ++i) {
    const uint32_t n = 0xffffu - (t32[i] & 0xffffu);
    const uint32_t idx = ((threadIdx.x + (n >> 3) * TOPK_THREADS) << 3) + (n & 7u);
    l[i] = t32[i] == 0 ? 0 : ((topk_key_t)(t32[i] >> 16) << 32) | (0xffffffffu - idx);
  }

  float gm = 0.f, ls = 0.f;
  if constexpr (OWN_LSE) {
    gm = block_max(m, red);
    ls = __logf(block_sum(m == -INFINITY ? s : s * __expf(m - gm), red));  // (a thread without a number: s is 0, or the NaN it saw)
  }

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  topk_key_t best[TOPK_MAX];
  topk_wave_extract(l, best);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < TOPK_MAX; ++j) wtop[w * TOPK_MAX + j] = best[j];
  }
  __syncthreads();
  if (w != 0) return;
#pragma unroll
  for (int i = 1; i < TOPK_MAX; ++i) l[i] = 0;
  l[0] = wtop[lane];  // TOPK_WAVES * TOPK_MAX == 64 candidates, one per lane
  topk_wave_extract(l, best);
  topk_key_t mine = 0;
#pragma unroll
  for (int j = 0; j < TOPK_MAX; ++j) mine = lane == j ? best[j] : mine;
  if (lane < k) {  // V >= 8 >= k: the k best are elements of the row (the guard keeps an empty key, which cannot occur, inside it)
    const int id = mine != 0 ? (int)(0xffffffffu - (uint32_t)mine) : 0;
    const float xv = bf2f(x[id]);
    float lp;
    if constexpr (!OWN_LSE) {
      lp = xv - lse_in[r];
      if (label_logp != nullptr && (int64_t)id == label) lp = label_logp[r];
    } else {
      lp = (xv - gm) - ls;
    }
    ids[o + lane] = id;
    logp[o + lane] = lp;
  }
}

// dst[i, :] = map[i] >= 0 ? src[map[i], :] : (-1, 0.0): the [T, k] results of the compacted rows back to their positions.
__global__ __launch_bounds__(256) void topk_map_rows_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ src_ids,
                                                             const float* __restrict__ src_logp, int32_t* __restrict__ dst_ids,
                                                             float* __restrict__ dst_logp, int T, int k) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)T * k) return;
  const int i = (int)(e / k), j = (int)(e % k);
  const int s = map[i];
  const bool ok = s >= 0 && s < T;
  dst_ids[e] = ok ? src_ids[(int64_t)s * k + j] : -1;
  dst_logp[e] = ok ? src_logp[(int64_t)s * k + j] : 0.f;
}

static_assert(TOPK_WAVES * TOPK_MAX == LLX_WAVE, "the block merge gives every lane of wave 0 one candidate");

extern "C" int llx_topk_logprobs_rows(const void* logits, int64_t ld, int64_t R, int64_t V, int k, const float* lse, const float* label_logp,
                                      const int64_t* labels, const int32_t* rows, const int64_t* pos, int64_t hist_base, const int32_t* finished,
                                      int32_t* ids, float* logp, int64_t ld_out, int64_t hist_cap, hipStream_t stream) {
  const char* name = "llx_topk_logprobs_rows";
  LLX_REQUIRE(logits && ids && logp, "%s: null pointer (logits, ids and logp are required)", name);
  LLX_REQUIRE(k >= 1 && k <= TOPK_MAX, "%s: k = %d outside 1..%d", name, k, TOPK_MAX);
  LLX_REQUIRE(V % 8 == 0 && ld % 8 == 0, "%s: V and the row stride must be multiples of 8", name);
  LLX_REQUIRE(R > 0 && R < (1ll << 31) && V > 0 && V <= (1 << 25) && ld >= V, "%s: bad sizes (V <= 2^25)", name);
  LLX_REQUIRE((uintptr_t)logits % 16 == 0, "%s: logits must be 16-byte aligned", name);
  LLX_REQUIRE(((uintptr_t)ids | (uintptr_t)logp | (uintptr_t)lse | (uintptr_t)label_logp | (uintptr_t)rows | (uintptr_t)finished) % 4 == 0,
              "%s: ids, logp, lse, label_logp, rows and finished must be aligned to 4 bytes", name);
  LLX_REQUIRE(((uintptr_t)labels | (uintptr_t)pos) % 8 == 0, "%s: labels and pos must be aligned to 8 bytes", name);
  LLX_REQUIRE(!(labels && pos), "%s: labels (scoring) and pos (generation) exclude each other", name);
  LLX_REQUIRE(!rows || labels, "%s: rows goes with labels", name);
  LLX_REQUIRE(!label_logp || (labels && lse), "%s: label_logp goes with labels and lse", name);
  LLX_REQUIRE(!finished || pos, "%s: finished goes with pos", name);
  if (pos) {
    LLX_REQUIRE(hist_cap > 0 && hist_cap < (1ll << 31) && ld_out >= hist_cap * k, "%s: generation needs hist_cap > 0 and ld_out >= hist_cap * k", name);
  } else {
    LLX_REQUIRE(ld_out >= k, "%s: ld_out must be at least k", name);
  }
  if (lse)
    hipLaunchKernelGGL(topk_logprobs_row_kernel<false>, dim3((unsigned)R), dim3(TOPK_THREADS), 0, stream, (const bf16_t*)logits, ld, (int)V, k, lse,
                       label_logp, labels, rows, pos, hist_base, finished, ids, logp, ld_out, hist_cap);
  else
    hipLaunchKernelGGL(topk_logprobs_row_kernel<true>, dim3((unsigned)R), dim3(TOPK_THREADS), 0, stream, (const bf16_t*)logits, ld, (int)V, k, lse,
                       label_logp, labels, rows, pos, hist_base, finished, ids, logp, ld_out, hist_cap);
  LLX_LAUNCH_CHECK(name);
  return LLX_OK;
}

extern "C" int llx_topk_map_rows(const int32_t* map, const int32_t* src_ids, const float* src_logp, int32_t* dst_ids, float* dst_logp, int64_t T,
                                 int k, hipStream_t stream) {
  const char* name = "llx_topk_map_rows";
  LLX_REQUIRE(map && src_ids && src_logp && dst_ids && dst_logp, "%s: null pointer", name);
  LLX_REQUIRE(k >= 1 && k <= TOPK_MAX, "%s: k = %d outside 1..%d", name, k, TOPK_MAX);
  LLX_REQUIRE(T > 0 && T < (1 << 28), "%s: bad T", name);
  LLX_REQUIRE(src_ids != dst_ids && src_logp != dst_logp, "%s: source and destination must differ", name);
  hipLaunchKernelGGL(topk_map_rows_kernel, dim3((unsigned)((T * k + 255) / 256)), dim3(256), 0, stream, map, src_ids, src_logp, dst_ids, dst_logp, (int)T,
                     k);
  LLX_LAUNCH_CHECK(name);
  return LLX_OK;
}
