// Beam search for generate(num_beams=W) (llx/generate.py): what a step needs besides the model call, on the device, so that no step reads
// the host.  The rule is llx.sampling.beam_shortlist / beam_step (the host reference the tests compare these kernels with):
//
//   llx_beam_rows        one workgroup per logits row: zmax, the sum of exp(z - zmax) and the row's W + 1 best tokens by (logit
//                        descending, index ascending) -> cand_score (the log-probabilities) and cand_token [W][W + 1].  The sum is over the
//                        sampler's integer weights floor(expf(z - zmax) * 2^40) in uint64, so it does not depend on any order; the shortlist
//                        is W + 1 block-argmax passes over the (L2-resident) row, each taking the largest key strictly below the last one.
//   llx_beam_merge       one workgroup: orders the W * (W + 1) candidates by (s[r] + logp descending, row, rank), walks them - an eos_id is
//                        offered to the bank of finished hypotheses, anything else becomes the next live beam, until W are live - and does
//                        the bookkeeping: parent, the next step's tokens, s, the token histories (permuted by parent, then appended to),
//                        the bank and the done flag.  A launch that finds done set writes identity parents and nothing else.
//   llx_kv_reorder_rows  cache[b, :, :len] <- cache[parent[b], :, :len] in place for every layer's k and v cache in one launch.
//
// No floating-point atomics anywhere; the state is written with plain vector stores, each address by one thread only.
#include "common.h"
#include "rowview.h"

#define BMR_THREADS 1024
#define BMR_WAVES (BMR_THREADS / 64)
#define BM_MAX_W 16
#define BM_MAX_C (BM_MAX_W * (BM_MAX_W + 1))
#define BM_WSCALE 1099511627776.0f  // 2^40
#define BMG_THREADS 256
#define KVR_THREADS 256
#define BM_DEAD -1.0e30f  // llx.sampling.BEAM_DEAD

namespace {

__device__ __forceinline__ unsigned long long bm_shfl_xor(unsigned long long v, int o) {
  const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

struct BeamRowsArgs {
  const void* logits;
  int64_t ld;
  int V, W;
  float* cand_score;
  int32_t* cand_token;
};

// key of element i with logit z: larger = better; among equal logits the lower index wins.  Every element's key is > 0.
__device__ __forceinline__ unsigned long long bm_key(float z, int i) {
  return ((unsigned long long)smp_key(z) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
}

template <typename T>
__global__ __launch_bounds__(BMR_THREADS) void beam_rows_kernel(BeamRowsArgs a) {
  constexpr int E = RowView<T>::E;
  __shared__ unsigned long long red[2][BMR_WAVES];
  __shared__ unsigned long long red_sum[BMR_WAVES];
  __shared__ unsigned long long top[BM_MAX_W + 1];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const RowView<T> row((const T*)a.logits + (int64_t)r * a.ld, a.V);

  // ---- the W + 1 best keys, one pass each: the largest key strictly below the previous one (V >= W + 1: every pass finds one)
  unsigned long long prev = ~0ull, first = 0;
#pragma unroll 1
  for (int k = 0; k <= a.W; ++k) {
    unsigned long long best = 0;
    for (int c = tid; c < row.nchunks; c += BMR_THREADS) {
      float v[E];
      const uint32_t m = row.load(c, v);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned long long key = bm_key(v[e], c * E - row.off + e);
        if (((m >> e) & 1) && key < prev) best = max(best, key);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, bm_shfl_xor(best, o));
    if (lane == 0) red[k & 1][wv] = best;
    __syncthreads();  // (the buffer written two passes ago has been read by everyone: they passed the barrier in between)
#pragma unroll
    for (int i = 0; i < BMR_WAVES; ++i) best = max(best, red[k & 1][i]);
    prev = best;
    if (k == 0) first = best;
    if (tid == 0) top[k] = best;
  }

  // ---- sum of the integer weights
  const float zm = smp_unkey((uint32_t)(first >> 32));
  unsigned long long sum = 0;
  for (int c = tid; c < row.nchunks; c += BMR_THREADS) {
    float v[E];
    const uint32_t m = row.load(c, v);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float w = (v[e] == zm) ? 1.f : expf(v[e] - zm);
      if ((m >> e) & 1) sum += (unsigned long long)(w * BM_WSCALE);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += bm_shfl_xor(sum, o);
  if (lane == 0) red_sum[wv] = sum;
  __syncthreads();  // (also orders thread 0's top[] stores before the reads below)
  if (tid <= a.W) {
    unsigned long long total = 0;
#pragma unroll
    for (int i = 0; i < BMR_WAVES; ++i) total += red_sum[i];
    const float lse = (float)log((double)total * 9.094947017729282e-13);  // 2^-40
    const unsigned long long key = top[tid];
    const float z = smp_unkey((uint32_t)(key >> 32));
    const int64_t o = (int64_t)r * (a.W + 1) + tid;
    a.cand_score[o] = ((z == zm) ? 0.f : z - zm) - lse;
    a.cand_token[o] = (int32_t)(0xffffffffu - (uint32_t)key);
  }
}

struct BeamMergeArgs {
  const float* cand_score;
  const int32_t* cand_token;
  float* s;
  int32_t* parent;
  int64_t* tok;
  int64_t* hist;
  int64_t hist_ld;
  int64_t* bank_tok;
  int64_t bank_ld;
  int32_t* bank_len;
  float* bank_score;
  int32_t* meta;  // count, done, steps
  int W;
  int64_t n, eos_id;
  float length_penalty;
  int init;
};

struct BmShared {
  float raw[BM_MAX_C];
  int order[BM_MAX_C];
  float s[BM_MAX_W];
  int parent[BM_MAX_W], tok[BM_MAX_W];
  float bank[BM_MAX_W];
  int ev_slot[2 * BM_MAX_W], ev_src[2 * BM_MAX_W];
  float ev_score[2 * BM_MAX_W];
  int n_eos, n_ev, count, done;
};

// the bank takes a hypothesis of final score f: the slot it gets, or -1.  Room first; else the worst entry (lowest score, lowest slot
// among equals) if f beats it.
__device__ __forceinline__ int bm_offer(BmShared& sh, int W, float f) {
  int slot;
  if (sh.count < W) {
    slot = sh.count++;
  } else {
    slot = 0;
    for (int i = 1; i < W; ++i)
      if (sh.bank[i] < sh.bank[slot]) slot = i;
    if (!(f > sh.bank[slot])) return -1;
  }
  sh.bank[slot] = f;
  return slot;
}

__global__ __launch_bounds__(BMG_THREADS) void beam_merge_kernel(BeamMergeArgs a) {
  __shared__ BmShared sh;
  const int tid = threadIdx.x, W = a.W, C = W + 1;
  const int steps0 = a.init ? 0 : a.meta[2];
  if ((!a.init && a.meta[1]) || steps0 < 0 || steps0 >= a.n) {  // frozen (uniform: every thread reads the same words)
    if (tid < W) a.parent[tid] = tid;
    return;
  }
  const int N = (a.init ? 1 : W) * C;  // before the first step only row 0 takes part
  for (int i = tid; i < N; i += BMG_THREADS) {
    const float sc = (a.init ? 0.f : a.s[i / C]) + a.cand_score[i];
    sh.raw[i] = (sc != sc) ? -INFINITY : sc;
  }
  __syncthreads();
  // candidate i = r * C + k: its place in the order (score descending, then i ascending = row, then rank in the row's shortlist)
  for (int i = tid; i < N; i += BMG_THREADS) {
    const float x = sh.raw[i];
    int rank = 0;
    for (int j = 0; j < N; ++j) rank += (sh.raw[j] > x || (sh.raw[j] == x && j < i)) ? 1 : 0;
    sh.order[rank] = i;
  }
  __syncthreads();

  const int len = steps0 + 1;  // tokens of every hypothesis this step ends or extends (an eos counted)
  if (tid == 0) {
    sh.count = a.init ? 0 : min(max(a.meta[0], 0), W);
    for (int i = 0; i < sh.count; ++i) sh.bank[i] = a.bank_score[i];
    const float norm = powf((float)len, a.length_penalty);
    int live = 0, ev = 0;
    for (int q = 0; q < N && live < W; ++q) {
      const int i = sh.order[q], r = i / C, t = a.cand_token[i];
      const float sc = sh.raw[i];
      if (a.eos_id >= 0 && (int64_t)t == a.eos_id) {
        const float f = sc / norm;
        const int slot = bm_offer(sh, W, f);
        if (slot >= 0) { sh.ev_slot[ev] = slot; sh.ev_src[ev] = r; sh.ev_score[ev] = f; ++ev; }
      } else {
        sh.parent[live] = r; sh.tok[live] = t; sh.s[live] = sc;
        ++live;
      }
    }
    for (; live < W; ++live) { sh.parent[live] = 0; sh.tok[live] = 0; sh.s[live] = BM_DEAD; }  // (V >= W + 1: not reached)
    sh.n_eos = ev;
    sh.done = (sh.count == W || len == a.n) ? 1 : 0;
    if (sh.done) {  // the live beams are offered as they are
      for (int j = 0; j < W; ++j) {
        const float f = sh.s[j] / norm;
        const int slot = bm_offer(sh, W, f);
        if (slot >= 0) { sh.ev_slot[ev] = slot; sh.ev_src[ev] = j; sh.ev_score[ev] = f; ++ev; }
      }
    }
    sh.n_ev = ev;
  }
  __syncthreads();

  // ---- tokens.  A thread owns column j of the histories and of the bank in every phase below, so the phases need no barrier: the
  // hypotheses that enter the bank, in the order of the walk, copy from the old histories - a finished one its row and the eos_id, a
  // live beam of a done state its parent's row and its new token - then the histories are permuted (all W read, then written) and
  // appended to.
  for (int j = tid; j < len; j += BMG_THREADS) {
    for (int e = 0; e < sh.n_eos; ++e)
      a.bank_tok[sh.ev_slot[e] * a.bank_ld + j] = (j < steps0) ? a.hist[sh.ev_src[e] * a.hist_ld + j] : a.eos_id;
    for (int e = sh.n_eos; e < sh.n_ev; ++e) {
      const int b = sh.ev_src[e];
      a.bank_tok[sh.ev_slot[e] * a.bank_ld + j] = (j < steps0) ? a.hist[sh.parent[b] * a.hist_ld + j] : (int64_t)sh.tok[b];
    }
    int64_t v[BM_MAX_W];
#pragma unroll
    for (int b = 0; b < BM_MAX_W; ++b)
      if (b < W) v[b] = (j < steps0) ? a.hist[sh.parent[b] * a.hist_ld + j] : (int64_t)sh.tok[b];
#pragma unroll
    for (int b = 0; b < BM_MAX_W; ++b)
      if (b < W) a.hist[b * a.hist_ld + j] = v[b];
  }
  if (tid != 0) return;
  for (int e = 0; e < sh.n_ev; ++e) {
    a.bank_len[sh.ev_slot[e]] = len;
    a.bank_score[sh.ev_slot[e]] = sh.ev_score[e];
  }
  for (int b = 0; b < W; ++b) {
    a.parent[b] = sh.parent[b];
    a.tok[b] = (int64_t)sh.tok[b];
    a.s[b] = sh.s[b];
  }
  a.meta[0] = sh.count;
  a.meta[1] = sh.done;
  a.meta[2] = len;
}

struct KvReorderArgs {
  bf16_t* const* table;
  int64_t sb, sh, ss;
  const int32_t* parent;
  int W, KVH;
  int64_t len;
};

// A thread owns one 16-byte chunk index (cache, head, position, chunk) for all W slots: it loads the chunks of the slots that move from
// their sources and then stores them; no other thread touches those addresses, so the permutation is safe in place.
__global__ __launch_bounds__(KVR_THREADS) void kv_reorder_rows_kernel(KvReorderArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * KVR_THREADS + threadIdx.x;
  if (idx >= (int64_t)a.KVH * a.len * (HD / 8)) return;
  const int64_t c = idx & (HD / 8 - 1), hp = idx / (HD / 8), p = hp % a.len, h = hp / a.len;
  bf16_t* base = a.table[blockIdx.y] + h * a.sh + p * a.ss + c * 8;
  u32x4_t v[BM_MAX_W];
  int src[BM_MAX_W];
#pragma unroll
  for (int b = 0; b < BM_MAX_W; ++b) {
    src[b] = b;
    if (b < a.W) {
      const int q = a.parent[b];
      if ((unsigned)q < (unsigned)a.W) src[b] = q;  // anything else is read as "stays"
      if (src[b] != b) v[b] = *reinterpret_cast<const u32x4_t*>(base + src[b] * a.sb);
    }
  }
#pragma unroll
  for (int b = 0; b < BM_MAX_W; ++b)
    if (b < a.W && src[b] != b) *reinterpret_cast<u32x4_t*>(base + b * a.sb) = v[b];
}

}  // namespace

// logits [W, V] (dtype 0 = bf16, 1 = fp32; row stride ld >= V elements, rows may start at any element) -> cand_score fp32 / cand_token
// int32 [W, W + 1]: the log-probabilities and indices of each row's W + 1 best tokens, best first.
extern "C" int llx_beam_rows(const void* logits, int dtype, int64_t ld, int64_t W, int64_t V, float* cand_score, int32_t* cand_token,
                             hipStream_t stream) {
  LLX_REQUIRE(logits && cand_score && cand_token, "llx_beam_rows: null pointer (logits, cand_score and cand_token are required)");
  LLX_REQUIRE(dtype == 0 || dtype == 1, "llx_beam_rows: dtype=%d (0 = bf16, 1 = fp32)", dtype);
  LLX_REQUIRE(W >= 2 && W <= BM_MAX_W, "llx_beam_rows: W=%lld beams outside 2..%d", (long long)W, BM_MAX_W);
  LLX_REQUIRE(V > W && V < (1ll << 30), "llx_beam_rows: V=%lld must be in [W + 1, 2^30) (a shortlist holds W + 1 tokens)", (long long)V);
  LLX_REQUIRE(ld >= V, "llx_beam_rows: row stride %lld < V=%lld", (long long)ld, (long long)V);
  LLX_REQUIRE((uintptr_t)logits % (dtype ? 4 : 2) == 0, "llx_beam_rows: logits not aligned to their element size");
  BeamRowsArgs a{logits, ld, (int)V, (int)W, cand_score, cand_token};
  if (dtype == 0)
    hipLaunchKernelGGL(beam_rows_kernel<bf16_t>, dim3((unsigned)W), dim3(BMR_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(beam_rows_kernel<float>, dim3((unsigned)W), dim3(BMR_THREADS), 0, stream, a);
  LLX_LAUNCH_CHECK("llx_beam_rows");
  return LLX_OK;
}

// cand_score / cand_token [W, W + 1] of llx_beam_rows; s fp32 [W]; parent int32 [W]; tok int64 [W]; hist int64 [W, n] (row stride
// hist_ld); bank_tok int64 [W, n] (row stride bank_ld), bank_len int32 [W], bank_score fp32 [W]; meta int32 [3] = (hypotheses in the
// bank, done, tokens generated).  init != 0: the first step after the prefill - the state is not read, only row 0 takes part.
extern "C" int llx_beam_merge(const float* cand_score, const int32_t* cand_token, float* s, int32_t* parent, int64_t* tok, int64_t* hist,
                              int64_t hist_ld, int64_t* bank_tok, int64_t bank_ld, int32_t* bank_len, float* bank_score, int32_t* meta,
                              int64_t W, int64_t n, int64_t eos_id, float length_penalty, int init, hipStream_t stream) {
  LLX_REQUIRE(cand_score && cand_token && s && parent && tok && hist && bank_tok && bank_len && bank_score && meta,
              "llx_beam_merge: null pointer (every array is required)");
  LLX_REQUIRE(W >= 2 && W <= BM_MAX_W, "llx_beam_merge: W=%lld beams outside 2..%d", (long long)W, BM_MAX_W);
  LLX_REQUIRE(n >= 1 && n < (1ll << 31), "llx_beam_merge: n=%lld new tokens must be in [1, 2^31)", (long long)n);
  LLX_REQUIRE(hist_ld >= n && bank_ld >= n, "llx_beam_merge: row strides hist_ld=%lld, bank_ld=%lld must be >= n=%lld", (long long)hist_ld,
              (long long)bank_ld, (long long)n);
  LLX_REQUIRE(eos_id >= -1 && eos_id < (1ll << 31), "llx_beam_merge: eos_id=%lld must be a token id or -1 (none)", (long long)eos_id);
  LLX_REQUIRE(length_penalty == length_penalty && length_penalty - length_penalty == 0.f, "llx_beam_merge: length_penalty=%g must be finite",
              (double)length_penalty);
  BeamMergeArgs a{cand_score, cand_token, s, parent, tok, hist, hist_ld, bank_tok, bank_ld, bank_len, bank_score, meta, (int)W, n, eos_id,
                  length_penalty, init ? 1 : 0};
  hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(BMG_THREADS), 0, stream, a);
  LLX_LAUNCH_CHECK("llx_beam_merge");
  return LLX_OK;
}

// table: DEVICE array of n_caches base pointers of bf16 caches [>= W, KVH, Smax, 128] with the common element strides sb, sh, ss (last
// dim dense); parent: DEVICE int32 [W].  cache[b, :, :len] <- cache[parent[b], :, :len] for b < W in every cache; slots with
// parent[b] == b, positions >= len and slots >= W are not written.
extern "C" int llx_kv_reorder_rows(const void* const* table, int64_t n_caches, int64_t sb, int64_t sh, int64_t ss, const int32_t* parent,
                                   int64_t W, int64_t KVH, int64_t len, int64_t Smax, int64_t head_dim, hipStream_t stream) {
  LLX_REQUIRE(table && (uintptr_t)table % 8 == 0, "llx_kv_reorder_rows: the pointer table is null or not aligned to 8 bytes");
  LLX_REQUIRE(parent, "llx_kv_reorder_rows: null pointer (parent)");
  LLX_REQUIRE(n_caches >= 1 && n_caches <= 65535, "llx_kv_reorder_rows: n_caches=%lld outside 1..65535", (long long)n_caches);
  LLX_REQUIRE(W >= 2 && W <= BM_MAX_W, "llx_kv_reorder_rows: W=%lld slots outside 2..%d", (long long)W, BM_MAX_W);
  LLX_REQUIRE(head_dim == HD, "llx_kv_reorder_rows: head_dim=%lld (only %d)", (long long)head_dim, HD);
  LLX_REQUIRE(KVH >= 1 && Smax >= 1, "llx_kv_reorder_rows: KVH=%lld, Smax=%lld must be >= 1", (long long)KVH, (long long)Smax);
  LLX_REQUIRE(len >= 1 && len <= Smax, "llx_kv_reorder_rows: len=%lld outside [1, Smax=%lld]", (long long)len, (long long)Smax);
  LLX_REQUIRE(sb % 8 == 0 && sh % 8 == 0 && ss % 8 == 0 && ss >= HD && sb > 0 && sh > 0,
              "llx_kv_reorder_rows: strides (%lld, %lld, %lld) must be positive multiples of 8 elements, the position stride >= %d",
              (long long)sb, (long long)sh, (long long)ss, HD);
  const int64_t blocks = cdiv64(KVH * len * (HD / 8), KVR_THREADS);
  LLX_REQUIRE(blocks < (1ll << 31), "llx_kv_reorder_rows: KVH * len too large");
  KvReorderArgs a{(bf16_t* const*)table, sb, sh, ss, parent, (int)W, (int)KVH, len};
  hipLaunchKernelGGL(kv_reorder_rows_kernel, dim3((unsigned)blocks, (unsigned)n_caches), dim3(KVR_THREADS), 0, stream, a);
  LLX_LAUNCH_CHECK("llx_kv_reorder_rows");
  return LLX_OK;
}
