// Prompt-lookup drafting for greedy generate(draft_tokens=k) (llx/generate.py): the bookkeeping of one speculative step on the device,
// so that no step reads the host.  One workgroup, one launch per step.  What it does is llx.sampling.lookup_accept followed by
// llx.sampling.lookup_draft (the host reference the tests compare it with, integer for integer):
//
//   accept   a = the longest prefix of the fed draft that the model's own greedy picks confirm: step_tok[1 + i] == picks[i], i < a.
//            picks[0 .. a] are emitted, cut to the room that is left (P + n - len) and after the first eos_id (which sets finished).
//   append   the emitted tokens go to seq[len ..], len advances.
//   draft    over the candidates e = 1 .. len - 1 (the index that follows an earlier occurrence), m(e) = the number of tokens that match
//            backwards from e - 1 and from the tail, at most g and e.  The longest match wins, the most recent among equals: the maximum
//            of (m << 32 | e).  draft[i] = ext[e + i], ext = seq extended by the draft so far (a match that overlaps the tail continues
//            periodically); without a match the last token is repeated.
//   next     step_tok = [seq[len - 1], draft], step_pos = len - 1 .. len - 1 + k, counters += (1, emitted - 1).
//
// A launch that finds finished set or len == P + n touches nothing: the steps the host launches before its next look re-feed the same
// tokens at the same positions.  Every store is a plain vector store by thread 0.
#include "common.h"

#define LKP_THREADS 256
#define LKP_WAVES (LKP_THREADS / 64)
#define LKP_MAX_K 3
#define LKP_MAX_G 8

namespace {

struct LookupArgs {
  const int64_t* picks;
  int64_t* seq;
  int64_t* len;
  int64_t* step_tok;
  int64_t* step_pos;
  int32_t* finished;
  int64_t* counters;
  int64_t P, n, eos_id;
  int k, g, init;
};

__global__ __launch_bounds__(LKP_THREADS) void lookup_step_kernel(LookupArgs a) {
  __shared__ unsigned long long red[LKP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t L0 = *a.len, end = a.P + a.n;
  if (*a.finished || L0 < 1 || L0 >= end) return;  // frozen (uniform: every thread reads the same words)

  // ---- accept: every thread works out the same few numbers from the picks and the fed row
  int64_t pk[LKP_MAX_K + 1];
#pragma unroll
  for (int i = 0; i <= LKP_MAX_K; ++i) pk[i] = (i == 0 || (!a.init && i <= a.k)) ? a.picks[i] : -1;
  int acc = 0;
  if (!a.init) {
    bool run = true;
#pragma unroll
    for (int i = 0; i < LKP_MAX_K; ++i) {
      run = run && i < a.k && a.step_tok[1 + i] == pk[i];
      acc += run ? 1 : 0;
    }
  }
  int emit = (int)min((int64_t)(acc + 1), end - L0);
  int fin = 0;
  if (a.eos_id >= 0) {
#pragma unroll
    for (int i = LKP_MAX_K; i >= 0; --i)
      if (i < emit && pk[i] == a.eos_id) { emit = i + 1; fin = 1; }
  }
  const int64_t L = L0 + emit;  // <= P + n <= cap
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i <= LKP_MAX_K; ++i)
      if (i < emit) a.seq[L0 + i] = pk[i];
  }
  __syncthreads();  // the appended tokens are read below by every thread; step_tok has been read by all before thread 0 rewrites it

  // ---- draft: the best (match length, candidate) over e = 1 .. L - 1
  unsigned long long best = 0;
  for (int64_t e = 1 + tid; e < L; e += LKP_THREADS) {
    int m = 0;
    while (m < a.g && m < e && a.seq[e - 1 - m] == a.seq[L - 1 - m]) ++m;
    if (m > 0) best = max(best, ((unsigned long long)m << 32) | (unsigned long long)e);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)best, o, 64), hi = __shfl_xor((uint32_t)(best >> 32), o, 64);
    best = max(best, ((unsigned long long)hi << 32) | lo);
  }
  if (lane == 0) red[wv] = best;
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int i = 0; i < LKP_WAVES; ++i) best = max(best, red[i]);

  const int64_t last = a.seq[L - 1];
  const int64_t src = (int64_t)(best & 0xffffffffull);  // 0: no match
  int64_t d[LKP_MAX_K];
#pragma unroll
  for (int i = 0; i < LKP_MAX_K; ++i) {
    int64_t t = last;
    if (i < a.k && src > 0) {
      const int64_t at = src + i;  // < L + i
      if (at < L) t = a.seq[at];
#pragma unroll
      for (int j = 0; j < i; ++j)
        if (at == L + j) t = d[j];
    }
    d[i] = t;
  }
  a.step_tok[0] = last;
  a.step_pos[0] = L - 1;
#pragma unroll
  for (int i = 0; i < LKP_MAX_K; ++i)
    if (i < a.k) { a.step_tok[1 + i] = d[i]; a.step_pos[1 + i] = L + i; }
  *a.len = L;
  if (fin) *a.finished = 1;
  a.counters[0] += 1;
  a.counters[1] += emit - 1;
}

}  // namespace

// picks int64 [k + 1] (init: [1]); seq int64 [cap]; len int64 [1]; step_tok / step_pos int64 [k + 1]; finished int32 [1]; counters int64 [2]
// (steps, accepted).  init != 0: the first token after the prefill - picks[0] is emitted, nothing is confirmed, step_tok is not read.
extern "C" int llx_lookup_step(const int64_t* picks, int64_t* seq, int64_t cap, int64_t* len, int64_t* step_tok, int64_t* step_pos,
                               int32_t* finished, int64_t* counters, int64_t P, int64_t n, int k, int g, int64_t eos_id, int init,
                               hipStream_t stream) {
  LLX_REQUIRE(picks && seq && len && step_tok && step_pos && finished && counters,
              "llx_lookup_step: null pointer (picks, seq, len, step_tok, step_pos, finished and counters are required)");
  LLX_REQUIRE(k >= 1 && k <= LKP_MAX_K, "llx_lookup_step: k=%d draft tokens outside 1..%d", k, LKP_MAX_K);
  LLX_REQUIRE(g >= 1 && g <= LKP_MAX_G, "llx_lookup_step: g=%d (the longest n-gram) outside 1..%d", g, LKP_MAX_G);
  LLX_REQUIRE(P >= 1, "llx_lookup_step: P=%lld prompt tokens must be >= 1", (long long)P);
  LLX_REQUIRE(n >= 1, "llx_lookup_step: n=%lld new tokens must be >= 1", (long long)n);
  LLX_REQUIRE(P < (1ll << 31) && n < (1ll << 31) && cap < (1ll << 31), "llx_lookup_step: P, n and cap must stay below 2^31");
  LLX_REQUIRE(cap >= P + n, "llx_lookup_step: cap=%lld is smaller than P + n = %lld", (long long)cap, (long long)(P + n));
  LLX_REQUIRE(eos_id >= -1, "llx_lookup_step: eos_id=%lld must be a token id or -1 (none)", (long long)eos_id);
  LookupArgs a{picks, seq, len, step_tok, step_pos, finished, counters, P, n, eos_id, k, g, init ? 1 : 0};
  hipLaunchKernelGGL(lookup_step_kernel, dim3(1), dim3(LKP_THREADS), 0, stream, a);
  LLX_LAUNCH_CHECK("llx_lookup_step");
  return LLX_OK;
}
