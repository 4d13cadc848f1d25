// Token sampler: one token for each of R independent rows of logits (greedy, temperature, top-k, top-p), one workgroup per row.
// The host loop that this replaces is softmax + a V-wide sort + cumsum + multinomial + .item() per token (llx/generate.py).
//
// Everything after the per-element weight is integer arithmetic, so the result does not depend on any summation order:
//   z_i = logit_i / temperature (fp32, IEEE divide),  key_i = order-preserving uint32 image of z_i,
//   w_i = floor(expf(z_i - z_max) * 2^40) as uint64  (the sum of a 2^17-wide row stays below 2^58).
// Passes over the row (the first reads HBM, the rest hit L2: the row is NOT kept in registers):
//   0  max / min / lowest argmax / size of the tie group                    (greedy ends here)
//   1  top-k: three histogram levels over the key bits (11 + 11 + 10) -> the exact k-th largest key, its count and weight above
//   2  top-p: the same three levels, descending by weight: the smallest present key whose strictly-greater weight is < top_p * W
//   3  without either filter: one plain sum for W
//   4  draw: block prefix scan of the kept weights in index order, rounds of 1024 chunks, stops at the round that crosses u * W
// Histograms are LDS atomics on integers (count u32, weight u64, smallest raw logit of the bin u32): deterministic.
//
// llx_sample_rows_ext (the EXT instances; the plain ones do not pay for it) adds rule 0 of llx/sampling.py in front: every
// pass above reads the row through the PENALISED view - element i with counts[r][i] > 0 becomes x > 0 ? x / theta : x * theta, then
// x - (alpha_p + alpha_f * c), single fp32 operations - the thread that writes the token also does counts[r][token] += 1, and one more
// pass over the RAW row gives the token's log-probability (max and sum of exp in fp32, a fixed reduction shape).
#include "common.h"
#include "rowview.h"  // RowView, smp_key / smp_unkey
#include <type_traits>

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)
#define SMP_BINS 2048
#define SMP_WSCALE 1099511627776.0f  // 2^40

namespace {

struct SampleArgs {
  const void* logits;
  int64_t ld;
  int V;
  float temperature;
  int64_t top_k;
  float top_p;
  uint64_t seed;
  int64_t* pos;
  int64_t* token_out;
  int64_t* history;
  int64_t hist_ld, hist_cap, hist_base;
  int advance;
  int64_t eos_id;
  int32_t* finished;
  float* aux_u;
  float* aux_thresh;
  int32_t* aux_kept;
};

struct SampleExtArgs : SampleArgs {
  int32_t* counts;  // [R, ldc], indexed by token id; null = no penalties
  int64_t ldc;
  float rep, pres, freq;
  float* logprob_history;  // the geometry of history
};

// The row through rule 0: a RowView whose load() penalises the elements that have occurred.  Counts are indexed by token id, which a
// row's grid offset shifts against the chunks, so they are per-element dword loads (of a table that stays in L2 between the passes).
template <typename T>
struct PenRow : RowView<T> {
  using RowView<T>::E;
  const int32_t* cnt;
  float rep, pres, freq;
  __device__ PenRow(const void* p, int V_, const int32_t* cnt_, float rep_, float pres_, float freq_)
      : RowView<T>(p, V_), cnt(cnt_), rep(rep_), pres(pres_), freq(freq_) {}
  __device__ __forceinline__ uint32_t load_raw(int c, float (&v)[E]) const { return RowView<T>::load(c, v); }
  __device__ __forceinline__ uint32_t load(int c, float (&v)[E]) const {
#pragma clang fp contract(off)
    const uint32_t m = RowView<T>::load(c, v);
    if (cnt) {
      const int i0 = c * E - this->off;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if ((m >> e) & 1) {
          const int n = cnt[i0 + e];
          if (n > 0) {
            float x = v[e];
            x = x > 0.f ? x / rep : x * rep;
            float t = freq * (float)n;
            t = pres + t;
            v[e] = x - t;
          }
        }
      }
    }
    return m;
  }
};

__device__ __forceinline__ uint64_t smp_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ uint64_t smp_weight(float z, float zmax) {
  const float w = (z == zmax) ? 1.f : expf(z - zmax);
  return (uint64_t)(w * SMP_WSCALE);
}

struct SmpShared {
  uint32_t cnt[SMP_BINS];
  uint64_t ws[SMP_BINS];
  uint32_t rawmin[SMP_BINS];  // smallest raw-logit key of the bin
  uint64_t wave_w[SMP_WAVES];
  uint32_t wave_c[SMP_WAVES];
  float red_f[SMP_WAVES];
  uint32_t red_u[SMP_WAVES];
  int red_i[SMP_WAVES];
  uint32_t sel;       // position (descending order) of the chosen bin
  uint32_t sel_cnt;   // count strictly above the chosen bin (inside the current prefix)
  uint64_t sel_w;     // weight strictly above the chosen bin (inside the current prefix)
  int token;
};

// inclusive block scan of (c, w) over the 1024 threads in thread order; returns the totals through tc / tw
__device__ __forceinline__ void smp_scan(uint32_t& c, uint64_t& w, uint32_t& tc, uint64_t& tw, SmpShared& sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t c2 = __shfl_up(c, o, 64);
    const uint32_t lo = __shfl_up((uint32_t)w, o, 64), hi = __shfl_up((uint32_t)(w >> 32), o, 64);
    if (lane >= o) { c += c2; w += ((uint64_t)hi << 32) | lo; }
  }
  __syncthreads();  // the previous user of wave_c / wave_w is done
  if (lane == 63) { sh.wave_c[wv] = c; sh.wave_w[wv] = w; }
  __syncthreads();
  tc = 0; tw = 0;
  uint32_t pc = 0; uint64_t pw = 0;
#pragma unroll
  for (int i = 0; i < SMP_WAVES; ++i) {
    const uint32_t ci = sh.wave_c[i]; const uint64_t wi = sh.wave_w[i];
    if (i < wv) { pc += ci; pw += wi; }
    tc += ci; tw += wi;
  }
  c += pc; w += pw;
}

// One filter = three histogram levels over the key bits, most significant first.  Among the elements with key >= klo, walk the
// values in descending order and stop at the LAST present value whose strictly-greater mass is below the target:
//   by_weight = false: mass = count,  target = k        -> the k-th largest key (duplicates counted)
//   by_weight = true:  mass = weight, target = top_p*W  -> the top-p threshold (W = the weight of all elements with key >= klo)
// Returns the key; kept / wkept = count and weight of key >= that key; rawkey = key image of the smallest raw logit at that key.
template <typename Row>
__device__ void smp_refine(const Row& row, float T_, float zmax, uint32_t klo, bool by_weight, uint32_t k, float top_p,
                           uint32_t& key_out, uint32_t& kept, uint64_t& wkept, uint32_t& rawkey, SmpShared& sh) {
  constexpr int E = Row::E;
  const int tid = threadIdx.x;
  uint32_t prefix = 0, pmask = 0;
  uint32_t cnt_above = 0;
  uint64_t w_above = 0;
  double wtarget = 0.0;
#pragma unroll 1
  for (int lvl = 0; lvl < 3; ++lvl) {
    const int shift = lvl == 0 ? 21 : (lvl == 1 ? 10 : 0);
    const uint32_t nb = lvl == 2 ? 1024u : 2048u;
    __syncthreads();
    for (int b = tid; b < SMP_BINS; b += SMP_THREADS) { sh.cnt[b] = 0; sh.ws[b] = 0; sh.rawmin[b] = 0xffffffffu; }
    if (tid == 0) sh.sel = 0;
    __syncthreads();
    for (int c = tid; c < row.nchunks; c += SMP_THREADS) {
      float v[E];
      const uint32_t m = row.load(c, v);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float z = v[e] / T_;
        const uint32_t key = smp_key(z);
        if (((m >> e) & 1) && (key & pmask) == prefix && key >= klo) {
          const uint32_t d = (key >> shift) & (nb - 1);
          atomicAdd(&sh.cnt[d], 1u);
          atomicAdd((unsigned long long*)&sh.ws[d], (unsigned long long)smp_weight(z, zmax));
          if (lvl == 2) atomicMin(&sh.rawmin[d], smp_key(v[e]));
        }
      }
    }
    __syncthreads();
    // thread t owns the bins at descending positions 2t, 2t+1 (position p = bin nb-1-p); positions >= nb are empty
    const uint32_t p0 = 2u * tid, p1 = p0 + 1;
    const uint32_t c0 = p0 < nb ? sh.cnt[nb - 1 - p0] : 0u, c1 = p1 < nb ? sh.cnt[nb - 1 - p1] : 0u;
    const uint64_t w0 = p0 < nb ? sh.ws[nb - 1 - p0] : 0ull, w1 = p1 < nb ? sh.ws[nb - 1 - p1] : 0ull;
    uint32_t ic = c0 + c1, tc;
    uint64_t iw = w0 + w1, tw;
    smp_scan(ic, iw, tc, tw, sh);
    if (lvl == 0 && by_weight) wtarget = (double)top_p * (double)tw;  // W of the kept set so far
    const uint32_t ec0 = cnt_above + ic - c0 - c1, ec1 = ec0 + c0;  // mass strictly above position p0 / p1
    const uint64_t ew0 = w_above + iw - w0 - w1, ew1 = ew0 + w0;
    const bool ok0 = c0 && (by_weight ? ((double)ew0 < wtarget) : (ec0 < k));
    const bool ok1 = c1 && (by_weight ? ((double)ew1 < wtarget) : (ec1 < k));
    // the topmost present position always qualifies (mass above it is 0 at level 0, and the chosen bin's own mass above at deeper levels)
    if (ok1) atomicMax(&sh.sel, p1 + 1);
    else if (ok0) atomicMax(&sh.sel, p0 + 1);
    __syncthreads();
    const uint32_t sel = sh.sel ? sh.sel - 1 : 0u;  // sel == 0 only if nothing matched (cannot happen for a non-empty candidate set)
    if (sel == p0) { sh.sel_cnt = ec0; sh.sel_w = ew0; }
    if (sel == p1) { sh.sel_cnt = ec1; sh.sel_w = ew1; }
    __syncthreads();
    cnt_above = sh.sel_cnt;
    w_above = sh.sel_w;
    const uint32_t d = nb - 1 - sel;
    prefix |= d << shift;
    pmask |= (nb - 1) << shift;
    if (lvl == 2) {
      key_out = prefix;
      kept = cnt_above + sh.cnt[d];
      wkept = w_above + sh.ws[d];
      rawkey = sh.rawmin[d];
    }
  }
  __syncthreads();
}

template <typename T, bool EXT>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(std::conditional_t<EXT, SampleExtArgs, SampleArgs> a) {
  using Row = std::conditional_t<EXT, PenRow<T>, RowView<T>>;
  constexpr int E = RowView<T>::E;
  __shared__ SmpShared sh;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (a.finished && a.finished[r]) {  // a finished row repeats eos and touches nothing else
    if (tid == 0) a.token_out[r] = a.eos_id;
    return;
  }
  const int64_t pos = a.pos[r];
  const Row row = [&] {
    if constexpr (EXT)
      return Row((const T*)a.logits + (int64_t)r * a.ld, a.V, a.counts ? a.counts + (int64_t)r * a.ldc : nullptr, a.rep, a.pres, a.freq);
    else
      return Row((const T*)a.logits + (int64_t)r * a.ld, a.V);
  }();
  const uint64_t m24 = smp_mix(smp_mix(smp_mix(a.seed) ^ (uint64_t)pos) ^ (uint64_t)r) >> 40;
  const float u = (float)m24 * 5.9604644775390625e-08f;  // 2^-24: exact

  // ---- pass 0: max, min, lowest index of the max, size of its tie group
  float mx = -INFINITY, mn = INFINITY;
  int amax = 0x7fffffff;
  uint32_t nmax = 0;
  for (int c = tid; c < row.nchunks; c += SMP_THREADS) {
    float v[E];
    const uint32_t m = row.load(c, v);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if ((m >> e) & 1) {
        const int i = c * E - row.off + e;
        if (v[e] > mx || amax == 0x7fffffff) { mx = v[e]; amax = i; nmax = 1; }
        else if (v[e] == mx) { nmax++; amax = min(amax, i); }
        mn = fminf(mn, v[e]);
      }
    }
  }
  const float wmx = wave_max(mx), wmn = -wave_max(-mn);
  if (lane == 0) { sh.red_f[wv] = wmx; }
  __syncthreads();
  float bmx = sh.red_f[0];
#pragma unroll
  for (int i = 1; i < SMP_WAVES; ++i) bmx = fmaxf(bmx, sh.red_f[i]);
  __syncthreads();
  if (lane == 0) { sh.red_f[wv] = wmn; }
  int ai = (mx == bmx && amax != 0x7fffffff) ? amax : 0x7fffffff;
  uint32_t ni = (mx == bmx && amax != 0x7fffffff) ? nmax : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { ai = min(ai, __shfl_xor(ai, o, 64)); ni += __shfl_xor(ni, o, 64); }
  if (lane == 0) { sh.red_i[wv] = ai; sh.red_u[wv] = ni; }
  __syncthreads();
  float bmn = sh.red_f[0];
  int bai = sh.red_i[0];
  uint32_t bni = sh.red_u[0];
#pragma unroll
  for (int i = 1; i < SMP_WAVES; ++i) { bmn = fminf(bmn, sh.red_f[i]); bai = min(bai, sh.red_i[i]); bni += sh.red_u[i]; }
  __syncthreads();

  int token = 0;
  float thresh = bmx;
  uint32_t kept = bni;
  const bool greedy = a.temperature == 0.f;
  if (greedy || bmx == -INFINITY) {  // argmax, lowest index among ties; a row of -inf has every index tied: index 0
    token = bai;
  } else {
    const float T_ = a.temperature;
    const float zmax = bmx / T_;
    uint32_t klo = 0, rawkey = smp_key(bmn);
    uint64_t W = 0;
    kept = (uint32_t)a.V;
    bool have_w = false;
    if (a.top_k > 0 && a.top_k < (int64_t)a.V) {
      smp_refine(row, T_, zmax, 0u, false, (uint32_t)a.top_k, 1.f, klo, kept, W, rawkey, sh);
      have_w = true;
    }
    if (a.top_p < 1.f) {
      smp_refine(row, T_, zmax, klo, true, 0u, a.top_p, klo, kept, W, rawkey, sh);
      have_w = true;
    }
    if (!have_w) {  // nothing filtered: W is the plain sum
      uint64_t s = 0;
      for (int c = tid; c < row.nchunks; c += SMP_THREADS) {
        float v[E];
        const uint32_t m = row.load(c, v);
#pragma unroll
        for (int e = 0; e < E; ++e)
          if ((m >> e) & 1) s += smp_weight(v[e] / T_, zmax);
      }
      uint32_t dc = 0, tc;
      smp_scan(dc, s, tc, W, sh);
    }
    thresh = smp_unkey(rawkey);
    // ---- draw: the first kept index whose running weight exceeds floor(m * W / 2^24), u = m * 2^-24
    const uint64_t target = (__umul64hi(m24, W) << 40) | ((m24 * W) >> 24);
    uint64_t carry = 0;
    if (tid == 0) sh.token = -1;
    const int rounds = (row.nchunks + SMP_THREADS - 1) / SMP_THREADS;
#pragma unroll 1
    for (int rd = 0; rd < rounds; ++rd) {
      const int c = rd * SMP_THREADS + tid;
      uint64_t w[E];
      uint64_t s = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) w[e] = 0;
      if (c < row.nchunks) {
        float v[E];
        const uint32_t m = row.load(c, v);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float z = v[e] / T_;
          if (((m >> e) & 1) && smp_key(z) >= klo) w[e] = smp_weight(z, zmax);
          s += w[e];
        }
      }
      uint32_t dc = 0, tc;
      uint64_t incl = s, tot;
      smp_scan(dc, incl, tc, tot, sh);
      if (carry + tot > target) {  // uniform: the crossing lies in this round
        const uint64_t excl = carry + incl - s;
        if (excl <= target && carry + incl > target) {
          uint64_t run = excl;
          int found = -1;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            run += w[e];
            if (found < 0 && run > target) found = c * E - row.off + e;
          }
          sh.token = found;
        }
        break;
      }
      carry += tot;
    }
    __syncthreads();
    token = sh.token;
    if (token < 0) token = bai;  // W == 0 cannot happen (the maximum weighs 2^40); stay inside the row regardless
  }

  if constexpr (EXT) {
    // ---- the log-probability of the token on the RAW row: (l_tok - l_max) - log sum exp(l - l_max), reduced per thread, per wave, then
    // over the 16 waves in order.  Only when its history slot exists.
    const int64_t h = pos - a.hist_base;
    if (a.logprob_history && h >= 0 && h < a.hist_cap) {
      float lmax = bmx;  // without counts pass 0 read the raw row
      if (a.counts) {
        float m_ = -INFINITY;
        for (int c = tid; c < row.nchunks; c += SMP_THREADS) {
          float v[E];
          row.load_raw(c, v);  // invalid elements read as -inf
#pragma unroll
          for (int e = 0; e < E; ++e) m_ = fmaxf(m_, v[e]);
        }
        m_ = wave_max(m_);
        __syncthreads();
        if (lane == 0) sh.red_f[wv] = m_;
        __syncthreads();
        lmax = sh.red_f[0];
#pragma unroll
        for (int i = 1; i < SMP_WAVES; ++i) lmax = fmaxf(lmax, sh.red_f[i]);
      }
      float s = 0.f;
      for (int c = tid; c < row.nchunks; c += SMP_THREADS) {
        float v[E];
        const uint32_t m = row.load_raw(c, v);
#pragma unroll
        for (int e = 0; e < E; ++e)
          if ((m >> e) & 1) s += (v[e] == lmax) ? 1.f : expf(v[e] - lmax);
      }
      s = wave_sum(s);
      __syncthreads();
      if (lane == 0) sh.red_f[wv] = s;
      __syncthreads();
      if (tid == 0) {
        float tot = sh.red_f[0];
#pragma unroll
        for (int i = 1; i < SMP_WAVES; ++i) tot += sh.red_f[i];
        const T raw = ((const T*)a.logits)[(int64_t)r * a.ld + token];
        float lt;
        if constexpr (sizeof(T) == 2) lt = bf2f(raw); else lt = raw;
        const float d = (lt == lmax) ? 0.f : ((lt != lt) ? -INFINITY : lt - lmax);
        a.logprob_history[(int64_t)r * a.hist_ld + h] = d - logf(tot);
      }
    }
    // one workgroup owns the row and every read of the counts lies behind a barrier: a plain read-modify-write
    if (tid == 0 && a.counts) a.counts[(int64_t)r * a.ldc + token] += 1;
  }

  if (tid == 0) {
    a.token_out[r] = (int64_t)token;
    if (a.history) {
      const int64_t h = pos - a.hist_base;
      if (h >= 0 && h < a.hist_cap) a.history[(int64_t)r * a.hist_ld + h] = (int64_t)token;
    }
    if (a.advance) a.pos[r] = pos + 1;
    if (a.finished && (int64_t)token == a.eos_id) a.finished[r] = 1;
    if (a.aux_u) a.aux_u[r] = u;
    if (a.aux_thresh) a.aux_thresh[r] = thresh;
    if (a.aux_kept) a.aux_kept[r] = (int32_t)kept;
  }
}

}  // namespace

// the checks both entry points share; `name` begins every message
static int smp_check(const char* name, const void* logits, int dtype, int64_t ld, int64_t R, int64_t V, float temperature, int64_t top_k, float top_p,
                     const int64_t* pos, const int64_t* token_out, const int64_t* history, int64_t hist_ld, int64_t hist_cap) {
  LLX_REQUIRE(logits && pos && token_out, "%s: null pointer (logits, pos and token_out are required)", name);
  LLX_REQUIRE(dtype == 0 || dtype == 1, "%s: dtype=%d (0 = bf16, 1 = fp32)", name, dtype);
  LLX_REQUIRE(R > 0 && R < (1ll << 31), "%s: R=%lld must be positive", name, (long long)R);
  LLX_REQUIRE(V > 0 && V < (1ll << 30), "%s: V=%lld must be in [1, 2^30)", name, (long long)V);
  LLX_REQUIRE(ld >= V, "%s: row stride %lld < V=%lld", name, (long long)ld, (long long)V);
  LLX_REQUIRE(temperature >= 0.f, "%s: temperature=%g must be >= 0", name, (double)temperature);
  LLX_REQUIRE(top_k >= 0, "%s: top_k=%lld must be >= 0 (0 = off)", name, (long long)top_k);
  LLX_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p=%g must be in (0, 1]", name, (double)top_p);
  LLX_REQUIRE((uintptr_t)logits % (dtype ? 4 : 2) == 0, "%s: logits not aligned to their element size", name);
  LLX_REQUIRE(!history || (hist_cap > 0 && hist_ld >= hist_cap), "%s: history needs cap > 0 and a row stride >= cap", name);
  return LLX_OK;
}

// dtype: 0 = bf16, 1 = fp32.  history / finished / aux_* nullable; eos_id is read only with finished.
extern "C" int llx_sample_rows(const void* logits, int dtype, int64_t ld, int64_t R, int64_t V, float temperature, int64_t top_k, float top_p,
                               uint64_t seed, int64_t* pos, int64_t* token_out, int64_t* history, int64_t hist_ld, int64_t hist_cap,
                               int64_t hist_base, int advance, int64_t eos_id, int32_t* finished, float* aux_u, float* aux_thresh,
                               int32_t* aux_kept, hipStream_t stream) {
  if (int rc = smp_check("llx_sample_rows", logits, dtype, ld, R, V, temperature, top_k, top_p, pos, token_out, history, hist_ld, hist_cap)) return rc;
  SampleArgs a{logits, ld, (int)V, temperature, top_k, top_p, seed, pos, token_out, history, hist_ld, hist_cap, hist_base, advance, eos_id,
               finished, aux_u, aux_thresh, aux_kept};
  if (dtype == 0)
    hipLaunchKernelGGL((sample_rows_kernel<bf16_t, false>), dim3((unsigned)R), dim3(SMP_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((sample_rows_kernel<float, false>), dim3((unsigned)R), dim3(SMP_THREADS), 0, stream, a);
  LLX_LAUNCH_CHECK("llx_sample_rows");
  return LLX_OK;
}

// llx_sample_rows with rule 0 and the log-probability.  counts (nullable, int32 [R, ldc], ldc >= V): null = no penalties whatever the
// three floats are; otherwise the row is read through the penalised view and counts[r][token] += 1 after the draw.  logprob_history
// (nullable, fp32, the geometry of history, which it needs): the raw-logit log-probability of the token at history's slot.
extern "C" int llx_sample_rows_ext(const void* logits, int dtype, int64_t ld, int64_t R, int64_t V, float temperature, int64_t top_k, float top_p,
                                   uint64_t seed, int64_t* pos, int64_t* token_out, int64_t* history, int64_t hist_ld, int64_t hist_cap,
                                   int64_t hist_base, int advance, int64_t eos_id, int32_t* finished, float* aux_u, float* aux_thresh,
                                   int32_t* aux_kept, int32_t* counts, int64_t ldc, float repetition_penalty, float presence_penalty,
                                   float frequency_penalty, float* logprob_history, hipStream_t stream) {
  const char* name = "llx_sample_rows_ext";
  if (int rc = smp_check(name, logits, dtype, ld, R, V, temperature, top_k, top_p, pos, token_out, history, hist_ld, hist_cap)) return rc;
  LLX_REQUIRE(repetition_penalty > 0.f && repetition_penalty - repetition_penalty == 0.f,
              "%s: repetition_penalty=%g must be finite and > 0 (1 = off)", name, (double)repetition_penalty);
  LLX_REQUIRE(presence_penalty - presence_penalty == 0.f, "%s: presence_penalty=%g must be finite (0 = off)", name, (double)presence_penalty);
  LLX_REQUIRE(frequency_penalty - frequency_penalty == 0.f, "%s: frequency_penalty=%g must be finite (0 = off)", name, (double)frequency_penalty);
  LLX_REQUIRE((uintptr_t)counts % 4 == 0, "%s: counts not aligned to 4 bytes", name);
  LLX_REQUIRE(!counts || ldc >= V, "%s: counts row stride ldc=%lld < V=%lld", name, (long long)ldc, (long long)V);
  LLX_REQUIRE(!logprob_history || history, "%s: logprob_history shares the geometry of history, which is null", name);
  LLX_REQUIRE((uintptr_t)logprob_history % 4 == 0, "%s: logprob_history not aligned to 4 bytes", name);
  SampleExtArgs a{{logits, ld, (int)V, temperature, top_k, top_p, seed, pos, token_out, history, hist_ld, hist_cap, hist_base, advance, eos_id,
                   finished, aux_u, aux_thresh, aux_kept},
                  counts, ldc, repetition_penalty, presence_penalty, frequency_penalty, logprob_history};
  if (dtype == 0)
    hipLaunchKernelGGL((sample_rows_kernel<bf16_t, true>), dim3((unsigned)R), dim3(SMP_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((sample_rows_kernel<float, true>), dim3((unsigned)R), dim3(SMP_THREADS), 0, stream, a);
  LLX_LAUNCH_CHECK(name);
  return LLX_OK;
}
