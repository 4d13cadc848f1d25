// Per-token log-probabilities over bf16 logits: -F.cross_entropy(logits.float(), labels, reduction="none", ignore_index=-100)
// (the per-row terms of the mean that ce.hip reduces), differentiable with a PER-ROW upstream gradient.  The loss path (ce.hip) writes
// d logits in its forward because its upstream gradient is one scalar that can be applied afterwards; a per-row gradient cannot be
// applied later without a second bf16 rounding, so here the forward keeps the logits and the backward makes the second pass over the
// row in place, when g[t] is known: one rounding of d logits, and the traffic of forward + backward equals the loss path's.
#include "rowlse.h"

#define LP_THREADS 512

// One block per row: logp[t] = x[label] - lse[t], lse from the online (max, sum exp) pass that ce_row_kernel runs too (rowlse.h: the
// values are those of its pass 1), top1[t] (nullable) = index of the largest logit, the lowest among ties.  Ignored rows
// (label == -100): logp = lse = 0, top1 = -1, logits not read.  Rows at or past rows_dyn[0] rounded up to 256: zeros, nothing read.
__global__ __launch_bounds__(LP_THREADS) void logprob_row_fwd_kernel(const bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                                      float* __restrict__ logp, float* __restrict__ lse_out, int32_t* __restrict__ top1,
                                                                      int V, const int32_t* __restrict__ rows_dyn) {
  __shared__ float red[16];
  __shared__ int redi[16];
  const int64_t t = blockIdx.x;
  if (rows_dyn != nullptr && t >= ((rows_dyn[0] + 255) & ~255)) {
    if (threadIdx.x == 0) {
      logp[t] = 0.f;
      lse_out[t] = 0.f;
      if (top1) top1[t] = 0;
    }
    return;
  }
  const int64_t label = labels[t];
  if (label == -100) {
    if (threadIdx.x == 0) {
      logp[t] = 0.f;
      lse_out[t] = 0.f;
      if (top1) top1[t] = -1;
    }
    return;
  }
  const bf16_t* x = logits + t * ld;
  const int nchunk = V >> 3;
  const float xl = (label >= 0 && label < V) ? bf2f(x[label]) : 0.f;  // a label outside [0, V): as ce_row_kernel, its logit counts as 0
  const RowLse r = row_lse_pass<true, LP_THREADS>(x, nchunk);
  const float gm = block_max(r.m, red);
  const float s = block_sum(r.s * __expf(r.m - gm), red);
  const float ls = __logf(s);
  if (threadIdx.x == 0) {
    // x[label] - lse, taken as (x[label] - max) - log(sum): the first difference is exact for bf16 operands, so logp does not inherit the
    // rounding of lse to the magnitude of the logits (2^-10 absolute for logits near -3e4, where |logp| is a few units)
    logp[t] = (xl - gm) - ls;
    lse_out[t] = gm + ls;
  }
  if (top1) {
    const int a = block_min_i32(r.m == gm ? r.arg : INT_MAX, redi);
    if (threadIdx.x == 0) top1[t] = a == INT_MAX ? 0 : a;  // (a row without any finite maximum: index 0)
  }
}

// One block per row: dlogits[t, v] = bf16(g[t] * ((v == label) - exp(x[t, v] - lse[t]))), one rounding.  Ignored rows and rows with
// g[t] == 0 get a zero row; rows at or past rows_dyn[0] rounded up to 256 are neither read nor written.  logits / dlogits carry no
// __restrict__: the caller may pass the same buffer (in place).  Every thread reads a 16-byte chunk and then writes that same chunk,
// and lse comes from the forward, so no thread needs a value another one has overwritten (the label's logit included).
__global__ __launch_bounds__(LP_THREADS) void logprob_row_bwd_kernel(const bf16_t* logits, int64_t ld, bf16_t* dlogits, int64_t dld,
                                                                      const int64_t* __restrict__ labels, const float* __restrict__ lse_in,
                                                                      const float* __restrict__ g, int V, const int32_t* __restrict__ rows_dyn) {
  const int64_t t = blockIdx.x;
  if (rows_dyn != nullptr && t >= ((rows_dyn[0] + 255) & ~255)) return;
  const int64_t label = labels[t];
  const float gt = g[t];
  const int nchunk = V >> 3;
  bf16_t* dx = dlogits + t * dld;
  if (label == -100 || gt == 0.f) {
    const u32x4_t z = {0u, 0u, 0u, 0u};
    for (int c = threadIdx.x; c < nchunk; c += LP_THREADS) *reinterpret_cast<u32x4_t*>(dx + c * 8) = z;
    return;
  }
  const bf16_t* x = logits + t * ld;
  const float lse = lse_in[t];
  for (int c = threadIdx.x; c < nchunk; c += LP_THREADS) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(x + c * 8);
    u32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float d0 = -__expf(bflo(v[e]) - lse), d1 = -__expf(bfhi(v[e]) - lse);
      if (c * 8 + 2 * e == label) d0 += 1.f;
      if (c * 8 + 2 * e + 1 == label) d1 += 1.f;
      o[e] = pack_bf2(d0 * gt, d1 * gt);
    }
    *reinterpret_cast<u32x4_t*>(dx + c * 8) = o;
  }
}

// The [T] vectors of the compacted rows back to their positions, and the upstream gradient of the positions to the compacted rows:
// dst[i] = map[i] >= 0 ? src[map[i]] : fill, for a float vector and (nullable) an int32 vector from one launch.
__global__ __launch_bounds__(256) void logprob_map_rows_kernel(const int32_t* __restrict__ map, const float* __restrict__ src_f, float* __restrict__ dst_f,
                                                                float fill_f, const int32_t* __restrict__ src_i, int32_t* __restrict__ dst_i,
                                                                int32_t fill_i, int T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  const int j = map[i];
  const bool ok = j >= 0 && j < T;
  dst_f[i] = ok ? src_f[j] : fill_f;
  if (dst_i) dst_i[i] = ok ? src_i[j] : fill_i;
}

extern "C" int llx_logprob_map_rows(const int32_t* map, const float* src_f, float* dst_f, float fill_f, const int32_t* src_i, int32_t* dst_i,
                                    int32_t fill_i, int64_t T, hipStream_t stream) {
  LLX_REQUIRE(map && src_f && dst_f && (src_i != nullptr) == (dst_i != nullptr), "llx_logprob_map_rows: null pointer");
  LLX_REQUIRE(T > 0 && T < (1 << 30), "llx_logprob_map_rows: bad T");
  LLX_REQUIRE(src_f != dst_f && (src_i == nullptr || src_i != dst_i), "llx_logprob_map_rows: source and destination must differ");
  hipLaunchKernelGGL(logprob_map_rows_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, map, src_f, dst_f, fill_f, src_i, dst_i, fill_i,
                     (int)T);
  LLX_LAUNCH_CHECK("llx_logprob_map_rows");
  return LLX_OK;
}

// rows (nullable, device int32): the rows are compacted (llx_head_compact_index) and *rows is the number of labelled ones - semantics of
// llx_ce_fwd_bwd_rows: rows at or past *rows rounded up to 256 are not read; logp / lse / top1 are zero there.
extern "C" int llx_logprob_rows_fwd(const void* logits, int64_t ld, const int64_t* labels, float* logp, float* lse, int32_t* top1, int64_t T,
                                    int64_t V, const int32_t* rows, hipStream_t stream) {
  LLX_REQUIRE(logits && labels && logp && lse, "llx_logprob_rows_fwd: null pointer");
  LLX_REQUIRE(V % 8 == 0 && ld % 8 == 0, "llx_logprob_rows_fwd: V and row strides must be multiples of 8");
  LLX_REQUIRE(T > 0 && T < (1ll << 31) && V > 0 && V < (1 << 30) && ld >= V, "llx_logprob_rows_fwd: bad sizes");
  LLX_REQUIRE(rows == nullptr || (uintptr_t)rows % 4 == 0, "llx_logprob_rows_fwd: rows must be a device int32 pointer");
  LLX_REQUIRE((uintptr_t)logits % 16 == 0, "llx_logprob_rows_fwd: logits must be 16-byte aligned");
  hipLaunchKernelGGL(logprob_row_fwd_kernel, dim3((unsigned)T), dim3(LP_THREADS), 0, stream, (const bf16_t*)logits, ld, labels, logp, lse, top1, (int)V,
                     rows);
  LLX_LAUNCH_CHECK("llx_logprob_rows_fwd");
  return LLX_OK;
}

// dlogits may alias logits (the in-place form the LM head uses: the logits buffer becomes the gradient); rows as above - nothing is
// written at or past *rows rounded up to 256.
extern "C" int llx_logprob_rows_bwd(const void* logits, int64_t ld, void* dlogits, int64_t dld, const int64_t* labels, const float* lse, const float* g,
                                    int64_t T, int64_t V, const int32_t* rows, hipStream_t stream) {
  LLX_REQUIRE(logits && dlogits && labels && lse && g, "llx_logprob_rows_bwd: null pointer");
  LLX_REQUIRE(V % 8 == 0 && ld % 8 == 0 && dld % 8 == 0, "llx_logprob_rows_bwd: V and row strides must be multiples of 8");
  LLX_REQUIRE(T > 0 && T < (1ll << 31) && V > 0 && V < (1 << 30) && ld >= V && dld >= V, "llx_logprob_rows_bwd: bad sizes");
  LLX_REQUIRE(rows == nullptr || (uintptr_t)rows % 4 == 0, "llx_logprob_rows_bwd: rows must be a device int32 pointer");
  LLX_REQUIRE(((uintptr_t)logits | (uintptr_t)dlogits) % 16 == 0, "llx_logprob_rows_bwd: logits and dlogits must be 16-byte aligned");
  hipLaunchKernelGGL(logprob_row_bwd_kernel, dim3((unsigned)T), dim3(LP_THREADS), 0, stream, (const bf16_t*)logits, ld, (bf16_t*)dlogits, dld, labels, lse,
                     g, (int)V, rows);
  LLX_LAUNCH_CHECK("llx_logprob_rows_bwd");
  return LLX_OK;
}
