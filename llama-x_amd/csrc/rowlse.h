// The online (max, sum exp) pass over a bf16 row in 16-byte chunks: pass 1 of the loss row kernel (ce.hip) and the whole read of the
// log-probability row kernel (logprob.hip).  One arithmetic in one order, so both kernels form the same lse = max + log(sum) of a row.
#pragma once
#include "common.h"

#include <climits>

struct RowLse {
  float m, s;  // this thread's running maximum and sum exp(x - m) over its chunks
  int arg;     // ARGMAX: index of the thread's first element equal to m (INT_MAX: the thread saw no chunk)
};

// Thread threadIdx.x of THREADS takes chunks threadIdx.x, threadIdx.x + THREADS, ... of the row's nchunk chunks of 8 elements.
template <bool ARGMAX, int THREADS>
__device__ __forceinline__ RowLse row_lse_pass(const bf16_t* x, int nchunk) {
  RowLse r = {-INFINITY, 0.f, INT_MAX};
  for (int c = threadIdx.x; c < nchunk; c += THREADS) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(x + c * 8);
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[2 * e] = bflo(v[e]); f[2 * e + 1] = bfhi(v[e]); }
    float cm = f[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) cm = fmaxf(cm, f[e]);
    if constexpr (ARGMAX) {
      if (cm > r.m) {  // strictly larger: a thread's chunks ascend, so its first maximum stays
        int ce = 7;
#pragma unroll
        for (int e = 6; e >= 0; --e) ce = (f[e] == cm) ? e : ce;
        r.arg = c * 8 + ce;
      }
    }
    const float mn = fmaxf(r.m, cm);
    float add = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) add += __expf(f[e] - mn);
    r.s = r.s * __expf(r.m - mn) + add;
    r.m = mn;
  }
  return r;
}
