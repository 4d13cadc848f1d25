// A row of logits as the token sampler (sample.hip) and the beam shortlist (beam.hip) read it: any element start, 16-byte interior
// loads, peeled ends, and the order-preserving integer image of a float that both compare by.
#pragma once
#include "common.h"

namespace {

// order-preserving image of a float: a < b  <=>  key(a) < key(b); -0 is folded onto +0 first (they compare equal)
__device__ __forceinline__ uint32_t smp_key(float z) {
  if (z == 0.f) z = 0.f;
  const uint32_t b = __float_as_uint(z);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float smp_unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// A row as a sequence of 16-byte chunks on the 16-byte grid of memory: chunk c holds elements [c*E - off, c*E - off + E) of the row,
// `off` = elements between the grid line below the row's first element and that element.  Interior chunks are one vector load; the
// first and last chunk (the peeled head and tail) are read element by element and never touch memory outside the row.
template <typename T>
struct RowView;
template <>
struct RowView<bf16_t> {
  static constexpr int E = 8;
  const bf16_t* base;  // grid-aligned: row - off
  int off, V, nchunks;
  __device__ RowView(const void* p, int V_) : V(V_) {
    const uintptr_t a = (uintptr_t)p;
    off = (int)((a & 15) >> 1);
    base = (const bf16_t*)p - off;
    nchunks = (V + off + E - 1) / E;
  }
  // v[e] for the valid elements (bit e of the returned mask); NaN reads as -inf
  __device__ __forceinline__ uint32_t load(int c, float (&v)[8]) const {
    const int i0 = c * E - off;
    if (i0 >= 0 && i0 + E <= V) {
      const u32x4_t q = *reinterpret_cast<const u32x4_t*>(base + (int64_t)c * E);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[2 * e] = bflo(q[e]); v[2 * e + 1] = bfhi(q[e]); }
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (v[e] != v[e]) ? -INFINITY : v[e];
      return 0xffu;
    }
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = i0 + e;
      v[e] = -INFINITY;
      if (i >= 0 && i < V) {
        const float x = bf2f(base[(int64_t)c * E + e]);
        v[e] = (x != x) ? -INFINITY : x;
        m |= 1u << e;
      }
    }
    return m;
  }
};
template <>
struct RowView<float> {
  static constexpr int E = 4;
  const float* base;
  int off, V, nchunks;
  __device__ RowView(const void* p, int V_) : V(V_) {
    const uintptr_t a = (uintptr_t)p;
    off = (int)((a & 15) >> 2);
    base = (const float*)p - off;
    nchunks = (V + off + E - 1) / E;
  }
  __device__ __forceinline__ uint32_t load(int c, float (&v)[4]) const {
    const int i0 = c * E - off;
    if (i0 >= 0 && i0 + E <= V) {
      const f32x4_t q = *reinterpret_cast<const f32x4_t*>(base + (int64_t)c * E);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (q[e] != q[e]) ? -INFINITY : q[e];
      return 0xfu;
    }
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = i0 + e;
      v[e] = -INFINITY;
      if (i >= 0 && i < V) {
        const float x = base[(int64_t)c * E + e];
        v[e] = (x != x) ? -INFINITY : x;
        m |= 1u << e;
      }
    }
    return m;
  }
};

}  // namespace
