// The FP8 KV cache format: OCP E4M3 (e4m3fn: bias 7, normals from 2^-6, subnormals in steps of 2^-9, no infinities, one
// NaN code per sign), no scale.  q(x) is defined on the bf16 value x the bf16 cache would have held: clamp to [-448, 448], round to
// nearest even on the E4M3 grid, the sign bit is the input's, NaN stays NaN.  dq(code) is exact in bf16 for every code.  Shared by
// the cache kernels (kvcache.hip), the q|k|v epilogue of the weight streams (wstream.h) and the decode attention (decode.hip).
#pragma once
#include "common.h"

// the clamp of q(): comparisons, not min / max - a NaN passes through them (fminf / fmaxf would return the bound), and -0 keeps its sign
__device__ __forceinline__ float kv8_clamp(float x) { return x > 448.f ? 448.f : (x < -448.f ? -448.f : x); }

// q() of four values (already rounded to bf16 by the caller) -> four codes, value 0 in the low byte: two v_cvt_pk_fp8_f32
__device__ __forceinline__ uint32_t kv8_encode4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a), kv8_clamp(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(c), kv8_clamp(d), w, true);
  return (uint32_t)w;
}
// q() of two values -> two codes in the low 16 bits
__device__ __forceinline__ uint32_t kv8_encode2(float a, float b) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a), kv8_clamp(b), 0, false) & 0xffffu;
}
// q() of two packed bf16 pairs (four cache elements) -> four codes
__device__ __forceinline__ uint32_t kv8_encode_bf4(uint32_t p0, uint32_t p1) { return kv8_encode4(bflo(p0), bfhi(p0), bflo(p1), bfhi(p1)); }

// dq() of the four codes of a word -> fp32 (exact): two v_cvt_pk_f32_fp8
__device__ __forceinline__ void kv8_decode4(uint32_t w, float (&f)[4]) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0]; f[1] = lo[1]; f[2] = hi[0]; f[3] = hi[1];
}
// dq() of the eight codes of two words -> fp32, element order
__device__ __forceinline__ void kv8_decode8(const u32x2_t& w, float (&f)[8]) {
  float a[4], b[4];
  kv8_decode4(w[0], a);
  kv8_decode4(w[1], b);
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
}
// dq() of the four codes of a word -> two packed bf16 pairs (every decoded value is a bf16 value: the rounding changes nothing)
__device__ __forceinline__ u32x2_t kv8_decode_bf4(uint32_t w) {
  float f[4];
  kv8_decode4(w, f);
  return u32x2_t{pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3])};
}
