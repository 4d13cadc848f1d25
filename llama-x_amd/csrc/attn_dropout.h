// Attention dropout: the keep decision of one (batch, head, query, key) element as a pure integer function of
// (seed, counter, stream_id, b, h, q, k) and the threshold.  The forward kernel, both backward kernels and llx_attn_dropout_keep call
// the functions below and nothing else, so the three register layouts of the score tile cannot disagree; tests/dropout_cases.py restates
// them in numpy.  Semantics as F.scaled_dot_product_attention(dropout_p=p): an element is dropped with probability t / 65536,
// t = round(p * 65536), and a kept one is scaled by c = 65536 / (65536 - t).
//
//   key   (64 bits, once per workgroup, scalar): splitmix64 finaliser over seed, counter, then (stream_id, b, h).
//   word  (32 bits, one per element - no word is shared between elements): the row term key.lo + q * G1 and the column term
//         key.hi + k * G2 are XORed and put through two multiply-xorshift rounds (the "lowbias32" constants); the element is dropped iff
//         the top 16 bits of the word are below t.
// One word per element is the same cost in all three kernels: the term of the index that sits on the lane is hoisted, the other one is
// an add with a literal per element (the per-tile base times G is wave-uniform), then 1 XOR + 6 mixing operations + compare + select.
// A word shared along k would halve that in the forward and dQ kernels (consecutive keys in a lane's registers) and save nothing in the
// dK/dV kernel (the key on the lane, 16 query rows in registers) - DESIGN.md section 8.
#pragma once
#include <stdint.h>

struct AttnDropKey { uint32_t lo, hi; };

__host__ __device__ __forceinline__ uint64_t attn_drop_mix64(uint64_t z) {  // splitmix64's finaliser (as csrc/sample.hip hashes)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// b, h < 2^16, 0 <= stream_id < 2^31 (checked by the entry points)
__host__ __device__ __forceinline__ AttnDropKey attn_dropout_key(int64_t seed, int64_t counter, int stream_id, int b, int h) {
  uint64_t z = attn_drop_mix64((uint64_t)seed + 0x9E3779B97F4A7C15ull * ((uint64_t)counter + 1));
  z = attn_drop_mix64(z ^ (((uint64_t)(uint32_t)stream_id << 32) | ((uint64_t)(uint32_t)b << 16) | (uint64_t)(uint32_t)h));
  return AttnDropKey{(uint32_t)z, (uint32_t)(z >> 32)};
}

__host__ __device__ __forceinline__ uint32_t attn_drop_row(AttnDropKey key, int q) { return key.lo + (uint32_t)q * 0x9E3779B1u; }
__host__ __device__ __forceinline__ uint32_t attn_drop_col(AttnDropKey key, int k) { return key.hi + (uint32_t)k * 0x85EBCA77u; }

// thr16 = t << 16 (0 < t < 65536): x >= thr16 compares the word's top 16 bits with t
__host__ __device__ __forceinline__ bool attn_drop_keep(uint32_t row, uint32_t col, uint32_t thr16) {
  uint32_t x = row ^ col;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  return x >= thr16;
}

__host__ __device__ __forceinline__ bool attn_dropout_keep(int64_t seed, int64_t counter, int stream_id, int b, int h, int q, int k,
                                                           uint32_t thr16) {
  const AttnDropKey key = attn_dropout_key(seed, counter, stream_id, b, h);
  return attn_drop_keep(attn_drop_row(key, q), attn_drop_col(key, k), thr16);
}
