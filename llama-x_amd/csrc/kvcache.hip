// The FP8 (OCP E4M3) KV cache outside the hot kernels: KVCache.update into a cache of codes - the two scatters of
// decode.hip with q() of kv8.h on the way - and the transient bf16 image of a cache that the prefill kernels read.  The decode step
// itself never comes here: its q|k|v epilogue (wstream.h, GV_QKV_F8) writes codes and llx_attn_decode_f8 (decode.hip) reads them.
#include "kv8.h"

// cache[b, h, input_pos[l], :] = q(src[b, h, l, :]) for k and v in one launch.  A thread owns 16 elements: two 16-byte loads, one
// 16-byte store; 8 threads per row, 16 (k | v, position) rows per workgroup.  Cache strides in bytes.
__global__ __launch_bounds__(256) void kv_scatter_f8_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t s_sb, int64_t s_sh, int64_t s_ss,
                                                            uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, int64_t c_sb, int64_t c_sh, int64_t c_ss,
                                                            const int64_t* __restrict__ pos, int64_t p_sb, int L, int Smax) {
  const int chunk = threadIdx.x & 7, which = (threadIdx.x >> 3) & 1, li = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int h = blockIdx.y, b = blockIdx.z;
  if (li >= L) return;
  const int64_t p = pos[b * p_sb + li];  // p_sb = 0: one position row for every batch element
  if (p < 0 || p >= Smax) return;        // an out-of-range position writes nothing, as kv_scatter_kernel
  const bf16_t* src = (which ? v : k) + b * s_sb + h * s_sh + (int64_t)li * s_ss + chunk * 16;
  const u32x4_t lo = *reinterpret_cast<const u32x4_t*>(src), hi = *reinterpret_cast<const u32x4_t*>(src + 8);
  const u32x4_t codes = {kv8_encode_bf4(lo[0], lo[1]), kv8_encode_bf4(lo[2], lo[3]), kv8_encode_bf4(hi[0], hi[1]), kv8_encode_bf4(hi[2], hi[3])};
  uint8_t* dst = (which ? vc : kc) + b * c_sb + h * c_sh + p * c_ss + chunk * 16;
  *reinterpret_cast<u32x4_t*>(dst) = codes;
}

// p_sb = the row stride of input_pos [B, L]; 0: one position row [L] for every batch element
static int kv_scatter_f8_run(const char* fn, const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache,
                             int64_t c_sb, int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t p_sb, int64_t B, int64_t KVH, int64_t L, int64_t Smax,
                             int64_t head_dim, hipStream_t stream) {
  LLX_REQUIRE(k && v && k_cache && v_cache && input_pos, "%s: null pointer", fn);
  LLX_REQUIRE(head_dim == HD, "%s: head_dim=%lld unsupported (only 128)", fn, (long long)head_dim);
  LLX_REQUIRE(B > 0 && KVH > 0 && L > 0 && Smax > 0 && B < 65536 && KVH < 65536 && Smax < (1ll << 31), "%s: bad sizes", fn);
  LLX_REQUIRE(((s_sb | s_sh | s_ss) % 8) == 0 && ((c_sb | c_sh | c_ss) % 16) == 0 && c_ss >= HD, "%s: bad strides (source rows and cache rows - strides in bytes - must be 16-byte aligned)", fn);
  LLX_REQUIRE(((uintptr_t)k | (uintptr_t)v | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 == 0, "%s: pointers must be 16-byte aligned", fn);
  hipLaunchKernelGGL(kv_scatter_f8_kernel, dim3((unsigned)cdiv64(L, 16), (unsigned)KVH, (unsigned)B), dim3(256), 0, stream, (const bf16_t*)k, (const bf16_t*)v,
                     s_sb, s_sh, s_ss, (uint8_t*)k_cache, (uint8_t*)v_cache, c_sb, c_sh, c_ss, input_pos, p_sb, (int)L, (int)Smax);
  LLX_LAUNCH_CHECK(fn);
  return LLX_OK;
}

// llx_kv_scatter into an FP8 cache: cache[b, h, input_pos[l], :] = q(src[b, h, l, :]); k / v bf16 through element strides, caches uint8
// [B, KVH, Smax, 128] through BYTE strides (multiples of 16).
extern "C" int llx_kv_scatter_f8(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb,
                                 int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t B, int64_t KVH, int64_t L, int64_t Smax, int64_t head_dim,
                                 hipStream_t stream) {
  return kv_scatter_f8_run("llx_kv_scatter_f8", k, v, s_sb, s_sh, s_ss, k_cache, v_cache, c_sb, c_sh, c_ss, input_pos, 0, B, KVH, L, Smax, head_dim, stream);
}

// llx_kv_scatter_rows into an FP8 cache (input_pos int64 [B, L] with row stride p_sb >= L)
extern "C" int llx_kv_scatter_rows_f8(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb,
                                      int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t p_sb, int64_t B, int64_t KVH, int64_t L, int64_t Smax,
                                      int64_t head_dim, hipStream_t stream) {
  LLX_REQUIRE(p_sb >= L, "llx_kv_scatter_rows_f8: bad sizes (a position row shorter than L)");
  return kv_scatter_f8_run("llx_kv_scatter_rows_f8", k, v, s_sb, s_sh, s_ss, k_cache, v_cache, c_sb, c_sh, c_ss, input_pos, p_sb, B, KVH, L, Smax, head_dim,
                           stream);
}

// out[b, h, s, :] = dq(cache[b, h, s, :]): a thread owns 16 codes, one 16-byte load and two 16-byte stores; 8 threads per row
__global__ __launch_bounds__(256) void kv_dequantize_f8_kernel(const uint8_t* __restrict__ c, int64_t c_sb, int64_t c_sh, int64_t c_ss, bf16_t* __restrict__ out,
                                                               int KVH, int S, int64_t rows) {
  const int64_t row = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int chunk = threadIdx.x & 7;
  if (row >= rows) return;
  const int64_t s = row % S, bh = row / S;
  const int64_t h = bh % KVH, b = bh / KVH;
  const u32x4_t w = *reinterpret_cast<const u32x4_t*>(c + b * c_sb + h * c_sh + s * c_ss + chunk * 16);
  const u32x2_t a0 = kv8_decode_bf4(w[0]), a1 = kv8_decode_bf4(w[1]), a2 = kv8_decode_bf4(w[2]), a3 = kv8_decode_bf4(w[3]);
  bf16_t* dst = out + row * HD + chunk * 16;
  *reinterpret_cast<u32x4_t*>(dst) = u32x4_t{a0[0], a0[1], a1[0], a1[1]};
  *reinterpret_cast<u32x4_t*>(dst + 8) = u32x4_t{a2[0], a2[1], a3[0], a3[1]};
}

// The bf16 image of an FP8 cache (exact): cache uint8 [B, KVH, S, 128] through BYTE strides (multiples of 16) -> out bf16
// [B, KVH, S, 128] contiguous.
extern "C" int llx_kv_dequantize_f8(const void* cache, int64_t c_sb, int64_t c_sh, int64_t c_ss, void* out, int64_t B, int64_t KVH, int64_t S,
                                    int64_t head_dim, hipStream_t stream) {
  const char* fn = "llx_kv_dequantize_f8";
  LLX_REQUIRE(cache && out, "%s: null pointer", fn);
  LLX_REQUIRE(head_dim == HD, "%s: head_dim=%lld unsupported (only 128)", fn, (long long)head_dim);
  LLX_REQUIRE(B > 0 && KVH > 0 && S > 0 && B < 65536 && KVH < 65536 && S < (1ll << 31) && B * KVH * S < (1ll << 36), "%s: bad sizes", fn);
  LLX_REQUIRE(((c_sb | c_sh | c_ss) % 16) == 0 && c_ss >= HD, "%s: bad strides (cache rows - strides in bytes - must be 16-byte aligned)", fn);
  LLX_REQUIRE(((uintptr_t)cache | (uintptr_t)out) % 16 == 0, "%s: pointers must be 16-byte aligned", fn);
  const int64_t rows = B * KVH * S;
  hipLaunchKernelGGL(kv_dequantize_f8_kernel, dim3((unsigned)cdiv64(rows, 32)), dim3(256), 0, stream, (const uint8_t*)cache, c_sb, c_sh, c_ss, (bf16_t*)out,
                     (int)KVH, (int)S, rows);
  LLX_LAUNCH_CHECK(fn);
  return LLX_OK;
}
