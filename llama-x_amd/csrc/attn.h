// What attn_fwd.hip, attn_bwd.hip and attn_dense.hip share: tile geometry, address-space typedefs, and host-side pieces that take the entry
// point's name (a message starts with the function the caller called).  What the entries check differently on purpose: DESIGN.md section 4.
#pragma once
#include "common.h"  // HD
#include <type_traits>

#define BQ 128                    // query rows of a tile-flag block
#define BKV 64                    // keys of a tile
#define TILE_BYTES (64 * HD * 2)  // a 64-row x 128-col bf16 tile = 16 KiB

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;

static inline int attn_check_shape(const char* fn, int64_t B, int64_t S, int64_t H, int64_t KVH, int64_t head_dim) {  // S = query rows
  LLX_REQUIRE(head_dim == HD, "%s: head_dim=%lld unsupported (only 128)", fn, (long long)head_dim);
  LLX_REQUIRE(B > 0 && S > 0 && H > 0 && KVH > 0 && H % KVH == 0, "%s: bad B/S/H/KVH", fn);
  return LLX_OK;
}
// the dropout entries' own operands (attn_fwd.hip): threshold = round(p * 65536), rng = device (seed, counter), stream_id per module
int attn_dropout_check(const char* fn, int64_t threshold, const void* rng, int64_t stream_id, int64_t B, int64_t H);
// raises the dynamic-LDS limit of every listed kernel to `bytes`; the first failure is returned
template <typename... K>
static inline hipError_t attn_lds_limit(int bytes, K... kernels) {
  hipError_t e = hipSuccess;
  for (const void* f : {(const void*)kernels...}) if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return e;
}
