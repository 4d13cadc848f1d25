// Flash-style attention forward for head_dim 128, GQA by head indexing, masks from per-token metadata.
//
// Replaces F.scaled_dot_product_attention(..., enable_gqa=True) and flex_attention(block_mask=...) of the
// reference (modelling/llama.py:129-137).  Mask rule (bit-exact with the reference's mask functions):
//     allow(q, k) = (k <= q  ||  k < prefix_len[b])  &&  (doc_ids == null || doc_ids[b,q] == doc_ids[b,k])
//   * causal:       prefix_len = null, doc_ids = null        (is_causal=True, modelling/llama.py:135)
//   * document:     doc_ids given                            (mask_mod, train_metamathqa.py:67-68)
//   * prefix-LM:    prefix_len given                         (README.md:16 plan)
// Layout: q [B,S,H,128], k/v [B,S,KVH,128] with arbitrary batch/sequence strides (so views of a fused QKV
// projection work), o [B,S,H,128] contiguous per row, lse [B,H,S] fp32 in log2 units (for the backward).
//
// One workgroup = 4 waves = 128 query rows of one (batch, head); each wave owns 32 rows.  Per 64-key tile:
//   S^T = K.Q^T   (keys on accumulator rows, the query row on the lane -> softmax statistics are lane-local)
//   O^T += V^T.P^T (P^T taken straight from the S^T accumulator registers as the MFMA B operand; V^T fragments
//                   come from the row-major LDS tile through ds_read_b64_tr_b16)
// K/V tiles are double-buffered in LDS by global_load_lds with the bank swizzle applied on the source address.
#include "attn.h"
#include "attn_dropout.h"

#define KV_TILE_BYTES TILE_BYTES
#define ATT_STAGE_BYTES (2 * KV_TILE_BYTES)  // K + V
#define ATT_LDS_BYTES (2 * ATT_STAGE_BYTES)  // 64 KiB

struct AttnFwdArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o; float* lse;
  int64_t q_sb, q_ss, k_sb, k_ss, v_sb, v_ss, o_sb, o_ss;  // element strides (batch, sequence)
  const int* doc_ids;     // [B,S] or null
  const int* prefix_len;  // [B] or null
  const uint8_t* flags;   // [B, nqb, nkt] tile classes (0 skip, 1 partial, 2 full) or null => causal arithmetic
  int B, S, H, KVH;
  float scale_log2;       // softmax scale * log2(e)
  unsigned long long* stamps;  // diagnostic (normally null): s_memtime stamps of block (x=0,h=0,b=0), wave 0
  // dense-mask mode only (attn_mask_fwd_kernel; there S is the number of QUERY rows):
  int Skv;                // keys (the whole cache: max_seq_len)
  int64_t k_sh, v_sh;     // element stride between kv heads ([B,KVH,Smax,128] cache, or 128 for views of a q|k|v row buffer)
  const uint8_t* mask;    // [B | 1, Sq, Skv] bool / uint8, last dim dense; nonzero = attend
  int64_t m_sb, m_sq;     // mask strides in bytes (m_sb = 0: broadcast over the batch)
  // attention dropout only (attn_fwd_dropout_kernel; attn_dropout.h):
  const int64_t* rng;     // device: (seed, counter) - the ticket of this training step
  uint32_t drop_thr;      // t << 16, t = round(p * 65536): an element is dropped iff the top 16 bits of its word are below t
  float drop_c;           // 65536 / (65536 - t)
  int stream_id;          // one value per attention module
};

enum { ATT_CAUSAL = 0, ATT_GENERAL = 1, ATT_MASK = 2 };

// MODE ATT_CAUSAL: pure causal (no doc_ids / prefix_len / tile flags) - the mask is index arithmetic only.
// NW = waves per workgroup (32 query rows each).  A K/V tile pair is 32 KiB of LDS-DMA per workgroup and key tile, and a CU takes
// LDS-DMA fills at ~25-40 GB/s whatever their source (measured on the dQ-from-dS kernel, attn_bwd.hip): two 4-wave workgroups per CU
// ask for ~60 GB/s at this kernel's MFMA rate, ONE 8-wave workgroup (256 query rows sharing every tile) for half of that.
// ATT_GENERAL: doc_ids / prefix_len with tile flags.  ATT_MASK: a dense bool mask is the ONLY rule (no causal index arithmetic): Sq = a.S
// query rows against a.Skv keys, K/V with a head stride, tile classes from llx_attn_mask_tile_flags, a partly masked tile tests the
// mask bytes of the lane's own query row, and a row without any allowed key comes out NaN (SDPA's softmax of all -inf).
template <bool GENERAL_, bool STAMP = false, int NW = 8>
__global__ __launch_bounds__(64 * NW, 2) void attn_fwd_kernel(const AttnFwdArgs a) {
  static_assert(NW == 8, "NW stays a parameter only because bench.py, tools/ and profiles/ key on the symbol attn_fwd_kernel<*, *, 8>");
  constexpr int MODE = GENERAL_ ? ATT_GENERAL : ATT_CAUSAL;
  constexpr bool DROPOUT = false;
#include "attn_fwd_body.h"
}

// Training with attention dropout (llx_attn_fwd_dropout): the DROPOUT build of the same body, causal and rule mode.  A kernel of its
// own and not a fourth template argument of attn_fwd_kernel: that would rename the measured instances (see the static_assert above).
template <bool GENERAL_>
__global__ __launch_bounds__(512, 2) void attn_fwd_dropout_kernel(const AttnFwdArgs a) {
  constexpr int MODE = GENERAL_ ? ATT_GENERAL : ATT_CAUSAL, NW = 8;
  constexpr bool STAMP = false, DROPOUT = true;
#include "attn_fwd_body.h"
}

// KV-cache prefill / explicit bool mask (llx_attn_mask_fwd): the same tile loop, driven by the mask bytes.
__global__ __launch_bounds__(512, 2) void attn_mask_fwd_kernel(const AttnFwdArgs a) {
  constexpr int MODE = ATT_MASK, NW = 8;
  constexpr bool STAMP = false, DROPOUT = false;
#include "attn_fwd_body.h"
}

// Tile classes for non-causal-only masks: flags[b][qb][kt] = 0 (no pair allowed) | 1 (some) | 2 (all, no masking).
__global__ void attn_tile_flags_kernel(const int* __restrict__ doc_ids, const int* __restrict__ prefix_len, uint8_t* flags, int S,
                                       int nqb, int nkt) {
  __shared__ int s_any, s_all;
  const int kt = blockIdx.x, qb = blockIdx.y, b = blockIdx.z;
  if (threadIdx.x == 0) { s_any = 0; s_all = 1; }
  __syncthreads();
  const int P = prefix_len ? prefix_len[b] : 0;
  int any = 0, all = 1;
  for (int idx = threadIdx.x; idx < BQ * BKV; idx += blockDim.x) {
    const int qi = qb * BQ + idx / BKV, kk = kt * BKV + idx % BKV;
    if (qi >= S) continue;  // rows past the end do not constrain the class
    bool ok = (kk < S) && (kk <= qi || kk < P);
    if (ok && doc_ids) ok = doc_ids[(int64_t)b * S + qi] == doc_ids[(int64_t)b * S + kk];
    any |= ok; all &= ok;
  }
  if (any) atomicOr(&s_any, 1);
  if (!all) atomicAnd(&s_all, 0);
  __syncthreads();
  if (threadIdx.x == 0) flags[((int64_t)b * nqb + qb) * nkt + kt] = s_any ? (s_all ? 2 : 1) : 0;
}

extern "C" int64_t llx_attn_flags_bytes(int64_t B, int64_t S) { return B * cdiv64(S, BQ) * cdiv64(S, BKV); }

// flags: llx_attn_flags_bytes(B,S) bytes (device), filled here. Needed only when doc_ids or prefix_len is used.
extern "C" int llx_attn_tile_flags(const int* doc_ids, const int* prefix_len, void* flags, int64_t B, int64_t S, hipStream_t stream) {
  LLX_REQUIRE(flags && B > 0 && S > 0, "llx_attn_tile_flags: bad arguments");
  const int nqb = (int)cdiv64(S, BQ), nkt = (int)cdiv64(S, BKV);
  hipLaunchKernelGGL(attn_tile_flags_kernel, dim3(nkt, nqb, (unsigned)B), dim3(256), 0, stream, doc_ids, prefix_len, (uint8_t*)flags,
                     (int)S, nqb, nkt);
  LLX_LAUNCH_CHECK("llx_attn_tile_flags");
  return LLX_OK;
}

// The forward entries' common operands (S = query rows), checked and filled in; the fields of rule, mask and stamps stay zero.
static int attn_fwd_args(const char* fn, AttnFwdArgs& a, const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss,
                         const void* v, int64_t v_sb, int64_t v_ss, void* o, int64_t o_sb, int64_t o_ss, float* lse, int64_t B, int64_t S,
                         int64_t H, int64_t KVH, int64_t head_dim, float scale) {
  LLX_REQUIRE(q && k && v && o, "%s: null pointer", fn);
  if (int rc = attn_check_shape(fn, B, S, H, KVH, head_dim)) return rc;
  LLX_REQUIRE((q_ss % 8 | k_ss % 8 | v_ss % 8 | o_ss % 4 | q_sb % 8 | k_sb % 8 | v_sb % 8 | o_sb % 4) == 0, "%s: strides must keep 16-byte alignment", fn);
  LLX_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0 && (uintptr_t)o % 8 == 0, "%s: unaligned pointer", fn);
  a = {};
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)o; a.lse = lse;
  a.q_sb = q_sb; a.q_ss = q_ss; a.k_sb = k_sb; a.k_ss = k_ss; a.v_sb = v_sb; a.v_ss = v_ss; a.o_sb = o_sb; a.o_ss = o_ss;
  a.B = (int)B; a.S = (int)S; a.H = (int)H; a.KVH = (int)KVH;
  a.scale_log2 = scale * 1.4426950408889634f;
  return LLX_OK;
}

// Any forward instance: 8 waves per 256 query rows of a (head, batch).  The static is initialised once, by one thread (checkpointing enters from several).
static int attn_fwd_launch(const char* fn, void (*kernel)(const AttnFwdArgs), const AttnFwdArgs& a, hipStream_t stream) {
  static const hipError_t err = attn_lds_limit(ATT_LDS_BYTES, attn_fwd_kernel<false, false, 8>, attn_fwd_kernel<true, false, 8>,
                                               attn_fwd_kernel<false, true, 8>, attn_mask_fwd_kernel, attn_fwd_dropout_kernel<false>,
                                               attn_fwd_dropout_kernel<true>);
  if (err != hipSuccess) { llx_set_error("%s: %s", fn, hipGetErrorString(err)); return LLX_ERR_LAUNCH; }
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.H, (unsigned)cdiv64(a.S, 256), (unsigned)a.B), dim3(512), ATT_LDS_BYTES, stream, a);
  LLX_LAUNCH_CHECK(fn);
  return LLX_OK;
}

// strides are in elements: *_sb per batch, *_ss per sequence position; head h starts at element h*128 of a row.
extern "C" int llx_attn_fwd(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss, const void* v,
                            int64_t v_sb, int64_t v_ss, void* o, int64_t o_sb, int64_t o_ss, float* lse, const int* doc_ids,
                            const int* prefix_len, const void* flags, int64_t B, int64_t S, int64_t H, int64_t KVH, int64_t head_dim,
                            float scale, hipStream_t stream) {
  AttnFwdArgs a;
  if (int rc = attn_fwd_args("llx_attn_fwd", a, q, q_sb, q_ss, k, k_sb, k_ss, v, v_sb, v_ss, o, o_sb, o_ss, lse, B, S, H, KVH, head_dim, scale)) return rc;
  LLX_REQUIRE(!(doc_ids || prefix_len) || flags, "llx_attn_fwd: tile flags required with doc_ids/prefix_len");
  a.doc_ids = doc_ids; a.prefix_len = prefix_len; a.flags = (doc_ids || prefix_len) ? (const uint8_t*)flags : nullptr;
  LLX_REQUIRE(S < (1 << 24), "llx_attn_fwd: S too large");
  return attn_fwd_launch("llx_attn_fwd", a.flags ? attn_fwd_kernel<true, false, 8> : attn_fwd_kernel<false, false, 8>, a, stream);
}

// The operands that the dropout entries (forward, backward, keep bytes) share: threshold = t = round(p * 65536), rng = device (seed, counter).
int attn_dropout_check(const char* fn, int64_t threshold, const void* rng, int64_t stream_id, int64_t B, int64_t H) {
  LLX_REQUIRE(rng && (uintptr_t)rng % 8 == 0, "%s: rng must be a device pointer to two int64 (seed, counter)", fn);
  LLX_REQUIRE(threshold > 0 && threshold < 65536, "%s: threshold=%lld out of range (0 < round(p * 65536) < 65536)", fn, (long long)threshold);
  LLX_REQUIRE(stream_id >= 0 && stream_id < (1ll << 31), "%s: stream_id=%lld out of range", fn, (long long)stream_id);
  LLX_REQUIRE(B < 65536 && H < 65536, "%s: B and H must stay below 65536 (the mask key takes 16 bits of each)", fn);
  return LLX_OK;
}

// llx_attn_fwd with attention dropout (SDPA's dropout_p in training): the same operands, then threshold = round(p * 65536), rng = device
// pointer to (seed, counter) as int64, stream_id = one value per attention module.  lse is that of the undropped rows.
extern "C" int llx_attn_fwd_dropout(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss, const void* v,
                                    int64_t v_sb, int64_t v_ss, void* o, int64_t o_sb, int64_t o_ss, float* lse, const int* doc_ids,
                                    const int* prefix_len, const void* flags, int64_t B, int64_t S, int64_t H, int64_t KVH, int64_t head_dim,
                                    float scale, int64_t threshold, const void* rng, int64_t stream_id, hipStream_t stream) {
  AttnFwdArgs a;
  if (int rc = attn_fwd_args("llx_attn_fwd_dropout", a, q, q_sb, q_ss, k, k_sb, k_ss, v, v_sb, v_ss, o, o_sb, o_ss, lse, B, S, H, KVH, head_dim, scale)) return rc;
  if (int rc = attn_dropout_check("llx_attn_fwd_dropout", threshold, rng, stream_id, B, H)) return rc;
  LLX_REQUIRE(!(doc_ids || prefix_len) || flags, "llx_attn_fwd_dropout: tile flags required with doc_ids/prefix_len");
  LLX_REQUIRE(S < (1 << 24), "llx_attn_fwd_dropout: S too large");
  a.doc_ids = doc_ids; a.prefix_len = prefix_len; a.flags = (doc_ids || prefix_len) ? (const uint8_t*)flags : nullptr;
  a.rng = (const int64_t*)rng; a.drop_thr = (uint32_t)threshold << 16; a.drop_c = 65536.f / (float)(65536 - threshold); a.stream_id = (int)stream_id;
  return attn_fwd_launch("llx_attn_fwd_dropout", a.flags ? attn_fwd_dropout_kernel<true> : attn_fwd_dropout_kernel<false>, a, stream);
}

// keep[b, h, q, k] = 1 where attention dropout keeps the element, 0 where it drops it: the bytes of the mask that llx_attn_fwd_dropout /
// llx_attn_bwd_dropout apply with the same (threshold, rng, stream_id), written out (tests; inspection).
__global__ __launch_bounds__(256) void attn_dropout_keep_kernel(uint8_t* __restrict__ keep, const int64_t* __restrict__ rng, int stream_id,
                                                               uint32_t thr16, int H, int Sq, int Skv, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % Skv);
  int64_t r = idx / Skv;
  const int q = (int)(r % Sq);
  r /= Sq;
  keep[idx] = attn_dropout_keep(rng[0], rng[1], stream_id, (int)(r / H), (int)(r % H), q, k, thr16) ? 1 : 0;
}

extern "C" int llx_attn_dropout_keep(void* keep, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t threshold, const void* rng,
                                     int64_t stream_id, hipStream_t stream) {
  LLX_REQUIRE(keep && B > 0 && H > 0 && Sq > 0 && Skv > 0, "llx_attn_dropout_keep: bad arguments");
  if (int rc = attn_dropout_check("llx_attn_dropout_keep", threshold, rng, stream_id, B, H)) return rc;
  LLX_REQUIRE(Sq < (1 << 24) && Skv < (1 << 24), "llx_attn_dropout_keep: Sq or Skv too large");
  const int64_t total = B * H * Sq * Skv;
  LLX_REQUIRE(cdiv64(total, 256) < (1ll << 31), "llx_attn_dropout_keep: too many elements");
  hipLaunchKernelGGL(attn_dropout_keep_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, stream, (uint8_t*)keep, (const int64_t*)rng,
                     (int)stream_id, (uint32_t)threshold << 16, (int)H, (int)Sq, (int)Skv, total);
  LLX_LAUNCH_CHECK("llx_attn_dropout_keep");
  return LLX_OK;
}

// Tile classes of a dense bool mask [B | 1, Sq, Skv] (row stride m_sq, batch stride m_sb, bytes): the layout llx_attn_tile_flags writes,
// 128-row blocks x 64-key tiles.  One workgroup per (key tile, row block, batch) reads its 128 x 64 bytes once, 4 at a time (rows have
// any alignment: unaligned dword loads; the group at a row's ragged end is read 4 bytes before the end and shifted, as in the kernel).
// Rows past Sq do not constrain the class; keys past Skv count as masked, so a ragged tile is never class 2.
__global__ __launch_bounds__(256) void attn_mask_tile_flags_kernel(const uint8_t* __restrict__ mask, int64_t m_sb, int64_t m_sq,
                                                                  uint8_t* __restrict__ flags, int Sq, int Skv, int nqb, int nkt) {
  __shared__ int s_any, s_all;
  const int kt = blockIdx.x, qb = blockIdx.y, b = blockIdx.z;
  if (threadIdx.x == 0) { s_any = 0; s_all = 1; }
  __syncthreads();
  const uint8_t* mb = mask + (int64_t)b * m_sb;
  const int n_in = min(BKV, Skv - kt * BKV);  // keys of this tile inside the mask
  int any = 0, all = (n_in == BKV);
  for (int idx = threadIdx.x; idx < BQ * (BKV / 4); idx += blockDim.x) {
    const int qi = qb * BQ + idx / (BKV / 4), g0 = kt * BKV + 4 * (idx % (BKV / 4));
    if (qi >= Sq || g0 >= Skv) continue;
    const int off = min(g0, Skv - 4), n = min(4, Skv - g0);  // n valid bytes, at the top of the word when the group was moved back
    uint32_t w;
    __builtin_memcpy(&w, mb + (int64_t)qi * m_sq + off, 4);
    w >>= 8 * (g0 - off);
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) cnt += (i < n && ((w >> (8 * i)) & 0xffu) != 0) ? 1 : 0;
    any |= cnt > 0; all &= cnt == n;
  }
  // LDS atomics (no atomics on global memory)
  if (any) atomicOr(&s_any, 1);
  if (!all) atomicAnd(&s_all, 0);
  __syncthreads();
  if (threadIdx.x == 0) flags[((int64_t)b * nqb + qb) * nkt + kt] = s_any ? (s_all ? 2 : 1) : 0;
}

extern "C" int64_t llx_attn_mask_flags_bytes(int64_t B, int64_t Sq, int64_t Skv) { return B * cdiv64(Sq, BQ) * cdiv64(Skv, BKV); }

// flags: llx_attn_mask_flags_bytes(B, Sq, Skv) bytes (device), filled here from the mask; m_sb / m_sq in bytes, m_sb = 0 broadcasts.
extern "C" int llx_attn_mask_tile_flags(const void* mask, int64_t m_sb, int64_t m_sq, void* flags, int64_t B, int64_t Sq, int64_t Skv,
                                        hipStream_t stream) {
  LLX_REQUIRE(mask && flags && B > 0 && Sq > 0, "llx_attn_mask_tile_flags: bad arguments");
  LLX_REQUIRE(Skv >= 4 && Skv < (1 << 24) && Sq < (1 << 24) && B < 65536, "llx_attn_mask_tile_flags: Skv=%lld (>= 4) / Sq=%lld / B=%lld out of range",
              (long long)Skv, (long long)Sq, (long long)B);
  LLX_REQUIRE(m_sq >= Skv && m_sb >= 0, "llx_attn_mask_tile_flags: mask rows overlap");
  const int nqb = (int)cdiv64(Sq, BQ), nkt = (int)cdiv64(Skv, BKV);
  hipLaunchKernelGGL(attn_mask_tile_flags_kernel, dim3(nkt, nqb, (unsigned)B), dim3(256), 0, stream, (const uint8_t*)mask, m_sb, m_sq,
                     (uint8_t*)flags, (int)Sq, (int)Skv, nqb, nkt);
  LLX_LAUNCH_CHECK("llx_attn_mask_tile_flags");
  return LLX_OK;
}

// SDPA(q, k, v, mask, is_causal=False, enable_gqa=True) through the MFMA tile loop: q / o rows [B, Sq, H*128] (batch, position strides;
// head h at h*128), k / v [B, KVH, Skv, 128] through (batch, head, position) strides, mask / flags as llx_attn_mask_tile_flags.
extern "C" int llx_attn_mask_fwd(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                                 const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, void* o, int64_t o_sb, int64_t o_ss, float* lse,
                                 const void* mask, int64_t m_sb, int64_t m_sq, const void* flags, int64_t B, int64_t Sq, int64_t Skv,
                                 int64_t H, int64_t KVH, int64_t head_dim, float scale, hipStream_t stream) {
  AttnFwdArgs a;
  if (int rc = attn_fwd_args("llx_attn_mask_fwd", a, q, q_sb, q_ss, k, k_sb, k_ss, v, v_sb, v_ss, o, o_sb, o_ss, lse, B, Sq, H, KVH, head_dim, scale)) return rc;
  LLX_REQUIRE(B < 65536, "llx_attn_mask_fwd: bad B/Sq/H/KVH");
  LLX_REQUIRE(Skv >= 4 && Skv < (1 << 24) && Sq < (1 << 24), "llx_attn_mask_fwd: Skv=%lld (>= 4) / Sq=%lld out of range", (long long)Skv, (long long)Sq);
  LLX_REQUIRE((k_sh % 8 | v_sh % 8) == 0, "llx_attn_mask_fwd: strides must keep 16-byte alignment");
  LLX_REQUIRE(k_ss >= 0 && v_ss >= 0 && k_ss < (1 << 24) && v_ss < (1 << 24), "llx_attn_mask_fwd: K/V position stride out of range");
  LLX_REQUIRE(mask && flags, "llx_attn_mask_fwd: null pointer");
  LLX_REQUIRE(m_sq >= Skv && m_sb >= 0, "llx_attn_mask_fwd: mask rows overlap");
  a.flags = (const uint8_t*)flags; a.Skv = (int)Skv; a.k_sh = k_sh; a.v_sh = v_sh; a.mask = (const uint8_t*)mask; a.m_sb = m_sb; a.m_sq = m_sq;
  return attn_fwd_launch("llx_attn_mask_fwd", attn_mask_fwd_kernel, a, stream);
}

// Diagnostic: resident workgroups per CU the runtime grants the forward kernel (occupancy API; advisory).
extern "C" int llx_debug_attn_fwd_occupancy(void) {
  int n = -1;
  hipFuncSetAttribute((const void*)attn_fwd_kernel<false, false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, ATT_LDS_BYTES);
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)attn_fwd_kernel<false, false, 8>, 512, ATT_LDS_BYTES);
  if (e != hipSuccess) { llx_set_error("occupancy query: %s", hipGetErrorString(e)); return -1; }
  return n;
}

// Diagnostic build of the forward kernel with in-kernel s_memtime stamps (5 per key tile) for one wave; timing only.
extern "C" int llx_debug_attn_fwd_stamps(const void* q, const void* k, const void* v, void* o, int64_t S, int64_t H, int64_t KVH,
                                         unsigned long long* stamps, hipStream_t stream) {
  AttnFwdArgs a;
  if (int rc = attn_fwd_args("llx_debug_attn_fwd_stamps", a, q, S * H * HD, H * HD, k, S * KVH * HD, KVH * HD, v, S * KVH * HD, KVH * HD, o,
                             S * H * HD, H * HD, nullptr, 1, S, H, KVH, HD, 0.08838834764f)) return rc;
  a.stamps = stamps;
  return attn_fwd_launch("llx_debug_attn_fwd_stamps", attn_fwd_kernel<false, true, 8>, a, stream);
}
