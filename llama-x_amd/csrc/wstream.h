// What the two weight streams of the decode step share: gemv_kernel (decode.hip: 1-4 activation rows, fp32 FMA in the vector pipe, bf16
// or int8 weights, LoRA) and rows16_kernel / rows16_combine_kernel (decode_rows.hip: 2-16 rows on the matrix pipe, bf16 or dynamic
// int8 weights).  Both compute
//   out[M, N] = epilogue( [rmsnorm(x) | x][M, K] . [W0; W1; W2]^T )
// and differ only in how a group of output features is summed.  Here: the constants (epilogues, weight kinds), the operand block, the norm-on-load pieces, the
// epilogue (one place where the roundings of the four epilogues live) and the host-side checks and fill of the operand block.
#pragma once
#include "common.h"  // HD
#include "kv8.h"     // q() of the FP8 KV cache
#include <type_traits>

// epilogue 0: out [M, N] | 1: + res [M, N] | 2 (q|k|v): rows [0, n_q) RoPE -> out [M, n_q]; [n_q, n_q + n_k) RoPE -> k cache; rest ->
// v cache | 3 (gate|up = W0|W1, N = 2 n_0): out [M, N/2] = silu(gate) * up | 4: epilogue 2 into FP8 caches (uint8 E4M3 codes, DESIGN
// 8.21; cache strides in bytes): the k / v branch stores q() of the bf16 values epilogue 2 would have stored, q rows are unchanged
enum { GV_NONE = 0, GV_RESIDUAL = 1, GV_QKV = 2, GV_SWIGLU = 3, GV_QKV_F8 = 4 };
static inline bool gv_is_qkv(int epilogue) { return epilogue == GV_QKV || epilogue == GV_QKV_F8; }
// weight kind: bf16 | int8 rows x bf16 activations (weight-only) | int8 rows x int8 activations quantised in the prologue (dynamic)
enum { WK_BF16 = 0, WK_I8W = 1, WK_I8D = 2 };

struct StreamArgs {
  const bf16_t* W[3]; int64_t ldw[3]; int seg_end[3];  // output rows [seg_end[s-1], seg_end[s]) come from W[s] (row-major [rows, K])
  const bf16_t* wscale[3];                              // int8 kinds: per-row scales of W[s] (W[s] then points at int8 rows, ldw in bytes);
                                                        // bf16 rows in gemv_kernel: DoRA's per-row factors m / ||W + s B A|| (null: none)
  const bf16_t* x; int64_t ldx;                         // [M, K]
  const bf16_t* norm_w; float eps;                      // NORM: x <- rmsnorm(x) * norm_w, rounded to bf16 (nn.RMSNorm, single rounding)
  int M, N, K;
  bf16_t* out; int64_t ldo;                             // NONE / RESIDUAL: [M, N]; QKV: q rows [M, n_q]; SWIGLU: h [M, N / 2]
  const bf16_t* res; int64_t ldr;                       // RESIDUAL: [M, N]
  const float* rope; int n_q, n_k;                      // QKV: rows [0, n_q) = q heads, [n_q, n_q + n_k) = k heads, then v; table [.., 64, 2]
  bf16_t* kc; bf16_t* vc; int64_t c_sh, c_ss;           //      caches [.., KVH, Smax, 128] through (head, position) strides (QKV_F8: uint8
                                                        //      codes behind the same pointers, strides in bytes)
  const int64_t* pos;                                   //      the cache position of every activation row
};

// ---- the GEMV (gemv_kernel of decode.hip, gemv_mx4_kernel of mxfp4.hip): its operand block and the pieces both kernels are made of
struct GemvArgs : StreamArgs {  // QKV: table row m and cache position pos[m] for activation row m, caches of batch 1
  // LoRA (modelling/lora.py:43): out += scale * (t . Bext[row]) with t = x . A^T computed by a previous launch of this kernel
  const bf16_t* bext[3]; int64_t ldb[3]; int t_off[3]; int rank[3];
  const bf16_t* t; int64_t ldt; float lora_scale;
};

__device__ __forceinline__ float dot8(const u32x4_t& w, const float (&xf)[8]) {
  float s = bflo(w[0]) * xf[0];
  s = __builtin_fmaf(bfhi(w[0]), xf[1], s);
  s = __builtin_fmaf(bflo(w[1]), xf[2], s);
  s = __builtin_fmaf(bfhi(w[1]), xf[3], s);
  s = __builtin_fmaf(bflo(w[2]), xf[4], s);
  s = __builtin_fmaf(bfhi(w[2]), xf[5], s);
  s = __builtin_fmaf(bflo(w[3]), xf[6], s);
  s = __builtin_fmaf(bfhi(w[3]), xf[7], s);
  return s;
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// Sum over the 64 lanes, every lane gets it, all in the vector pipe: DPP inside the rows of 16 (quad swaps, half mirror, mirror), then
// v_permlane16_swap / v_permlane32_swap pair the rows (common.h's wave_sum takes six trips through the LDS crossbar; other sum order).
__device__ __forceinline__ float wave_sum_valu(float v) {
  v += dpp_f32<0xB1>(v);
  v += dpp_f32<0x4E>(v);
  v += dpp_f32<0x141>(v);
  v += dpp_f32<0x140>(v);
  // (__uint_as_float on the elements, not __builtin_bit_cast: hipcc 7.2 reads element 0 for BOTH halves of the pair through bit_cast)
  const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
  const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
}

// ---- norm on load: the pieces of x <- bf16(x * rstd * norm_w) on 8 packed bf16 elements
__device__ __forceinline__ float sumsq8(const u32x4_t& v, float ss) {
#pragma unroll
  for (int e = 0; e < 4; ++e) ss += bflo(v[e]) * bflo(v[e]) + bfhi(v[e]) * bfhi(v[e]);
  return ss;
}
__device__ __forceinline__ u32x4_t norm8(u32x4_t v, float rstd, const bf16_t* norm_w) {
  const u32x4_t w = *reinterpret_cast<const u32x4_t*>(norm_w);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = pack_bf2(bflo(v[e]) * rstd * bflo(w[e]), bfhi(v[e]) * rstd * bfhi(w[e]));
  return v;
}

// ---- the epilogue of NV (2 or 4) consecutive output features of activation row m, starting at feature row0 (SwiGLU: at hidden unit
// row0).  v: the linear's outputs, already rounded to bf16; SwiGLU: v[0 .. NV/2) gates, v[NV/2 .. NV) ups of the same units.
// q|k|v: rope_row = the RoPE table row of this activation row, kv_off() = the element offset of its (batch slot, position) in the
// caches; negative: the k / v heads of this row are not written.  (A callable, so that the position is read where the parent
// kernels read it, after the rotation: as a value it cost the q|k|v instances of decode_rows.hip two VGPRs.)
template <int EPI, int NV, class KvOff>
__device__ __forceinline__ void stream_epilogue(const StreamArgs& a, int row0, int m, const float* rope_row, KvOff&& kv_off, float (&v)[4]) {
  static_assert(NV == 2 || NV == 4, "features per call");
  if constexpr (EPI == GV_SWIGLU) {
    // h = silu(g) * u with the roundings of the bf16 eager graph (modelling/llama.py:150-152), as swiglu_fwd8
    const int half = a.N / 2;
#pragma unroll
    for (int j = 0; j < NV / 2; ++j) {
      const float gg = v[j], uu = v[NV / 2 + j];
      const float sg = bf2f(f2bf(gg * sigmoidf_(gg)));
      if (row0 + j < half) a.out[(int64_t)m * a.ldo + row0 + j] = f2bf(sg * uu);
    }
  } else if constexpr (EPI == GV_QKV || EPI == GV_QKV_F8) {
    // apply_rope on q and k (modelling/llama.py:63-73,122-123), then KVCache.update (:83-90) for k and v
    const bool is_q = row0 < a.n_q, is_k = !is_q && row0 < a.n_q + a.n_k;
    const int hrow = is_q ? row0 : (is_k ? row0 - a.n_q : row0 - a.n_q - a.n_k);
    const int d = hrow & (HD - 1);
    if (is_q || is_k) {
      const float* tp = rope_row + (d >> 1) * 2;
      const float c0 = tp[0], s0 = tp[1], c1 = NV == 4 ? tp[2] : 1.f, s1 = NV == 4 ? tp[3] : 0.f;
      const float y0 = v[0] * c0 - v[1] * s0, y1 = v[1] * c0 + v[0] * s0, y2 = v[2] * c1 - v[3] * s1, y3 = v[3] * c1 + v[2] * s1;
      v[0] = y0; v[1] = y1; v[2] = y2; v[3] = y3;
    }
    u32x2_t pk;
    pk[0] = pack_bf2(v[0], v[1]);
    pk[1] = pack_bf2(v[2], v[3]);
    auto store = [&](bf16_t* dst) {
      if constexpr (NV == 4) *reinterpret_cast<u32x2_t*>(dst) = pk;
      else *reinterpret_cast<uint32_t*>(dst) = pk[0];  // one rotation pair
    };
    if (is_q) {
      store(a.out + (int64_t)m * a.ldo + row0);
    } else {
      const int64_t off = kv_off();
      if constexpr (EPI == GV_QKV_F8) {
        // the FP8 cache: q() of the rounded values above (fp32 -> bf16 -> E4M3, the double rounding of the format's contract), one 4-byte
        // (one pair: 2-byte) store at byte offsets
        if (off >= 0) {
          uint8_t* dst = reinterpret_cast<uint8_t*>(is_k ? a.kc : a.vc) + (int64_t)(hrow >> 7) * a.c_sh + off + d;
          if constexpr (NV == 4) *reinterpret_cast<uint32_t*>(dst) = kv8_encode_bf4(pk[0], pk[1]);
          else *reinterpret_cast<uint16_t*>(dst) = (uint16_t)kv8_encode2(bflo(pk[0]), bfhi(pk[0]));
        }
      } else {
        if (off >= 0) store((is_k ? a.kc : a.vc) + (int64_t)(hrow >> 7) * a.c_sh + off + d);
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < NV; ++r) {
      if (row0 + r < a.N) {
        float o = v[r];
        if constexpr (EPI == GV_RESIDUAL) o += bf2f(a.res[(int64_t)m * a.ldr + row0 + r]);  // bf16 output + bf16 residual, rounded
        a.out[(int64_t)m * a.ldo + row0 + r] = f2bf(o);
      }
    }
  }
}

// ---- host: the operands the eight entry points of the two streams have in common, as they arrive over the C ABI (include/llx.h); c_sb
// and Smax are the batched stream's, 0 for the GEMVs.  Every entry point fills one of these, once, and hands it on.
struct StreamCall {
  const void* w[3]; int64_t ldw[3], n[3];
  const void* x; int64_t ldx, M, K;
  const void* norm_w; float eps; int epilogue;
  void* out; int64_t ldo; const void* res; int64_t ldr;
  const float* rope; int64_t n_q, n_k;
  void* k_cache; void* v_cache; int64_t c_sb, c_sh, c_ss, Smax; const int64_t* pos;
};
// the adapter operands of both streams: bext_s bf16 [n_s, rank_s] row-major, t bf16 [M, sum rank] (row stride ldt), colscale_s bf16 [n_s]
// = DoRA's cached row factors where they come with the adapter (the _lora entry points of the batched stream; all null: LoRA)
struct StreamLora {
  const void* bext[3]; int64_t rank[3]; const void* t; int64_t ldt; float scale; const void* colscale[3];
};

// ---- host: the checks every entry point of the two streams makes on the common operands, then their fill into `a`.  fn = the entry
// point's name (every message begins with it); m_lo .. m_hi = its row counts (m_note says where other counts go); epl = weight
// elements per 16-byte load (K and the weight row strides are multiples of it); seg_gran = what the inner segments' row counts must
// be multiples of (a row group or tile never straddles two weights).  W[] / ldw[] of absent segments repeat segment 0, seg_end[] of
// the last present segment is N.
static inline int stream_check_fill(const char* fn, StreamArgs& a, int m_lo, int m_hi, const char* m_note, int epl, int seg_gran, const StreamCall& c) {
  const int64_t n0 = c.n[0], n1 = c.n[1], n2 = c.n[2], N = n0 + n1 + n2;
  const void *w0 = c.w[0], *w1 = c.w[1], *w2 = c.w[2];
  LLX_REQUIRE(w0 && c.x && c.out, "%s: null pointer", fn);
  LLX_REQUIRE(c.M >= m_lo && c.M <= m_hi, "%s: M=%lld outside %d..%d (%s)", fn, (long long)c.M, m_lo, m_hi, m_note);
  LLX_REQUIRE(c.K > 0 && c.K % epl == 0 && c.K <= 32768, "%s: K=%lld must be a multiple of %d and at most 32768", fn, (long long)c.K, epl);
  LLX_REQUIRE(c.epilogue >= GV_NONE && c.epilogue <= GV_QKV_F8, "%s: unknown epilogue %d", fn, c.epilogue);
  LLX_REQUIRE(n0 > 0 && n1 >= 0 && n2 >= 0 && (w1 || n1 == 0) && (w2 || n2 == 0) && (n1 > 0 || n2 == 0), "%s: bad segment sizes", fn);
  LLX_REQUIRE((n1 == 0 || n0 % seg_gran == 0) && (n2 == 0 || n1 % seg_gran == 0), "%s: inner segment sizes must be multiples of %d", fn, seg_gran);
  LLX_REQUIRE(c.ldw[0] % epl == 0 && c.ldw[1] % epl == 0 && c.ldw[2] % epl == 0 && c.ldx % 8 == 0, "%s: row strides must be multiples of 16 bytes", fn);
  LLX_REQUIRE(((uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)c.x | (uintptr_t)c.norm_w) % 16 == 0, "%s: pointers must be 16-byte aligned", fn);
  LLX_REQUIRE(N < (1 << 30), "%s: too many rows", fn);
  LLX_REQUIRE(c.epilogue != GV_RESIDUAL || c.res, "%s: residual missing", fn);
  LLX_REQUIRE(c.epilogue != GV_SWIGLU || (n0 == n1 && n2 == 0 && w1), "%s: the SwiGLU epilogue takes gate and up weights of equal size", fn);
  // (epilogue 4: the caches hold one byte per element, so the same "4 elements" rule is 4-byte alignment of pointers and byte strides)
  LLX_REQUIRE(!gv_is_qkv(c.epilogue) ||
                  (c.rope && c.k_cache && c.v_cache && c.pos && c.n_q % HD == 0 && c.n_k % HD == 0 && (N - c.n_q - c.n_k) % HD == 0 && c.n_q + c.n_k <= N &&
                   (uintptr_t)c.rope % 8 == 0 && (uintptr_t)c.out % 8 == 0 &&
                   ((uintptr_t)c.k_cache | (uintptr_t)c.v_cache) % (c.epilogue == GV_QKV_F8 ? 4 : 8) == 0 && c.ldo % 4 == 0 && c.c_sh % 4 == 0 && c.c_ss % 4 == 0),
              "%s: bad q|k|v epilogue arguments (the RoPE table, both caches and the positions; whole heads of 128; 8-byte aligned rows)", fn);
  a.W[0] = (const bf16_t*)w0; a.W[1] = (const bf16_t*)(w1 ? w1 : w0); a.W[2] = (const bf16_t*)(w2 ? w2 : w0);
  a.ldw[0] = c.ldw[0]; a.ldw[1] = w1 ? c.ldw[1] : c.ldw[0]; a.ldw[2] = w2 ? c.ldw[2] : c.ldw[0];
  a.seg_end[0] = (int)n0; a.seg_end[1] = (int)(n0 + n1); a.seg_end[2] = (int)N;
  if (n1 == 0) { a.seg_end[0] = a.seg_end[1] = (int)N; }  // single source: every row is segment 0
  else if (n2 == 0) { a.seg_end[1] = (int)N; }
  a.x = (const bf16_t*)c.x; a.ldx = c.ldx; a.norm_w = (const bf16_t*)c.norm_w; a.eps = c.eps;
  a.M = (int)c.M; a.N = (int)N; a.K = (int)c.K;
  a.out = (bf16_t*)c.out; a.ldo = c.ldo; a.res = (const bf16_t*)c.res; a.ldr = c.ldr;
  a.rope = c.rope; a.n_q = (int)c.n_q; a.n_k = (int)c.n_k; a.kc = (bf16_t*)c.k_cache; a.vc = (bf16_t*)c.v_cache;
  a.c_sh = c.c_sh; a.c_ss = c.c_ss; a.pos = c.pos;
  a.wscale[0] = a.wscale[1] = a.wscale[2] = nullptr;
  return LLX_OK;
}

// ---- host: the per-row scales ws[0..2] of int8 weights, or the per-row DoRA factors of bf16 weights (bf16 [n_s]; what = "int8" | "DoRA"),
// after stream_check_fill; scales of absent segments repeat segment 0
static inline int stream_check_fill_scales(const char* fn, StreamArgs& a, const char* what, const StreamCall& c, const void* const* ws) {
  LLX_REQUIRE(ws[0] && (ws[1] || c.n[1] == 0) && (ws[2] || c.n[2] == 0), "%s: null scale (every %s weight needs its per-row scales)", fn, what);
  LLX_REQUIRE(((uintptr_t)ws[0] | (uintptr_t)ws[1] | (uintptr_t)ws[2]) % 2 == 0, "%s: scale pointers must be 2-byte aligned", fn);
  for (int s = 0; s < 3; ++s) a.wscale[s] = (const bf16_t*)(ws[s] ? ws[s] : ws[0]);
  return LLX_OK;
}

// ---- host: the LoRA operands of a GEMV (nullable bext_s [n_s, rank_s], t [M, sum rank] bf16, offsets into t by segment), after stream_check_fill
static inline int gemv_check_fill_lora(const char* fn, GemvArgs& a, const StreamCall& c, const StreamLora& lo) {
  const int64_t* rank = lo.rank;
  const bool lora = lo.bext[0] || lo.bext[1] || lo.bext[2];
  LLX_REQUIRE(!lora || (lo.t && lo.ldt % 8 == 0 && (uintptr_t)lo.t % 16 == 0 && rank[0] % 8 == 0 && rank[1] % 8 == 0 && rank[2] % 8 == 0 && rank[0] <= 512 &&
                        rank[1] <= 512 && rank[2] <= 512 && ((uintptr_t)lo.bext[0] | (uintptr_t)lo.bext[1] | (uintptr_t)lo.bext[2]) % 16 == 0),
              "%s: bad LoRA operands (ranks must be multiples of 8, at most 512)", fn);
  for (int s = 0; s < 3; ++s) { a.bext[s] = (const bf16_t*)lo.bext[s]; a.ldb[s] = rank[s]; a.rank[s] = (int)rank[s]; }
  a.t_off[0] = 0; a.t_off[1] = (int)rank[0]; a.t_off[2] = (int)(rank[0] + rank[1]);
  a.t = (const bf16_t*)lo.t; a.ldt = lo.ldt; a.lora_scale = lo.scale;
  if (c.n[1] == 0 && lora) { a.bext[1] = a.bext[2] = a.bext[0]; a.ldb[1] = a.ldb[2] = a.ldb[0]; a.rank[1] = a.rank[2] = a.rank[0]; a.t_off[1] = a.t_off[2] = 0; }
  return LLX_OK;
}

// ---- host: the run-time epilogue of a call as a compile-time constant: f(std::integral_constant<int, GV_*>{}) launches the instance
// and returns the entry point's status (stream_check_fill has checked the range before a call comes here)
template <class F>
static inline int stream_with_epilogue(int epilogue, F&& f) {
  switch (epilogue) {
    case GV_NONE: return f(std::integral_constant<int, GV_NONE>{});
    case GV_RESIDUAL: return f(std::integral_constant<int, GV_RESIDUAL>{});
    case GV_QKV: return f(std::integral_constant<int, GV_QKV>{});
    case GV_QKV_F8: return f(std::integral_constant<int, GV_QKV_F8>{});
    default: return f(std::integral_constant<int, GV_SWIGLU>{});
  }
}

// ---- host: the launches of a GEMV (gemv_kernel, gemv_mx4_kernel), after the checks.
// Grid: rpw output rows (SwiGLU: rpw / 2 hidden units) make a row group, a wave walks row groups, four waves a workgroup; the wave count
// is trimmed so that every wave gets the same number of row groups where possible.
static inline int gemv_grid(int64_t N, int epilogue, int rpw) {
  const int64_t groups = epilogue == GV_SWIGLU ? cdiv64(N / 2, rpw / 2) : cdiv64(N, rpw);
  constexpr int wave_cap = 2048;
  const int64_t per_wave = cdiv64(groups, wave_cap);
  return (int)cdiv64(cdiv64(groups, per_wave), 4);
}
// Passes: the build for m rows stages MT = 1 | 2 | 4 rows of x in LDS, Kp elements of xb bytes each (the kernel's LDS row length).  Rows per
// pass: all of them where the kind has that build (max_pass = 4 | 2) and their stage fits 64 KiB, else pairs, else one; each pass streams
// the weights again, on its own rows of x / out / res / rope / pos / t.  launch(b, MT, lds): the launch of one pass.
template <class Args, class Launch>
static inline int gemv_passes(const char* fn, const Args& a, int max_pass, int64_t Kp, int64_t xb, Launch&& launch) {
  auto stage = [&](int64_t mt) { return mt * Kp * xb + 64; };
  auto fits = [&](int64_t mt) { return stage(mt) <= 64 * 1024; };
  int per_pass = a.M > 2 ? 4 : a.M;
  if (per_pass == 4 && (max_pass < 4 || !fits(4))) per_pass = 2;
  if (per_pass == 2 && !fits(2)) per_pass = 1;
  LLX_REQUIRE(fits(per_pass), "%s: K too large for the LDS stage", fn);
  for (int m0 = 0; m0 < a.M; m0 += per_pass) {
    const int mc = a.M - m0 < per_pass ? a.M - m0 : per_pass;
    Args b = a;
    b.M = mc;
    b.x = a.x + (int64_t)m0 * a.ldx;
    b.out = a.out + (int64_t)m0 * a.ldo;
    if (a.res) b.res = a.res + (int64_t)m0 * a.ldr;
    if (a.rope) b.rope = a.rope + (int64_t)m0 * 128;
    if (a.pos) b.pos = a.pos + m0;
    if (a.t) b.t = a.t + (int64_t)m0 * a.ldt;
    const int MT = mc == 1 ? 1 : (mc == 2 ? 2 : 4);
    const int rc = launch(b, MT, (size_t)stage(MT));
    if (rc != LLX_OK) return rc;
  }
  return LLX_OK;
}
