// Decode path (inference with a KV cache, a handful of query tokens per call): modelling/llama.py:76-90 (KVCache), :126-127,:135-137
// (cached keys/values through SDPA with the row-gathered causal mask), :189-194,:205-207 (Llama.forward with input_pos).
//
// Every linear of a decode step is a weight stream: M <= 4 activation rows against [N, K] bf16 weights that are read exactly once.
// The 256 x 256 MFMA tile kernel of gemm_bf16.hip covers such a product with N/256 workgroups (16-112 of 256 CUs); here
//   * gemv_kernel: all CUs stream weight rows (16 B per lane, whole 1-KiB row pieces per wave-instruction, non-temporal, 8 loads in
//     flight per lane), the activation row sits in LDS (optionally RMS-normalised on the way in: the norm of an 8-KiB row is cheaper
//     to redo per workgroup than a launch), fp32 FMA dot products, wave butterfly reduce, and the neighbours of the reference's call
//     sites in the epilogue: + residual | apply_rope on q,k + scatter of k,v into the caches | SwiGLU;
//   * attn_decode_kernel: the cache of one kv head is split over workgroups (>= 256 at B = 1), the G query heads of the group (x the
//     query tokens of the call) are served from ONE read of K and V, rows are loaded coalesced (16 lanes x 16 B = one 256-B row),
//     partial (m, l, o) per wave are merged by attn_decode_combine_kernel;
//   * mask_extent_kernel: the number of leading keys any query row may attend to (the mask is a bool tensor - the reference gathers
//     rows of its tril matrix, :194,:205 - so the extent is data; it stays on the device and sizes the key ranges of the workgroups);
//   * kv_scatter_kernel: KVCache.update (:83-90) for calls that do not go through the fused projection.
// int8 weights (subclasses/int8.py:106-121) stream through the same kernel at one byte per element: weight-only (bf16 activations,
// bytes sign-extended to fp32, EPI_COLSCALE's rounding points) and dynamic (the prologue quantises the activation rows as
// int8_quant.hip does, v_dot4c_i32_i8 into int32, EPI_ROWCOLSCALE's dequantisation).
// HBM-bound: the step moves (weights + live K/V) bytes once; bench.py --config decode reports that against the 8 TB/s peak.
// The operand block, the norm-on-load pieces, the epilogues and the host-side operand checks of gemv_kernel are wstream.h's, shared
// with the batched stream of decode_rows.hip.
#include "wstream.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------- weight-streaming GEMV
// (the weight kinds WK_*, the per-row scale pointers of the int8 kinds, GemvArgs with its LoRA operands, dot8 and wave_sum_valu are
// wstream.h's: the MXFP4 GEMV of mxfp4.hip is built from the same pieces)

// 16 int8 weights (sign-extended to fp32: one v_cvt_f32_i32 with a byte selector each) against 16 fp32 activations, chained onto s
__device__ __forceinline__ float dot16_i8(const u32x4_t& w, const float (&xf)[16], float s) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int b = 0; b < 4; ++b) s = __builtin_fmaf((float)(signed char)(w[e] >> (8 * b)), xf[4 * e + b], s);
  }
  return s;
}

// the same butterfly on int32 (the dynamic int8 kind: integer sums are exact in any order)
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ int wave_sum_valu_i(int v) {
  v += dpp_i32<0xB1>(v);
  v += dpp_i32<0x4E>(v);
  v += dpp_i32<0x141>(v);
  v += dpp_i32<0x140>(v);
  const auto s16 = __builtin_amdgcn_permlane16_swap((uint32_t)v, (uint32_t)v, false, false);
  v = (int)(s16[0] + s16[1]);
  const auto s32 = __builtin_amdgcn_permlane32_swap((uint32_t)v, (uint32_t)v, false, false);
  return (int)(s32[0] + s32[1]);
}

// RPW output rows per wave at a time (4, or 2 for the narrow projections: twice the waves, each with the same 8 loads in flight, so
// that 4096 output rows still put 2 workgroups on every CU); a step is 8 / RPW pieces of 512 elements (64 lanes x 8) of those rows.
// int8 kinds: a lane's 16 bytes are 16 elements, a piece is 1024 elements.  WK_I8W keeps x in LDS as bf16, each piece stored as its
// lanes' first eight elements (1 KiB) followed by their second eight, so that both 16-byte reads of a lane are conflict-free;
// WK_I8D keeps x as int8 (after the optional norm each row is quantised here, the row scales stay in registers).
// DORA (bf16 rows): a.wscale holds DoRA's per-row factors.  A build of its own, not a test of the pointer: the test cost the existing
// instances 2-7 SGPRs and the 4-token q|k|v instance four more spilled registers.
template <int MT, int EPI, bool NORM, int RPW = 2, int WK = WK_BF16, bool DORA = false>
__global__ __launch_bounds__(256, 2) void gemv_kernel(const GemvArgs a) {
  static_assert(!DORA || WK == WK_BF16, "DoRA factors ride on bf16 rows only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K;
  static_assert(RPW == 4 || RPW == 2, "rows per wave");
  using WT = std::conditional_t<WK == WK_BF16, bf16_t, int8_t>;  // a stored weight element
  constexpr int EPL = 16 / (int)sizeof(WT), PIECE = 64 * EPL;      // elements per lane and load; per wave-instruction
  constexpr int PIECES = 8 / RPW, STEP = PIECE * PIECES;
  const int nsteps = (K + STEP - 1) / STEP;  // a step = PIECES 512-element pieces of RPW weight rows: 8 x 16-byte loads per lane
  // the LDS copy of x is zero-padded to whole steps: weight lanes past K multiply zeros (int8 kinds, whose steps are 4096 elements:
  // padded to whole pieces plus ONE piece of zeros that every piece past the row end reads)
  const int Kp = WK == WK_BF16 ? nsteps * STEP : ((K + PIECE - 1) / PIECE + 1) * PIECE;
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [MT][Kp]
  int8_t* xq = reinterpret_cast<int8_t*>(smem);  // [MT][Kp] (WK_I8D)
  float* red = reinterpret_cast<float*>(smem + (size_t)MT * Kp * (WK == WK_I8D ? 1 : 2));
  float xsc[MT];                                 // WK_I8D: the activation rows' scales, as the bf16 the reference keeps

  // ---- row groups: RPW output rows per wave at a time.  SWIGLU: the gate and up rows of RPW / 2 hidden units (W[0] rows UPG g .. and
  // W[1] rows UPG g ..; r = matrix * UPG + unit), so that the epilogue has g and u of one unit side by side.
  constexpr int UPG = RPW / 2;  // hidden units per SwiGLU group
  // sc: the rows' weight scales (int8 kinds); cp: where the rows' DoRA factors sit (DORA; clamped like the weight rows; wave-uniform,
  // so the addresses wait in scalar registers while the rows stream and the factors themselves are only read in the epilogue)
  struct Grp { const WT* wr[RPW]; int row0, seg; float sc[RPW]; const bf16_t* cp[RPW]; };
  auto setup = [&](int g, Grp& G) {
    if constexpr (EPI == GV_SWIGLU) {
      const int half = a.N / 2;
      G.row0 = UPG * g; G.seg = 0;
#pragma unroll
      for (int r = 0; r < RPW; ++r) G.wr[r] = reinterpret_cast<const WT*>(a.W[r / UPG]) + (int64_t)min(G.row0 + (r % UPG), half - 1) * a.ldw[r / UPG];
      if constexpr (WK != WK_BF16) {
#pragma unroll
        for (int r = 0; r < RPW; ++r) G.sc[r] = bf2f(a.wscale[r / UPG][min(G.row0 + (r % UPG), half - 1)]);
      }
      if constexpr (DORA) {
#pragma unroll
        for (int r = 0; r < RPW; ++r) G.cp[r] = a.wscale[r / UPG] + min(G.row0 + (r % UPG), half - 1);
      }
    } else {
      G.row0 = RPW * g;
      G.seg = G.row0 >= a.seg_end[0] ? (G.row0 >= a.seg_end[1] ? 2 : 1) : 0;  // wave-uniform (segment boundaries are multiples of 4)
      const int base = G.seg == 0 ? 0 : a.seg_end[G.seg - 1];
      const int last = a.seg_end[G.seg] - 1 - base;
#pragma unroll
      for (int r = 0; r < RPW; ++r) G.wr[r] = reinterpret_cast<const WT*>(a.W[G.seg]) + (int64_t)min(G.row0 - base + r, last) * a.ldw[G.seg];
      if constexpr (WK != WK_BF16) {
#pragma unroll
        for (int r = 0; r < RPW; ++r) G.sc[r] = bf2f(a.wscale[G.seg][min(G.row0 - base + r, last)]);
      }
      if constexpr (DORA) {
#pragma unroll
        for (int r = 0; r < RPW; ++r) G.cp[r] = a.wscale[G.seg] + min(G.row0 - base + r, last);
      }
    }
  };
  auto load_step = [&](u32x4_t (&w)[8], const Grp& G, int s) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int k = (PIECES * s + j) * PIECE + lane * EPL;
      const int kk = k < K ? k : 0;  // lanes past the row end re-read its start; their x is zero
#pragma unroll
      for (int r = 0; r < RPW; ++r) w[RPW * j + r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(G.wr[r] + kk));
    }
  };
  const int nwaves = gridDim.x * 4;
  const int ngroups = EPI == GV_SWIGLU ? (a.N / 2 + UPG - 1) / UPG : (a.N + RPW - 1) / RPW;
  int g = blockIdx.x * 4 + wave, s = 0;
  Grp cur, nxt;
  u32x4_t WA[8], WB[8];
  // the first weight loads do not depend on x: they fly while the activation rows are staged (and normalised)
  if (g < ngroups) { setup(g, cur); load_step(WA, cur, 0); }

  // ---- the activation rows into LDS (normalised on the way when NORM)
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const bf16_t* xr = a.x + (int64_t)min(m, a.M - 1) * a.ldx;
    float rstd = 1.f;
    if constexpr (NORM) {
      float ss = 0.f;
      for (int i = tid * 8; i < K; i += 2048) ss = sumsq8(*reinterpret_cast<const u32x4_t*>(xr + i), ss);
      ss = block_sum(ss, red);
      rstd = rsqrtf(ss / (float)K + a.eps);
    }
    // 8 elements of the (normalised, bf16-rounded) row: what the linear of the reference sees
    auto xrow8 = [&](int i) -> u32x4_t {
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(xr + i);
      if constexpr (NORM) return norm8(v, rstd, a.norm_w + i);
      else return v;
    };
    if constexpr (WK == WK_BF16) {
      for (int i = tid * 8; i < Kp; i += 2048) {
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (i < K) v = xrow8(i);
        *reinterpret_cast<u32x4_t*>(xs + (size_t)m * Kp + i) = v;
      }
    } else {
      if constexpr (WK == WK_I8W) {
        for (int i = tid * 8; i < Kp; i += 2048) {
          u32x4_t v = {0u, 0u, 0u, 0u};
          if (i < K) v = xrow8(i);
          // element (piece, lane l, half h, e) of the row -> piece * 1024 + h * 512 + l * 8 + e
          const int at = (i & ~1023) + ((i >> 3) & 1) * 512 + ((i & 1023) >> 4) * 8;
          *reinterpret_cast<u32x4_t*>(xs + (size_t)m * Kp + at) = v;
        }
      } else {
        // quantize_int8_rowwise on the row (the pieces int8_quant.hip is made of); the second pass recomputes the same bf16 values
        float amax = 0.f;
        for (int i = tid * 8; i < K; i += 2048) amax = q8_absmax8(xrow8(i), amax);
        amax = block_max(amax, red);
        const float scale = q8_scale(amax);
        const float div = q8_divisor(scale);
        xsc[m] = bf2f(f2bf(scale));
        for (int i = tid * 8; i < Kp; i += 2048) {
          u32x2_t q = {0u, 0u};
          if (i < K) q = q8_quant8(xrow8(i), div);
          *reinterpret_cast<u32x2_t*>(xq + (size_t)m * Kp + i) = q;
        }
      }
    }
  }
  __syncthreads();

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
  int iacc[RPW][MT];  // WK_I8D: the integer dot products
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) iacc[r][m] = 0;
  auto compute_step = [&](const u32x4_t (&w)[8], int st) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int k = (PIECES * st + j) * PIECE + lane * EPL;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        if constexpr (WK == WK_BF16) {
          const u32x4_t xv = *reinterpret_cast<const u32x4_t*>(xs + (size_t)m * Kp + k);
          float xf[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { xf[2 * e] = bflo(xv[e]); xf[2 * e + 1] = bfhi(xv[e]); }
#pragma unroll
          for (int r = 0; r < RPW; ++r) acc[r][m] += dot8(w[RPW * j + r], xf);
        } else if constexpr (WK == WK_I8W) {
          const bf16_t* xp = xs + (size_t)m * Kp + min((PIECES * st + j) * PIECE, Kp - PIECE) + lane * 8;
          const u32x4_t x0 = *reinterpret_cast<const u32x4_t*>(xp), x1 = *reinterpret_cast<const u32x4_t*>(xp + 512);
          float xf[16];
#pragma unroll
          for (int e = 0; e < 4; ++e) { xf[2 * e] = bflo(x0[e]); xf[2 * e + 1] = bfhi(x0[e]); xf[8 + 2 * e] = bflo(x1[e]); xf[9 + 2 * e] = bfhi(x1[e]); }
#pragma unroll
          for (int r = 0; r < RPW; ++r) acc[r][m] = dot16_i8(w[RPW * j + r], xf, acc[r][m]);
        } else {
          const u32x4_t xv = *reinterpret_cast<const u32x4_t*>(xq + (size_t)m * Kp + min((PIECES * st + j) * PIECE, Kp - PIECE) + lane * EPL);
#pragma unroll
          for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) iacc[r][m] = __builtin_amdgcn_sdot4((int)w[RPW * j + r][e], (int)xv[e], iacc[r][m], false);
        }
      }
    }
  };
  auto finish = [&](const Grp& G) {
    const int row0 = G.row0, seg = G.seg;
    // int8 kinds: the adapter term is summed on its own and meets the base after the base's bf16 rounding (modelling/lora.py:41-43)
    const bool any_lora = WK != WK_BF16 && (a.bext[0] != nullptr || a.bext[1] != nullptr || a.bext[2] != nullptr);
    float lacc[RPW][MT];
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) lacc[r][m] = 0.f;
    // LoRA extension: lanes 0 .. rank/8-1 hold 8 elements of the row's B factor each
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int s2 = EPI == GV_SWIGLU ? (r / UPG) : seg;
      const bf16_t* bp = a.bext[s2];
      if (bp != nullptr && lane * 8 < a.rank[s2]) {
        int lrow;
        if constexpr (EPI == GV_SWIGLU) {
          lrow = min(row0 + (r % UPG), a.N / 2 - 1);
        } else {
          const int base = seg == 0 ? 0 : a.seg_end[seg - 1];
          lrow = min(row0 - base + r, a.seg_end[seg] - 1 - base);
        }
        const u32x4_t bv = *reinterpret_cast<const u32x4_t*>(bp + (int64_t)lrow * a.ldb[s2] + lane * 8);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const u32x4_t tv = *reinterpret_cast<const u32x4_t*>(a.t + (int64_t)min(m, a.M - 1) * a.ldt + a.t_off[s2] + lane * 8);
          float xf[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) { xf[2 * e] = bflo(tv[e]); xf[2 * e + 1] = bfhi(tv[e]); }
          if constexpr (WK == WK_BF16) acc[r][m] += a.lora_scale * dot8(bv, xf);
          else lacc[r][m] += a.lora_scale * dot8(bv, xf);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        if constexpr (WK == WK_I8D) iacc[r][m] = wave_sum_valu_i(iacc[r][m]);
        else acc[r][m] = wave_sum_valu(acc[r][m]);
      }
    if (any_lora) {
#pragma unroll
      for (int r = 0; r < RPW; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m) lacc[r][m] = wave_sum_valu(lacc[r][m]);
    }
    // ---- epilogue: lane m writes token m (every lane holds every sum)
    if (lane < MT && lane < a.M) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        if constexpr (WK == WK_BF16) {
          float sm = acc[r][0];
#pragma unroll
          for (int m = 1; m < MT; ++m) sm = lane == m ? acc[r][m] : sm;
          v[r] = bf2f(f2bf(sm));  // the linear's bf16 output
          // DoRA (modelling/lora.py:57-59): times the row's cached factor c = m / ||W + s B A||, rounded - out * (m / norm) of the bf16
          // eager graph.  Read here, by the lanes that write, through the address setup left in scalar registers
          if constexpr (DORA) v[r] = bf2f(f2bf(v[r] * bf2f(*G.cp[r])));
        } else {
          float ls = lacc[r][0];
#pragma unroll
          for (int m = 1; m < MT; ++m) ls = lane == m ? lacc[r][m] : ls;
          if constexpr (WK == WK_I8W) {
            // (x @ W_i8^T) rounded to bf16, times the row's scale, rounded (subclasses/int8.py:118; EPI_COLSCALE of gemm_bf16.hip)
            float sm = acc[r][0];
#pragma unroll
            for (int m = 1; m < MT; ++m) sm = lane == m ? acc[r][m] : sm;
            v[r] = bf2f(f2bf(bf2f(f2bf(sm)) * G.sc[r]));
          } else {
            // int32 sum x activation-row scale x weight-row scale in fp32, rounded (int8_mm.py:93-118; EPI_ROWCOLSCALE)
            int sm = iacc[r][0];
            float xm = xsc[0];
#pragma unroll
            for (int m = 1; m < MT; ++m) { sm = lane == m ? iacc[r][m] : sm; xm = lane == m ? xsc[m] : xm; }
            v[r] = bf2f(f2bf(((float)sm * xm) * G.sc[r]));
          }
          if (any_lora) v[r] = bf2f(f2bf(v[r] + ls));
        }
      }
      // q|k|v: the table row is the token's index IN THIS CALL (modelling/llama.py:207); the position is not checked against the cache
      const int m = lane;
      stream_epilogue<EPI, RPW>(a, row0, m, a.rope + (int64_t)m * 128, [&] { return a.pos[m] * a.c_ss; }, v);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) { acc[r][m] = 0.f; iacc[r][m] = 0; }
  };
  // software pipeline over the flattened (row group, step) sequence of this wave: while one register set is consumed the next step's
  // 8 loads (of this group or of the wave's next group) are in flight
  auto body = [&](const u32x4_t (&wc)[8], u32x4_t (&wn)[8]) -> bool {
    int g2 = g, s2 = s + 1;
    bool newg = false;
    if (s2 == nsteps) { g2 = g + nwaves; s2 = 0; newg = true; }
    const bool has2 = g2 < ngroups;
    if (has2) {
      if (newg) { setup(g2, nxt); load_step(wn, nxt, s2); }
      else load_step(wn, cur, s2);
    }
    compute_step(wc, s);
    if (newg) {
      finish(cur);
      cur = nxt;
    }
    g = g2; s = s2;
    return has2;
  };
  if (g < ngroups) {
    while (true) {
      if (!body(WA, WB)) break;
      if (!body(WB, WA)) break;
    }
  }
}

// the instance of one pass: MT = 1 | 2 | 4 staged rows of x, two output rows per wave
template <int WK, bool DORA = false>
static int launch_gemv(const char* fn, const GemvArgs& a, int MT, int epi, int grid, size_t lds, hipStream_t stream) {
  auto go = [&](auto mt) {
    return stream_with_epilogue(epi, [&](auto e) {
      constexpr int MT_ = decltype(mt)::value, EPI = decltype(e)::value;
      if (a.norm_w) hipLaunchKernelGGL((gemv_kernel<MT_, EPI, true, 2, WK, DORA>), dim3(grid), dim3(256), lds, stream, a);
      else hipLaunchKernelGGL((gemv_kernel<MT_, EPI, false, 2, WK, DORA>), dim3(grid), dim3(256), lds, stream, a);
      LLX_LAUNCH_CHECK(fn);
      return LLX_OK;
    });
  };
  switch (MT) {
    case 1: return go(std::integral_constant<int, 1>{});
    case 2: return go(std::integral_constant<int, 2>{});
    default:
      // (weight-only int8 has no 4-token build: 16 fp32 activations per lane and token next to the two weight register sets do not fit
      // the 256 registers of two workgroups per CU without scratch; its callers run 3 and 4 tokens as two passes of the 2-token build)
      if constexpr (WK == WK_I8W) { llx_set_error("llx_gemv_i8: no 4-token build of the weight-only kind"); return LLX_ERR_UNSUPPORTED; }
      else return go(std::integral_constant<int, 4>{});
  }
}

// out[M, N] = epilogue( x[M, K] . [W0; W1; W2]^T ), M <= 4, bf16, fp32 accumulate; F.linear at decode shapes
// (modelling/llama.py:118-120,140,152,216).  W_s: [n_s, K] row-major with row stride ldw_s (nullable from s = 1 on; n_s % 4 == 0 except
// the last, or any n_0 = n_1 under the SwiGLU epilogue), K % 8 == 0.  norm_w (nullable): x is RMS-normalised with this weight first (llama.py:172-173,215).
// The epilogues are wstream.h's; q|k|v rotates row m by table row m and writes its k / v heads at input_pos[m] (device int64), caches
// through (head, position) strides.  LoRA (nullable bext_s [n_s, rank_s], t [M, sum rank] bf16 = x . A^T, offsets t_off_s, scale):
// out += scale * t_s . bext_s[row].
// the three entry points below: fn = the caller's name for messages, wk = weight kind, scales = per-row scales of W_s (int8 kinds) or
// DoRA's per-row factors (bf16 rows with dora set: every present segment has one), null for plain bf16 rows
static int gemv_run(const char* fn, int wk, bool dora, const void* const* scales, const StreamCall& c, const StreamLora& lo, hipStream_t stream) {
  const int wa = wk == WK_BF16 ? 8 : 16;  // weight elements per 16-byte lane load
  GemvArgs a;
  // (inner segments in multiples of 4 rows keep a row group inside one weight; SwiGLU pairs gate row i with up row i whatever their count)
  const int rc0 = stream_check_fill(fn, a, 1, 4, "larger row counts run the MFMA GEMM", wa, c.epilogue == GV_SWIGLU ? 1 : 4, c);
  if (rc0 != LLX_OK) return rc0;
  if (wk != WK_BF16 || dora) {
    const int rc1 = stream_check_fill_scales(fn, a, dora ? "DoRA" : "int8", c, scales);
    if (rc1 != LLX_OK) return rc1;
  }
  const int rc2 = gemv_check_fill_lora(fn, a, c, lo);
  if (rc2 != LLX_OK) return rc2;
  // rows per wave: 2 (steps of 2048 elements per row: half the dependent steps of the 4-row form on every product of the decode step and
  // twice the waves where N <= 4096 would fill only half of the 2048 slots: 3.39 ms per token against the 4-row form's 3.51 and 3.43 with
  // one row per wave).
  // int8 rows: 2 as well (steps of 4 pieces = 4096 elements per row, so a K = 4096 row is one step and K = 14336 pads its last step
  // by two pieces; the 4-row form with steps of 2048 elements, which tile both K exactly, was measured next to it on the 8B decode
  // step: 2.64 / 2.81 ms per token (weight-only / dynamic, context 4096) against 2.54 / 2.71 with 2 rows - the wider grid of the
  // N = 4096 and 6144 products decides, as for bf16).  Only the 2-row form is built.
  constexpr int rpw = 2;
  const int grid = gemv_grid(a.N, c.epilogue, rpw);
  const int64_t piece = 64 * wa, kstep = piece * (8 / rpw);
  const int64_t Kp = wk == WK_BF16 ? cdiv64(c.K, kstep) * kstep : (cdiv64(c.K, piece) + 1) * piece;  // the kernel's LDS row length
  // (the weight-only int8 kind has no 4-token build; the dynamic kind stages int8 codes, one byte per element)
  return gemv_passes(fn, a, wk == WK_I8W ? 2 : 4, Kp, wk == WK_I8D ? 1 : 2, [&](const GemvArgs& b, int MT, size_t lds) {
    if (wk == WK_I8W) return launch_gemv<WK_I8W>(fn, b, MT, c.epilogue, grid, lds, stream);
    if (wk == WK_I8D) return launch_gemv<WK_I8D>(fn, b, MT, c.epilogue, grid, lds, stream);
    if (dora) return launch_gemv<WK_BF16, true>(fn, b, MT, c.epilogue, grid, lds, stream);
    return launch_gemv<WK_BF16>(fn, b, MT, c.epilogue, grid, lds, stream);
  });
}

extern "C" int llx_gemv_bf16(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                             int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                             void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache,
                             void* v_cache, int64_t c_sh, int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1,
                             const void* bext2, int64_t rank0, int64_t rank1, int64_t rank2, const void* t, int64_t ldt, float lora_scale,
                             hipStream_t stream) {
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, 0, c_sh, c_ss, 0, input_pos};
  const StreamLora lo = {{bext0, bext1, bext2}, {rank0, rank1, rank2}, t, ldt, lora_scale, {}};
  return gemv_run("llx_gemv_bf16", WK_BF16, false, nullptr, c, lo, stream);
}

// llx_gemv_bf16 on DoRA linears (modelling/lora.py:51-59) with the row factor c_s = m / ||W_s + s B_s A_s||_row cached by the caller
// (bf16 [n_s], one per present segment): out = epilogue(bf16(bf16(x . W^T + lora_scale * t . bext[row]) * c[row])) - the rounding points
// of out * (m / norm) in the bf16 eager graph; gate and up are scaled by their own factors before SwiGLU, q and k before RoPE.
extern "C" int llx_gemv_bf16_dora(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                                  int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                                  void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache,
                                  void* v_cache, int64_t c_sh, int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1,
                                  const void* bext2, int64_t rank0, int64_t rank1, int64_t rank2, const void* t, int64_t ldt, float lora_scale,
                                  const void* colscale0, const void* colscale1, const void* colscale2, hipStream_t stream) {
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, 0, c_sh, c_ss, 0, input_pos};
  const StreamLora lo = {{bext0, bext1, bext2}, {rank0, rank1, rank2}, t, ldt, lora_scale, {colscale0, colscale1, colscale2}};
  return gemv_run("llx_gemv_bf16_dora", WK_BF16, true, lo.colscale, c, lo, stream);
}

// The same product on int8 weight rows (subclasses/int8.py:106-121): W_s [n_s, K] int8 row-major (ldw_s in bytes, multiples of 16),
// scale_s [n_s] bf16 per-row scales, K % 16 == 0.  dynamic = 0 (weight-only, :118): out = bf16(bf16(x . W^T) * scale), fp32 FMA on
// the sign-extended bytes.  dynamic = 1 (:112-113, int8_mm.py:93-118): every (normalised) row of x is quantised as
// llx_quantize_int8_rowwise does, int32 dot products, out = bf16(((float)acc * x_scale[m]) * scale[row]) - bit-exact with the
// reference when no norm is fused.  Epilogues, norm and the q|k|v / SwiGLU neighbours as llx_gemv_bf16; LoRA (t from llx_gemv_bf16 on
// the un-quantised x): out = bf16(out + lora_scale * t_s . bext_s[row]).
extern "C" int llx_gemv_i8(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                           int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                           void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache,
                           void* v_cache, int64_t c_sh, int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1,
                           const void* bext2, int64_t rank0, int64_t rank1, int64_t rank2, const void* t, int64_t ldt, float lora_scale,
                           const void* scale0, const void* scale1, const void* scale2, int dynamic, hipStream_t stream) {
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, 0, c_sh, c_ss, 0, input_pos};
  const StreamLora lo = {{bext0, bext1, bext2}, {rank0, rank1, rank2}, t, ldt, lora_scale, {}};
  const void* const scales[3] = {scale0, scale1, scale2};
  return gemv_run("llx_gemv_i8", dynamic ? WK_I8D : WK_I8W, false, scales, c, lo, stream);
}

// ------------------------------------------------------------------------------------------------- mask extent / cache scatter
// *extent = 1 + the largest key index that ANY of the `rows` mask rows (uint8 / bool, row stride m_sr) allows; 0 if none.
__global__ __launch_bounds__(256) void mask_extent_kernel(const uint8_t* __restrict__ mask, int64_t m_sr, int rows, int Skv, int* __restrict__ extent) {
  __shared__ int red[4];
  int best = 0;
  for (int r = 0; r < rows; ++r) {
    const uint8_t* mr = mask + (int64_t)r * m_sr;
    for (int k = threadIdx.x; k < Skv; k += 256)
      if (mr[k]) best = max(best, k + 1);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) *extent = max(max(red[0], red[1]), max(red[2], red[3]));
}

extern "C" int llx_mask_extent(const void* mask, int64_t row_stride, int64_t rows, int64_t Skv, int* extent, hipStream_t stream) {
  LLX_REQUIRE(mask && extent && rows > 0 && Skv > 0 && Skv < (1 << 30) && rows < (1 << 20), "llx_mask_extent: bad arguments");
  hipLaunchKernelGGL(mask_extent_kernel, dim3(1), dim3(256), 0, stream, (const uint8_t*)mask, row_stride, (int)rows, (int)Skv, extent);
  LLX_LAUNCH_CHECK("llx_mask_extent");
  return LLX_OK;
}

// KVCache.update (modelling/llama.py:83-90): cache[b, h, input_pos[l], :] = src[b, h, l, :] for k and v in one launch.
__global__ __launch_bounds__(256) void kv_scatter_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t s_sb, int64_t s_sh, int64_t s_ss,
                                                         bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, int64_t c_sb, int64_t c_sh, int64_t c_ss,
                                                         const int64_t* __restrict__ pos, int64_t p_sb, int L, int KVH, int Smax) {
  const int chunk = threadIdx.x & 15, which = (threadIdx.x >> 4) & 1, li = blockIdx.x * 8 + (threadIdx.x >> 5);
  const int h = blockIdx.y, b = blockIdx.z;
  if (li >= L) return;
  const int64_t p = pos[b * p_sb + li];  // p_sb = 0: one position row for every batch element
  if (p < 0 || p >= Smax) return;  // torch's index_put would raise; an out-of-range position must never write outside the cache
  const bf16_t* src = (which ? v : k) + b * s_sb + h * s_sh + (int64_t)li * s_ss + chunk * 8;
  bf16_t* dst = (which ? vc : kc) + b * c_sb + h * c_sh + p * c_ss + chunk * 8;
  *reinterpret_cast<u32x4_t*>(dst) = *reinterpret_cast<const u32x4_t*>(src);
}

// p_sb = the row stride of input_pos [B, L]; 0: one position row [L] for every batch element
static int kv_scatter_run(const char* fn, const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb,
                          int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t p_sb, int64_t B, int64_t KVH, int64_t L, int64_t Smax, int64_t head_dim,
                          hipStream_t stream) {
  LLX_REQUIRE(k && v && k_cache && v_cache && input_pos, "%s: null pointer", fn);
  LLX_REQUIRE(head_dim == HD, "%s: head_dim=%lld unsupported (only 128)", fn, (long long)head_dim);
  LLX_REQUIRE(B > 0 && KVH > 0 && L > 0 && Smax > 0 && B < 65536 && KVH < 65536, "%s: bad sizes", fn);
  LLX_REQUIRE(((s_sb | s_sh | s_ss | c_sb | c_sh | c_ss) % 8) == 0 && ((uintptr_t)k | (uintptr_t)v | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 == 0,
              "%s: rows must be 16-byte aligned", fn);
  hipLaunchKernelGGL(kv_scatter_kernel, dim3((unsigned)cdiv64(L, 8), (unsigned)KVH, (unsigned)B), dim3(256), 0, stream, (const bf16_t*)k, (const bf16_t*)v,
                     s_sb, s_sh, s_ss, (bf16_t*)k_cache, (bf16_t*)v_cache, c_sb, c_sh, c_ss, input_pos, p_sb, (int)L, (int)KVH, (int)Smax);
  LLX_LAUNCH_CHECK(fn);
  return LLX_OK;
}

extern "C" int llx_kv_scatter(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb,
                              int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t B, int64_t KVH, int64_t L, int64_t Smax,
                              int64_t head_dim, hipStream_t stream) {
  return kv_scatter_run("llx_kv_scatter", k, v, s_sb, s_sh, s_ss, k_cache, v_cache, c_sb, c_sh, c_ss, input_pos, 0, B, KVH, L, Smax, head_dim, stream);
}

// KVCache.update with a position row per batch element: cache[b, h, input_pos[b, l], :] = src[b, h, l, :] (input_pos int64 [B, L] with
// row stride p_sb >= L): the sequences of a batch sit at their own positions.  Everything else as llx_kv_scatter.
extern "C" int llx_kv_scatter_rows(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb,
                                   int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t p_sb, int64_t B, int64_t KVH, int64_t L, int64_t Smax,
                                   int64_t head_dim, hipStream_t stream) {
  LLX_REQUIRE(p_sb >= L, "llx_kv_scatter_rows: bad sizes (a position row shorter than L)");
  return kv_scatter_run("llx_kv_scatter_rows", k, v, s_sb, s_sh, s_ss, k_cache, v_cache, c_sb, c_sh, c_ss, input_pos, p_sb, B, KVH, L, Smax, head_dim, stream);
}

// ------------------------------------------------------------------------------------------------- decode attention
#define DEC_PART 132  // floats per partial: o[128], m, l, pad

struct DecodeArgs {
  const bf16_t* q; int64_t q_sb, q_sh, q_ss;             // [B, H, M, 128] through strides
  const bf16_t* kc; const bf16_t* vc; int64_t c_sb, c_sh, c_ss;
  const uint8_t* mask; int64_t m_sb, m_sh, m_sq;         // bool [.., M, Skv], broadcast strides, last dim dense
  const int* extent;                                     // nullable: keys >= *extent are masked for every row
  float* part;                                           // [B, H, M, nsplit, DEC_PART]
  int B, H, KVH, M, Skv, nsplit;
  float scale_log2;
};

// One workgroup = 4 waves = one key range of one (batch, kv head); ROWS = G * M query rows (the G heads of the group x the tokens of
// the call) share every K / V row read.  A 16-lane group owns one key per load (lane = 16-byte chunk of the 256-byte row): four keys
// per wave-instruction, sixteen per wave and step (8 x 16-byte loads in flight per lane), 64 per workgroup step.
// DEC_KPG = keys per lane group and step: 4 for up to 4 query rows (the batch-1 decode step), fewer for more rows (register budget)
// F8: the caches hold E4M3 codes (a.kc / a.vc point at bytes, cache strides in bytes).  The lane layout is the bf16 one -
// a lane owns the same 8 elements of a row, now an 8-byte load, 16 lanes x 8 B = one 128-byte row - so every sum below runs over the
// same elements in the same order and the kernel computes what the bf16 instance computes on dq(code); the codes are unpacked with
// v_cvt_pk_f32_fp8 where the bf16 instance shifts.
template <int ROWS, int DEC_KPG, bool F8 = false>
__global__ __launch_bounds__(256) void attn_decode_kernel(const DecodeArgs a) {
  using CT = std::conditional_t<F8, uint8_t, bf16_t>;     // a stored cache element
  using ld_t = std::conditional_t<F8, u32x2_t, u32x4_t>;  // a lane's 8 elements of a row
  // partials that meet in LDS: one per wave after a shuffle merge of its four lane groups, or - for up to 4 rows, where 16 partials fit
  // in 32 KB - one per lane group straight from the registers (the 80 dependent shuffles of the merge cost 1.6 us of a 7.5 us block)
  constexpr int NPART = ROWS <= 4 ? 16 : 4;
  __shared__ float sm_o[NPART][ROWS][HD];
  __shared__ float sm_ml[NPART][ROWS][2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int G = a.H / a.KVH;
  const int grp = lane >> 4, c = lane & 15;
  const int ext = a.extent ? min(*a.extent, a.Skv) : a.Skv;
  const int span = ((ext + a.nsplit - 1) / a.nsplit + 15) & ~15;  // keys per workgroup, multiple of 16
  const int k_lo = split * span, k_hi = min(ext, k_lo + span);

  // (the query rows are only REQUESTED here: they are unpacked after the first K / V loads have been issued - unpacking them first
  // put a full memory round trip, 1.2 us, in front of those loads)
  u32x4_t qraw[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int g = r / a.M, m = r % a.M;  // row r = (head g of the group, token m)
    const int h = kvh * G + min(g, G - 1);
    qraw[r] = *reinterpret_cast<const u32x4_t*>(a.q + b * a.q_sb + h * a.q_sh + (int64_t)m * a.q_ss + c * 8);
  }
  float qf[ROWS][8];
  float mx[ROWS], ls[ROWS], o[ROWS][8];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    mx[r] = -INFINITY; ls[r] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[r][e] = 0.f;
  }
  const CT* kb = reinterpret_cast<const CT*>(a.kc) + b * a.c_sb + kvh * a.c_sh + c * 8;
  const CT* vb = reinterpret_cast<const CT*>(a.vc) + b * a.c_sb + kvh * a.c_sh + c * 8;
  const bool shared_mask = a.m_sh == 0;  // the reference's mask (tril rows gathered at input_pos) is the same for every head
  const uint8_t* mbase = a.mask + b * a.m_sb;
  // Two register sets: the K / V rows and mask bytes of step i+1 are in flight while step i is computed - a wave walks only 2-8
  // steps, so with the loads issued step by step every step paid a full HBM round trip (the kernel ran at 1.5 TB/s).  The mask bytes
  // are only LOADED in the load step, unconditionally and with clamped indices: turning them into bits needs their values and would
  // make the step wait for its own loads.
  auto load_step = [&](int k0, ld_t (&kv)[DEC_KPG], ld_t (&vv)[DEC_KPG], uint8_t (&mb)[DEC_KPG][ROWS]) {
#pragma unroll
    for (int j = 0; j < DEC_KPG; ++j) {
      const int key = k0 + j * 4 + grp;
      const int kk = min(key, a.Skv - 1);
      kv[j] = *reinterpret_cast<const ld_t*>(kb + (int64_t)kk * a.c_ss);
      vv[j] = *reinterpret_cast<const ld_t*>(vb + (int64_t)kk * a.c_ss);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        // shared mask: entry m = token m (expanded to the G heads below); per-head mask: entry r = (head g, token m)
        const int g = min(r / a.M, G - 1), m = shared_mask ? min(r, a.M - 1) : r % a.M;
        mb[j][r] = mbase[(shared_mask ? (int64_t)0 : (int64_t)(kvh * G + g) * a.m_sh) + (int64_t)m * a.m_sq + kk];
      }
    }
  };
  auto compute_step = [&](int k0, const ld_t (&kv)[DEC_KPG], const ld_t (&vv)[DEC_KPG], const uint8_t (&mb)[DEC_KPG][ROWS]) {
    uint32_t allow[DEC_KPG];  // shared mask: bit m = token m; per-head mask: bit r = query row r
#pragma unroll
    for (int j = 0; j < DEC_KPG; ++j) {
      uint32_t w = 0;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const bool valid = shared_mask ? r < a.M : r / a.M < G;
        if (valid && mb[j][r] != 0) w |= 1u << r;
      }
      allow[j] = (k0 + j * 4 + grp) < k_hi ? w : 0u;
    }
    float vf[F8 ? DEC_KPG : 1][8];  // F8: the V rows unpacked once per step, not once per query row
    if constexpr (F8) {
#pragma unroll
      for (int j = 0; j < DEC_KPG; ++j) kv8_decode8(vv[j], vf[j]);
    }
    float s[DEC_KPG][ROWS];
#pragma unroll
    for (int j = 0; j < DEC_KPG; ++j) {
      float kf[8];
      if constexpr (F8) {
        kv8_decode8(kv[j], kf);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) { kf[2 * e] = bflo(kv[j][e]); kf[2 * e + 1] = bfhi(kv[j][e]); }
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = __builtin_fmaf(qf[r][e], kf[e], d);
        // sum over the 16 lanes of the key's group in the vector pipe (DPP: quad swaps, then the mirrors pair quads and halves - the same
        // additions as an xor butterfly, without four trips through the LDS crossbar)
        d += dpp_f32<0xB1>(d);   // quad_perm [1,0,3,2]
        d += dpp_f32<0x4E>(d);   // quad_perm [2,3,0,1]
        d += dpp_f32<0x141>(d);  // row_half_mirror
        d += dpp_f32<0x140>(d);  // row_mirror
        const bool ok = shared_mask ? ((allow[j] >> (r % a.M)) & 1u) != 0 : ((allow[j] >> r) & 1u) != 0;
        s[j][r] = ok ? d : -INFINITY;
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      float mn = mx[r];
#pragma unroll
      for (int j = 0; j < DEC_KPG; ++j) mn = fmaxf(mn, s[j][r]);
      if (mn == -INFINITY) continue;  // nothing to attend to so far for this row in this lane group
      const float alpha = __builtin_amdgcn_exp2f(mx[r] - mn);
      float p[DEC_KPG], psum = 0.f;
#pragma unroll
      for (int j = 0; j < DEC_KPG; ++j) { p[j] = __builtin_amdgcn_exp2f(s[j][r] - mn); psum += p[j]; }
      ls[r] = ls[r] * alpha + psum;
      mx[r] = mn;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float lo = o[r][2 * e] * alpha, hi = o[r][2 * e + 1] * alpha;
#pragma unroll
        for (int j = 0; j < DEC_KPG; ++j) {
          if constexpr (F8) { lo = __builtin_fmaf(p[j], vf[j][2 * e], lo); hi = __builtin_fmaf(p[j], vf[j][2 * e + 1], hi); }
          else { lo = __builtin_fmaf(p[j], bflo(vv[j][e]), lo); hi = __builtin_fmaf(p[j], bfhi(vv[j][e]), hi); }
        }
        o[r][2 * e] = lo; o[r][2 * e + 1] = hi;
      }
    }
  };
  {
    const int kstep = 16 * DEC_KPG;
    ld_t kvA[DEC_KPG], vvA[DEC_KPG], kvB[DEC_KPG], vvB[DEC_KPG];
    uint8_t mbA[DEC_KPG][ROWS], mbB[DEC_KPG][ROWS];
    int k0 = k_lo + wave * (4 * DEC_KPG);
    if (k0 < k_hi) load_step(k0, kvA, vvA, mbA);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) { qf[r][2 * e] = bflo(qraw[r][e]) * a.scale_log2; qf[r][2 * e + 1] = bfhi(qraw[r][e]) * a.scale_log2; }
    while (k0 < k_hi) {
      if (k0 + kstep < k_hi) load_step(k0 + kstep, kvB, vvB, mbB);
      compute_step(k0, kvA, vvA, mbA);
      k0 += kstep;
      if (k0 >= k_hi) break;
      if (k0 + kstep < k_hi) load_step(k0 + kstep, kvA, vvA, mbA);
      compute_step(k0, kvB, vvB, mbB);
      k0 += kstep;
    }
  }
  // merge the four lane groups of the wave (lanes l, l^16, l^32, l^48 hold the same dims of different keys), then the four waves
  // through LDS: ONE partial (m, l, o) per workgroup and query row
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    if constexpr (NPART == 4) {
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const float m2 = __shfl_xor(mx[r], off, 64), l2 = __shfl_xor(ls[r], off, 64);
        const float mn = fmaxf(mx[r], m2);
        const float fa = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mx[r] - mn), fb = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m2 - mn);
        ls[r] = ls[r] * fa + l2 * fb;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[r][e] = o[r][e] * fa + __shfl_xor(o[r][e], off, 64) * fb;
        mx[r] = mn;
      }
    }
    const int slot = NPART == 4 ? wave : wave * 4 + grp;
    if (NPART == 16 || grp == 0) {
      *reinterpret_cast<f32x4_t*>(&sm_o[slot][r][c * 8]) = f32x4_t{o[r][0], o[r][1], o[r][2], o[r][3]};
      *reinterpret_cast<f32x4_t*>(&sm_o[slot][r][c * 8 + 4]) = f32x4_t{o[r][4], o[r][5], o[r][6], o[r][7]};
      if (c == 0) { sm_ml[slot][r][0] = mx[r]; sm_ml[slot][r][1] = ls[r]; }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < ROWS * HD; idx += 256) {
    const int r = idx >> 7, d = idx & (HD - 1);
    const int g = r / a.M, m = r % a.M;
    if (g >= G) continue;
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < NPART; ++w) mm = fmaxf(mm, sm_ml[w][r][0]);
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int w = 0; w < NPART; ++w) {
      const float f = sm_ml[w][r][0] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sm_ml[w][r][0] - mm);
      num += sm_o[w][r][d] * f;
      den += sm_ml[w][r][1] * f;
    }
    float* pp = a.part + ((((int64_t)b * a.H + kvh * G + g) * a.M + m) * a.nsplit + split) * DEC_PART;
    pp[d] = num;
    if (d == 0) { pp[128] = mm; pp[129] = den; }
  }
}

// o[b, m, h, :] = sum_i o_i 2^(m_i - M) / sum_i l_i 2^(m_i - M) over the nparts partials of (b, h, m); a row without any allowed key
// comes out NaN, as SDPA's softmax of an all -inf row does.  One block per (b, h, m): the (m_i, l_i) pairs go through LDS, then every
// thread sums its output dim over the partials with independent loads.
__global__ __launch_bounds__(512) void attn_decode_combine_kernel(const float* __restrict__ part, int nparts, bf16_t* __restrict__ o, int64_t o_sb, int64_t o_sh,
                                                                  int64_t o_ss, int H, int M) {
  // 4 groups of 128 threads share the partials of one (b, h, m) (with 64 of them a single group's serial loop was most of this
  // 32-block kernel's 7.6 us); every group sums its quarter in partial order, the quarters are added in group order
  __shared__ float sf[1024], sl[1024], snum[4][HD], sden[4];
  const int d = threadIdx.x & 127, grp = threadIdx.x >> 7;
  const int m = blockIdx.x % M, h = (blockIdx.x / M) % H, b = blockIdx.x / (M * H);
  const float* pp = part + (int64_t)blockIdx.x * nparts * DEC_PART;
  for (int i = threadIdx.x; i < nparts; i += 512) { sf[i] = pp[i * DEC_PART + 128]; sl[i] = pp[i * DEC_PART + 129]; }
  __syncthreads();
  float mm = -INFINITY;
  for (int i = 0; i < nparts; ++i) mm = fmaxf(mm, sf[i]);
  const int per = (nparts + 3) / 4, i0 = grp * per, i1 = min(nparts, i0 + per);
  float num = 0.f, den = 0.f;
#pragma unroll 8
  for (int i = i0; i < i1; ++i) {
    const float f = sf[i] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sf[i] - mm);
    num += pp[i * DEC_PART + d] * f;
    den += sl[i] * f;
  }
  snum[grp][d] = num;
  if (d == 0) sden[grp] = den;
  __syncthreads();
  if (grp == 0) {
    const float n4 = ((snum[0][d] + snum[1][d]) + snum[2][d]) + snum[3][d];
    const float d4 = ((sden[0] + sden[1]) + sden[2]) + sden[3];
    o[b * o_sb + h * o_sh + (int64_t)m * o_ss + d] = f2bf(n4 / d4);
  }
}

extern "C" int64_t llx_attn_decode_workspace_bytes(int64_t B, int64_t H, int64_t M, int64_t nsplit) { return B * H * M * nsplit * DEC_PART * 4; }

// SDPA(q, k_cache, v_cache, mask, is_causal=False, enable_gqa=True) for a few query tokens (M * H / KVH <= 16) against the whole cache
// (modelling/llama.py:126-127,135-137).  q [B,H,M,128], caches [B,KVH,Skv,128], o [B,H,M,128] through (batch, head, position) element
// strides; mask bool [.., M, Skv] with broadcast strides; extent (nullable device int, llx_mask_extent): bound on the keys any row
// may attend to; workspace: llx_attn_decode_workspace_bytes(B, H, M, nsplit) bytes of fp32.
// what the two entry points share; f8: the caches hold E4M3 codes, cache strides in bytes
static int attn_decode_run(const char* fn, bool f8, const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k_cache, const void* v_cache, int64_t c_sb,
                           int64_t c_sh, int64_t c_ss, void* o, int64_t o_sb, int64_t o_sh, int64_t o_ss, const void* mask, int64_t m_sb,
                           int64_t m_sh, int64_t m_sq, const int* extent, float* workspace, int64_t B, int64_t H, int64_t KVH, int64_t M,
                           int64_t Skv, int64_t nsplit, int64_t head_dim, float scale, hipStream_t stream) {
  LLX_REQUIRE(q && k_cache && v_cache && o && mask && workspace, "%s: null pointer", fn);
  LLX_REQUIRE(head_dim == HD, "%s: head_dim=%lld unsupported (only 128)", fn, (long long)head_dim);
  LLX_REQUIRE(B > 0 && H > 0 && KVH > 0 && H % KVH == 0 && M > 0 && Skv > 0 && nsplit > 0 && nsplit <= 1024 && B < 65536 && KVH < 65536, "%s: bad sizes", fn);
  const int64_t rows = H / KVH * M;
  LLX_REQUIRE(rows <= 16, "%s: %lld query rows per kv head (heads per group x tokens) exceed 16: use llx_attn_dense_fwd", fn, (long long)rows);
  LLX_REQUIRE(((q_sb | q_sh | q_ss | c_sb | c_sh | c_ss) % 8) == 0 && ((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 == 0 && (uintptr_t)workspace % 16 == 0,
              "%s: rows must be 16-byte aligned", fn);
  DecodeArgs a;
  a.q = (const bf16_t*)q; a.q_sb = q_sb; a.q_sh = q_sh; a.q_ss = q_ss;
  a.kc = (const bf16_t*)k_cache; a.vc = (const bf16_t*)v_cache; a.c_sb = c_sb; a.c_sh = c_sh; a.c_ss = c_ss;
  a.mask = (const uint8_t*)mask; a.m_sb = m_sb; a.m_sh = m_sh; a.m_sq = m_sq; a.extent = extent; a.part = workspace;
  a.B = (int)B; a.H = (int)H; a.KVH = (int)KVH; a.M = (int)M; a.Skv = (int)Skv; a.nsplit = (int)nsplit;
  a.scale_log2 = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)nsplit, (unsigned)KVH, (unsigned)B);
  if (f8) {
    if (rows <= 4) hipLaunchKernelGGL((attn_decode_kernel<4, 4, true>), grid, dim3(256), 0, stream, a);
    else if (rows <= 8) hipLaunchKernelGGL((attn_decode_kernel<8, 2, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((attn_decode_kernel<16, 1, true>), grid, dim3(256), 0, stream, a);
  } else {
    if (rows <= 4) hipLaunchKernelGGL((attn_decode_kernel<4, 4>), grid, dim3(256), 0, stream, a);
    else if (rows <= 8) hipLaunchKernelGGL((attn_decode_kernel<8, 2>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((attn_decode_kernel<16, 1>), grid, dim3(256), 0, stream, a);
  }
  LLX_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((unsigned)(B * H * M)), dim3(512), 0, stream, (const float*)workspace, (int)nsplit, (bf16_t*)o, o_sb,
                     o_sh, o_ss, (int)H, (int)M);
  char name[64];
  snprintf(name, sizeof name, "%s(combine)", fn);
  LLX_LAUNCH_CHECK(name);
  return LLX_OK;
}

extern "C" int llx_attn_decode(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k_cache, const void* v_cache, int64_t c_sb,
                               int64_t c_sh, int64_t c_ss, void* o, int64_t o_sb, int64_t o_sh, int64_t o_ss, const void* mask, int64_t m_sb,
                               int64_t m_sh, int64_t m_sq, const int* extent, float* workspace, int64_t B, int64_t H, int64_t KVH, int64_t M,
                               int64_t Skv, int64_t nsplit, int64_t head_dim, float scale, hipStream_t stream) {
  return attn_decode_run("llx_attn_decode", false, q, q_sb, q_sh, q_ss, k_cache, v_cache, c_sb, c_sh, c_ss, o, o_sb, o_sh, o_ss, mask, m_sb, m_sh, m_sq, extent,
                         workspace, B, H, KVH, M, Skv, nsplit, head_dim, scale, stream);
}

// llx_attn_decode over FP8 caches: caches uint8 [B, KVH, Skv, 128] of E4M3 codes through BYTE strides (multiples of 8, the
// pointers 16-byte aligned); everything else - the ROWS classes, the split plan, the mask, the partials, the combine launch and the
// workspace - as llx_attn_decode, and so is the result: what llx_attn_decode computes on the caches' bf16 images.
extern "C" int llx_attn_decode_f8(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k_cache, const void* v_cache, int64_t c_sb,
                                  int64_t c_sh, int64_t c_ss, void* o, int64_t o_sb, int64_t o_sh, int64_t o_ss, const void* mask, int64_t m_sb,
                                  int64_t m_sh, int64_t m_sq, const int* extent, float* workspace, int64_t B, int64_t H, int64_t KVH, int64_t M,
                                  int64_t Skv, int64_t nsplit, int64_t head_dim, float scale, hipStream_t stream) {
  return attn_decode_run("llx_attn_decode_f8", true, q, q_sb, q_sh, q_ss, k_cache, v_cache, c_sb, c_sh, c_ss, o, o_sb, o_sh, o_ss, mask, m_sb, m_sh, m_sq,
                         extent, workspace, B, H, KVH, M, Skv, nsplit, head_dim, scale, stream);
}
