// Batched decode (2-16 sequences, one token each): the weight stream of decode.hip's gemv_kernel on the matrix pipe.
//
// gemv_kernel does one fp32 FMA per weight element and activation row in the vector pipe; at 16 rows that is the vector pipe's whole
// FMA peak at the HBM rate.  A block of <= 16 activation rows is exactly one operand of v_mfma_f32_16x16x32_bf16, so here
//   * a wave owns a tile of 16 weight rows over one K slice: the weight rows are the MFMA's A operand (lane l = row l % 16, 8 elements
//     at k-chunk l / 16), loaded straight from global memory to VGPRs - non-temporal 16-byte loads, two register sets of 8 loads per
//     lane, so 8 are always in flight behind the 8 being consumed; the waits are the counted ones the compiler places per use;
//   * the activation rows (zero-padded to 16 columns in registers, never in memory) are staged once per workgroup in LDS, normalised on
//     the way in as gemv_kernel does, in the order the lanes consume them: both operands are indexed by the same k, so the LDS image
//     is permuted to whatever chunk order the weight lanes use (chunk_k below);
//   * K is split over workgroups (slice = blockIdx % S) so that every product of the 8B decode step has >= 2048 wave items; the four
//     waves of a workgroup share the slice's LDS image and take different tiles.  S > 1: every wave writes its fp32 tile to a slab
//     with plain stores and goes on streaming; rows16_combine_kernel, a second small launch, sums the S slabs of a tile in slice order
//     (fixed order, no floating-point atomics: repeat launches are bit-identical) and runs the epilogue.  The in-launch alternative -
//     an arrival counter per tile, the last wave to arrive sums - was built first and measured 3-8 x slower on the five 8B products
//     (DESIGN 8.11): with a 16-row tile as the unit every wave item pays an agent-scope release, which drains its loads in flight;
//   * accumulator lane (q = l / 16, m = l % 16) holds output features 4q .. 4q+3 of the tile for sequence m: a RoPE pair, and (SwiGLU,
//     whose tile interleaves the gate and up rows of 8 hidden units) gate and up of two units, sit in one lane.
// The operand block, the norm-on-load pieces, the epilogues and the host-side operand checks are wstream.h's, shared with gemv_kernel.
// q|k|v here is the batched mode: row m = sequence m at token index 0 of its call, so RoPE table row 0 and k / v into cache[m] at pos[m].
//
// The dynamic int8 kind (WK_I8D: int8 weight rows with bf16 per-row scales, subclasses/int8.py:106-121 with dynamic_int8_act) is the same
// kernel at one byte per element: a lane's 16-byte load is 16 elements = one A operand of v_mfma_i32_16x16x64_i8 (same lane -> row /
// k-chunk map, same accumulator layout), a batch of 8 loads is 16 rows x 512 elements.  The prologue quantises every (normalised)
// activation row as gemv_kernel<.., WK_I8D> does - absmax of the WHOLE row (one wave per row, every workgroup: it adds no launch),
// scale = absmax / 127, codes = rint(x / max(scale, 1e-12)) - and the LDS image holds the int8 codes, M x KS bytes.  The int32 sums
// are exact in any order; a finished sum is dequantised as the reference does, bf16(((float)acc * x_scale[m]) * w_scale[row]), and
// then takes the same epilogue.  Split K: the partial tiles are int32, and the M activation-row scales travel to the combine launch
// in a 16-float header of the workspace (every workgroup computes identical bits; workgroup 0 stores them).
//
// LoRA / DoRA linears (AD_LORA / AD_DORA, instances of their own: the un-adapted builds keep their argument block and registers): the
// adapter term l = t . Bext[row] of a finished tile (t = x . A^T from a previous launch of this stream on the A factors) is a chain of
// one to four more v_mfma_f32_16x16x32_bf16 in the accumulator layout, rows16_adapter, run where the tile's epilogue runs - finish
// (S == 1) or the combine launch - with the GEMV's rounding points (decode.hip, finish): bf16 rows v = bf16(acc + scale * l), DoRA then
// v = bf16(v * c[row]) with the cached factors in wscale, dynamic int8 v = bf16(bf16((acc * xscale) * wscale) + scale * l).
#include "wstream.h"
#include <type_traits>

struct Rows16Args : StreamArgs {
  int64_t c_sb; int Smax;  // q|k|v: the caches' batch stride (row m goes to slot m); a row whose pos[m] is outside [0, Smax) writes no k / v
  int S, KS, ntiles, wgs;  // K slices, slice length (multiple of 256), 16-row tiles, workgroups per slice
  float* slab;             // S > 1: [ntiles][S][64 lanes][4] partial tiles, fp32 (WK_I8D: int32)
  float* xscale;           // WK_I8D, S > 1: [16] the activation rows' scales for the combine launch (the workspace's header)
};

// adapters of the batched stream: none | LoRA (bf16 or dynamic int8 rows) | DoRA (bf16 rows; the cached row factors in wscale)
enum { AD_NONE = 0, AD_LORA = 1, AD_DORA = 2 };
// LoRA (modelling/lora.py:43): bext[s] [n_s, rank[s]] row-major, t [M, sum rank] with the ranks of segment s at t_off[s]; ranks are
// multiples of 16 up to 64 (the t product's segments are 16-row tiles of this stream)
struct Rows16LoraArgs : Rows16Args {
  const bf16_t* bext[3]; int rank[3]; int t_off[3];
  const bf16_t* t; int64_t ldt; float lora_scale;
};
// the argument block of an instance.  (A trait, not std::conditional_t<AD == AD_NONE, ..>: this type is part of the kernels' signatures,
// and an expression on an unnamed enum is mangled with the enum's per-compilation number, which differs between the host and the
// device pass - the host then registers a kernel name the code object does not have.)
template <int AD> struct rows16_args { using type = Rows16LoraArgs; };
template <> struct rows16_args<0> { using type = Rows16Args; };
template <int AD>
using rows16_args_t = typename rows16_args<AD>::type;

// element offset inside a batch (32 chunks of EPL elements = 16 bytes: 256 bf16 or 512 int8 elements) of the chunk that lane group q
// (= lane / 16) takes with load j of the batch: a lane's loads 2i and 2i+1 are adjacent (32 contiguous bytes per lane), so one
// wave-instruction touches the whole 128-byte line of each of its 16 rows and the next one hits the same lines.  (The fragment's
// native order, j * 32 + q * 8 - 16 rows x 64 contiguous bytes per instruction - was built as well and is gone again: DESIGN 8.11.)
template <int EPL>
__device__ __forceinline__ int chunk_k(int j, int q) { return ((j >> 1) * 8 + q * 2 + (j & 1)) * EPL; }

// The adapter term of one 16 x 16 tile in the accumulator layout: lane (q, m) gets l[e] = sum_r Bext[row 4q + e][r] * t[m][r].  A
// operand: the tile's 16 rows of the B factor (lane = row lane % 16, clamped as row_ptr clamps the weight row; ranks 8q .. 8q + 7 of
// chunk j), B operand: t[m][t_off + 32 j + 8 q ..].  Lanes whose rank chunk lies outside their row's ranks and columns m >= M hold
// zeros in registers and load nothing.  SwiGLU: the tile interleaves gate and up rows, which multiply different slices of t - the
// chain runs over the concatenated ranks [t_gate | t_up] (t_off = 0, rank_0), a gate row is zero over the up part and an up row over
// the gate part.  Rank 16 fills half a chunk, 48 one and a half; the chunk test is wave-uniform.
template <int EPI>
__device__ __forceinline__ f32x4_t rows16_adapter(const Rows16LoraArgs& a, int tile, int lane) {
  const int q = lane >> 4, r = lane & 15;
  const bf16_t* bp;   // this lane's row of its B factor
  int lo, rk, R, tb;  // the row's ranks are [lo, lo + rk) of the R ranks of the chain, which start at t column tb
  if constexpr (EPI == GV_SWIGLU) {
    const int mat = (r >> 1) & 1, unit = min(8 * tile + 2 * (r >> 2) + (r & 1), a.N / 2 - 1);
    rk = a.rank[mat]; lo = mat ? a.rank[0] : 0; R = a.rank[0] + a.rank[1]; tb = 0;
    bp = a.bext[mat] + (int64_t)unit * rk;
  } else {
    const int n0 = 16 * tile;
    const int seg = n0 >= a.seg_end[0] ? (n0 >= a.seg_end[1] ? 2 : 1) : 0;
    const int base = seg == 0 ? 0 : a.seg_end[seg - 1];
    rk = a.rank[seg]; lo = 0; R = rk; tb = a.t_off[seg];
    bp = a.bext[seg] + (int64_t)min(n0 - base + r, a.seg_end[seg] - 1 - base) * rk;
  }
  const bf16_t* tp = a.t + (int64_t)r * a.ldt + tb;  // (column m = r; only read for m < M)
  f32x4_t l = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < (EPI == GV_SWIGLU ? 4 : 2); ++j) {
    if (32 * j < R) {
      const int kk = 32 * j + 8 * q;
      u32x4_t bv = {0u, 0u, 0u, 0u}, tv = {0u, 0u, 0u, 0u};
      if (kk >= lo && kk < lo + rk) bv = *reinterpret_cast<const u32x4_t*>(bp + (kk - lo));
      if (r < a.M && kk < R) tv = *reinterpret_cast<const u32x4_t*>(tp + kk);
      l = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, bv), __builtin_bit_cast(bf16x8_t, tv), l, 0, 0, 0);
    }
  }
  return l;
}

// The epilogue of one finished 16 x 16 tile: lane (q = lane / 16, m = lane % 16) holds output features 4q .. 4q+3 of sequence m (SwiGLU:
// gate and up of hidden units 8 tile + 2q, + 1).  WK_I8D: acc = the int32 sums, xscale = the scale of activation row m.  AD: ladd =
// lora_scale * the adapter term of the same features (rows16_adapter); AD_DORA: a.wscale = the rows' cached DoRA factors.
template <int EPI, int WK, int AD, class Acc>
__device__ __forceinline__ void rows16_epilogue(const Rows16Args& a, int tile, int lane, const Acc& acc, float xscale, const f32x4_t& ladd) {
  static_assert(AD != AD_DORA || WK == WK_BF16, "DoRA factors ride on bf16 rows only");
  const int q = lane >> 4, m = lane & 15;
  if (m >= a.M) return;
  float v[4];
  float wsc[4];  // the rows' weight scales (WK_I8D) or DoRA factors (AD_DORA)
  if constexpr (WK == WK_I8D || AD == AD_DORA) {
    if constexpr (EPI == GV_SWIGLU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) wsc[e] = bf2f(a.wscale[e >> 1][min(8 * tile + 2 * q + (e & 1), a.N / 2 - 1)]);
    } else {
      const int n0 = 16 * tile;
      const int seg = n0 >= a.seg_end[0] ? (n0 >= a.seg_end[1] ? 2 : 1) : 0;
      const int base = seg == 0 ? 0 : a.seg_end[seg - 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) wsc[e] = bf2f(a.wscale[seg][min(n0 - base + 4 * q + e, a.seg_end[seg] - 1 - base)]);
    }
  }
  if constexpr (WK == WK_BF16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (AD == AD_NONE) v[e] = bf2f(f2bf(acc[e]));  // the linear's bf16 output
      else v[e] = bf2f(f2bf(acc[e] + ladd[e]));                // base and adapter meet in fp32 (modelling/lora.py:43), as gemv_kernel
      // DoRA (modelling/lora.py:57-59): times the row's cached factor c = m / ||W + s B A||, rounded, as gemv_kernel<.., DORA>
      if constexpr (AD == AD_DORA) v[e] = bf2f(f2bf(v[e] * wsc[e]));
    }
  } else {
    // int32 sum x activation-row scale x weight-row scale in fp32, rounded (int8_mm.py:93-118), as gemv_kernel<.., WK_I8D>; the adapter
    // term meets the base after the base's bf16 rounding (modelling/lora.py:41-43)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = bf2f(f2bf(((float)acc[e] * xscale) * wsc[e]));
      if constexpr (AD != AD_NONE) v[e] = bf2f(f2bf(v[e] + ladd[e]));
    }
  }
  auto kv_off = [&]() -> int64_t {
    const int64_t p = a.pos[m];
    return p >= 0 && p < a.Smax ? (int64_t)m * a.c_sb + p * a.c_ss : -1;
  };
  stream_epilogue<EPI, 4>(a, EPI == GV_SWIGLU ? 8 * tile + 2 * q : 16 * tile + 4 * q, m, a.rope, kv_off, v);
}

// what finish and the combine launch share: the adapter term of the tile (every lane takes part in its MFMAs), then the epilogue
template <int EPI, int WK, int AD, class Acc>
__device__ __forceinline__ void rows16_tile_out(const rows16_args_t<AD>& a, int tile, int lane, const Acc& acc, float xscale) {
  f32x4_t ladd = {0.f, 0.f, 0.f, 0.f};
  if constexpr (AD != AD_NONE) ladd = rows16_adapter<EPI>(a, tile, lane) * a.lora_scale;
  rows16_epilogue<EPI, WK, AD>(a, tile, lane, acc, xscale, ladd);
}

template <int EPI, bool NORM, int WK, int AD = AD_NONE>
__global__ __launch_bounds__(256, 2) void rows16_kernel(const rows16_args_t<AD> a) {
  static_assert(WK == WK_BF16 || WK == WK_I8D, "weight kinds of the batched stream");
  using WT = std::conditional_t<WK == WK_BF16, bf16_t, int8_t>;      // a stored weight element
  using acc_t = std::conditional_t<WK == WK_BF16, f32x4_t, i32x4_t>;
  constexpr int EPL = 16 / (int)sizeof(WT), BATCH = 32 * EPL;        // elements per 16-byte load; per batch of 8 loads x 4 lane groups
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float rs[16];
  __shared__ float qdiv[WK == WK_I8D ? 16 : 1], xsc[WK == WK_I8D ? 16 : 1];  // WK_I8D: the rows' divisors and (bf16-rounded) scales
  u32x4_t* xs = reinterpret_cast<u32x4_t*>(smem);  // [KS / EPL chunks in consumption order][M] (WK_I8D: 16 int8 codes per chunk)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, m = lane & 15;
  const int K = a.K, M = a.M;
  const int s = blockIdx.x % a.S, wg = blockIdx.x / a.S;
  const int k_lo = s * a.KS;
  const int nb = (min(a.KS, K - k_lo) + BATCH - 1) / BATCH;  // batches of this slice (the last may run past K: zeros in LDS)

  // ---- the weight row of this lane in tile t.  SwiGLU: tile row 4j + i = gate (i < 2) or up row of hidden unit 8t + 2j + (i & 1)
  auto row_ptr = [&](int t) -> const WT* {
    const int r = lane & 15;
    if constexpr (EPI == GV_SWIGLU) {
      const int mat = (r >> 1) & 1, unit = min(8 * t + 2 * (r >> 2) + (r & 1), a.N / 2 - 1);
      return reinterpret_cast<const WT*>(a.W[mat]) + (int64_t)unit * a.ldw[mat];
    } else {
      const int n0 = 16 * t;  // segment boundaries are multiples of 16: a tile lies in one segment
      const int seg = n0 >= a.seg_end[0] ? (n0 >= a.seg_end[1] ? 2 : 1) : 0;
      const int base = seg == 0 ? 0 : a.seg_end[seg - 1];
      return reinterpret_cast<const WT*>(a.W[seg]) + (int64_t)min(n0 - base + r, a.seg_end[seg] - 1 - base) * a.ldw[seg];
    }
  };
  auto load_batch = [&](u32x4_t (&w)[8], const WT* wr, int b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k_lo + b * BATCH + chunk_k<EPL>(j, q);
      w[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr + (k < K ? k : 0)));  // chunks past the row end: their x is zero
    }
  };
  const int wave_stride = a.wgs * 4;
  int t = wg * 4 + wave, b = 0;
  const WT *cur = nullptr, *nxt = nullptr;
  u32x4_t WA[8], WB[8];
  // the first weight loads do not depend on x: they fly while the activation rows are staged (and normalised)
  if (t < a.ntiles) { cur = row_ptr(t); load_batch(WA, cur, 0); }

  // ---- the slice of the activation rows into LDS; NORM: 1 / rms of the WHOLE row first, one wave per row.  WK_I8D:
  // quantize_int8_rowwise on the (normalised, bf16-rounded) row, the pieces and the order of gemv_kernel<.., WK_I8D>: the absmax of the
  // WHOLE row in the same pass structure (an all-zero row: scale 0, divisor 1e-12, zero codes, zero output)
  if constexpr (NORM || WK == WK_I8D) {
    for (int r = wave; r < M; r += 4) {
      const bf16_t* xr = a.x + (int64_t)r * a.ldx;
      float rstd = 1.f;
      if constexpr (NORM) {
        float ss = 0.f;
        for (int i = lane * 8; i < K; i += 512) ss = sumsq8(*reinterpret_cast<const u32x4_t*>(xr + i), ss);
        ss = wave_sum(ss);
        rstd = rsqrtf(ss / (float)K + a.eps);
        if (lane == 0) rs[r] = rstd;
      }
      if constexpr (WK == WK_I8D) {
        float amax = 0.f;
        for (int i = lane * 8; i < K; i += 512) {
          u32x4_t v = *reinterpret_cast<const u32x4_t*>(xr + i);
          if constexpr (NORM) v = norm8(v, rstd, a.norm_w + i);
          amax = q8_absmax8(v, amax);
        }
        amax = wave_max(amax);
        const float scale = q8_scale(amax);
        if (lane == 0) { qdiv[r] = q8_divisor(scale); xsc[r] = bf2f(f2bf(scale)); }
      }
    }
    __syncthreads();
  }
  if constexpr (WK == WK_I8D) {
    if (a.S > 1 && blockIdx.x == 0 && tid < M) a.xscale[tid] = xsc[tid];  // for the combine launch
  }
  for (int u = tid; u < nb * 32 * M; u += 256) {
    const int c = u / M, r = u - c * M;  // chunk c of the image = (batch c / 32, load (c / 4) % 8, lane group c % 4)
    const int k = k_lo + (c >> 5) * BATCH + chunk_k<EPL>((c >> 2) & 7, c & 3);
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (k < K) {  // (K is a multiple of EPL: a chunk is live or past the row end as a whole)
      const bf16_t* xp = a.x + (int64_t)r * a.ldx + k;
      v = *reinterpret_cast<const u32x4_t*>(xp);
      if constexpr (NORM) v = norm8(v, rs[r], a.norm_w + k);
      if constexpr (WK == WK_I8D) {
        u32x4_t v1 = *reinterpret_cast<const u32x4_t*>(xp + 8);
        if constexpr (NORM) v1 = norm8(v1, rs[r], a.norm_w + k + 8);
        const float div = qdiv[r];
        const u32x2_t c0 = q8_quant8(v, div), c1 = q8_quant8(v1, div);
        v = u32x4_t{c0[0], c0[1], c1[0], c1[1]};
      }
    }
    xs[u] = v;
  }
  __syncthreads();

  acc_t acc = {};
  auto compute_batch = [&](const u32x4_t (&w)[8], int bb) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      u32x4_t xv = {0u, 0u, 0u, 0u};
      if (m < M) xv = xs[((bb * 8 + j) * 4 + q) * M + m];  // columns M .. 15 of the activation operand are zeros
      if constexpr (WK == WK_BF16) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[j]), __builtin_bit_cast(bf16x8_t, xv), acc, 0, 0, 0);
      else acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4_t, w[j]), __builtin_bit_cast(i32x4_t, xv), acc, 0, 0, 0);
    }
  };
  auto finish = [&](int tile) {
    if (a.S > 1) {  // the partial tile of this slice; rows16_combine_kernel sums the slices and runs the epilogue
      *reinterpret_cast<acc_t*>(a.slab + ((((int64_t)tile * a.S) + s) << 8) + lane * 4) = acc;
      return;
    }
    float xm = 0.f;
    if constexpr (WK == WK_I8D) xm = xsc[min(m, M - 1)];
    rows16_tile_out<EPI, WK, AD>(a, tile, lane, acc, xm);
  };
  // software pipeline over the flattened (tile, batch) sequence of this wave: while one register set is consumed the next batch's 8
  // loads (of this tile or of the wave's next tile) are in flight
  auto body = [&](const u32x4_t (&wc)[8], u32x4_t (&wn)[8]) -> bool {
    int t2 = t, b2 = b + 1;
    bool newt = false;
    if (b2 == nb) { t2 = t + wave_stride; b2 = 0; newt = true; }
    const bool has2 = t2 < a.ntiles;
    if (has2) {
      if (newt) nxt = row_ptr(t2);
      load_batch(wn, newt ? nxt : cur, b2);
    }
    compute_batch(wc, b);
    if (newt) {
      finish(t);
      acc = acc_t{};
      cur = nxt;
    }
    t = t2; b = b2;
    return has2;
  };
  if (t < a.ntiles) {
    while (true) {
      if (!body(WA, WB)) break;
      if (!body(WB, WA)) break;
    }
  }
}

// S > 1: one wave per tile sums the S partial tiles in slice order and runs the epilogue (AD: with the tile's adapter term)
template <int EPI, int WK, int AD = AD_NONE>
__global__ __launch_bounds__(256) void rows16_combine_kernel(const rows16_args_t<AD> a) {
  using acc_t = std::conditional_t<WK == WK_BF16, f32x4_t, i32x4_t>;
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  const float* sl = a.slab + (((int64_t)tile * a.S) << 8) + lane * 4;
  acc_t sum = *reinterpret_cast<const acc_t*>(sl);
  for (int s2 = 1; s2 < a.S; ++s2) sum += *reinterpret_cast<const acc_t*>(sl + ((int64_t)s2 << 8));
  float xm = 0.f;
  if constexpr (WK == WK_I8D) xm = a.xscale[min(lane & 15, a.M - 1)];
  rows16_tile_out<EPI, WK, AD>(a, tile, lane, sum, xm);
}

// fn = the entry point's name for messages
template <int WK, int AD>
static int launch_rows16(const char* fn, const rows16_args_t<AD>& a, int epi, int grid, size_t lds, hipStream_t stream) {
  return stream_with_epilogue(epi, [&](auto e) {
    constexpr int EPI = decltype(e)::value;
    if (a.norm_w) hipLaunchKernelGGL((rows16_kernel<EPI, true, WK, AD>), dim3(grid), dim3(256), lds, stream, a);
    else hipLaunchKernelGGL((rows16_kernel<EPI, false, WK, AD>), dim3(grid), dim3(256), lds, stream, a);
    LLX_LAUNCH_CHECK(fn);
    if (a.S > 1) {
      hipLaunchKernelGGL((rows16_combine_kernel<EPI, WK, AD>), dim3((a.ntiles + 3) / 4), dim3(256), 0, stream, a);
      char name[64];
      snprintf(name, sizeof name, "%s(combine)", fn);
      LLX_LAUNCH_CHECK(name);
    }
    return LLX_OK;
  });
}

// The launcher's dispatch decisions, all of them.  esz = bytes per weight / staged activation element (2: bf16, 1: the dynamic int8
// kind, whose LDS image holds int8 codes); a batch = 8 loads x 4 lane groups x 16 bytes = 512 / esz elements (256 bf16, 512 int8):
//   ntiles = ceil(N / 16) (SwiGLU: ceil(n_0 / 8): a tile is the gate and up rows of 8 hidden units);
//   S (K slices): at least ceil(K / ks_max) with ks_max = the largest multiple of a batch whose M-row LDS image (M x KS x esz bytes)
//     fits 60 KiB, and as many as bring ntiles * S to 2048 wave items while a slice keeps >= one batch, at most 64; from there the
//     first count up to twice that which cuts K into equal slices of whole batches, if there is one;
//   KS = ceil(K / S) rounded up to a batch (the last slice may be shorter, and its last batch may run past K);
//   workgroups per slice: the tiles are dealt to ceil(ntiles / tiles_per_wave) waves with tiles_per_wave = ceil(ntiles * S / 2048).
struct Rows16Plan { int ntiles, S, KS, wgs; };
static Rows16Plan rows16_plan(int64_t M, int64_t N, int64_t K, int epilogue, int64_t esz) {
  Rows16Plan p;
  const int64_t batch = 512 / esz;
  p.ntiles = (int)(epilogue == GV_SWIGLU ? cdiv64(N / 2, 8) : cdiv64(N, 16));
  const int64_t ks_max = (60 * 1024 / (esz * M)) / batch * batch;
  const int64_t s_min = cdiv64(K, ks_max);
  int64_t s_req = cdiv64(2048, p.ntiles);
  if (s_req > cdiv64(K, batch)) s_req = cdiv64(K, batch);
  if (s_req > 64) s_req = 64;
  if (s_req < s_min) s_req = s_min;
  int64_t S = s_req;
  for (int64_t c = s_req; c <= 2 * s_req && c <= 64; ++c)
    if (K % (c * batch) == 0) { S = c; break; }
  p.KS = (int)(cdiv64(cdiv64(K, S), batch) * batch);
  p.S = (int)cdiv64(K, p.KS);
  const int64_t per_wave = cdiv64((int64_t)p.ntiles * p.S, 2048);
  p.wgs = (int)cdiv64(cdiv64(p.ntiles, per_wave), 4);
  return p;
}

// bytes of the workspace of one product: the partial tiles of a split K (fp32 or int32, 1 KiB each; 0 without a split) behind `header`
// bytes (the int8 kind's 16 activation-row scales)
static int64_t rows16_workspace(int64_t M, int64_t N, int64_t K, int epilogue, int64_t esz, int64_t header) {
  if (M < 2 || M > 16 || N < 1 || K < 1 || N >= (1 << 30) || K > 32768) return 0;
  const Rows16Plan p = rows16_plan(M, N, K, epilogue, esz);
  return p.S > 1 ? header + (int64_t)p.ntiles * p.S * 1024 : 0;
}
#define ROWS16_I8_HEADER 64  // 16 floats

// bytes of the workspace llx_gemm_rows16_bf16 needs for this product: the fp32 partial tiles of a split K (0 without a split)
extern "C" int64_t llx_gemm_rows16_workspace_bytes(int64_t M, int64_t N, int64_t K, int epilogue) { return rows16_workspace(M, N, K, epilogue, 2, 0); }
// the same for llx_gemm_rows16_i8: the int32 partial tiles behind the 16-float header of activation-row scales (0 without a split)
extern "C" int64_t llx_gemm_rows16_i8_workspace_bytes(int64_t M, int64_t N, int64_t K, int epilogue) {
  return rows16_workspace(M, N, K, epilogue, 1, ROWS16_I8_HEADER);
}

// the four entry points below: fn = the caller's name for messages, wk = WK_BF16 | WK_I8D, scales = per-row scales of W_s (WK_I8D),
// lo = the adapter operands (null: the un-adapted entry points)
static int rows16_run(const char* fn, int wk, const void* const* scales, const StreamCall& c, const StreamLora* lo, void* workspace, int64_t workspace_bytes,
                      hipStream_t stream) {
  const int esz = wk == WK_BF16 ? 2 : 1;
  const int64_t header = wk == WK_BF16 ? 0 : ROWS16_I8_HEADER;
  Rows16LoraArgs a;
  const int rc = stream_check_fill(fn, a, 2, 16, wk == WK_BF16 ? "one row runs llx_gemv_bf16, more than 16 the MFMA GEMM" : "one row runs llx_gemv_i8, more than 16 the MFMA GEMM",
                                   16 / esz, c.epilogue == GV_SWIGLU ? 1 : 16, c);
  if (rc != LLX_OK) return rc;
  if (wk != WK_BF16) {
    const int rc1 = stream_check_fill_scales(fn, a, "int8", c, scales);
    if (rc1 != LLX_OK) return rc1;
  }
  int ad = AD_NONE;
  if (lo) {
    const void* w[3] = {c.w[0], c.n[1] > 0 ? c.w[1] : nullptr, c.n[2] > 0 ? c.w[2] : nullptr};
    int64_t off = 0;
    for (int s = 0; s < 3; ++s) {
      LLX_REQUIRE((w[s] != nullptr) == (lo->bext[s] != nullptr), "%s: every present weight needs its B factor, and only those (segment %d)", fn, s);
      LLX_REQUIRE(!w[s] || (lo->rank[s] >= 16 && lo->rank[s] <= 64 && lo->rank[s] % 16 == 0),
                  "%s: rank %lld of segment %d must be a multiple of 16, at most 64", fn, (long long)lo->rank[s], s);
      LLX_REQUIRE((uintptr_t)lo->bext[s] % 16 == 0, "%s: B factors must be 16-byte aligned", fn);
      a.bext[s] = (const bf16_t*)lo->bext[s]; a.rank[s] = w[s] ? (int)lo->rank[s] : 0; a.t_off[s] = (int)off;
      off += a.rank[s];
    }
    LLX_REQUIRE(lo->t && (uintptr_t)lo->t % 16 == 0 && lo->ldt % 8 == 0 && lo->ldt >= off,
                "%s: t missing (bf16 [M, sum of ranks], 16-byte aligned, row stride a multiple of 8 and at least the sum of the ranks)", fn);
    a.t = (const bf16_t*)lo->t; a.ldt = lo->ldt; a.lora_scale = lo->scale;
    for (int s = 1; s < 3; ++s)
      if (!w[s]) { a.bext[s] = a.bext[0]; a.rank[s] = a.rank[0]; a.t_off[s] = 0; }  // absent segments repeat segment 0, as W[]
    ad = AD_LORA;
    if (lo->colscale[0] || lo->colscale[1] || lo->colscale[2]) {
      LLX_REQUIRE(wk == WK_BF16, "%s: DoRA factors ride on bf16 rows only", fn);
      const int rc2 = stream_check_fill_scales(fn, a, "DoRA", c, lo->colscale);
      if (rc2 != LLX_OK) return rc2;
      ad = AD_DORA;
    }
  }
  LLX_REQUIRE(!gv_is_qkv(c.epilogue) || (c.n_q > 0 && c.Smax > 0 && c.Smax < (1ll << 31) && c.c_sb % 4 == 0),
              "%s: the q|k|v epilogue needs q heads, a cache length below 2^31 and 8-byte aligned cache slots", fn);
  const Rows16Plan p = rows16_plan(c.M, a.N, c.K, c.epilogue, esz);
  LLX_REQUIRE(p.S == 1 || (workspace && (uintptr_t)workspace % 16 == 0 && workspace_bytes >= header + (int64_t)p.ntiles * p.S * 1024),
              "%s: workspace missing or smaller than %s()", fn, wk == WK_BF16 ? "llx_gemm_rows16_workspace_bytes" : "llx_gemm_rows16_i8_workspace_bytes");
  a.c_sb = c.c_sb; a.Smax = (int)c.Smax;
  a.S = p.S; a.KS = p.KS; a.ntiles = p.ntiles; a.wgs = p.wgs;
  a.xscale = (float*)workspace;
  a.slab = (float*)((char*)workspace + header);
  const int grid = p.wgs * p.S;
  const size_t lds = (size_t)c.M * p.KS * esz;
  if (ad == AD_NONE) {
    const Rows16Args& b = a;  // the un-adapted instances take the base block
    return wk == WK_BF16 ? launch_rows16<WK_BF16, AD_NONE>(fn, b, c.epilogue, grid, lds, stream) : launch_rows16<WK_I8D, AD_NONE>(fn, b, c.epilogue, grid, lds, stream);
  }
  if (ad == AD_DORA) return launch_rows16<WK_BF16, AD_DORA>(fn, a, c.epilogue, grid, lds, stream);
  return wk == WK_BF16 ? launch_rows16<WK_BF16, AD_LORA>(fn, a, c.epilogue, grid, lds, stream) : launch_rows16<WK_I8D, AD_LORA>(fn, a, c.epilogue, grid, lds, stream);
}

extern "C" int llx_gemm_rows16_bf16(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                                    int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                                    void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k,
                                    void* k_cache, void* v_cache, int64_t c_sb, int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos,
                                    void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, c_sb, c_sh, c_ss, Smax, pos};
  return rows16_run("llx_gemm_rows16_bf16", WK_BF16, nullptr, c, nullptr, workspace, workspace_bytes, stream);
}

// The same product on int8 weight rows of the DYNAMIC kind (subclasses/int8.py:112-113, int8_mm.py:93-118; the weight-only kind has
// no batched stream): W_s [n_s, K] int8 row-major (ldw_s in bytes, multiples of 16), scale_s [n_s] bf16 per-row scales, K % 16 == 0.
// Every (normalised) row of x is quantised as llx_quantize_int8_rowwise does, v_mfma_i32_16x16x64_i8 into int32,
// out = bf16(((float)acc * x_scale[m]) * scale[row]) - bit-exact with the reference and with llx_gemv_i8(dynamic = 1) when no norm is
// fused - then the epilogues of llx_gemm_rows16_bf16.  Workspace: llx_gemm_rows16_i8_workspace_bytes().
extern "C" int llx_gemm_rows16_i8(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                                  int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                                  void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k,
                                  void* k_cache, void* v_cache, int64_t c_sb, int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos,
                                  void* workspace, int64_t workspace_bytes, const void* scale0, const void* scale1, const void* scale2,
                                  hipStream_t stream) {
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, c_sb, c_sh, c_ss, Smax, pos};
  const void* const scales[3] = {scale0, scale1, scale2};
  return rows16_run("llx_gemm_rows16_i8", WK_I8D, scales, c, nullptr, workspace, workspace_bytes, stream);
}

// llx_gemm_rows16_bf16 on LoRA linears (modelling/lora.py:43): bext_s bf16 [n_s, rank_s] row-major for every present weight, ranks
// multiples of 16 up to 64, t bf16 [M, sum rank] = x . [A_0; A_1; A_2]^T from a call of llx_gemm_rows16_bf16 on the A factors
// (16-byte aligned, ldt % 8 == 0): out = epilogue(bf16(x . W^T + lora_scale * t_s . bext_s[row])).  colscale_s (bf16 [n_s], all
// present segments or none): DoRA's cached row factors (modelling/lora.py:51-59), out = epilogue(bf16(bf16(..) * colscale[row])) -
// the rounding points of llx_gemv_bf16 / llx_gemv_bf16_dora.  Workspace: llx_gemm_rows16_workspace_bytes().
extern "C" int llx_gemm_rows16_bf16_lora(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                                         int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                                         void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k,
                                         void* k_cache, void* v_cache, int64_t c_sb, int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos,
                                         void* workspace, int64_t workspace_bytes, const void* bext0, const void* bext1, const void* bext2,
                                         int64_t rank0, int64_t rank1, int64_t rank2, const void* t, int64_t ldt, float lora_scale,
                                         const void* colscale0, const void* colscale1, const void* colscale2, hipStream_t stream) {
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, c_sb, c_sh, c_ss, Smax, pos};
  const StreamLora lo = {{bext0, bext1, bext2}, {rank0, rank1, rank2}, t, ldt, lora_scale, {colscale0, colscale1, colscale2}};
  return rows16_run("llx_gemm_rows16_bf16_lora", WK_BF16, nullptr, c, &lo, workspace, workspace_bytes, stream);
}

// llx_gemm_rows16_i8 on LoRA linears: out = epilogue(bf16(bf16(((float)acc * x_scale[m]) * scale[row]) + lora_scale * t_s . bext_s[row])),
// the rounding points of llx_gemv_i8(dynamic = 1); t from llx_gemm_rows16_bf16 on the un-quantised x.  Workspace:
// llx_gemm_rows16_i8_workspace_bytes().
extern "C" int llx_gemm_rows16_i8_lora(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                                       int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                                       void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k,
                                       void* k_cache, void* v_cache, int64_t c_sb, int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos,
                                       void* workspace, int64_t workspace_bytes, const void* scale0, const void* scale1, const void* scale2,
                                       const void* bext0, const void* bext1, const void* bext2, int64_t rank0, int64_t rank1, int64_t rank2,
                                       const void* t, int64_t ldt, float lora_scale, hipStream_t stream) {
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, c_sb, c_sh, c_ss, Smax, pos};
  const StreamLora lo = {{bext0, bext1, bext2}, {rank0, rank1, rank2}, t, ldt, lora_scale, {}};
  const void* const scales[3] = {scale0, scale1, scale2};
  return rows16_run("llx_gemm_rows16_i8_lora", WK_I8D, scales, c, &lo, workspace, workspace_bytes, stream);
}
