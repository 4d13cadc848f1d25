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
// Epilogues as llx_gemv_bf16: none | + residual | q|k|v in batched mode (row m = sequence m at token index 0 of the call: RoPE table
// row 0, k / v into cache[m] at pos[m]) | SwiGLU.
#include "common.h"

#define HD 128
enum { GV_NONE = 0, GV_RESIDUAL = 1, GV_QKV = 2, GV_SWIGLU = 3 };

struct Rows16Args {
  const bf16_t* W[3]; int64_t ldw[3]; int seg_end[3];
  const bf16_t* x; int64_t ldx;
  const bf16_t* norm_w; float eps;
  int M, N, K;
  bf16_t* out; int64_t ldo;
  const bf16_t* res; int64_t ldr;
  const float* rope; int n_q, n_k;
  bf16_t* kc; bf16_t* vc; int64_t c_sb, c_sh, c_ss; int Smax;
  const int64_t* pos;
  int S, KS, ntiles, wgs;  // K slices, slice length (multiple of 256), 16-row tiles, workgroups per slice
  float* slab;             // S > 1: [ntiles][S][64 lanes][4] fp32 partial tiles
};

// element offset inside a 256-element batch of the 8-element chunk that lane group q (= lane / 16) takes with load j of the batch: a
// lane's loads 2i and 2i+1 are adjacent (32 contiguous bytes per lane), so one wave-instruction touches the whole 128-byte line of
// each of its 16 rows and the next one hits the same lines.  (The fragment's native order, j * 32 + q * 8 - 16 rows x 64 contiguous
// bytes per instruction - was built as well and is gone again: DESIGN 8.11.)
__device__ __forceinline__ int chunk_k(int j, int q) { return (j >> 1) * 64 + q * 16 + (j & 1) * 8; }

// The epilogue of one finished 16 x 16 tile: lane (q = lane / 16, m = lane % 16) holds output features 4q .. 4q+3 of sequence m.
template <int EPI>
__device__ __forceinline__ void rows16_epilogue(const Rows16Args& a, int tile, int lane, const f32x4_t& acc) {
  const int q = lane >> 4, m = lane & 15, M = a.M;
  if (m >= M) return;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = bf2f(f2bf(acc[e]));  // the linear's bf16 output
  if constexpr (EPI == GV_SWIGLU) {
    // h = silu(g) * u with the roundings of the bf16 eager graph (modelling/llama.py:150-152), as swiglu_fwd8
    const int half = a.N / 2, u0 = 8 * tile + 2 * q;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float sg = bf2f(f2bf(v[j] * sigmoidf_(v[j])));
      if (u0 + j < half) a.out[(int64_t)m * a.ldo + u0 + j] = f2bf(sg * v[2 + j]);
    }
  } else if constexpr (EPI == GV_QKV) {
    // apply_rope with table row 0 (every row is token 0 of its sequence's call, modelling/llama.py:207), then KVCache.update of
    // sequence m at pos[m]; a position outside the cache writes nothing
    const int n0 = 16 * tile + 4 * q;
    const bool is_q = n0 < a.n_q, is_k = !is_q && n0 < a.n_q + a.n_k;
    const int hrow = is_q ? n0 : (is_k ? n0 - a.n_q : n0 - a.n_q - a.n_k);
    const int d = hrow & (HD - 1);
    if (is_q || is_k) {
      const float* tp = a.rope + (d >> 1) * 2;
      const float c0 = tp[0], s0 = tp[1], c1 = tp[2], s1 = tp[3];
      const float y0 = v[0] * c0 - v[1] * s0, y1 = v[1] * c0 + v[0] * s0, y2 = v[2] * c1 - v[3] * s1, y3 = v[3] * c1 + v[2] * s1;
      v[0] = y0; v[1] = y1; v[2] = y2; v[3] = y3;
    }
    u32x2_t pk;
    pk[0] = pack_bf2(v[0], v[1]);
    pk[1] = pack_bf2(v[2], v[3]);
    if (is_q) {
      *reinterpret_cast<u32x2_t*>(a.out + (int64_t)m * a.ldo + n0) = pk;
    } else {
      const int64_t p = a.pos[m];
      if (p >= 0 && p < a.Smax) *reinterpret_cast<u32x2_t*>((is_k ? a.kc : a.vc) + (int64_t)m * a.c_sb + (int64_t)(hrow >> 7) * a.c_sh + p * a.c_ss + d) = pk;
    }
  } else {
    const int n0 = 16 * tile + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (n0 + e < a.N) {
        float o = v[e];
        if constexpr (EPI == GV_RESIDUAL) o += bf2f(a.res[(int64_t)m * a.ldr + n0 + e]);  // bf16 output + bf16 residual, rounded
        a.out[(int64_t)m * a.ldo + n0 + e] = f2bf(o);
      }
    }
  }
}

template <int EPI, bool NORM>
__global__ __launch_bounds__(256, 2) void rows16_kernel(const Rows16Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float rs[16];
  u32x4_t* xs = reinterpret_cast<u32x4_t*>(smem);  // [KS / 8 chunks in consumption order][M]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, m = lane & 15;
  const int K = a.K, M = a.M;
  const int s = blockIdx.x % a.S, wg = blockIdx.x / a.S;
  const int k_lo = s * a.KS;
  const int nb = (min(a.KS, K - k_lo) + 255) >> 8;  // 256-element batches of this slice (the last may run past K: zeros in LDS)

  // ---- the weight row of this lane in tile t.  SwiGLU: tile row 4j + i = gate (i < 2) or up row of hidden unit 8t + 2j + (i & 1)
  auto row_ptr = [&](int t) -> const bf16_t* {
    const int r = lane & 15;
    if constexpr (EPI == GV_SWIGLU) {
      const int mat = (r >> 1) & 1, unit = min(8 * t + 2 * (r >> 2) + (r & 1), a.N / 2 - 1);
      return a.W[mat] + (int64_t)unit * a.ldw[mat];
    } else {
      const int n0 = 16 * t;  // segment boundaries are multiples of 16: a tile lies in one segment
      const int seg = n0 >= a.seg_end[0] ? (n0 >= a.seg_end[1] ? 2 : 1) : 0;
      const int base = seg == 0 ? 0 : a.seg_end[seg - 1];
      return a.W[seg] + (int64_t)min(n0 - base + r, a.seg_end[seg] - 1 - base) * a.ldw[seg];
    }
  };
  auto load_batch = [&](u32x4_t (&w)[8], const bf16_t* wr, int b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k_lo + b * 256 + chunk_k(j, q);
      w[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr + (k < K ? k : 0)));  // chunks past the row end: their x is zero
    }
  };
  const int wave_stride = a.wgs * 4;
  int t = wg * 4 + wave, b = 0;
  const bf16_t *cur = nullptr, *nxt = nullptr;
  u32x4_t WA[8], WB[8];
  // the first weight loads do not depend on x: they fly while the activation rows are staged (and normalised)
  if (t < a.ntiles) { cur = row_ptr(t); load_batch(WA, cur, 0); }

  // ---- the slice of the activation rows into LDS; NORM: 1 / rms of the WHOLE row first, one wave per row
  if constexpr (NORM) {
    for (int r = wave; r < M; r += 4) {
      const bf16_t* xr = a.x + (int64_t)r * a.ldx;
      float ss = 0.f;
      for (int i = lane * 8; i < K; i += 512) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(xr + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss += bflo(v[e]) * bflo(v[e]) + bfhi(v[e]) * bfhi(v[e]);
      }
      ss = wave_sum(ss);
      if (lane == 0) rs[r] = rsqrtf(ss / (float)K + a.eps);
    }
    __syncthreads();
  }
  for (int u = tid; u < nb * 32 * M; u += 256) {
    const int c = u / M, r = u - c * M;  // chunk c of the image = (batch c / 32, load (c / 4) % 8, lane group c % 4)
    const int k = k_lo + (c >> 5) * 256 + chunk_k((c >> 2) & 7, c & 3);
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (k < K) {
      v = *reinterpret_cast<const u32x4_t*>(a.x + (int64_t)r * a.ldx + k);
      if constexpr (NORM) {
        const float rstd = rs[r];
        const u32x4_t w = *reinterpret_cast<const u32x4_t*>(a.norm_w + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = pack_bf2(bflo(v[e]) * rstd * bflo(w[e]), bfhi(v[e]) * rstd * bfhi(w[e]));
      }
    }
    xs[u] = v;
  }
  __syncthreads();

  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  auto compute_batch = [&](const u32x4_t (&w)[8], int bb) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      u32x4_t xv = {0u, 0u, 0u, 0u};
      if (m < M) xv = xs[((bb * 8 + j) * 4 + q) * M + m];  // columns M .. 15 of the activation operand are zeros
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[j]), __builtin_bit_cast(bf16x8_t, xv), acc, 0, 0, 0);
    }
  };
  auto finish = [&](int tile) {
    if (a.S > 1) {  // the partial tile of this slice; rows16_combine_kernel sums the slices and runs the epilogue
      *reinterpret_cast<f32x4_t*>(a.slab + ((((int64_t)tile * a.S) + s) << 8) + lane * 4) = acc;
      return;
    }
    rows16_epilogue<EPI>(a, tile, lane, acc);
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
      acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
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

// S > 1: one wave per tile sums the S partial tiles in slice order and runs the epilogue
template <int EPI>
__global__ __launch_bounds__(256) void rows16_combine_kernel(const Rows16Args a) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= a.ntiles) return;
  const float* sl = a.slab + (((int64_t)tile * a.S) << 8) + lane * 4;
  f32x4_t sum = *reinterpret_cast<const f32x4_t*>(sl);
  for (int s2 = 1; s2 < a.S; ++s2) sum += *reinterpret_cast<const f32x4_t*>(sl + ((int64_t)s2 << 8));
  rows16_epilogue<EPI>(a, tile, lane, sum);
}

template <int EPI>
static int launch_rows16(const Rows16Args& a, int grid, size_t lds, hipStream_t stream) {
  if (a.norm_w) hipLaunchKernelGGL((rows16_kernel<EPI, true>), dim3(grid), dim3(256), lds, stream, a);
  else hipLaunchKernelGGL((rows16_kernel<EPI, false>), dim3(grid), dim3(256), lds, stream, a);
  LLX_LAUNCH_CHECK("llx_gemm_rows16_bf16");
  if (a.S > 1) {
    hipLaunchKernelGGL((rows16_combine_kernel<EPI>), dim3((a.ntiles + 3) / 4), dim3(256), 0, stream, a);
    LLX_LAUNCH_CHECK("llx_gemm_rows16_bf16(combine)");
  }
  return LLX_OK;
}

static int launch_rows16_epi(const Rows16Args& a, int epi, int grid, size_t lds, hipStream_t stream) {
  switch (epi) {
    case GV_NONE: return launch_rows16<GV_NONE>(a, grid, lds, stream);
    case GV_RESIDUAL: return launch_rows16<GV_RESIDUAL>(a, grid, lds, stream);
    case GV_QKV: return launch_rows16<GV_QKV>(a, grid, lds, stream);
    default: return launch_rows16<GV_SWIGLU>(a, grid, lds, stream);
  }
}

// The launcher's dispatch decisions, all of them:
//   ntiles = ceil(N / 16) (SwiGLU: ceil(n_0 / 8): a tile is the gate and up rows of 8 hidden units);
//   S (K slices): at least ceil(K / ks_max) with ks_max = the largest multiple of 256 whose M-row LDS image fits 60 KiB, and as many
//     as bring ntiles * S to 2048 wave items while a slice keeps >= 256 elements, at most 64; from there the first count up to twice
//     that which cuts K into equal slices of whole 256-element batches, if there is one;
//   KS = ceil(K / S) rounded up to 256 (the last slice may be shorter, and its last batch may run past K);
//   workgroups per slice: the tiles are dealt to ceil(ntiles / tiles_per_wave) waves with tiles_per_wave = ceil(ntiles * S / 2048).
struct Rows16Plan { int ntiles, S, KS, wgs; };
static Rows16Plan rows16_plan(int64_t M, int64_t N, int64_t K, int epilogue) {
  Rows16Plan p;
  p.ntiles = (int)(epilogue == GV_SWIGLU ? cdiv64(N / 2, 8) : cdiv64(N, 16));
  const int64_t ks_max = (60 * 1024 / (2 * M)) / 256 * 256;
  const int64_t s_min = cdiv64(K, ks_max);
  int64_t s_req = cdiv64(2048, p.ntiles);
  if (s_req > cdiv64(K, 256)) s_req = cdiv64(K, 256);
  if (s_req > 64) s_req = 64;
  if (s_req < s_min) s_req = s_min;
  int64_t S = s_req;
  for (int64_t c = s_req; c <= 2 * s_req && c <= 64; ++c)
    if (K % (c * 256) == 0) { S = c; break; }
  p.KS = (int)(cdiv64(cdiv64(K, S), 256) * 256);
  p.S = (int)cdiv64(K, p.KS);
  const int64_t per_wave = cdiv64((int64_t)p.ntiles * p.S, 2048);
  p.wgs = (int)cdiv64(cdiv64(p.ntiles, per_wave), 4);
  return p;
}

// bytes of the workspace llx_gemm_rows16_bf16 needs for this product: the fp32 partial tiles of a split K (0 without a split)
extern "C" int64_t llx_gemm_rows16_workspace_bytes(int64_t M, int64_t N, int64_t K, int epilogue) {
  if (M < 2 || M > 16 || N < 1 || K < 1 || N >= (1 << 30) || K > 32768) return 0;
  const Rows16Plan p = rows16_plan(M, N, K, epilogue);
  return p.S > 1 ? (int64_t)p.ntiles * p.S * 1024 : 0;
}

extern "C" int llx_gemm_rows16_bf16(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                                    int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue,
                                    void* out, int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k,
                                    void* k_cache, void* v_cache, int64_t c_sb, int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos,
                                    void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const char* fn = "llx_gemm_rows16_bf16";
  LLX_REQUIRE(w0 && x && out, "%s: null pointer", fn);
  LLX_REQUIRE(M >= 2 && M <= 16, "%s: M=%lld outside 2..16 (one row runs llx_gemv_bf16, more than 16 the MFMA GEMM)", fn, (long long)M);
  LLX_REQUIRE(K > 0 && K % 8 == 0 && K <= 32768, "%s: K=%lld must be a multiple of 8 and at most 32768", fn, (long long)K);
  LLX_REQUIRE(n0 > 0 && n1 >= 0 && n2 >= 0 && (w1 || n1 == 0) && (w2 || n2 == 0) && (n1 > 0 || n2 == 0), "%s: bad segment sizes", fn);
  LLX_REQUIRE(epilogue >= GV_NONE && epilogue <= GV_SWIGLU, "%s: unknown epilogue %d", fn, epilogue);
  LLX_REQUIRE(epilogue == GV_SWIGLU || ((n1 == 0 || n0 % 16 == 0) && (n2 == 0 || n1 % 16 == 0)), "%s: inner segment sizes must be multiples of 16", fn);
  LLX_REQUIRE(ldw0 % 8 == 0 && ldw1 % 8 == 0 && ldw2 % 8 == 0 && ldx % 8 == 0, "%s: row strides must be multiples of 16 bytes", fn);
  LLX_REQUIRE(((uintptr_t)w0 | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)x | (uintptr_t)norm_w) % 16 == 0, "%s: pointers must be 16-byte aligned", fn);
  const int64_t N = n0 + n1 + n2;
  LLX_REQUIRE(N < (1 << 30), "%s: too many rows", fn);
  LLX_REQUIRE(epilogue != GV_RESIDUAL || res, "%s: residual missing", fn);
  LLX_REQUIRE(epilogue != GV_SWIGLU || (n0 == n1 && n2 == 0 && w1), "%s: the SwiGLU epilogue takes gate and up weights of equal size", fn);
  LLX_REQUIRE(epilogue != GV_QKV || (rope && k_cache && v_cache && pos), "%s: the q|k|v epilogue needs the RoPE table, both caches and the positions", fn);
  LLX_REQUIRE(epilogue != GV_QKV || (n_q > 0 && n_q % HD == 0 && n_k % HD == 0 && (N - n_q - n_k) % HD == 0 && n_q + n_k <= N && Smax > 0 && Smax < (1ll << 31) &&
                                     (uintptr_t)rope % 8 == 0 && ((uintptr_t)out | (uintptr_t)k_cache | (uintptr_t)v_cache) % 8 == 0 && ldo % 4 == 0 &&
                                     c_sb % 4 == 0 && c_sh % 4 == 0 && c_ss % 4 == 0),
              "%s: bad q|k|v epilogue arguments", fn);
  const Rows16Plan p = rows16_plan(M, N, K, epilogue);
  LLX_REQUIRE(p.S == 1 || (workspace && (uintptr_t)workspace % 16 == 0 && workspace_bytes >= (int64_t)p.ntiles * p.S * 1024),
              "%s: workspace missing or smaller than llx_gemm_rows16_workspace_bytes()", fn);
  Rows16Args a;
  a.W[0] = (const bf16_t*)w0; a.W[1] = (const bf16_t*)(w1 ? w1 : w0); a.W[2] = (const bf16_t*)(w2 ? w2 : w0);
  a.ldw[0] = ldw0; a.ldw[1] = w1 ? ldw1 : ldw0; a.ldw[2] = w2 ? ldw2 : ldw0;
  a.seg_end[0] = (int)n0; a.seg_end[1] = (int)(n0 + n1); a.seg_end[2] = (int)N;
  if (n1 == 0) { a.seg_end[0] = a.seg_end[1] = (int)N; }
  else if (n2 == 0) { a.seg_end[1] = (int)N; }
  a.x = (const bf16_t*)x; a.ldx = ldx; a.norm_w = (const bf16_t*)norm_w; a.eps = eps;
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.out = (bf16_t*)out; a.ldo = ldo; a.res = (const bf16_t*)res; a.ldr = ldr;
  a.rope = rope; a.n_q = (int)n_q; a.n_k = (int)n_k; a.kc = (bf16_t*)k_cache; a.vc = (bf16_t*)v_cache;
  a.c_sb = c_sb; a.c_sh = c_sh; a.c_ss = c_ss; a.Smax = (int)Smax; a.pos = pos;
  a.S = p.S; a.KS = p.KS; a.ntiles = p.ntiles; a.wgs = p.wgs;
  a.slab = (float*)workspace;
  const int grid = p.wgs * p.S;
  const size_t lds = (size_t)M * p.KS * 2;
  return launch_rows16_epi(a, epilogue, grid, lds, stream);
}
