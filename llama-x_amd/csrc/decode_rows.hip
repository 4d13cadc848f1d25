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
#include "wstream.h"

struct Rows16Args : StreamArgs {
  int64_t c_sb; int Smax;  // q|k|v: the caches' batch stride (row m goes to slot m); a row whose pos[m] is outside [0, Smax) writes no k / v
  int S, KS, ntiles, wgs;  // K slices, slice length (multiple of 256), 16-row tiles, workgroups per slice
  float* slab;             // S > 1: [ntiles][S][64 lanes][4] fp32 partial tiles
};

// element offset inside a 256-element batch of the 8-element chunk that lane group q (= lane / 16) takes with load j of the batch: a
// lane's loads 2i and 2i+1 are adjacent (32 contiguous bytes per lane), so one wave-instruction touches the whole 128-byte line of
// each of its 16 rows and the next one hits the same lines.  (The fragment's native order, j * 32 + q * 8 - 16 rows x 64 contiguous
// bytes per instruction - was built as well and is gone again: DESIGN 8.11.)
__device__ __forceinline__ int chunk_k(int j, int q) { return (j >> 1) * 64 + q * 16 + (j & 1) * 8; }

// The epilogue of one finished 16 x 16 tile: lane (q = lane / 16, m = lane % 16) holds output features 4q .. 4q+3 of sequence m (SwiGLU:
// gate and up of hidden units 8 tile + 2q, + 1).
template <int EPI>
__device__ __forceinline__ void rows16_epilogue(const Rows16Args& a, int tile, int lane, const f32x4_t& acc) {
  const int q = lane >> 4, m = lane & 15;
  if (m >= a.M) return;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = bf2f(f2bf(acc[e]));  // the linear's bf16 output
  auto kv_off = [&]() -> int64_t {
    const int64_t p = a.pos[m];
    return p >= 0 && p < a.Smax ? (int64_t)m * a.c_sb + p * a.c_ss : -1;
  };
  stream_epilogue<EPI, 4>(a, EPI == GV_SWIGLU ? 8 * tile + 2 * q : 16 * tile + 4 * q, m, a.rope, kv_off, v);
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
      for (int i = lane * 8; i < K; i += 512) ss = sumsq8(*reinterpret_cast<const u32x4_t*>(xr + i), ss);
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
      if constexpr (NORM) v = norm8(v, rs[r], a.norm_w + k);
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
  Rows16Args a;
  const int rc = stream_check_fill(fn, a, 2, 16, "one row runs llx_gemv_bf16, more than 16 the MFMA GEMM", 8, epilogue == GV_SWIGLU ? 1 : 16, w0, ldw0, n0, w1, ldw1,
                                   n1, w2, ldw2, n2, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr, rope, n_q, n_k, k_cache, v_cache, c_sh, c_ss, pos);
  if (rc != LLX_OK) return rc;
  LLX_REQUIRE(epilogue != GV_QKV || (n_q > 0 && Smax > 0 && Smax < (1ll << 31) && c_sb % 4 == 0),
              "%s: the q|k|v epilogue needs q heads, a cache length below 2^31 and 8-byte aligned cache slots", fn);
  const Rows16Plan p = rows16_plan(M, a.N, K, epilogue);
  LLX_REQUIRE(p.S == 1 || (workspace && (uintptr_t)workspace % 16 == 0 && workspace_bytes >= (int64_t)p.ntiles * p.S * 1024),
              "%s: workspace missing or smaller than llx_gemm_rows16_workspace_bytes()", fn);
  a.c_sb = c_sb; a.Smax = (int)Smax;
  a.S = p.S; a.KS = p.KS; a.ntiles = p.ntiles; a.wgs = p.wgs;
  a.slab = (float*)workspace;
  const int grid = p.wgs * p.S;
  const size_t lds = (size_t)M * p.KS * 2;
  return launch_rows16_epi(a, epilogue, grid, lds, stream);
}
