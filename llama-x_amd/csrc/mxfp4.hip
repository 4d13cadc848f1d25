// OCP MXFP4 weight-only linears: the quantiser, the dequantiser and the decode GEMV on the packed rows.
//
// The format.  A weight is [N, K], K % 32 == 0; a block is 32 consecutive k of one row.
//   packed uint8 [N, K/2]: byte j = element 2j in bits 0-3, element 2j+1 in bits 4-7; a code is sign << 3 | e2m1 with the magnitudes
//                          0, 0.5, 1, 1.5, 2, 3, 4, 6;
//   scale  uint8 [N, K/32]: the biased exponent b of the block, block scale 2^(b - 127).
// Quantise (fp32): amax = max |x| of the block; amax == 0: b = 127; else e = clamp(floor(log2 amax) - 2, -125, 125), b = e + 127;
// v = |x| * 2^-e (exact), rounded to the nearest magnitude, ties to the code with mantissa bit 0, above 6 saturated; the sign bit is
// the input's.  Dequantise: magnitude * 2^e - with e in [-125, 125] a normal bf16, exact; no kernel meets a denormal.
//
// gemv_mx4_kernel is the weight stream of decode.hip on these rows: a lane's 16-byte non-temporal load is one block (32 codes, one
// scale byte), v_cvt_scalef32_pk_bf16_fp4 turns a byte into two bf16 weights already multiplied by the block scale (the fp32
// b << 23), v_dot2c_f32_bf16 sums them against the bf16 activations of the LDS stage into fp32.  Its rounding points are those of
// llx_gemv_bf16 on the dequantised image: out = epilogue(bf16(sum_k x_k dq(W)_k + lora_scale * t . B[row])), the adapter meets the
// base in fp32.  Operand block, norm-on-load, epilogues, LoRA operands and the wave sum are wstream.h's.
#include "wstream.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ bf16x2_t as_bf16x2(uint32_t v) { return __builtin_bit_cast(bf16x2_t, v); }

// ------------------------------------------------------------------------------------------------- quantiser / dequantiser
// the e2m1 code of a magnitude v >= 0 (already divided by the block scale): the midpoints of the grid, each tie on the side of the
// even code; above 5 everything is 6
__device__ __forceinline__ uint32_t mx4_code(float v) {
  return (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) + (uint32_t)(v > 2.5f) + (uint32_t)(v >= 3.5f) +
         (uint32_t)(v > 5.0f);
}

// one thread = one block: 32 elements in, 16 bytes and a scale byte out
template <bool F32>
__global__ __launch_bounds__(256) void mx4_quantize_kernel(const void* __restrict__ x, int64_t ldx, int64_t N, int KB, uint8_t* __restrict__ packed,
                                                           uint8_t* __restrict__ scale) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * KB) return;
  const int64_t row = t / KB;
  const int kb = (int)(t - row * KB);
  float v[32];
  if constexpr (F32) {
    const f32x4_t* p = reinterpret_cast<const f32x4_t*>((const float*)x + row * ldx + (int64_t)kb * 32);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4_t q = p[i];
      v[4 * i] = q[0]; v[4 * i + 1] = q[1]; v[4 * i + 2] = q[2]; v[4 * i + 3] = q[3];
    }
  } else {
    const u32x4_t* p = reinterpret_cast<const u32x4_t*>((const bf16_t*)x + row * ldx + (int64_t)kb * 32);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4_t q = p[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[8 * i + 2 * e] = bflo(q[e]); v[8 * i + 2 * e + 1] = bfhi(q[e]); }
    }
  }
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));
  // floor(log2 amax) is the exponent field of a normal fp32; a denormal amax (field 0) lands below the clamp either way
  int e = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - 2;
  e = amax == 0.f ? 0 : min(max(e, -125), 125);
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e, a normal fp32
  u32x4_t o = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const uint32_t code = ((__float_as_uint(v[i]) >> 31) << 3) | mx4_code(fabsf(v[i]) * inv);
    o[i >> 3] |= code << (4 * (i & 7));
  }
  *reinterpret_cast<u32x4_t*>(packed + (row * KB + kb) * 16) = o;
  scale[row * KB + kb] = (uint8_t)(e + 127);
}

// x [N, K] bf16 (is_f32 = 0) or fp32 (1), row stride ldx elements (rows 16-byte aligned) -> packed [N, K/2], scale [N, K/32], both
// contiguous.  Non-finite input is the caller's to refuse (subclasses/mxfp4.py: one host check at model-surgery time).
extern "C" int llx_quantize_mxfp4(const void* x, int64_t ldx, int is_f32, int64_t N, int64_t K, void* packed, void* scale, hipStream_t stream) {
  LLX_REQUIRE(x && packed && scale, "llx_quantize_mxfp4: null pointer");
  LLX_REQUIRE(N > 0 && K > 0 && K % 32 == 0 && K <= (1 << 24) && N < (1ll << 31), "llx_quantize_mxfp4: K=%lld must be a positive multiple of 32 (N=%lld)",
              (long long)K, (long long)N);
  LLX_REQUIRE(ldx >= K && ldx % (is_f32 ? 4 : 8) == 0, "llx_quantize_mxfp4: row stride %lld shorter than K or not a multiple of 16 bytes", (long long)ldx);
  LLX_REQUIRE(((uintptr_t)x | (uintptr_t)packed) % 16 == 0, "llx_quantize_mxfp4: pointers must be 16-byte aligned");
  const int64_t blocks = N * (K / 32);
  LLX_REQUIRE(cdiv64(blocks, 256) < (1ll << 31), "llx_quantize_mxfp4: too many blocks");
  const dim3 grid((unsigned)cdiv64(blocks, 256));
  if (is_f32) hipLaunchKernelGGL(mx4_quantize_kernel<true>, grid, dim3(256), 0, stream, x, ldx, N, (int)(K / 32), (uint8_t*)packed, (uint8_t*)scale);
  else hipLaunchKernelGGL(mx4_quantize_kernel<false>, grid, dim3(256), 0, stream, x, ldx, N, (int)(K / 32), (uint8_t*)packed, (uint8_t*)scale);
  LLX_LAUNCH_CHECK("llx_quantize_mxfp4");
  return LLX_OK;
}

// the bf16 bits of code c (4 bits) under the biased block exponent b: integer arithmetic on the exponent field, exact.
// e2m1: exponent field 0 is 0 or 0.5, else (1 + m/2) * 2^(field - 1)
__device__ __forceinline__ uint32_t mx4_bf16_bits(uint32_t c, int b) {
  const uint32_t sign = (c >> 3) << 15, ef = (c >> 1) & 3, m = c & 1;
  if ((c & 7) == 0) return sign;
  const int field = (ef == 0 ? 126 : 126 + (int)ef) + (b - 127);  // 0.5 = 2^-1; (1 + m/2) * 2^(ef - 1)
  return sign | ((uint32_t)field << 7) | ((ef == 0 ? 0u : m) << 6);
}

// one thread = one block.  Plain: out[row, 32 kb ..] as four 16-byte stores, threads walk a row.  Transposed: out[32 kb + i, row],
// threads walk the rows so that a wave's 2-byte stores of one k are neighbours.
template <bool TR>
__global__ __launch_bounds__(256) void mx4_dequantize_kernel(const uint8_t* __restrict__ packed, int64_t ldw, const uint8_t* __restrict__ scale, int64_t lds,
                                                             int64_t N, int KB, bf16_t* __restrict__ out, int64_t ldo) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * KB) return;
  const int64_t row = TR ? t % N : t / KB;
  const int kb = (int)(TR ? t / N : t - row * KB);
  const u32x4_t w = *reinterpret_cast<const u32x4_t*>(packed + row * ldw + (int64_t)kb * 16);
  const int b = scale[row * lds + kb];
  if constexpr (TR) {
#pragma unroll
    for (int i = 0; i < 32; ++i) out[((int64_t)kb * 32 + i) * ldo + row] = (bf16_t)mx4_bf16_bits((w[i >> 3] >> (4 * (i & 7))) & 15, b);
  } else {
    u32x4_t* op = reinterpret_cast<u32x4_t*>(out + row * ldo + (int64_t)kb * 32);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = mx4_bf16_bits((w[q] >> (8 * e)) & 15, b) | (mx4_bf16_bits((w[q] >> (8 * e + 4)) & 15, b) << 16);
      op[q] = o;
    }
  }
}

// packed [N, K/2] (row stride ldw bytes, a multiple of 16), scale [N, K/32] (row stride lds bytes) -> the bf16 image out [N, K] (row stride
// ldo elements, a multiple of 8), or with transpose out [K, N] (any row stride >= N)
extern "C" int llx_dequantize_mxfp4(const void* packed, int64_t ldw, const void* scale, int64_t lds, int64_t N, int64_t K, void* out, int64_t ldo,
                                    int transpose, hipStream_t stream) {
  LLX_REQUIRE(packed && scale && out, "llx_dequantize_mxfp4: null pointer");
  LLX_REQUIRE(N > 0 && K > 0 && K % 32 == 0 && K <= (1 << 24) && N < (1ll << 31), "llx_dequantize_mxfp4: K=%lld must be a positive multiple of 32 (N=%lld)",
              (long long)K, (long long)N);
  LLX_REQUIRE(ldw >= K / 2 && ldw % 16 == 0 && lds >= K / 32, "llx_dequantize_mxfp4: short or unaligned row stride of the packed rows or the scales");
  LLX_REQUIRE(transpose ? ldo >= N : (ldo >= K && ldo % 8 == 0), "llx_dequantize_mxfp4: short or unaligned output row stride %lld", (long long)ldo);
  LLX_REQUIRE((uintptr_t)packed % 16 == 0 && (uintptr_t)out % (transpose ? 2 : 16) == 0, "llx_dequantize_mxfp4: pointers must be 16-byte aligned");
  const int64_t blocks = N * (K / 32);
  LLX_REQUIRE(cdiv64(blocks, 256) < (1ll << 31), "llx_dequantize_mxfp4: too many blocks");
  const dim3 grid((unsigned)cdiv64(blocks, 256));
  if (transpose)
    hipLaunchKernelGGL(mx4_dequantize_kernel<true>, grid, dim3(256), 0, stream, (const uint8_t*)packed, ldw, (const uint8_t*)scale, lds, N, (int)(K / 32),
                       (bf16_t*)out, ldo);
  else
    hipLaunchKernelGGL(mx4_dequantize_kernel<false>, grid, dim3(256), 0, stream, (const uint8_t*)packed, ldw, (const uint8_t*)scale, lds, N, (int)(K / 32),
                       (bf16_t*)out, ldo);
  LLX_LAUNCH_CHECK("llx_dequantize_mxfp4");
  return LLX_OK;
}

// ------------------------------------------------------------------------------------------------- weight-streaming GEMV
struct Mx4Args : GemvArgs {  // W[s]: packed rows (ldw in bytes); sc[s] / lds[s]: the scale bytes of W[s] and their row stride
  const uint8_t* sc[3]; int64_t lds[3];
};

// one block of one weight row (16 bytes, scale = 2^(b - 127) as fp32) against the same 32 activations of MT rows: x[m][q] = elements
// 8q .. 8q+7 of the block as packed bf16 pairs, so byte 4q + j of the block meets x[m][q][j]
template <int MT>
__device__ __forceinline__ void dot32_mx4(const u32x4_t& w, float scale, const u32x4_t (&x)[MT][4], float (&acc)[MT]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bf16x2_t c0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[q], scale, 0);
    const bf16x2_t c1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[q], scale, 1);
    const bf16x2_t c2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[q], scale, 2);
    const bf16x2_t c3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[q], scale, 3);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      // (the elements go through scalars: __builtin_bit_cast on a vector element reads element 0 whatever the index, hipcc 7.2)
      const uint32_t x0 = x[m][q][0], x1 = x[m][q][1], x2 = x[m][q][2], x3 = x[m][q][3];
      acc[m] = __builtin_amdgcn_fdot2_f32_bf16(c0, as_bf16x2(x0), acc[m], false);
      acc[m] = __builtin_amdgcn_fdot2_f32_bf16(c1, as_bf16x2(x1), acc[m], false);
      acc[m] = __builtin_amdgcn_fdot2_f32_bf16(c2, as_bf16x2(x2), acc[m], false);
      acc[m] = __builtin_amdgcn_fdot2_f32_bf16(c3, as_bf16x2(x3), acc[m], false);
    }
  }
}

// Four output rows per wave at a time; a piece is 2048 elements of a row (64 lanes x one block), a step two pieces of the four rows:
// 8 x 16-byte loads (and 8 scale bytes) per lane in flight, two register sets.  K = 4096 is one step, K = 14336 three and a half: a
// piece past the row end is skipped by the whole wave (loads and arithmetic), lanes past the end inside the last piece re-read the
// row's start against zeros.  x stays bf16 in LDS, zero-padded to whole pieces, each piece stored as its lanes' four 16-byte quarters
// one after the other (quarter q of lane l at q * 512 + l * 8 elements), so that every 16-byte read of a wave is conflict-free.
// SWIGLU: the gate and up rows of two hidden units.  LDS traffic: 64 bytes of x per activation row serve 4 x 16 weight bytes.
template <int MT, int EPI, bool NORM>
__global__ __launch_bounds__(256, 2) void gemv_mx4_kernel(const Mx4Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K;
  constexpr int RPW = 4, UPG = 2, PIECE = 2048, PIECES = 2;
  const int npieces = (K + PIECE - 1) / PIECE;
  const int nsteps = (npieces + PIECES - 1) / PIECES;
  const int Kp = npieces * PIECE;
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);  // [MT][Kp]
  float* red = reinterpret_cast<float*>(smem + (size_t)MT * Kp * 2);

  struct Grp { const uint8_t* wr[RPW]; const uint8_t* sr[RPW]; int row0, seg; };
  auto setup = [&](int g, Grp& G) {
    if constexpr (EPI == GV_SWIGLU) {
      const int half = a.N / 2;
      G.row0 = UPG * g; G.seg = 0;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const int64_t row = min(G.row0 + (r % UPG), half - 1);
        G.wr[r] = reinterpret_cast<const uint8_t*>(a.W[r / UPG]) + row * a.ldw[r / UPG];
        G.sr[r] = a.sc[r / UPG] + row * a.lds[r / UPG];
      }
    } else {
      G.row0 = RPW * g;
      G.seg = G.row0 >= a.seg_end[0] ? (G.row0 >= a.seg_end[1] ? 2 : 1) : 0;  // wave-uniform (segment boundaries are multiples of 4)
      const int base = G.seg == 0 ? 0 : a.seg_end[G.seg - 1];
      const int last = a.seg_end[G.seg] - 1 - base;
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        const int64_t row = min(G.row0 - base + r, last);
        G.wr[r] = reinterpret_cast<const uint8_t*>(a.W[G.seg]) + row * a.ldw[G.seg];
        G.sr[r] = a.sc[G.seg] + row * a.lds[G.seg];
      }
    }
  };
  auto load_step = [&](u32x4_t (&w)[8], uint32_t (&sb)[8], const Grp& G, int s) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int p = PIECES * s + j;
      if (p < npieces) {  // wave-uniform
        const int k = p * PIECE + lane * 32;
        const int kk = k < K ? k : 0;  // lanes past the row end re-read its start; their x is zero
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
          w[RPW * j + r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(G.wr[r] + (kk >> 1)));
          sb[RPW * j + r] = G.sr[r][kk >> 5];
        }
      }
    }
  };
  const int nwaves = gridDim.x * 4;
  const int ngroups = EPI == GV_SWIGLU ? (a.N / 2 + UPG - 1) / UPG : (a.N + RPW - 1) / RPW;
  int g = blockIdx.x * 4 + wave, s = 0;
  Grp cur, nxt;
  u32x4_t WA[8], WB[8];
  uint32_t SA[8], SB[8];
  // the first weight loads do not depend on x: they fly while the activation rows are staged (and normalised)
  if (g < ngroups) { setup(g, cur); load_step(WA, SA, cur, 0); }

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
    for (int i = tid * 8; i < Kp; i += 2048) {
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (i < K) {
        v = *reinterpret_cast<const u32x4_t*>(xr + i);
        if constexpr (NORM) v = norm8(v, rstd, a.norm_w + i);
      }
      // element (piece, lane l, quarter q, e) of the row -> piece * 2048 + q * 512 + l * 8 + e
      const int at = (i & ~(PIECE - 1)) + ((i >> 3) & 3) * 512 + ((i & (PIECE - 1)) >> 5) * 8;
      *reinterpret_cast<u32x4_t*>(xs + (size_t)m * Kp + at) = v;
    }
  }
  __syncthreads();

  float acc[RPW][MT];
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
  auto compute_step = [&](const u32x4_t (&w)[8], const uint32_t (&sb)[8], int st) {
#pragma unroll
    for (int j = 0; j < PIECES; ++j) {
      const int p = PIECES * st + j;
      if (p < npieces) {
        u32x4_t xv[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int q = 0; q < 4; ++q) xv[m][q] = *reinterpret_cast<const u32x4_t*>(xs + (size_t)m * Kp + p * PIECE + q * 512 + lane * 8);
#pragma unroll
        for (int r = 0; r < RPW; ++r) dot32_mx4<MT>(w[RPW * j + r], __uint_as_float(sb[RPW * j + r] << 23), xv, acc[r]);
      }
    }
  };
  auto finish = [&](const Grp& G) {
    const int row0 = G.row0, seg = G.seg;
    // LoRA extension: lanes 0 .. rank/8-1 hold 8 elements of the row's B factor each; the term joins the base sum in fp32
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
          acc[r][m] += a.lora_scale * dot8(bv, xf);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[r][m] = wave_sum_valu(acc[r][m]);
    // ---- epilogue: lane m writes token m (every lane holds every sum)
    if (lane < MT && lane < a.M) {
      float v[4];
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        float sm = acc[r][0];
#pragma unroll
        for (int m = 1; m < MT; ++m) sm = lane == m ? acc[r][m] : sm;
        v[r] = bf2f(f2bf(sm));  // the linear's bf16 output
      }
      const int m = lane;
      stream_epilogue<EPI, RPW>(a, row0, m, a.rope + (int64_t)m * 128, [&] { return a.pos[m] * a.c_ss; }, v);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
  };
  // software pipeline over the flattened (row group, step) sequence of this wave, as gemv_kernel
  auto body = [&](const u32x4_t (&wc)[8], const uint32_t (&sc)[8], u32x4_t (&wn)[8], uint32_t (&sn)[8]) -> bool {
    int g2 = g, s2 = s + 1;
    bool newg = false;
    if (s2 == nsteps) { g2 = g + nwaves; s2 = 0; newg = true; }
    const bool has2 = g2 < ngroups;
    if (has2) {
      if (newg) { setup(g2, nxt); load_step(wn, sn, nxt, s2); }
      else load_step(wn, sn, cur, s2);
    }
    compute_step(wc, sc, s);
    if (newg) {
      finish(cur);
      cur = nxt;
    }
    g = g2; s = s2;
    return has2;
  };
  if (g < ngroups) {
    while (true) {
      if (!body(WA, SA, WB, SB)) break;
      if (!body(WB, SB, WA, SA)) break;
    }
  }
}

// llx_gemv_bf16 on MXFP4 weights: W_s = packed rows [n_s, K/2] (ldw_s in bytes, multiples of 16), scale_s = their scale bytes
// [n_s, K/32] (row stride lds_s bytes), K % 32 == 0, M in 1..4.  Segments, norm, epilogues and LoRA operands as llx_gemv_bf16, and its
// rounding points: out = epilogue(bf16(x . dq(W)^T + lora_scale * t . bext[row])), fp32 sums.  The kernel is built for one and two
// activation rows: three and four rows are two passes over the weights (as weight-only int8), and rows longer than 14336 go one by one
// (two of them do not fit the 64-KiB LDS stage).
extern "C" int llx_gemv_mxfp4(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2, int64_t n2,
                              const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out, int64_t ldo,
                              const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache, int64_t c_sh,
                              int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1, const void* bext2, int64_t rank0,
                              int64_t rank1, int64_t rank2, const void* t, int64_t ldt, float lora_scale, const void* scale0, int64_t lds0,
                              const void* scale1, int64_t lds1, const void* scale2, int64_t lds2, hipStream_t stream) {
  const char* fn = "llx_gemv_mxfp4";
  const StreamCall c = {{w0, w1, w2}, {ldw0, ldw1, ldw2}, {n0, n1, n2}, x, ldx, M, K, norm_w, eps, epilogue, out, ldo, res, ldr,
                        rope, n_q, n_k, k_cache, v_cache, 0, c_sh, c_ss, 0, input_pos};
  const StreamLora lo = {{bext0, bext1, bext2}, {rank0, rank1, rank2}, t, ldt, lora_scale, {}};
  Mx4Args a;
  LLX_REQUIRE(K > 0 && K % 32 == 0, "%s: K=%lld must be a multiple of 32 (one scale per block of 32)", fn, (long long)K);
  // (the common checks see the packed rows in bytes: strides in multiples of 16; K in multiples of 32 is checked above)
  const int rc0 = stream_check_fill(fn, a, 1, 4, "larger row counts run the MFMA GEMM on the dequantised image", 16, epilogue == GV_SWIGLU ? 1 : 4, c);
  if (rc0 != LLX_OK) return rc0;
  LLX_REQUIRE(scale0 && (scale1 || n1 == 0) && (scale2 || n2 == 0), "%s: null scale (every MXFP4 weight needs its scale bytes)", fn);
  LLX_REQUIRE(ldw0 >= K / 2 && (n1 == 0 || ldw1 >= K / 2) && (n2 == 0 || ldw2 >= K / 2), "%s: a packed row stride shorter than K / 2 bytes", fn);
  LLX_REQUIRE(lds0 >= K / 32 && (n1 == 0 || lds1 >= K / 32) && (n2 == 0 || lds2 >= K / 32), "%s: a scale row stride shorter than K / 32 bytes", fn);
  LLX_REQUIRE(ldx >= K || M == 1, "%s: activation row stride shorter than K", fn);
  a.sc[0] = (const uint8_t*)scale0; a.sc[1] = (const uint8_t*)(scale1 ? scale1 : scale0); a.sc[2] = (const uint8_t*)(scale2 ? scale2 : scale0);
  a.lds[0] = lds0; a.lds[1] = scale1 ? lds1 : lds0; a.lds[2] = scale2 ? lds2 : lds0;
  const int rc1 = gemv_check_fill_lora(fn, a, c, lo);
  if (rc1 != LLX_OK) return rc1;
  const int grid = gemv_grid(a.N, epilogue, 4);  // four rows per wave
  const int64_t Kp = cdiv64(K, 2048) * 2048;     // the kernel's LDS row length, bf16
  // at most two rows per pass.  There is no 4-row build: next to the two weight register sets its 64 activation registers put 80 bytes
  // of scratch into every instance
  return gemv_passes(fn, a, 2, Kp, 2, [&](const Mx4Args& b, int MT, size_t lds) {
    auto go = [&](auto mt) {
      return stream_with_epilogue(epilogue, [&](auto e) {
        constexpr int MT_ = decltype(mt)::value, EPI = decltype(e)::value;
        if (b.norm_w) hipLaunchKernelGGL((gemv_mx4_kernel<MT_, EPI, true>), dim3(grid), dim3(256), lds, stream, b);
        else hipLaunchKernelGGL((gemv_mx4_kernel<MT_, EPI, false>), dim3(grid), dim3(256), lds, stream, b);
        LLX_LAUNCH_CHECK(fn);
        return LLX_OK;
      });
    };
    return MT == 1 ? go(std::integral_constant<int, 1>{}) : go(std::integral_constant<int, 2>{});
  });
}
