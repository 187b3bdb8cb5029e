// The W8A8 int8 decoder layer, fused.  Dynamic per-token int8 quantisation is a row-wise
// operation like RMSNorm and SiLU*mul, so it rides in the same kernels: every kernel here that ends in an int8
// activation owns ONE ROW PER WORKGROUP, finds the row's absmax after producing it and stores int8 + one fp32 scale.
//
// Producers        mi_rmsnorm_int8, mi_silu_and_mul_int8: the 16-bit producer + mi_int8_quant_per_token in one launch.
// GEMM + consumer  mi_int8_gemm_add_rmsnorm_int8, mi_int8_gemm_rope_kvwrite, mi_int8_gemm_silu_mul_int8: the decode
//                  kernel of int8_gemm.hip leaves raw int32 accumulators in slab[S][M][N] (its "partial" launch, also
//                  when S == 1) and ONE consumer kernel sums the slabs (exact), applies the GEMM's epilogue
//                  x = round_T(((float)acc * sa[m]) * sb[n]) and the next op(s) of the layer.  Two launches per call.
// Every rounding of the unfused sequence (mi_int8_gemm -> mi_rmsnorm / mi_rope_neox + mi_kv_write / mi_silu_and_mul ->
// mi_int8_quant_per_token) is reproduced in its order, so the results are bit-identical to it.
//
// Row kernels, work split: thread t of the workgroup owns the 8-element vectors t, t + NT, t + 2 NT, ... of its row
//   (16-byte loads, 16-byte T stores, 8-byte int8 stores).  Three sweeps over the thread's own vectors: (1) produce the
//   fp32 row [norm: x (+ residual), residual written back, sum of squares; silu: the T-rounded product], (2) [norm only]
//   scale by rsqrt and the weight, round to T, absmax, (3) quantise.  Between the sweeps the row stays on the CU:
//     narrow rows (at most 2 vectors per thread: H or I <= 4096 at 256 threads) in registers, and EVERY global load
//       of the thread -- x or the first 8 slabs of both vectors, the residual, the norm weight, the column scales --
//       is requested before the first dependent add: the kernel is latency-bound and pays one memory latency;
//     wide rows parked in LDS, each thread reading back only what it wrote (no barrier for the park): norm rows as
//       fp32 in two 16-byte planes (conflict-free ds_*_b128; 4 H bytes, 64 KiB at H = 16384), silu rows as packed T
//       (2 I bytes, 56 KiB at I = 28672).  Parking instead of re-reading from L2 because the row a norm kernel needs
//       again is the fp32 sum x + residual, which exists nowhere in memory (the residual is written back rounded, and a
//       slab row would have to be summed again); one strategy serves all five row kernels.
//   Reductions: wave shuffles, then one LDS word per wave.  The norm kernels keep mi_rmsnorm's 256 threads, column
//   ownership and summation order -- the sum of squares is a float sum and its order is part of the bits; max is
//   order-free, so the wide silu kernels use 512 threads.
// No atomics, no memset, no allocation, no synchronisation: capturable.
#include "common.h"

#include <type_traits>

MI_INTERNAL void mi_int8_gemm_plan_splits(int64_t N, int64_t K, int* S, int* per);
MI_INTERNAL int mi_int8_gemm_partial(const void* a, const void* b_nk, int32_t* slab, int64_t M, int64_t N, int64_t K,
                                     int64_t lda, int64_t ldb, void* stream);

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int kNormThreads = 256;   // = mi_rmsnorm's: the column ownership fixes the order of the sum of squares
constexpr int kNormSB = 8;          // slabs per batch of loads (norm consumer: 2 x 16 bytes per slab and vector)
constexpr int kPairSB = 4;          // silu / rope consumers: 4 x 16 bytes per slab and vector
constexpr int64_t kMaxRows = 256;   // the int8 decode kernel's pass
constexpr int64_t kMaxH = 16384, kMaxI = 65536;

template <typename T> __device__ __forceinline__ float rnd(float v) { return round_to<T>(v); }

template <typename T> __device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[2 * j] = Elem<T>::lo(w[j]); f[2 * j + 1] = Elem<T>::hi(w[j]); }
}
template <typename T> __device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  return make_uint4(pack2<T>(f[0], f[1]), pack2<T>(f[2], f[3]), pack2<T>(f[4], f[5]), pack2<T>(f[6], f[7]));
}
__device__ __forceinline__ float absmax8(const float (&f)[8], float mx) {
#pragma unroll
  for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(f[j]));
  return mx;
}
// 8 T-valued floats -> 8 int8 bytes, the arithmetic of int8_quant.hip: roundf is round-half-away, |f * mult| <= 127 (1 + 2^-22)
__device__ __forceinline__ uint2 quant8(const float (&f)[8], float mult) {
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j >> 2] |= ((uint32_t)(int)roundf(f[j] * mult) & 0xffu) << (8 * (j & 3));
  return make_uint2(w[0], w[1]);
}

// workgroup reductions: wave shuffles + one LDS word per wave; the sum adds the waves left to right as mi_rmsnorm does
template <int NT> __device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) s += red[w];
  return s;
}
template <int NT> __device__ __forceinline__ float block_max(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) s = fmaxf(s, red[w]);
  return s;
}

// where a GEMM result row comes from: SLAB == false: T-typed x; SLAB == true: S int32 slabs [S][M][N] + the scales
struct SlabSrc {
  const int32_t* slab;
  const float* sa;   // [M]
  const float* sb;   // [N]
  int S;
};

// the absmax -> (scale, multiplier) step of mi_int8_quant_per_token
__device__ __forceinline__ float finish_scale(float mx, float* scales, int64_t row) {
  mx = fmaxf(mx, 1e-10f);
  if (threadIdx.x == 0) scales[row] = mx / 127.0f;
  return (1.0f / mx) * 127.0f;
}

// ------------------------------------------------------------------------------------------------ (add +) RMSNorm -> int8
// layers/layernorm.py:128-146 (forward_native) + per_token_quant_int8 (w8a8_int8.py:136-145).  VPT > 0: that many
// vectors per thread in registers; VPT == 0: any width, the row parked in LDS.
template <typename T> struct NormRow {
  const T* x;          // !SLAB
  int64_t ldx;
  SlabSrc g;           // SLAB
  T* residual;         // nullable, in/out
  const T* w;
  T* out;              // nullable
  int8_t* q;           // nullable
  float* qs;
  int64_t ldr, ldo, M, H;
  float eps;
};

template <typename T, int VPT, bool SLAB>
__global__ __launch_bounds__(kNormThreads) void norm_int8_kernel(const NormRow<T> p) {
  constexpr bool WIDE = VPT == 0;
  constexpr int NR = WIDE ? 1 : VPT, SB = kNormSB, NT = kNormThreads;
  extern __shared__ __attribute__((aligned(16))) char park_raw[];
  __shared__ float red_s[NT / 64], red_m[NT / 64];
  f32x4* park = (f32x4*)park_raw;                      // WIDE: plane 0 = elements 0..3 of every vector, plane 1 = 4..7
  const int64_t row = blockIdx.x, nvec = p.H / 8;
  const int nit = WIDE ? (int)((nvec + NT - 1) / NT) : VPT;
  const float sav = SLAB ? p.g.sa[row] : 0.f;
  float v[NR][8];
  uint4 xr[NR], rr[NR], wr[NR];
  i32x4 la[NR][SB], lb[NR][SB];
  f32x4 sb0[NR], sb1[NR];

  auto put = [&](int i, int64_t c, const float (&f)[8]) __attribute__((always_inline)) {
    if constexpr (WIDE) {
      park[c] = f32x4{f[0], f[1], f[2], f[3]};
      park[nvec + c] = f32x4{f[4], f[5], f[6], f[7]};
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = f[j];
    }
  };
  auto get = [&](int i, int64_t c, float (&f)[8]) __attribute__((always_inline)) {
    if constexpr (WIDE) {
      const f32x4 a = park[c], b = park[nvec + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) { f[j] = a[j]; f[4 + j] = b[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = v[i][j];
    }
  };
  // every global load of vector c into register slot k
  auto load = [&](int k, int64_t c) __attribute__((always_inline)) {
    if constexpr (SLAB) {
#pragma unroll
      for (int s = 0; s < SB; ++s)
        if (s < p.g.S) {
          const int32_t* src = p.g.slab + ((int64_t)s * p.M + row) * p.H + c * 8;
          la[k][s] = *(const i32x4*)src;
          lb[k][s] = *(const i32x4*)(src + 4);
        }
      sb0[k] = *(const f32x4*)(p.g.sb + c * 8);
      sb1[k] = *(const f32x4*)(p.g.sb + c * 8 + 4);
    } else {
      xr[k] = *(const uint4*)(p.x + row * p.ldx + c * 8);
    }
    if (p.residual) rr[k] = *(const uint4*)(p.residual + row * p.ldr + c * 8);
    wr[k] = *(const uint4*)(p.w + c * 8);
  };

  if constexpr (!WIDE) {
#pragma unroll
    for (int i = 0; i < VPT; ++i)
      if (threadIdx.x + i * NT < nvec) load(i, threadIdx.x + i * NT);
  }
  // ---- sweep 1: x (+ residual) in fp32, residual written back, sum of squares
  float ss = 0.f;
#pragma unroll NR
  for (int i = 0; i < nit; ++i) {
    const int64_t c = threadIdx.x + (int64_t)i * NT;
    const int k = WIDE ? 0 : i;
    if (c < nvec) {
      if constexpr (WIDE) load(0, c);
      float x[8];
      if constexpr (SLAB) {
        int acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0;
#pragma unroll
        for (int s = 0; s < SB; ++s)
          if (s < p.g.S) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[j] += la[k][s][j]; acc[4 + j] += lb[k][s][j]; }
          }
        for (int s0 = SB; s0 < p.g.S; s0 += SB) {       // more than SB slabs: further batches (int32 sums commute)
          i32x4 a[SB], b[SB];
#pragma unroll
          for (int s = 0; s < SB; ++s)
            if (s0 + s < p.g.S) {
              const int32_t* src = p.g.slab + ((int64_t)(s0 + s) * p.M + row) * p.H + c * 8;
              a[s] = *(const i32x4*)src;
              b[s] = *(const i32x4*)(src + 4);
            }
#pragma unroll
          for (int s = 0; s < SB; ++s)
            if (s0 + s < p.g.S) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { acc[j] += a[s][j]; acc[4 + j] += b[s][j]; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {                  // mi_int8_gemm's epilogue: (acc * sa) * sb, one rounding to T
          x[j] = rnd<T>(((float)acc[j] * sav) * sb0[k][j]);
          x[4 + j] = rnd<T>(((float)acc[4 + j] * sav) * sb1[k][j]);
        }
      } else {
        unpack8<T>(xr[k], x);
      }
      if (p.residual) {
        float r[8];
        unpack8<T>(rr[k], r);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] += r[j];
        *(uint4*)(p.residual + row * p.ldr + c * 8) = pack8<T>(x);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
      put(i, c, x);
    }
  }
  ss = block_sum<NT>(ss, red_s);
  const float inv = rsqrtf(ss / (float)p.H + p.eps);
  // ---- sweep 2: y = round_T(x * inv * w), `out`, absmax
  float mx = 0.f;
#pragma unroll NR
  for (int i = 0; i < nit; ++i) {
    const int64_t c = threadIdx.x + (int64_t)i * NT;
    if (c < nvec) {
      float x[8], wf[8], o[8];
      get(i, c, x);
      if constexpr (WIDE) unpack8<T>(*(const uint4*)(p.w + c * 8), wf);
      else unpack8<T>(wr[i], wf);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rnd<T>(x[j] * inv * wf[j]);
      if (p.out) *(uint4*)(p.out + row * p.ldo + c * 8) = pack8<T>(o);
      mx = absmax8(o, mx);
      put(i, c, o);
    }
  }
  if (!p.q) return;
  const float mult = finish_scale(block_max<NT>(mx, red_m), p.qs, row);
  // ---- sweep 3: int8
#pragma unroll NR
  for (int i = 0; i < nit; ++i) {
    const int64_t c = threadIdx.x + (int64_t)i * NT;
    if (c < nvec) {
      float o[8];
      get(i, c, o);
      *(uint2*)(p.q + row * p.H + c * 8) = quant8(o, mult);
    }
  }
}

template <typename T, bool SLAB>
void launch_norm(const NormRow<T>& p, hipStream_t st) {
  const int vpt = (int)cdiv64(p.H / 8, kNormThreads);
  if (vpt <= 1) norm_int8_kernel<T, 1, SLAB><<<(unsigned)p.M, kNormThreads, 0, st>>>(p);
  else if (vpt <= 2) norm_int8_kernel<T, 2, SLAB><<<(unsigned)p.M, kNormThreads, 0, st>>>(p);
  else norm_int8_kernel<T, 0, SLAB><<<(unsigned)p.M, kNormThreads, (size_t)p.H * 4, st>>>(p);
}

template <bool SLAB>
int run_norm(const void* x, int64_t ldx, const SlabSrc& g, void* residual, const void* weight, void* out, void* q,
             float* qs, int64_t M, int64_t H, int64_t ldr, int64_t ldo, float eps, int dtype, void* stream) {
  auto fill = [&](auto* tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    NormRow<T> p;
    p.x = (const T*)x; p.ldx = ldx; p.g = g; p.residual = (T*)residual; p.w = (const T*)weight; p.out = (T*)out;
    p.q = (int8_t*)q; p.qs = qs; p.ldr = ldr; p.ldo = ldo; p.M = M; p.H = H; p.eps = eps;
    launch_norm<T, SLAB>(p, (hipStream_t)stream);
  };
  if (dtype == MI_BF16) fill((bf16_t*)nullptr);
  else fill((f16_t*)nullptr);
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ SiLU * mul -> int8
// layers/activation.py:56-58 + per_token_quant_int8.  The row of I products must exist before its first byte can be
// stored (the scale needs the whole row): it waits as packed T, in registers (VPT > 0) or in LDS (VPT == 0).
template <typename T> struct SiluRow {
  const T* x;          // !SLAB: [M, 2I] = [gate | up], row stride ldx
  int64_t ldx;
  SlabSrc g;           // SLAB: N = 2I
  T* out;              // nullable
  int8_t* q;
  float* qs;
  int64_t ldo, M, I;
};

template <typename T, int VPT, int NT, bool SLAB>
__global__ __launch_bounds__(NT) void silu_int8_kernel(const SiluRow<T> p) {
  constexpr bool WIDE = VPT == 0;
  constexpr int NR = WIDE ? 1 : VPT, SB = kPairSB;
  extern __shared__ __attribute__((aligned(16))) char park_raw[];
  __shared__ float red_m[NT / 64];
  uint4* park = (uint4*)park_raw;
  const int64_t row = blockIdx.x, nvec = p.I / 8, N = 2 * p.I;
  const int nit = WIDE ? (int)((nvec + NT - 1) / NT) : VPT;
  const float sav = SLAB ? p.g.sa[row] : 0.f;
  uint4 keep[NR], gr[NR], ur[NR];
  i32x4 ga[NR][SB], gb[NR][SB], ua[NR][SB], ub[NR][SB];
  f32x4 sg0[NR], sg1[NR], su0[NR], su1[NR];

  auto load = [&](int k, int64_t c) __attribute__((always_inline)) {
    if constexpr (SLAB) {
#pragma unroll
      for (int s = 0; s < SB; ++s)
        if (s < p.g.S) {
          const int32_t* src = p.g.slab + ((int64_t)s * p.M + row) * N + c * 8;
          ga[k][s] = *(const i32x4*)src; gb[k][s] = *(const i32x4*)(src + 4);
          ua[k][s] = *(const i32x4*)(src + p.I); ub[k][s] = *(const i32x4*)(src + p.I + 4);
        }
      sg0[k] = *(const f32x4*)(p.g.sb + c * 8); sg1[k] = *(const f32x4*)(p.g.sb + c * 8 + 4);
      su0[k] = *(const f32x4*)(p.g.sb + p.I + c * 8); su1[k] = *(const f32x4*)(p.g.sb + p.I + c * 8 + 4);
    } else {
      gr[k] = *(const uint4*)(p.x + row * p.ldx + c * 8);
      ur[k] = *(const uint4*)(p.x + row * p.ldx + p.I + c * 8);
    }
  };
  if constexpr (!WIDE) {
#pragma unroll
    for (int i = 0; i < VPT; ++i)
      if (threadIdx.x + i * NT < nvec) load(i, threadIdx.x + i * NT);
  }
  // ---- sweep 1: o = round_T(round_T(silu(gate)) * up), `out`, absmax
  float mx = 0.f;
#pragma unroll NR
  for (int i = 0; i < nit; ++i) {
    const int64_t c = threadIdx.x + (int64_t)i * NT;
    const int k = WIDE ? 0 : i;
    if (c < nvec) {
      if constexpr (WIDE) load(0, c);
      float gv[8], uv[8], o[8];
      if constexpr (SLAB) {
        int g[8], u[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { g[j] = 0; u[j] = 0; }
#pragma unroll
        for (int s = 0; s < SB; ++s)
          if (s < p.g.S) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { g[j] += ga[k][s][j]; g[4 + j] += gb[k][s][j]; u[j] += ua[k][s][j]; u[4 + j] += ub[k][s][j]; }
          }
        for (int s0 = SB; s0 < p.g.S; s0 += SB) {
          i32x4 a[SB], b[SB], e[SB], f[SB];
#pragma unroll
          for (int s = 0; s < SB; ++s)
            if (s0 + s < p.g.S) {
              const int32_t* src = p.g.slab + ((int64_t)(s0 + s) * p.M + row) * N + c * 8;
              a[s] = *(const i32x4*)src; b[s] = *(const i32x4*)(src + 4);
              e[s] = *(const i32x4*)(src + p.I); f[s] = *(const i32x4*)(src + p.I + 4);
            }
#pragma unroll
          for (int s = 0; s < SB; ++s)
            if (s0 + s < p.g.S) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { g[j] += a[s][j]; g[4 + j] += b[s][j]; u[j] += e[s][j]; u[4 + j] += f[s][j]; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          gv[j] = rnd<T>(((float)g[j] * sav) * sg0[k][j]); gv[4 + j] = rnd<T>(((float)g[4 + j] * sav) * sg1[k][j]);
          uv[j] = rnd<T>(((float)u[j] * sav) * su0[k][j]); uv[4 + j] = rnd<T>(((float)u[4 + j] * sav) * su1[k][j]);
        }
      } else {
        unpack8<T>(gr[k], gv);
        unpack8<T>(ur[k], uv);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rnd<T>(rnd<T>(silu_f32(gv[j])) * uv[j]);
      const uint4 packed = pack8<T>(o);
      if (p.out) *(uint4*)(p.out + row * p.ldo + c * 8) = packed;
      mx = absmax8(o, mx);
      if constexpr (WIDE) park[c] = packed;
      else keep[i] = packed;
    }
  }
  const float mult = finish_scale(block_max<NT>(mx, red_m), p.qs, row);
  // ---- sweep 2: int8
#pragma unroll NR
  for (int i = 0; i < nit; ++i) {
    const int64_t c = threadIdx.x + (int64_t)i * NT;
    if (c < nvec) {
      float o[8];
      if constexpr (WIDE) unpack8<T>(park[c], o);
      else unpack8<T>(keep[i], o);
      *(uint2*)(p.q + row * p.I + c * 8) = quant8(o, mult);
    }
  }
}

template <bool SLAB>
int run_silu(const void* x, int64_t ldx, const SlabSrc& g, void* out, void* q, float* qs, int64_t M, int64_t I,
             int64_t ldo, int dtype, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  auto go = [&](auto* tag) {
    typedef typename std::remove_pointer<decltype(tag)>::type T;
    SiluRow<T> p;
    p.x = (const T*)x; p.ldx = ldx; p.g = g; p.out = (T*)out; p.q = (int8_t*)q; p.qs = qs; p.ldo = ldo; p.M = M; p.I = I;
    const int vpt = (int)cdiv64(I / 8, 256);
    if (vpt <= 1) silu_int8_kernel<T, 1, 256, SLAB><<<(unsigned)M, 256, 0, st>>>(p);
    else if (vpt <= 2) silu_int8_kernel<T, 2, 256, SLAB><<<(unsigned)M, 256, 0, st>>>(p);
    else silu_int8_kernel<T, 0, 512, SLAB><<<(unsigned)M, 512, (size_t)I * 2, st>>>(p);
  };
  if (dtype == MI_BF16) go((bf16_t*)nullptr);
  else go((f16_t*)nullptr);
  return MI_OK;
}

// ------------------------------------------------------------------------------------------------ slabs (qkv) -> RoPE -> q, KV pool
// == mi_int8_gemm's epilogue, RotaryEmbedding.forward_native (neox, rotary_embedding.py:49-166) on q and k,
// set_kv_buffer (memory_pool.py:454-455).  Not a row kernel (nothing row-wide is needed): one thread per 8 rotation
// pairs / 16 v elements, all loads of a slab batch and the position / slot requested before the first add.
template <typename T>
__global__ __launch_bounds__(256) void slab_rope_kvwrite_int8_kernel(const SlabSrc g, const int64_t* __restrict__ positions,
                                                                     const float* __restrict__ cos_sin, T* __restrict__ q_out,
                                                                     T* __restrict__ k_cache, T* __restrict__ v_cache,
                                                                     const int64_t* __restrict__ loc, int64_t tokens, int Hq,
                                                                     int Hkv, int D, int64_t ldq, int64_t cache_stride_k,
                                                                     int64_t cache_stride_v) {
  constexpr int SB = kPairSB;
  const int half = D / 2, vph = half / 8;
  const int heads = Hq + 2 * Hkv;
  const int64_t N = (int64_t)heads * D;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_tok = (int64_t)heads * vph;
  if (gid >= tokens * per_tok) return;
  const int64_t t = gid / per_tok;
  const int rem = (int)(gid % per_tok);
  const int h = rem / vph, c = rem % vph;
  const int64_t col = (int64_t)h * D + c * 8;
  const int64_t pos = (h < Hq + Hkv) ? positions[t] : 0;
  const int64_t slot = (h >= Hq) ? loc[t] : 0;
  const float sav = g.sa[t];
  const f32x4 sl0 = *(const f32x4*)(g.sb + col), sl1 = *(const f32x4*)(g.sb + col + 4);
  const f32x4 sh0 = *(const f32x4*)(g.sb + col + half), sh1 = *(const f32x4*)(g.sb + col + half + 4);
  int acc1[8], acc2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { acc1[j] = 0; acc2[j] = 0; }
  for (int s0 = 0; s0 < g.S; s0 += SB) {
    i32x4 a[SB], b[SB], e[SB], f[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s)
      if (s0 + s < g.S) {
        const int32_t* base = g.slab + ((int64_t)(s0 + s) * tokens + t) * N + col;
        a[s] = *(const i32x4*)base; b[s] = *(const i32x4*)(base + 4);
        e[s] = *(const i32x4*)(base + half); f[s] = *(const i32x4*)(base + half + 4);
      }
#pragma unroll
    for (int s = 0; s < SB; ++s)
      if (s0 + s < g.S) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc1[j] += a[s][j]; acc1[4 + j] += b[s][j]; acc2[j] += e[s][j]; acc2[4 + j] += f[s][j]; }
      }
  }
  float x1[8], x2[8], o1[8], o2[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x1[j] = rnd<T>(((float)acc1[j] * sav) * sl0[j]); x1[4 + j] = rnd<T>(((float)acc1[4 + j] * sav) * sl1[j]);
    x2[j] = rnd<T>(((float)acc2[j] * sav) * sh0[j]); x2[4 + j] = rnd<T>(((float)acc2[4 + j] * sav) * sh1[j]);
  }
  if (h < Hq + Hkv) {  // q or k head: rotate, every product and sum rounded to T as mi_rope_neox does
    const float* cs = cos_sin + pos * D;
    const f32x4 c0 = *(const f32x4*)(cs + c * 8), c1 = *(const f32x4*)(cs + c * 8 + 4);
    const f32x4 s0 = *(const f32x4*)(cs + half + c * 8), s1 = *(const f32x4*)(cs + half + c * 8 + 4);
    const float cv[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    const float sv[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float co = rnd<T>(cv[j]), si = rnd<T>(sv[j]);
      o1[j] = rnd<T>(rnd<T>(x1[j] * co) - rnd<T>(x2[j] * si));
      o2[j] = rnd<T>(rnd<T>(x2[j] * co) + rnd<T>(x1[j] * si));
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) { o1[j] = x1[j]; o2[j] = x2[j]; }
  }
  T* dst;
  if (h < Hq) dst = q_out + t * ldq + (int64_t)h * D;
  else if (h < Hq + Hkv) dst = k_cache + slot * cache_stride_k + (int64_t)(h - Hq) * D;
  else dst = v_cache + slot * cache_stride_v + (int64_t)(h - Hq - Hkv) * D;
  *(uint4*)(dst + c * 8) = pack8<T>(o1);
  *(uint4*)(dst + half + c * 8) = pack8<T>(o2);
}

// the checks the three GEMM + consumer forms share; *S = the split plan.  Returns MI_OK, or the error to hand back.
int fused_prologue(const char* name, const void* a, const void* b_nk, const float* scale_a, const float* scale_b,
                   int64_t M, int64_t N, int64_t K, int dtype, const void* workspace, int64_t workspace_bytes, int* S) {
  if (!(M > 0 && N > 0 && K > 0 && a && b_nk && scale_a && scale_b && (dtype == MI_BF16 || dtype == MI_FP16)))
    MI_FAIL(MI_ERR_INVALID, "%s: invalid argument (sizes, null operand or dtype)", name);
  if (M > kMaxRows || K % 64 != 0 || N % 8 != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "%s: decode shapes only (M <= 256, K %% 64 == 0, N %% 8 == 0; M %lld N %lld K %lld)", name,
            (long long)M, (long long)N, (long long)K);
  const int64_t need = mi_int8_gemm_fused_workspace_bytes(M, N, K);
  if (need <= 0) MI_FAIL(MI_ERR_UNSUPPORTED, "%s: no int8 decode GEMM for M %lld N %lld K %lld", name, (long long)M, (long long)N, (long long)K);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))
    MI_FAIL(MI_ERR_INVALID, "%s: workspace of mi_int8_gemm_fused_workspace_bytes() = %lld bytes needed", name, (long long)need);
  int per;
  mi_int8_gemm_plan_splits(N, K, S, &per);
  return MI_OK;
}

}  // namespace

// ================================================================================================ producers
extern "C" int mi_rmsnorm_int8(const void* x, void* residual, const void* weight, void* out, void* q_out, float* q_scales,
                               int64_t M, int64_t H, int64_t ldx, int64_t ldr, int64_t ldo, float eps, int dtype,
                               void* stream) {
  MI_CHECK_ARG(M >= 0 && M <= 0x7fffffff && H > 0);
  if (M == 0) return MI_OK;
  MI_CHECK_ARG(x && weight && q_out && q_scales);
  MI_CHECK_ARG(dtype == MI_BF16 || dtype == MI_FP16);
  MI_CHECK_ARG(ldx >= H && (!residual || ldr >= H) && (!out || ldo >= H));
  if (H % 8 != 0 || H > kMaxH || ldx % 8 || (out && ldo % 8) || (residual && ldr % 8))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_rmsnorm_int8: H and the row strides must be multiples of 8, H <= 16384 (H=%lld)", (long long)H);
  MI_CHECK_ARG((((uintptr_t)x | (uintptr_t)residual | (uintptr_t)weight | (uintptr_t)out) & 15) == 0 && ((uintptr_t)q_out & 7) == 0);
  run_norm<false>(x, ldx, SlabSrc{nullptr, nullptr, nullptr, 0}, residual, weight, out, q_out, q_scales, M, H, ldr, ldo, eps,
                  dtype, stream);
  MI_CHECK_LAUNCH();
  return MI_OK;
}

extern "C" int mi_silu_and_mul_int8(const void* x, void* out, void* q_out, float* q_scales, int64_t M, int64_t I,
                                    int64_t ldx, int64_t ldo, int dtype, void* stream) {
  MI_CHECK_ARG(M >= 0 && M <= 0x7fffffff && I > 0);
  if (M == 0) return MI_OK;
  MI_CHECK_ARG(x && q_out && q_scales);
  MI_CHECK_ARG(dtype == MI_BF16 || dtype == MI_FP16);
  MI_CHECK_ARG(ldx >= 2 * I && (!out || ldo >= I));
  if (I % 8 != 0 || I > kMaxI || ldx % 8 || (out && ldo % 8))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_silu_and_mul_int8: I and the row strides must be multiples of 8, I <= 65536 (I=%lld)", (long long)I);
  MI_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0 && ((uintptr_t)q_out & 7) == 0);
  run_silu<false>(x, ldx, SlabSrc{nullptr, nullptr, nullptr, 0}, out, q_out, q_scales, M, I, ldo, dtype, stream);
  MI_CHECK_LAUNCH();
  return MI_OK;
}

// ================================================================================================ GEMM + consumer
// One answer for the three forms: the int32 slabs of the plan, S * M * N * 4 bytes (the 16-bit intermediate the gate_up
// form takes when S == 1 is half of that).  0: no fused form for this shape.
extern "C" int64_t mi_int8_gemm_fused_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || M > kMaxRows || N <= 0 || K <= 0 || mi_int8_gemm_workspace_bytes(M, N, K) < 0) return 0;
  int S, per;
  mi_int8_gemm_plan_splits(N, K, &S, &per);
  return (int64_t)S * M * N * (int64_t)sizeof(int32_t);
}

extern "C" int mi_int8_gemm_add_rmsnorm_int8(const void* a, const void* b_nk, const float* scale_a, const float* scale_b,
                                             void* residual, const void* norm_weight, void* out, void* q_out,
                                             float* q_scales, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                             float eps, int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M == 0) return MI_OK;
  int S;
  if (const int rc = fused_prologue("mi_int8_gemm_add_rmsnorm_int8", a, b_nk, scale_a, scale_b, M, N, K, dtype, workspace,
                                    workspace_bytes, &S))
    return rc;
  MI_CHECK_ARG(norm_weight && (out || q_out) && (!q_out || q_scales));
  MI_CHECK_ARG((((uintptr_t)residual | (uintptr_t)norm_weight | (uintptr_t)out | (uintptr_t)scale_b) & 15) == 0 && ((uintptr_t)q_out & 7) == 0);
  if (N > kMaxH) MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm_add_rmsnorm_int8: N <= 16384 (N=%lld)", (long long)N);
  if (const int rc = mi_int8_gemm_partial(a, b_nk, (int32_t*)workspace, M, N, K, lda, ldb, stream)) return rc;
  run_norm<true>(nullptr, 0, SlabSrc{(const int32_t*)workspace, scale_a, scale_b, S}, residual, norm_weight, out, q_out,
                 q_scales, M, N, N, N, eps, dtype, stream);
  MI_CHECK_LAUNCH();
  return MI_OK;
}

extern "C" int mi_int8_gemm_rope_kvwrite(const void* a, const void* b_nk, const float* scale_a, const float* scale_b,
                                         const int64_t* positions, const float* cos_sin_cache, void* q_out, void* k_cache,
                                         void* v_cache, const int64_t* loc, int64_t M, int64_t num_q_heads,
                                         int64_t num_kv_heads, int64_t head_dim, int64_t K, int64_t lda, int64_t ldb,
                                         int64_t ldq, int64_t cache_stride_k, int64_t cache_stride_v, int dtype,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  if (M == 0) return MI_OK;
  MI_CHECK_ARG(num_q_heads > 0 && num_kv_heads > 0 && head_dim > 0 && num_q_heads + 2 * num_kv_heads <= 0x7fffffff / head_dim);
  const int64_t N = (num_q_heads + 2 * num_kv_heads) * head_dim;
  int S;
  if (const int rc = fused_prologue("mi_int8_gemm_rope_kvwrite", a, b_nk, scale_a, scale_b, M, N, K, dtype, workspace,
                                    workspace_bytes, &S))
    return rc;
  MI_CHECK_ARG(positions && cos_sin_cache && q_out && k_cache && v_cache && loc);
  MI_CHECK_ARG((((uintptr_t)cos_sin_cache | (uintptr_t)scale_b | (uintptr_t)q_out | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0);
  if (head_dim % 16 != 0 || ldq % 8 || cache_stride_k % 8 || cache_stride_v % 8)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm_rope_kvwrite: head_dim %% 16 and 16-byte aligned rows required");
  MI_CHECK_ARG(ldq >= num_q_heads * head_dim && cache_stride_k >= num_kv_heads * head_dim && cache_stride_v >= num_kv_heads * head_dim);
  if (const int rc = mi_int8_gemm_partial(a, b_nk, (int32_t*)workspace, M, N, K, lda, ldb, stream)) return rc;
  const int64_t total = M * (num_q_heads + 2 * num_kv_heads) * (head_dim / 16);
  const SlabSrc g{(const int32_t*)workspace, scale_a, scale_b, S};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MI_BF16)
    slab_rope_kvwrite_int8_kernel<bf16_t><<<(unsigned)cdiv64(total, 256), 256, 0, st>>>(g, positions, cos_sin_cache, (bf16_t*)q_out, (bf16_t*)k_cache, (bf16_t*)v_cache, loc, M, (int)num_q_heads, (int)num_kv_heads, (int)head_dim, ldq, cache_stride_k, cache_stride_v);
  else
    slab_rope_kvwrite_int8_kernel<f16_t><<<(unsigned)cdiv64(total, 256), 256, 0, st>>>(g, positions, cos_sin_cache, (f16_t*)q_out, (f16_t*)k_cache, (f16_t*)v_cache, loc, M, (int)num_q_heads, (int)num_kv_heads, (int)head_dim, ldq, cache_stride_k, cache_stride_v);
  MI_CHECK_LAUNCH();
  return MI_OK;
}

// The S == 1 rule.  Slab route: the GEMM writes and the consumer reads S * M * 2I * 4 bytes.  When the plan does not
// split (2I fills the chip by itself: >= 200 column blocks, e.g. 2I = 28672) the GEMM's own epilogue can round to T
// for free, and a T-typed [M, 2I] intermediate is half the bytes of one int32 slab: then the ordinary kernel writes it
// into `workspace` and the T-reading row kernel of mi_silu_and_mul_int8 follows.  With S > 1 the T route would need
// the slabs AND the reduce launch in front, so the slab route moves fewer bytes.  Two launches and the same bits either way.
extern "C" int mi_int8_gemm_silu_mul_int8(const void* a, const void* b_nk, const float* scale_a, const float* scale_b,
                                          void* q_out, float* q_scales, int64_t M, int64_t I, int64_t K, int64_t lda,
                                          int64_t ldb, int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M == 0) return MI_OK;
  MI_CHECK_ARG(I > 0 && I <= 0x3fffffff);
  const int64_t N = 2 * I;
  int S;
  if (const int rc = fused_prologue("mi_int8_gemm_silu_mul_int8", a, b_nk, scale_a, scale_b, M, N, K, dtype, workspace,
                                    workspace_bytes, &S))
    return rc;
  MI_CHECK_ARG(q_out && q_scales && ((uintptr_t)q_out & 7) == 0 && ((uintptr_t)scale_b & 15) == 0);
  if (I % 64 != 0 || I > kMaxI)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm_silu_mul_int8: I must be a multiple of 64 (the next GEMM's K), <= 65536 (I=%lld)", (long long)I);
  if (S == 1) {
    if (const int rc = mi_int8_gemm(a, b_nk, scale_a, scale_b, nullptr, workspace, M, N, K, lda, ldb, N, dtype, nullptr, 0, stream))
      return rc;
    run_silu<false>(workspace, N, SlabSrc{nullptr, nullptr, nullptr, 0}, nullptr, q_out, q_scales, M, I, 0, dtype, stream);
  } else {
    if (const int rc = mi_int8_gemm_partial(a, b_nk, (int32_t*)workspace, M, N, K, lda, ldb, stream)) return rc;
    run_silu<true>(nullptr, 0, SlabSrc{(const int32_t*)workspace, scale_a, scale_b, S}, nullptr, q_out, q_scales, M, I, 0,
                   dtype, stream);
  }
  MI_CHECK_LAUNCH();
  return MI_OK;
}
