// Per-token int8 activation quantisation for the W8A8 int8 linears.  Bit-exact with the reference arithmetic
// (per_token_quant_int8): absmax = max(max_k |x|, 1e-10), scale = absmax / 127 (IEEE divide),
// q = round(x * (127 / absmax)) in fp32, ties away from zero; q lies in [-127, 127] and an all-zero row gives q = 0.
// The multiplier is what torch makes of the reference's `127 / absmax` (a number over a tensor): reciprocal(absmax) * 127,
// two fp32 roundings -- a single IEEE 127 / absmax differs in the last bit for a quarter of all rows.
// HBM-bound: 16-byte loads, 8-byte stores, the row stays in registers between the two passes.
#include "common.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

template <typename T> __device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = Elem<T>::lo(w[j]);
    f[2 * j + 1] = Elem<T>::hi(w[j]);
  }
}

__device__ __forceinline__ float absmax8(const float (&f)[8], float mx) {
#pragma unroll
  for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(f[j]));
  return mx;
}

// 8 floats -> 8 int8 bytes: roundf is round-half-away, |f * mult| <= 127 (1 + 2^-22) so no clamp is needed
__device__ __forceinline__ uint2 quant8(const float (&f)[8], float mult) {
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j >> 2] |= ((uint32_t)(int)roundf(f[j] * mult) & 0xffu) << (8 * (j & 3));
  return make_uint2(w[0], w[1]);
}

// One 256-thread workgroup per row; the first 256*8*RV elements of the row stay in registers between the two passes,
// a longer row is re-read (L2-hot).
template <typename T, int RV>
__global__ __launch_bounds__(256) void int8_quant_token_kernel(const T* __restrict__ x, int8_t* __restrict__ q,
                                                               float* __restrict__ scales, int64_t K, int64_t ldx) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const T* xr = x + row * ldx;
  int8_t* qr = q + row * K;
  const int64_t nvec = K / 8;
  uint4 keep[RV];
  float mx = 0.f;
#pragma unroll
  for (int v = 0; v < RV; ++v) {
    const int64_t i = threadIdx.x + v * 256;
    keep[v] = make_uint4(0, 0, 0, 0);
    if (i < nvec) keep[v] = *(const uint4*)(xr + i * 8);
    float f[8];
    unpack8<T>(keep[v], f);
    mx = absmax8(f, mx);
  }
  for (int64_t i = threadIdx.x + RV * 256; i < nvec; i += 256) {
    float f[8];
    unpack8<T>(*(const uint4*)(xr + i * 8), f);
    mx = absmax8(f, mx);
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])), 1e-10f);
  if (threadIdx.x == 0) scales[row] = mx / 127.0f;
  const float mult = (1.0f / mx) * 127.0f;
#pragma unroll
  for (int v = 0; v < RV; ++v) {
    const int64_t i = threadIdx.x + v * 256;
    if (i < nvec) {
      float f[8];
      unpack8<T>(keep[v], f);
      *(uint2*)(qr + i * 8) = quant8(f, mult);
    }
  }
  for (int64_t i = threadIdx.x + RV * 256; i < nvec; i += 256) {
    float f[8];
    unpack8<T>(*(const uint4*)(xr + i * 8), f);
    *(uint2*)(qr + i * 8) = quant8(f, mult);
  }
}

}  // namespace

extern "C" int mi_int8_quant_per_token(const void* x, void* q, float* scales, int64_t M, int64_t K, int64_t ldx,
                                       int dtype, void* stream) {
  MI_CHECK_ARG(M >= 0 && M <= 0x7fffffff && K > 0);
  if (M == 0) return MI_OK;
  MI_CHECK_ARG(x && q && scales);
  MI_CHECK_ARG(dtype == MI_BF16 || dtype == MI_FP16);
  MI_CHECK_ARG(ldx >= K);
  if (K % 8 != 0 || ldx % 8 != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_quant_per_token: K and ldx must be multiples of 8");
  MI_CHECK_ARG((((uintptr_t)x & 15) | ((uintptr_t)q & 7)) == 0);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MI_BF16)
    int8_quant_token_kernel<bf16_t, 2><<<(unsigned)M, 256, 0, st>>>((const bf16_t*)x, (int8_t*)q, scales, K, ldx);
  else
    int8_quant_token_kernel<f16_t, 2><<<(unsigned)M, 256, 0, st>>>((const f16_t*)x, (int8_t*)q, scales, K, ldx);
  MI_CHECK_LAUNCH();
  return MI_OK;
}
