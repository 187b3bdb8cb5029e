// Decode-shaped 16-bit linear: out[M,N] = x[M,K] . W[N,K]^T (+ bias), x and W both bf16 or both fp16, fp32
// accumulation, output in the activation dtype or fp32 (logits).  The unquantised sibling of fp8_gemm_xw_kernel.
//
// One pass covers up to 256 rows and reads every weight byte exactly once.
//   work split   a 512-thread workgroup owns 128 output columns (= 128 weight rows) x all rows of the pass; the grid is
//                column blocks x S split-K slices of `per` k-phases.  A k-phase is 128 bytes of K (64 elements).
//   wave roles   waves 4-7 (loaders) only issue 1-KiB LDS-DMA pieces -- 4 weight pieces and their share of the
//                activation block per phase -- wait for them with a counted vmcnt and meet the barrier.  Waves 0-3
//                (consumers, one per SIMD) own 32 weight rows x all rows: ds_read_b128 + MFMA and nothing else.
//   LDS ring     a stage is [16 MT rows of x][128 weight rows], 128 bytes each; 3 stages at MT = 16 (144 KiB), else 4.
//                Two consecutive rows share a 256-byte line and the 16-byte slot inside the line is XORed with
//                (line & 15).  The DMA destination is lane-linear, so the swizzle is applied to the SOURCE address of
//                each lane; the fragment reads (16 rows x 4 slots per instruction) then touch every bank group once.
//   MFMA         v_mfma_f32_16x16x32_{bf16,f16}: 8 elements (one 16-byte read) per lane and operand, two per phase
//                and tile pair.  Weights are the A operand and activations B: a lane ends with 4 consecutive output
//                columns of one row, and every x fragment feeds both weight tiles of its consumer.
//   k rotation   workgroup b walks the phases of its slice cyclically from (7 b) % count, so the chip does not ask for
//                the same 128-byte column of every activation row at once.  The order is fixed per workgroup.
//   epilogue     the consumers park the fp32 tile in the (drained) ring, rows padded to 528 bytes, and all 8 waves
//                write whole rows: to `out` (acc + bias, ONE rounding) when S == 1, else raw fp32 into slab[s][m][n];
//                bf16_gemm_reduce_kernel then sums the slabs in split order, adds the bias and rounds once.
// No atomics, no memset, no allocation, no synchronisation: capturable.
#include "common.h"

namespace {

constexpr int kPhaseBytes = 128;          // bytes of K per k-phase
constexpr int kPhaseElems = 64;
constexpr int kBlockCols = 128;           // output columns per workgroup
constexpr int kPassRows = 256;            // rows one pass covers
constexpr int kMaxRows = 512;             // rows one call covers (two passes)
constexpr int kTilePitch = kBlockCols * 4 + 16;   // epilogue tile row: 128 fp32 + 16 bytes (conflict-free b128 writes)
constexpr int kRotStep = 7;

struct HalfGemm {
  const uint8_t* x;
  const uint8_t* w;
  const void* bias;   // T[N] or null
  void* out;          // OutT, row stride ldo
  float* slab;        // [S][M][N] when S > 1
  int64_t M, N, K, lda, ldb, ldo;   // strides in elements
  int S, per;         // split-K slices, k-phases per slice
};

template <int MT> constexpr int ring_depth() { return MT == 16 ? 3 : 4; }
template <int MT> constexpr size_t ring_bytes() {
  return (size_t)ring_depth<MT>() * ((size_t)MT * 16 + kBlockCols) * kPhaseBytes;
}

// 4 consecutive columns n0.. of one output row; `vec`: the row takes one aligned vector store and all 4 exist
template <typename OutT>
__device__ __forceinline__ void store4(OutT* o, const float (&v)[4], int64_t n0, int64_t N, bool vec) {
  if (vec) {
    if constexpr (__is_same(OutT, float)) *(f32x4*)o = f32x4{v[0], v[1], v[2], v[3]};
    else *(uint2*)o = make_uint2(pack2<OutT>(v[0], v[1]), pack2<OutT>(v[2], v[3]));
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n0 + r < N) o[r] = (OutT)v[r];
  }
}

template <typename T, typename OutT, int MT>
__global__ __launch_bounds__(512) void bf16_gemm_kernel(const HalfGemm p) {
  typedef typename Elem<T>::vec8 vec8;
  constexpr int R = ring_depth<MT>(), AHEAD = R - 1;    // stages; phases issued ahead of the one being consumed
  constexpr int ROWS = MT * 16;
  constexpr int XBYTES = ROWS * kPhaseBytes, WBYTES = kBlockCols * kPhaseBytes, STAGE = XBYTES + WBYTES;
  constexpr int XPIECES = ROWS / 8, WPIECES = kBlockCols / 8;      // 1-KiB DMA pieces (8 rows) per phase
  constexpr int XL = XPIECES >= 4 ? XPIECES / 4 : 1;              // per loader (MT = 1: two loaders repeat a piece)
  constexpr int WL = WPIECES / 4;
  constexpr int E = XL + WL;                                      // vmcnt entries per loader and phase
  static_assert(AHEAD == 2 || AHEAD == 3, "the counted wait below enumerates 1..2 younger phases");
  static_assert((AHEAD - 1) * E < 64, "vmcnt is a 6-bit counter");
  static_assert((size_t)ROWS * kTilePitch <= ring_bytes<MT>(), "the epilogue tile reuses the ring");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, q = lane >> 4;
  const int sp = blockIdx.y;
  const int64_t n_blk = (int64_t)blockIdx.x * kBlockCols;
  const int64_t ph0 = (int64_t)sp * p.per;
  const int nph = (int)min((int64_t)p.per, p.K / kPhaseElems - ph0);   // >= 1 by the plan

  if (wave >= 4) {
    // ---------------------------------------------------------------- loaders
    const int ld = wave - 4;
    const uint32_t lds0 = lds_addr_of(smem);
    // lane -> (row, 16-byte slot) of the piece it fills: LDS byte piece*1024 + lane*16 is line piece*4 + lane/16,
    // physical position lane%16, which holds logical position lane%16 ^ (line & 15) = (row & 1) * 8 + slot
    uint32_t xoff[XL], woff[WL], xdst[XL], wdst[WL];
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int piece = (ld * XL + i) % XPIECES;
      const int line = piece * 4 + (lane >> 4);
      const int logical = (lane & 15) ^ (line & 15);
      const int64_t m = min((int64_t)(line * 2 + (logical >> 3)), p.M - 1);     // rows past M: re-read the last
      xoff[i] = (uint32_t)(m * p.lda * 2 + (logical & 7) * 16);
      xdst[i] = __builtin_amdgcn_readfirstlane(lds0 + piece * 1024);
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int piece = ld * WL + i;
      const int line = piece * 4 + (lane >> 4);
      const int logical = (lane & 15) ^ (line & 15);
      const int64_t n = min(n_blk + line * 2 + (logical >> 3), p.N - 1);        // ragged last block: clamp
      woff[i] = (uint32_t)(n * p.ldb * 2 + (logical & 7) * 16);
      wdst[i] = __builtin_amdgcn_readfirstlane(lds0 + XBYTES + piece * 1024);
    }
    const int rot = (int)(((int64_t)blockIdx.x * kRotStep) % nph);
    auto issue = [&](int i) __attribute__((always_inline)) {
      const uint32_t st = (uint32_t)(i % R) * STAGE;
      int k = i + rot;
      k = k >= nph ? k - nph : k;
      const int64_t kbyte = (ph0 + k) * kPhaseBytes;                // wave-uniform: scalar base
      const uint8_t* xa = p.x + kbyte;
      const uint8_t* wa = p.w + kbyte;
#pragma unroll
      for (int j = 0; j < XL; ++j) glds16_s(xoff[j], xa, xdst[j] + st);
#pragma unroll
      for (int j = 0; j < WL; ++j) glds16_s(woff[j], wa, wdst[j] + st);
    };
#pragma unroll
    for (int d = 0; d < AHEAD; ++d)
      if (d < nph) issue(d);
    for (int i = 0; i < nph; ++i) {
      const int younger = min(AHEAD - 1, nph - 1 - i);              // phases issued after i may stay in flight
      if (AHEAD >= 3 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * E) : "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(E) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                                 // phase i published; consumers are done with i-1
      if (i + AHEAD < nph) issue(i + AHEAD);                        // into the stage phase i-1 used
    }
    __builtin_amdgcn_s_barrier();                                   // (every stage consumed)
  } else {
    // ---------------------------------------------------------------- consumers
    f32x4 acc[2][MT];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[tn][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto frag = [&](const char* base, int row, int slot) __attribute__((always_inline)) -> vec8 {
      const uint4 v = *(const uint4*)(base + (row >> 1) * 256 + (((((row & 1) << 3) | slot) ^ ((row >> 1) & 15)) * 16));
      return __builtin_bit_cast(vec8, v);
    };
    int stage = 0;
    for (int i = 0; i < nph; ++i) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                                 // phase i landed (the loaders waited for it)
      const char* xb = smem + stage * STAGE;
      const char* wb = xb + XBYTES;
      stage = stage + 1 == R ? 0 : stage + 1;
      vec8 wf[2][2], xf[MT][2];
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int s = 0; s < 2; ++s) wf[tn][s] = frag(wb, wave * 32 + tn * 16 + r16, s * 4 + q);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) xf[t][s] = frag(xb, t * 16 + r16, s * 4 + q);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) acc[tn][t] = Elem<T>::mfma16(wf[tn][s], xf[t][s], acc[tn][t]);
      // one wave per SIMD, so nothing else hides the LDS latency: the x fragments run PF row tiles ahead of their MFMAs
      constexpr int PF = MT < 2 ? MT : 2;
      __builtin_amdgcn_sched_group_barrier(0x100, 4 + 2 * PF, 0);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t + PF < MT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                   // every stage consumed: LDS is free
    // lane holds columns 32*wave + 16*tn + 4*q .. +3 of rows 16*t + r16
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        *(f32x4*)(smem + (t * 16 + r16) * kTilePitch + (wave * 32 + tn * 16 + 4 * q) * 4) = acc[tn][t];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // ------------------------------------------------------------------ whole-row stores: 32 lanes x 4 columns per row,
  // two rows per wave instruction, 16 rows per sweep of the 8 waves
  const int c = (lane & 31) * 4;
  const int64_t n0 = n_blk + c;
  if (n0 >= p.N) return;
  const bool to_slab = p.S > 1;
  const bool full4 = n0 + 3 < p.N;
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (!to_slab && p.bias) {
#pragma unroll
    for (int r = 0; r < 4; ++r) bv[r] = (float)((const T*)p.bias)[min(n0 + r, p.N - 1)];
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = i * 16 + wave * 2 + (lane >> 5);
    if (row >= p.M) continue;
    const f32x4 a = *(const f32x4*)(smem + row * kTilePitch + c * 4);
    if (to_slab) {
      const float v[4] = {a[0], a[1], a[2], a[3]};
      store4<float>(p.slab + ((int64_t)sp * p.M + row) * p.N + n0, v, n0, p.N, full4 && (p.N & 3) == 0);
    } else {
      const float v[4] = {a[0] + bv[0], a[1] + bv[1], a[2] + bv[2], a[3] + bv[3]};
      store4<OutT>((OutT*)p.out + (int64_t)row * p.ldo + n0, v, n0, p.N, full4 && (p.ldo & 3) == 0);
    }
  }
}

// out = round_once(slab[0] + slab[1] + ... (in this order) + bias): one thread per 4 consecutive columns
template <typename T, typename OutT>
__global__ __launch_bounds__(256) void bf16_gemm_reduce_kernel(const HalfGemm p) {
  const int64_t nq = (p.N + 3) / 4;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= p.M * nq) return;
  const int64_t m = gid / nq, n0 = (gid % nq) * 4;
  const bool full4 = n0 + 3 < p.N;
  const bool vec = full4 && (p.N & 3) == 0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.S; ++s) {
    const float* src = p.slab + ((int64_t)s * p.M + m) * p.N + n0;
    if (vec) {
      const f32x4 a = *(const f32x4*)src;
      v[0] += a[0]; v[1] += a[1]; v[2] += a[2]; v[3] += a[3];
    } else {
      for (int r = 0; r < 4; ++r)
        if (n0 + r < p.N) v[r] += src[r];
    }
  }
  if (p.bias) {
    for (int r = 0; r < 4; ++r) v[r] += (float)((const T*)p.bias)[min(n0 + r, p.N - 1)];
  }
  store4<OutT>((OutT*)p.out + m * p.ldo + n0, v, n0, p.N, full4 && (p.ldo & 3) == 0);
}

// Split-K plan: S slices of `per` phases.  With at least 200 column blocks the grid fills the 256 CUs by itself;
// below that K is split until about one round of workgroups exists, but never into slices of less than 4 phases
// (the ring prologue and the slab traffic of a slice are paid per slice).  Independent of M: the second chunk of a
// 257..512-row call uses the slabs of the first.
void plan_splits(int64_t N, int64_t K, int* S, int* per) {
  const int64_t nph = K / kPhaseElems, nblk = cdiv64(N, kBlockCols);
  int64_t want = nblk >= 200 ? 1 : 256 / nblk;
  if (want > nph / 4) want = nph / 4;
  if (want < 1) want = 1;
  *per = (int)cdiv64(nph, want);
  *S = (int)cdiv64(nph, *per);
}

// the shape-only part of the preconditions (what mi_bf16_gemm_workspace_bytes can see)
const char* shape_refusal(int64_t M, int64_t N, int64_t K) {
  if (K % kPhaseElems != 0) return "K must be a multiple of 64";
  if (M > kMaxRows) return "more than 512 rows (prefill-shaped 16-bit GEMMs are not this kernel)";
  if (N > (int64_t)kBlockCols * 0x7fffffff) return "N too large for the grid";
  return nullptr;
}

template <typename T, typename OutT, int MT>
void launch_pass(const HalfGemm& p, hipStream_t st) {
  const dim3 grid((unsigned)cdiv64(p.N, kBlockCols), (unsigned)p.S);
  bf16_gemm_kernel<T, OutT, MT><<<grid, 512, ring_bytes<MT>(), st>>>(p);
  if (p.S > 1) {
    const int64_t total = p.M * cdiv64(p.N, 4);
    bf16_gemm_reduce_kernel<T, OutT><<<(unsigned)cdiv64(total, 256), 256, 0, st>>>(p);
  }
}

template <typename T, typename OutT>
void launch_rows(const HalfGemm& p, hipStream_t st) {
  for (int64_t m0 = 0; m0 < p.M; m0 += kPassRows) {   // chunks share the slabs: stream order keeps them apart
    HalfGemm c = p;
    c.M = min(p.M - m0, (int64_t)kPassRows);
    c.x = p.x + m0 * p.lda * 2;
    c.out = (char*)p.out + m0 * p.ldo * (int64_t)sizeof(OutT);
    if (c.M <= 16) launch_pass<T, OutT, 1>(c, st);
    else if (c.M <= 32) launch_pass<T, OutT, 2>(c, st);
    else if (c.M <= 64) launch_pass<T, OutT, 4>(c, st);
    else if (c.M <= 128) launch_pass<T, OutT, 8>(c, st);
    else launch_pass<T, OutT, 16>(c, st);
  }
}

}  // namespace

// the slab reduction on its own, for the prefill tile kernel (bf16_gemm_tile.hip), whose slabs have the same form
MI_INTERNAL void mi_bf16_gemm_reduce(float* slab, const void* bias, void* out, int64_t M, int64_t N, int64_t ldo, int S,
                                     int dtype, int out_dtype, hipStream_t st) {
  HalfGemm p = {};
  p.bias = bias; p.out = out; p.slab = slab; p.M = M; p.N = N; p.ldo = ldo; p.S = S;
  const unsigned blocks = (unsigned)cdiv64(M * cdiv64(N, 4), 256);
  if (dtype == MI_BF16) {
    if (out_dtype == MI_F32) bf16_gemm_reduce_kernel<bf16_t, float><<<blocks, 256, 0, st>>>(p);
    else bf16_gemm_reduce_kernel<bf16_t, bf16_t><<<blocks, 256, 0, st>>>(p);
  } else {
    if (out_dtype == MI_F32) bf16_gemm_reduce_kernel<f16_t, float><<<blocks, 256, 0, st>>>(p);
    else bf16_gemm_reduce_kernel<f16_t, f16_t><<<blocks, 256, 0, st>>>(p);
  }
}

extern "C" int64_t mi_bf16_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M < 0 || N < 0 || K <= 0 || shape_refusal(M, N, K)) return -1;
  if (M == 0 || N == 0) return 0;
  int S, per;
  plan_splits(N, K, &S, &per);
  return S > 1 ? (int64_t)S * min(M, (int64_t)kPassRows) * N * (int64_t)sizeof(float) : 0;
}

extern "C" int mi_bf16_gemm_check(const void* x, const void* w_nk, const void* out, int64_t M, int64_t N, int64_t K,
                                  int64_t lda, int64_t ldb, int64_t ldo, int dtype, int out_dtype) {
  MI_CHECK_ARG(M >= 0 && N >= 0 && K > 0);
  MI_CHECK_ARG(dtype == MI_BF16 || dtype == MI_FP16);
  MI_CHECK_ARG(out_dtype == dtype || out_dtype == MI_F32);
  if (M == 0 || N == 0) return MI_OK;
  MI_CHECK_ARG(x && w_nk && out);
  MI_CHECK_ARG(lda >= K && ldb >= K && ldo >= N);
  if (const char* why = shape_refusal(M, N, K))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm: %s (M %lld N %lld K %lld)", why, (long long)M, (long long)N, (long long)K);
  if (lda % 8 != 0 || ldb % 8 != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm: lda and ldb must be multiples of 8 (got %lld %lld)", (long long)lda,
            (long long)ldb);
  if ((((uintptr_t)x | (uintptr_t)w_nk | (uintptr_t)out) & 15) != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm: x, w_nk and out must be 16-byte aligned");
  // the DMA addresses are a scalar base + a 32-bit lane offset (row * pitch + at most 128 bytes of the phase)
  const uint64_t lim = 1ull << 32;
  if ((uint64_t)(N - 1) * (uint64_t)ldb * 2 + 256 >= lim || (uint64_t)(M - 1) * (uint64_t)lda * 2 + 256 >= lim)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm: operand spans 4 GiB or more (32-bit lane offsets)");
  return MI_OK;
}

extern "C" int mi_bf16_gemm(const void* x, const void* w_nk, const void* bias, void* out, int64_t M, int64_t N, int64_t K,
                            int64_t lda, int64_t ldb, int64_t ldo, int dtype, int out_dtype, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  const int rc = mi_bf16_gemm_check(x, w_nk, out, M, N, K, lda, ldb, ldo, dtype, out_dtype);
  if (rc != MI_OK || M == 0 || N == 0) return rc;
  MI_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= 0);
  HalfGemm p;
  p.x = (const uint8_t*)x; p.w = (const uint8_t*)w_nk; p.bias = bias; p.out = out; p.slab = (float*)workspace;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldo = ldo;
  plan_splits(N, K, &p.S, &p.per);
  const int64_t need = p.S > 1 ? (int64_t)p.S * min(M, (int64_t)kPassRows) * N * (int64_t)sizeof(float) : 0;
  if (need > workspace_bytes || (need > 0 && workspace == nullptr)) {   // no room for slabs: no split-K
    p.S = 1;
    p.per = (int)(K / kPhaseElems);
  }
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MI_BF16) {
    if (out_dtype == MI_F32) launch_rows<bf16_t, float>(p, st);
    else launch_rows<bf16_t, bf16_t>(p, st);
  } else {
    if (out_dtype == MI_F32) launch_rows<f16_t, float>(p, st);
    else launch_rows<f16_t, f16_t>(p, st);
  }
  MI_CHECK_LAUNCH();
  return MI_OK;
}
