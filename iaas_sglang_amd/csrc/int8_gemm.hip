// W8A8 int8 linear: out[M,N] = round_once(((float)acc * scale_a[m]) * scale_b[n] + (float)bias[n]),
// acc = sum_k a[m][k] * b[n][k] exact in int32; a int8 [M,K] (per-token scales), b_nk int8 [N,K] (per-channel scales),
// out bf16 or fp16.  Two kernels behind mi_int8_gemm: a decode-shaped one for M <= 256 and a tile kernel above.
// Int32 sums commute, so split-K, the k rotation and the phase order change no bit of the result.
//
// int8_gemm_kernel (M <= 256, weight-bandwidth-bound; the int8 sibling of bf16_gemm_kernel / fp8_gemm_xw_kernel)
//   work split   a 512-thread workgroup owns 128 output columns (= 128 weight rows) x all MT * 16 rows; the grid is
//                column blocks x S split-K slices of `per` k-phases.  A k-phase is 128 bytes = 128 elements of K.
//   wave roles   waves 4-7 (loaders) only issue 1-KiB LDS-DMA pieces -- 4 weight pieces and their share of the
//                activation block per phase -- wait for them with a counted vmcnt and meet the barrier.  Waves 0-3
//                (consumers, one per SIMD) own 32 weight rows x all rows: ds_read_b128 + MFMA and nothing else.  This
//                is the split fp8_gemm.hip measured for the same bytes per phase; it is kept.
//   LDS ring     a stage is [16 MT rows of a][128 weight rows], 128 bytes each: (16 MT + 128) * 128 bytes.  4 stages
//                up to MT = 8 (72 / 80 / 96 / 128 KiB for MT = 1 / 2 / 4 / 8), 3 stages at MT = 16 (144 KiB of the
//                CU's 160 KiB).  Two consecutive rows share a 256-byte line and the 16-byte slot inside the line is
//                XORed with (line & 15).  The DMA destination is lane-linear, so the swizzle is applied to the SOURCE
//                address of each lane; a fragment read (16 rows x 4 slots per instruction) touches every bank group
//                once: conflict-free ds_read_b128.
//   MFMA         v_mfma_i32_16x16x64_i8: a lane supplies 16 consecutive k-bytes of row lane % 16 (one 16-byte read),
//                lane group lane / 16 takes bytes 16 (lane / 16) .. +15 of the 64; both operands use the same slot, so
//                every k meets its partner whatever order the hardware sums them in.  Two MFMAs per (m-tile, n-tile,
//                phase).  Weights are the A operand: a lane ends with 4 consecutive output columns of one row.
//   K % 64       K need only be a multiple of one MFMA depth.  An odd number of 64-byte halves leaves a half phase at
//                the end of the last slice: its loaders read the first half twice (the second would lie past the row)
//                and its consumers issue one MFMA per tile instead of two.  It is walked last, outside the rotation.
//   k rotation   workgroup b walks the full phases of its slice cyclically from (7 b) % count, so the chip does not
//                ask for the same 128-byte column of every activation row at once.
//   epilogue     the consumers park the int32 tile in the (drained) ring, rows padded to 528 bytes, and all 8 waves
//                write whole rows: the scaled, biased, once-rounded result to `out` when S == 1, else raw int32 into
//                slab[s][m][n]; int8_gemm_reduce_kernel sums the slabs (exactly) and applies the same epilogue.  The
//                partial launch of the fused forms (bottom of the file, int8_glue.hip) always takes the slab branch.
//
// int8_gemm_tile_kernel (M > 256): one 512-thread workgroup per 256 x 256 output tile, wave (wm, wn) of the 2 x 4 wave
//   grid owns 128 x 64.  k-steps of 128 bytes; both operands go global -> LDS by LDS-DMA into the same swizzled image,
//   double-buffered (2 stages x 64 KiB): step k + 1 is requested before step k is consumed, one vmcnt(0) + barrier per
//   step.  Rows and columns past the edge are clamped onto the last one when loading and masked when storing.  The
//   epilogue parks the int32 tile in LDS in two rounds of 128 rows (130 KiB, which sets the allocation) and writes
//   whole rows.  No split-K; correct and MFMA-based, not yet tuned to the FP8 tile kernel's level.
// No atomics, no memset, no allocation, no synchronisation: capturable.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
template <int V> struct IntC { static constexpr int value = V; };

constexpr int kPhaseBytes = 128;          // bytes (= elements) of K per k-phase
constexpr int kHalfBytes = 64;            // one MFMA depth
constexpr int kBlockCols = 128;           // output columns per decode workgroup
constexpr int kPassRows = 256;            // rows the decode kernel covers; above: the tile kernel
constexpr int kTilePitch = kBlockCols * 4 + 16;   // parked row: 128 int32 + 16 bytes (conflict-free b128 writes)
constexpr int kRotStep = 7;
constexpr int64_t kMaxK = 131072;         // K * 128 * 128 <= 2^31: the accumulator cannot wrap

constexpr int kBM = 256, kBN = 256;       // tile kernel: output tile
constexpr int kStage = kBM * kPhaseBytes; // 32 KiB per operand and stage
constexpr int kParkRows = 128;
constexpr int kParkPitch = kBN * 4 + 16;
constexpr int kTileLds = kParkRows * kParkPitch > 4 * kStage ? kParkRows * kParkPitch : 4 * kStage;

struct Int8Gemm {
  const uint8_t* a;
  const uint8_t* b;
  const float* sa;    // [M]
  const float* sb;    // [N]
  const void* bias;   // OutT[N] or null
  void* out;          // OutT, row stride ldo
  int32_t* slab;      // [S][M][N] when S > 1
  int64_t M, N, K, lda, ldb, ldo;
  int S, per;         // split-K slices, k-phases per slice
  int raw;            // the decode kernel leaves raw int32 in slab[sp] (S > 1, or the partial launch of the fused forms)
};

__device__ __forceinline__ i32x4 mfma_i8(const uint4& a, const uint4& b, i32x4 c) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0);
}

// the fragment of (row, 16-byte slot) in the swizzled LDS image of an operand block
__device__ __forceinline__ uint4 frag(const char* base, int row, int slot) {
  return *(const uint4*)(base + (row >> 1) * 256 + (((((row & 1) << 3) | slot) ^ ((row >> 1) & 15)) * 16));
}

// the contract's order of operations: (acc * scale_a) * scale_b, then + bias; the caller rounds once
__device__ __forceinline__ float dequant(int acc, float sa, float sb, float bias, bool has_bias) {
  const float v = ((float)acc * sa) * sb;
  return has_bias ? v + bias : v;
}

template <typename OutT>
__device__ __forceinline__ void store4(OutT* o, const float (&v)[4], int64_t n0, int64_t N, bool vec) {
  if (vec) {
    *(uint2*)o = make_uint2(pack2<OutT>(v[0], v[1]), pack2<OutT>(v[2], v[3]));
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n0 + r < N) o[r] = (OutT)v[r];
  }
}

template <int MT> constexpr int ring_depth() { return MT == 16 ? 3 : 4; }
template <int MT> constexpr size_t ring_bytes() {
  return (size_t)ring_depth<MT>() * ((size_t)MT * 16 + kBlockCols) * kPhaseBytes;
}

template <typename OutT, int MT>
__global__ __launch_bounds__(512) void int8_gemm_kernel(const Int8Gemm p) {
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
  // phases of this slice: `nfull` whole ones and, at the very end of an odd K / 64, one half phase
  const int64_t halves = p.K / kHalfBytes, phases = (halves + 1) >> 1;
  const int64_t ph0 = (int64_t)sp * p.per;
  const int nph = (int)min((int64_t)p.per, phases - ph0);            // >= 1 by the plan
  const int nfull = nph - (((halves & 1) != 0 && ph0 + nph == phases) ? 1 : 0);

  if (wave >= 4) {
    // ---------------------------------------------------------------- loaders
    const int ld = wave - 4;
    const uint32_t lds0 = lds_addr_of(smem);
    // lane -> (row, 16-byte slot) of the piece it fills: LDS byte piece*1024 + lane*16 is line piece*4 + lane/16,
    // physical position lane%16, which holds logical position lane%16 ^ (line & 15) = (row & 1) * 8 + slot.
    // *fix: what a lane of the second half (slot >= 4) steps back in the half phase, where only 64 bytes exist
    uint32_t xoff[XL], woff[WL], xfix[XL], wfix[WL], xdst[XL], wdst[WL];
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int piece = (ld * XL + i) % XPIECES;
      const int line = piece * 4 + (lane >> 4);
      const int logical = (lane & 15) ^ (line & 15);
      const int64_t m = min((int64_t)(line * 2 + (logical >> 3)), p.M - 1);     // rows past M: re-read the last
      xoff[i] = (uint32_t)(m * p.lda + (logical & 7) * 16);
      xfix[i] = (logical & 4) ? kHalfBytes : 0;
      xdst[i] = __builtin_amdgcn_readfirstlane(lds0 + piece * 1024);
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int piece = ld * WL + i;
      const int line = piece * 4 + (lane >> 4);
      const int logical = (lane & 15) ^ (line & 15);
      const int64_t n = min(n_blk + line * 2 + (logical >> 3), p.N - 1);        // ragged last block: clamp
      woff[i] = (uint32_t)(n * p.ldb + (logical & 7) * 16);
      wfix[i] = (logical & 4) ? kHalfBytes : 0;
      wdst[i] = __builtin_amdgcn_readfirstlane(lds0 + XBYTES + piece * 1024);
    }
    const int rot = nfull > 0 ? (int)(((int64_t)blockIdx.x * kRotStep) % nfull) : 0;
    auto issue = [&](int i) __attribute__((always_inline)) {
      const uint32_t st = (uint32_t)(i % R) * STAGE;
      const bool half = i >= nfull;                                 // wave-uniform
      int k = i + rot;
      k = half ? nfull : (k >= nfull ? k - nfull : k);
      const int64_t kbyte = (ph0 + k) * kPhaseBytes;                // wave-uniform: scalar base
      const uint8_t* xa = p.a + kbyte;
      const uint8_t* wa = p.b + kbyte;
#pragma unroll
      for (int j = 0; j < XL; ++j) glds16_s(xoff[j] - (half ? xfix[j] : 0u), xa, xdst[j] + st);
#pragma unroll
      for (int j = 0; j < WL; ++j) glds16_s(woff[j] - (half ? wfix[j] : 0u), wa, wdst[j] + st);
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
    i32x4 acc[2][MT];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[tn][t] = i32x4{0, 0, 0, 0};
    int stage = 0;
    // one phase: KC = 2 MFMA depths, or 1 in the half phase
    auto phase = [&](auto kc) __attribute__((always_inline)) {
      constexpr int KC = decltype(kc)::value;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                                 // the phase landed (the loaders waited for it)
      const char* xb = smem + stage * STAGE;
      const char* wb = xb + XBYTES;
      stage = stage + 1 == R ? 0 : stage + 1;
      uint4 wf[2][KC], xf[MT][KC];
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int s = 0; s < KC; ++s) wf[tn][s] = frag(wb, wave * 32 + tn * 16 + r16, s * 4 + q);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int s = 0; s < KC; ++s) xf[t][s] = frag(xb, t * 16 + r16, s * 4 + q);
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int s = 0; s < KC; ++s)
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) acc[tn][t] = mfma_i8(wf[tn][s], xf[t][s], acc[tn][t]);
      if constexpr (KC == 2) {
        // one wave per SIMD, so nothing else hides the LDS latency: the a fragments run PF row tiles ahead of their MFMAs
        constexpr int PF = MT < 2 ? MT : 2;
        __builtin_amdgcn_sched_group_barrier(0x100, 4 + 2 * PF, 0);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          if (t + PF < MT) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
      }
    };
    for (int i = 0; i < nfull; ++i) phase(IntC<2>());
    if (nfull < nph) phase(IntC<1>());
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                   // every stage consumed: LDS is free
    // lane holds columns 32*wave + 16*tn + 4*q .. +3 of rows 16*t + r16
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        *(i32x4*)(smem + (t * 16 + r16) * kTilePitch + (wave * 32 + tn * 16 + 4 * q) * 4) = acc[tn][t];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // ------------------------------------------------------------------ whole-row stores: 32 lanes x 4 columns per row,
  // two rows per wave instruction, 16 rows per sweep of the 8 waves
  const int c = (lane & 31) * 4;
  const int64_t n0 = n_blk + c;
  if (n0 >= p.N) return;
  const bool to_slab = p.raw != 0;
  const bool full4 = n0 + 3 < p.N;
  const bool has_bias = p.bias != nullptr;
  float bv[4] = {0.f, 0.f, 0.f, 0.f}, sbv[4] = {0.f, 0.f, 0.f, 0.f};
  if (!to_slab) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sbv[r] = p.sb[min(n0 + r, p.N - 1)];
      if (has_bias) bv[r] = (float)((const OutT*)p.bias)[min(n0 + r, p.N - 1)];
    }
  }
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = i * 16 + wave * 2 + (lane >> 5);
    if (row >= p.M) continue;
    const i32x4 a = *(const i32x4*)(smem + row * kTilePitch + c * 4);
    if (to_slab) {
      int32_t* dst = p.slab + ((int64_t)sp * p.M + row) * p.N + n0;
      if (full4 && (p.N & 3) == 0) {
        *(i32x4*)dst = a;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n0 + r < p.N) dst[r] = a[r];
      }
    } else {
      const float sa = p.sa[row];
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = dequant(a[r], sa, sbv[r], bv[r], has_bias);
      store4<OutT>((OutT*)p.out + (int64_t)row * p.ldo + n0, v, n0, p.N, full4 && (p.ldo & 3) == 0);
    }
  }
}

// out = epilogue(slab[0] + slab[1] + ...): one thread per 4 consecutive columns; the int32 sum is exact
template <typename OutT>
__global__ __launch_bounds__(256) void int8_gemm_reduce_kernel(const Int8Gemm p) {
  const int64_t nq = (p.N + 3) / 4;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= p.M * nq) return;
  const int64_t m = gid / nq, n0 = (gid % nq) * 4;
  const bool full4 = n0 + 3 < p.N;
  const bool vec = full4 && (p.N & 3) == 0;
  const bool has_bias = p.bias != nullptr;
  int acc[4] = {0, 0, 0, 0};
  for (int s = 0; s < p.S; ++s) {
    const int32_t* src = p.slab + ((int64_t)s * p.M + m) * p.N + n0;
    if (vec) {
      const i32x4 a = *(const i32x4*)src;
      acc[0] += a[0]; acc[1] += a[1]; acc[2] += a[2]; acc[3] += a[3];
    } else {
      for (int r = 0; r < 4; ++r)
        if (n0 + r < p.N) acc[r] += src[r];
    }
  }
  const float sa = p.sa[m];
  float v[4];
  for (int r = 0; r < 4; ++r) {
    const int64_t n = min(n0 + r, p.N - 1);
    v[r] = dequant(acc[r], sa, p.sb[n], has_bias ? (float)((const OutT*)p.bias)[n] : 0.f, has_bias);
  }
  store4<OutT>((OutT*)p.out + m * p.ldo + n0, v, n0, p.N, full4 && (p.ldo & 3) == 0);
}

// ------------------------------------------------------------------------------------------------ tile kernel
template <typename OutT>
__global__ __launch_bounds__(512) void int8_gemm_tile_kernel(const Int8Gemm p) {
  constexpr int MF = 16;                       // rows of an MFMA operand
  constexpr int NI = 128 / MF, NJ = 64 / MF;   // m- and n-tiles of a wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rl = lane & 15, qg = lane >> 4;
  const int wm = wave >> 2, wn = wave & 3;
  const int64_t m0 = (int64_t)blockIdx.y * kBM, n0 = (int64_t)blockIdx.x * kBN;
  const int64_t halves = p.K / kHalfBytes;
  const int steps = (int)((halves + 1) >> 1);
  const bool odd = (halves & 1) != 0;          // the last k-step holds 64 bytes only

  // DMA geometry: piece i of wave w covers tile rows 8 (4w + i) ..+7 of either operand; stage s is [a 32 KiB][b 32 KiB]
  const uint32_t lds_piece = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + wave * 4096);
  const int xclamp = (int)min((int64_t)(kBM - 1), p.M - 1 - m0);
  const int wclamp = (int)min((int64_t)(kBN - 1), p.N - 1 - n0);
  uint32_t xoff[4], woff[4], fix[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int line = (wave * 4 + i) * 4 + (lane >> 4);
    const int logical = (lane & 15) ^ (line & 15);
    const int row = line * 2 + (logical >> 3);
    xoff[i] = (uint32_t)min(row, xclamp) * (uint32_t)p.lda + (uint32_t)(logical & 7) * 16;   // < 2^32 (host check)
    woff[i] = (uint32_t)min(row, wclamp) * (uint32_t)p.ldb + (uint32_t)(logical & 7) * 16;
    fix[i] = (logical & 4) ? kHalfBytes : 0;
  }
  const uint8_t* xblk = uniform_ptr(p.a + m0 * p.lda);
  const uint8_t* wblk = uniform_ptr(p.b + n0 * p.ldb);
  auto request = [&](int kt) __attribute__((always_inline)) {
    const bool half = odd && kt == steps - 1;   // the second half would lie past the row: read the first twice
    const uint32_t dst = lds_piece + (uint32_t)(kt & 1) * (2 * kStage);
    const uint8_t* xs = xblk + (int64_t)kt * kPhaseBytes;
    const uint8_t* ws = wblk + (int64_t)kt * kPhaseBytes;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      glds16_s(xoff[i] - (half ? fix[i] : 0u), xs, dst + i * 1024);
      glds16_s(woff[i] - (half ? fix[i] : 0u), ws, dst + kStage + i * 1024);
    }
  };

  i32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  auto compute = [&](int kt, auto kc) __attribute__((always_inline)) {
    constexpr int KC = decltype(kc)::value;
    const char* xb = smem + (kt & 1) * (2 * kStage) + wm * 128 * kPhaseBytes;
    const char* wb = smem + (kt & 1) * (2 * kStage) + kStage + wn * 64 * kPhaseBytes;
    uint4 wf[NJ][KC], xf[KC];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int c = 0; c < KC; ++c) wf[j][c] = frag(wb, j * MF + rl, c * 4 + qg);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
#pragma unroll
      for (int c = 0; c < KC; ++c) xf[c] = frag(xb, i * MF + rl, c * 4 + qg);
#pragma unroll
      for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = mfma_i8(wf[j][c], xf[c], acc[i][j]);
    }
  };

  request(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int nfull = steps - (odd ? 1 : 0);
  for (int kt = 0; kt < nfull; ++kt) {
    if (kt + 1 < steps) request(kt + 1);               // into the stage every wave left at the last barrier
    compute(kt, IntC<2>());
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // step kt + 1 landed; every wave is done with step kt
  }
  if (odd) {                                           // the half step, one MFMA depth
    compute(nfull, IntC<1>());
    __syncthreads();
  }

  // ---- epilogue: the lane holds out[m0 + wm*128 + i*16 + rl][n0 + wn*64 + j*16 + 4*qg + r]; two rounds of 128 parked
  // rows (64 of each wm), then whole rows leave: 32 lanes x 8 columns, 2 rows per wave instruction
  const int c = (lane & 31) * 8;
  const int64_t n = n0 + c;
  const bool has_bias = p.bias != nullptr;
  const bool vec = n + 8 <= p.N && p.ldo % 8 == 0;
  float sbv[8], bv[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int64_t nn = min(n + r, p.N - 1);
    sbv[r] = p.sb[nn];
    bv[r] = has_bias ? (float)((const OutT*)p.bias)[nn] : 0.f;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int ii = 0; ii < NI / 2; ++ii)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        *(i32x4*)(smem + (wm * 64 + ii * MF + rl) * kParkPitch + (wn * 64 + j * MF + 4 * qg) * 4) =
            acc[h * (NI / 2) + ii][j];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kParkRows / 16; ++it) {
      const int pr = (it * 8 + wave) * 2 + (lane >> 5);
      const int64_t m = m0 + (pr >> 6) * 128 + h * 64 + (pr & 63);
      if (m >= p.M || n >= p.N) continue;
      const float sa = p.sa[m];
      float v[8];
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const i32x4 a = *(const i32x4*)(smem + pr * kParkPitch + (c + 4 * g) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[4 * g + r] = dequant(a[r], sa, sbv[4 * g + r], bv[4 * g + r], has_bias);
      }
      OutT* o = (OutT*)p.out + m * p.ldo + n;
      if (vec) {
        *(u32x4*)o = u32x4{pack2<OutT>(v[0], v[1]), pack2<OutT>(v[2], v[3]), pack2<OutT>(v[4], v[5]), pack2<OutT>(v[6], v[7])};
      } else {
#pragma unroll
        for (int r = 0; r < 8; ++r)
          if (n + r < p.N) o[r] = (OutT)v[r];
      }
    }
    __syncthreads();      // every wave has read its parked rows before the next round overwrites them
  }
}

// Split-K plan of the decode kernel: S slices of `per` phases.  With at least 200 column blocks the grid fills the 256
// CUs by itself; below that K is split until about one round of workgroups exists, but never into slices of less than
// 4 phases (the ring prologue and the slab traffic of a slice are paid per slice).  Independent of M.
void plan_splits(int64_t N, int64_t K, int* S, int* per) {
  const int64_t nph = cdiv64(K, kPhaseBytes), nblk = cdiv64(N, kBlockCols);
  int64_t want = nblk >= 200 ? 1 : 256 / nblk;
  if (want > nph / 4) want = nph / 4;
  if (want < 1) want = 1;
  *per = (int)cdiv64(nph, want);
  *S = (int)cdiv64(nph, *per);
}

// the shape-only part of the preconditions (what mi_int8_gemm_workspace_bytes can see)
const char* shape_refusal(int64_t M, int64_t N, int64_t K) {
  if (K % kHalfBytes != 0) return "K must be a multiple of 64";
  if (K > kMaxK) return "K above 131072 (the int32 accumulator could wrap)";
  if (cdiv64(N, kBlockCols) > 0x7fffffff) return "N too large for the grid";
  if (M > kPassRows && cdiv64(M, kBM) > 65535) return "M too large for the grid";
  return nullptr;
}

int64_t slab_bytes(int64_t M, int64_t N, int S) {
  return M <= kPassRows && S > 1 ? (int64_t)S * M * N * (int64_t)sizeof(int32_t) : 0;
}

template <typename OutT, int MT>
void launch_decode(const Int8Gemm& p, hipStream_t st) {
  const dim3 grid((unsigned)cdiv64(p.N, kBlockCols), (unsigned)p.S);
  int8_gemm_kernel<OutT, MT><<<grid, 512, ring_bytes<MT>(), st>>>(p);
  if (p.S > 1 && p.out != nullptr) {             // (the partial launch has no `out`: its caller consumes the slabs)
    const int64_t total = p.M * cdiv64(p.N, 4);
    int8_gemm_reduce_kernel<OutT><<<(unsigned)cdiv64(total, 256), 256, 0, st>>>(p);
  }
}

template <typename OutT>
void launch(const Int8Gemm& p, hipStream_t st) {
  if (p.M <= 16) launch_decode<OutT, 1>(p, st);
  else if (p.M <= 32) launch_decode<OutT, 2>(p, st);
  else if (p.M <= 64) launch_decode<OutT, 4>(p, st);
  else if (p.M <= 128) launch_decode<OutT, 8>(p, st);
  else if (p.M <= kPassRows) launch_decode<OutT, 16>(p, st);
  else {
    const dim3 grid((unsigned)cdiv64(p.N, kBN), (unsigned)cdiv64(p.M, kBM));
    int8_gemm_tile_kernel<OutT><<<grid, 512, kTileLds, st>>>(p);
  }
}

}  // namespace

extern "C" int64_t mi_int8_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M < 0 || N < 0 || K <= 0 || shape_refusal(M, N, K)) return -1;
  if (M == 0 || N == 0) return 0;
  int S, per;
  plan_splits(N, K, &S, &per);
  return slab_bytes(M, N, S);
}

extern "C" int mi_int8_gemm(const void* a, const void* b_nk, const float* scale_a, const float* scale_b, const void* bias,
                            void* out, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldo,
                            int out_dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  MI_CHECK_ARG(M >= 0 && N >= 0 && K > 0);
  MI_CHECK_ARG(out_dtype == MI_BF16 || out_dtype == MI_FP16);
  if (M == 0 || N == 0) return MI_OK;
  MI_CHECK_ARG(a && b_nk && scale_a && scale_b && out);
  MI_CHECK_ARG(lda >= K && ldb >= K && ldo >= N);
  MI_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= 0);
  if (const char* why = shape_refusal(M, N, K))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm: %s (M %lld N %lld K %lld)", why, (long long)M, (long long)N, (long long)K);
  if (lda % 16 != 0 || ldb % 16 != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm: lda and ldb must be multiples of 16 (got %lld %lld)", (long long)lda,
            (long long)ldb);
  if ((((uintptr_t)a | (uintptr_t)b_nk | (uintptr_t)out) & 15) != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm: a, b_nk and out must be 16-byte aligned");
  // the DMA addresses are a scalar base + a 32-bit lane offset (row * pitch + at most 128 bytes of the phase): rows
  // of the whole operand in the decode kernel, of one 256-row block in the tile kernel
  const uint64_t lim = 1ull << 32;
  const uint64_t arows = (uint64_t)min(M, (int64_t)kBM) - 1, brows = (uint64_t)(M <= kPassRows ? N : min(N, (int64_t)kBN)) - 1;
  if (arows * (uint64_t)lda + kPhaseBytes >= lim || brows * (uint64_t)ldb + kPhaseBytes >= lim)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm: operand rows span 4 GiB or more (32-bit lane offsets)");
  Int8Gemm p;
  p.a = (const uint8_t*)a; p.b = (const uint8_t*)b_nk; p.sa = scale_a; p.sb = scale_b; p.bias = bias; p.out = out;
  p.slab = (int32_t*)workspace;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldo = ldo;
  plan_splits(N, K, &p.S, &p.per);
  const int64_t need = slab_bytes(M, N, p.S);
  if (M > kPassRows || need > workspace_bytes || (need > 0 && workspace == nullptr)) {   // no room for slabs: no split-K
    p.S = 1;
    p.per = (int)cdiv64(K, kPhaseBytes);
  }
  p.raw = p.S > 1;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == MI_BF16) launch<bf16_t>(p, st);
  else launch<f16_t>(p, st);
  MI_CHECK_LAUNCH();
  return MI_OK;
}

// ---- hooks of the fused "GEMM + consumer" forms (int8_glue.hip); not part of the C ABI
MI_INTERNAL void mi_int8_gemm_plan_splits(int64_t N, int64_t K, int* S, int* per) { plan_splits(N, K, S, per); }

// The decode kernel alone (M <= 256): raw int32 accumulators into slab[S][M][N], S = the plan's, also when S == 1; no
// reduce, no scales.  Same operand preconditions as mi_int8_gemm; N % 4 == 0 and a 16-byte aligned slab on top.
MI_INTERNAL int mi_int8_gemm_partial(const void* a, const void* b_nk, int32_t* slab, int64_t M, int64_t N, int64_t K,
                                     int64_t lda, int64_t ldb, void* stream) {
  MI_CHECK_ARG(M > 0 && M <= kPassRows && N > 0 && N % 4 == 0 && K > 0 && a && b_nk && slab);
  MI_CHECK_ARG(lda >= K && ldb >= K && ((uintptr_t)slab & 15) == 0);
  if (const char* why = shape_refusal(M, N, K))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm (fused): %s (M %lld N %lld K %lld)", why, (long long)M, (long long)N, (long long)K);
  if (lda % 16 != 0 || ldb % 16 != 0 || (((uintptr_t)a | (uintptr_t)b_nk) & 15) != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm (fused): a and b_nk must be 16-byte aligned, lda and ldb multiples of 16");
  if ((uint64_t)(M - 1) * (uint64_t)lda + kPhaseBytes >= (1ull << 32) || (uint64_t)(N - 1) * (uint64_t)ldb + kPhaseBytes >= (1ull << 32))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_int8_gemm (fused): operand rows span 4 GiB or more (32-bit lane offsets)");
  Int8Gemm p;
  p.a = (const uint8_t*)a; p.b = (const uint8_t*)b_nk; p.sa = nullptr; p.sb = nullptr; p.bias = nullptr; p.out = nullptr;
  p.slab = slab;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldo = N;
  plan_splits(N, K, &p.S, &p.per);
  p.raw = 1;
  launch<bf16_t>(p, (hipStream_t)stream);      // OutT only types the epilogue this launch does not take
  MI_CHECK_LAUNCH();
  return MI_OK;
}
