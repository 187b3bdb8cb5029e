// Prefill-shaped 16-bit linear: out[M,N] = x[M,K] . W[N,K]^T (+ bias), x and W both bf16 or both fp16, fp32
// accumulation, output in the activation dtype or fp32, ONE rounding.  The M > 512 sibling of bf16_gemm_kernel and the
// unquantised sibling of fp8_gemm_tile_kernel; weights stay in the torch.nn.Linear layout.
//
//   work split   a 512-thread workgroup owns a 256 x 256 output tile; wave (wm, wn) of the 2 x 4 wave grid owns
//                128 (m) x 64 (n) = 128 accumulator registers per lane.  The grid is persistent, min(tiles, CUs)
//                workgroups, and the tiles are renumbered so that each XCD walks a contiguous range in groups of
//                8 m-blocks x all n: what is resident on one XCD shares both operand blocks in its L2.
//   k-step       128 bytes of K = 64 elements.  Both operands go global -> LDS by LDS-DMA in 1-KiB pieces of 8 rows x
//                128 B, wave w issues pieces 4w..4w+3 of either operand: one scalar base per operand and k-step, one
//                32-bit lane offset per piece (rebuilt per tile, rows past the matrix edge clamped onto the last one).
//   LDS image    lane-linear destination; two consecutive rows share a 256-byte line and the 16-byte slot inside the
//                line pair is XORed with (line & 15) on the SOURCE address: every ds_read_b128 fragment read (16 rows x
//                4 slots) touches each bank group once.
//   ring         160 KiB = 5 stages of 32 KiB: TWO activation stages (requested one k-step ahead) and THREE weight
//                stages (requested two ahead).  A 16-bit k-step stages the same 64 KiB as an FP8 one for half the
//                MFMA time, so the kernel is at least as DMA-bound as fp8_gemm_tile_kernel; the weights are what comes
//                from HBM, the activation block is re-read by every n-block and sits in L2.  One counted wait
//                (vmcnt(4): everything but the weight pieces just requested) and one barrier per k-step.
//   MFMA         v_mfma_f32_16x16x32_{bf16,f16}, 8 x 4 tiles per wave, two per tile and k-step: 8 elements = one
//                16-byte LDS read per lane and operand, 24 reads per wave and k-step.  Weights are the A operand,
//                activations B: a lane ends with 4 consecutive output columns of one row.  (v_mfma_f32_32x32x16 reads
//                the same bytes for half the instructions and measured 5-8 % slower at every C2 shape: DESIGN 3.3c.)
//   epilogue     the ring is drained; the fp32 tile is parked in it in two rounds of 128 rows (64 of each wave), rows
//                padded to 1040 bytes, and all 8 waves write whole rows with 16-byte non-temporal stores: acc + bias,
//                one rounding, to `out`, or raw fp32 to slab[s][m][n] under split-K.  Ragged edges mask; a row stride
//                or column count that does not allow 16-byte stores takes the per-element path.
//   split-K      grids that leave half the CUs idle split K into S <= 4 slices (grid.y) of at least 16 k-steps;
//                bf16_gemm_reduce_kernel (bf16_gemm.hip) sums the slabs in split order, adds the bias, rounds once.
// No atomics, no memset, no allocation, no synchronisation: capturable.
#include "common.h"

MI_INTERNAL void mi_bf16_gemm_reduce(float* slab, const void* bias, void* out, int64_t M, int64_t N, int64_t ldo, int S,
                                     int dtype, int out_dtype, hipStream_t st);      // bf16_gemm.hip

namespace {

constexpr int kBM = 256, kBN = 256;       // output tile
constexpr int kStepBytes = 128;           // bytes of K per k-step
constexpr int kStepElems = 64;
constexpr int kStage = kBM * kStepBytes;  // 32 KiB per operand and stage
constexpr int kXStages = 2, kWStages = 3;
constexpr int kRing = (kXStages + kWStages) * kStage;   // 160 KiB
constexpr int kParkRows = 128;            // rows parked per epilogue round
constexpr int kParkPitch = kBN * 4 + 16;  // 256 fp32 + 16 bytes: conflict-free b128 writes from the MFMA layout
constexpr int kGroupM = 8;                // m-blocks per tile group
constexpr int kMaxSplits = 4, kMinSliceSteps = 16, kFillCUs = 256;
static_assert(kParkRows * kParkPitch <= kRing, "the parked half tile reuses the ring");

struct TileGemm {
  const uint8_t* x;
  const uint8_t* w;
  const void* bias;   // T[N] or null
  void* out;          // OutT, row stride ldo
  float* slab;        // [S][M][N] when S > 1
  int64_t M, N, K, lda, ldb, ldo;   // strides in elements
  int mblocks, nblocks;
  int S, per;         // split-K slices, k-steps per slice
};

// 16-byte streaming store: the output is not read again by this kernel, and written the ordinary way it displaces the
// operand blocks the workgroups of the XCD share in L2
__device__ __forceinline__ void stream_store16(void* dst, u32x4 v) { __builtin_nontemporal_store(v, (u32x4*)dst); }

// One epilogue round: the 128 parked rows leave as whole rows, 16 bytes per lane (8 columns of a 16-bit, 4 of an fp32
// destination), 2 or 1 rows per wave instruction, 16 or 8 rows per sweep of the 8 waves.  Parked row r is tile row
// (r / 64) * 128 + h * 64 + r % 64.  dst = round_once(parked + bias).
template <typename DstT, typename T>
__device__ __forceinline__ void store_rows(const char* park, DstT* dst, int64_t ld, const T* bias, int64_t m0, int64_t n0,
                                           int64_t M, int64_t N, int h, int wave, int lane) {
  constexpr int CPL = 16 / (int)sizeof(DstT);   // columns per lane
  constexpr int LPR = kBN / CPL;                // lanes per row
  constexpr int RPI = 64 / LPR;                 // rows per wave instruction
  const int c = (lane % LPR) * CPL;
  const int64_t n = n0 + c;
  if (n >= N) return;
  const bool vec = n + CPL <= N && ld % CPL == 0;
  float bv[CPL];
#pragma unroll
  for (int r = 0; r < CPL; ++r) bv[r] = bias ? (float)bias[min(n + r, N - 1)] : 0.f;
#pragma unroll
  for (int it = 0; it < kParkRows / (8 * RPI); ++it) {
    const int pr = (it * 8 + wave) * RPI + lane / LPR;
    const int64_t m = m0 + (pr >> 6) * 128 + h * 64 + (pr & 63);
    if (m >= M) continue;
    float v[CPL];
#pragma unroll
    for (int g = 0; g < CPL / 4; ++g) {
      const f32x4 a = *(const f32x4*)(park + pr * kParkPitch + (c + 4 * g) * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * g + r] = a[r] + bv[4 * g + r];
    }
    DstT* o = dst + m * ld + n;
    if (vec) {
      if constexpr (__is_same(DstT, float))
        stream_store16(o, u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])});
      else
        stream_store16(o, u32x4{pack2<DstT>(v[0], v[1]), pack2<DstT>(v[2], v[3]), pack2<DstT>(v[4], v[5]), pack2<DstT>(v[6], v[7])});
    } else {
#pragma unroll
      for (int r = 0; r < CPL; ++r)
        if (n + r < N) o[r] = (DstT)v[r];
    }
  }
}

template <typename T, typename OutT>
__global__ __launch_bounds__(512) void bf16_gemm_tile_kernel(const TileGemm p) {
  typedef typename Elem<T>::vec8 vec8;
  constexpr int MF = 16;                   // rows of an MFMA operand; a lane reads slot c * 4 + lane / 16 of row lane % 16
  constexpr int KC = 2;                    // MFMAs along k per k-step (32 elements each)
  constexpr int NI = 128 / MF, NJ = 64 / MF;   // m- and n-tiles of a wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rl = lane & 15, qg = lane >> 4;
  const int wm = wave >> 2, wn = wave & 3;

  // tile order: hardware deals workgroup ids round-robin to the 8 XCDs, so XCD x takes a contiguous range of the tile
  // list and its workgroups walk that range together; inside the range the tiles are grouped kGroupM m-blocks x all n
  const int nwg = p.mblocks * p.nblocks;
  const int orig = blockIdx.x, G = gridDim.x;
  const int xcd = orig & 7, slot = orig >> 3, gx = (G - xcd + 7) >> 3;
  const int qd = nwg >> 3, rm = nwg & 7;
  const int xstart = xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd;
  const int xcnt = qd + (xcd < rm ? 1 : 0);
  const int per_group = kGroupM * p.nblocks;

  // split-K (grid.y = S): this workgroup walks k-steps [kt0, kt0 + nk) of its tile
  const int sp = blockIdx.y;
  const int64_t kt0 = (int64_t)sp * p.per;
  const int nk = (int)min((int64_t)p.per, p.K / kStepElems - kt0);     // >= 1 by the plan
  const bool to_slab = p.S > 1;

  // DMA geometry: piece i of wave w covers tile rows 8 (4w + i) ..+7; lane L -> LDS byte piece * 1024 + L * 16, which is
  // line piece * 4 + L / 16, physical position L % 16, holding logical position (row & 1) * 8 + slot = L % 16 ^ (line & 15)
  const uint32_t lds_piece = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + wave * 4096);
  int prow[4];
  uint32_t pslot[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int line = (wave * 4 + i) * 4 + (lane >> 4);
    const int logical = (lane & 15) ^ (line & 15);
    prow[i] = line * 2 + (logical >> 3);
    pslot[i] = (uint32_t)(logical & 7) * 16;
  }
  const uint32_t lda2 = (uint32_t)p.lda * 2, ldb2 = (uint32_t)p.ldb * 2;    // 255 * pitch + 128 < 2^32 (host check)
  auto frag = [&](const char* base, int row, int s) __attribute__((always_inline)) -> vec8 {
    const uint4 v = *(const uint4*)(base + (row >> 1) * 256 + (((((row & 1) << 3) | s) ^ ((row >> 1) & 15)) * 16));
    return __builtin_bit_cast(vec8, v);
  };

  for (int li = slot; li < xcnt; li += gx) {
    const int tid = xstart + li;
    const int grp = tid / per_group, in_grp = tid % per_group;
    const int first_m = grp * kGroupM;
    const int gsz = min(p.mblocks - first_m, kGroupM);
    const int64_t m0 = (int64_t)(first_m + in_grp % gsz) * kBM, n0 = (int64_t)(in_grp / gsz) * kBN;
    const uint8_t* xblk = uniform_ptr(p.x + (m0 * p.lda + kt0 * kStepElems) * 2);
    const uint8_t* wblk = uniform_ptr(p.w + (n0 * p.ldb + kt0 * kStepElems) * 2);
    const int xclamp = __builtin_amdgcn_readfirstlane((int)min((int64_t)(kBM - 1), p.M - 1 - m0));
    const int wclamp = __builtin_amdgcn_readfirstlane((int)min((int64_t)(kBN - 1), p.N - 1 - n0));
    uint32_t xoff[4], woff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xoff[i] = (uint32_t)min(prow[i], xclamp) * lda2 + pslot[i];
      woff[i] = (uint32_t)min(prow[i], wclamp) * ldb2 + pslot[i];
    }

    f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // prologue: activations of k-step 0, weights of k-steps 0 and 1 (a one-step slice repeats step 0: never read)
    const uint8_t* w1 = wblk + (nk > 1 ? kStepBytes : 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      glds16_s(xoff[i], xblk, lds_piece + i * 1024);
      glds16_s(woff[i], wblk, lds_piece + kXStages * kStage + i * 1024);
      glds16_s(woff[i], w1, lds_piece + (kXStages + 1) * kStage + i * 1024);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int ws = 0;                                      // weight stage of the k-step being consumed: kt % 3
    for (int kt = 0; kt < nk; ++kt) {
      // requests: this wave's 4 activation pieces of k-step kt + 1 FIRST, then its 4 weight pieces of kt + 2, placed
      // between the first MFMA groups; the wait at the end leaves exactly those 4 weight pieces in flight.  Past the
      // end of the slice the last k-step is requested again (never read): the loop body stays one basic block.
      const uint8_t* xs = xblk + (int64_t)min(kt + 1, nk - 1) * kStepBytes;
      const uint8_t* wsrc = wblk + (int64_t)min(kt + 2, nk - 1) * kStepBytes;
      const uint32_t xdst = lds_piece + (uint32_t)((kt + 1) & 1) * kStage;
      const uint32_t wdst = lds_piece + (uint32_t)(kXStages + (ws == 0 ? 2 : ws - 1)) * kStage;
      const char* xb = smem + (kt & 1) * kStage + wm * 128 * kStepBytes;
      const char* wb = smem + (kXStages + ws) * kStage + wn * 64 * kStepBytes;
      ws = ws == 2 ? 0 : ws + 1;
      vec8 wf[NJ][KC], xfb[2][KC];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int c = 0; c < KC; ++c) wf[j][c] = frag(wb, j * MF + rl, c * 4 + qg);
#pragma unroll
      for (int c = 0; c < KC; ++c) xfb[0][c] = frag(xb, rl, c * 4 + qg);
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        // activation fragments one m-tile ahead, in a second register set
        if (i + 1 < NI) {
#pragma unroll
          for (int c = 0; c < KC; ++c) xfb[(i + 1) & 1][c] = frag(xb, (i + 1) * MF + rl, c * 4 + qg);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (i < 2) {
          glds16_s(xoff[2 * i], xs, xdst + (2 * i) * 1024);
          glds16_s(xoff[2 * i + 1], xs, xdst + (2 * i + 1) * 1024);
        } else if (i < 4) {
          glds16_s(woff[2 * i - 4], wsrc, wdst + (2 * i - 4) * 1024);
          glds16_s(woff[2 * i - 3], wsrc, wdst + (2 * i - 3) * 1024);
        }
#pragma unroll
        for (int c = 0; c < KC; ++c)
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[i][j] = Elem<T>::mfma16(wf[j][c], xfb[i & 1][c], acc[i][j]);
      }
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __syncthreads();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the repeated requests have landed: the ring is free
    __syncthreads();

    // ---- epilogue: the lane holds out[m0 + wm*128 + i*16 + rl][n0 + wn*64 + j*16 + 4*qg + r]
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int ii = 0; ii < NI / 2; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          *(f32x4*)(smem + (wm * 64 + ii * MF + rl) * kParkPitch + (wn * 64 + j * MF + 4 * qg) * 4) =
              acc[h * (NI / 2) + ii][j];
      __syncthreads();
      if (to_slab)
        store_rows<float, T>(smem, p.slab + (int64_t)sp * p.M * p.N, p.N, nullptr, m0, n0, p.M, p.N, h, wave, lane);
      else
        store_rows<OutT, T>(smem, (OutT*)p.out, p.ldo, (const T*)p.bias, m0, n0, p.M, p.N, h, wave, lane);
      __syncthreads();      // every wave has read its parked rows before the next round, or the next tile, overwrites them
    }
  }
}

// Split-K plan: S slices of `per` k-steps.  A grid of more than half the CUs runs unsplit; below that K is split until
// about one round of workgroups exists, into at most 4 slices (each costs a write and a read of M x N fp32) of at
// least 16 k-steps (the ring prologue and the drain are paid per slice).
void plan_splits(int64_t M, int64_t N, int64_t K, int* S, int* per) {
  const int64_t steps = K / kStepElems, tiles = cdiv64(M, kBM) * cdiv64(N, kBN);
  int64_t want = min((int64_t)kMaxSplits, min(kFillCUs / tiles, steps / kMinSliceSteps));
  if (want < 1) want = 1;
  *per = (int)cdiv64(steps, want);
  *S = (int)cdiv64(steps, *per);
}

// the shape-only part of the preconditions (what mi_bf16_gemm_tile_workspace_bytes can see)
const char* shape_refusal(int64_t M, int64_t N, int64_t K) {
  if (K % kStepElems != 0) return "K must be a multiple of 64";
  if (K / kStepElems > 0x7fffffff) return "K too large";
  if (M > 0 && N > 0 && cdiv64(M, kBM) > 0x7fffffff / cdiv64(N, kBN)) return "too many tiles for the grid";
  return nullptr;
}

int tile_cus() {
  static const int cus = [] {
    const int n = mi_device_cu_count();
    return n > 0 ? n : kFillCUs;
  }();
  return cus;
}

template <typename T, typename OutT>
void launch_tile(const TileGemm& p, hipStream_t st) {
  // S == 1: persistent, one workgroup per CU walks its share of the tiles; split-K: one workgroup per (tile, slice)
  const int tiles = p.mblocks * p.nblocks;
  const dim3 grid((unsigned)(p.S == 1 ? min(tiles, tile_cus()) : tiles), (unsigned)p.S);
  bf16_gemm_tile_kernel<T, OutT><<<grid, 512, kRing, st>>>(p);
}

}  // namespace

extern "C" int64_t mi_bf16_gemm_tile_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M < 0 || N < 0 || K <= 0 || shape_refusal(M, N, K)) return -1;
  if (M == 0 || N == 0) return 0;
  int S, per;
  plan_splits(M, N, K, &S, &per);
  return S > 1 ? (int64_t)S * M * N * (int64_t)sizeof(float) : 0;
}

extern "C" int mi_bf16_gemm_tile_check(const void* x, const void* w_nk, const void* out, int64_t M, int64_t N, int64_t K,
                                       int64_t lda, int64_t ldb, int64_t ldo, int dtype, int out_dtype) {
  MI_CHECK_ARG(M >= 0 && N >= 0 && K > 0);
  MI_CHECK_ARG(dtype == MI_BF16 || dtype == MI_FP16);
  MI_CHECK_ARG(out_dtype == dtype || out_dtype == MI_F32);
  if (M == 0 || N == 0) return MI_OK;
  MI_CHECK_ARG(x && w_nk && out);
  MI_CHECK_ARG(lda >= K && ldb >= K && ldo >= N);
  if (const char* why = shape_refusal(M, N, K))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm_tile: %s (M %lld N %lld K %lld)", why, (long long)M, (long long)N, (long long)K);
  if (lda % 8 != 0 || ldb % 8 != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm_tile: lda and ldb must be multiples of 8 (got %lld %lld)", (long long)lda,
            (long long)ldb);
  if ((((uintptr_t)x | (uintptr_t)w_nk | (uintptr_t)out) & 15) != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm_tile: x, w_nk and out must be 16-byte aligned");
  // the DMA addresses are a scalar base (block start + k offset) + a 32-bit lane offset: at most 255 rows + 128 bytes
  const uint64_t lim = 1ull << 32;
  if ((uint64_t)(kBM - 1) * (uint64_t)lda * 2 + kStepBytes >= lim || (uint64_t)(kBN - 1) * (uint64_t)ldb * 2 + kStepBytes >= lim)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_bf16_gemm_tile: 255 rows of x or w_nk span 4 GiB or more (32-bit lane offsets)");
  return MI_OK;
}

extern "C" int mi_bf16_gemm_tile(const void* x, const void* w_nk, const void* bias, void* out, int64_t M, int64_t N,
                                 int64_t K, int64_t lda, int64_t ldb, int64_t ldo, int dtype, int out_dtype,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = mi_bf16_gemm_tile_check(x, w_nk, out, M, N, K, lda, ldb, ldo, dtype, out_dtype);
  if (rc != MI_OK || M == 0 || N == 0) return rc;
  MI_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= 0);
  TileGemm p;
  p.x = (const uint8_t*)x; p.w = (const uint8_t*)w_nk; p.bias = bias; p.out = out; p.slab = (float*)workspace;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldo = ldo;
  p.mblocks = (int)cdiv64(M, kBM); p.nblocks = (int)cdiv64(N, kBN);
  plan_splits(M, N, K, &p.S, &p.per);
  const int64_t need = p.S > 1 ? (int64_t)p.S * M * N * (int64_t)sizeof(float) : 0;
  if (need > workspace_bytes || (need > 0 && workspace == nullptr)) {   // no room for slabs: no split-K
    p.S = 1;
    p.per = (int)(K / kStepElems);
  }
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MI_BF16) {
    if (out_dtype == MI_F32) launch_tile<bf16_t, float>(p, st);
    else launch_tile<bf16_t, bf16_t>(p, st);
  } else {
    if (out_dtype == MI_F32) launch_tile<f16_t, float>(p, st);
    else launch_tile<f16_t, f16_t>(p, st);
  }
  if (p.S > 1) mi_bf16_gemm_reduce(p.slab, bias, out, M, N, ldo, p.S, dtype, out_dtype, st);
  MI_CHECK_LAUNCH();
  return MI_OK;
}
