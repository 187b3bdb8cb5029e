// Sparse MLP (mixture of experts) for unquantised bf16 / fp16 experts: the top-k softmax router and the fused experts
// call (align, gate_up GEMM + SiLU, down GEMM x router weight, sum over the slots), fp32 accumulation throughout.
// Per call only T, E, k, H, I are host values; which token goes to which expert is read on the device, so a captured
// launch follows topk_ids / topk_weights rewritten in place.  No atomics on global memory, no memset, no allocation,
// no synchronisation: capturable.
//
// router (moe_topk_softmax_kernel): one wave per token, 4 tokens per workgroup, no LDS.
//   registers    lane l holds the logits of experts l, l + 64, l + 128, l + 192 (E <= 256) as fp32; experts >= E hold
//                -inf.  Row max and row sum by xor-shuffles over the 64 lanes; p = expf(v - max) / sum (IEEE divide).
//   top-k        k rounds: each lane's best remaining (value, index), then a 6-step butterfly that keeps the larger
//                value and, on equal values, the LOWER index (moe_topk_softmax_kernels.cu's rule); every lane ends
//                with the same winner, its owner retires it, lane `round` keeps it.  Lanes 0 .. k-1 store.
//
// align (moe_align_kernel): ONE workgroup of 256 threads, a counting sort of the T*k (token, slot) pairs by expert.
//   LDS          count[256] and cursor[256]; pass 1 counts with LDS atomics, thread e < E then sums count[0 .. e) for
//                expert_indptr[e] and its first tile, pass 2 scatters pair indices through the LDS cursors.  The order
//                inside a segment depends on the atomics' order; no result depends on it (an output row depends on
//                its own input row only).  Segments are NOT padded: the tile list holds (expert, first sorted row,
//                rows <= BM) for every row block of BM rows, and n_tiles; the GEMM grids cover the host's bound
//                ceil(T*k / BM) + E and the workgroups past n_tiles exit.  Ids outside [0, E) are not sorted at all.
//
// The two GEMMs are one template each per form over the epilogue (GATEUP: act = silu(g) * u; else y = acc * weight):
//   MFMA         v_mfma_f32_16x16x32_{bf16,f16}, weights as the A operand and activations as B: a lane ends with 4
//                consecutive output columns of ONE row (row = lane & 15, columns 4 (lane >> 4) ..+4), stores are
//                8-byte vectors.  A 64-element k chunk is laid out as lane group g = lane >> 4 holding k0 + 16 g ..+16
//                (32 contiguous bytes per lane, two MFMAs); a sum over k does not care which lane holds which k.
//   gate / up    a wave always owns matching gate and up columns (n and I + n) in the same lane positions, so the
//                [T*k, 2I] intermediate never exists.
//
// rows16 form (decode; moe_rows16_kernel): workgroup = (tile of <= 16 sorted rows of one expert, 64 output columns).
//   work split   the 4 waves split the COLUMNS, 16 each (gate_up: 16 gate + the 16 matching up = two weight tiles);
//                every wave walks all of K, so there is no reduction, no LDS and no barrier.  (Splitting K instead
//                was not measured: DESIGN 3.3g.)
//   registers    weight and activation fragments go global -> registers, steps of 256 (down) or 128 (gate_up) k
//                elements, two steps in flight per wave: 16 KiB of weights per wave on the way at any time.
//   rows         rows past the tile are clamped onto its last row when loaded and masked when stored.  x rows are
//                gathered by token (pair / k) in the B-operand loads; the down GEMM reads act by sorted row.
//   K tail       I % 64 != 0: lane groups whose 16 elements start at or past K load nothing and hold zeros in BOTH
//                operands (I % 16 == 0, so a group is all inside or all outside).
//
// tile form (prefill; moe_tile_kernel): workgroup = (tile of <= 128 sorted rows of one expert, 128 columns); for
//   gate_up the 128 columns are 64 gate + the 64 matching up.
//   work split   4 waves as 2 (rows) x 2 (columns), 64 x 64 each = 4 x 4 MFMA tiles, 64 accumulator registers per
//                lane.  A gate_up wave owns 32 gate + its 32 up columns.  Waves whose 64 rows lie past the tile skip
//                their MFMAs but keep the barriers.
//   LDS          k-step = 64 elements.  Both operands go global -> registers -> LDS as 16-byte pieces, 4 per thread
//                and operand (piece q: row q / 8, slot q % 8), the loads of step kt + 1 issued before the MFMAs of
//                step kt and parked in LDS after them: two stages of 2 x 128 rows, ONE barrier per k-step.  Rows are
//                padded to 144 bytes: the 16 lanes of an operand read (rows s .. s + 15, one slot) start at banks
//                36 s mod 64 = 16 distinct multiples of 4, so a ds_read_b128 wave read is conflict-free.
//   edges        rows past the tile and columns past N are clamped when loaded and masked when stored; pieces at or
//                past K are zero in both operands.
//
// sum (moe_sum_kernel): out[t] = round(scale * sum_j y[t k + j]) in slot order, 8 columns per thread; slots whose id
//   is outside [0, E) are skipped (their y rows were never written).  Reads y only, so out may alias x.
//
// 32-bit lane offsets from a 64-bit wave-uniform base inside one expert's matrix: 2 I * H * 2 < 2^32.  Activation
// rows (gathered x, act, y) are addressed by 64-bit per-lane row pointers: no limit on T * ldx.  T * k < 2^31.
#include "common.h"

#include <math.h>

namespace {

struct MoeArgs {
  const uint8_t* x;          // [T, H] rows ldx
  const uint8_t* w13;        // [E, 2I, H]
  const uint8_t* w2;         // [E, H, I]
  const float* topk_weights; // [T*k]
  const int32_t* topk_ids;   // [T*k]
  uint8_t* out;              // [T, H] rows ldo
  int32_t* sorted_ids;       // workspace: [T*k]
  int32_t* expert_indptr;    // workspace: [E+1]
  int32_t* tiles;            // workspace: [max_tiles][3], then n_tiles
  int32_t* n_tiles;
  uint8_t* act;              // workspace: [T*k, I]
  uint8_t* y;                // workspace: [T*k, H]
  int T, E, k, H, I, P;      // P = T * k
  int bm;                    // rows per tile: 16 or 128
  int64_t ldx, ldo;          // elements
  float scale;
};

constexpr int kTileBM = 128, kTileBN = 128, kTileStep = 64;
constexpr int kPitch = kTileStep * 2 + 16;                // bytes per LDS row
constexpr int kOperand = kTileBM * kPitch;                // one operand of one stage
constexpr int kTileLds = 4 * kOperand;                    // 2 stages x 2 operands = 72 KiB

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// ---------------------------------------------------------------------------------------------------- router
template <typename G>
__global__ __launch_bounds__(256) void moe_topk_softmax_kernel(const G* __restrict__ gating, float* __restrict__ weights,
                                                               int32_t* __restrict__ ids, int T, int E, int k,
                                                               int64_t ldg, int renormalize) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const G* row = gating + (int64_t)t * ldg;
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + 64 * i;
    v[i] = e < E ? (float)row[e] : -INFINITY;
  }
  const float mx = wave_max(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = lane + 64 * i < E ? expf(v[i] - mx) : 0.f;
    s += v[i];
  }
  s = wave_sum(s);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = lane + 64 * i < E ? v[i] / s : -1.f;   // -1: not a candidate (p >= 0)

  float my_w = 0.f, picked = 0.f;
  int my_id = 0;
  for (int r = 0; r < k; ++r) {
    float bv = v[0];
    int bi = lane;
#pragma unroll
    for (int i = 1; i < 4; ++i)
      if (v[i] > bv) {   // strict: the lower index of the lane's own four wins a tie
        bv = v[i];
        bi = lane + 64 * i;
      }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(bv, m);
      const int oi = __shfl_xor(bi, m);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (bi == lane + 64 * i) v[i] = -1.f;
    if (lane == r) {
      my_w = bv;
      my_id = bi;
    }
    picked += bv;   // the same sequence of adds in every lane
  }
  if (lane < k) {
    weights[(int64_t)t * k + lane] = renormalize ? my_w / picked : my_w;
    ids[(int64_t)t * k + lane] = my_id;
  }
}

// ---------------------------------------------------------------------------------------------------- align
__global__ __launch_bounds__(256) void moe_align_kernel(const MoeArgs p) {
  __shared__ int count[256], cursor[256];
  const int t = threadIdx.x;
  count[t] = 0;
  __syncthreads();
  for (int i = t; i < p.P; i += 256) {
    const int e = p.topk_ids[i];
    if (e >= 0 && e < p.E) atomicAdd(&count[e], 1);
  }
  __syncthreads();
  if (t < p.E) {
    int row0 = 0, tile0 = 0;
    for (int e = 0; e < t; ++e) {
      row0 += count[e];
      tile0 += (count[e] + p.bm - 1) / p.bm;
    }
    const int n = count[t];
    cursor[t] = row0;
    p.expert_indptr[t] = row0;
    for (int r = 0; r < n; r += p.bm, ++tile0) {
      p.tiles[3 * tile0] = t;
      p.tiles[3 * tile0 + 1] = row0 + r;
      p.tiles[3 * tile0 + 2] = min(p.bm, n - r);
    }
    if (t == p.E - 1) {
      p.expert_indptr[p.E] = row0 + n;
      *p.n_tiles = tile0;
    }
  }
  __syncthreads();
  for (int i = t; i < p.P; i += 256) {
    const int e = p.topk_ids[i];
    if (e >= 0 && e < p.E) p.sorted_ids[atomicAdd(&cursor[e], 1)] = i;
  }
}

// ---------------------------------------------------------------------------------------------------- epilogues
// 4 consecutive columns n ..+4 of sorted row r (pair `pair`).  GATEUP: act[r, n] = round(silu(round(g)) * round(u));
// else y[pair, n] = round(acc * topk_weights[pair]).
template <typename T, bool GATEUP>
__device__ __forceinline__ void store_epilogue(const MoeArgs& p, const f32x4& a, const f32x4& u, int r, int pair, float wgt,
                                               int n) {
  f32x4 v;
  if constexpr (GATEUP) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = silu_f32(round_to<T>(a[i])) * round_to<T>(u[i]);
    *(uint2*)(p.act + ((int64_t)r * p.I + n) * 2) = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = a[i] * wgt;
    *(uint2*)(p.y + ((int64_t)pair * p.H + n) * 2) = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
  }
}

// ---------------------------------------------------------------------------------------------------- rows16 form
template <typename T, int CT, int KU> struct Frags16 {
  typename Elem<T>::vec8 x[KU][2], w[CT][KU][2];
};

// fragments of the KU chunks at k0.  xrow: the lane's activation row, lane group included; wo: byte offsets of the
// lane's weight rows, lane group included.  Lane groups at or past K hold zeros and load nothing.
template <typename T, int CT, int KU>
__device__ __forceinline__ void load_frags16(Frags16<T, CT, KU>& f, const uint8_t* xrow, const uint8_t* wb,
                                             const uint32_t (&wo)[CT], int k0, int K, int g) {
  typedef typename Elem<T>::vec8 V;
#pragma unroll
  for (int u = 0; u < KU; ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kk = k0 + u * 64 + h * 8;   // + 16 g: the lane's own k
      const bool ok = kk + g * 16 < K;      // K % 16 == 0: a lane group is all inside or all outside
      const V zero = {};
      f.x[u][h] = zero;
      if (ok) f.x[u][h] = *(const V*)(xrow + (uint32_t)kk * 2u);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f.w[ct][u][h] = zero;
        if (ok) f.w[ct][u][h] = *(const V*)(wb + wo[ct] + (uint32_t)kk * 2u);
      }
    }
}

template <typename T, int CT, int KU>
__device__ __forceinline__ void mma_frags16(f32x4 (&acc)[CT], const Frags16<T, CT, KU>& f) {
#pragma unroll
  for (int u = 0; u < KU; ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[ct] = Elem<T>::mfma16(f.w[ct][u][h], f.x[u][h], acc[ct]);
}

template <typename T, bool GATEUP>
__global__ __launch_bounds__(256) void moe_rows16_kernel(const MoeArgs p) {
  constexpr int CT = GATEUP ? 2 : 1, KU = 4 / CT, STEP = KU * 64;
  const int tile = blockIdx.x;
  if (tile >= *p.n_tiles) return;
  const int e = p.tiles[3 * tile], r0 = p.tiles[3 * tile + 1], cnt = p.tiles[3 * tile + 2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
  const int N = GATEUP ? p.I : p.H, K = GATEUP ? p.H : p.I;
  const int n0 = (blockIdx.y * 4 + wave) * 16;
  if (n0 >= N) return;                           // N % 16 == 0: a wave's 16 columns are all inside or all outside

  const int r = r0 + min(s, cnt - 1);            // rows past the tile: clamped here, masked at the store
  const int pair = p.sorted_ids[r];
  const uint8_t* xrow = (GATEUP ? p.x + (int64_t)(pair / p.k) * p.ldx * 2 : p.act + (int64_t)r * p.I * 2) + g * 32;
  const uint8_t* wb = GATEUP ? p.w13 + (int64_t)e * 2 * p.I * p.H * 2 : p.w2 + (int64_t)e * p.H * p.I * 2;
  uint32_t wo[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) wo[ct] = (uint32_t)(ct * p.I + n0 + s) * (uint32_t)K * 2u + (uint32_t)g * 32u;

  f32x4 acc[CT] = {};
  Frags16<T, CT, KU> fa, fb;
  load_frags16<T, CT, KU>(fa, xrow, wb, wo, 0, K, g);
  for (int k0 = 0;;) {
    load_frags16<T, CT, KU>(fb, xrow, wb, wo, k0 + STEP, K, g);   // past K: all zero, no load
    mma_frags16<T, CT, KU>(acc, fa);
    k0 += STEP;
    if (k0 >= K) break;
    load_frags16<T, CT, KU>(fa, xrow, wb, wo, k0 + STEP, K, g);
    mma_frags16<T, CT, KU>(acc, fb);
    k0 += STEP;
    if (k0 >= K) break;
  }
  if (s >= cnt) return;
  const float wgt = GATEUP ? 0.f : p.topk_weights[pair];
  store_epilogue<T, GATEUP>(p, acc[0], acc[CT - 1], r, pair, wgt, n0 + g * 4);
}

// ---------------------------------------------------------------------------------------------------- tile form
template <typename T, bool GATEUP>
__global__ __launch_bounds__(256) void moe_tile_kernel(const MoeArgs p) {
  typedef typename Elem<T>::vec8 V;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tile = blockIdx.x;
  if (tile >= *p.n_tiles) return;                 // (uniform over the workgroup, as every exit before the barriers)
  const int e = p.tiles[3 * tile], r0 = p.tiles[3 * tile + 1], cnt = p.tiles[3 * tile + 2];
  const int N = GATEUP ? p.I : p.H, K = GATEUP ? p.H : p.I;
  const int n0 = blockIdx.y * (GATEUP ? kTileBN / 2 : kTileBN);
  if (n0 >= N) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;

  // staging: piece q = threadIdx.x + 256 i is row q / 8, 16-byte slot q % 8 of either operand
  const uint8_t* wb = GATEUP ? p.w13 + (int64_t)e * 2 * p.I * p.H * 2 : p.w2 + (int64_t)e * p.H * p.I * 2;
  const uint8_t* asrc[4];
  uint32_t woff[4], dst[4];
  const int slot = threadIdx.x & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (threadIdx.x >> 3) + 32 * i;
    const int r = r0 + min(row, cnt - 1);
    asrc[i] = (GATEUP ? p.x + (int64_t)(p.sorted_ids[r] / p.k) * p.ldx * 2 : p.act + (int64_t)r * p.I * 2) + slot * 16;
    int wrow;
    if constexpr (GATEUP) wrow = (row < 64 ? 0 : p.I) + min(n0 + (row & 63), p.I - 1);
    else wrow = min(n0 + row, p.H - 1);
    woff[i] = (uint32_t)wrow * (uint32_t)K * 2u + (uint32_t)slot * 16u;
    dst[i] = (uint32_t)row * kPitch + (uint32_t)slot * 16u;
  }
  uint4 ra[4], rw[4];
  auto fetch = [&](int kt) __attribute__((always_inline)) {
    const bool ok = kt * kTileStep + slot * 8 < K;   // K % 8 == 0: a piece is all inside or all outside
    const uint32_t kb = (uint32_t)kt * (kTileStep * 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = make_uint4(0, 0, 0, 0);
      rw[i] = make_uint4(0, 0, 0, 0);
      if (ok) {
        ra[i] = *(const uint4*)(asrc[i] + kb);
        rw[i] = *(const uint4*)(wb + woff[i] + kb);
      }
    }
  };
  auto park = [&](int stage) __attribute__((always_inline)) {
    char* base = smem + stage * 2 * kOperand;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(uint4*)(base + dst[i]) = ra[i];
      *(uint4*)(base + kOperand + dst[i]) = rw[i];
    }
  };

  // weight rows of this wave's column tile j inside the staged block: gate_up j = 0, 1 gate, j = 2, 3 the matching up
  int brow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) brow[j] = GATEUP ? (j >> 1) * 64 + wn * 32 + (j & 1) * 16 : wn * 64 + j * 16;
  const int ncols = GATEUP ? 32 : 64;              // output columns of a wave
  const bool active = wm * 64 < cnt && n0 + wn * ncols < N;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (K + kTileStep - 1) / kTileStep;
  fetch(0);
  park(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) fetch(kt + 1);
    if (active) {
      const char* ab = smem + (kt & 1) * 2 * kOperand + (wm * 64 + s) * kPitch + g * 32;
      const char* bb = smem + (kt & 1) * 2 * kOperand + kOperand + s * kPitch + g * 32;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        V xf[4], wf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[i] = *(const V*)(ab + i * 16 * kPitch + h * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) wf[j] = *(const V*)(bb + brow[j] * kPitch + h * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = Elem<T>::mfma16(wf[j], xf[i], acc[i][j]);
      }
    }
    if (kt + 1 < nk) park((kt + 1) & 1);   // the other stage: last read before the barrier that ended step kt - 1
    __syncthreads();
  }
  if (!active) return;

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = wm * 64 + i * 16 + s;
    if (row >= cnt) continue;
    const int r = r0 + row;
    const int pair = p.sorted_ids[r];
    const float wgt = GATEUP ? 0.f : p.topk_weights[pair];
#pragma unroll
    for (int j = 0; j < (GATEUP ? 2 : 4); ++j) {
      const int n = n0 + wn * ncols + j * 16 + g * 4;
      if (n < N) store_epilogue<T, GATEUP>(p, acc[i][j], acc[i][GATEUP ? j + 2 : j], r, pair, wgt, n);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- sum
template <typename T>
__global__ __launch_bounds__(256) void moe_sum_kernel(const MoeArgs p) {
  const int vpr = p.H / 8;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)p.T * vpr) return;
  const int t = (int)(gid / vpr), c = (int)(gid % vpr) * 8;
  float sum[8] = {};
  for (int j = 0; j < p.k; ++j) {
    const int64_t pair = (int64_t)t * p.k + j;
    const int e = p.topk_ids[pair];
    if (e < 0 || e >= p.E) continue;
    const uint4 v = *(const uint4*)(p.y + (pair * p.H + c) * 2);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sum[2 * i] += Elem<T>::lo(w[i]);
      sum[2 * i + 1] += Elem<T>::hi(w[i]);
    }
  }
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = pack2<T>(sum[2 * i] * p.scale, sum[2 * i + 1] * p.scale);
  *(uint4*)(p.out + ((int64_t)t * p.ldo + c) * 2) = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------------------- host
int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// workspace layout (every part 16-byte aligned); the tile list is sized for the smaller BM, so both forms fit
struct Layout {
  int64_t sorted, indptr, tiles, act, y, total, max_tiles16;
};
Layout layout(int64_t T, int64_t E, int64_t k, int64_t H, int64_t I) {
  Layout l;
  const int64_t P = T * k;
  l.max_tiles16 = cdiv64(P, 16) + E;
  l.sorted = 0;
  l.indptr = l.sorted + align16(P * 4);
  l.tiles = l.indptr + align16((E + 1) * 4);
  l.act = l.tiles + align16((l.max_tiles16 * 3 + 1) * 4);
  l.y = l.act + align16(P * I * 2);
  l.total = l.y + align16(P * H * 2);
  return l;
}

const char* shape_refusal(int64_t T, int64_t E, int64_t k, int64_t H, int64_t I) {
  if (H % 64 != 0) return "H must be a multiple of 64";
  if (I % 16 != 0) return "I must be a multiple of 16";
  if (E > 256) return "E must be at most 256";
  if (k > 8) return "k must be at most 8";
  if ((uint64_t)2 * I * H * 2 >= (1ull << 32)) return "one expert's w13 spans 4 GiB or more (32-bit lane offsets)";
  if (T * k >= (1ll << 31) - 256) return "T * k too large";
  if (cdiv64(I, 64) > 65535 || cdiv64(H, 64) > 65535) return "H or I too large for the grid";
  return nullptr;
}

template <typename T> void launch_experts(const MoeArgs& p, bool tile_form, hipStream_t st) {
  moe_align_kernel<<<1, 256, 0, st>>>(p);
  const unsigned tiles = (unsigned)(cdiv64(p.P, p.bm) + p.E);
  if (tile_form) {
    moe_tile_kernel<T, true><<<dim3(tiles, (unsigned)cdiv64(p.I, kTileBN / 2)), 256, kTileLds, st>>>(p);
    moe_tile_kernel<T, false><<<dim3(tiles, (unsigned)cdiv64(p.H, kTileBN)), 256, kTileLds, st>>>(p);
  } else {
    moe_rows16_kernel<T, true><<<dim3(tiles, (unsigned)cdiv64(p.I, 64)), 256, 0, st>>>(p);
    moe_rows16_kernel<T, false><<<dim3(tiles, (unsigned)cdiv64(p.H, 64)), 256, 0, st>>>(p);
  }
  moe_sum_kernel<T><<<(unsigned)cdiv64((int64_t)p.T * (p.H / 8), 256), 256, 0, st>>>(p);
}

template <typename G>
void launch_router(const void* gating, float* w, int32_t* ids, int64_t T, int64_t E, int64_t k, int64_t ldg, int renorm,
                   hipStream_t st) {
  moe_topk_softmax_kernel<G><<<(unsigned)cdiv64(T, 4), 256, 0, st>>>((const G*)gating, w, ids, (int)T, (int)E, (int)k, ldg,
                                                                    renorm);
}

}  // namespace

extern "C" int mi_moe_topk_softmax(const void* gating, float* topk_weights, int32_t* topk_ids, int64_t T, int64_t E,
                                   int64_t k, int64_t ldg, int renormalize, int gating_dtype, void* stream) {
  MI_CHECK_ARG(T >= 0 && E >= 1 && k >= 1 && ldg >= E);
  MI_CHECK_ARG(gating_dtype == MI_BF16 || gating_dtype == MI_FP16 || gating_dtype == MI_F32);
  if (E > 256 || k > 8 || k > E)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_moe_topk_softmax: needs E <= 256 and k <= min(E, 8) (got E %lld k %lld)", (long long)E,
            (long long)k);
  if (T > 0x7fffffff) MI_FAIL(MI_ERR_UNSUPPORTED, "mi_moe_topk_softmax: T too large");
  if (T == 0) return MI_OK;
  MI_CHECK_ARG(gating && topk_weights && topk_ids);
  hipStream_t st = (hipStream_t)stream;
  if (gating_dtype == MI_F32) launch_router<float>(gating, topk_weights, topk_ids, T, E, k, ldg, renormalize, st);
  else if (gating_dtype == MI_BF16) launch_router<bf16_t>(gating, topk_weights, topk_ids, T, E, k, ldg, renormalize, st);
  else launch_router<f16_t>(gating, topk_weights, topk_ids, T, E, k, ldg, renormalize, st);
  MI_CHECK_LAUNCH();
  return MI_OK;
}

extern "C" int64_t mi_moe_workspace_bytes(int64_t T, int64_t E, int64_t k, int64_t H, int64_t I) {
  if (T < 0 || E < 1 || k < 1 || H < 1 || I < 1 || shape_refusal(T, E, k, H, I)) return -1;
  return layout(T, E, k, H, I).total;
}

extern "C" int mi_moe_fused_experts(const void* x, const void* w13, const void* w2, const float* topk_weights,
                                    const int32_t* topk_ids, void* out, void* workspace, int64_t workspace_bytes,
                                    int64_t T, int64_t E, int64_t k, int64_t H, int64_t I, int64_t ldx, int64_t ldo,
                                    float routed_scaling, int form, int dtype, void* stream) {
  MI_CHECK_ARG(T >= 0 && E >= 1 && k >= 1 && H >= 1 && I >= 1 && form >= 0 && form <= 2);
  if (dtype != MI_BF16 && dtype != MI_FP16) MI_FAIL(MI_ERR_UNSUPPORTED, "mi_moe_fused_experts: dtype must be MI_BF16 or MI_FP16");
  if (const char* why = shape_refusal(T, E, k, H, I))
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_moe_fused_experts: %s (T %lld E %lld k %lld H %lld I %lld)", why, (long long)T,
            (long long)E, (long long)k, (long long)H, (long long)I);
  if (T == 0) return MI_OK;
  MI_CHECK_ARG(x && w13 && w2 && topk_weights && topk_ids && out && workspace);
  MI_CHECK_ARG(ldx >= H && ldo >= H);
  if (ldx % 8 != 0 || ldo % 8 != 0 ||
      (((uintptr_t)x | (uintptr_t)w13 | (uintptr_t)w2 | (uintptr_t)out | (uintptr_t)workspace) & 15) != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_moe_fused_experts: operands must be 16-byte aligned, ldx and ldo multiples of 8");
  const Layout l = layout(T, E, k, H, I);
  if (workspace_bytes < l.total)
    MI_FAIL(MI_ERR_INVALID, "mi_moe_fused_experts: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
            (long long)l.total);

  // the form follows T, k and E only: a captured launch stays valid whatever the ids become
  const bool tile_form = form == 2 || (form == 0 && T * k >= (int64_t)mi_tune("MI_MOE_TILE_MIN_ROWS_PER_EXPERT", kMoeTileMinRowsPerExpert) * E);
  MoeArgs p = {};
  uint8_t* ws = (uint8_t*)workspace;
  p.x = (const uint8_t*)x; p.w13 = (const uint8_t*)w13; p.w2 = (const uint8_t*)w2;
  p.topk_weights = topk_weights; p.topk_ids = topk_ids; p.out = (uint8_t*)out;
  p.sorted_ids = (int32_t*)(ws + l.sorted); p.expert_indptr = (int32_t*)(ws + l.indptr);
  p.tiles = (int32_t*)(ws + l.tiles); p.n_tiles = p.tiles + l.max_tiles16 * 3;
  p.act = ws + l.act; p.y = ws + l.y;
  p.T = (int)T; p.E = (int)E; p.k = (int)k; p.H = (int)H; p.I = (int)I; p.P = (int)(T * k);
  p.bm = tile_form ? kTileBM : 16;
  p.ldx = ldx; p.ldo = ldo; p.scale = routed_scaling;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MI_BF16) launch_experts<bf16_t>(p, tile_form, st);
  else launch_experts<f16_t>(p, tile_form, st);
  MI_CHECK_LAUNCH();
  return MI_OK;
}
