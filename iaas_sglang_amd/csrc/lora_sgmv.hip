// Multi-LoRA segmented GEMMs: shrink (x . A^T, thin N, long K) and expand (out += s * y . B^T, tiny K, wide N), bf16 /
// fp16 with fp32 accumulation.  A batch is `bs` segments of rows; segment b uses adapter weight_indices[b] at rank
// lora_ranks[adapter].  Everything per batch except bs and max_len is read from device memory by the kernels, so a
// captured launch follows batch info rewritten in place.  Every kernel reads seg_indptr / weight_indices / lora_ranks
// defensively: a segment outside [0, S], an adapter outside [0, num_lora) or a rank <= 0 makes its workgroups exit.
//
//   MFMA         v_mfma_f32_16x16x32_{bf16,f16} everywhere, weights as the A operand and activations as B: a lane ends
//                with 4 consecutive output columns of ONE row (row = lane & 15, columns 4 (lane >> 4) ..+4), so stores
//                and the expand's read-modify-write are 8-byte vectors.  Rows past a segment and columns past a rank
//                are CLAMPED to a valid row / column when loaded (an MFMA output depends on its own A row and B column
//                only) and masked when stored; only the K tail is zero-filled.
//   k mapping    (shrink) a sum over k does not care which lane holds which k, so a 64-element chunk is laid out
//                as lane group g = lane >> 4 holding k0 + 16 g ..+16: 32 contiguous bytes per lane, 128 contiguous bytes
//                (one cache line) per weight row and chunk, fed to two MFMAs.
//
// shrink, decode (max_len <= 16): bound by streaming stack_num * rank * K weight elements per segment.
//   work split   workgroup = (segment, 16 output columns); its 4 waves split K: wave w takes the 256-element steps
//                w, w + 4, ...  Fragments go global -> registers (two steps in flight per wave), no LDS in the loop.
//   reduction    each wave parks its 16 x 16 fp32 tile in LDS; after one barrier thread t sums element t of the four
//                tiles in wave order 0..3 and rounds once.  One launch, no atomics, bit-reproducible.
// shrink, prefill (max_len > 16): a workgroup owns 64 rows x up to 256 columns (all of stack_num * rank <= 256; wider N
//   runs as passes of 256 columns on grid.y) in accumulator registers, so x comes from HBM once per row block.
//   work split   nt = 16-column tiles of this segment's width; the waves form a WR x WC grid with WC = 1 (nt <= 4),
//                2 (nt <= 8) or 4 and WR = 4 / WC: a wave owns 16 WC rows x up to 4 tiles.  Narrow adapters split the
//                rows, wide ones the columns; the x lines a row block's waves share meet in L1 / L2.
// expand: workgroup = (segment, 16-row block, 64 TPW columns of one slice), grid.z = slice.  The 16 x rank x fragment
//   stays in registers for all tiles of a wave; weight rows [n, 0..rank) are 16-byte lane loads straight into the A
//   operand; no LDS.  TPW = 4 tiles per wave up to r_max 64, 2 above.  Ranks that are no multiple of 8 take
//   element-wise masked loads (the slice offset j * rank is then unaligned).  K steps at or past the rank are skipped,
//   the partial step is zero-filled in BOTH operands: nothing beyond the rank enters a sum, whatever the buffers hold.
//
// 32-bit lane offsets from a 64-bit wave-uniform base.  shrink: N * K * 2 < 2^32 (one adapter's matrix),
// 64 * ldx * 2 < 2^32 and 64 * ldo * 2 < 2^32 (one row block).  expand: N_out * R * 2 < 2^32, 16 * ldx * 2 < 2^32,
// 16 * ldo * 2 < 2^32.  No allocation, no memset, no synchronisation: capturable.
#include "common.h"

namespace {

struct LoraArgs {
  const uint8_t* x;
  const uint8_t* w;
  uint8_t* out;
  const int32_t* seg_indptr;
  const int32_t* weight_indices;
  const void* ranks;
  const float* scalings;   // expand only
  const int32_t* n_offs;   // expand only, nullable
  int ranks_is_i64;
  int S, N, K;             // shrink: N = stack_num * r_max, K = input dim.  expand: N = N_out, K = R
  int stack_num, num_lora, num_slices, slice_width;
  int64_t ldx, ldo;        // elements
  int row_blocks;          // row blocks per segment on grid.x
};

struct Segment {
  int row0, len, adapter, rank;
};

// wave-uniform; false: this segment has nothing to do (or its batch info is out of range)
__device__ __forceinline__ bool load_segment(const LoraArgs& p, int b, Segment& sg) {
  const int p0 = p.seg_indptr[b], p1 = p.seg_indptr[b + 1];
  const int a = p.weight_indices[b];
  if (p0 < 0 || p1 > p.S || p1 <= p0 || a < 0 || a >= p.num_lora) return false;
  const int64_t r = p.ranks_is_i64 ? ((const int64_t*)p.ranks)[a] : (int64_t)((const int32_t*)p.ranks)[a];
  if (r <= 0) return false;
  sg.row0 = p0;
  sg.len = p1 - p0;
  sg.adapter = a;
  sg.rank = (int)min(r, (int64_t)1 << 20);
  return true;
}

// fp32 -> T, the fp32 value materialised first (see round_to in common.h)
template <typename T> __device__ __forceinline__ T cvt_once(float v) {
  asm volatile("" : "+v"(v));
  return (T)v;
}

// 4 consecutive columns n.. of one row of a T matrix; `vec`: all 4 exist and the address is 8-byte aligned
template <typename T> __device__ __forceinline__ void store4(T* o, const f32x4& v, int n, int n_end, bool vec) {
  if (vec) {
    *(uint2*)o = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (n + i < n_end) o[i] = cvt_once<T>(v[i]);
  }
}

// ---------------------------------------------------------------------------------------------------- shrink
constexpr int kChunk = 64;   // k elements per chunk: lane group g holds k0 + 16 g ..+16, as two MFMA operands

template <typename T, int RT, int CT, int KU> struct Frags {
  typename Elem<T>::vec8 x[RT][KU][2], w[CT][KU][2];
};

// fragments of the KU chunks at k0.  xo / wo: byte offset of the lane's (clamped) row, lane group included.
template <typename T, int RT, int CT, int KU>
__device__ __forceinline__ void load_frags(Frags<T, RT, CT, KU>& f, const uint8_t* xb, const uint32_t (&xo)[RT],
                                           const uint8_t* wb, const uint32_t (&wo)[CT], int nct, int k0, int K, int g) {
  typedef typename Elem<T>::vec8 V;
#pragma unroll
  for (int u = 0; u < KU; ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kk = k0 + u * kChunk + h * 8;        // + 16 g: the lane's own k
      const bool ok = kk + g * 16 < K;               // K % 8 == 0: a vector is all inside or all outside
      const V zero = {};
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        f.x[rt][u][h] = zero;
        if (ok) f.x[rt][u][h] = *(const V*)(xb + xo[rt] + (uint32_t)kk * 2u);
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        f.w[ct][u][h] = zero;
        if (ok && ct < nct) f.w[ct][u][h] = *(const V*)(wb + wo[ct] + (uint32_t)kk * 2u);
      }
    }
}

template <typename T, int RT, int CT, int KU>
__device__ __forceinline__ void mma_frags(f32x4 (&acc)[RT][CT], const Frags<T, RT, CT, KU>& f, int nct) {
#pragma unroll
  for (int u = 0; u < KU; ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        if (ct < nct) {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = Elem<T>::mfma16(f.w[ct][u][h], f.x[rt][u][h], acc[rt][ct]);
        }
}

// acc[rt][ct] += W tile ct . x tile rt over the steps kbeg, kbeg + kstride, ... < K; two steps in flight
template <typename T, int RT, int CT, int KU>
__device__ __forceinline__ void accumulate(f32x4 (&acc)[RT][CT], const uint8_t* xb, const uint32_t (&xo)[RT],
                                           const uint8_t* wb, const uint32_t (&wo)[CT], int nct, int kbeg, int kstride,
                                           int K, int g) {
  Frags<T, RT, CT, KU> fa, fb;
  int k = kbeg;
  if (k >= K) return;
  load_frags<T, RT, CT, KU>(fa, xb, xo, wb, wo, nct, k, K, g);
  for (;;) {
    load_frags<T, RT, CT, KU>(fb, xb, xo, wb, wo, nct, k + kstride, K, g);   // past K: all zero, no load
    mma_frags<T, RT, CT, KU>(acc, fa, nct);
    k += kstride;
    if (k >= K) break;
    load_frags<T, RT, CT, KU>(fa, xb, xo, wb, wo, nct, k + kstride, K, g);
    mma_frags<T, RT, CT, KU>(acc, fb, nct);
    k += kstride;
    if (k >= K) break;
  }
}

constexpr int kDecodeKU = 4;   // a decode wave's step: 4 chunks = 256 k elements

template <typename T>
__global__ __launch_bounds__(256) void lora_shrink_decode_kernel(const LoraArgs p) {
  __shared__ float red[4][256];
  Segment sg;
  if (!load_segment(p, blockIdx.x, sg)) return;
  const int n_b = min(p.N, p.stack_num * sg.rank);
  const int c0 = blockIdx.y * 16;
  if (c0 >= n_b) return;   // (all exits above are uniform over the workgroup: the barrier below is safe)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;

  const uint8_t* xb = p.x + (int64_t)sg.row0 * p.ldx * 2;
  const uint8_t* wb = p.w + (int64_t)sg.adapter * p.N * p.K * 2;
  const uint32_t xo[1] = {(uint32_t)min(s, sg.len - 1) * (uint32_t)p.ldx * 2u + (uint32_t)g * 32u};
  const uint32_t wo[1] = {(uint32_t)min(c0 + s, n_b - 1) * (uint32_t)p.K * 2u + (uint32_t)g * 32u};
  f32x4 acc[1][1] = {};
  constexpr int step = kDecodeKU * kChunk;
  accumulate<T, 1, 1, kDecodeKU>(acc, xb, xo, wb, wo, 1, wave * step, 4 * step, p.K, g);

  *(f32x4*)&red[wave][s * 16 + g * 4] = acc[0][0];   // [row s][column 4 g ..+4]
  __syncthreads();
  const int t = threadIdx.x, row = t >> 4, col = c0 + (t & 15);
  const float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (row < sg.len && col < n_b) ((T*)p.out)[(int64_t)(sg.row0 + row) * p.ldo + col] = cvt_once<T>(v);
}

template <typename T, int WC>   // WC: waves across the columns = row tiles per wave
__device__ __forceinline__ void shrink_prefill_body(const LoraArgs& p, const Segment& sg, int r0, int c0, int n_b, int nt) {
  constexpr int RT = WC, CT = 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
  const int wr = wave / WC, wc = wave % WC;
  const int tpw = (nt + WC - 1) / WC;              // column tiles per wave, <= 4
  const int t0 = wc * tpw;
  const int nct = min(tpw, nt - t0);
  const int wrow0 = r0 + wr * RT * 16;             // first row of this wave, relative to the segment
  if (nct <= 0 || wrow0 >= sg.len) return;

  const uint8_t* xb = p.x + (int64_t)(sg.row0 + r0) * p.ldx * 2;
  const uint8_t* wb = p.w + (int64_t)sg.adapter * p.N * p.K * 2;
  uint32_t xo[RT], wo[CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    xo[rt] = (uint32_t)(min(wrow0 + rt * 16 + s, sg.len - 1) - r0) * (uint32_t)p.ldx * 2u + (uint32_t)g * 32u;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
    wo[ct] = (uint32_t)min(c0 + (t0 + ct) * 16 + s, n_b - 1) * (uint32_t)p.K * 2u + (uint32_t)g * 32u;
  f32x4 acc[RT][CT] = {};
  accumulate<T, RT, CT, 1>(acc, xb, xo, wb, wo, nct, 0, kChunk, p.K, g);

#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = wrow0 + rt * 16 + s;
    if (row >= sg.len) continue;
    T* orow = (T*)p.out + (int64_t)(sg.row0 + row) * p.ldo;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int n = c0 + (t0 + ct) * 16 + g * 4;
      if (ct < nct && n < n_b) store4<T>(orow + n, acc[rt][ct], n, n_b, n + 4 <= n_b);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void lora_shrink_prefill_kernel(const LoraArgs p) {
  Segment sg;
  if (!load_segment(p, blockIdx.x / p.row_blocks, sg)) return;
  const int r0 = (blockIdx.x % p.row_blocks) * 64;
  if (r0 >= sg.len) return;
  const int n_b = min(p.N, p.stack_num * sg.rank);
  const int c0 = blockIdx.y * 256;
  if (c0 >= n_b) return;
  const int nt = (min(256, n_b - c0) + 15) / 16;
  if (nt <= 4) shrink_prefill_body<T, 1>(p, sg, r0, c0, n_b, nt);
  else if (nt <= 8) shrink_prefill_body<T, 2>(p, sg, r0, c0, n_b, nt);
  else shrink_prefill_body<T, 4>(p, sg, r0, c0, n_b, nt);
}

// ---------------------------------------------------------------------------------------------------- expand
// 8 elements at ptr, those at index >= nvalid replaced by zero and never read; `vec`: ptr is 16-byte aligned
template <typename T>
__device__ __forceinline__ typename Elem<T>::vec8 load8_masked(const T* ptr, int nvalid, bool vec) {
  typename Elem<T>::vec8 v = {};
  if (nvalid >= 8 && vec) {
    v = *(const typename Elem<T>::vec8*)ptr;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nvalid) v[e] = ptr[e];
  }
  return v;
}

template <int KS> constexpr int expand_tiles_per_wave() { return KS <= 2 ? 4 : 2; }

template <typename T, int KS>   // KS: 32-element k steps that cover r_max
__global__ __launch_bounds__(256) void lora_expand_kernel(const LoraArgs p) {
  typedef typename Elem<T>::vec8 V;
  constexpr int TPW = expand_tiles_per_wave<KS>();
  Segment sg;
  if (!load_segment(p, blockIdx.x / p.row_blocks, sg)) return;
  const int r0 = (blockIdx.x % p.row_blocks) * 16;
  if (r0 >= sg.len) return;
  const int R = p.K, rho = min(R, sg.rank), j = blockIdx.z;
  int o0 = p.n_offs ? p.n_offs[j] : j * p.slice_width;
  int o1 = p.n_offs ? p.n_offs[j + 1] : o0 + p.slice_width;
  o0 = max(o0, 0);
  o1 = min(o1, p.N);
  const int nsz = o1 - o0;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
  const int c0 = (blockIdx.y * 4 + wave) * TPW * 16;
  if (c0 >= nsz) return;
  const float scale = p.scalings[sg.adapter];

  // the segment's x fragment: row r0 + s, slice columns j rho + 32 ks + 8 g ..+8
  const T* xp = (const T*)(p.x + (int64_t)(sg.row0 + r0) * p.ldx * 2) +
                (uint32_t)(min(r0 + s, sg.len - 1) - r0) * (uint32_t)p.ldx + (uint32_t)(j * rho + g * 8);
  const bool xvec = (rho & 7) == 0;
  V xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = load8_masked<T>(xp + ks * 32, rho - ks * 32 - g * 8, xvec);

  const T* wbase = (const T*)(p.w + (int64_t)sg.adapter * p.N * R * 2);
  T* obase = (T*)(p.out + (int64_t)(sg.row0 + r0) * p.ldo * 2);
  const bool row_ok = r0 + s < sg.len;
  const bool aligned = (o0 & 3) == 0;

  V wf[TPW][KS];
  uint2 old[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int n0 = c0 + t * 16;
    if (n0 >= nsz) break;
    const T* wp = wbase + (uint32_t)(o0 + min(n0 + s, nsz - 1)) * (uint32_t)R + (uint32_t)(g * 8);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      if (ks * 32 < rho) wf[t][ks] = load8_masked<T>(wp + ks * 32, rho - ks * 32 - g * 8, true);
    const int n = n0 + g * 4;
    if (row_ok && aligned && n + 4 <= nsz) old[t] = *(const uint2*)(obase + (uint32_t)s * (uint32_t)p.ldo + (uint32_t)(o0 + n));
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int n0 = c0 + t * 16;
    if (n0 >= nsz) break;
    f32x4 acc = {};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      if (ks * 32 < rho) acc = Elem<T>::mfma16(wf[t][ks], xf[ks], acc);
    const int n = n0 + g * 4;
    if (!row_ok || n >= nsz) continue;
    T* op = obase + (uint32_t)s * (uint32_t)p.ldo + (uint32_t)(o0 + n);
    if (aligned && n + 4 <= nsz) {
      f32x4 v;
      v[0] = round_to<T>(acc[0] * scale) + Elem<T>::lo(old[t].x);
      v[1] = round_to<T>(acc[1] * scale) + Elem<T>::hi(old[t].x);
      v[2] = round_to<T>(acc[2] * scale) + Elem<T>::lo(old[t].y);
      v[3] = round_to<T>(acc[3] * scale) + Elem<T>::hi(old[t].y);
      *(uint2*)op = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (n + i < nsz) op[i] = cvt_once<T>(round_to<T>(acc[i] * scale) + (float)op[i]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- host
int check_common(const char* fn, const void* x, const void* w, const void* out, const void* seg_indptr,
                 const void* weight_indices, const void* ranks, int64_t S, int64_t num_lora, int64_t ldx, int64_t ldo,
                 int64_t bs, int64_t max_len, int dtype) {
  if (!(S >= 0 && num_lora >= 0 && bs >= 0 && max_len >= 0 && S < (1ll << 31) && num_lora < (1ll << 31)))
    MI_FAIL(MI_ERR_INVALID, "%s: invalid argument: S / num_lora / bs / max_len out of range", fn);
  if (dtype != MI_BF16 && dtype != MI_FP16) MI_FAIL(MI_ERR_INVALID, "%s: dtype must be MI_BF16 or MI_FP16", fn);
  if (!(x && w && out && seg_indptr && weight_indices && ranks)) MI_FAIL(MI_ERR_INVALID, "%s: null pointer", fn);
  if (ldx % 8 != 0 || ldo % 8 != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "%s: ldx and ldo must be multiples of 8 (got %lld %lld)", fn, (long long)ldx, (long long)ldo);
  if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) & 15) != 0)
    MI_FAIL(MI_ERR_UNSUPPORTED, "%s: x, weights and out must be 16-byte aligned", fn);
  return MI_OK;
}

template <typename T, int KS>
void launch_expand(const LoraArgs& p, int64_t bs, int64_t max_width, hipStream_t st) {
  const dim3 grid((unsigned)(bs * p.row_blocks), (unsigned)cdiv64(max_width, 64 * expand_tiles_per_wave<KS>()),
                  (unsigned)p.num_slices);
  lora_expand_kernel<T, KS><<<grid, 256, 0, st>>>(p);
}

template <typename T> void launch_expand_ks(const LoraArgs& p, int64_t bs, int64_t max_width, hipStream_t st) {
  if (p.K <= 32) launch_expand<T, 1>(p, bs, max_width, st);
  else if (p.K <= 64) launch_expand<T, 2>(p, bs, max_width, st);
  else if (p.K <= 128) launch_expand<T, 4>(p, bs, max_width, st);
  else launch_expand<T, 8>(p, bs, max_width, st);
}

}  // namespace

extern "C" int mi_lora_shrink(const void* x, const void* weights, void* out, const int32_t* seg_indptr,
                              const int32_t* weight_indices, const void* lora_ranks, int ranks_is_i64, int64_t S,
                              int64_t N, int64_t K, int64_t stack_num, int64_t num_lora, int64_t ldx, int64_t ldo,
                              int64_t bs, int64_t max_len, int dtype, void* stream) {
  MI_CHECK_ARG(N > 0 && K > 0 && stack_num >= 1 && stack_num <= 3 && N % stack_num == 0);
  if (int rc = check_common(__func__, x, weights, out, seg_indptr, weight_indices, lora_ranks, S, num_lora, ldx, ldo, bs,
                            max_len, dtype))
    return rc;
  MI_CHECK_ARG(ldx >= K && ldo >= N);
  const int64_t r_max = N / stack_num;
  if (K % 8 != 0) MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_shrink: K must be a multiple of 8 (got %lld)", (long long)K);
  if (r_max % 8 != 0 || r_max > 256)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_shrink: r_max must be a multiple of 8, at most 256 (got %lld)", (long long)r_max);
  if (N > 1024) MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_shrink: N must be at most 1024 (got %lld)", (long long)N);
  const uint64_t lim = 1ull << 32;
  if ((uint64_t)N * (uint64_t)K * 2 >= lim || 64 * (uint64_t)ldx * 2 >= lim || 64 * (uint64_t)ldo * 2 >= lim)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_shrink: an adapter matrix or a 64-row block spans 4 GiB or more (32-bit lane offsets)");
  const bool decode = max_len <= 16;
  const int64_t row_blocks = decode ? 1 : cdiv64(max_len, 64);
  if (bs * row_blocks > 0x7fffffff) MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_shrink: bs * row blocks too large for the grid");
  if (bs == 0 || S == 0 || max_len == 0 || num_lora == 0) return MI_OK;

  LoraArgs p = {};
  p.x = (const uint8_t*)x; p.w = (const uint8_t*)weights; p.out = (uint8_t*)out;
  p.seg_indptr = seg_indptr; p.weight_indices = weight_indices; p.ranks = lora_ranks; p.ranks_is_i64 = ranks_is_i64;
  p.S = (int)S; p.N = (int)N; p.K = (int)K; p.stack_num = (int)stack_num; p.num_lora = (int)num_lora;
  p.ldx = ldx; p.ldo = ldo; p.row_blocks = (int)row_blocks;
  hipStream_t st = (hipStream_t)stream;
  if (decode) {
    const dim3 grid((unsigned)bs, (unsigned)cdiv64(N, 16));
    if (dtype == MI_BF16) lora_shrink_decode_kernel<bf16_t><<<grid, 256, 0, st>>>(p);
    else lora_shrink_decode_kernel<f16_t><<<grid, 256, 0, st>>>(p);
  } else {
    const dim3 grid((unsigned)(bs * row_blocks), (unsigned)cdiv64(N, 256));
    if (dtype == MI_BF16) lora_shrink_prefill_kernel<bf16_t><<<grid, 256, 0, st>>>(p);
    else lora_shrink_prefill_kernel<f16_t><<<grid, 256, 0, st>>>(p);
  }
  MI_CHECK_LAUNCH();
  return MI_OK;
}

extern "C" int mi_lora_expand(const void* x, const void* weights, void* out, const int32_t* seg_indptr,
                              const int32_t* weight_indices, const void* lora_ranks, int ranks_is_i64,
                              const float* scalings, const int32_t* n_offs, int64_t slice_width, int64_t num_slices,
                              int64_t S, int64_t N_out, int64_t R, int64_t num_lora, int64_t ldx, int64_t ldo,
                              int64_t bs, int64_t max_len, int dtype, void* stream) {
  MI_CHECK_ARG(N_out > 0 && R > 0 && num_slices >= 1 && num_slices <= 3 && slice_width > 0 && slice_width <= N_out);
  MI_CHECK_ARG(n_offs || num_slices * slice_width <= N_out);
  if (int rc = check_common(__func__, x, weights, out, seg_indptr, weight_indices, lora_ranks, S, num_lora, ldx, ldo, bs,
                            max_len, dtype))
    return rc;
  MI_CHECK_ARG(scalings && ldx >= num_slices * R && ldo >= N_out);
  if (R % 8 != 0 || R > 256)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_expand: r_max must be a multiple of 8, at most 256 (got %lld)", (long long)R);
  const uint64_t lim = 1ull << 32;
  if ((uint64_t)N_out * (uint64_t)R * 2 >= lim || 16 * (uint64_t)ldx * 2 >= lim || 16 * (uint64_t)ldo * 2 >= lim)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_expand: an adapter matrix or a 16-row block spans 4 GiB or more (32-bit lane offsets)");
  const int64_t row_blocks = cdiv64(max_len, 16);
  if (bs * row_blocks > 0x7fffffff || cdiv64(slice_width, 128) > 65535)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_lora_expand: bs * row blocks or the slice width too large for the grid");
  if (bs == 0 || S == 0 || max_len == 0 || num_lora == 0) return MI_OK;

  LoraArgs p = {};
  p.x = (const uint8_t*)x; p.w = (const uint8_t*)weights; p.out = (uint8_t*)out;
  p.seg_indptr = seg_indptr; p.weight_indices = weight_indices; p.ranks = lora_ranks; p.ranks_is_i64 = ranks_is_i64;
  p.scalings = scalings; p.n_offs = n_offs;
  p.S = (int)S; p.N = (int)N_out; p.K = (int)R; p.num_lora = (int)num_lora; p.num_slices = (int)num_slices;
  p.slice_width = (int)slice_width;
  p.ldx = ldx; p.ldo = ldo; p.row_blocks = (int)row_blocks;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MI_BF16) launch_expand_ks<bf16_t>(p, bs, slice_width, st);
  else launch_expand_ks<f16_t>(p, bs, slice_width, st);
  MI_CHECK_LAUNCH();
  return MI_OK;
}
