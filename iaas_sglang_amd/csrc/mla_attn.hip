// MLA (multi-head latent attention, absorbed form) over a latent KV pool -- gfx950, wave64, MFMA 16x16x32.
//
// DeepSeek-class geometry: every pool row holds kv_lora_rank 512 + qk_rope_head_dim 64 = 576 elements (1152 B) and is
// at once the KEY of every q head (all 576 dims) and its VALUE (the first 512 dims):
//   o[t,h] = softmax_j(sm_scale * q[t,h] . kv[idx_j, :576]) . kv[idx_j, :512]
// One kernel serves decode (one row per request) and plain extend (row t of request b sees the first n_t keys of the
// request; the new tokens are already in the pool).
//
// Workgroup = 4 waves = one (row t, block of 16 q heads, kv split).  All 16 rows of the block belong to ONE token, so
// the key limit n_t is uniform: only the last tile is masked.  Keys are walked in tiles of 64, double-buffered in LDS
// (2 x 64 rows x (1152 + 32) B = 148 KiB): a tile is fetched from memory ONCE per workgroup (register-staged: the rows of
// tile n+1 are requested before tile n is computed and written to the other stage after it) and read from LDS for both
// products.  Per tile:
//   S^T[key][head]   wave w: keys 16w .. 16w+15 against all 16 heads, 18 MFMA (A = K rows by ds_read_b128, B = Q
//                    fragments held in registers) -- every score is computed once, by one wave
//   softmax          C layout (lane: head = l&15, keys 4*(l>>4)+r), fp32, exp2 domain; the four waves exchange their
//                    per-head tile maxima through LDS, so all of them hold the same running max m and rescale factor
//   P                rounded to T and written to a [16 heads][64 keys] LDS tile (2 KiB)
//   O^T[d][head]     wave w: output dims 128w .. 128w+127 over all 64 keys, 16 MFMA (A = V^T by ds_read_b64_tr_b16 from
//                    the SAME LDS rows, B = P from the P tile), 32 accumulator VGPRs; every wave rescales its own slice
// Three workgroup barriers per tile (maxima, P, stage hand-over), none inside a divergent branch: every loop bound and
// every branch around a barrier depends on (t, split) only.  Tiles are never skipped per wave; rows past the end are
// masked and their loads clamped to the split's last key.
// Split-KV: the split rule, work list, device plan, workspace layout and merge kernel of decode_attn.hip.
#include "common.h"

// decode_attn.hip: decode_merge_kernel<T, 512> over [rows][heads][splits] partials; kv_indptr / plan as in mi_decode_attn
MI_INTERNAL int mi_attn_merge_splits512(const float* ws_o, const float* ws_ml, void* o, int64_t rows, int64_t num_q_heads,
                                        int64_t num_splits, int64_t stride_o_tok, const int32_t* kv_indptr,
                                        int64_t split_chunk, const int32_t* plan, int dtype, void* stream);

struct MlaParams {
  const void* q;
  const void* kv;
  void* o;
  const int32_t* qo_indptr;   // extend: [batch + 1]; nullptr = decode (row t is request t)
  const int32_t* kv_indptr;
  const int32_t* kv_indices;
  float* ws_o;    // [T][H][splits][512]
  float* ws_ml;   // [T][H][splits][2]
  const int32_t* plan;   // decode only: DEVICE {num_work, num_splits, split_chunk}, as in DecodeParams
  const int32_t* work;   // decode only: [num_work][2] = (row, split)
  int32_t batch, total_tokens, num_q_heads, num_splits, split_chunk;
  int64_t stride_q_tok, stride_o_tok, stride_kv_slot;
  float scale_log2;      // sm_scale * log2(e)
};

typedef __attribute__((ext_vector_type(4))) short mla_s16x4;
typedef __attribute__((ext_vector_type(8))) short mla_s16x8;
typedef __attribute__((address_space(3))) mla_s16x4 mla_lds_s16x4;

constexpr int MLA_DK = 576, MLA_DV = 512;
constexpr int MLA_KT = 64;                       // keys per tile
constexpr int MLA_ROW = MLA_DK * 2 + 32;         // padded LDS row (bytes): 296 dwords = 8 x odd, as the 128-dim tiles
constexpr int MLA_STAGE = MLA_KT * MLA_ROW;      // 75776 B
constexpr int MLA_PROW = MLA_KT * 2 + 8;         // P tile row (bytes), padded
constexpr int MLA_LDS = 2 * MLA_STAGE + 16 * MLA_PROW + 4 * 16 * 4;   // 153984 B of the 160 KiB

template <typename T>
__global__ __launch_bounds__(256) void mla_attn_kernel(const MlaParams p) {
  constexpr int KS = MLA_DK / 32;      // 18 MFMA k-steps over the 576 key dims
  constexpr int NST = MLA_DK / 32;     // 18 staged 16-byte pieces per thread and tile (4 threads per row)
  constexpr int ROW = MLA_ROW, STAGE = MLA_STAGE, PROW = MLA_PROW;
  typedef typename Elem<T>::vec8 vec8;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* pbuf = smem + 2 * STAGE;                    // P [16 heads][64 keys] of T
  float* wred = (float*)(pbuf + 16 * PROW);         // [4 waves][16 heads]: tile maxima, and the sums at the end

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g4 = lane >> 4, c16 = lane & 15;
  if (p.plan && (int)blockIdx.x >= p.plan[0]) return;
  const int t = p.work ? p.work[2 * blockIdx.x] : (int)blockIdx.x;
  const int s = p.work ? p.work[2 * blockIdx.x + 1] : (int)blockIdx.z;
  const int h0 = blockIdx.y * 16;
  const int H = p.num_q_heads;
  const int nsplit = p.num_splits;                       // workspace stride (the capacity when a plan is given)
  const int nsplit_eff = p.plan ? p.plan[1] : nsplit;
  const int32_t chunk_eff = p.plan ? p.plan[2] : p.split_chunk;

  // ---- request of this row and its key limit n_t (uniform for the workgroup)
  int b = t;
  int32_t n_t;
  if (p.qo_indptr) {
    int lo = 0, hi = p.batch;            // largest b with qo_indptr[b] <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (p.qo_indptr[mid] <= t) lo = mid; else hi = mid;
    }
    b = lo;
    const int32_t S = p.kv_indptr[b + 1] - p.kv_indptr[b];
    const int32_t q_end = p.qo_indptr[b + 1];
    n_t = (t < q_end) ? max(S - (q_end - 1 - t), 0) : 0;   // the last new token sees all S keys
  } else {
    n_t = p.kv_indptr[b + 1] - p.kv_indptr[b];
  }
  const int32_t base = p.kv_indptr[b];
  int32_t per = (n_t + nsplit_eff - 1) / nsplit_eff;       // the split rule of decode_attn_kernel (the merge relies on it)
  per = (per + 15) & ~15;
  per = max(per, chunk_eff);
  const int32_t start = s * per;
  const int32_t end = min(n_t, start + per);

  if (start >= end) {   // empty split or zero-length row: the whole workgroup leaves before any barrier
    if (nsplit > 1) {
      if (tid < 16 && h0 + tid < H) {
        float* ml = p.ws_ml + (((int64_t)t * H + h0 + tid) * nsplit + s) * 2;
        ml[0] = -INFINITY;
        ml[1] = 0.f;
      }
    } else {
      for (int i = tid; i < 16 * (MLA_DV / 8); i += 256) {
        const int h = h0 + i / (MLA_DV / 8);
        if (h < H) *(uint4*)((T*)p.o + (int64_t)t * p.stride_o_tok + (int64_t)h * MLA_DV + (i % (MLA_DV / 8)) * 8) = make_uint4(0, 0, 0, 0);
      }
    }
    return;
  }

  // ---- Q fragments (B operand): lane -> head h0 + c16, dims 32 ks + 8 g4 .. +7; heads past H are zeros
  vec8 qf[KS];
  {
    const bool live = h0 + c16 < H;
    const T* qp = (const T*)p.q + (int64_t)t * p.stride_q_tok + (int64_t)(live ? h0 + c16 : 0) * MLA_DK + g4 * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const u32x4 z = *(const u32x4*)(qp + ks * 32);    // head 0 for the missing heads: a valid row, then zeroed
      qf[ks] = __builtin_bit_cast(vec8, live ? z : u32x4{0, 0, 0, 0});
    }
  }

  // ---- staging: thread -> key row tid >> 2 of the tile, 16-byte pieces (tid & 3) + 4 j: four lanes read 64 contiguous
  // bytes, a wave instruction 16 rows x 64 B
  const int srow = tid >> 2, spc = tid & 3;
  const int32_t* idx = p.kv_indices + base;
  const uint32_t kstride = (uint32_t)p.stride_kv_slot;       // 0 < stride < 2^31 (host check)
  const T* kvb = (const T*)p.kv + spc * 8;
  auto slot_of = [&](int32_t tile) __attribute__((always_inline)) -> int32_t {
    return idx[min(start + tile * MLA_KT + srow, end - 1)];   // rows past the end: the split's last key (masked below)
  };
  // 18 x 16 B in flight per thread, plain unrolled loops over a register array
  u32x4 st[NST];     // (ext-vector type: an array of HIP's uint4 structs is not promoted to registers either)
#define MLA_STAGE_LOAD(slot_)                                            \
  {                                                                      \
    const T* rp_ = kvb + (uint64_t)(uint32_t)(slot_) * kstride;          \
    _Pragma("unroll") for (int j = 0; j < NST; ++j) st[j] = *(const u32x4*)(rp_ + j * 32); \
  }
#define MLA_STAGE_WRITE(stg_)                                            \
  {                                                                      \
    char* d_ = smem + (stg_) * STAGE + srow * ROW + spc * 16;            \
    _Pragma("unroll") for (int j = 0; j < NST; ++j) *(u32x4*)(d_ + j * 64) = st[j]; \
  }

  f32x4 acc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;     // per head c16; m is the same in all four waves, lsum covers this lane's keys

  const int32_t ntiles = (end - start + MLA_KT - 1) / MLA_KT;
  MLA_STAGE_LOAD(slot_of(0));
  int32_t slot_next = slot_of(1);      // indices run one tile ahead of the rows
  MLA_STAGE_WRITE(0);
  __syncthreads();

  for (int32_t tile = 0; tile < ntiles; ++tile) {
    const int stg = tile & 1;
    const char* ks_lds = smem + stg * STAGE;
    // branch-free: behind the last tile this fetches the split's last row once more (clamped, cached) and the write
    // below fills the stage nobody reads; with `if (tile + 1 < ntiles)` the staging registers went through scratch
    MLA_STAGE_LOAD(slot_next);
    slot_next = slot_of(tile + 2);

    // ---- S^T = K . Q^T for this wave's 16 keys (two accumulator chains)
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    {
      const char* kr = ks_lds + (16 * wave + c16) * ROW + g4 * 16;
#pragma unroll
      for (int ks = 0; ks < KS; ks += 2) {
        s0 = Elem<T>::mfma16(__builtin_bit_cast(vec8, *(const uint4*)(kr + ks * 64)), qf[ks], s0);
        s1 = Elem<T>::mfma16(__builtin_bit_cast(vec8, *(const uint4*)(kr + (ks + 1) * 64)), qf[ks + 1], s1);
      }
    }
    float sc[4];
    const int32_t k0 = start + tile * MLA_KT + 16 * wave + 4 * g4;   // key of sc[0]
    float tm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float x = (s0[r] + s1[r]) * p.scale_log2;
      sc[r] = (k0 + r < end) ? x : -INFINITY;
      tm = fmaxf(tm, sc[r]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 16));
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    if (g4 == 0) wred[wave * 16 + c16] = tm;
    __syncthreads();
    tm = fmaxf(fmaxf(wred[c16], wred[16 + c16]), fmaxf(wred[32 + c16], wred[48 + c16]));
    // the first key of a non-empty split is live, so the tile maximum of tile 0 -- and m from then on -- is finite
    const float mn = fmaxf(m, tm);
    const float alpha = fast_exp2(m - mn);     // m = -inf on the first tile -> 0
    m = mn;
    float pr[4], psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pr[r] = fast_exp2(sc[r] - mn);           // masked keys: exp2(-inf) = 0
      psum += pr[r];
    }
    lsum = lsum * alpha + psum;
    *(uint2*)(pbuf + c16 * PROW + (16 * wave + 4 * g4) * 2) = make_uint2(pack2<T>(pr[0], pr[1]), pack2<T>(pr[2], pr[3]));
    __syncthreads();

    // ---- O^T += V^T . P^T for this wave's 128 output dims over all 64 keys
#pragma unroll
    for (int db = 0; db < 8; ++db) acc[db] *= alpha;
    const int qq = c16 >> 2, pp = c16 & 3;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      // B operand: k-slot (g4, j): j < 4 -> key 32 sub + 4 g4 + j, j >= 4 -> key 32 sub + 16 + 4 g4 + j - 4
      const char* pr0 = pbuf + c16 * PROW + (32 * sub + 4 * g4) * 2;
      const uint2 plo = *(const uint2*)pr0, phi = *(const uint2*)(pr0 + 32);
      const vec8 pf = __builtin_bit_cast(vec8, make_uint4(plo.x, plo.y, phi.x, phi.y));
      const char* vr0 = ks_lds + (32 * sub + 4 * g4 + qq) * ROW + pp * 8 + wave * 256;
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        const mla_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mla_lds_s16x4*)(vr0 + db * 32));
        const mla_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mla_lds_s16x4*)(vr0 + 16 * ROW + db * 32));
        const mla_s16x8 both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        acc[db] = Elem<T>::mfma16(__builtin_bit_cast(vec8, both), pf, acc[db]);
      }
    }
    // the other stage was last read in the previous iteration (every wave is past that iteration's last barrier)
    MLA_STAGE_WRITE(stg ^ 1);
    __syncthreads();
  }

  // ---- sums: the 4 lane rows of a wave, then the 4 waves
  lsum += __shfl_xor(lsum, 16);
  lsum += __shfl_xor(lsum, 32);
  if (g4 == 0) wred[wave * 16 + c16] = lsum;
  __syncthreads();
  const float l = (wred[c16] + wred[16 + c16]) + (wred[32 + c16] + wred[48 + c16]);

  // ---- epilogue: lane holds O[head h0 + c16][d = 128 wave + 16 db + 4 g4 + r]
  const int h = h0 + c16;
  if (h >= H) return;
  const int d0 = 128 * wave + 4 * g4;
  if (nsplit == 1) {
    const float inv = 1.f / l;
    T* op = (T*)p.o + (int64_t)t * p.stride_o_tok + (int64_t)h * MLA_DV + d0;
#pragma unroll
    for (int db = 0; db < 8; ++db)
      *(uint2*)(op + db * 16) = make_uint2(pack2<T>(acc[db][0] * inv, acc[db][1] * inv),
                                           pack2<T>(acc[db][2] * inv, acc[db][3] * inv));
  } else {
    const int64_t slot = ((int64_t)t * H + h) * nsplit + s;
    float* wo = p.ws_o + slot * MLA_DV + d0;
#pragma unroll
    for (int db = 0; db < 8; ++db) *(f32x4*)(wo + db * 16) = acc[db];
    if (wave == 0 && g4 == 0) {
      p.ws_ml[slot * 2] = m;
      p.ws_ml[slot * 2 + 1] = l;
    }
  }
}

#undef MLA_STAGE_LOAD
#undef MLA_STAGE_WRITE

// ---------------------------------------------------------------------------- host side
extern "C" int mi_mla_attn(const void* q, const void* kv_buf, void* o, const int32_t* qo_indptr,
                           const int32_t* kv_indptr, const int32_t* kv_indices, void* workspace, int64_t batch,
                           int64_t total_tokens, int64_t num_q_heads, int64_t qk_head_dim, int64_t v_head_dim,
                           int64_t stride_q_tok, int64_t stride_o_tok, int64_t stride_kv_slot, float sm_scale,
                           int64_t num_splits, int64_t split_chunk, const int32_t* work, int64_t num_work,
                           const int32_t* plan, int dtype, void* stream) {
  if (qk_head_dim != MLA_DK || v_head_dim != MLA_DV)
    MI_FAIL(MI_ERR_UNSUPPORTED, "mi_mla_attn: latent geometry %lld -> %lld not supported (576 -> 512)",
            (long long)qk_head_dim, (long long)v_head_dim);
  if (dtype != MI_BF16 && dtype != MI_FP16) MI_FAIL(MI_ERR_UNSUPPORTED, "mi_mla_attn: dtype %d not supported (bf16 / fp16)", dtype);
  MI_CHECK_ARG(batch >= 0 && total_tokens >= 0);
  if (batch == 0 || total_tokens == 0) return MI_OK;
  MI_CHECK_ARG(q && kv_buf && o && kv_indptr && kv_indices);
  MI_CHECK_ARG(qo_indptr || total_tokens == batch);          // decode: one row per request
  MI_CHECK_ARG(num_q_heads > 0 && num_q_heads <= 16 * 65535);
  MI_CHECK_ARG(num_splits >= 1 && num_splits <= 65535 && batch <= 0x7fffffff && total_tokens <= 0x7fffffff);
  MI_CHECK_ARG(num_splits == 1 || workspace != nullptr);
  MI_CHECK_ARG(split_chunk >= 0 && split_chunk % 16 == 0 && split_chunk < (1 << 30));
  MI_CHECK_ARG(stride_q_tok % 8 == 0 && stride_o_tok % 8 == 0 && stride_kv_slot % 8 == 0);   // 16-byte row accesses
  MI_CHECK_ARG(stride_kv_slot > 0 && stride_kv_slot < (1ll << 31));
  MI_CHECK_ARG((((uintptr_t)q | (uintptr_t)kv_buf | (uintptr_t)o | (uintptr_t)workspace) & 15) == 0);
  // the work list and the plan name rows by request: decode only (the merge derives the live splits from kv_indptr[row])
  MI_CHECK_ARG(!work || (!qo_indptr && num_work > 0 && num_work <= 0x7fffffff && num_splits > 1 && (split_chunk > 0 || plan)));
  MI_CHECK_ARG(!plan || work);

  MlaParams p;
  p.q = q; p.kv = kv_buf; p.o = o;
  p.qo_indptr = qo_indptr; p.kv_indptr = kv_indptr; p.kv_indices = kv_indices;
  p.ws_o = num_splits > 1 ? (float*)workspace : nullptr;
  p.ws_ml = p.ws_o ? p.ws_o + total_tokens * num_q_heads * num_splits * MLA_DV : nullptr;
  p.plan = plan; p.work = work;
  p.batch = (int32_t)batch; p.total_tokens = (int32_t)total_tokens; p.num_q_heads = (int32_t)num_q_heads;
  p.num_splits = (int32_t)num_splits; p.split_chunk = (int32_t)split_chunk;
  p.stride_q_tok = stride_q_tok; p.stride_o_tok = stride_o_tok; p.stride_kv_slot = stride_kv_slot;
  p.scale_log2 = sm_scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;

  const dim3 grid((unsigned)(work ? num_work : total_tokens), (unsigned)cdiv64(num_q_heads, 16), (unsigned)(work ? 1 : num_splits));
  if (dtype == MI_BF16) mla_attn_kernel<bf16_t><<<grid, 256, MLA_LDS, st>>>(p);
  else mla_attn_kernel<f16_t><<<grid, 256, MLA_LDS, st>>>(p);
  MI_CHECK_LAUNCH();
  if (num_splits > 1)
    // without a work list every (row, split) workgroup ran and wrote its (m, l): the merge need not read kv_indptr
    return mi_attn_merge_splits512(p.ws_o, p.ws_ml, o, total_tokens, num_q_heads, num_splits, stride_o_tok,
                                   work ? kv_indptr : nullptr, split_chunk, plan, dtype, stream);
  return MI_OK;
}
