// Flash-attention forward, bf16 in / fp32 softmax+accumulate / bf16 out, head_dim 128, no mask
// (the reference's SDPA path: wan_fantasy_transformer3d_1B.py:158-207 with q_lens/k_lens ignored,
// which it warns about at :190-193).  One kernel serves every attention site of the DiT:
//   * self-attention            (1B:402-407)   segments = batch rows, Lq = Lk = seq_len
//   * text / image cross-attn   (1B:556-570)   Lk = 512 / 257 (tail key block masked)
//   * per-frame vocal cross-attn(1B:575-586)   segments = (batch, latent frame), Lk = 17
// Segments come from a device table {q_row0, q_len, kv_row0, kv_len}; rows index flat
// [rows, stride] bf16 matrices with head h at column h*128, so Q/K/V are read straight out of
// the fused QKV GEMM output (no transposes).  ACCUMULATE adds into an existing bf16 output,
// which is how the three cross-attention terms are summed (1B:603).
//
// Structure (cdna_hip_programming.md App. B "Fused attention prefill"): 8 waves x 32 query rows,
// KV blocks of 64 keys staged by global_load_lds into a 2-deep LDS ring (XOR-swizzled 256-B rows).
// Swapped product S^T = K·Q^T puts one query per lane, so the online softmax is lane-local; P^T is
// fed back as the B operand straight from the accumulator and V^T comes from ds_read_b64_tr_b16,
// giving O^T with the query on the lane (rescale is per lane).
//
// Layout of this file: the small-query kernels; the pieces of a 64-key block on mfma_f32_16x16x32_bf16 (v6_*), the
// two V layouts (VRows: V rows beside K, VTrans: V^T from the QKV GEMM's epilogue) and the one block over them,
// attn_v6_block; the pieces of a kernel body (attn_grid_tile, attn_zero_rows, attn_load_q, attn_row_rsrc /
// attn_row_load, attn_k_bases, attn_pair16, attn_store_o) and the one 2-stage ring, attn_ring2 (a plain counter, or a
// block list for the sparse launches).  Every self-attention kernel -- 8 waves, 4 waves, the key split, V^T, and the
// block-sparse forms of the 8-wave ones -- is attn_fwd_body<layout, waves, SPLIT, SPARSE>; the fused cross-attention
// (attn_cross3_body) keeps its own staging (three sources through per-block descriptors) and its NST-stage ring, and
// takes the rest from the same pieces.  What each kernel kept of its own, and the records that say the fold left
// bytes, loops and speed alone: DESIGN.md, "Self-attention, the fold".
#include <stdlib.h>

#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace {

struct AttnArgs {
  const bf16* q; const bf16* k; const bf16* v; bf16* o;
  const int* segs;
  long qs, ks, vs, os;
  float c;  // softmax scale * log2(e)
  int accumulate;
  const int* orows;  // output row of query row r = orows[r] (null: r); the Ulysses exchange's receive layout
  // key-split launches (attn_fwd_v6_split_kernel): a 1-D grid whose first split_full workgroups are whole query tiles
  // and whose last 2 x split_n are the two key halves of the last split_n tiles (tile = (segment, head, query block),
  // nqb query blocks per segment, nheads heads); the halves write unnormalised fp32 partials to work
  int nqb, nheads, split_full, split_n;
  float* work;
};

// block-sparse launches (attn_fwd_v6_sparse_kernel, attn_fwd_v6t_sparse_kernel): query block qb of every segment and
// head runs the 64-key blocks blk_idx[blk_ptr[qb] .. blk_ptr[qb + 1]) of its segment, ascending, instead of all of them
struct AttnSparseArgs : AttnArgs {
  const int* blk_ptr;
  const int* blk_idx;
};
// a table word at a wave-uniform address: the constant address space makes it one scalar load (s_load_dword)
__device__ __forceinline__ int sload(const int* p) {
  return *(const __attribute__((address_space(4))) int*)(uintptr_t)p;
}

constexpr int D = 128;
constexpr int WAVES = 8;
constexpr int QB = WAVES * 32;
constexpr int KVB = 64;
constexpr int TILE_BYTES = KVB * D * 2;      // 16 KB
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // K + V
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 64 KB

constexpr float RESCALE_THR = 8.0f;  // log2 units: P <= 2^8 between rescales (fused cross-attention)
// self-attention blocks (v6_softmax_p): the running max sits RESCALE_BIAS above the rows' maxima after each move, and
// the next move comes when a score passes its row's maximum by RESCALE_BIAS + 1 = RESCALE_THR
constexpr float RESCALE_BIAS = RESCALE_THR - 1.0f;

// vmax3's two-operand form (common.h)
__device__ __forceinline__ float vmax2(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// the transposed LDS read, issued and retired as ds_b128 (common.h)
template <int OFF>
__device__ __forceinline__ void ds_tr64(u32x2& d, uint32_t addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
template <int N>
__device__ __forceinline__ void wait_v(u32x2* f) {
  asm volatile("s_waitcnt lgkmcnt(%8)"
               : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7])
               : "i"(N));
}
// The fused cross-attention keeps K and V of a block in separate 3-stage regions (K stage b at b * 16 KB,
// V stage b at 48 KB + b * 16 KB; the V read bases include the 48 KB) so a block's DMA is issued two blocks
// ahead
constexpr int X3_LDS = 6 * TILE_BYTES;  // 96 KB

// ---- fused cross-attention of WanI2VTalkingCrossAttention (1B:556-603): per query block, the text
// (1B:564-570), image (1B:556-562) and per-frame vocal (1B:575-586) attentions run back to back over
// one K/V block stream, each with its own online softmax, and the three outputs are summed with the
// reference's bf16 rounding, (bf16(text) + bf16(img)) + bf16(vocal) (1B:602), so Q is read once and O
// written once.  A query block must lie inside one latent frame (tokens_per_frame % 256 == 0).
struct Cross3Args {
  const bf16* q; long qs;
  const bf16* kt; const bf16* vt; long ts; int t_len;
  const bf16* ki; const bf16* vi; long is; int i_len;
  const bf16* kv; const bf16* vv; long vs; int nper, tpf, n_frames, tok_offset;
  bf16* o; long os;
  int q_len;
  float c;
};

// ---- small-query attention for head dims the MFMA kernel does not take (vocal projector, D=192 for
// 1.3B and 640 for 14B, 17 queries per frame vs one latent frame's tokens: vocal_projector_fantasy_1B.py:
// 259-270, vocal_projector_fantasy_14B.py:254-267; wav2vec2, D=64).  One wave
// per (segment, head, query): scores for all keys in LDS, exact softmax, lane-parallel P·V.
constexpr int SMALL_MAXK = 4096;
constexpr int SMALL_MAXD = 640;

__global__ __launch_bounds__(256) void attn_small_kernel(const bf16* q, const bf16* k, const bf16* v, bf16* o,
                                                         const int* segs, int heads, int D, long qs, long ks, long vs,
                                                         long os, float scale) {
  __shared__ float p[4][SMALL_MAXK];
  __shared__ float qv[4][SMALL_MAXD];
  const int* sg = segs + blockIdx.z * 4;
  const int q_row0 = sg[0], q_len = sg[1], kv_row0 = sg[2], kv_len = sg[3];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int qi = blockIdx.x * 4 + w;
  const int h = blockIdx.y;
  if (qi >= q_len) return;
  const bf16* qp = q + (long)(q_row0 + qi) * qs + h * D;
  for (int d = lane; d < D; d += 64) qv[w][d] = bf2f(qp[d]) * scale;
  __builtin_amdgcn_wave_barrier();
  float mx = -INFINITY;
  for (int j = lane; j < kv_len; j += 64) {
    const bf16* kp = k + (long)(kv_row0 + j) * ks + h * D;
    float s = 0.f;
    for (int d = 0; d < D; d += 8) {
      const bf16x8 kk = *(const bf16x8*)(kp + d);
#pragma unroll
      for (int t = 0; t < 8; ++t) s = fmaf(qv[w][d + t], bf2f(kk[t]), s);
    }
    p[w][j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < kv_len; j += 64) {
    const float e = __expf(p[w][j] - mx);
    p[w][j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __builtin_amdgcn_wave_barrier();
  const float inv = sum > 0.f ? 1.f / sum : 0.f;  // no keys: zeros, as SDPA
  bf16* op = o + (long)(q_row0 + qi) * os + h * D;
  for (int d = lane; d < D; d += 64) {
    float acc = 0.f;
    for (int j = 0; j < kv_len; ++j) acc = fmaf(p[w][j], bf2f(v[(long)(kv_row0 + j) * vs + h * D + d]), acc);
    op[d] = f2bf(acc * inv);
  }
}

// ---- small-query attention, head dim <= 256 (vocal projector D = 192, wav2vec2 D = 64, CLIP D = 80): one
// workgroup per (32-query chunk, head, segment), 4 waves x 8 queries; keys in chunks of 64 staged into LDS
// (K / V rows padded by 16 B: conflict-free row-per-lane b128 reads), scores with the key on the lane
// (Q broadcast from LDS, prescaled by scale·log2e), online softmax in fp32, then O with 4 head dims per
// lane.  The one-wave-per-query kernel above re-read K and V from L2 for every query (0.7 ms per vocal-
// projector call at config 2); this reads them once per 32 queries.
// Key split (nsplit > 1): the workgroups of a 32-query chunk each take kper keys and write their unnormalised O,
// running max and row sum to `work`, and attn_small2_combine_kernel merges them.  A sequence-parallel rank's vocal
// projector has 17 queries x 8 heads x 3 frames = 24 workgroups, each walking 1024 keys alone (0.28 ms per call at
// N = 8); split 8 ways, the same keys run on 192 CUs.
constexpr int SM2_D = 256, SM2_DP = SM2_D + 8, SM2_KC = 64, SM2_QW = 32;

// work block of one (segment, head, query chunk, split): O [32][D], then m [32], then l [32] (fp32)
__device__ __forceinline__ float* sm2_work_block(float* work, int seg, int h, int qc, int s, int heads, int nqc,
                                                 int nsplit, int D) {
  return work + ((((long)seg * heads + h) * nqc + qc) * nsplit + s) * (long)(SM2_QW * (D + 2));
}

__global__ __launch_bounds__(256) void attn_small2_kernel(const bf16* q, const bf16* k, const bf16* v, bf16* o,
                                                          const int* segs, int D, long qs, long ks, long vs, long os,
                                                          float c, int nsplit, int kper, float* work) {
  __shared__ __attribute__((aligned(16))) bf16 Ks[SM2_KC * SM2_DP];
  __shared__ __attribute__((aligned(16))) bf16 Vs[SM2_KC * SM2_DP];
  __shared__ __attribute__((aligned(16))) float Qs[SM2_QW * SM2_D];
  __shared__ __attribute__((aligned(16))) float Ps[4][8][SM2_KC];
  const int* sg = segs + blockIdx.z * 4;
  const int q_row0 = sg[0], q_len = sg[1], kv_row0 = sg[2], kv_len = sg[3];
  const int qc = blockIdx.x / nsplit, split = blockIdx.x % nsplit;
  const int q0 = qc * SM2_QW;
  if (q0 >= q_len) return;
  const int kb0 = split * kper, kb1 = min(kv_len, kb0 + kper);  // this workgroup's keys
  const int h = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int DP = D + 8, nch = D / 8;  // padded row (elements), 16-B chunks per row
  // Q rows of this chunk, fp32, prescaled (rows past q_len: zeros, never stored)
  for (int i = tid; i < SM2_QW * nch; i += 256) {
    const int r = i / nch, ch = i % nch;
    float* dst = Qs + r * SM2_D + ch * 8;
    if (q0 + r < q_len) {
      const bf16x8 x = *(const bf16x8*)(q + (long)(q_row0 + q0 + r) * qs + h * D + ch * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = bf2f(x[j]) * c;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = 0.f;
    }
  }
  float m[8], l[8], O[8][4];
#pragma unroll
  for (int qq = 0; qq < 8; ++qq) {
    m[qq] = -INFINITY;
    l[qq] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) O[qq][t] = 0.f;
  }
  const float* Qw = Qs + w * 8 * SM2_D;
  for (int kc = kb0; kc < kb1; kc += SM2_KC) {
    __syncthreads();  // previous chunk's K / V reads done (and Q written, first time)
    for (int i = tid; i < SM2_KC * nch; i += 256) {
      const int r = i / nch, ch = i % nch;
      u32x4 kx = {0u, 0u, 0u, 0u}, vx = {0u, 0u, 0u, 0u};
      if (kc + r < kb1) {
        kx = *(const u32x4*)(k + (long)(kv_row0 + kc + r) * ks + h * D + ch * 8);
        vx = *(const u32x4*)(v + (long)(kv_row0 + kc + r) * vs + h * D + ch * 8);
      }
      *(u32x4*)(Ks + r * DP + ch * 8) = kx;
      *(u32x4*)(Vs + r * DP + ch * 8) = vx;
    }
    __syncthreads();
    // scores of this lane's key for the wave's 8 queries
    float sc[8];
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) sc[qq] = 0.f;
    for (int d = 0; d < D; d += 8) {
      const bf16x8 kk = *(const bf16x8*)(Ks + lane * DP + d);
      float kf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[j] = bf2f(kk[j]);
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) {
        const f32x4 a = *(const f32x4*)(Qw + qq * SM2_D + d), b = *(const f32x4*)(Qw + qq * SM2_D + d + 4);
        sc[qq] = fmaf(kf[0], a[0], sc[qq]); sc[qq] = fmaf(kf[1], a[1], sc[qq]);
        sc[qq] = fmaf(kf[2], a[2], sc[qq]); sc[qq] = fmaf(kf[3], a[3], sc[qq]);
        sc[qq] = fmaf(kf[4], b[0], sc[qq]); sc[qq] = fmaf(kf[5], b[1], sc[qq]);
        sc[qq] = fmaf(kf[6], b[2], sc[qq]); sc[qq] = fmaf(kf[7], b[3], sc[qq]);
      }
    }
    const bool valid = kc + lane < kb1;
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) {
      const float s = valid ? sc[qq] : -INFINITY;
      const float m_new = fmaxf(m[qq], wave_max(s));  // finite: every chunk has a valid key
      const float alpha = __builtin_amdgcn_exp2f(m[qq] - m_new);
      const float p = __builtin_amdgcn_exp2f(s - m_new);
      l[qq] = l[qq] * alpha + wave_sum(p);
      m[qq] = m_new;
#pragma unroll
      for (int t = 0; t < 4; ++t) O[qq][t] *= alpha;
      Ps[w][qq][lane] = p;
    }
    __builtin_amdgcn_wave_barrier();  // the wave's own P writes before its broadcast reads (LDS is in order)
    // O[q][4 lane .. 4 lane + 3] += sum_j P[q][j] V[j][..]
    if (4 * lane < D) {
      for (int j = 0; j < SM2_KC; j += 4) {
        float vf[4][4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const bf16x4 vv = *(const bf16x4*)(Vs + (j + jj) * DP + 4 * lane);
#pragma unroll
          for (int t = 0; t < 4; ++t) vf[jj][t] = bf2f(vv[t]);
        }
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) {
          const f32x4 p4 = *(const f32x4*)(&Ps[w][qq][j]);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int t = 0; t < 4; ++t) O[qq][t] = fmaf(p4[jj], vf[jj][t], O[qq][t]);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();  // P reads done before the next chunk overwrites P
  }
  if (nsplit > 1) {  // partial result (a split with no keys: m = -inf, l = 0, O = 0)
    float* blk = sm2_work_block(work, blockIdx.z, h, qc, split, gridDim.y, (gridDim.x + nsplit - 1) / nsplit,
                                nsplit, D);
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) {
      const int r = w * 8 + qq;
      if (q0 + r < q_len) {
        if (4 * lane < D) *(f32x4*)(blk + r * D + 4 * lane) = (f32x4){O[qq][0], O[qq][1], O[qq][2], O[qq][3]};
        if (lane == 0) {
          blk[SM2_QW * D + r] = m[qq];
          blk[SM2_QW * D + SM2_QW + r] = l[qq];
        }
      }
    }
    return;
  }
  if (4 * lane < D) {
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) {
      const int qi = q0 + w * 8 + qq;
      if (qi < q_len) {
        const float inv = l[qq] > 0.f ? 1.f / l[qq] : 0.f;  // a segment with no keys: zeros, as SDPA
        *(bf16x4*)(o + (long)(q_row0 + qi) * os + h * D + 4 * lane) =
            (bf16x4){f2bf(O[qq][0] * inv), f2bf(O[qq][1] * inv), f2bf(O[qq][2] * inv), f2bf(O[qq][3] * inv)};
      }
    }
  }
}

// merge of the key splits: O = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s, M = max_s m_s (m in log2 units)
__global__ __launch_bounds__(256) void attn_small2_combine_kernel(bf16* o, const int* segs, int D, long os,
                                                                  int nsplit, const float* work) {
  const int* sg = segs + blockIdx.z * 4;
  const int q_row0 = sg[0], q_len = sg[1];
  const int qc = blockIdx.x, q0 = qc * SM2_QW, h = blockIdx.y;
  if (q0 >= q_len) return;
  const int nq = min(SM2_QW, q_len - q0), n4 = D / 4;
  const float* blk0 = sm2_work_block(const_cast<float*>(work), blockIdx.z, h, qc, 0, gridDim.y, gridDim.x, nsplit, D);
  const long bstride = (long)SM2_QW * (D + 2);
  for (int i = threadIdx.x; i < nq * n4; i += 256) {
    const int r = i / n4, d = (i % n4) * 4;
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, blk0[s * bstride + SM2_QW * D + r]);
    float L = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (M != -INFINITY) {
      for (int s = 0; s < nsplit; ++s) {
        const float* b = blk0 + s * bstride;
        const float a = __builtin_amdgcn_exp2f(b[SM2_QW * D + r] - M);
        L += a * b[SM2_QW * D + SM2_QW + r];
        const f32x4 x = *(const f32x4*)(b + r * D + d);
        acc[0] += a * x[0]; acc[1] += a * x[1]; acc[2] += a * x[2]; acc[3] += a * x[3];
      }
    }
    const float inv = L > 0.f ? 1.f / L : 0.f;  // no keys at all: zeros, as SDPA
    *(bf16x4*)(o + (long)(q_row0 + q0 + r) * os + h * D + d) =
        (bf16x4){f2bf(acc[0] * inv), f2bf(acc[1] * inv), f2bf(acc[2] * inv), f2bf(acc[3] * inv)};
  }
}

}  // namespace

static bool sm2_applies(const void* q, const void* v, const void* o, int head_dim, int64_t q_stride, int64_t v_stride,
                        int64_t o_stride) {
  return head_dim <= SM2_D && !(q_stride % 8) && !(v_stride % 8) && !(o_stride % 4) &&
         !(((uintptr_t)q | (uintptr_t)v) & 15) && !(((uintptr_t)o) & 7);
}

extern "C" int sa_attn_small(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                             int max_q_len, int max_kv_len, int heads, int head_dim, int64_t q_stride,
                             int64_t k_stride, int64_t v_stride, int64_t o_stride, float scale, void* stream);

extern "C" int sa_attn_small_split(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                                   int max_q_len, int max_kv_len, int heads, int head_dim, int64_t q_stride,
                                   int64_t k_stride, int64_t v_stride, int64_t o_stride, float scale, int nsplit,
                                   void* work, int64_t work_bytes, void* stream) {
  if (!q || !k || !v || !o || !segs || nseg <= 0 || max_q_len <= 0 || heads <= 0 || nsplit < 2) return SA_ERR_ARG;
  if (head_dim <= 0 || head_dim % 8 || max_kv_len <= 0 || (k_stride % 8) || (((uintptr_t)k) & 15)) return SA_ERR_ARG;
  if (!sm2_applies(q, v, o, head_dim, q_stride, v_stride, o_stride)) return SA_ERR_ARG;
  const int nchunks = (max_kv_len + SM2_KC - 1) / SM2_KC;
  const int per = (nchunks + nsplit - 1) / nsplit;  // 64-key chunks per split
  nsplit = (nchunks + per - 1) / per;               // no split without keys at the longest segment
  const int nqc = (max_q_len + SM2_QW - 1) / SM2_QW;
  const int64_t need = (int64_t)nseg * heads * nqc * nsplit * SM2_QW * (head_dim + 2) * 4;
  if (!work || (((uintptr_t)work) & 15) || work_bytes < need) return SA_ERR_ARG;
  if (nsplit < 2) return sa_attn_small(q, k, v, o, segs, nseg, max_q_len, max_kv_len, heads, head_dim, q_stride,
                                       k_stride, v_stride, o_stride, scale, stream);
  hipLaunchKernelGGL(attn_small2_kernel, dim3(nqc * nsplit, heads, nseg), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, segs, head_dim, q_stride, k_stride,
                     v_stride, o_stride, scale * 1.4426950408889634f, nsplit, per * SM2_KC, (float*)work);
  SA_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_small2_combine_kernel, dim3(nqc, heads, nseg), dim3(256), 0, (hipStream_t)stream, (bf16*)o,
                     segs, head_dim, o_stride, nsplit, (const float*)work);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

extern "C" int sa_attn_small(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                             int max_q_len, int max_kv_len, int heads, int head_dim, int64_t q_stride,
                             int64_t k_stride, int64_t v_stride, int64_t o_stride, float scale, void* stream) {
  if (!q || !k || !v || !o || !segs || nseg <= 0 || max_q_len <= 0 || heads <= 0) return SA_ERR_ARG;
  if (head_dim <= 0 || head_dim > SMALL_MAXD || head_dim % 8 || max_kv_len <= 0) return SA_ERR_ARG;
  if ((k_stride % 8) || (((uintptr_t)k) & 15)) return SA_ERR_ARG;
  // the tiled kernel: 16-byte Q / K / V row chunks, 8-byte O stores (head_dim % 8 == 0 already holds)
  if (sm2_applies(q, v, o, head_dim, q_stride, v_stride, o_stride)) {
    dim3 grid2((max_q_len + SM2_QW - 1) / SM2_QW, heads, nseg);
    hipLaunchKernelGGL(attn_small2_kernel, grid2, dim3(256), 0, (hipStream_t)stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (bf16*)o, segs, head_dim, q_stride, k_stride, v_stride, o_stride,
                       scale * 1.4426950408889634f, 1, max_kv_len, (float*)nullptr);
    SA_LAUNCH_CHECK();
    return SA_OK;
  }
  if (max_kv_len > SMALL_MAXK) return SA_ERR_ARG;  // the one-wave-per-query kernel keeps a score row in LDS
  dim3 grid((max_q_len + 3) / 4, heads, nseg);
  hipLaunchKernelGGL(attn_small_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)q, (const bf16*)k,
                     (const bf16*)v, (bf16*)o, segs, heads, head_dim, q_stride, k_stride, v_stride, o_stride, scale);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

// ---- v6: v3's pipeline (2-deep K/V ring by LDS-DMA, asm LDS reads with counted waits, prescaled Q
// and -m as the QK^T initial accumulator, deferred rescale) on mfma_f32_16x16x32_bf16 instead of
// 32x32x16.  The two shapes take the same cycles per FLOP, but under load the chip holds a higher
// clock on the 16x16x32 stream (MI355X_MICROARCH.md "DVFS give-back" item 7: ~1.12-1.15x FLOP/s on
// random data).  Per wave: 32 queries as two 16-query tiles, 64-key blocks as four 16-key tiles.
//   S^T tile (kt, qt) = K_kt · Q_qt^T: lane holds keys 4g+i (g = lane/16) of tile kt for query lane%16
//   P^T as the PV B operand: the 32-key chunk c is taken in the permuted key order
//     k = 8g + j -> key 32c + 4g + j (j < 4), 32c + 16 + 4g + j - 4 (j >= 4)
//   so a lane's 8 P values are its own S^T registers of tiles 2c and 2c+1 (no lane exchange), and the
//   V^T A operand uses the same order: two ds_read_b64_tr_b16 (rows 32c+4g.. and 32c+16+4g..)
//   row max over 64 keys: 15 VALU max + permlane32 / permlane16 swaps; row sums stay per lane until
//   the end.
// LDS images: K rows chunk ^ (row & 15) (conflict-free 16-row b128 reads), V rows chunk ^ 2(row & 7)
// (conflict-free transposed reads).
__device__ __forceinline__ bf16x8 v6_as_bf8(u32x4 x) { return __builtin_bit_cast(bf16x8, x); }
__device__ __forceinline__ bf16x8 v6_as_bf8(u32x2 lo, u32x2 hi) {
  const u32x4 x = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(bf16x8, x);
}

// K fragments of key tile KT (d chunks 0-3) of the K stage at byte KOFF from the K read bases
template <int KOFF, int KT>
__device__ __forceinline__ void v6_read_k(u32x4* f, const uint32_t* ka) {
  constexpr int base = KOFF + KT * 4096;
  ds_b128<base>(f[0], ka[0]);
  ds_b128<base>(f[1], ka[1]);
  ds_b128<base>(f[2], ka[2]);
  ds_b128<base>(f[3], ka[3]);
}
// V^T fragments of key chunk C for d tiles DT0..DT0+3 of the V stage at byte VOFF from the V read bases:
// f[2*t + h], h = rows +0 / +16
template <int VOFF, int C, int DT0>
__device__ __forceinline__ void v6_read_v(u32x2* f, const uint32_t* va) {
  constexpr int base = VOFF + C * 8192;
  ds_tr64<base>(f[0], va[DT0 + 0]); ds_tr64<base + 4096>(f[1], va[DT0 + 0]);
  ds_tr64<base>(f[2], va[DT0 + 1]); ds_tr64<base + 4096>(f[3], va[DT0 + 1]);
  ds_tr64<base>(f[4], va[DT0 + 2]); ds_tr64<base + 4096>(f[5], va[DT0 + 2]);
  ds_tr64<base>(f[6], va[DT0 + 3]); ds_tr64<base + 4096>(f[7], va[DT0 + 3]);
}
template <int NKT>
__device__ __forceinline__ void v6_mma_k(f32x4 (&S)[NKT][2], int kt, const u32x4* f, const bf16x8 (&qf)[2][4]) {
#pragma unroll
  for (int dc = 0; dc < 4; ++dc) {
    S[kt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v6_as_bf8(f[dc]), qf[0][dc], S[kt][0], 0, 0, 0);
    S[kt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v6_as_bf8(f[dc]), qf[1][dc], S[kt][1], 0, 0, 0);
  }
}
__device__ __forceinline__ void v6_mma_v(f32x4 (&O)[8][2], int dt0, const u32x2* f, const bf16x8 (&pb)[2]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bf16x8 a = v6_as_bf8(f[2 * t], f[2 * t + 1]);
    O[dt0 + t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb[0], O[dt0 + t][0], 0, 0, 0);
    O[dt0 + t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb[1], O[dt0 + t][1], 0, 0, 0);
  }
}
template <int N>
__device__ __forceinline__ void wait_k4(u32x4* f) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) : "i"(N));
}

struct V6State {
  f32x4 O[8][2];
  f32x4 L[2];     // row sums of the bf16 P (every element equal), from a ones x P^T MFMA
  float negm[2];  // -m per query tile (this lane's query)
  f32x4 negm4[2];  // the same as the QK^T chains' initial accumulator (refreshed only on a rescale)
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) O[dt][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    L[0] = L[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    negm[0] = negm[1] = 0.f;
    negm4[0] = negm4[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
};

// max over 16 values of one query's S^T column slice, then over the 4 lane groups (permlane32 / 16 swaps)
__device__ __forceinline__ float rowmax64(const f32x4 (&S)[4][2], int qt) {
  float m = vmax3(S[0][qt][0], S[0][qt][1], S[0][qt][2]);
  m = vmax3(m, S[0][qt][3], S[1][qt][0]);
  m = vmax3(m, S[1][qt][1], S[1][qt][2]);
  m = vmax3(m, S[1][qt][3], S[2][qt][0]);
  m = vmax3(m, S[2][qt][1], S[2][qt][2]);
  m = vmax3(m, S[2][qt][3], S[3][qt][0]);
  m = vmax3(m, S[3][qt][1], S[3][qt][2]);
  m = vmax2(m, S[3][qt][3]);
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  m = vmax2(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return vmax2(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// max over this lane's 32 scores (both query tiles), as a 3-ary tree (depth 4 instead of a 16-long chain)
__device__ __forceinline__ float lanemax32(const f32x4 (&S)[4][2]) {
  float v[32];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[kt * 8 + qt * 4 + i] = S[kt][qt][i];
  float r[12];
#pragma unroll
  for (int j = 0; j < 10; ++j) r[j] = vmax3(v[3 * j], v[3 * j + 1], v[3 * j + 2]);
  r[10] = v[30];
  r[11] = v[31];
  const float a = vmax3(r[0], r[1], r[2]), b = vmax3(r[3], r[4], r[5]), c = vmax3(r[6], r[7], r[8]),
              d = vmax3(r[9], r[10], r[11]);
  return vmax2(vmax3(a, b, c), d);
}

// the fused cross-attention's softmax step (attn_v6_block<.., false>): the rescale test on the scores (a lane max
// over its 32 scores against RESCALE_THR, no row reduction unless it fails), the exponentials in place in S.  It
// keeps the cross-attention kernels inside 256 VGPRs with the fewest spills (the P-side test of v6_softmax_p holds
// the scores and the packed P of the whole block at once)
__device__ __forceinline__ void v6_softmax_s(V6State& st, f32x4 (&S)[4][2], const bool FIRST) {
  if (FIRST || !__all(lanemax32(S) <= RESCALE_THR)) {  // wave-uniform
    float mx[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) mx[qt] = rowmax64(S, qt);  // max of c S - m over the block's 64 keys
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float delta = FIRST ? mx[qt] : fmaxf(mx[qt], 0.f);
      if (!FIRST) {  // O and L are still zero on the first block (no 0 x inf for a very negative max)
        const float alpha = __builtin_amdgcn_exp2f(-delta);
        st.L[qt] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
#pragma unroll
          for (int i = 0; i < 4; ++i) st.O[dt][qt][i] *= alpha;
      }
      st.negm[qt] -= delta;
      st.negm4[qt] = (f32x4){st.negm[qt], st.negm[qt], st.negm[qt], st.negm[qt]};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) S[kt][qt][i] -= delta;
    }
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) S[kt][qt][i] = __builtin_amdgcn_exp2f(S[kt][qt][i]);
}

// P = bf16(exp2(S)) of a block in PV operand order (pb[c][qt]: key tiles 2c, 2c+1 of query tile qt); S is kept
__device__ __forceinline__ void v6_pack_exp(const f32x4 (&S)[4][2], bf16x8 (&pb)[2][2]) {
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pb[c][qt][j] = f2bf(__builtin_amdgcn_exp2f(S[2 * c][qt][j]));
        pb[c][qt][4 + j] = f2bf(__builtin_amdgcn_exp2f(S[2 * c + 1][qt][j]));
      }
}

// The online-softmax step of one 64-key block (attn_v6_block): P into pb, the running max moved
// first where needed.  The running max is kept RESCALE_BIAS log2 units above the rows' maxima (P <= 2^-7 right after
// a move), and the test runs on the bf16 P: some P >= 2 -- a score 8 above its row's maximum -- iff bit 14 of some
// packed P is set (P >= 0: biased exponent >= 128), so the OR of the 16 P dwords (8 v_or3) decides, where a max tree
// over the 32 scores took 16 ops (6.08-6.18 vs 6.19-6.22 ms per config-2 launch).  The first block, or a failed test,
// moves the running max of every row whose block maximum passes it, rescales O and L and forms P again from S.
template <bool FIRST_CT>
__device__ __forceinline__ void v6_softmax_p(V6State& st, f32x4 (&S)[4][2], bf16x8 (&pb)[2][2], bool first_rt) {
  const bool FIRST = FIRST_CT || first_rt;
  bool move = FIRST;
  if (!FIRST) {
    v6_pack_exp(S, pb);
    u32x4 w[4];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) w[2 * c + qt] = __builtin_bit_cast(u32x4, pb[c][qt]);
    // a depth-3 tree of v_or3 (a 7-long dependent chain measured 0.5 % slower, attn_or_tree_ab_r6tr.jsonl)
    const uint32_t a = w[0][0] | w[0][1] | w[0][2], b = w[0][3] | w[1][0] | w[1][1], c = w[1][2] | w[1][3] | w[2][0],
                   d = w[2][1] | w[2][2] | w[2][3], e = w[3][0] | w[3][1] | w[3][2];
    const uint32_t acc = (a | b | c) | (d | e | w[3][3]);
    move = !__all((acc & 0x40004000u) == 0u);  // wave-uniform
  }
  if (move) {
    float mx[2], alpha[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) mx[qt] = rowmax64(S, qt);  // max of c S - m over the block's 64 keys
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float delta = FIRST ? mx[qt] + RESCALE_BIAS : fmaxf(mx[qt] + RESCALE_BIAS, 0.f);
      alpha[qt] = __builtin_amdgcn_exp2f(-delta);
      st.negm[qt] -= delta;
      st.negm4[qt] = (f32x4){st.negm[qt], st.negm[qt], st.negm[qt], st.negm[qt]};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) S[kt][qt][i] -= delta;
    }
    if (!FIRST)  // O and L are still zero on the first block (no 0 x inf for a very negative max)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        st.L[qt] *= alpha[qt];
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
#pragma unroll
          for (int i = 0; i < 4; ++i) st.O[dt][qt][i] *= alpha[qt];
      }
    v6_pack_exp(S, pb);
  }
}

// ---- V^T form of the PV operand (V read as V^T from a d-major producer layout, [H*128][Rv] bf16: row h*128 + d holds
// d of head h for every key row), so each PV operand is ds_read_b128 instead of two ds_read_b64_tr_b16.
// V^T is staged 128 d-rows x 64 keys (128 B per d-row, 16-B chunk c of row d at position c ^ (d & 7)); the producer
//   stores the keys of each 32-key chunk in P's permuted order (position 8g + j <-> key 4g + j, j < 4;
//   16 + 4g + j - 4, j >= 4), so a lane's 16x16x32 PV operand is one b128 read.  (Measured and removed, records under
//   profiles/r05/: the PV product on 32x32x16 MFMAs, a two-wave ping-pong, a 3-stage ring.)
template <int VOFF, int C, int T0>
__device__ __forceinline__ void v6t_read_v(u32x4* f, const uint32_t* vb) {
  ds_b128<VOFF + (T0 + 0) * 2048>(f[0], vb[C]);
  ds_b128<VOFF + (T0 + 1) * 2048>(f[1], vb[C]);
  ds_b128<VOFF + (T0 + 2) * 2048>(f[2], vb[C]);
  ds_b128<VOFF + (T0 + 3) * 2048>(f[3], vb[C]);
}
__device__ __forceinline__ void v6t_mma_v(f32x4 (&O)[8][2], int dt0, const u32x4* f, const bf16x8 (&pb)[2]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const bf16x8 a = v6_as_bf8(f[t]);
    O[dt0 + t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb[0], O[dt0 + t][0], 0, 0, 0);
    O[dt0 + t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb[1], O[dt0 + t][1], 0, 0, 0);
  }
}

// descriptors of one head's rows of a row-major K (or V) of a segment: `all` over rows 0 .. len - 1 (a block in
// soffset), and a partial last block's own (base = its first row, soffset 0) whose range ends at the segment's last
// row, so its rows past len read as zeros (masked in S, and 0 x 0 in PV) instead of whatever follows.  The range check
// takes voffset + soffset + the instruction offset against the records (a V^T form reading per-source chunks, measured
// and removed in round 6, read zeros past a records value that left soffset out)
struct RowRsrc {
  __amdgpu_buffer_rsrc_t all, tail;
};
__device__ __forceinline__ RowRsrc attn_row_rsrc(const bf16* p, long stride, int row0, int len, int h) {
  const long tail0 = (long)((len + KVB - 1) / KVB - 1) * KVB;  // first row of the last block
  return {__builtin_amdgcn_make_buffer_rsrc((void*)(p + (long)row0 * stride + h * D), (short)0,
                                            (int)(((long)len - 1) * stride * 2 + 256), 0x00020000),
          __builtin_amdgcn_make_buffer_rsrc((void*)(p + (row0 + tail0) * stride + h * D), (short)0,
                                            (int)((len - tail0 - 1) * stride * 2 + 256), 0x00020000)};
}
// one 1-KB piece (4 rows) of block kb into LDS at dst: by buffer_load...lds from the SGPR descriptor, a per-lane 32-bit
// offset and the block in soffset -- no 64-bit address VALU.  tail: kb is the partial last block (wave-uniform)
__device__ __forceinline__ void attn_row_load(const RowRsrc& r, bool tail, int kb, int stride, uint32_t dst, int off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(tail ? r.tail : r.all, LDS_PTR((uintptr_t)dst), 16, off,
                                           tail ? 0 : kb * KVB * stride * 2, 0, 0);
}

// ---- V layouts: how a block's V gets into its 16-KB LDS tile (Src, off, load: piece = 1 KB, 16 per block), and from
// there into the PV MFMAs' A operand (bases, read, wait, mma: a fragment group = the operands of 4 d tiles, NF
// registers of type Frag).  Everything else of a block and of a kernel body is written once over them.
// VRows: V row-major beside K; LDS rows chunk ^ 2(row & 7); two ds_read_b64_tr_b16 per operand from bases va[d tile]
struct VRows {
  using Frag = u32x2;
  using Src = RowRsrc;
  static constexpr int NF = 8, NBASE = 8;
  static __device__ __forceinline__ Src src(const bf16* v, long vs, int row0, int len, int h) {
    return attn_row_rsrc(v, vs, row0, len, h);
  }
  static __device__ __forceinline__ int off(int piece, int lane, int vs) {
    const int srow = piece * 4 + (lane >> 4);
    return srow * vs * 2 + (((lane & 15) ^ ((srow & 7) << 1)) << 4);
  }
  static __device__ __forceinline__ void load(const Src& r, bool tail, int kb, int vs, uint32_t dst, int off) {
    attn_row_load(r, tail, kb, vs, dst, off);
  }
  // lds_v: the V tile of stage 0; the rest are +immediate
  static __device__ __forceinline__ void bases(uint32_t (&va)[NBASE], uint32_t lds_v, int g, int r16) {
    const int q = r16 >> 2, p = r16 & 3;
    const int row = 4 * g + q;  // + 32 c (+16): same swizzle
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const int ch = 2 * dt + (p >> 1);
      va[dt] = lds_v + row * 256 + ((ch ^ ((row & 7) << 1)) << 4) + 8 * (p & 1);
    }
  }
  template <int VOFF, int C, int T0>
  static __device__ __forceinline__ void read(Frag* f, const uint32_t* va) { v6_read_v<VOFF, C, T0>(f, va); }
  template <int N>
  static __device__ __forceinline__ void wait(Frag* f) { wait_v<N>(f); }
  static __device__ __forceinline__ void mma(f32x4 (&O)[8][2], int dt0, const Frag* f, const bf16x8 (&pb)[2]) {
    v6_mma_v(O, dt0, f, pb);
  }
};
// VTrans: V^T [heads * 128][vs] (v6t_read_v above); one ds_read_b128 per operand from bases vb[key chunk].  vs >= the
// columns any segment's last 64-key block reaches, i.e. kv_row0 + ceil64(kv_len); segments start on 32-key boundaries;
// every element of a row readable and finite through that block: the partial last block reads the keys past kv_len,
// masked to P = 0
struct VTrans {
  using Frag = u32x4;
  using Src = __amdgpu_buffer_rsrc_t;
  static constexpr int NF = 4, NBASE = 2;
  // the head's 128 d-rows from key row0, each through the segment's last block
  static __device__ __forceinline__ Src src(const bf16* v, long vs, int row0, int len, int h) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(v + (long)h * D * vs + row0), (short)0,
                                             (int)(((long)(D - 1) * vs + (long)((len + KVB - 1) / KVB) * KVB) * 2),
                                             0x00020000);
  }
  static __device__ __forceinline__ int off(int piece, int lane, int vs) {
    const int d = piece * 8 + (lane >> 3);  // a 1-KB piece = 8 d-rows x 128 B
    return d * vs * 2 + (((lane & 7) ^ (d & 7)) << 4);
  }
  static __device__ __forceinline__ void load(const Src& r, bool, int kb, int, uint32_t dst, int off) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, LDS_PTR((uintptr_t)dst), 16, off, kb * KVB * 2, 0, 0);
  }
  static __device__ __forceinline__ void bases(uint32_t (&vb)[NBASE], uint32_t lds_v, int g, int r16) {
#pragma unroll
    for (int c = 0; c < 2; ++c) vb[c] = lds_v + r16 * 128 + (((4 * c + g) ^ (r16 & 7)) << 4);
  }
  template <int VOFF, int C, int T0>
  static __device__ __forceinline__ void read(Frag* f, const uint32_t* vb) { v6t_read_v<VOFF, C, T0>(f, vb); }
  template <int N>
  static __device__ __forceinline__ void wait(Frag* f) { wait_k4<N>(f); }
  static __device__ __forceinline__ void mma(f32x4 (&O)[8][2], int dt0, const Frag* f, const bf16x8 (&pb)[2]) {
    v6t_mma_v(O, dt0, f, pb);
  }
};

// S'^T = c K Q^T - m of a block, K fragments two key tiles ahead
template <int KOFF>
__device__ __forceinline__ void v6_qk(f32x4 (&S)[4][2], const f32x4 (&negm4)[2], const bf16x8 (&qf)[2][4],
                                      const uint32_t* ka) {
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) S[kt][qt] = negm4[qt];
  u32x4 k0[4], k1[4];
  v6_read_k<KOFF, 0>(k0, ka);
  v6_read_k<KOFF, 1>(k1, ka);
  wait_k4<4>(k0);
  v6_mma_k(S, 0, k0, qf);
  v6_read_k<KOFF, 2>(k0, ka);
  wait_k4<4>(k1);
  v6_mma_k(S, 1, k1, qf);
  v6_read_k<KOFF, 3>(k1, ka);
  wait_k4<4>(k0);
  v6_mma_k(S, 2, k0, qf);
  wait_k4<0>(k1);
  v6_mma_k(S, 3, k1, qf);
}

__device__ __forceinline__ void v6_tail_mask(f32x4 (&S)[4][2], int kb, int kv_len, int g) {
  if (kb * KVB + KVB > kv_len) {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (kb * KVB + kt * 16 + 4 * g + i >= kv_len) { S[kt][0][i] = -INFINITY; S[kt][1][i] = -INFINITY; }
  }
}

// row sums of a key chunk's bf16 P: a ones x P^T MFMA per query tile
__device__ __forceinline__ void v6_rowsum(V6State& st, const bf16x8 (&pb)[2]) {
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (bf16)1.0f;
  st.L[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pb[0], st.L[0], 0, 0, 0);
  st.L[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pb[1], st.L[1], 0, 0, 0);
}

// one 64-key block whose K / V stages sit at KOFF / VOFF from the read bases (self-attention: K and V of a
// stage adjacent in a 2-stage ring; the fused cross-attention: separate NST-stage K and V regions), V in layout VL.
// The first block of a softmax sets the running max: FIRST_CT at compile time (self-attention), first_rt per source
// (cross-attention).  PTEST: the self-attention kernels' softmax step (P-side rescale test, P for the whole block);
// else the fused cross-attention's (v6_softmax_s, P formed per key chunk)
template <class VL, int KOFF, int VOFF, bool FIRST_CT, bool PTEST = true>
__device__ __forceinline__ void attn_v6_block(V6State& st, const bf16x8 (&qf)[2][4], const uint32_t* ka,
                                              const uint32_t* va, int kb, int kv_len, int g,
                                              bool first_rt = false) {
  f32x4 S[4][2];
  v6_qk<KOFF>(S, st.negm4, qf, ka);
  // first V fragments under the softmax
  typename VL::Frag v0[VL::NF], v1[VL::NF];
  VL::template read<VOFF, 0, 0>(v0, va);
  VL::template read<VOFF, 0, 4>(v1, va);
  v6_tail_mask(S, kb, kv_len, g);
  bf16x8 pb[2][2];
  if constexpr (PTEST) v6_softmax_p<FIRST_CT>(st, S, pb, first_rt);
  else v6_softmax_s(st, S, FIRST_CT || first_rt);
  // O^T += V^T P^T, key chunk c = tiles (2c, 2c+1); chunk 1's fragments are read as chunk 0's are consumed
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if constexpr (!PTEST)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pb[c][qt][j] = f2bf(S[2 * c][qt][j]);
          pb[c][qt][4 + j] = f2bf(S[2 * c + 1][qt][j]);
        }
    v6_rowsum(st, pb[c]);
    VL::template wait<VL::NF>(v0);
    VL::mma(st.O, 0, v0, pb[c]);
    if (c == 0) {
      VL::template read<VOFF, 1, 0>(v0, va);
      VL::template wait<VL::NF>(v1);
      VL::mma(st.O, 4, v1, pb[c]);
      VL::template read<VOFF, 1, 4>(v1, va);
    } else {
      VL::template wait<0>(v1);
      VL::mma(st.O, 4, v1, pb[c]);
    }
  }
}

// the fused cross-attention's last block of a source with at most 32 keys left (the image's 257th key, the 32
// vocal keys of a frame): attn_v6_block on key tiles 0-1 only -- half the QK^T / PV MFMAs and exponentials
__device__ __forceinline__ float rowmax32_c0(const f32x4 (&S)[2][2], int qt) {
  float m = vmax3(S[0][qt][0], S[0][qt][1], S[0][qt][2]);
  m = vmax3(m, S[0][qt][3], S[1][qt][0]);
  m = vmax3(m, S[1][qt][1], S[1][qt][2]);
  m = vmax2(m, S[1][qt][3]);
  const auto x = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  m = vmax2(__uint_as_float(x[0]), __uint_as_float(x[1]));
  const auto y = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return vmax2(__uint_as_float(y[0]), __uint_as_float(y[1]));
}

template <int KOFF, int VOFF>
__device__ __forceinline__ void attn_half_block(V6State& st, const bf16x8 (&qf)[2][4], const uint32_t* ka,
                                                const uint32_t* va, int kb, int kv_len, int g, bool first) {
  f32x4 S[2][2];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) S[kt][qt] = st.negm4[qt];
  u32x4 k0[4], k1[4];
  v6_read_k<KOFF, 0>(k0, ka);
  v6_read_k<KOFF, 1>(k1, ka);
  wait_k4<4>(k0);
  v6_mma_k(S, 0, k0, qf);
  wait_k4<0>(k1);
  v6_mma_k(S, 1, k1, qf);
  u32x2 v0[8], v1[8];
  v6_read_v<VOFF, 0, 0>(v0, va);
  v6_read_v<VOFF, 0, 4>(v1, va);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (kb * KVB + kt * 16 + 4 * g + i >= kv_len) { S[kt][0][i] = -INFINITY; S[kt][1][i] = -INFINITY; }
  float lm = vmax3(S[0][0][0], S[0][0][1], S[0][0][2]);
  lm = vmax3(lm, S[0][0][3], S[0][1][0]);
  lm = vmax3(lm, S[0][1][1], S[0][1][2]);
  lm = vmax3(lm, S[0][1][3], S[1][0][0]);
  lm = vmax3(lm, S[1][0][1], S[1][0][2]);
  lm = vmax3(lm, S[1][0][3], S[1][1][0]);
  lm = vmax3(lm, S[1][1][1], S[1][1][2]);
  lm = vmax2(lm, S[1][1][3]);
  if (first || !__all(lm <= RESCALE_THR)) {  // wave-uniform
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float mx = rowmax32_c0(S, qt);
      const float delta = first ? mx : fmaxf(mx, 0.f);
      if (!first) {
        const float alpha = __builtin_amdgcn_exp2f(-delta);
        st.L[qt] *= alpha;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
#pragma unroll
          for (int i = 0; i < 4; ++i) st.O[dt][qt][i] *= alpha;
      }
      st.negm[qt] -= delta;
      st.negm4[qt] = (f32x4){st.negm[qt], st.negm[qt], st.negm[qt], st.negm[qt]};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) S[kt][qt][i] -= delta;
    }
  }
  bf16x8 pb[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pb[qt][j] = f2bf(__builtin_amdgcn_exp2f(S[0][qt][j]));
      pb[qt][4 + j] = f2bf(__builtin_amdgcn_exp2f(S[1][qt][j]));
    }
  v6_rowsum(st, pb);
  wait_v<8>(v0);
  v6_mma_v(st.O, 0, v0, pb);
  wait_v<0>(v1);
  v6_mma_v(st.O, 4, v1, pb);
}

namespace {

// ---- pieces every flash body below is built from
// a 3-D grid (query blocks, heads, segments) flattened, remapped over the XCDs and decoded again
struct AttnTile {
  int qb, h, seg;
};
__device__ __forceinline__ AttnTile attn_tile(int flat, int nqb, int nheads) {
  return {flat % nqb, (flat / nqb) % nheads, flat / (nqb * nheads)};
}
__device__ __forceinline__ AttnTile attn_grid_tile() {
  const int nx = gridDim.x, ny = gridDim.y;
  return attn_tile(xcd_remap(blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z), nx * ny * gridDim.z), nx, ny);
}

// a segment (or a block list) without keys: zeros, as SDPA (nothing to add when accumulating)
template <int QBW>
__device__ __forceinline__ void attn_zero_rows(const AttnArgs& a, int qb, int h, int q_row0, int q_len) {
  if (a.accumulate) return;
  for (int i = threadIdx.x; i < QBW * (D / 8); i += QBW * 2) {  // QBW * 2 threads: a wave per 32 query rows
    const int qi = qb * QBW + i / (D / 8);
    if (qi < q_len) {
      const int orow = a.orows ? a.orows[q_row0 + qi] : q_row0 + qi;
      *(u32x4*)(a.o + (long)orow * a.os + h * D + (i % (D / 8)) * 8) = (u32x4){0u, 0u, 0u, 0u};
    }
  }
}

// Q as the B operand: query tile qt, d chunk dc: Q[query][dc*32 + 8g .. +7], prescaled by c; this wave's 32 queries
// from q0 of the segment, rows clamped to the segment
__device__ __forceinline__ void attn_load_q(bf16x8 (&qf)[2][4], const bf16* q, long qs, float c, int q_row0, int q_len,
                                            int q0, int h, int g, int r16) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int qc = min(q0 + qt * 16 + r16, q_len - 1);
    const bf16* qp = q + (long)(q_row0 + qc) * qs + h * D + 8 * g;
#pragma unroll
    for (int dc = 0; dc < 4; ++dc) {
      qf[qt][dc] = *(const bf16x8*)(qp + 32 * dc);
#pragma unroll
      for (int j = 0; j < 8; ++j) qf[qt][dc][j] = f2bf(bf2f(qf[qt][dc][j]) * c);
    }
  }
}

// per-lane LDS read bases of the K fragments (K tile of stage 0, key tile 0; the rest are +immediate)
__device__ __forceinline__ void attn_k_bases(uint32_t (&ka)[4], uint32_t lds_k, int g, int r16) {
#pragma unroll
  for (int dc = 0; dc < 4; ++dc) ka[dc] = lds_k + r16 * 256 + (((dc * 4 + g) ^ r16) << 4);
}

// the output address of this lane's 16 bytes of d tiles (0, 1) of one row: lane rows g and g^1 (lanes l, l^16) hold
// adjacent 4-column groups of one query row, and attn_pair16 below pairs d tiles (dt, dt+1) at + dt * 16 elements
__device__ __forceinline__ bf16* attn_o_ptr(bf16* o, long row, long os, int h, int g) {
  return o + row * os + h * D + 4 * (g & ~1) + 16 * (g & 1);
}
// one permlane16 swap per dword, so each lane stores 16 contiguous bytes (T21)
__device__ __forceinline__ u32x4 attn_pair16(bf16x4 pa, bf16x4 pb) {
  const u32x2 ga = __builtin_bit_cast(u32x2, pa), gb = __builtin_bit_cast(u32x2, pb);
  const auto rx = __builtin_amdgcn_permlane16_swap(ga[0], gb[0], false, false);
  const auto ry = __builtin_amdgcn_permlane16_swap(ga[1], gb[1], false, false);
  return (u32x4){rx[0], ry[0], rx[1], ry[1]};
}

// the self-attention output of this wave's 32 queries from q0 of the segment: bf16(O / l), added to the bf16 output
// when accumulating (bf16 + bf16 as the reference's sum of attention outputs, 1B:602)
__device__ __forceinline__ void attn_store_o(const V6State& st, const AttnArgs& a, int q_row0, int q_len, int q0, int h,
                                             int g, int r16) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float inv = 1.0f / st.L[qt][0];
    const int qi = q0 + qt * 16 + r16;
    const int qrow = q_row0 + min(qi, q_len - 1);
    bf16* op = attn_o_ptr(a.o, a.orows ? a.orows[qrow] : qrow, a.os, h, g);
#pragma unroll
    for (int dt = 0; dt < 8; dt += 2) {
      const f32x4& A = st.O[dt][qt];
      const f32x4& B = st.O[dt + 1][qt];
      const bf16x4 pa = {f2bf(A[0] * inv), f2bf(A[1] * inv), f2bf(A[2] * inv), f2bf(A[3] * inv)};
      const bf16x4 pb = {f2bf(B[0] * inv), f2bf(B[1] * inv), f2bf(B[2] * inv), f2bf(B[3] * inv)};
      u32x4 out = attn_pair16(pa, pb);
      bf16* p = op + dt * 16;
      if (a.accumulate) {
        const bf16x8 ov = *(const bf16x8*)p;
        bf16x8 nv = __builtin_bit_cast(bf16x8, out);
#pragma unroll
        for (int j = 0; j < 8; ++j) nv[j] = f2bf(bf2f(ov[j]) + bf2f(nv[j]));
        out = __builtin_bit_cast(u32x4, nv);
      }
      if (qi < q_len) *(u32x4*)p = out;
    }
  }
}

// the 2-stage ring over n >= 1 blocks: block i runs from stage i & 1 while block i + 1's DMA lands in the other (one
// block of lead, vmcnt(0) + __syncthreads() per block), the loop unrolled by two so the stage is a compile-time
// offset.  stage(kb, buf) issues block kb's DMA; block(buf, first, kb) runs it (buf, first: integral constants).
// LIST: block i is list[i] (a scalar table load), else i itself -- a plain counter.  Over a list, kc is the block being
// run, kn the one staged behind it, and the entry after that is read (clamped to the list) before the barrier that
// precedes its staging.  PRIO: the upper four of eight waves raise their priority (waves w and w+4 share a SIMD)
template <bool LIST, bool PRIO, class Stage, class Block>
__device__ __forceinline__ void attn_ring2(int n, [[maybe_unused]] const int* list, Stage stage, Block block) {
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  auto at = [&](int i) {
    if constexpr (LIST) return sload(list + min(i, n - 1));
    else return i;
  };
  [[maybe_unused]] int kn = at(1);
  auto step = [&](int i, auto buf) {  // block i from stage buf, block i + 1 staged behind it
    const int kc = LIST ? kn : i;
    kn = at(i + 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (i + 1 < n) stage(kn, 1 - buf());
    block(buf, std::false_type{}, kc);
  };
  const int k0 = at(0);
  stage(k0, 0);
  if (PRIO && __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256) __builtin_amdgcn_s_setprio(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (1 < n) stage(kn, 1);
  block(B0{}, std::true_type{}, k0);
  for (int i = 1; i < n; i += 2) {
    step(i, B1{});
    if (i + 1 >= n) break;
    step(i + 1, B0{});
  }
}

// The self-attention body over a V layout (VRows, VTrans).
// NW = 8: 256 query rows per workgroup, waves w and w+4 share a SIMD (one workgroup per CU); NW = 4: 128
// query rows, one wave per SIMD, two workgroups per CU -- the same per-SIMD pairing at half the work
// granularity, for launches whose 256-row workgroup count leaves the last round over the CUs mostly empty
// (the per-rank shapes of Ulysses SP: 378 workgroups at N = 8)
// SPLIT: the key-split launch (AttnArgs split_*): a half workgroup runs the flash loop over its half of the keys and
// writes O (unnormalised), the running max and the row sum instead of the output; attn_split_merge_kernel combines the
// two halves
// SPARSE: the block loop runs the query block's list (AttnSparseArgs) instead of 0 .. nkb - 1; an empty list is a
// segment with no keys
template <class VL, int NW, bool SPLIT = false, bool SPARSE = false>
__device__ __forceinline__ void attn_fwd_body(const std::conditional_t<SPARSE, AttnSparseArgs, AttnArgs>& a) {
  static_assert(!SPARSE || (NW == 8 && !SPLIT), "the block list serves the 8-wave whole-tile launches");
  constexpr int QBW = NW * 32, PPW = 16 / NW;  // query rows per workgroup, K (and V) 1-KB pieces per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  AttnTile t;
  int half = -1, stile = 0;
  if constexpr (SPLIT) {
    int tile;
    if ((int)blockIdx.x < a.split_full) {
      tile = xcd_remap(blockIdx.x, a.split_full);
    } else {
      const int idx = blockIdx.x - a.split_full;
      stile = idx >> 1;
      half = idx & 1;
      tile = a.split_full + stile;
    }
    t = attn_tile(tile, a.nqb, a.nheads);
  } else {
    t = attn_grid_tile();
  }
  const int qb = t.qb, h = t.h;
  const int* sg = a.segs + t.seg * 4;
  const int q_row0 = sg[0], q_len = sg[1];
  int kv_row0 = sg[2], kv_len = sg[3];
  if (SPLIT && half >= 0) {  // this half's keys: whole 64-key blocks in the first half
    const int kper = ((kv_len + 1) / 2 + KVB - 1) / KVB * KVB;
    if (half == 0) {
      kv_len = min(kv_len, kper);
    } else {
      kv_row0 += kper;
      kv_len -= kper;
    }
  }
  if (qb * QBW >= q_len) return;
  const int tid = threadIdx.x, lane = tid & 63;
  float* const wblk = SPLIT && half >= 0 ? a.work + ((long)stile * 2 + half) * QBW * (D + 2) : nullptr;
  if (SPLIT && half >= 0 && kv_len <= 0) {  // an empty half: m = -inf, l = 0, O = 0
    for (int i = tid; i < QBW * D; i += NW * 64) wblk[i] = 0.f;
    for (int i = tid; i < QBW; i += NW * 64) {
      wblk[QBW * D + i] = -INFINITY;
      wblk[QBW * D + QBW + i] = 0.f;
    }
    return;
  }
  [[maybe_unused]] const int* bl = nullptr;  // SPARSE: this query block's list and its length
  [[maybe_unused]] int nbl = 0;
  if constexpr (SPARSE) {
    const int p0 = sload(a.blk_ptr + qb);
    nbl = sload(a.blk_ptr + qb + 1) - p0;
    bl = a.blk_idx + p0;
  }
  if (kv_len <= 0 || (SPARSE && nbl <= 0)) return attn_zero_rows<QBW>(a, qb, h, q_row0, q_len);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const int q0 = qb * QBW + wave * 32;  // this wave's first query
  bf16x8 qf[2][4];
  attn_load_q(qf, a.q, a.qs, a.c, q_row0, q_len, q0, h, g, r16);

  // K/V pieces: each wave moves PPW x 1-KB pieces of K and of V per block; K lane -> row (lane / 16), stored position
  // lane % 16 holding source chunk (lane % 16) ^ (row & 15) (conflict-free 16-row b128 reads); V as its layout says
  const int nkb = (kv_len + KVB - 1) / KVB;
  const bool ragged = kv_len % KVB != 0;
  const RowRsrc rk = attn_row_rsrc(a.k, a.ks, kv_row0, kv_len, h);
  const typename VL::Src rv = VL::src(a.v, a.vs, kv_row0, kv_len, h);
  int koff[PPW], voff[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int srow = (wave * PPW + i) * 4 + g;
    koff[i] = srow * (int)a.ks * 2 + ((r16 ^ (srow & 15)) << 4);
    voff[i] = VL::off(wave * PPW + i, lane, (int)a.vs);
  }
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
  const uint32_t lds_dma = __builtin_amdgcn_readfirstlane(lds0 + wave * PPW * 1024);
  auto stage = [&](int kb, int buf) {  // LDS: 2 stages as K | V pairs
    const bool tail = ragged && kb == nkb - 1;  // wave-uniform
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      attn_row_load(rk, tail, kb, (int)a.ks, lds_dma + buf * STAGE_BYTES + i * 1024, koff[i]);
      VL::load(rv, tail, kb, (int)a.vs, lds_dma + buf * STAGE_BYTES + TILE_BYTES + i * 1024, voff[i]);
    }
  };
  uint32_t ka[4], va[VL::NBASE];
  attn_k_bases(ka, lds0, g, r16);
  VL::bases(va, lds0, g, r16);  // stage 0's V tile is TILE_BYTES on: in the blocks' VOFF

  V6State st;
  st.reset();
  attn_ring2<SPARSE, NW == 8>(SPARSE ? nbl : nkb, bl, stage, [&](auto buf, auto first, int kb) {
    attn_v6_block<VL, buf() * STAGE_BYTES, buf() * STAGE_BYTES + TILE_BYTES, first()>(st, qf, ka, va, kb, kv_len, g);
  });

  if (SPLIT && half >= 0) {  // partials: O^T[d][query] of this lane's d = 16 dt + 4 g + i, the query's max and sum
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int row = wave * 32 + qt * 16 + r16;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) *(f32x4*)(wblk + row * D + dt * 16 + 4 * g) = st.O[dt][qt];
      if (g == 0) {
        wblk[QBW * D + row] = -st.negm[qt];
        wblk[QBW * D + QBW + row] = st.L[qt][0];
      }
    }
    return;
  }
  attn_store_o(st, a, q_row0, q_len, q0, h, g, r16);
}

// the fused cross-attention on the self-attention block body: 8 waves x 32 queries of one query block,
// the text, image and per-frame vocal K/V streams one after the other through 3-stage K / V regions (each
// block's DMA two blocks ahead), a separate online softmax per source (its first block sets the max), the
// three bf16 outputs summed as the reference does
// NW waves x 32 queries per workgroup, NST-stage K / V ring (block j's DMA NST - 1 blocks ahead)
template <int NW, int NST>
__device__ __forceinline__ void attn_cross3_body(const Cross3Args& a) {
  constexpr int QBW = NW * 32, PPW = 16 / NW;  // queries per workgroup, K (and V) 1-KB pieces per wave per block
  constexpr int VBASE = NST * TILE_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AttnTile t = attn_grid_tile();
  const int qb = t.qb, h = t.h, b = t.seg;
  if (qb * QBW >= a.q_len) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const int q_row0 = b * a.q_len, q0 = qb * QBW + wave * 32;
  const int frame = (a.tok_offset + qb * QBW) / a.tpf;
  bf16x8 qf[2][4];
  attn_load_q(qf, a.q, a.qs, a.c, q_row0, a.q_len, q0, h, g, r16);

  // block stream: text blocks, image blocks, vocal block(s); LDS images as the self-attention kernel's
  // (K rows chunk ^ (row & 15), V rows chunk ^ 2 (row & 7)); each wave moves 2 x 1-KB pieces of K and V
  const int nT = (a.t_len + KVB - 1) / KVB, nI = (a.i_len + KVB - 1) / KVB, nV = (a.nper + KVB - 1) / KVB;
  const int ntot = nT + nI + nV;
  // staging by buffer descriptors rebased per block (SALU: base = the block's first row of this batch row's
  // source, range = its rows up to the source's last), so rows past the source read as zeros and are masked;
  // per-lane 32-bit offsets -- no 64-bit address VALU per block (the round-3 kernel formed clamped 64-bit row
  // addresses for every piece of every block).  The rows past a source's last key (the image stream's last block:
  // 257 = 4 x 64 + 1 keys) read as zeros through the records bound (the range check counts soffset too, round 6)
  int srow[PPW], kch[PPW], vch[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    srow[i] = (wave * PPW + i) * 4 + (lane >> 4);
    kch[i] = r16 ^ (srow[i] & 15);
    vch[i] = r16 ^ ((srow[i] & 7) << 1);
  }
  const long vrow0 = (long)(b * a.n_frames + frame) * a.nper;
  const bf16* const kt0 = a.kt + (long)b * a.t_len * a.ts + h * D;
  const bf16* const vt0 = a.vt + (long)b * a.t_len * a.ts + h * D;
  const bf16* const ki0 = a.ki + (long)b * a.i_len * a.is + h * D;
  const bf16* const vi0 = a.vi + (long)b * a.i_len * a.is + h * D;
  const bf16* const kv0 = a.kv + vrow0 * a.vs + h * D;
  const bf16* const vv0 = a.vv + vrow0 * a.vs + h * D;
  const uint32_t lds_k = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)LDS_PTR(smem) + wave * PPW * 1024);
  auto stage = [&](int j, int buf) {
    const bf16 *kb0 = kt0, *vb0 = vt0;
    int st = (int)a.ts, blk = j, len = a.t_len;
    if (j >= nT + nI) {
      kb0 = kv0; vb0 = vv0; st = (int)a.vs; blk = j - nT - nI; len = a.nper;
    } else if (j >= nT) {
      kb0 = ki0; vb0 = vi0; st = (int)a.is; blk = j - nT; len = a.i_len;
    }
    const long r0 = (long)blk * KVB;
    const int nrec = (int)((min((long)len - r0, (long)KVB) - 1) * st * 2 + 256);
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)(kb0 + r0 * st), (short)0, nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)(vb0 + r0 * st), (short)0, nrec, 0x00020000);
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
      const int rowoff = srow[i] * st * 2;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, LDS_PTR((uintptr_t)(lds_k + buf * TILE_BYTES + i * 1024)), 16,
                                               rowoff + kch[i] * 16, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rv, LDS_PTR((uintptr_t)(lds_k + VBASE + buf * TILE_BYTES + i * 1024)), 16, rowoff + vch[i] * 16, 0, 0, 0);
    }
  };

  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
  uint32_t ka[4], va[8];
  attn_k_bases(ka, lds0, g, r16);
  VRows::bases(va, lds0 + VBASE, g, r16);

  V6State st;
  // through a lambda of this body: with finish() below calling st.reset() itself, hipcc schedules the block loop
  // differently (the same instructions, 6 / 3 more s_nop cycles per block, 0.7 % / 0.3 % per launch at config 2)
  auto reset = [&]() { st.reset(); };
  reset();
  bf16x4 acc[8][2];  // running (text + img) + vocal, bf16 as in the reference
  // finish source `src` (0 text, 1 image, 2 vocal): bf16(O / l) folded into acc
  auto finish = [&](int src) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float inv = 1.0f / st.L[qt][0];
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) {
        bf16x4 x;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = f2bf(st.O[dt][qt][i] * inv);
        if (src == 0) {
          acc[dt][qt] = x;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[dt][qt][i] = f2bf(bf2f(acc[dt][qt][i]) + bf2f(x[i]));
        }
      }
    }
    reset();
  };

  // Block j sits in ring slot j % NST, chosen at run time through the LDS read bases (kas / vas): one copy of the
  // block body.  With a copy per slot (the slot as the ds_read immediate offset, round 4) hipcc spilled 118 (8 waves)
  // / 152 (4 waves) VGPRs to scratch: every copy's temporaries live across the unrolled loop.
  uint32_t kas[4], vas[8];
  auto at_slot = [&](int slot) {
    const uint32_t so = (uint32_t)slot * TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) kas[i] = ka[i] + so;
#pragma unroll
    for (int i = 0; i < 8; ++i) vas[i] = va[i] + so;
  };
  // block j's DMA issued NST - 1 blocks ahead (with one block of lead the L2 latency of the next block was exposed
  // at the barriers of these short streams)
  auto step = [&](int jj) {
    if (NST > 2 && jj + 1 < ntot)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * PPW) : "memory");  // block jj landed; jj+1 may still fly
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (jj + NST - 1 < ntot) stage(jj + NST - 1, (jj + NST - 1) % NST);
    const int src = jj < nT ? 0 : (jj < nT + nI ? 1 : 2);
    const int kb = src == 0 ? jj : (src == 1 ? jj - nT : jj - nT - nI);
    const int len = src == 0 ? a.t_len : (src == 1 ? a.i_len : a.nper);
    at_slot(jj % NST);
    attn_v6_block<VRows, 0, 0, false, false>(st, qf, kas, vas, kb, len, g, kb == 0);
    if (jj == nT - 1 || jj == nT + nI - 1 || jj == ntot - 1) finish(src);
  };
  // the vocal stream's single block when a frame has at most 32 audio tokens (StableAvatar: 32), and the image
  // stream's last block when it holds at most 32 keys (CLIP: 257 = 4 x 64 + 1) while the vocal block is peeled too:
  // peeled out of the loop as half blocks (key tiles 0-1: half the MFMAs and exponentials of a 64-key block)
  const bool vhalf = nV == 1 && a.nper <= KVB / 2;
  const bool ihalf = vhalf && a.i_len % KVB != 0 && a.i_len % KVB <= KVB / 2;
  auto half = [&](bool voc) {
    const int jj = voc ? ntot - 1 : ntot - 2;
    if (!voc && NST > 2)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * PPW) : "memory");  // this block landed; the vocal block may fly
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!voc && NST == 2) stage(jj + 1, (jj + 1) % NST);  // the vocal block, one ahead
    at_slot(jj % NST);
    attn_half_block<0, 0>(st, qf, kas, vas, voc ? 0 : nI - 1, voc ? a.nper : a.i_len, g, voc || nI == 1);
    finish(voc ? 2 : 1);
  };
  const int nloop = vhalf ? (ihalf ? ntot - 2 : ntot - 1) : ntot;
  if (NW == 8 && __builtin_amdgcn_readfirstlane(tid) >= 256) __builtin_amdgcn_s_setprio(1);
  stage(0, 0);
  if (NST > 2 && 1 < ntot) stage(1, 1);
  for (int j = 0; j < nloop; ++j) step(j);
  for (int hb = ihalf ? 0 : 1; hb < (vhalf ? 2 : 0); ++hb) half(hb == 1);

  // 16-byte stores from permlane16-swapped column-group pairs, as the self-attention epilogue (T21)
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int qi = q0 + qt * 16 + r16;
    bf16* op = attn_o_ptr(a.o, q_row0 + min(qi, a.q_len - 1), a.os, h, g);
#pragma unroll
    for (int dt = 0; dt < 8; dt += 2) {
      const u32x4 out = attn_pair16(acc[dt][qt], acc[dt + 1][qt]);
      if (qi < a.q_len) *(u32x4*)(op + dt * 16) = out;
    }
  }
}

__global__ __launch_bounds__(512) void attn_cross3_kernel(Cross3Args a) { attn_cross3_body<8, 3>(a); }
// 4 waves x 32 queries, 2-stage ring (64 KB): two workgroups per CU, so one's prologue (Q from HBM) and epilogue
// stores run beside the other's blocks
__global__ __launch_bounds__(256, 2) void attn_cross3_w4_kernel(Cross3Args a) { attn_cross3_body<4, 2>(a); }

__global__ __launch_bounds__(512) void attn_fwd_v6_kernel(AttnArgs a) { attn_fwd_body<VRows, 8>(a); }
__global__ __launch_bounds__(512) void attn_fwd_v6_split_kernel(AttnArgs a) { attn_fwd_body<VRows, 8, true>(a); }

// the two key halves of each split tile -> the output: O = (w0 O0 + w1 O1) / (w0 l0 + w1 l1), w = 2^(m - max(m0, m1))
__global__ __launch_bounds__(256) void attn_split_merge_kernel(AttnArgs a) {
  const int stile = blockIdx.x, tile = a.split_full + stile;
  const AttnTile t = attn_tile(tile, a.nqb, a.nheads);
  const int qb = t.qb, h = t.h;
  const int* sg = a.segs + t.seg * 4;
  const int q_row0 = sg[0], q_len = sg[1];
  if (qb * QB >= q_len) return;
  const float* w0 = a.work + (long)stile * 2 * QB * (D + 2);
  const float* w1 = w0 + QB * (D + 2);
  for (int i = threadIdx.x; i < QB * (D / 4); i += 256) {
    const int row = i / (D / 4), d = (i % (D / 4)) * 4, qi = qb * QB + row;
    if (qi >= q_len) continue;
    const float m0 = w0[QB * D + row], m1 = w1[QB * D + row];
    const float M = fmaxf(m0, m1);
    const float a0 = m0 == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m0 - M);
    const float a1 = m1 == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m1 - M);
    const float l = a0 * w0[QB * D + QB + row] + a1 * w1[QB * D + QB + row];
    const float inv = l > 0.f ? 1.0f / l : 0.f;  // a segment with no keys (both halves empty): zeros, as SDPA
    const f32x4 x0 = *(const f32x4*)(w0 + row * D + d), x1 = *(const f32x4*)(w1 + row * D + d);
    const int orow = a.orows ? a.orows[q_row0 + qi] : q_row0 + qi;
    bf16* p = a.o + (long)orow * a.os + h * D + d;
    bf16x4 o4;
#pragma unroll
    for (int j = 0; j < 4; ++j) o4[j] = f2bf((a0 * x0[j] + a1 * x1[j]) * inv);
    if (a.accumulate) {
      const bf16x4 ov = *(const bf16x4*)p;
#pragma unroll
      for (int j = 0; j < 4; ++j) o4[j] = f2bf(bf2f(ov[j]) + bf2f(o4[j]));
    }
    *(bf16x4*)p = o4;
  }
}
__global__ __launch_bounds__(256, 2) void attn_fwd_v6_w4_kernel(AttnArgs a) { attn_fwd_body<VRows, 4>(a); }
__global__ __launch_bounds__(512) void attn_fwd_v6t_kernel(AttnArgs a) { attn_fwd_body<VTrans, 8>(a); }
// the block-sparse launches of the two 8-wave kernels (sa_attn_fwd_sparse)
__global__ __launch_bounds__(512) void attn_fwd_v6_sparse_kernel(AttnSparseArgs a) {
  attn_fwd_body<VRows, 8, false, true>(a);
}
__global__ __launch_bounds__(512) void attn_fwd_v6t_sparse_kernel(AttnSparseArgs a) {
  attn_fwd_body<VTrans, 8, false, true>(a);
}

}  // namespace

// what the three self-attention entries check alike; vt: v is V^T (rows of whole 64-key blocks)
static bool self_attn_args_ok(const void* q, const void* k, const void* v, const void* o, const int32_t* segs, int nseg,
                              int max_q_len, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                              int64_t v_stride, int64_t o_stride, bool vt) {
  if (!q || !k || !v || !o || !segs || nseg <= 0 || max_q_len <= 0 || heads <= 0 || head_dim != D) return false;
  if ((q_stride | k_stride | v_stride | o_stride) % 8) return false;
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)o)) & 15) return false;
  return !(vt && (v_stride % 64 || (((uintptr_t)v) & 127)));
}
static AttnArgs make_args(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int64_t q_stride,
                          int64_t k_stride, int64_t v_stride, int64_t o_stride, float scale, int accumulate,
                          const int32_t* o_rows) {
  return AttnArgs{(const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)o, segs, q_stride, k_stride, v_stride,
                  o_stride, scale * 1.4426950408889634f, accumulate, o_rows};
}
// the kernels' dynamic LDS above the default limit: the initialiser of a function-local static (one-time, thread-safe)
static bool allow_lds(std::initializer_list<const void*> kernels, int bytes) {
  for (const void* f : kernels) (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  return true;
}

// kernel: 0 = auto, 1 = attn_fwd_v6_kernel (8 waves x 32 queries, mfma_f32_16x16x32_bf16), 2 = the 4-wave
// attn_fwd_v6_w4_kernel (two workgroups per CU).  Auto estimates both launches in rounds of one 8-wave
// workgroup per CU: a 4-wave round holds two workgroups per CU and runs 3 % slower per FLOP; a last 4-wave
// round of at most one workgroup per CU (one wave per SIMD) takes 0.75 of a round (measured,
// profiles/r02/attn_sp_shapes.json: the Ulysses N = 8 shape, 378 / 756 workgroups, 1.036 vs 0.927 ms).
// o_rows (optional, device int32 indexed by query row): query row r's output goes to row o_rows[r] of o --
// the sequence-parallel path writes this rank's own token chunk straight into the O-projection's input
// panels and the other chunks into their send slabs (stableavatar_amd/sp.py)
extern "C" int sa_attn_fwd_map(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                               int max_q_len, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                               int64_t v_stride, int64_t o_stride, float scale, int accumulate, int kernel,
                               const int32_t* o_rows, void* stream) {
  if (kernel < 0 || kernel > 3) return SA_ERR_ARG;
  if (!self_attn_args_ok(q, k, v, o, segs, nseg, max_q_len, heads, head_dim, q_stride, k_stride, v_stride, o_stride,
                         kernel == 3))
    return SA_ERR_ARG;
  static const bool attr = allow_lds({(const void*)attn_fwd_v6_kernel, (const void*)attn_fwd_v6_w4_kernel,
                                      (const void*)attn_fwd_v6t_kernel}, LDS_BYTES);
  (void)attr;
  const AttnArgs a = make_args(q, k, v, o, segs, q_stride, k_stride, v_stride, o_stride, scale, accumulate, o_rows);
  if (kernel == 0) {
    static int cus[64] = {0};  // per device, queried once
    int dev = 0, ncu = 256;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
      if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus[dev] = 256;
      ncu = cus[dev] > 0 ? cus[dev] : 256;
    }
    const long n8 = (long)nseg * heads * ((max_q_len + 255) / 256), n4 = (long)nseg * heads * ((max_q_len + 127) / 128);
    const long t8 = (n8 + ncu - 1) / ncu, full = n4 / (2 * ncu), rem = n4 % (2 * ncu);
    const double t4 = 1.03 * (full + (rem == 0 ? 0.0 : (rem <= ncu ? 0.75 : 1.0)));
    kernel = t4 < (double)t8 ? 2 : 1;
  }
  if (kernel == 2) {
    dim3 grid((max_q_len + 127) / 128, heads, nseg);
    hipLaunchKernelGGL(attn_fwd_v6_w4_kernel, grid, dim3(256), LDS_BYTES, (hipStream_t)stream, a);
  } else if (kernel == 3) {  // v = V^T [heads * 128][v_stride] (VTrans)
    dim3 grid((max_q_len + QB - 1) / QB, heads, nseg);
    hipLaunchKernelGGL(attn_fwd_v6t_kernel, grid, dim3(512), LDS_BYTES, (hipStream_t)stream, a);
  } else {
    dim3 grid((max_q_len + QB - 1) / QB, heads, nseg);
    hipLaunchKernelGGL(attn_fwd_v6_kernel, grid, dim3(512), LDS_BYTES, (hipStream_t)stream, a);
  }
  SA_LAUNCH_CHECK();
  return SA_OK;
}

// sa_attn_fwd_map over a block list per 256-query block (include/stableavatar_hip.h): kernel 0 and 1 run the row-major
// 8-wave body, 3 the V^T one; the 4-wave kernel 2 and the key-split launch have no sparse form
extern "C" int sa_attn_fwd_sparse(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                                  int max_q_len, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                                  int64_t v_stride, int64_t o_stride, float scale, int accumulate, int kernel,
                                  const int32_t* o_rows, const int32_t* blk_ptr, const int32_t* blk_idx, int n_qblocks,
                                  void* stream) {
  if (kernel != 0 && kernel != 1 && kernel != 3) return SA_ERR_ARG;
  if (!self_attn_args_ok(q, k, v, o, segs, nseg, max_q_len, heads, head_dim, q_stride, k_stride, v_stride, o_stride,
                         kernel == 3))
    return SA_ERR_ARG;
  if (!blk_ptr || !blk_idx || ((((uintptr_t)blk_ptr) | ((uintptr_t)blk_idx)) & 3)) return SA_ERR_ARG;
  if (n_qblocks != (max_q_len + QB - 1) / QB) return SA_ERR_ARG;
  static const bool attr =
      allow_lds({(const void*)attn_fwd_v6_sparse_kernel, (const void*)attn_fwd_v6t_sparse_kernel}, LDS_BYTES);
  (void)attr;
  const AttnSparseArgs a{make_args(q, k, v, o, segs, q_stride, k_stride, v_stride, o_stride, scale, accumulate, o_rows),
                         blk_ptr, blk_idx};
  const dim3 grid(n_qblocks, heads, nseg);
  if (kernel == 3) hipLaunchKernelGGL(attn_fwd_v6t_sparse_kernel, grid, dim3(512), LDS_BYTES, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(attn_fwd_v6_sparse_kernel, grid, dim3(512), LDS_BYTES, (hipStream_t)stream, a);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

extern "C" int sa_attn_fwd_split(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                                 int max_q_len, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                                 int64_t v_stride, int64_t o_stride, float scale, int accumulate, const int32_t* o_rows,
                                 int split_tiles, void* work, int64_t work_bytes, void* stream) {
  if (!self_attn_args_ok(q, k, v, o, segs, nseg, max_q_len, heads, head_dim, q_stride, k_stride, v_stride, o_stride,
                         false))
    return SA_ERR_ARG;
  const int nqb = (max_q_len + QB - 1) / QB;
  const long ntiles = (long)nseg * heads * nqb;
  if (split_tiles <= 0 || split_tiles > ntiles) return SA_ERR_ARG;
  if (!work || (((uintptr_t)work) & 15) || work_bytes < (int64_t)split_tiles * 2 * QB * (D + 2) * 4) return SA_ERR_ARG;
  static const bool attr = allow_lds({(const void*)attn_fwd_v6_split_kernel}, LDS_BYTES);
  (void)attr;
  AttnArgs a = make_args(q, k, v, o, segs, q_stride, k_stride, v_stride, o_stride, scale, accumulate, o_rows);
  a.nqb = nqb, a.nheads = heads, a.split_full = (int)(ntiles - split_tiles), a.split_n = split_tiles;
  a.work = (float*)work;
  hipLaunchKernelGGL(attn_fwd_v6_split_kernel, dim3((unsigned)(ntiles + split_tiles)), dim3(512), LDS_BYTES,
                     (hipStream_t)stream, a);
  SA_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_split_merge_kernel, dim3(split_tiles), dim3(256), 0, (hipStream_t)stream, a);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

extern "C" int sa_attn_fwd_ex(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                              int max_q_len, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                              int64_t v_stride, int64_t o_stride, float scale, int accumulate, int kernel,
                              void* stream) {
  return sa_attn_fwd_map(q, k, v, o, segs, nseg, max_q_len, heads, head_dim, q_stride, k_stride, v_stride, o_stride,
                         scale, accumulate, kernel, nullptr, stream);
}

extern "C" int sa_attn_fwd(const void* q, const void* k, const void* v, void* o, const int32_t* segs, int nseg,
                           int max_q_len, int heads, int head_dim, int64_t q_stride, int64_t k_stride,
                           int64_t v_stride, int64_t o_stride, float scale, int accumulate, void* stream) {
  return sa_attn_fwd_ex(q, k, v, o, segs, nseg, max_q_len, heads, head_dim, q_stride, k_stride, v_stride, o_stride,
                        scale, accumulate, 0, stream);
}

extern "C" int sa_attn_cross3(const void* q, int64_t q_stride, const void* kt, const void* vt, int64_t t_stride,
                              int t_len, const void* ki, const void* vi, int64_t i_stride, int i_len, const void* kv,
                              const void* vv, int64_t v_stride, int nper, int tokens_per_frame, int n_frames,
                              int tok_offset, void* o, int64_t o_stride, int batch, int q_len, int heads,
                              float scale, void* stream) {
  if (!q || !kt || !vt || !ki || !vi || !kv || !vv || !o) return SA_ERR_ARG;
  if (batch <= 0 || q_len <= 0 || heads <= 0 || t_len <= 0 || i_len <= 0 || nper <= 0 || n_frames <= 0)
    return SA_ERR_ARG;
  if (tokens_per_frame <= 0 || tokens_per_frame % QB != 0 || tok_offset < 0 || tok_offset % QB != 0 ||
      (long)n_frames * tokens_per_frame < (long)tok_offset + q_len)
    return SA_ERR_ARG;
  if ((q_stride | t_stride | i_stride | v_stride | o_stride) % 8) return SA_ERR_ARG;
  if ((((uintptr_t)q) | ((uintptr_t)kt) | ((uintptr_t)vt) | ((uintptr_t)ki) | ((uintptr_t)vi) | ((uintptr_t)kv) |
       ((uintptr_t)vv) | ((uintptr_t)o)) & 15)
    return SA_ERR_ARG;
  static const bool attr = allow_lds({(const void*)attn_cross3_kernel}, X3_LDS) &&
                           allow_lds({(const void*)attn_cross3_w4_kernel}, 4 * TILE_BYTES);
  (void)attr;
  Cross3Args a{(const bf16*)q, q_stride, (const bf16*)kt, (const bf16*)vt, t_stride, t_len, (const bf16*)ki,
               (const bf16*)vi, i_stride, i_len, (const bf16*)kv, (const bf16*)vv, v_stride, nper,
               tokens_per_frame, n_frames, tok_offset, (bf16*)o, o_stride, q_len, scale * 1.4426950408889634f};
  // 4-wave workgroups, two per CU (0.369-0.377 vs 0.390 ms per config-2 launch, same output; SA_X3_W4=0: 8 waves)
  const char* w4 = getenv("SA_X3_W4");
  if (!w4 || atoi(w4)) {
    dim3 grid((q_len + 127) / 128, heads, batch);
    hipLaunchKernelGGL(attn_cross3_w4_kernel, grid, dim3(256), 4 * TILE_BYTES, (hipStream_t)stream, a);
  } else {
    dim3 grid((q_len + QB - 1) / QB, heads, batch);
    hipLaunchKernelGGL(attn_cross3_kernel, grid, dim3(512), X3_LDS, (hipStream_t)stream, a);
  }
  SA_LAUNCH_CHECK();
  return SA_OK;
}
