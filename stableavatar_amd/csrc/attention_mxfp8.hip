// Self-attention on MXFP8 operands (opt-in fp8 attention mode; the default path stays on attention.hip).
// stableavatar_amd/mxfp8_attn.py is the definition: Q^ = quant(q * scale * log2 e) and K^ = quant(k - k_mean) along D,
// V^T quantised along the keys in the P^T operand's position order, P^ = e4m3(exp2(s - m) * 2^P_SHIFT),
// o = (P^ V^) / sum(P^).  Three kernels: sa_attn_kmean (column means of K per segment), sa_attn_pack_mxfp8 (the three
// operands, bit for bit the definition's; sa_attn_pack_k_mxfp8 is its K third alone, for the fp8 q/k/v mode whose
// GEMM and RoPE kernels write V^T and Q^ themselves) and sa_attn_fwd_mxfp8, the flash loop on
// v_mfma_scale_f32_16x16x128_f8f6f4 (lane map: gemm_mxfp8.hip).
//
// sa_attn_fwd_mxfp8: 8 waves x 32 queries as attention.hip's kernels, 128-key blocks.  S^T = K^ Q^T: one scaled MFMA
// per 16-key x 16-query tile (D = 128 is its whole reduction), the query on the lane, so the softmax is lane-local;
// the initial accumulator is P_SHIFT - m (m: the running maximum), so exp2 of the MFMA's output is P * 2^P_SHIFT.
// The lane's 32 scores per query tile pack (v_cvt_pk_fp8_f32) straight into the P^T operand of O^T = V^T P^T --
// key tile t is operand VGPR t -- which is why V^T is stored in that position order.  The row sum is one more MFMA
// against an all-ones operand, so it is the sum of the rounded P.  Deferred rescale: the running maximum moves only
// when a score passes it by more than LAG (P^ <= 2^(P_SHIFT + LAG) = 256 < 448).
// K^ and V^T tiles (128 rows x 128 B each, gemm.hip's swz128 image) and their scale dwords are staged by
// global_load ... lds into a 2-stage ring, one barrier per block; rows past kv_len are clamped to the last key (read
// again, masked to P = 0), so every load stays inside the operand.
//
// sa_attn_fwd_mxfp8_split: the same body with SPLIT set (attention.hip's key-split launch on this kernel).  Tiles are
// numbered (seg * heads + h) * nqb + qb; a 1-D grid whose first split_full workgroups run whole tiles exactly as
// above and whose last 2 x split_tiles are the two key halves of the last split_tiles tiles.  The halves meet at
// kper = ceil128(ceil(kv_len / 2)), so the second half's V^T columns start on a block boundary.  A half runs the same
// block loop over its keys and writes fp32 partials to its block of `work` instead of the output; block
// (split tile s, half) starts at float (2 s + half) * 256 * 130 and holds
//   O  [8][256][16]  unnormalised O of d tile dt, query row r of the tile, d = 16 dt + j (a wave's store of one d
//                    tile is 1 KB contiguous),
//   m  [256]         the running maximum the half used, P_SHIFT - cinit (it lags the half's true maximum by at most
//                    LAG; O and l are relative to it), -inf for a half with no keys,
//   l  [256]         the row sum of the rounded P (times 2^P_SHIFT, as O).
// attn_mx_split_merge_kernel: o = (w0 O0 + w1 O1) / (w0 l0 + w1 l1), w_h = exp2(m_h - max(m0, m1)), and w_h = 0
// for a half whose reported maximum stands more than FLUSH_GAP below the other's: its true maximum then stands
// more than 10 + P_SHIFT below the row's, the definition's drop rule (mxfp8_attn.attend_split).  No keys at all: zeros.
//
// sa_attn_fwd_mxfp8_o8 / sa_attn_fwd_mxfp8_split_o8 (the fp8 self-O mode): the same kernels with O8 set, a switch on
// the epilogue alone.  The output leaves as the MXFP8 operand of the O-projection -- the bf16-rounded O quantised
// along the row, bit for bit the bf16 entry point followed by sa_mxfp8_quant -- as bytes o_q [rows][ldo] and scale
// bytes o_scales [rows][ldos], byte 4 h + b for columns 128 h + 32 b .. of head h.  In the flash kernel lane
// (query r16, group g) holds O[dt][qt][e] = column 16 dt + 4 g + e, so block b of a query is d tiles 2 b and 2 b + 1
// over the four lanes r16 + 16 g, eight values a lane: round to bf16, the lane's amax, shfl_xor 16 and 32 for the
// block's, mx_quant8 (mxfp8.h's rule), one dword store per d tile at column 16 dt + 4 g; the lane with g = 0 writes
// the head's four scale bytes as one dword.  In the merge a thread holds four columns of a row, a block is eight
// adjacent threads (shfl_xor 1, 2, 4), and the block's first thread writes its scale byte.  Lanes that share a block
// share the query, so they skip rows at or past q_len together.  kv_len == 0: zero bytes, scale byte 127.
#include <type_traits>

#include "mxfp8.h"

namespace {

constexpr int D = 128;
constexpr int KVB = 128;                       // keys per block
constexpr int QBW = 256;                       // queries per workgroup: 8 waves x 32
constexpr int TILE_BYTES = KVB * D;            // 16 KB: K^ tile [key][d], V^T tile [d][position]
constexpr int STAGE_BYTES = 2 * TILE_BYTES;    // K | V
constexpr int RING_BYTES = 2 * STAGE_BYTES;    // 64 KB
constexpr int SCALE_STAGE = 2 * KVB * 4;       // 1 KB: K scale dwords by key, V^T scale dwords by d
constexpr int LDS_TOTAL = RING_BYTES + 2 * SCALE_STAGE;
constexpr float P_SHIFT = 4.0f, LAG = 4.0f;    // mxfp8_attn.py
// a move of the running maximum by more than this drops what was accumulated: every key seen so far has
// s <= m_old + LAG, so against the final maximum its P * 2^P_SHIFT < 2^-10 and the definition rounds it to zero
constexpr float FLUSH_GAP = 10.0f + P_SHIFT + LAG;
constexpr int P_SCALE_BYTE = 127 - (int)P_SHIFT;
constexpr uint32_t ONES_E4M3 = 0x38383838u;    // four e4m3 1.0

typedef int __attribute__((ext_vector_type(8))) i32x8;

struct FwdArgs {
  const uint8_t* qq; const uint8_t* qs;
  const uint8_t* kq; const uint8_t* ks;
  const uint8_t* vq; const uint8_t* vs;
  long Rv;
  bf16* o; long os;
  const int* segs; const int* vcol0; const int* orows;
  int heads;
};
// O8: o / os are the operand's bytes and their row stride in bytes; sc / lds the scale bytes and their row stride.
// (A type of its own for the O8 instantiations, so the kernel arguments of the others stay where they were.)
struct FwdArgs8 : FwdArgs {
  uint8_t* sc; long lds;
};
template <bool O8>
using FwdArgsOf = std::conditional_t<O8, FwdArgs8, FwdArgs>;
// the key-split launch (the header comment): tile decode and the partials
struct SplitArgs {
  int nqb, split_full;  // query blocks per (segment, head); the number of whole tiles
  float* work;
};
constexpr int WBLK = QBW * (D + 2);  // floats per (split tile, half)

template <int OFF>
__device__ __forceinline__ void ds_u8(uint32_t& d, uint32_t addr) {
  asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
__device__ __forceinline__ i32x8 join(const u32x4& lo, const u32x4& hi) {
  return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
// c += a (16 rows on the accumulator's 4 g + e axis) x b (16 rows on the lane axis), e4m3, scale byte 0 of sa / sb
__device__ __forceinline__ f32x4 mma(const i32x8& a, const i32x8& b, const f32x4& c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, sa, 0, sb);
}

// the fragments of four 16-row tiles T0 .. T0 + 3 of a staged tile (rows 16 t + r16, 16-byte chunks g and 4 + g) and
// byte g of the rows' scale dwords (the lane group's block, read as a byte so that it sits in byte 0); waited for here
template <int T0>
__device__ __forceinline__ void read4(u32x4 (&lo)[4], u32x4 (&hi)[4], uint32_t (&sc)[4], uint32_t a_lo, uint32_t a_hi,
                                      uint32_t a_sc) {
  ds_b128<(T0 + 0) * 2048>(lo[0], a_lo); ds_b128<(T0 + 0) * 2048>(hi[0], a_hi); ds_u8<(T0 + 0) * 64>(sc[0], a_sc);
  ds_b128<(T0 + 1) * 2048>(lo[1], a_lo); ds_b128<(T0 + 1) * 2048>(hi[1], a_hi); ds_u8<(T0 + 1) * 64>(sc[1], a_sc);
  ds_b128<(T0 + 2) * 2048>(lo[2], a_lo); ds_b128<(T0 + 2) * 2048>(hi[2], a_hi); ds_u8<(T0 + 2) * 64>(sc[2], a_sc);
  ds_b128<(T0 + 3) * 2048>(lo[3], a_lo); ds_b128<(T0 + 3) * 2048>(hi[3], a_hi); ds_u8<(T0 + 3) * 64>(sc[3], a_sc);
  // the wait "writes" every register the reads fill, so nothing that uses them moves above it
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]),
                 "+v"(sc[0]), "+v"(sc[1]), "+v"(sc[2]), "+v"(sc[3])::"memory");
}

// (a template on the kernel itself: called as an inlined body from two wrappers, as attention.hip's split is, the
// compiler schedules the unsplit instantiation differently; this way its instruction stream is what it was)
template <bool SPLIT, bool O8>
__global__ __launch_bounds__(512) void attn_fwd_mx_kernel(FwdArgsOf<O8> a, SplitArgs sp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int qb, h, seg, half = -1, stile = 0;
  if constexpr (SPLIT) {
    int tile;
    if ((int)blockIdx.x < sp.split_full) {
      tile = xcd_remap(blockIdx.x, sp.split_full);
    } else {
      const int idx = blockIdx.x - sp.split_full;
      stile = idx >> 1;
      half = idx & 1;
      tile = sp.split_full + stile;
    }
    qb = tile % sp.nqb;
    h = (tile / sp.nqb) % a.heads;
    seg = tile / (sp.nqb * a.heads);
  } else {
    const int nx = gridDim.x, ny = gridDim.y;
    const int flat = xcd_remap(blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z), nx * ny * gridDim.z);
    qb = flat % nx, h = (flat / nx) % ny, seg = flat / (nx * ny);
  }
  const int* sg = a.segs + seg * 4;
  const int q_row0 = sg[0], q_len = sg[1];
  int kv_row0 = sg[2], kv_len = sg[3];
  if (qb * QBW >= q_len) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int C = a.heads * D, CS = a.heads * 4;  // row bytes of Q^ / K^, of their scales
  long vc0 = a.vcol0[seg];
  float* const wblk = SPLIT && half >= 0 ? sp.work + ((long)stile * 2 + half) * WBLK : nullptr;
  if (SPLIT && half >= 0) {
    // a segment whose V^T columns leave the operand is skipped whole (the merge skips it too)
    if (kv_len > 0 && (vc0 < 0 || vc0 + ((long)kv_len + KVB - 1) / KVB * KVB > a.Rv)) return;
    const int kper = ((kv_len + 1) / 2 + KVB - 1) / KVB * KVB;  // this half's keys: whole blocks in the first half
    if (half == 0) {
      kv_len = min(kv_len, kper);
    } else {
      kv_row0 += kper;
      kv_len -= kper;
      vc0 += kper;
    }
    if (kv_len <= 0) {  // a half with no keys: m = -inf, l = 0, O = 0
      for (int i = tid; i < QBW * D; i += 512) wblk[i] = 0.f;
      if (tid < QBW) {
        wblk[QBW * D + tid] = -__builtin_inff();
        wblk[QBW * D + QBW + tid] = 0.f;
      }
      return;
    }
  }
  const int nkb = (kv_len + KVB - 1) / KVB;
  if (kv_len <= 0) {
    if constexpr (O8) {  // all-zero blocks: zero bytes (dword stores, as the epilogue's), scale byte 127
      for (int i = tid; i < QBW * (D / 4); i += 512) {
        const int qi = qb * QBW + i / (D / 4);
        if (qi < q_len) {
          const long orow = a.orows ? a.orows[q_row0 + qi] : q_row0 + qi;
          *(uint32_t*)((uint8_t*)a.o + orow * a.os + h * D + (i % (D / 4)) * 4) = 0u;
          if (i % (D / 4) == 0) *(uint32_t*)(a.sc + orow * a.lds + h * 4) = 0x7f7f7f7fu;
        }
      }
      return;
    }
    for (int i = tid; i < QBW * (D / 8); i += 512) {
      const int qi = qb * QBW + i / (D / 8);
      if (qi < q_len) {
        const int orow = a.orows ? a.orows[q_row0 + qi] : q_row0 + qi;
        *(u32x4*)(a.o + (long)orow * a.os + h * D + (i % (D / 8)) * 8) = (u32x4){0u, 0u, 0u, 0u};
      }
    }
    return;
  }
  if (vc0 < 0 || vc0 + (long)nkb * KVB > a.Rv) return;  // the segment's V^T columns must lie inside the operand
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r16 = lane & 15;
  const int sh = 8 * g;  // Q^'s scale dword comes from global memory: its byte g shifted down once

  // Q^ fragments (the B operand of S^T = K^ Q^T): query r16 of tile qt, chunks g and 4 + g, scale byte g
  i32x8 qf[2];
  int qsc[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const long row = q_row0 + min(qb * QBW + wave * 32 + qt * 16 + r16, q_len - 1);
    const uint8_t* qp = a.qq + row * C + h * D;
    qf[qt] = join(*(const u32x4*)(qp + 16 * g), *(const u32x4*)(qp + 64 + 16 * g));
    qsc[qt] = (int)(*(const uint32_t*)(a.qs + row * CS + h * 4) >> sh);
  }

  // staging: a tile is 16 pieces of 1 KB (8 rows x 128 B), two per wave; lane l of a piece writes LDS bytes 16 l..
  // and so reads row l / 8, chunk (l % 8) ^ swizzle.  The scale dwords: waves 0-1 the 128 keys', waves 2-3 the 128
  // d-rows' (one dword = the row's four blocks of this tile)
  const uint8_t* kbase = a.kq + (long)kv_row0 * C + h * D;
  const uint8_t* vbase = a.vq + (long)h * D * a.Rv + vc0;
  const uint8_t* ksbase = a.ks + (long)kv_row0 * CS + h * 4;
  const uint8_t* vsbase = a.vs + (long)h * D * (a.Rv / 32) + vc0 / 32;
  auto issue = [&](int kb) {
    char* st = smem + (kb & 1) * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int p = i * 8 + wave;
      const int row = p * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ ((row >> 1) & 7);
      const long key = min(kb * KVB + row, kv_len - 1);
      __builtin_amdgcn_global_load_lds((const void*)(kbase + key * C + chunk * 16), LDS_PTR(st + p * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(vbase + (long)row * a.Rv + kb * KVB + chunk * 16),
                                       LDS_PTR(st + TILE_BYTES + p * 1024), 16, 0, 0);
    }
    if (wave < 4) {
      char* dst = smem + RING_BYTES + (kb & 1) * SCALE_STAGE + wave * 256;
      const int row = (wave & 1) * 64 + lane;
      const uint8_t* src = wave < 2 ? ksbase + (long)min(kb * KVB + row, kv_len - 1) * CS
                                    : vsbase + (long)row * (a.Rv / 32) + kb * (KVB / 32);
      __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(dst), 4, 0, 0);
    }
  };

  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
  const uint32_t swz = (r16 >> 1) & 7;
  const uint32_t f_lo = lds0 + r16 * 128 + ((g ^ swz) << 4), f_hi = lds0 + r16 * 128 + (((4 + g) ^ swz) << 4);
  const uint32_t f_sc = lds0 + RING_BYTES + r16 * 4 + g;

  f32x4 O[8][2], L[2];
  float cinit[2] = {P_SHIFT, P_SHIFT};  // P_SHIFT - m, m the running maximum
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    L[qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) O[dt][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const i32x8 ones = {(int)ONES_E4M3, (int)ONES_E4M3, (int)ONES_E4M3, (int)ONES_E4M3,
                      (int)ONES_E4M3, (int)ONES_E4M3, (int)ONES_E4M3, (int)ONES_E4M3};

  issue(0);
  for (int kb = 0; kb < nkb; ++kb) {
    // block kb has landed (every wave waits for its own pieces, then the barrier), and every wave is done reading
    // the other stage (block kb - 1), which block kb + 1 now overwrites
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kb + 1 < nkb) issue(kb + 1);
    const uint32_t so = (kb & 1) * STAGE_BYTES, ss = (kb & 1) * SCALE_STAGE;

    // scores: S[t][qt][e] = key 16 t + 4 g + e of the block, query r16 of tile qt, less m, plus P_SHIFT
    f32x4 S[8][2];
    {
      u32x4 lo[4], hi[4];
      uint32_t sc[4];
      const f32x4 c0 = {cinit[0], cinit[0], cinit[0], cinit[0]}, c1 = {cinit[1], cinit[1], cinit[1], cinit[1]};
      read4<0>(lo, hi, sc, f_lo + so, f_hi + so, f_sc + ss);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const i32x8 kf = join(lo[t], hi[t]);
        S[t][0] = mma(kf, qf[0], c0, (int)sc[t], qsc[0]);
        S[t][1] = mma(kf, qf[1], c1, (int)sc[t], qsc[1]);
      }
      read4<4>(lo, hi, sc, f_lo + so, f_hi + so, f_sc + ss);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const i32x8 kf = join(lo[t], hi[t]);
        S[4 + t][0] = mma(kf, qf[0], c0, (int)sc[t], qsc[0]);
        S[4 + t][1] = mma(kf, qf[1], c1, (int)sc[t], qsc[1]);
      }
    }
    if (kb == nkb - 1 && (kv_len % KVB) != 0) {  // the ragged last block: keys at or past kv_len take P = 0
      const int k0 = kb * KVB + 4 * g;
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k0 + 16 * t + e >= kv_len) S[t][0][e] = S[t][1][e] = -__builtin_inff();
    }

    // the lane's maximum per query; the running maximum moves (for the whole wave) in the first block and when
    // some score passes it by more than LAG
    float lm[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float m4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        m4[e] = vmax3(vmax3(S[0][qt][e], S[1][qt][e], S[2][qt][e]), vmax3(S[3][qt][e], S[4][qt][e], S[5][qt][e]),
                      __builtin_elementwise_maximum(S[6][qt][e], S[7][qt][e]));
      lm[qt] = vmax3(__builtin_elementwise_maximum(m4[0], m4[1]), m4[2], m4[3]);
    }
    const bool first = kb == 0;
    if (first || __builtin_amdgcn_ballot_w64(fmaxf(lm[0], lm[1]) > P_SHIFT + LAG) != 0) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        float mx = lm[qt];
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float gap = mx - P_SHIFT;  // how far the row's maximum stands above the running one
        gap = (first || gap > 0.f) ? gap : 0.f;
        const float f = first ? 1.0f : (gap > FLUSH_GAP ? 0.f : __builtin_amdgcn_exp2f(-gap));
        cinit[qt] -= gap;
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) S[t][qt][e] -= gap;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
#pragma unroll
          for (int e = 0; e < 4; ++e) O[dt][qt][e] *= f;
#pragma unroll
        for (int e = 0; e < 4; ++e) L[qt][e] *= f;
      }
    }

    // P^ = e4m3(exp2(S)) in operand order: key tile t is VGPR t of the P^T operand
    i32x8 pb[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int t = 0; t < 8; ++t)
        pb[qt][t] = (int)mx_pack4(__builtin_amdgcn_exp2f(S[t][qt][0]), __builtin_amdgcn_exp2f(S[t][qt][1]),
                                  __builtin_amdgcn_exp2f(S[t][qt][2]), __builtin_amdgcn_exp2f(S[t][qt][3]));
    L[0] = mma(ones, pb[0], L[0], 127, P_SCALE_BYTE);
    L[1] = mma(ones, pb[1], L[1], 127, P_SCALE_BYTE);

    // O^T += V^T P^T: d tile dt, d = 16 dt + 4 g + e on the accumulator, the query on the lane
    {
      u32x4 lo[4], hi[4];
      uint32_t sc[4];
      read4<0>(lo, hi, sc, f_lo + so + TILE_BYTES, f_hi + so + TILE_BYTES, f_sc + ss + KVB * 4);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const i32x8 vf = join(lo[t], hi[t]);
        O[t][0] = mma(vf, pb[0], O[t][0], (int)sc[t], P_SCALE_BYTE);
        O[t][1] = mma(vf, pb[1], O[t][1], (int)sc[t], P_SCALE_BYTE);
      }
      read4<4>(lo, hi, sc, f_lo + so + TILE_BYTES, f_hi + so + TILE_BYTES, f_sc + ss + KVB * 4);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const i32x8 vf = join(lo[t], hi[t]);
        O[4 + t][0] = mma(vf, pb[0], O[4 + t][0], (int)sc[t], P_SCALE_BYTE);
        O[4 + t][1] = mma(vf, pb[1], O[4 + t][1], (int)sc[t], P_SCALE_BYTE);
      }
    }
  }

  if (SPLIT && half >= 0) {  // partials: this lane's d = 16 dt + 4 g + e of query row `row`, the row's max and sum
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int row = wave * 32 + qt * 16 + r16;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) *(f32x4*)(wblk + (dt * QBW + row) * 16 + 4 * g) = O[dt][qt];
      if (g == 0) {
        wblk[QBW * D + row] = P_SHIFT - cinit[qt];
        wblk[QBW * D + QBW + row] = L[qt][0];
      }
    }
    return;
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int qi = qb * QBW + wave * 32 + qt * 16 + r16;
    if (qi >= q_len) continue;
    const float inv = 1.0f / L[qt][0];
    const int qrow = q_row0 + qi;
    const int orow = a.orows ? a.orows[qrow] : qrow;
    if constexpr (O8) {  // the header comment: the four lanes r16 + 16 g of a query all get here or none does
      uint8_t* op = (uint8_t*)a.o + (long)orow * a.os + h * D + 4 * g;
      uint32_t sc4 = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = bf2f(f2bf(O[2 * b + (j >> 2)][qt][j & 3] * inv));
        float amax = mx_amax8(v);
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        uint32_t s;
        const u32x2 w = mx_quant8(v, amax, &s);
        *(uint32_t*)(op + 32 * b) = w[0];
        *(uint32_t*)(op + 32 * b + 16) = w[1];
        sc4 |= s << (8 * b);
      }
      if (g == 0) *(uint32_t*)(a.sc + (long)orow * a.lds + h * 4) = sc4;
    } else {
      bf16* op = a.o + (long)orow * a.os + h * D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) {
        const f32x4& v = O[dt][qt];
        *(bf16x4*)(op + dt * 16) = (bf16x4){f2bf(v[0] * inv), f2bf(v[1] * inv), f2bf(v[2] * inv), f2bf(v[3] * inv)};
      }
    }
  }
}

// the two key halves of each split tile -> the output (the header comment).  A thread takes four d of a row: 32
// threads a row, so a wave reads 128 contiguous bytes of each half's d tile and writes two 256-byte rows
template <bool O8>
__global__ __launch_bounds__(256) void attn_mx_split_merge_kernel(FwdArgsOf<O8> a, SplitArgs sp) {
  const int stile = blockIdx.x, tile = sp.split_full + stile;
  const int qb = tile % sp.nqb, h = (tile / sp.nqb) % a.heads, seg = tile / (sp.nqb * a.heads);
  const int* sg = a.segs + seg * 4;
  const int q_row0 = sg[0], q_len = sg[1], kv_len = sg[3];
  if (qb * QBW >= q_len) return;
  const long vc0 = a.vcol0[seg];
  if (kv_len > 0 && (vc0 < 0 || vc0 + ((long)kv_len + KVB - 1) / KVB * KVB > a.Rv)) return;  // skipped, as the halves
  const float* w0 = sp.work + (long)stile * 2 * WBLK;
  const float* w1 = w0 + WBLK;
  for (int i = threadIdx.x; i < QBW * (D / 4); i += 256) {
    const int row = i / (D / 4), c = i % (D / 4), qi = qb * QBW + row;
    if (qi >= q_len) continue;  // a row is 32 threads: the eight threads of an O8 block skip together
    u32x2 out = {0u, 0u};
    if (kv_len > 0) {
      const float m0 = w0[QBW * D + row], m1 = w1[QBW * D + row];
      const float M = fmaxf(m0, m1);  // finite: the first half has a key
      const float a0 = M - m0 > FLUSH_GAP ? 0.f : __builtin_amdgcn_exp2f(m0 - M);
      const float a1 = M - m1 > FLUSH_GAP ? 0.f : __builtin_amdgcn_exp2f(m1 - M);  // m1 = -inf: an empty half
      const float inv = 1.0f / (a0 * w0[QBW * D + QBW + row] + a1 * w1[QBW * D + QBW + row]);
      const int off = ((c >> 2) * QBW + row) * 16 + 4 * (c & 3);
      const f32x4 x0 = *(const f32x4*)(w0 + off), x1 = *(const f32x4*)(w1 + off);
      const bf16x4 o4 = {f2bf((a0 * x0[0] + a1 * x1[0]) * inv), f2bf((a0 * x0[1] + a1 * x1[1]) * inv),
                         f2bf((a0 * x0[2] + a1 * x1[2]) * inv), f2bf((a0 * x0[3] + a1 * x1[3]) * inv)};
      out = __builtin_bit_cast(u32x2, o4);
    }
    const int orow = a.orows ? a.orows[q_row0 + qi] : q_row0 + qi;
    if constexpr (O8) {  // the bf16 values quantised; no key at all: zeros, an all-zero block (scale byte 127)
      const bf16x4 o4 = __builtin_bit_cast(bf16x4, out);
      const float v0 = bf2f(o4[0]), v1 = bf2f(o4[1]), v2 = bf2f(o4[2]), v3 = bf2f(o4[3]);
      float amax = fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3)));
      amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
      const uint32_t s = mx_scale_byte(amax);
      const float k = mx_inv_scale(s);
      *(uint32_t*)((uint8_t*)a.o + (long)orow * a.os + h * D + 4 * c) = mx_pack4(v0 * k, v1 * k, v2 * k, v3 * k);
      if ((c & 7) == 0) a.sc[(long)orow * a.lds + h * 4 + (c >> 3)] = (uint8_t)s;
    } else {
      *(u32x2*)(a.o + (long)orow * a.os + h * D + 4 * c) = out;
    }
  }
}

// ---------------------------------------------------------------------------------------------- K column means

// two passes, no atomics, so a fixed launch gives fixed bits.  Pass 1, one workgroup per (head, segment, one of
// KM_SPLIT row ranges): a lane sums 8 adjacent columns of every 16th row of the range (4 waves x 4 rows per step,
// 16-byte loads), the 16 partial sums are added in a fixed order and written to work[seg][split][column].  Pass 2
// adds the KM_SPLIT partials in order and divides by kv_len.
constexpr int KM_SPLIT = 16;
__global__ __launch_bounds__(256) void attn_kmean_part_kernel(const bf16* k, long ks, const int* segs, int heads,
                                                              float* work) {
  __shared__ float part[16][D];
  const int h = blockIdx.x, seg = blockIdx.y, sp = blockIdx.z;
  const int kv_row0 = segs[seg * 4 + 2], kv_len = segs[seg * 4 + 3];
  const int per = (kv_len + KM_SPLIT - 1) / KM_SPLIT;
  const int r0 = sp * per, r1 = min(kv_len, r0 + per);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = wave * 4 + (lane >> 4), c = (lane & 15) * 8;
  const bf16* p = k + (long)kv_row0 * ks + h * D + c;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + slot; r < r1; r += 16) {
    const bf16x8 x = *(const bf16x8*)(p + (long)r * ks);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] += bf2f(x[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[slot][c + j] = s[j];
  __syncthreads();
  if (threadIdx.x < D) {
    float t = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < 16; ++w) t += part[w][threadIdx.x];
    work[((long)(seg * KM_SPLIT + sp) * heads + h) * D + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void attn_kmean_final_kernel(const float* work, const int* segs, int heads,
                                                               float* out) {
  const int seg = blockIdx.y, C = heads * D;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int kv_len = segs[seg * 4 + 3];
  float t = work[(long)seg * KM_SPLIT * C + c];
#pragma unroll
  for (int sp = 1; sp < KM_SPLIT; ++sp) t += work[((long)seg * KM_SPLIT + sp) * C + c];
  out[(long)seg * C + c] = kv_len > 0 ? t / (float)kv_len : 0.f;
}

// ---------------------------------------------------------------------------------------------- operand pack

struct PackArgs {
  const bf16* q; long qs;
  const bf16* k; long ks;
  const bf16* v; long vs;
  const int* segs; const int* vcol0;
  const float* kmean;
  float c;
  uint8_t* qq; uint8_t* qsc;
  uint8_t* kq; uint8_t* ksc;
  uint8_t* vq; uint8_t* vsc;
  long Rv;
  int heads;
  int only_k;  // sa_attn_pack_k_mxfp8: the grid has no query half
};

// Q^ and K^: one wave per row, 8 elements per lane per 512-column chunk, a block is four adjacent lanes (as
// mxfp8_quant_kernel); blockIdx.z = 0 the segment's query rows, 1 its key rows (only_k: the key rows alone)
__global__ __launch_bounds__(256) void attn_pack_qk_kernel(PackArgs a) {
  const int seg = blockIdx.y, isk = a.only_k ? 1 : blockIdx.z;
  const int* sg = a.segs + seg * 4;
  const int row0 = sg[isk ? 2 : 0], len = sg[isk ? 3 : 1];
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= len) return;
  const int C = a.heads * D;
  const long row = row0 + r;
  const bf16* x = (isk ? a.k + row * a.ks : a.q + row * a.qs);
  uint8_t* oq = (isk ? a.kq : a.qq) + row * C;
  uint8_t* osc = (isk ? a.ksc : a.qsc) + row * (C / 32);
  const float* mean = (isk && a.kmean) ? a.kmean + (long)seg * C : nullptr;
  for (int c0 = lane * 8; c0 < C; c0 += 512) {
    const bf16x8 xv = *(const bf16x8*)(x + c0);
    float v[8];
    if (isk) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = mean ? bf2f(xv[j]) - mean[c0 + j] : bf2f(xv[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = bf2f(xv[j]) * a.c;
    }
    float amax = mx_amax8(v);
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    uint32_t s;
    const u32x2 q = mx_quant8(v, amax, &s);
    *(u32x2*)(oq + c0) = q;
    if ((lane & 3) == 0) osc[c0 / 32] = (uint8_t)s;
  }
}

// V^T: one workgroup per (128-key block, head, segment).  The block's V rows go to LDS (keys at or past kv_len as
// zeros); wave b then takes quantisation block b (positions 32 b .. 32 b + 31 of every d-row), lane l the d-rows 2 l
// and 2 l + 1: position 64 hi + 16 g + 4 t + e holds key 16 (4 hi + t) + 4 g + e (mxfp8_attn.KEY_OF_POS), so each of
// the wave's 32 LDS reads takes one key's 128 d as 64 dwords (conflict-free)
constexpr int VP_LD = D + 8;
__global__ __launch_bounds__(256) void attn_pack_vt_kernel(PackArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 tile[KVB][VP_LD];
  const int kblk = blockIdx.x, h = blockIdx.y, seg = blockIdx.z;
  const int kv_row0 = a.segs[seg * 4 + 2], kv_len = a.segs[seg * 4 + 3];
  if (kblk * KVB >= kv_len) return;
  const long col0 = (long)a.vcol0[seg] + (long)kblk * KVB;
  if (a.vcol0[seg] < 0 || col0 + KVB > a.Rv) return;  // outside the operand: nothing is written
  const int tid = threadIdx.x;
  for (int i = tid; i < KVB * (D / 8); i += 256) {
    const int key = i / (D / 8), ch = i % (D / 8);
    u32x4 x = {0u, 0u, 0u, 0u};
    if (kblk * KVB + key < kv_len)
      x = *(const u32x4*)(a.v + (long)(kv_row0 + kblk * KVB + key) * a.vs + h * D + ch * 8);
    *(u32x4*)&tile[key][ch * 8] = x;
  }
  __syncthreads();
  const int b = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int hi = b >> 1, g0 = 2 * (b & 1);
  float v[2][32];
#pragma unroll
  for (int p = 0; p < 32; ++p) {
    const int key = 16 * (4 * hi + ((p >> 2) & 3)) + 4 * (g0 + (p >> 4)) + (p & 3);
    const bf16x2 x = *(const bf16x2*)&tile[key][2 * lane];
    v[0][p] = bf2f(x[0]);
    v[1][p] = bf2f(x[1]);
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int d = 2 * lane + r;
    float amax = 0.f;
#pragma unroll
    for (int p = 0; p < 32; ++p) amax = fmaxf(amax, fabsf(v[r][p]));
    uint32_t s = 0;
    u32x2 w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = mx_quant8(v[r] + 8 * j, amax, &s);
    uint8_t* oq = a.vq + (long)(h * D + d) * a.Rv + col0 + 32 * b;
    *(u32x4*)oq = (u32x4){w[0][0], w[0][1], w[1][0], w[1][1]};
    *(u32x4*)(oq + 16) = (u32x4){w[2][0], w[2][1], w[3][0], w[3][1]};
    a.vsc[(long)(h * D + d) * (a.Rv / 32) + col0 / 32 + b] = (uint8_t)s;
  }
}

}  // namespace

extern "C" int sa_attn_kmean(const void* k, int64_t k_stride, const int32_t* segs, int nseg, int heads, int head_dim,
                             float* k_mean, float* work, void* stream) {
  if (!k || !segs || !k_mean || !work || nseg <= 0 || heads <= 0 || head_dim != D) return SA_ERR_ARG;
  if (k_stride < (int64_t)heads * D || k_stride % 8 || (((uintptr_t)k) & 15)) return SA_ERR_ARG;  // 16-byte loads
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_kmean_part_kernel, dim3(heads, nseg, KM_SPLIT), dim3(256), 0, st, (const bf16*)k,
                     (long)k_stride, segs, heads, work);
  SA_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_kmean_final_kernel, dim3((heads * D + 255) / 256, nseg), dim3(256), 0, st,
                     (const float*)work, segs, heads, k_mean);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

extern "C" int sa_attn_pack_mxfp8(const void* q, int64_t q_stride, const void* k, int64_t k_stride, const void* v,
                                  int64_t v_stride, const int32_t* segs, const int32_t* vcol0, int nseg, int max_q_len,
                                  int max_kv_len, int heads, int head_dim, float scale, const float* k_mean, void* q_out,
                                  void* q_scales, void* k_out, void* k_scales, void* vt_out, void* vt_scales,
                                  int64_t Rv, void* stream) {
  if (!q || !k || !v || !segs || !vcol0 || !q_out || !q_scales || !k_out || !k_scales || !vt_out || !vt_scales)
    return SA_ERR_ARG;
  if (nseg <= 0 || heads <= 0 || head_dim != D || max_q_len < 0 || max_kv_len < 0) return SA_ERR_ARG;
  const int64_t C = (int64_t)heads * D;
  // 16-byte row loads of q, k, v
  if (q_stride < C || k_stride < C || v_stride < C || q_stride % 8 || k_stride % 8 || v_stride % 8) return SA_ERR_ARG;
  if ((((uintptr_t)q) & 15) || (((uintptr_t)k) & 15) || (((uintptr_t)v) & 15)) return SA_ERR_ARG;
  if (Rv <= 0 || Rv % KVB) return SA_ERR_ARG;
  if ((((uintptr_t)q_out) & 15) || (((uintptr_t)k_out) & 15) || (((uintptr_t)vt_out) & 15)) return SA_ERR_ARG;
  if (k_mean && (((uintptr_t)k_mean) & 3)) return SA_ERR_ARG;
  PackArgs a{(const bf16*)q, q_stride, (const bf16*)k, k_stride, (const bf16*)v, v_stride, segs, vcol0, k_mean,
             scale * 1.4426950408889634f, (uint8_t*)q_out, (uint8_t*)q_scales, (uint8_t*)k_out, (uint8_t*)k_scales,
             (uint8_t*)vt_out, (uint8_t*)vt_scales, Rv, heads, 0};
  hipStream_t st = (hipStream_t)stream;
  const int rows = max_q_len > max_kv_len ? max_q_len : max_kv_len;
  if (rows > 0) {
    hipLaunchKernelGGL(attn_pack_qk_kernel, dim3((rows + 3) / 4, nseg, 2), dim3(256), 0, st, a);
    SA_LAUNCH_CHECK();
  }
  if (max_kv_len > 0) {
    hipLaunchKernelGGL(attn_pack_vt_kernel, dim3((max_kv_len + KVB - 1) / KVB, heads, nseg), dim3(256), 0, st, a);
    SA_LAUNCH_CHECK();
  }
  return SA_OK;
}

extern "C" int sa_attn_pack_k_mxfp8(const void* k, int64_t k_stride, const int32_t* segs, int nseg, int max_kv_len,
                                    int heads, const float* k_mean, void* k_out, void* k_scales, void* stream) {
  if (!k || !segs || !k_out || !k_scales || nseg <= 0 || heads <= 0 || max_kv_len < 0) return SA_ERR_ARG;
  const int64_t C = (int64_t)heads * D;
  if (k_stride < C || k_stride % 8 || (((uintptr_t)k) & 15) || (((uintptr_t)k_out) & 15)) return SA_ERR_ARG;
  if (k_mean && (((uintptr_t)k_mean) & 3)) return SA_ERR_ARG;
  PackArgs a{nullptr, 0, (const bf16*)k, k_stride, nullptr, 0, segs, nullptr, k_mean, 0.f, nullptr, nullptr,
             (uint8_t*)k_out, (uint8_t*)k_scales, nullptr, nullptr, 0, heads, 1};
  if (max_kv_len > 0) {
    hipLaunchKernelGGL(attn_pack_qk_kernel, dim3((max_kv_len + 3) / 4, nseg, 1), dim3(256), 0, (hipStream_t)stream, a);
    SA_LAUNCH_CHECK();
  }
  return SA_OK;
}

// the argument checks the four flash entry points share (16-byte operand loads, dword scale loads)
static bool fwd_operands_ok(const void* q, const void* q_scales, const void* k, const void* k_scales, const void* vt,
                            const void* vt_scales, int64_t Rv, const int32_t* segs, const int32_t* vcol0, int nseg,
                            int max_q_len, int heads, int head_dim) {
  if (!q || !q_scales || !k || !k_scales || !vt || !vt_scales || !segs || !vcol0) return false;
  if (nseg <= 0 || heads <= 0 || head_dim != D || max_q_len <= 0) return false;
  if (Rv <= 0 || Rv % KVB) return false;
  if ((((uintptr_t)q) & 15) || (((uintptr_t)k) & 15) || (((uintptr_t)vt) & 15)) return false;
  if ((((uintptr_t)q_scales) & 3) || (((uintptr_t)k_scales) & 3) || (((uintptr_t)vt_scales) & 3)) return false;
  return true;
}
// the bf16 output: 8- and 16-byte stores
static bool fwd_out_ok(const void* o, int64_t o_stride, int heads) {
  return o && o_stride >= (int64_t)heads * D && o_stride % 8 == 0 && !(((uintptr_t)o) & 15);
}
// the MXFP8 output: dword stores of bytes and of a head's four scale bytes
static bool fwd_out8_ok(const void* o_q, int64_t ldo, const void* o_scales, int64_t ldos, int heads) {
  if (!o_q || !o_scales || ldo < (int64_t)heads * D || ldos < (int64_t)heads * 4 || ldo % 4 || ldos % 4) return false;
  return !(((uintptr_t)o_q) & 3) && !(((uintptr_t)o_scales) & 3);
}

template <bool O8>
static int fwd_launch(const FwdArgsOf<O8>& a, int nseg, int max_q_len, void* stream) {
  static const bool attr = [] {
    (void)hipFuncSetAttribute((const void*)attn_fwd_mx_kernel<false, O8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              LDS_TOTAL);
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL((attn_fwd_mx_kernel<false, O8>), dim3((max_q_len + QBW - 1) / QBW, a.heads, nseg), dim3(512),
                     LDS_TOTAL, (hipStream_t)stream, a, SplitArgs{});
  SA_LAUNCH_CHECK();
  return SA_OK;
}

template <bool O8>
static int fwd_split_launch(const FwdArgsOf<O8>& a, int nseg, int max_q_len, int split_tiles, void* work,
                            int64_t work_bytes, void* stream) {
  const int nqb = (max_q_len + QBW - 1) / QBW;
  const int64_t ntiles = (int64_t)nseg * a.heads * nqb;
  if (!work || split_tiles <= 0 || split_tiles > ntiles || ntiles + split_tiles > 0x7fffffff) return SA_ERR_ARG;
  if ((((uintptr_t)work) & 15) || work_bytes < (int64_t)split_tiles * 2 * WBLK * 4) return SA_ERR_ARG;
  static const bool attr = [] {
    (void)hipFuncSetAttribute((const void*)attn_fwd_mx_kernel<true, O8>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              LDS_TOTAL);
    return true;
  }();
  (void)attr;
  SplitArgs sp{nqb, (int)(ntiles - split_tiles), (float*)work};
  hipLaunchKernelGGL((attn_fwd_mx_kernel<true, O8>), dim3((unsigned)(ntiles + split_tiles)), dim3(512), LDS_TOTAL,
                     (hipStream_t)stream, a, sp);
  SA_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_mx_split_merge_kernel<O8>, dim3(split_tiles), dim3(256), 0, (hipStream_t)stream, a, sp);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

extern "C" int sa_attn_fwd_mxfp8(const void* q, const void* q_scales, const void* k, const void* k_scales,
                                 const void* vt, const void* vt_scales, int64_t Rv, void* o, int64_t o_stride,
                                 const int32_t* segs, const int32_t* vcol0, int nseg, int max_q_len, int heads,
                                 int head_dim, const int32_t* o_rows, void* stream) {
  if (!fwd_operands_ok(q, q_scales, k, k_scales, vt, vt_scales, Rv, segs, vcol0, nseg, max_q_len, heads, head_dim) ||
      !fwd_out_ok(o, o_stride, heads))
    return SA_ERR_ARG;
  FwdArgs a{(const uint8_t*)q, (const uint8_t*)q_scales, (const uint8_t*)k, (const uint8_t*)k_scales,
            (const uint8_t*)vt, (const uint8_t*)vt_scales, Rv, (bf16*)o, o_stride, segs, vcol0, o_rows, heads};
  return fwd_launch<false>(a, nseg, max_q_len, stream);
}

extern "C" int sa_attn_fwd_mxfp8_split(const void* q, const void* q_scales, const void* k, const void* k_scales,
                                       const void* vt, const void* vt_scales, int64_t Rv, void* o, int64_t o_stride,
                                       const int32_t* segs, const int32_t* vcol0, int nseg, int max_q_len, int heads,
                                       int head_dim, const int32_t* o_rows, int split_tiles, void* work,
                                       int64_t work_bytes, void* stream) {
  if (!fwd_operands_ok(q, q_scales, k, k_scales, vt, vt_scales, Rv, segs, vcol0, nseg, max_q_len, heads, head_dim) ||
      !fwd_out_ok(o, o_stride, heads))
    return SA_ERR_ARG;
  FwdArgs a{(const uint8_t*)q, (const uint8_t*)q_scales, (const uint8_t*)k, (const uint8_t*)k_scales,
            (const uint8_t*)vt, (const uint8_t*)vt_scales, Rv, (bf16*)o, o_stride, segs, vcol0, o_rows, heads};
  return fwd_split_launch<false>(a, nseg, max_q_len, split_tiles, work, work_bytes, stream);
}

extern "C" int sa_attn_fwd_mxfp8_o8(const void* q, const void* q_scales, const void* k, const void* k_scales,
                                    const void* vt, const void* vt_scales, int64_t Rv, void* o_q, int64_t ldo,
                                    void* o_scales, int64_t ldos, const int32_t* segs, const int32_t* vcol0, int nseg,
                                    int max_q_len, int heads, int head_dim, const int32_t* o_rows, void* stream) {
  if (!fwd_operands_ok(q, q_scales, k, k_scales, vt, vt_scales, Rv, segs, vcol0, nseg, max_q_len, heads, head_dim) ||
      !fwd_out8_ok(o_q, ldo, o_scales, ldos, heads))
    return SA_ERR_ARG;
  FwdArgs8 a{{(const uint8_t*)q, (const uint8_t*)q_scales, (const uint8_t*)k, (const uint8_t*)k_scales,
              (const uint8_t*)vt, (const uint8_t*)vt_scales, Rv, (bf16*)o_q, ldo, segs, vcol0, o_rows, heads},
             (uint8_t*)o_scales, ldos};
  return fwd_launch<true>(a, nseg, max_q_len, stream);
}

extern "C" int sa_attn_fwd_mxfp8_split_o8(const void* q, const void* q_scales, const void* k, const void* k_scales,
                                          const void* vt, const void* vt_scales, int64_t Rv, void* o_q, int64_t ldo,
                                          void* o_scales, int64_t ldos, const int32_t* segs, const int32_t* vcol0,
                                          int nseg, int max_q_len, int heads, int head_dim, const int32_t* o_rows,
                                          int split_tiles, void* work, int64_t work_bytes, void* stream) {
  if (!fwd_operands_ok(q, q_scales, k, k_scales, vt, vt_scales, Rv, segs, vcol0, nseg, max_q_len, heads, head_dim) ||
      !fwd_out8_ok(o_q, ldo, o_scales, ldos, heads))
    return SA_ERR_ARG;
  FwdArgs8 a{{(const uint8_t*)q, (const uint8_t*)q_scales, (const uint8_t*)k, (const uint8_t*)k_scales,
              (const uint8_t*)vt, (const uint8_t*)vt_scales, Rv, (bf16*)o_q, ldo, segs, vcol0, o_rows, heads},
             (uint8_t*)o_scales, ldos};
  return fwd_split_launch<true>(a, nseg, max_q_len, split_tiles, work, work_bytes, stream);
}
