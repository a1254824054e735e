// MXFP8 "NT" GEMM for the DiT's FFN Linears (opt-in fp8 FFN mode) and its self-attention q/k/v Linears (opt-in fp8
// q/k/v mode); the default path stays on gemm.hip:
//   C[M,N] = epi(deq(A)[M,K] · deq(W)[N,K]^T + bias)
// A and W are e4m3fn bytes, K-contiguous, with one E8M0 scale byte per 32 consecutive K elements
// (stableavatar_amd/mxfp8.py is the definition); accumulation is fp32 on
// v_mfma_scale_f32_16x16x128_f8f6f4.  Replaces, when the mode is on, the aten::addmm of the FFN
// (wan_fantasy_transformer3d_1B.py:644-646 through :687-691), which has no fp8 counterpart in the reference.
//
// Three kernels share one tile, one K step, one staging path and one row epilogue, each written once below:
//   tile      4 waves, one per SIMD, over 256x256 (2 x 2 waves of 128 x 128, the 256 accumulators in AGPRs, as
//             gemm.hip's persistent kernel), raster xcd_remap / tile_coords
//   staging   mx_place / mx_dma / mx_dma_scale / mx_issue: K-tiles of 128 bytes by global_load ... lds into the bf16
//             kernels' XOR-swizzled LDS image (a 128-element fp8 K-tile is the same 128 bytes per row as their 64
//             bf16), two 64-KB stages (+ 2 KB of scale bytes each), rows past the operand clamped to its last row
//   K step    mx_frag / mx_step: 34 LDS reads, then 8 x 8 scaled MFMAs with A row m + 1 read under row m's
//   epilogue  mx_epilogue<EPI> (bias, GELU, bf16 / fp32 / gated residual / MXFP8 rows), mx_epilogue_vt (V^T)
// Lane map of the scaled MFMA (established with the exact-integer test): lane l = (row r = l % 16, group g = l / 16)
// supplies K bytes 16 g .. 16 g + 15 in its first four operand VGPRs and 64 + 16 g .. 64 + 16 g + 15 in the last
// four (the 16-byte chunks g and 4 + g of the row -- the bf16 kernels' fragment addresses), and byte 0 of its scale
// operand is the E8M0 scale of K block g (bytes 32 g .. 32 g + 31) of row r.  Operands are swapped (C^T = W·A^T) so
// each lane holds 4 consecutive output columns of one row.
// Each accumulator adds K-tiles 0 .. nk - 1 in order, one MFMA each, under every schedule, so the three kernels
// write the same bytes.  What each adds to the shared pieces:
// gemm_mx_kernel: one tile per workgroup, one barrier per K step: K-tile t + 1 is issued in one burst behind the
// barrier and lands while K-tile t multiplies.  With EPI_VT it is sa_gemm_mxfp8_vt's kernel (below).
// gemm_mxp_kernel (sa_gemm_mxfp8_ex, kernel 2): that step, one workgroup walking several tiles and loading its next
// tile's first K-tile under the current tile's epilogue (its header, below).
// gemm_mxk_kernel (sa_gemm_mxfp8_ks, kstep 2): one tile per workgroup on a K step that issues K-tile t + 2's DMA
// pieces between the MFMAs of step t into the regions of the stage step t has read (four barriers per step) and ends
// on a counted vmcnt (its header, below).  Auto picks it from 64 K-tiles on (the DiT's FFN-down).
//
// sa_gemm_mxfp8_vt (the V projection of the fp8 q/k/v mode, feeding sa_attn_fwd_mxfp8): the same K loop with the
// operands NOT swapped (C = A·W^T; the product of two operand rows does not depend on which side they sit, so the
// accumulators hold the same fp32 values as sa_gemm_mxfp8's), which leaves lane l = (column c = l % 16, group
// g = l / 16) of tile (m, n) holding acc[m][n][e] = token row 16 m + 4 g + e of the wave's 128-row half, output column
// 16 n + c.  The half is one 128-key block of one segment (the M axis is tiled per segment), m = 4 hi + t, and
// mxfp8_attn.KEY_OF_POS puts key 16 (4 hi + t) + 4 g + e at position 64 hi + 16 g + 4 t + e of the block: for each hi
// the lane's 16 values (t, e) are the 16 consecutive positions 64 hi + 16 g .. + 15 of V^T row (column) 16 n + c --
// one 16-byte store -- and the 32-position quantisation block 2 hi + g / 2 is this lane's 16 values and those of the
// lane 16 further (g ^ 1): one shfl_xor for its amax.
// Also here: sa_mxfp8_quant, the bf16 -> MXFP8 quantiser (weights at pack time; the definition's GPU twin).
#include <stdlib.h>

#include <utility>

#include "mxfp8.h"

namespace {

enum { EPI_BF16 = 0, EPI_GELU_BF16 = 1, EPI_F32 = 2, EPI_RES_F32 = 3, EPI_GELU_MXFP8 = 8 };
constexpr int EPI_VT = 100;  // sa_gemm_mxfp8_vt's kernel (not an epilogue code of the ABI)

typedef int __attribute__((ext_vector_type(8))) i32x8;

struct MxArgs {
  const uint8_t* A; long lda; const uint8_t* SA; long ldsa;
  const uint8_t* W; long ldw; const uint8_t* SW; long ldsw;
  const float* bias;
  void* C; long ldc; uint8_t* SC; long ldsc;  // SC: the output's scale bytes (EPI_GELU_MXFP8)
  const float* R; long ldr;                   // residual (EPI_RES_F32); may alias C
  const float* gate; long gate_bstride;       // gate[(m / rows_per_batch) * gate_bstride + n]
  int rows_per_batch;
  int M, N, K;
  int group_m;
  int rows_per_seg, seg_mt;  // EPI_VT: rows of a segment, 256-row tiles per segment (C = V^T bytes, ldc = Rv)
};

constexpr int BM = 256, BN = 256, BKB = 128;  // BKB: K-tile bytes = fp8 elements
constexpr int HALF_BYTES = 128 * BKB;         // 16 KB: 128 rows
constexpr int STAGE_BYTES = 4 * HALF_BYTES;   // 64 KB: A0 A1 W0 W1
constexpr int LDS_BYTES = 2 * STAGE_BYTES;    // 128 KB
constexpr int SCALE_STAGE = 2 * 256 * 4;      // 2 KB: a K-tile's scale dwords, A rows then W rows
constexpr int LDS_TOTAL = LDS_BYTES + 2 * SCALE_STAGE;

// gemm.hip's tile raster: runs of gm tile rows, column-major inside a run
__device__ __forceinline__ void tile_coords(int wg, int nm, int nn, int gm, int& mt, int& nt) {
  const int per = gm * nn;
  const int first = (wg / per) * gm;
  const int gsz = min(nm - first, gm);
  const int r = wg % per;
  mt = first + r % gsz;
  nt = r / gsz;
}

// compile-time loop: f(std::integral_constant<int, 0>) ... f(<N - 1>)
template <class F, int... I>
__device__ __forceinline__ void unroll_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void unroll(F&& f) { unroll_impl(f, std::make_integer_sequence<int, N>{}); }

// LDS reads and MFMAs as inline asm, as gemm.hip's persistent kernel (cdna_hip_programming.md 5.7): hipcc keeps them
// in program order, the accumulators stay in AGPRs ("+a") and the fragment waits are explicit
template <int OFF>
__device__ __forceinline__ void mx_ds(u32x4& d, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
template <int OFF>
__device__ __forceinline__ void mx_ds32(uint32_t& d, uint32_t addr) {
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF));
}
__device__ __forceinline__ i32x8 mx_join(const u32x4& lo, const u32x4& hi) {
  return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
// c += w (rows of W, scale byte sw) x x (rows of A, scale byte sa): e4m3 operands, scale byte 0 of each VGPR
__device__ __forceinline__ void mx_mma(f32x4& c, const i32x8& w, const i32x8& x, int sw, int sa) {
  asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
               : "+a"(c)
               : "v"(w), "v"(x), "v"(sw), "v"(sa));
}

__device__ __forceinline__ void mx_zero(f32x4 (&acc)[8][8]) {
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// Staging.  Half-tile h (0, 1 = A rows 0-127 / 128-255, 2, 3 = W) is 16 pieces of 1 KB (8 rows), four per wave (piece
// i of a wave is piece 4 i + wave of the half); lane l of a piece writes LDS bytes 16 l.. and so reads row l / 8, chunk
// (l % 8) ^ swizzle (gemm.hip's swz128).  The K-tile's scale bytes ride along: one dword (the tile's four K blocks)
// per row, thread i fetching row i of the A and of the W tile into [256] dwords each behind the ring.
// MxOff: a thread's byte offsets of K-tile 0 of one tile, 16 operand pieces and 2 scale rows.
struct MxOff {
  int g[4][4], sa, sw;
};

// the offsets of the tile at (m0, n0).  Rows past m_last / N - 1 are clamped to that row (read again, never stored),
// so every load stays inside the operand; m_last is M - 1, or the last row of the tile's segment under EPI_VT
__device__ __forceinline__ void mx_place(const MxArgs& g, int m0, int n0, int m_last, int wave, int tid, MxOff& o) {
  const int lane = tid & 63;
#pragma unroll
  for (int h = 0; h < 4; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (i * 4 + wave) * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ ((row >> 1) & 7);
      if (h < 2)
        o.g[h][i] = min(m0 + h * 128 + row, m_last) * (int)g.lda + chunk * 16;
      else
        o.g[h][i] = min(n0 + (h - 2) * 128 + row, g.N - 1) * (int)g.ldw + chunk * 16;
    }
  o.sa = min(m0 + tid, m_last) * (int)g.ldsa;
  o.sw = min(n0 + tid, g.N - 1) * (int)g.ldsw;
}

// piece I of half-tile H of K-tile kt into ring stage st
template <int H, int I>
__device__ __forceinline__ void mx_dma(const MxArgs& g, char* smem, const MxOff& o, int wave, int kt, int st) {
  __builtin_amdgcn_global_load_lds((const void*)((H < 2 ? g.A : g.W) + o.g[H][I] + (long)kt * BKB),
                                   LDS_PTR(smem + st * STAGE_BYTES + H * HALF_BYTES + (I * 4 + wave) * 1024), 16, 0, 0);
}
// K-tile kt's scale dword of the thread's A (SIDE 0) or W (SIDE 1) row into ring stage st
template <int SIDE>
__device__ __forceinline__ void mx_dma_scale(const MxArgs& g, char* smem, const MxOff& o, int wave, int kt, int st) {
  __builtin_amdgcn_global_load_lds((const void*)((SIDE ? g.SW + o.sw : g.SA + o.sa) + kt * 4),
                                   LDS_PTR(smem + LDS_BYTES + st * SCALE_STAGE + SIDE * 1024 + wave * 256), 4, 0, 0);
}
// the 18-piece burst: the operand pieces h-major, then the A and the W scales
__device__ __forceinline__ void mx_issue(const MxArgs& g, char* smem, const MxOff& o, int wave, int kt, int st) {
  unroll<16>([&](auto p) { mx_dma<p.value / 4, p.value % 4>(g, smem, o, wave, kt, st); });
  mx_dma_scale<0>(g, smem, o, wave, kt, st);
  mx_dma_scale<1>(g, smem, o, wave, kt, st);
}

// per-lane fragment read bases: row m * 16 + fr of a half-tile, chunks fc and 4 + fc (swz128: the XOR term
// depends on fr only, so m is an immediate offset); the row's scale dword, byte fc of it shifted down to byte 0
struct MxFrag {
  uint32_t a_lo, a_hi, w_lo, w_hi, sa_rd, sw_rd;
  int sh;
};
__device__ __forceinline__ MxFrag mx_frag(const char* smem, int wm, int wn, int fr, int fc) {
  const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
  const uint32_t swz = (fr >> 1) & 7;
  MxFrag f;
  f.a_lo = lds0 + wm * HALF_BYTES + fr * 128 + ((fc ^ swz) << 4);
  f.a_hi = lds0 + wm * HALF_BYTES + fr * 128 + (((4 + fc) ^ swz) << 4);
  f.w_lo = f.a_lo + (2 + wn - wm) * HALF_BYTES;
  f.w_hi = f.a_hi + (2 + wn - wm) * HALF_BYTES;
  f.sa_rd = lds0 + LDS_BYTES + (wm * 128 + fr) * 4;
  f.sw_rd = lds0 + LDS_BYTES + 1024 + (wn * 128 + fr) * 4;
  f.sh = 8 * fc;
  return f;
}

// One K step out of ring stage `stage`: the W fragments, every scale and A row 0 first; then row m's 8 MFMAs run
// while row m + 1 is read.  VT: the operands not swapped (the file header).  The schedules hang their own work on
// three callables: top() after the fragment wait, row(integral_constant m) after row m + 1's reads are issued,
// slot(integral_constant 8 m + n) after each MFMA; empty lambdas leave the plain step.
// The reads are asm the compiler does not count, so each wait "writes" every register the reads before it fill:
// nothing that uses them moves above it.
// The step is one body under one loop in every kernel: peeling a step out of the loop duplicated the body, and the
// compiler moved accumulators between the two copies' register assignments right behind inline-asm MFMAs whose
// latency it cannot see (wrong results, no fault).
template <bool VT, class Top, class Row, class Slot>
__device__ __forceinline__ void mx_step(f32x4 (&acc)[8][8], const MxFrag& f, int stage, Top&& top, Row&& row,
                                        Slot&& slot) {
  const uint32_t so = stage * STAGE_BYTES, ss = stage * SCALE_STAGE;
  u32x4 bl[8], bh[8], al[2], ah[2];
  uint32_t sar[8], swr[8];
  unroll<8>([&](auto n) {
    mx_ds<n.value * 2048>(bl[n.value], f.w_lo + so);
    mx_ds<n.value * 2048>(bh[n.value], f.w_hi + so);
    mx_ds32<n.value * 64>(swr[n.value], f.sw_rd + ss);
    mx_ds32<n.value * 64>(sar[n.value], f.sa_rd + ss);
  });
  mx_ds<0>(al[0], f.a_lo + so);
  mx_ds<0>(ah[0], f.a_hi + so);
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(bl[0]), "+v"(bl[1]), "+v"(bl[2]), "+v"(bl[3]), "+v"(bl[4]), "+v"(bl[5]), "+v"(bl[6]), "+v"(bl[7]),
                 "+v"(bh[0]), "+v"(bh[1]), "+v"(bh[2]), "+v"(bh[3]), "+v"(bh[4]), "+v"(bh[5]), "+v"(bh[6]), "+v"(bh[7]),
                 "+v"(al[0]), "+v"(ah[0])::"memory");
  asm volatile("" : "+v"(sar[0]), "+v"(sar[1]), "+v"(sar[2]), "+v"(sar[3]), "+v"(sar[4]), "+v"(sar[5]), "+v"(sar[6]),
                    "+v"(sar[7]), "+v"(swr[0]), "+v"(swr[1]), "+v"(swr[2]), "+v"(swr[3]), "+v"(swr[4]), "+v"(swr[5]),
                    "+v"(swr[6]), "+v"(swr[7]));
  top();
  i32x8 b[8];
  int sa[8], sw[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    b[n] = mx_join(bl[n], bh[n]);
    sa[n] = (int)(sar[n] >> f.sh);
    sw[n] = (int)(swr[n] >> f.sh);
  }
  unroll<8>([&](auto mc) {
    constexpr int m = mc.value;
    if constexpr (m > 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(al[m & 1]), "+v"(ah[m & 1])::"memory");
    if constexpr (m < 7) {
      mx_ds<(m + 1) * 2048>(al[(m + 1) & 1], f.a_lo + so);
      mx_ds<(m + 1) * 2048>(ah[(m + 1) & 1], f.a_hi + so);
    }
    row(mc);
    const i32x8 a = mx_join(al[m & 1], ah[m & 1]);
    unroll<8>([&](auto nc) {
      constexpr int n = nc.value;
      mx_mma(acc[m][n], VT ? a : b[n], VT ? b[n] : a, VT ? sa[m] : sw[n], VT ? sw[n] : sa[m]);
      slot(std::integral_constant<int, 8 * m + n>{});
    });
  });
}

// the MFMAs are opaque to the compiler's hazard handling: let the last ones retire before their results are read
__device__ __forceinline__ void mx_drain() { asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); }

// Row epilogue of the tile at (m0, n0), straight from the accumulators: acc[m][n] of lane (fr, fc) = row
// m0 + wm*128 + m*16 + fr, columns n0 + wn*128 + n*16 + 4 fc + 0..3.  Walked in column pairs (n = 2p, 2p + 1): the 32
// columns of pair p in one row are one MXFP8 block, held by the four lanes fr, fr + 16, fr + 32, fr + 48.
template <int EPI>
__device__ __forceinline__ void mx_epilogue(const MxArgs& g, f32x4 (&acc)[8][8], int m0, int n0, int wm, int wn,
                                            int fr, int fc) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    // pair p's accumulators leave the AGPRs here, after pair p - 1's stores: read all at once (the compiler's choice
    // when left free) the 256 of them fill the VGPR file and the gated-residual and MXFP8 epilogues spill
#pragma unroll
    for (int m = 0; m < 8; ++m) asm volatile("" : "+a"(acc[m][2 * p]), "+a"(acc[m][2 * p + 1])::"memory");
    const int cb = n0 + wn * 128 + p * 32;  // the block's first column (wave-uniform)
    if (cb >= g.N) continue;
    const int c[2] = {cb + 4 * fc, cb + 16 + 4 * fc};
    float bv[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[h][e] = (g.bias && c[h] + e < g.N) ? g.bias[c[h] + e] : 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int row = m0 + wm * 128 + m * 16 + fr;
      const bool live = row < g.M;
      float v[8];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * h + e] = acc[m][2 * p + h][e] + bv[h][e];
      if constexpr (EPI == EPI_GELU_BF16 || EPI == EPI_GELU_MXFP8) {
        // as gemm.hip's epi_row: the bf16 rounding of the Linear output, then the packed GELU
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const bf16x2 hb = __builtin_convertvector((f32x2){v[j], v[j + 1]}, bf16x2);
          const f32x2 y = gelu_tanh2(__builtin_convertvector(hb, f32x2));
          v[j] = y[0];
          v[j + 1] = y[1];
        }
      }
      if constexpr (EPI == EPI_GELU_MXFP8) {
        // the bf16-rounded GELU output quantised: SA_EPI_GELU_TANH_BF16 followed by sa_mxfp8_quant, N % 32 == 0
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = bf2f(f2bf(v[j]));
        float amax = mx_amax8(v);
        amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
        uint32_t s;
        const u32x2 q = mx_quant8(v, amax, &s);
        if (live) {
          uint8_t* C = (uint8_t*)g.C + (long)row * g.ldc;
          *(uint32_t*)(C + c[0]) = q[0];
          *(uint32_t*)(C + c[1]) = q[1];
          if (fc == 0) g.SC[(long)row * g.ldsc + cb / 32] = (uint8_t)s;
        }
      } else if constexpr (EPI == EPI_BF16 || EPI == EPI_GELU_BF16) {
        if (live) {
          bf16* C = (bf16*)g.C + (long)row * g.ldc;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (c[h] + 4 <= g.N) {
              *(bf16x4*)(C + c[h]) = (bf16x4){f2bf(v[4 * h]), f2bf(v[4 * h + 1]), f2bf(v[4 * h + 2]), f2bf(v[4 * h + 3])};
            } else {
              for (int e = 0; e < 4; ++e)
                if (c[h] + e < g.N) C[c[h] + e] = f2bf(v[4 * h + e]);
            }
          }
        }
      } else {
        if (live) {
          float* C = (float*)g.C + (long)row * g.ldc;
          const float* R = EPI == EPI_RES_F32 ? g.R + (long)row * g.ldr : nullptr;
          const float* gt =
              (EPI == EPI_RES_F32 && g.gate) ? g.gate + (long)(row / g.rows_per_batch) * g.gate_bstride : nullptr;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (c[h] + 4 <= g.N) {
              f32x4 o = {v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
              if constexpr (EPI == EPI_RES_F32) {
                // the reference's nn.Linear returns bf16 under autocast; the gated residual consumes that value
                const f32x4 r = *(const f32x4*)(R + c[h]);
                const f32x4 gg = gt ? *(const f32x4*)(gt + c[h]) : (f32x4){1.f, 1.f, 1.f, 1.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = r[e] + bf2f(f2bf(o[e])) * gg[e];
              }
              *(f32x4*)(C + c[h]) = o;
            } else {
              for (int e = 0; e < 4; ++e)
                if (c[h] + e < g.N) {
                  float o = v[4 * h + e];
                  if constexpr (EPI == EPI_RES_F32) o = R[c[h] + e] + bf2f(f2bf(o)) * (gt ? gt[c[h] + e] : 1.0f);
                  C[c[h] + e] = o;
                }
            }
          }
        }
      }
    }
  }
}

// V^T epilogue (lane map: the file header) of the tile at rows t0 .. t0 + 255 of segment sg, columns n0 ..: this wave's
// half is keys k0 .. k0 + 127 of the segment, V^T columns vc .. vc + 127; a half that starts at or past the segment's
// end owns no columns and writes nothing
__device__ __forceinline__ void mx_epilogue_vt(const MxArgs& g, f32x4 (&acc)[8][8], int sg, int t0, int n0, int wm,
                                               int wn, int fr, int fc) {
  const int k0 = t0 + wm * 128, cw = n0 + wn * 128;
  if (k0 >= g.rows_per_seg || cw >= g.N) return;
  const long vc = (long)sg * ((g.rows_per_seg + 127) / 128 * 128) + k0;
  uint8_t* Vq = (uint8_t*)g.C;
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int col = cw + n * 16 + fr;
    const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
    for (int hi = 0; hi < 2; ++hi) {
      float v[16];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // the bf16 rounding of the Linear output (SA_EPI_BF16), keys past the segment as zeros
          const bool live = k0 + 16 * (4 * hi + t) + 4 * fc + e < g.rows_per_seg;
          v[4 * t + e] = live ? bf2f(f2bf(acc[4 * hi + t][n][e] + bv)) : 0.f;
        }
      float amax = fmaxf(mx_amax8(v), mx_amax8(v + 8));
      amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
      uint32_t s;
      const u32x2 lo = mx_quant8(v, amax, &s), hi2 = mx_quant8(v + 8, amax, &s);
      *(u32x4*)(Vq + (long)col * g.ldc + vc + 64 * hi + 16 * fc) = (u32x4){lo[0], lo[1], hi2[0], hi2[1]};
      if ((fc & 1) == 0) g.SC[(long)col * g.ldsc + vc / 32 + 2 * hi + (fc >> 1)] = (uint8_t)s;
    }
  }
}

// tiles of the M axis: per segment under EPI_VT (a segment's last tile may be partly live)
__host__ __device__ __forceinline__ int mx_tiles_m(const MxArgs& g, bool vt) {
  return vt ? (g.M / g.rows_per_seg) * g.seg_mt : (g.M + BM - 1) / BM;
}
__host__ __device__ __forceinline__ int mx_tiles(const MxArgs& g, bool vt = false) {
  return mx_tiles_m(g, vt) * ((g.N + BN - 1) / BN);
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_mx_kernel(MxArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fc = lane >> 4;
  constexpr bool VT = EPI == EPI_VT;
  const int nm = mx_tiles_m(g, VT), nn = (g.N + BN - 1) / BN;
  int mt, nt;
  tile_coords(xcd_remap(blockIdx.x, nm * nn), nm, nn, g.group_m, mt, nt);
  // EPI_VT tiles the M axis per segment: tile mt is rows t0 .. t0 + 255 of segment sg (rows at or past rows_per_seg
  // are clamped to the segment's last row on load and written as zeros)
  const int sg = VT ? mt / g.seg_mt : 0, t0 = VT ? (mt % g.seg_mt) * BM : 0;
  const int m0 = VT ? sg * g.rows_per_seg + t0 : mt * BM, n0 = nt * BN;
  const int nk = g.K / BKB;
  MxOff off;
  mx_place(g, m0, n0, VT ? (sg + 1) * g.rows_per_seg - 1 : g.M - 1, wave, tid, off);
  const MxFrag frag = mx_frag(smem, wm, wn, fr, fc);
  f32x4 acc[8][8];
  mx_zero(acc);

  mx_issue(g, smem, off, wave, 0, 0);
  for (int t = 0; t < nk; ++t) {
    // tile t has landed (every wave waits for its own pieces, then the barrier), and every wave is done reading
    // the other stage (tile t - 1), which tile t + 1 now overwrites
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (t + 1 < nk) mx_issue(g, smem, off, wave, t + 1, (t + 1) & 1);
    mx_step<VT>(acc, frag, t & 1, [] {}, [](auto) {}, [](auto) {});
  }
  mx_drain();
  if constexpr (VT)
    mx_epilogue_vt(g, acc, sg, t0, n0, wm, wn, fr, fc);
  else
    mx_epilogue<EPI>(g, acc, m0, n0, wm, wn, fr, fc);
}

// gemm_mxp_kernel: gemm_mx_kernel's step, persistent over tiles.  Workgroup w of a grid of G = min(tiles, workgroups)
// walks tiles w, w + G, ... of the xcd_remap / tile_coords order.  One running K-step counter s gives the ring stage
// (s & 1), so a tile with an odd K-tile count hands the next tile the other stage.  During a tile's last K step the
// free stage receives K-tile 0 (and its scales) of the workgroup's next tile, from load offsets worked out in that
// step; those loads fly under the epilogue and the next tile's first step waits for them as any step waits for its
// tile.
// Barriers: one per K step, under tile- and step-loop bounds that depend on blockIdx.x, gridDim.x and the tile count
// only; a workgroup without a tile returns before the first.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_mxp_kernel(MxArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nm = mx_tiles_m(g, false), nn = (g.N + BN - 1) / BN, total = nm * nn;
  const int nk = g.K / BKB;
  const int G = gridDim.x;
  if ((int)blockIdx.x >= total) return;

  // the load offsets of tile u
  auto place = [&](int u, int tid, MxOff& o, int& m0, int& n0) {
    int mt, nt;
    tile_coords(xcd_remap(u, total), nm, nn, g.group_m, mt, nt);
    m0 = mt * BM;
    n0 = nt * BN;
    mx_place(g, m0, n0, g.M - 1, wave, tid, o);
  };

  f32x4 acc[8][8];
  mx_zero(acc);
  {
    MxOff first;
    int m0, n0;
    place(blockIdx.x, threadIdx.x, first, m0, n0);
    mx_issue(g, smem, first, wave, 0, 0);
  }
  int s = 0;  // K steps this workgroup has run, over all its tiles
  for (int u = blockIdx.x; u < total; u += G) {
    // Everything per lane is derived again, tile by tile, from a thread id the compiler cannot see through: nothing
    // but the accumulators is then live across the epilogue, which needs most of the VGPR file (kept live across it,
    // the fragment addresses and load offsets spilled)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, fr = lane & 15, fc = lane >> 4;
    const MxFrag frag = mx_frag(smem, wm, wn, fr, fc);
    MxOff cur;
    int m0, n0;
    place(u, tid, cur, m0, n0);
    for (int t = 0; t < nk; ++t, ++s) {
      // step s's tile has landed, and every wave is done reading the other stage (step s - 1, of this tile or of the
      // workgroup's previous one), which the loads below overwrite
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < nk) {
        mx_issue(g, smem, cur, wave, t + 1, (s + 1) & 1);
      } else if (u + G < total) {
        // the next tile's offsets live in this branch only: replacing `cur` here makes every step of the loop copy
        // and sign-extend all 18 of them (measured: 4 % on a 70-step tile); the next tile derives them again
        MxOff nxt;
        int nm0, nn0;
        place(u + G, tid, nxt, nm0, nn0);
        mx_issue(g, smem, nxt, wave, 0, (s + 1) & 1);
      }
      mx_step<false>(acc, frag, s & 1, [] {}, [](auto) {}, [](auto) {});
    }
    mx_drain();
    mx_epilogue<EPI>(g, acc, m0, n0, wm, wn, fr, fc);
    mx_zero(acc);
  }
}

// gemm_mxk_kernel (sa_gemm_mxfp8_ks, kstep 2): one tile per workgroup, with a K step that issues no DMA burst and ends
// on a counted vmcnt.  A wave's 18 DMA pieces of a K-tile are numbered 0-7 = its W pieces (half 2 + p / 4, piece
// p % 4), 8, 9 = the A and W scale dwords, 10-13 = A rows 0-63 of both halves, 14-17 = A rows 64-127 of both halves.
// Step t multiplies K-tile t out of stage S = t & 1 while K-tile t + 1 lands in stage S ^ 1 and K-tile t + 2 is issued
// into stage S, region by region as the step's reads free it (MFMA slot s = 8 m + n, row-major over the wave's 8 x 8
// fragment tiles), through mx_step's three callables:
//   top         34 LDS reads (8 W fragments, 16 scale dwords, A row 0)  -> lgkmcnt(0), barrier #1: W and scales free
//   slots 0-19  pieces 0-9 (W, scales) of K-tile t + 2, one after every second MFMA from slot 1
//   slot 24     A row 3 has been read (row m + 1 is read under row m's MFMAs) -> barrier #2: A rows 0-63 free
//   slots 26-38 pieces 10-13, one after every fourth MFMA
//   slot 56     A row 7 has been read                                         -> barrier #3: A rows 64-127 free
//   slots 56-62 pieces 14-17, one after every second MFMA
//   end         vmcnt(18): K-tile t + 1 has landed, K-tile t + 2's 18 pieces stay in flight -> barrier #4
// With no K-tile t + 2 (the last two steps; every step of nk = 1, 2) nothing is issued and the step ends on vmcnt(0).
// The prologue issues K-tiles 0 and 1 (K-tile 0 alone when nk = 1) and waits as a step's end does.  STAGE = 1 is the
// first stage of that schedule, kept for measurement (SA_MXGEMM_KSTEP_STAGE): one barrier per step as gemm_mx_kernel,
// K-tile t + 1's pieces issued one after every third MFMA from slot 2, vmcnt(0) at the end.
// The branch around a piece tests a condition the compiler cannot relate to the next piece's, so it has no reason to
// duplicate the MFMAs between them (mx_step: one body under one loop).
// Barriers: one before the loop and four (STAGE 1: one) per K step, all under the bound t < nk alone.
template <int STAGE>
constexpr int mxk_piece_after(int s) {
  if (STAGE == 1) return (s >= 2 && (s - 2) % 3 == 0 && s < 56) ? (s - 2) / 3 : -1;
  if (s < 20) return (s & 1) ? s / 2 : -1;
  if (s >= 26 && s <= 38) return (s - 26) % 4 == 0 ? 10 + (s - 26) / 4 : -1;
  if (s >= 56) return (s & 1) ? -1 : 14 + (s - 56) / 2;
  return -1;
}

template <int EPI, int STAGE>
__global__ __launch_bounds__(256) void gemm_mxk_kernel(MxArgs g) {
  static_assert(STAGE == 1 || STAGE == 2, "K-step stage: 1 = interleaved issue, 2 = two tiles in flight");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fc = lane >> 4;
  const int nm = mx_tiles_m(g, false), nn = (g.N + BN - 1) / BN;
  int mt, nt;
  tile_coords(xcd_remap(blockIdx.x, nm * nn), nm, nn, g.group_m, mt, nt);
  const int m0 = mt * BM, n0 = nt * BN;
  const int nk = g.K / BKB;
  // mx_place's statements, kept inline in this kernel alone: behind the call the compiler forms each piece's address
  // after the M0 write, right in front of the load, at all 16 operand sites between the MFMAs, and the step measured
  // 0.6 - 0.7 % slower on the FFN shapes (DESIGN.md "MXFP8 GEMM K step", the fold)
  MxOff off;
#pragma unroll
  for (int h = 0; h < 4; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (i * 4 + wave) * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ ((row >> 1) & 7);
      if (h < 2)
        off.g[h][i] = min(m0 + h * 128 + row, g.M - 1) * (int)g.lda + chunk * 16;
      else
        off.g[h][i] = min(n0 + (h - 2) * 128 + row, g.N - 1) * (int)g.ldw + chunk * 16;
    }
  off.sa = min(m0 + tid, g.M - 1) * (int)g.ldsa;
  off.sw = min(n0 + tid, g.N - 1) * (int)g.ldsw;
  // piece P (the header's numbering) of K-tile kt < nk into ring stage kt & 1
  auto dma = [&](auto pc, int kt) {
    constexpr int P = pc.value, q = P < 8 ? P : (P - 10) & 3;
    if constexpr (P == 8 || P == 9)
      mx_dma_scale<P - 8>(g, smem, off, wave, kt, kt & 1);
    else
      mx_dma<(P < 8 ? 2 + q / 4 : q >> 1), (P < 8 ? q % 4 : (P < 14 ? 0 : 2) + (q & 1))>(g, smem, off, wave, kt, kt & 1);
  };
  auto barrier = [] {
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  const MxFrag frag = mx_frag(smem, wm, wn, fr, fc);
  f32x4 acc[8][8];
  mx_zero(acc);

  unroll<18>([&](auto p) { dma(p, 0); });
  if (STAGE == 2 && nk > 1) {
    unroll<18>([&](auto p) { dma(p, 1); });
    asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  barrier();
  for (int t = 0; t < nk; ++t) {
    // K-tile t has landed in every wave's sight (the wait and barrier that ended step t - 1, or the prologue's)
    const int kt = t + STAGE;  // the K-tile this step fetches
    const bool more = kt < nk;
    mx_step<false>(
        acc, frag, t & 1,
        [&] {  // #1: every wave holds its W fragments and scales of stage t & 1
          if constexpr (STAGE == 2) barrier();
        },
        [&](auto mc) {  // #2, #3: every wave holds A rows 0-3 / 4-7 of its half (the read just issued at m = 3 is of row 4)
          if constexpr (STAGE == 2 && (mc.value == 3 || mc.value == 7)) barrier();
        },
        [&](auto sc) {
          constexpr int P = mxk_piece_after<STAGE>(sc.value);
          if constexpr (P >= 0) {
            int go = more;
            asm volatile("" : "+v"(go));
            if (__builtin_amdgcn_readfirstlane(go)) dma(std::integral_constant<int, P>{}, kt);
          }
        });
    if (STAGE == 2 && more)
      asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    barrier();
  }
  mx_drain();
  mx_epilogue<EPI>(g, acc, m0, n0, wm, wn, fr, fc);
}

// one launcher for the three kernels: the LDS attribute is set once per instantiation
template <auto KERNEL>
int mx_launch(const MxArgs& g, int grid, hipStream_t st) {
  static const bool attr = [] {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TOTAL);
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(256), LDS_TOTAL, st, g);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

enum { KERNEL_AUTO = 0, KERNEL_ONE_TILE = 1, KERNEL_PERSISTENT = 2 };
// what auto resolves to (DESIGN.md "Persistent MXFP8 GEMM", Decision); the two kernels are bit-identical
#ifndef SA_MXGEMM_KERNEL_DEFAULT
#define SA_MXGEMM_KERNEL_DEFAULT KERNEL_ONE_TILE
#endif

// the kernel auto picks (SA_MXGEMM_KERNEL=1|2 overrides, read once per process)
int env_kernel() {
  static const int k = [] {
    const char* e = getenv("SA_MXGEMM_KERNEL");
    const int v = e ? atoi(e) : 0;
    return (v == KERNEL_ONE_TILE || v == KERNEL_PERSISTENT) ? v : SA_MXGEMM_KERNEL_DEFAULT;
  }();
  return k;
}

int num_cus() {
  // per device: the persistent grid is one workgroup per CU
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

enum { KSTEP_AUTO = 0, KSTEP_ONE_BARRIER = 1, KSTEP_SPLIT = 2 };
// what auto resolves to for the one-tile kernels (DESIGN.md "MXFP8 GEMM K step", Decision; bit-identical either way):
// the default step, and the split step from SA_MXGEMM_KSTEP_SPLIT_MIN_NK K-tiles on -- the measured win is the 70-step
// FFN-down tile; the 12-step tiles tie or lose
#ifndef SA_MXGEMM_KSTEP_DEFAULT
#define SA_MXGEMM_KSTEP_DEFAULT KSTEP_ONE_BARRIER
#endif
#ifndef SA_MXGEMM_KSTEP_SPLIT_MIN_NK
#define SA_MXGEMM_KSTEP_SPLIT_MIN_NK 64
#endif
// which stage of the new step kstep 2 runs: 2 = the whole schedule, 1 = interleaved issue alone (measurement builds)
#ifndef SA_MXGEMM_KSTEP_STAGE
#define SA_MXGEMM_KSTEP_STAGE 2
#endif

// the K step auto picks for a launch of nk K-tiles (SA_MXGEMM_KSTEP=1|2 overrides, read once per process)
int auto_kstep(int nk) {
  static const int k = [] {
    const char* e = getenv("SA_MXGEMM_KSTEP");
    const int v = e ? atoi(e) : 0;
    return (v == KSTEP_ONE_BARRIER || v == KSTEP_SPLIT) ? v : KSTEP_AUTO;
  }();
  if (k != KSTEP_AUTO) return k;
  return nk >= SA_MXGEMM_KSTEP_SPLIT_MIN_NK ? KSTEP_SPLIT : SA_MXGEMM_KSTEP_DEFAULT;
}

// auto, per launch: a persistent selection (explicit, or auto under SA_MXGEMM_KERNEL=2) keeps the one-barrier step.
// workgroups: 0 = one per CU, > 0 = the cap on the persistent grid (tests and A/B)
template <int EPI>
int launch_sel(const MxArgs& g, int kernel, int workgroups, int kstep, hipStream_t st) {
  if (kernel == KERNEL_AUTO && kstep != KSTEP_SPLIT) kernel = env_kernel();
  if (kstep == KSTEP_AUTO) kstep = kernel == KERNEL_PERSISTENT ? KSTEP_ONE_BARRIER : auto_kstep(g.K / BKB);
  if (kstep == KSTEP_SPLIT) return mx_launch<gemm_mxk_kernel<EPI, SA_MXGEMM_KSTEP_STAGE>>(g, mx_tiles(g), st);
  if (kernel == KERNEL_PERSISTENT)
    return mx_launch<gemm_mxp_kernel<EPI>>(g, min(mx_tiles(g), workgroups > 0 ? workgroups : num_cus()), st);
  return mx_launch<gemm_mx_kernel<EPI>>(g, mx_tiles(g), st);
}

// what every GEMM entry point asks of its operands (out: C or vt_out)
int check_operands(const void* A, int64_t lda, const void* SA, int64_t ldsa, const void* W, int64_t ldw, const void* SW,
                   int64_t ldsw, const void* out, int M, int N, int K) {
  if (!A || !SA || !W || !SW || !out || M <= 0 || N <= 0 || K <= 0) return SA_ERR_ARG;
  if (K % BKB != 0 || lda % 16 != 0 || ldw % 16 != 0 || lda < K || ldw < K || ldsa < K / 32 || ldsw < K / 32)
    return SA_ERR_ARG;
  if ((((uintptr_t)A) & 15) || (((uintptr_t)W) & 15)) return SA_ERR_ARG;
  // a K-tile's four scale bytes of a row are fetched as one dword
  if (ldsa % 4 != 0 || ldsw % 4 != 0 || (((uintptr_t)SA) & 3) || (((uintptr_t)SW) & 3)) return SA_ERR_ARG;
  // 32-bit element / scale offsets inside the kernel
  if ((long)M * lda >= 0x7fffffffL || (long)N * ldw >= 0x7fffffffL || (long)M * ldsa >= 0x7fffffffL ||
      (long)N * ldsw >= 0x7fffffffL)
    return SA_ERR_ARG;
  return SA_OK;
}

struct QuantArgs {
  const bf16* x; long ldx;
  uint8_t* q; long ldq;
  uint8_t* s; long lds;
  int M, K;
};

// one wave per row, 8 elements per lane per 512-column chunk: a block is four adjacent lanes
__global__ __launch_bounds__(256) void mxfp8_quant_kernel(QuantArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.M) return;
  const bf16* x = a.x + (long)row * a.ldx;
  for (int c0 = lane * 8; c0 < a.K; c0 += 512) {  // K % 32 == 0: the four lanes of a block leave together
    const bf16x8 xv = *(const bf16x8*)(x + c0);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(xv[j]);
    float amax = mx_amax8(v);
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    uint32_t s;
    const u32x2 q = mx_quant8(v, amax, &s);
    *(u32x2*)(a.q + (long)row * a.ldq + c0) = q;
    if ((lane & 3) == 0) a.s[(long)row * a.lds + c0 / 32] = (uint8_t)s;
  }
}

}  // namespace

extern "C" int sa_mxfp8_quant(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t lds, int M, int K,
                              void* stream) {
  if (!x || !q || !scales || M <= 0 || K <= 0 || K % 32) return SA_ERR_ARG;
  if (ldx < K || ldx % 8 || ldq < K || ldq % 8 || lds < K / 32) return SA_ERR_ARG;
  if ((((uintptr_t)x) & 15) || (((uintptr_t)q) & 7)) return SA_ERR_ARG;
  QuantArgs a{(const bf16*)x, ldx, (uint8_t*)q, ldq, (uint8_t*)scales, lds, M, K};
  hipLaunchKernelGGL(mxfp8_quant_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  SA_LAUNCH_CHECK();
  return SA_OK;
}

extern "C" int sa_gemm_mxfp8_ks(const void* A, int64_t lda, const void* A_scales, int64_t ldas, const void* W,
                                int64_t ldw, const void* W_scales, int64_t ldws, const float* bias, void* C, int64_t ldc,
                                void* C_scales, int64_t ldcs, int M, int N, int K, int epilogue, const float* residual,
                                int64_t ldr, const float* gate, int64_t gate_bstride, int rows_per_batch, int kernel,
                                int workgroups, int kstep, void* stream) {
  if (kernel < KERNEL_AUTO || kernel > KERNEL_PERSISTENT || workgroups < 0) return SA_ERR_ARG;
  if (kstep < KSTEP_AUTO || kstep > KSTEP_SPLIT) return SA_ERR_ARG;
  // the new step is a one-tile kernel: no persistent form, no grid cap
  if (kstep == KSTEP_SPLIT && (kernel == KERNEL_PERSISTENT || workgroups != 0)) return SA_ERR_ARG;
  if (check_operands(A, lda, A_scales, ldas, W, ldw, W_scales, ldws, C, M, N, K) != SA_OK) return SA_ERR_ARG;
  if (ldc < N || ldc % 4 != 0 || (((uintptr_t)C) & 15)) return SA_ERR_ARG;  // 4-column vector stores
  if (epilogue == EPI_RES_F32 &&
      (!residual || ldr % 4 != 0 || (((uintptr_t)residual) & 15) || (gate && rows_per_batch <= 0))) return SA_ERR_ARG;
  if (epilogue == EPI_RES_F32 && gate && ((gate_bstride % 4 != 0) || (((uintptr_t)gate) & 15))) return SA_ERR_ARG;
  if (epilogue == EPI_GELU_MXFP8 && (N % 32 != 0 || !C_scales || ldcs < N / 32)) return SA_ERR_ARG;
  MxArgs g{(const uint8_t*)A, lda, (const uint8_t*)A_scales, ldas, (const uint8_t*)W, ldw, (const uint8_t*)W_scales, ldws,
           bias, C, ldc, (uint8_t*)C_scales, ldcs, residual, ldr, gate, gate_bstride,
           rows_per_batch > 0 ? rows_per_batch : 1, M, N, K, epilogue == EPI_RES_F32 ? 4 : 8, M, 0};
  hipStream_t st = (hipStream_t)stream;
  switch (epilogue) {
    case EPI_BF16: return launch_sel<EPI_BF16>(g, kernel, workgroups, kstep, st);
    case EPI_GELU_BF16: return launch_sel<EPI_GELU_BF16>(g, kernel, workgroups, kstep, st);
    case EPI_F32: return launch_sel<EPI_F32>(g, kernel, workgroups, kstep, st);
    case EPI_RES_F32: return launch_sel<EPI_RES_F32>(g, kernel, workgroups, kstep, st);
    case EPI_GELU_MXFP8: return launch_sel<EPI_GELU_MXFP8>(g, kernel, workgroups, kstep, st);
    default: return SA_ERR_ARG;
  }
}

extern "C" int sa_gemm_mxfp8(const void* A, int64_t lda, const void* A_scales, int64_t ldas, const void* W, int64_t ldw,
                             const void* W_scales, int64_t ldws, const float* bias, void* C, int64_t ldc,
                             void* C_scales, int64_t ldcs, int M, int N, int K, int epilogue, const float* residual,
                             int64_t ldr, const float* gate, int64_t gate_bstride, int rows_per_batch, void* stream) {
  return sa_gemm_mxfp8_ks(A, lda, A_scales, ldas, W, ldw, W_scales, ldws, bias, C, ldc, C_scales, ldcs, M, N, K, epilogue,
                          residual, ldr, gate, gate_bstride, rows_per_batch, KERNEL_AUTO, 0, KSTEP_AUTO, stream);
}

extern "C" int sa_gemm_mxfp8_ex(const void* A, int64_t lda, const void* A_scales, int64_t ldas, const void* W,
                                int64_t ldw, const void* W_scales, int64_t ldws, const float* bias, void* C, int64_t ldc,
                                void* C_scales, int64_t ldcs, int M, int N, int K, int epilogue, const float* residual,
                                int64_t ldr, const float* gate, int64_t gate_bstride, int rows_per_batch, int kernel,
                                int workgroups, void* stream) {
  // an explicit kernel keeps the one-barrier step (kernel 1 is the baseline arm of every A/B); auto forwards auto
  return sa_gemm_mxfp8_ks(A, lda, A_scales, ldas, W, ldw, W_scales, ldws, bias, C, ldc, C_scales, ldcs, M, N, K, epilogue,
                          residual, ldr, gate, gate_bstride, rows_per_batch, kernel, workgroups,
                          kernel == KERNEL_AUTO ? KSTEP_AUTO : KSTEP_ONE_BARRIER, stream);
}

extern "C" int sa_gemm_mxfp8_vt(const void* A, int64_t lda, const void* A_scales, int64_t ldas, const void* W,
                                int64_t ldw, const void* W_scales, int64_t ldws, const float* bias, void* vt_out,
                                void* vt_scales, int64_t Rv, int M, int N, int K, int rows_per_seg, int nseg,
                                void* stream) {
  if (check_operands(A, lda, A_scales, ldas, W, ldw, W_scales, ldws, vt_out, M, N, K) != SA_OK) return SA_ERR_ARG;
  if (!vt_scales || N % 128 != 0) return SA_ERR_ARG;
  if (rows_per_seg <= 0 || nseg <= 0 || (long)nseg * rows_per_seg != M) return SA_ERR_ARG;
  // every segment owns ceil128(rows_per_seg) columns of the Rv; 16-byte stores into vt_out
  const long seg_cols = ((long)rows_per_seg + 127) / 128 * 128;
  if (Rv <= 0 || Rv % 128 != 0 || Rv < nseg * seg_cols || (((uintptr_t)vt_out) & 15)) return SA_ERR_ARG;
  MxArgs g{(const uint8_t*)A, lda, (const uint8_t*)A_scales, ldas, (const uint8_t*)W, ldw, (const uint8_t*)W_scales, ldws,
           bias, vt_out, Rv, (uint8_t*)vt_scales, Rv / 32, nullptr, 0, nullptr, 0, 1, M, N, K, 8, rows_per_seg,
           (rows_per_seg + BM - 1) / BM};
  return mx_launch<gemm_mx_kernel<EPI_VT>>(g, mx_tiles(g, true), (hipStream_t)stream);
}
