// rade_corr2.h -- the two-stage pilot correlator on v_mfma_f32_16x16x32_f16, stated once for its three kernels: the unsynchronised search (rx2_detect_q,
// rade_rx_search.h), check_pilots' row refreshes (check2_rows_q, rade_rx_check.h) and whole-file acquisition (k_acq_detect, rade_acq.hip).  Each of them keeps only
// what is its own: where the table fragments and the sample planes come from, which timings a wavefront owns, and what it does with |Dt|.
// The moment form (the basis and its accuracy: rade_host.c, corr_basis).  Dt[t][f] = sum_m conj(rx[t + m]) p_w[m][f] over the 160 samples of the pilot symbol, for 40
// frequencies.  p_w[m][f] = sum_r alpha[r][f] s_r[m] over RD_NQ = 16 polynomial moments, so Dt[t][f] = sum_r alpha[r][f] Mom_r[t] with Mom_r[t] = sum_m conj(rx[t + m]) s_r[m]:
//   stage 1  rows (r, re | im) = RD_CORR_NRT = 2 tiles of 16, K = (m, re | im) = RD_CORR_NKS = 10 steps of 32, columns = 16 timings.  A operand: corrq16, the realified s_r
//            scaled by 2^12, [row tile][k-step][plane][lane][8].  B operand: the samples, (re, im) of one sample in one word per plane (rx2_split16), under the power of
//            two that puts the block's largest component into [2^7, 2^8) (operand_scale, rade_devutil.h); lane (i, g) holds samples t_i + 16 s + 4 g .. + 3 of k-step s.
//            Both operands are two binary16 planes (hi + lo, 22 bits) and the product is hi hi + hi lo + lo hi: 2 x 10 x 3 = 60 matrix instructions per timing tile
//            where the 80 rows (f, re | im) of p_w itself take 5 x 10 x 3 = 150 (tools/experiments/rx2_search_one_stage.inc).
//   stage 2  rows (f, re | im) = RD_CORR_NFT = 5 tiles of 16, ONE k-step: K = the 32 rows of stage 1.  A operand: corra16, {ar, -ai; ai, ar} of alpha scaled by 2^10,
//            [frequency tile][plane][lane][8].  B operand: stage 1's accumulators, without leaving the lane -- the C layout of two 16-row tiles gives lane group g rows
//            4 g .. 4 g + 3 of either tile, and the host orders corra16's K axis exactly so (k-slot (g, j): row 4 g + j of tile 0 for j < 4, of tile 1 behind it).  The
//            moments are scaled by 2^-7 (|moment| <= 2^8 sqrt(2) x the table row's L1 norm: 2^-7 of it is below 7100, far inside binary16) and split into three
//            planes (33 bits: stage 2 adds nothing to stage 1's rounding), times the two planes of alpha in five instructions.
// C layout of the result: column = lane & 15 (timing), rows 4 g + (0..3) = (re, im) of f = 8 q + 2 g and of f + 1 in frequency tile q.
// The product order is SMALLEST PARTIAL PRODUCTS FIRST, in both stages: the cross planes (2^-11 of the main product) are summed before the main product joins them, so
// their bits are not rounded away against it; this is what the rounding bound of include/rade_batch.h counts on.  The other hi hi + hi lo + lo hi sites of the project
// (the demodulator DFT of rade_rx.hip, bpf_fir_tile) keep the three products in separate chains and add them in the same order.
// A caller's un-scale factor undoes the sample scale, stage 1's 2^12, the moments' 2^-7 and stage 2's 2^10: operand_scale<12 + 3> where one factor does it all.
#ifndef RADE_CORR2_H
#define RADE_CORR2_H
#include "rade_dev.h"
#include "rade_devutil.h"
static_assert(RD_CORR_NRT * 16 == 2 * RD_NQ && RD_CORR_NKS * 32 == 2 * RD_M && RD_CORR_NFT * 16 == 2 * RD_NFC && RD_CORR_NRT == 2, "whole tiles and k-steps; stage 2's one k-step = two row tiles");
// halves from a table's start to a fragment plane (the lane's 8 halves at + 8 lane); CORR2_FRAG_BYTES: one plane in bytes
constexpr int corrq_frag(int tile, int s, int plane) { return ((tile * RD_CORR_NKS + s) * 2 + plane) * RD_FRAG_HALFS; }
constexpr int corra_frag(int q, int plane) { return (q * 2 + plane) * RD_FRAG_HALFS; }
#define CORR2_FRAG_BYTES (RD_FRAG_HALFS * 2)
// a scaled sample v = hi + lo (22 bits), (re, im) packed in one word per plane; every caller has its own layout for the two words
__device__ __forceinline__ void rx2_split16(float2 v, unsigned &hi, unsigned &lo)
{
    _Float16 h0, h1, l0, l1;
    split16(v.x, h0, l0); split16(v.y, h1, l1);
    hi = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
    lo = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
}
// ---- stage 1: one k-step.  a<tile><plane> are the table's fragments of the step, wh(rt) / wl(rt) the sample planes of timing tile rt as f16x8 --------------------
// search and acquisition: the cross products of both row tiles over all timing tiles, then the main products.  The receiver passes one accumulator array for
// both, acquisition keeps the main product apart and joins the two with one float32 addition per element (mom_split_by)
template <int RT, class WH, class WL>
__device__ __forceinline__ void corr2_kstep(f32x4 (&cross)[RT][2], f32x4 (&mainp)[RT][2], const f16x8 a0h, const f16x8 a0l, const f16x8 a1h, const f16x8 a1l, WH wh, WL wl)
{
#pragma unroll
    for (int rt = 0; rt < RT; rt++) cross[rt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0l, wh(rt), cross[rt][0], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) cross[rt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1l, wh(rt), cross[rt][1], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) cross[rt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0h, wl(rt), cross[rt][0], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) cross[rt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1h, wl(rt), cross[rt][1], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) mainp[rt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0h, wh(rt), mainp[rt][0], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) mainp[rt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1h, wh(rt), mainp[rt][1], 0, 0, 0);
}
// check_pilots: lo hi, hi lo, hi hi of ONE row tile nt over all timing tiles (its table fragments arrive per row tile)
template <int RT, class WH, class WL>
__device__ __forceinline__ void corr2_kstep_tile(f32x4 (&acc)[RT][2], int nt, const f16x8 ah, const f16x8 al, WH wh, WL wl)
{
#pragma unroll
    for (int rt = 0; rt < RT; rt++) acc[rt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wh(rt), acc[rt][nt], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) acc[rt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wl(rt), acc[rt][nt], 0, 0, 0);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) acc[rt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wh(rt), acc[rt][nt], 0, 0, 0);
}
// ---- stage 2 ------------------------------------------------------------------------------------------------------------------------------------------------------
// the lane's eight moments (get(j): element j & 3 of row tile j >> 2) as stage 2's B operand: 2^-7 of them in three binary16 planes
struct MomPlanes { f16x8 h, m, l; };
template <class Get> __device__ __forceinline__ MomPlanes mom_split_by(Get get)
{
    MomPlanes p;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float v = 0x1p-7f * get(j);
        const _Float16 h = (_Float16)v; const float r1 = v - (float)h;
        const _Float16 m = (_Float16)r1; const float r2 = r1 - (float)m;
        p.h[j] = h; p.m[j] = m; p.l[j] = (_Float16)r2;
    }
    return p;
}
__device__ __forceinline__ MomPlanes mom_split(const f32x4 a0, const f32x4 a1) { return mom_split_by([&](int j) { return j < 4 ? a0[j & 3] : a1[j & 3]; }); }
// one frequency tile (8 frequencies x (re, im)) of Dt for the 16 timings whose moments are in p
__device__ __forceinline__ f32x4 mom_expand(const f16x8 ah, const f16x8 al, const MomPlanes &p)
{
    f32x4 c = { 0.0f, 0.0f, 0.0f, 0.0f };
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, p.l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, p.m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, p.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, p.m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, p.h, c, 0, 0, 0);
    return c;
}
// sum over the four lane groups of a C tile, i.e. over a timing's frequencies: v_permlane16/32_swap (vector ALU, no LDS round trip); every lane gets the sum
__device__ __forceinline__ float corr2_group_sum(float s)
{
    const auto p16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    s = __uint_as_float(p16[0]) + __uint_as_float(p16[1]);
    const auto p32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return __uint_as_float(p32[0]) + __uint_as_float(p32[1]);
}
#endif
