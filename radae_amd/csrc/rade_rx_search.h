// rade_rx_search.h -- the pilot search of the unsynchronised receiver: acquisition.detect_pilots (dsp.py:178-231; the noise estimate sigma_r dsp.py:218-220) as
// the two-stage correlator rx2_detect_q, and the workgroup reductions every stage of k_rx_sync2 uses (block_argmax2, block_sum_multi2).
// Part of rade_rx.hip's translation unit, behind RxShared2.  Members of RxShared2 it owns: sA, sA2 (the correlator's tables), srxh / srxl (rx_buf as binary16
// planes: written by the caller, read here), rowsum1 / rowsum2 (written here, kept across calls), redf / redi / redj slots 1..NW2 and redd (reduction scratch).
#include "rade_corr2.h"
// ---- rx_buf as matrix-core operands: two binary16 planes under one power-of-two scale (the pilot search, check_pilots, the demodulator's window) ----
// The scale comes from the largest component of the filtered samples of this call and the two before it (all rx_buf holds): it lands in [2^7, 2^8).
// rx_unsc undoes it together with the 2^12 of the correlators' stage-1 table.
__device__ __forceinline__ void rx2_operand_scale(const RxScalars *S, float &rx_sc, float &rx_unsc) { operand_scale<12>(max(max(S->rxmax_cur, S->rxmax_h0), S->rxmax_h1), rx_sc, rx_unsc); }
__device__ __forceinline__ float sigma_r_from_sums(double t1, double t2)
{   // dsp.py:218-220: (mean|Dt1| + mean|Dt2|)/sqrt(pi/2)/2 in float32
    const float k = (float)sqrt(PI_D / 2.0);
    const float m1 = (float)(t1 / (RD_NMF * RD_NFC)) / k, m2 = (float)(t2 / (RD_NMF * RD_NFC)) / k;
    return (m1 + m2) / 2.0f;
}

// ---- workgroup reductions on four wavefronts (ties go to the smallest (k0, k1); every thread gets the result) ------------------------------------
__device__ void block_argmax2(RxShared2 *sh, float &v, int &k0, int &k1)
{
    const int tid = rx_tid(), lane = tid & 63, wave = tid >> 6;
#define ARGMAX_STEP(CTRL) do { const float ov = quad_dpp<CTRL>(v); const int o0 = quad_dpp_i<CTRL>(k0), o1 = quad_dpp_i<CTRL>(k1); \
        if (ov > v || (ov == v && (o0 < k0 || (o0 == k0 && o1 < k1)))) { v = ov; k0 = o0; k1 = o1; } } while (0)
    ARGMAX_STEP(QUAD_XOR1); ARGMAX_STEP(QUAD_XOR2); ARGMAX_STEP(ROW_ROR4); ARGMAX_STEP(ROW_ROR8);
#undef ARGMAX_STEP
    {
        float bv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)); int b0 = __builtin_amdgcn_readlane(k0, 0), b1 = __builtin_amdgcn_readlane(k1, 0);
#pragma unroll
        for (int r = 1; r < 4; r++) {
            const float ov = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * r)); const int o0 = __builtin_amdgcn_readlane(k0, 16 * r), o1 = __builtin_amdgcn_readlane(k1, 16 * r);
            if (ov > bv || (ov == bv && (o0 < b0 || (o0 == b0 && o1 < b1)))) { bv = ov; b0 = o0; b1 = o1; }
        }
        v = bv; k0 = b0; k1 = b1;
    }
    if (lane == 0) { sh->redf[1 + wave] = v; sh->redi[1 + wave] = k0; sh->redj[1 + wave] = k1; }
    __syncthreads();
    float bv = sh->redf[1]; int b0 = sh->redi[1], b1 = sh->redj[1];
#pragma unroll
    for (int w = 1; w < NW2; w++) {
        const float ov = sh->redf[1 + w]; const int o0 = sh->redi[1 + w], o1 = sh->redj[1 + w];
        if (ov > bv || (ov == bv && (o0 < b0 || (o0 == b0 && o1 < b1)))) { bv = ov; b0 = o0; b1 = o1; }
    }
    v = bv; k0 = b0; k1 = b1;
}
template <int NV>
__device__ void block_sum_multi2(RxShared2 *sh, double (&v)[NV])
{
    const int tid = rx_tid(), lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NV; k++) v[k] = wave_sum_f64(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; k++) sh->redd[wave * NV + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; k++) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW2; w++) t += sh->redd[w * NV + k];
        v[k] = t;
    }
}
__device__ float sigma_r_from_rowsums2(RxShared2 *sh)
{
    double v[2] = { 0.0, 0.0 };
    for (int t = rx_tid(); t < RD_NMF; t += NT2) { v[0] += (double)sh->rowsum1[t]; v[1] += (double)sh->rowsum2[t]; }
    block_sum_multi2<2>(sh, v);
    return sigma_r_from_sums(v[0], v[1]);
}

// ---- |Dt| surfaces on the matrix cores: acquisition.detect_pilots (dsp.py:178-231) for all 960 timings x 40 frequencies of a frame, by the two-stage correlator of
// rade_corr2.h (the algebra, the tables, the product order).  What is the search's own:
//   * a wavefront owns 15 timing tiles (240 timings) and walks them in groups of RT = 5;
//   * stage 1's A operands (table) are staged through LDS by the whole workgroup, double-buffered, one barrier per stage of two k-steps;
//   * the B operand of (timing tile T, k-step s) is the fragment of (T + s, 0): the window slides by one tile per k-step, so a group reads RT + 9 fragments
//     from the planes instead of 10 RT.
// Outputs: |Dt2| -- and |Dt1| when not cached -- to the stream's cache in HBM, the row sums to rowsum1 / rowsum2, the lane's best (Dt1 + Dt2, t, f).  rx_unsc undoes
// the scales of the rx planes and the stage-1 table; the 2^-7 of the moments and the 2^10 of the stage-2 table are undone here.
__device__ __forceinline__ void rx2_detect_q(RxShared2 *sh, const unsigned short *corrq16_, const unsigned short *corra16_, float *cache_, int cached, int oldb, int newb,
                                             float rx_unsc_, float &best, int &bt, int &bfi)
{
    constexpr int RT = 5, NTF = RD_CORR_NFT, NKS = RD_CORR_NKS, TPW = 15;
    static_assert(TPW * NW2 * 16 == RD_NMF && TPW % RT == 0, "timing tiles per wavefront");
    static_assert(NKS % 2 == 0 && NT2 == 4 * 64, "a stage of two k-steps of both row tiles = 8 fragment planes: two 16-byte chunks per thread");
    const int tid = rx_tid(), wave = rx2_wave(), lane = tid & 63, i = lane & 15, g = lane >> 4;
    const float rx_unsc = rx_unsc_ * 0x1p-3f;
    // stage 1's table [tile][k-step][plane][lane] (16 B per lane): a stage buffer holds two k-steps of both tiles, chunk u = 256 tile + 128 (k-step & 1) + 64 plane + lane,
    // i.e. thread tid brings chunks tid and 256 + tid: one lane offset under two uniform bases
    const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc((void *)uni_ptr(corrq16_), 0, RD_CORRQ16_HALFS * 2, 0x00020000);
    const int vo = tid * 16;
    u32x4 stg[2];
    auto stage_load = [&](int sb) {
        stg[0] = __builtin_amdgcn_raw_buffer_load_b128(qrs, vo, corrq_frag(0, 2 * sb, 0) * 2, 0); stg[1] = __builtin_amdgcn_raw_buffer_load_b128(qrs, vo, corrq_frag(1, 2 * sb, 0) * 2, 0);
    };
    auto stage_store = [&](int buf) { _Float16 *d = &sh->sA[buf][tid * 8]; *(u32x4 *)d = stg[0]; *(u32x4 *)(d + 4 * RD_FRAG_HALFS) = stg[1]; };
    PH2_T0();
    {   // stage 2's table, whole: 10 fragment planes = 640 x 16 B, four planes per round of the workgroup
        static_assert(RD_CORRA16_HALFS == 10 * RD_FRAG_HALFS, "two rounds of all four wavefronts and one of two");
        const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc((void *)uni_ptr(corra16_), 0, RD_CORRA16_HALFS * 2, 0x00020000);
        const u32x4 t0 = __builtin_amdgcn_raw_buffer_load_b128(ars, vo, 0, 0), t1 = __builtin_amdgcn_raw_buffer_load_b128(ars, vo, 4 * CORR2_FRAG_BYTES, 0);
        u32x4 t2 = { 0u, 0u, 0u, 0u };
        if (wave < 2) t2 = __builtin_amdgcn_raw_buffer_load_b128(ars, vo, 8 * CORR2_FRAG_BYTES, 0);
        stage_load(0);
        _Float16 *d = &sh->sA2[tid * 8];
        *(u32x4 *)d = t0; *(u32x4 *)(d + 4 * RD_FRAG_HALFS) = t1;
        if (wave < 2) *(u32x4 *)(d + 8 * RD_FRAG_HALFS) = t2;
        stage_store(0);
    }
    float lbest = best; int lkey = 0x7fffffff;
    int pb = 0;                                                 // the stage buffer being read: flips every stage (five stages per group: the parity runs on across groups)
    __syncthreads();
    PH2(15);
#pragma unroll 1
    for (int pass = cached ? 1 : 0; pass < 2; pass++) {
        const unsigned *ph = sh->srxh + pass * RD_NMF + i + 4 * g, *pl = sh->srxl + pass * RD_NMF + i + 4 * g;
        const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void *)uni_ptr(cache_ + (size_t)(pass ? newb : oldb) * RD_NFC * RD_NMF), 0, RD_NFC * RD_NMF * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc((void *)uni_ptr(cache_ + (size_t)oldb * RD_NFC * RD_NMF), 0, RD_NFC * RD_NMF * 4, 0x00020000);
        float *rowsum = pass ? sh->rowsum2 : sh->rowsum1;
#pragma unroll 1
        for (int grp = 0; grp < TPW / RT; grp++) {
            const int T0 = wave * TPW + grp * RT;
            f32x4 acc1[RT][2];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) { acc1[rt][0] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f }; acc1[rt][1] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f }; }
            u32x4 wh[RT + 1], wl[RT + 1];
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int j = 0; j < 4; j++) { wh[rt][j] = ph[16 * (T0 + rt) + j]; wl[rt][j] = pl[16 * (T0 + rt) + j]; }
#pragma unroll
            for (int sb = 0; sb < NKS / 2; sb++) {
                stage_load(sb == NKS / 2 - 1 ? 0 : sb + 1);
#pragma unroll
                for (int ds = 0; ds < 2; ds++) {
                    const int sidx = 2 * sb + ds;
                    // fragment F of the sliding window lives in slot (F - T0) mod (RT + 1): tile rt reads slot (rt + sidx) mod (RT + 1), the fragment the NEXT k-step adds goes
                    // into the slot the first tile just left (all indices are compile-time: the loops are unrolled).  Rounds 3-4 shifted the window through the registers
                    // instead: 40 moves per k-step behind the matrix instructions
                    if (sidx < NKS - 1) {
#pragma unroll
                        for (int j = 0; j < 4; j++) { wh[(RT + sidx) % (RT + 1)][j] = ph[16 * (T0 + RT + sidx) + j]; wl[(RT + sidx) % (RT + 1)][j] = pl[16 * (T0 + RT + sidx) + j]; }
                    }
                    const _Float16 *Ab = &sh->sA[pb][lane * 8];          // the stage buffer: [row tile][k-step & 1][plane][lane][8]
                    const f16x8 a0h = *(const f16x8 *)(Ab + ((0 * 2 + ds) * 2 + 0) * RD_FRAG_HALFS), a0l = *(const f16x8 *)(Ab + ((0 * 2 + ds) * 2 + 1) * RD_FRAG_HALFS);
                    const f16x8 a1h = *(const f16x8 *)(Ab + ((1 * 2 + ds) * 2 + 0) * RD_FRAG_HALFS), a1l = *(const f16x8 *)(Ab + ((1 * 2 + ds) * 2 + 1) * RD_FRAG_HALFS);
                    __builtin_amdgcn_sched_barrier(0);
                    corr2_kstep<RT>(acc1, acc1, a0h, a0l, a1h, a1l, [&](int rt) { return __builtin_bit_cast(f16x8, wh[(rt + sidx) % (RT + 1)]); },
                                    [&](int rt) { return __builtin_bit_cast(f16x8, wl[(rt + sidx) % (RT + 1)]); });
                    __builtin_amdgcn_sched_barrier(0);
                }
                stage_store(pb ^ 1);
                pb ^= 1;
                __syncthreads();
            }
            PH2(16);
            // ---- stage 2 and the epilogue, one timing tile at a time.  The surfaces in the stream's HBM cache are only ever read back by the lane that wrote them
            // (|Dt2| of this call is |Dt1| of the next), so their layout is the lane's: per (wavefront, group, timing tile) 64 lanes x 10 values (frequency tile,
            // then the two frequencies) as two 16-byte vectors [lane] + one 8-byte vector [lane]: fully coalesced.
            f16x8 A2h[NTF], A2l[NTF];
#pragma unroll
            for (int q = 0; q < NTF; q++) { A2h[q] = *(const f16x8 *)&sh->sA2[corra_frag(q, 0) + lane * 8]; A2l[q] = *(const f16x8 *)&sh->sA2[corra_frag(q, 1) + lane * 8]; }
            const int gb = (wave * (TPW / RT) + grp) * RT * 2560;         // byte offset of the group's block; 2560 B per timing tile
            float pv[2][2 * NTF];
            auto pv_load = [&](int slot, int rt) {
                const u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(prs, lane * 16, gb + rt * 2560, 0), v1 = __builtin_amdgcn_raw_buffer_load_b128(prs, lane * 16, gb + rt * 2560 + 1024, 0);
                const u32x2 v2 = __builtin_amdgcn_raw_buffer_load_b64(prs, lane * 8, gb + rt * 2560 + 2048, 0);
#pragma unroll
                for (int k = 0; k < 4; k++) { pv[slot][k] = __uint_as_float(v0[k]); pv[slot][4 + k] = __uint_as_float(v1[k]); }
                pv[slot][8] = __uint_as_float(v2[0]); pv[slot][9] = __uint_as_float(v2[1]);
            };
            if (pass) pv_load(0, 0);
            const int tb = 16 * T0 + i;
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                if (pass && rt + 1 < RT) pv_load((rt + 1) & 1, rt + 1);
                const MomPlanes mp = mom_split(acc1[rt][0], acc1[rt][1]);
                float dd[2 * NTF], rs = 0.0f;
#pragma unroll
                for (int q = 0; q < NTF; q++) {
                    const f32x4 c = mom_expand(A2h[q], A2l[q], mp);
                    const float d0 = rx_unsc * __builtin_amdgcn_sqrtf(fmaf(c[0], c[0], c[1] * c[1])), d1 = rx_unsc * __builtin_amdgcn_sqrtf(fmaf(c[2], c[2], c[3] * c[3]));
                    rs += d0; rs += d1;
                    dd[2 * q] = d0; dd[2 * q + 1] = d1;
                }
                rs = corr2_group_sum(rs);                                  // the other three lane groups hold the row's other frequencies
                __builtin_amdgcn_raw_buffer_store_b128((u32x4){ __float_as_uint(dd[0]), __float_as_uint(dd[1]), __float_as_uint(dd[2]), __float_as_uint(dd[3]) }, drs, lane * 16, gb + rt * 2560, 0);
                __builtin_amdgcn_raw_buffer_store_b128((u32x4){ __float_as_uint(dd[4]), __float_as_uint(dd[5]), __float_as_uint(dd[6]), __float_as_uint(dd[7]) }, drs, lane * 16, gb + rt * 2560 + 1024, 0);
                __builtin_amdgcn_raw_buffer_store_b64((u32x2){ __float_as_uint(dd[8]), __float_as_uint(dd[9]) }, drs, lane * 8, gb + rt * 2560 + 2048, 0);
                // every lane keeps its own best (t ascending, then f ascending, strict >: the earliest wins); block_argmax2 orders the lanes the same way.  Branch-free,
                // (t, f) packed in one register
                const int t = tb + 16 * rt;
                if (pass) {
#pragma unroll
                    for (int q = 0; q < NTF; q++) {
                        const int k0 = (t << 6) | (8 * q + 2 * g);
                        const float s0 = pv[rt & 1][2 * q] + dd[2 * q], s1 = pv[rt & 1][2 * q + 1] + dd[2 * q + 1];
                        const bool c0 = s0 > lbest; lbest = c0 ? s0 : lbest; lkey = c0 ? k0 : lkey;
                        const bool c1 = s1 > lbest; lbest = c1 ? s1 : lbest; lkey = c1 ? k0 + 1 : lkey;
                    }
                }
                if (g == 0) rowsum[t] = rs;
            }
            PH2(17);
        }
        __syncthreads();
        PH2(18);
    }
    best = lbest; bt = lkey >> 6; bfi = lkey & 63;
}
