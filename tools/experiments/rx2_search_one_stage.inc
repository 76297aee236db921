// Not compiled.  Rounds 3-4's pilot search of k_rx_sync2: the |Dt| surface as ONE split-binary16 GEMM against the 80-row table of p_w (150 matrix instructions per
// tile of 16 timings).  Replaced in round 5 by the two-stage form (16 polynomial moments, then their expansion: 85 per tile; rade_rx.hip: rx2_detect_q).
// LDS: _Float16 sA[2][5 * 2 * 64 * 8] (one k-step of the table, double-buffered).
// ---- |Dt| surfaces on the matrix cores ----------------------------------------------------------------------------------------------
// acquisition.detect_pilots (dsp.py:178-231): Dt[t, f] = sum_m conj(rx[t + m]) p_w[m, f] for all 960 timings x 40 frequencies of a frame.
// The retired round-3 kernel did this by FFT convolution on the vector ALU (one 2048-point inverse transform per frequency): 52 % of ALL vector
// instructions of a k_rx_sync2 launch on the bench workload although only one call in eight is in the search state (tools/rx2_census.sh),
// and with two workgroups per CU the vector ALU is the shared resource.  Here the same sums are the real GEMM check_pilots already runs
// for its 48 rows -- [80 = (f, re | im)] x [320 = (m, re | im)] times the Toeplitz matrix rx[t + m] -- on v_mfma_f32_16x16x32_f16 with both
// operands in two binary16 planes (hi hi + hi lo + lo hi: 22 bits): 9000 instructions per surface, 36 k cycles per SIMD, and under 10 %
// of the FFT form's vector instructions (the |.|, the row sums and the running arg-max are all that is left).
//   * a wavefront owns 15 timing tiles (240 timings) and walks them in groups of RT = 5 against all five frequency tiles: 25 accumulators;
//   * the A operands (table, 100 KB: too big for LDS) are staged one k-step (10 KB) at a time by the whole workgroup, double-buffered,
//     one barrier per k-step: 300 KB of L2 reads per surface and workgroup instead of 1.2 MB if every wavefront fetched its own;
//   * the B operand of (timing tile T, k-step s) is the fragment of (T + s, 0): the window slides by one tile per k-step, so a group
//     reads RT + 9 fragments from the planes instead of 10 RT.
// Outputs: |Dt2| (and |Dt1| when not cached) to the stream's cache in HBM, the row sums to rowsum1 / rowsum2, and the lane's best
// (Dt1 + Dt2, t, f) with the earliest t and lowest f on ties, to be reduced by block_argmax2.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void rx2_detect_mfma(RxShared2 *sh, const unsigned short *corr16_, float *cache_, int cached, int oldb, int newb, float rx_unsc,
                                                float &best, int &bt, int &bfi)
{
    constexpr int RT = 5, NTF = 5, TPW = 15;
    static_assert(TPW * NW2 * 16 == RD_NMF && TPW % RT == 0, "timing tiles per wavefront");
    typedef const __attribute__((address_space(1))) f16x8 glb_f16x8_t;
    const int tid = rx_tid(), wave = rx2_wave(), lane = tid & 63, i = lane & 15, g = lane >> 4;
    // chunk c = 128 nt + 64 plane + lane of a k-step (640 x 16 B): thread tid takes c = tid, tid + 256 and (wavefronts 0 / 1) tid + 512, i.e. the
    // same lane offset under three uniform bases
    // Buffer loads (uniform descriptor + 32-bit lane offset + scalar offset): with plain pointers the compiler keeps one 64-bit address
    // per (base, k-step) in VGPRs, spills them, and every k-step starts with scratch reloads under s_waitcnt vmcnt(0).
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc((void *)uni_ptr(corr16_), 0, 5 * 10 * 2048, 0x00020000);
    const int vo = (((tid >> 7) * 10) * 128 + (tid & 127)) * 16;
    const bool third = wave < 2;                       // wave-uniform
    u32x4 stg[3];
    auto stage_load = [&](int sidx) {
        stg[0] = __builtin_amdgcn_raw_buffer_load_b128(crs, vo, sidx * 2048, 0); stg[1] = __builtin_amdgcn_raw_buffer_load_b128(crs, vo, sidx * 2048 + 2 * 10 * 2048, 0);
        if (third) stg[2] = __builtin_amdgcn_raw_buffer_load_b128(crs, vo, sidx * 2048 + 4 * 10 * 2048, 0);
    };
    auto stage_store = [&](int buf) {
        _Float16 *d = &sh->sA[buf][tid * 8];
        *(u32x4 *)d = stg[0]; *(u32x4 *)(d + 256 * 8) = stg[1];
        if (third) *(u32x4 *)(d + 512 * 8) = stg[2];
    };
    PH2_T0();
    float lbest = best; int lkey = 0x7fffffff;                      // (t << 6) | f of the best; callers start from best = -1, which the first sum replaces
    stage_load(0); stage_store(0);
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
            f32x4 acc[RT][NTF];
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int q = 0; q < NTF; q++) acc[rt][q] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
            u32x4 wh[RT + 1], wl[RT + 1];
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int j = 0; j < 4; j++) { wh[rt][j] = ph[16 * (T0 + rt) + j]; wl[rt][j] = pl[16 * (T0 + rt) + j]; }
#pragma unroll
            for (int sidx = 0; sidx < 10; sidx++) {
                stage_load(sidx == 9 ? 0 : sidx + 1);
                if (sidx < 9) {
#pragma unroll
                    for (int j = 0; j < 4; j++) { wh[RT][j] = ph[16 * (T0 + RT + sidx) + j]; wl[RT][j] = pl[16 * (T0 + RT + sidx) + j]; }
                }
                const _Float16 *Ab = &sh->sA[sidx & 1][lane * 8];
                // the next frequency tile's fragments are in flight while this one's 15 instructions issue (left to itself the compiler
                // reads each fragment right before its use and waits for it: ten exposed LDS latencies per k-step, half the phase)
                f16x8 ch[2], cl[2];
                ch[0] = *(const f16x8 *)(Ab); cl[0] = *(const f16x8 *)(Ab + 512);
#pragma unroll
                for (int q = 0; q < NTF; q++) {
                    if (q + 1 < NTF) { ch[(q + 1) & 1] = *(const f16x8 *)(Ab + ((q + 1) * 2) * 512); cl[(q + 1) & 1] = *(const f16x8 *)(Ab + ((q + 1) * 2 + 1) * 512); }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cl[q & 1], __builtin_bit_cast(f16x8, wh[rt]), acc[rt][q], 0, 0, 0);
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ch[q & 1], __builtin_bit_cast(f16x8, wl[rt]), acc[rt][q], 0, 0, 0);
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ch[q & 1], __builtin_bit_cast(f16x8, wh[rt]), acc[rt][q], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int rt = 0; rt < RT; rt++) { wh[rt] = wh[rt + 1]; wl[rt] = wl[rt + 1]; }
                stage_store((sidx & 1) ^ 1);
                __syncthreads();
            }
            PH2(16);
            // C layout: column = lane & 15 (timing), rows 4 g + r = (re, im) of f = 8 q + 2 g and f + 1
            const int tb = 16 * T0 + i;
            // The surfaces in the stream's HBM cache are only ever read back by the lane that wrote them (|Dt2| of this call is |Dt1| of the
            // next), so their layout is the lane's: per (wavefront, group) 64 lanes x 50 values (rt-major, then frequency tile, then the two
            // frequencies) as twelve 16-byte vectors [k][lane] + one 8-byte vector [lane].  13 fully coalesced instructions per group and
            // direction instead of 50 single dwords (store ISSUE was the epilogue: ~10 k cycles per group).
            const int gb = (wave * (TPW / RT) + grp) * 64 * 2 * RT * NTF * 4;     // byte offset of the group's block
            // all of the group's |Dt1| (HBM latency) are requested before any arithmetic; the accumulators turn into |Dt2| in place (4 -> 2
            // registers per tile), which is what makes room for them
            float pv[RT * 2 * NTF];
            if (pass) {
#pragma unroll
                for (int k = 0; k < 12; k++) {
                    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(prs, lane * 16, gb + k * 1024, 0);
                    pv[4 * k] = __uint_as_float(v[0]); pv[4 * k + 1] = __uint_as_float(v[1]); pv[4 * k + 2] = __uint_as_float(v[2]); pv[4 * k + 3] = __uint_as_float(v[3]);
                }
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(prs, lane * 8, gb + 12 * 1024, 0);
                pv[48] = __uint_as_float(v[0]); pv[49] = __uint_as_float(v[1]);
            }
            float dd[RT * 2 * NTF], rsum[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                float rs = 0.0f;
#pragma unroll
                for (int q = 0; q < NTF; q++) {
                    const f32x4 c = acc[rt][q];
                    const float d0 = rx_unsc * __builtin_amdgcn_sqrtf(fmaf(c[0], c[0], c[1] * c[1])), d1 = rx_unsc * __builtin_amdgcn_sqrtf(fmaf(c[2], c[2], c[3] * c[3]));
                    rs += d0; rs += d1;
                    dd[rt * 2 * NTF + 2 * q] = d0; dd[rt * 2 * NTF + 2 * q + 1] = d1;
                }
                {   // the other three lane groups hold the row's other frequencies: v_permlane16/32_swap (vector ALU, no LDS round trip)
                    const auto p16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
                    rs = __uint_as_float(p16[0]) + __uint_as_float(p16[1]);
                    const auto p32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(rs), __float_as_uint(rs), false, false);
                    rs = __uint_as_float(p32[0]) + __uint_as_float(p32[1]);
                }
                rsum[rt] = rs;
            }
#pragma unroll
            for (int k = 0; k < 12; k++)
                __builtin_amdgcn_raw_buffer_store_b128((u32x4){ __float_as_uint(dd[4 * k]), __float_as_uint(dd[4 * k + 1]), __float_as_uint(dd[4 * k + 2]), __float_as_uint(dd[4 * k + 3]) }, drs, lane * 16, gb + k * 1024, 0);
            __builtin_amdgcn_raw_buffer_store_b64((u32x2){ __float_as_uint(dd[48]), __float_as_uint(dd[49]) }, drs, lane * 8, gb + 12 * 1024, 0);
            // every lane keeps its own best (t ascending, then f ascending, strict >: the earliest wins); block_argmax2 orders the lanes the same
            // way.  Branch-free, (t, f) packed in one register: as conditional blocks the compiler kept the three in scratch memory and every
            // one of the 50 updates was a store + load under s_waitcnt vmcnt(0).
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const int t = tb + 16 * rt;
                if (pass) {
#pragma unroll
                    for (int q = 0; q < NTF; q++) {
                        const int k0 = (t << 6) | (8 * q + 2 * g);
                        const float s0 = pv[rt * 2 * NTF + 2 * q] + dd[rt * 2 * NTF + 2 * q], s1 = pv[rt * 2 * NTF + 2 * q + 1] + dd[rt * 2 * NTF + 2 * q + 1];
                        const bool c0 = s0 > lbest; lbest = c0 ? s0 : lbest; lkey = c0 ? k0 : lkey;
                        const bool c1 = s1 > lbest; lbest = c1 ? s1 : lbest; lkey = c1 ? k0 + 1 : lkey;
                    }
                }
                if (g == 0) rowsum[t] = rsum[rt];
            }
            PH2(17);
        }
        __syncthreads();
        PH2(18);
    }
    best = lbest; bt = lkey >> 6; bfi = lkey & 63;
}

