// rade_rx_check.h -- acquisition.check_pilots (dsp.py:273-320): the row refreshes of the noise estimate in the synchronised state, 48 pseudo-random timings x
// {Dt1, Dt2} x 40 frequencies per call (check2_rows_q), by the two-stage correlator of rade_corr2.h (the algebra, the tables, the product order).
// Part of rade_rx.hip's translation unit.  Members of RxShared2 it reads: rxhl (rx_buf's planes, written by the caller), rows48 (the row draws); it writes
// rowsum1 / rowsum2 at the drawn rows.
// check_pilots' row refreshes of one modem frame, NRT tiles of 16 row draws per wavefront, by the two-stage correlator: the three tiles of 16 row draws against the
// moment table (A fragments straight from L2, two k-steps ahead: 40 KB per call and wavefront instead of 60 + 40 over the two wavefronts a frame had), the moments
// expanded to the 40 frequencies, |Dt| summed over them in the wavefront -> rowsum1 / rowsum2 directly (rounds 3-4: partial sums of two wavefronts through a table and
// a second barrier).  The gathers: lane (row draw i, group g) needs samples 16 s + 4 g .. + 3 of its window in k-step s, and the windows start at random offsets, so the
// lanes of a read hit banks at random whatever the layout.  What the layout decides is how many LDS cycles that costs: with a sample's two plane words side by side
// one ds_read_b64 (64 banks, 2 cycles conflict-free) brings what took two ds_read_b32 (32 banks, 2 cycles each) -- measured by bank model over random draws: 6.6 against
// 13.1 LDS cycles per sample and wave-instruction -- and every window is read by ONE wavefront, not two.
typedef __attribute__((address_space(3))) const u32x2 lds_cu32x2;
// pre() runs once behind the first table requests, side(s) behind the matrix instructions of k-step s: work of the caller's that does not depend on this
// function's results, placed where the wavefront would otherwise wait for table fragments from L2 (6 NRT matrix instructions per k-step cover 100-200 cycles of
// a round trip of 800)
template <int NRT, int DA, class Pre, class Side>
__device__ __forceinline__ void check2_rows_q(RxShared2 *sh, const unsigned short *corrq16_, const unsigned short *corra16_, int frame, int rt0, int lane, float rx_unsc_, Pre pre, Side side)
{
    const int i = lane & 15, g = lane >> 4;
    const float rx_unsc = rx_unsc_ * 0x1p-3f;
    const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc((void *)uni_ptr(corrq16_), 0, RD_CORRQ16_HALFS * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc((void *)uni_ptr(corra16_), 0, RD_CORRA16_HALFS * 2, 0x00020000);
    // four address registers per row tile that the compiler cannot see through: merged into ds_read2_b64 (or an unaligned ds_read_b128) the reads would run at half rate
    lds_cu32x2 *px[NRT][4];
#pragma unroll
    for (int rt = 0; rt < NRT; rt++) {
        lds_cu32x2 *b0 = (lds_cu32x2 *)&sh->rxhl[0] + (sh->rows48[(rt0 + rt) * 16 + i] + frame * RD_NMF + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; j++) { px[rt][j] = b0 + j; asm volatile("" : "+v"(px[rt][j])); }
    }
    f32x4 acc1[NRT][2];
#pragma unroll
    for (int rt = 0; rt < NRT; rt++) { acc1[rt][0] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f }; acc1[rt][1] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f }; }
    u32x4 A[DA][4];                                            // [k-step mod DA][2 tile + plane]: DA k-steps of table fragments in flight
    auto fetchA = [&](int slot, int s) {
#pragma unroll
        for (int u = 0; u < 4; u++) A[slot][u] = __builtin_amdgcn_raw_buffer_load_b128(qrs, lane * 16, corrq_frag(u >> 1, s, u & 1) * 2, 0);
    };
    u32x4 bh[2][NRT], bl[2][NRT];
    auto rows = [&](int slot, int s) {
#pragma unroll
        for (int rt = 0; rt < NRT; rt++)
#pragma unroll
            for (int j = 0; j < 4; j++) { const u32x2 v = px[rt][j][16 * s]; bh[slot][rt][j] = v[0]; bl[slot][rt][j] = v[1]; }
    };
#pragma unroll
    for (int d = 0; d < DA; d++) fetchA(d, d);
    pre();
    rows(0, 0);
    constexpr int NKS = RD_CORR_NKS, NTF = RD_CORR_NFT;
    u32x4 A2[2 * NTF];                                         // stage 2's fragments [2 q + plane]: requested under the last k-steps
#pragma unroll
    for (int s = 0; s < NKS; s++) {
        if (s + 1 < NKS) rows((s + 1) & 1, s + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int nt = 0; nt < RD_CORR_NRT; nt++)
            corr2_kstep_tile<NRT>(acc1, nt, __builtin_bit_cast(f16x8, A[s % DA][2 * nt]), __builtin_bit_cast(f16x8, A[s % DA][2 * nt + 1]),
                                  [&](int rt) { return __builtin_bit_cast(f16x8, bh[s & 1][rt]); }, [&](int rt) { return __builtin_bit_cast(f16x8, bl[s & 1][rt]); });
        __builtin_amdgcn_sched_barrier(0);
        if (s + DA < NKS) fetchA(s % DA, s + DA);
        if (s == NKS - DA) {
#pragma unroll
            for (int u = 0; u < 2 * NTF; u++) A2[u] = __builtin_amdgcn_raw_buffer_load_b128(ars, lane * 16, u * CORR2_FRAG_BYTES, 0);
        }
        side(s);
        __builtin_amdgcn_sched_barrier(0);
    }
    float *rowsum = frame ? sh->rowsum2 : sh->rowsum1;
#pragma unroll
    for (int rt = 0; rt < NRT; rt++) {
        const MomPlanes mp = mom_split(acc1[rt][0], acc1[rt][1]);
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < NTF; q++) {    // the C tile's columns are the 16 row draws
            const f32x4 c = mom_expand(__builtin_bit_cast(f16x8, A2[2 * q]), __builtin_bit_cast(f16x8, A2[2 * q + 1]), mp);
            s += rx_unsc * __builtin_amdgcn_sqrtf(fmaf(c[0], c[0], c[1] * c[1])) + rx_unsc * __builtin_amdgcn_sqrtf(fmaf(c[2], c[2], c[3] * c[3]));
        }
        s = corr2_group_sum(s);             // the other three lane groups hold the row's other frequencies
        // (two draws of the same row compute the same sum from the same samples: whichever store lands last, the value is the same)
        if (g == 0) rowsum[sh->rows48[(rt0 + rt) * 16 + i]] = s;
    }
}
