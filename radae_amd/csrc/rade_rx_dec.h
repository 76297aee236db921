// rade_rx_dec.h -- the decoder stage inside the receiver kernel: CoreDecoder (radae_base.py:358-430; GRU step radae_base.py:97-108) for the at most 12 rows of a
// chunk of one stream on the four wavefronts of its workgroup.  dq2_layers is the stage; rx2_decode_pending (rade_rx.hip) feeds it the pending rows.
// Part of rade_rx.hip's translation unit (needs NT2, rx2_wave, PH2).  Owns no member of RxShared2 by name: DecShared2 overlays the whole of its big union
// through dec_raw (64 KB), which is why rx_buf and the row sums are parked in the stream's HBM record while the stage runs.
// ---- LDS layout helpers and product descriptors ----
#define DQ_XB 96                 // 8-half blocks per x row
#define DQ_HB 16                 // blocks per GRU-output row (12 used)
#define DQ_PEND_MAX 64           // pending rows a stream can hold (engine: dec_rows <= 63)
// floats per row of the GRU-input sums in LDS: 288 + 4.  With 288 (= 9 x 32) every row started on the same bank, and the 16-byte accesses of a product's epilogue -- lanes = rows --
// were 8-way conflicts: two thirds of ALL bank-conflict cycles of the kernel (tools/rx2_lds_conflicts.sh, round 5); with 292 a row starts 16 bytes further on.
#ifndef DQ_GIS
#define DQ_GIS (RM_DEC_G + 4)
#endif
static_assert(DQ_XB * 8 >= RD_DEC_W && DQ_HB * 8 >= RM_DEC_H, "an x row and a GRU-output row fit their LDS rows");
// half index of x[logical row t][col] inside a plane; the history row is logical -1 (swizzle key 15), the zero row needs no key
__device__ __forceinline__ int dq_xoff(int t, int col) { return (t + 1) * (DQ_XB * 8) + ((((col >> 3) ^ (t & 15)) << 3) | (col & 7)); }
__device__ __forceinline__ int dq_hoff(int t, int col) { return t * (DQ_HB * 8) + ((((col >> 3) ^ (t & 15)) << 3) | (col & 7)); }

enum { DQ_OUT_X = 0, DQ_OUT_GI = 1, DQ_OUT_GLOBAL = 2 };
struct DqGemm {
    const unsigned short *wa; int nct;     // rd_pack_weights_f16x2_a16: [K/32][nct][2 planes][64 lanes][8]
    const float *bias; int N;              // bias may be null; N = valid output columns
    const float *wscale;                   // non-null: int8-exact layer, ONE plane of integers, wscale[n] = the column's scale; null: two planes of 2^10 w
    int from_hb;                           // B operand: 0 = the x planes, 1 = the GRU-output planes
    int ktap;                              // k-steps [0, ktap) read the PREVIOUS row (conv tap 0), the rest the row itself
    int ks0, nks;                          // k-steps of the weight's K axis this product covers
    int init_gi;                           // accumulators start from gi[t][n] (fix-up products) instead of zero
    int out, ocol, act;                    // DQ_OUT_*; first x column (DQ_OUT_X); act 0 none, 1 tanh+clamp, 2 GLU
    float *gout; int gstride;              // DQ_OUT_GLOBAL
};
#define DQ2_ROWS 12
#ifndef RX2_DQ_D3
#define RX2_DQ_D3 4
#endif

struct DecShared2 {
    __attribute__((aligned(16))) _Float16 xh[DQ2_ROWS + 2][DQ_XB * 8];   // physical row 0: conv history, 1..12: the chunk, 13: zeros
    __attribute__((aligned(16))) _Float16 xl[DQ2_ROWS + 2][DQ_XB * 8];
    __attribute__((aligned(16))) float gi[DQ2_ROWS][DQ_GIS];
    __attribute__((aligned(16))) _Float16 hbh[DQ2_ROWS][DQ_HB * 8], hbl[DQ2_ROWS][DQ_HB * 8];
    __attribute__((aligned(16))) float hs[2][RM_DEC_H];
    int rst[DQ_PEND_MAX];
    int err[DQ_PEND_MAX];
};

// NT adjacent column tiles of a product for rows [0, Tb), Tb <= 12: ONE 16-row tile (the retired round-3 kernel carried two).
// sync_first: the barrier that separates this product from the phase before it is taken HERE, behind the first weight requests (which depend on nothing the phase before
// wrote): the round trip to L2 (~800 cycles, once per phase: five phases per layer and chunk) runs while the workgroup's other wavefronts arrive, instead of after them
template <int NT, bool SINGLE>
__device__ __forceinline__ void dq2_gemm_tiles_(DecShared2 *sh_, const DqGemm g_, int ct_, int Tb_, unsigned rstmask_, int sync_first)
{
    constexpr int D = NT == 1 ? 12 : ((NT == 3 && SINGLE) ? RX2_DQ_D3 : 4);   // k-steps of weights in flight (one plane of a three-tile product: 48 registers at 4, 96 at 8)
    const int ct = uni(ct_), Tb = uni(Tb_); const unsigned rstmask = (unsigned)uni((int)rstmask_);
    const int nct = uni(g_.nct), N = uni(g_.N), from_hb = uni(g_.from_hb), ktap = uni(g_.ktap), ks0 = uni(g_.ks0), nks = uni(g_.nks), init_gi = uni(g_.init_gi),
              outk = uni(g_.out), ocol = uni(g_.ocol), act = uni(g_.act), gstride = uni(g_.gstride);
    DecShared2 *sh = uni_ptr(sh_);
    glb_u16 *wbase = (glb_u16 *)uni_ptr(g_.wa); glb_cf32 *biasp = (glb_cf32 *)uni_ptr(g_.bias); glb_f32 *gout = (glb_f32 *)uni_ptr(g_.gout);
    glb_cf32 *wscale = (glb_cf32 *)uni_ptr(g_.wscale);
    constexpr bool single = SINGLE;
    const int lane = threadIdx.x & 63, t = lane & 15, gq = lane >> 4;
    const int r0 = min(t, Tb - 1);                                     // rows beyond Tb repeat the last one (results dropped)
    const lds_half *bh = (const lds_half *)(from_hb ? &sh->hbh[0][0] : &sh->xh[0][0]), *bl = (const lds_half *)(from_hb ? &sh->hbl[0][0] : &sh->xl[0][0]);
    const int stride = from_hb ? DQ_HB * 8 : DQ_XB * 8;
    const int p1a = (from_hb ? r0 : r0 + 1) * stride, k1a = r0 & 15;
    const int p0a = ((rstmask >> r0) & 1u) ? (DQ2_ROWS + 1) * stride : r0 * stride;
    const int k0a = (r0 - 1) & 15;
    const int planes = single ? 1 : 2;
    glb_u16 *wa = wbase + (((size_t)ks0 * nct + ct) * planes * 64 + lane) * 8;
    const size_t wstep = (size_t)nct * planes * 64 * 8, tstep = (size_t)planes * 64 * 8;
    lds_f32 *gi = (lds_f32 *)&sh->gi[0][0];
    f32x4 acc0[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) acc0[i] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
    const int n0 = 16 * ct + 4 * gq;
    typedef const __attribute__((address_space(1))) f16x8 glb_f16x8;
    typedef const __attribute__((address_space(3))) f16x8 lds_f16x8;
    f16x8 wh[D][NT], wl[D][NT];
    auto fetch = [&](int d, int ks) {
        const int kq = min(ks, nks - 1);
#pragma unroll
        for (int i = 0; i < NT; i++) {
            wh[d][i] = *(glb_f16x8 *)(wa + kq * wstep + i * tstep);
            if (!single) wl[d][i] = *(glb_f16x8 *)(wa + kq * wstep + i * tstep + 64 * 8);
        }
    };
#pragma unroll
    for (int d = 0; d < D; d++) fetch(d, d);
    if (sync_first) __syncthreads();
    f16x8 nha, nla;
    auto rows = [&](int kidx) {
        const int kk = ks0 + min(kidx, nks - 1);
        const bool tap0 = kk < ktap;
        const int cb = 4 * (tap0 ? kk : kk - ktap) + gq;
        const int oa = (tap0 ? p0a : p1a) + ((cb ^ (tap0 ? k0a : k1a)) << 3);
        nha = *(lds_f16x8 *)(bh + oa); nla = *(lds_f16x8 *)(bl + oa);
    };
    rows(0);
    auto step = [&](int d, int kidx, bool refill) {
        const f16x8 xha = nha, xla = nla;
        rows(kidx + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NT; i++) {
            if (!single) acc0[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[d][i], xha, acc0[i], 0, 0, 0);
            acc0[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[d][i], xla, acc0[i], 0, 0, 0);
            acc0[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[d][i], xha, acc0[i], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (refill) fetch(d, kidx + D);
        __builtin_amdgcn_sched_barrier(0);
    };
    int ks = 0;
#pragma unroll 1
    for (; ks + D <= nks; ks += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(d, ks + d, true);
    }
    // bias and row scales are requested here, under the last k-steps: held from the top of the function they cost up to 48 registers
    // across the K loop, and came back from scratch one s_waitcnt vmcnt(0) at a time in the epilogue
    f32x4 bias[NT], scl[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) {
        bias[i] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f }; scl[i] = (f32x4){ 0x1p-18f, 0x1p-18f, 0x1p-18f, 0x1p-18f };
        if (biasp && !init_gi) {        // (N is a multiple of 4 in every layer: one 16-byte load from a clamped address instead of four guarded dwords)
            const int nn = n0 + 16 * i;
            bias[i] = *(const __attribute__((address_space(1))) f32x4 *)(biasp + min(nn, N - 4));
            if (nn >= N) bias[i] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
        }
        if (single) scl[i] = *(const __attribute__((address_space(1))) f32x4 *)(wscale + n0 + 16 * i) * 0x1p-8f;
    }
#pragma unroll
    for (int d = 0; d < D; d++) if (ks + d < nks) step(d, ks + d, false);
    lds_half *xh = (lds_half *)&sh->xh[0][0], *xl = (lds_half *)&sh->xl[0][0];
    const lds_half *hbh = (const lds_half *)&sh->hbh[0][0], *hbl = (const lds_half *)&sh->hbl[0][0];
    typedef __attribute__((address_space(3))) f16x4 lds_f16x4;
    if (t < Tb) {
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const int n = n0 + 16 * i, tt = t;
            f32x4 v = acc0[i] * scl[i] + bias[i];
            if (init_gi) v += *(const __attribute__((address_space(3))) f32x4 *)(gi + tt * DQ_GIS + n);
            if (outk == DQ_OUT_GI) { *(__attribute__((address_space(3))) f32x4 *)(gi + tt * DQ_GIS + n) = v; continue; }
            if (outk == DQ_OUT_GLOBAL) {
#pragma unroll
                for (int r = 0; r < 4; r++) if (n + r < N) gout[(size_t)tt * gstride + n + r] = v[r];
                continue;
            }
            if (act == 2) {
                const f16x4 hh = *(const lds_f16x4 *)(hbh + dq_hoff(tt, n)), hl = *(const lds_f16x4 *)(hbl + dq_hoff(tt, n));
#pragma unroll
                for (int r = 0; r < 4; r++) v[r] = clamp1(((float)hh[r] + (float)hl[r]) * 0x1p-8f * gate_sigmoid(v[r]));
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) v[r] = clamp1(gate_tanh(v[r]));
            }
            f16x4 oh, ol;
#pragma unroll
            for (int r = 0; r < 4; r++) { _Float16 a, b; split16_act(v[r], a, b); oh[r] = a; ol[r] = b; }
            *(lds_f16x4 *)(xh + dq_xoff(tt, ocol + n)) = oh; *(lds_f16x4 *)(xl + dq_xoff(tt, ocol + n)) = ol;
        }
    }
}
template <int NT>
__device__ __forceinline__ void dq2_gemm_tiles(DecShared2 *sh, const DqGemm g, int ct, int Tb, unsigned rstmask, int sync_first)
{
    if (uni_ptr(g.wscale) != nullptr) dq2_gemm_tiles_<NT, true>(sh, g, ct, Tb, rstmask, sync_first);
    else dq2_gemm_tiles_<NT, false>(sh, g, ct, Tb, rstmask, sync_first);
}

// dense1 on the f32 matrix cores (v_mfma_f32_32x32x2_f32, exact f32 products): three wavefronts, 32 columns each
__device__ void dq2_dense1(DecShared2 *sh, const float *z, const rd_lin w, int Tb)
{
    constexpr int NKB = RD_LATENT / 8;
    const int lane = threadIdx.x & 63, nt = threadIdx.x >> 6, half = lane >> 5;
    if (nt >= 3) return;
    const float *wp = w.wp + ((size_t)nt * 64 + lane) * 4;
    const size_t wstep = (size_t)3 * 256;
    const int col = nt * 32 + (lane & 31);
    const float bias = w.bias[col];
    const int t = min(lane & 31, Tb - 1);
    const float *p1 = z + (size_t)t * RD_LATENT + 4 * half;
    f32x4 av[NKB], bv[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; kb++) { av[kb] = *(const f32x4 *)(p1 + kb * 8); bv[kb] = *(const f32x4 *)(wp + kb * wstep); }
    f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = 0.0f;
#pragma unroll
    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
        for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kb][s], bv[kb][s], acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int tt = (j & 3) + 8 * (j >> 2) + 4 * half;
        if (tt >= Tb) continue;
        _Float16 a, b; split16_act(clamp1(gate_tanh(acc[j] + bias)), a, b);
        sh->xh[0][dq_xoff(tt, col)] = a; sh->xl[0][dq_xoff(tt, col)] = b;
    }
}

// two plain FMAs (see the FIR in k_rx_sync2 for why this kernel avoids v_pk_fma_f32)
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return (f32x2){ fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1]) }; }
// GRU recurrence over Tb steps: TWO lanes per hidden unit (192 threads; the fourth wavefront only keeps the barriers)
__device__ void dq2_scan(DecShared2 *sh, const float *Whh, const float *bhh, float *hstate, int Tb, unsigned rstmask)
{
    constexpr int H = RM_DEC_H, KP = H / 2;
    const int tid = rx_tid();
    const bool on = tid < 2 * H;
    const int j = on ? tid >> 1 : 0, p = tid & 1;
    f32x2 wr[KP / 2], wz[KP / 2], wn[KP / 2];
    {
        const float *w0 = Whh + (size_t)j * H + p * KP;
#pragma unroll
        for (int k = 0; k < KP; k += 4) {
            const f32x4 v0 = *(const f32x4 *)(w0 + k), v1 = *(const f32x4 *)(w0 + (size_t)H * H + k), v2 = *(const f32x4 *)(w0 + (size_t)2 * H * H + k);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                wr[k / 2 + u] = (f32x2){ v0[2 * u], v0[2 * u + 1] }; wz[k / 2 + u] = (f32x2){ v1[2 * u], v1[2 * u + 1] }; wn[k / 2 + u] = (f32x2){ v2[2 * u], v2[2 * u + 1] };
            }
        }
    }
    const float br = bhh[j], bz = bhh[H + j], bn = bhh[2 * H + j];
    float hj = hstate[j];
    __syncthreads();                                   // (the barrier behind the input projection / fix-up that wrote gi: taken behind this function's global loads)
    if (on && p == 0) sh->hs[0][j] = hj;
    const float *gi = &sh->gi[0][0] + j;
    float g0r = gi[0], g0z = gi[H], g0n = gi[2 * H];
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < Tb; t++) {
        if ((rstmask >> t) & 1u) {                     // uniform over the workgroup
            hj = 0.0f;
            __syncthreads();
            if (on && p == 0) sh->hs[cur][j] = 0.0f;
            __syncthreads();
        }
        const float *gn_ = gi + (size_t)min(t + 1, Tb - 1) * DQ_GIS;
        const float g1r = gn_[0], g1z = gn_[H], g1n = gn_[2 * H];          // next step's inputs: their LDS latency hides under this step
        f32x2 ar = { 0.0f, 0.0f }, az = { 0.0f, 0.0f }, an = { 0.0f, 0.0f }, ar2 = { 0.0f, 0.0f }, az2 = { 0.0f, 0.0f }, an2 = { 0.0f, 0.0f };
        const float *hp = sh->hs[cur] + p * KP;
#pragma unroll
        for (int k = 0; k < KP; k += 8) {
            const f32x4 hv = *(const f32x4 *)(hp + k), hw = *(const f32x4 *)(hp + k + 4);
            const f32x2 h0 = { hv[0], hv[1] }, h1 = { hv[2], hv[3] }, h2 = { hw[0], hw[1] }, h3 = { hw[2], hw[3] };
            ar = fma2(wr[k / 2], h0, ar); az = fma2(wz[k / 2], h0, az); an = fma2(wn[k / 2], h0, an);
            ar2 = fma2(wr[k / 2 + 1], h1, ar2); az2 = fma2(wz[k / 2 + 1], h1, az2); an2 = fma2(wn[k / 2 + 1], h1, an2);
            ar = fma2(wr[k / 2 + 2], h2, ar); az = fma2(wz[k / 2 + 2], h2, az); an = fma2(wn[k / 2 + 2], h2, an);
            ar2 = fma2(wr[k / 2 + 3], h3, ar2); az2 = fma2(wz[k / 2 + 3], h3, az2); an2 = fma2(wn[k / 2 + 3], h3, an2);
        }
        ar += ar2; az += az2; an += an2;
        float sr = ar[0] + ar[1], sz = az[0] + az[1], sn = an[0] + an[1];
        sr += quad_dpp<QUAD_XOR1>(sr); sz += quad_dpp<QUAD_XOR1>(sz); sn += quad_dpp<QUAD_XOR1>(sn);
        const float r = gate_sigmoid((sr + br) + g0r);
        const float z = gate_sigmoid((sz + bz) + g0z);
        const float n = gate_tanh(g0n + (sn + bn) * r);
        hj = (hj - n) * z + n;
        if (on && p == 0) {
            sh->hs[cur ^ 1][j] = hj;
            _Float16 a, b; split16_act(clamp1(hj), a, b);
            sh->hbh[0][dq_hoff(t, j)] = a; sh->hbl[0][dq_hoff(t, j)] = b;
        }
        g0r = g1r; g0z = g1z; g0n = g1n;
        cur ^= 1;
        if (t + 1 < Tb) __syncthreads();               // (the last step's barrier is the consumer's: dq2_gemm_tiles(..., sync_first))
    }
    if (on && p == 0) hstate[j] = hj;
}

// The recurrence with W_hh h on the matrix cores.  Beside another stream's workgroup on the same CU the vector ALU is what the two compete
// for, and dq2_scan spends 432 vector FMAs per step and hidden unit row on a product the matrix pipe does in a few instructions: W_hh is
// int8 in the blob, its integers sit in registers as A-operand fragments of v_mfma_f32_16x16x32_f16 (exact in binary16, row scales
// applied afterwards); h_{t-1} is the B operand, read from LDS as two binary16 planes (2^8 h = hi + lo): EVEN columns of B carry the
// high plane, ODD columns the low plane, so one instruction per (gate tile, k-step) yields both partial products and a DPP add of
// neighbouring lanes (quad_perm [1,0,3,2]) joins them -- 9 instructions per block of 16 hidden units instead of 18.  A wavefront
// owns "unit blocks": the three tiles r / z / n of its units, so the gates are evaluated in registers by the lanes that hold them
// (lane column c < 4 finalises row c of its lane group).  Four wavefronts: blocks {0,1} {2,3} {4} {5}; the two-block wavefronts issue
// both blocks' matrix instructions first and then evaluate both blocks' gates in one straight-line region (two independent chains).
// (In the retired round-3 kernel, alone on its CU, the matrix form was no faster -- the step there is latency, not ALU -- and was not kept.)
template <int NB>
__device__ __forceinline__ void dq2_scan_mfma_body(DecShared2 *sh, const unsigned short *whq, const float *whs, const float *bhh, float *hstate, int Tb, unsigned rstmask, int ub0)
{
    constexpr int H = RM_DEC_H;
    const int tid = rx_tid(), lane = tid & 63, c = lane & 15, g = lane >> 4, cs = c & 3, par = c & 1;
    // every column of a tile's C holds the same sums once neighbouring lanes are added (the planes sit in even / odd columns), so in a two-block wavefront the lanes of
    // columns 8..15 take block 1 and those of columns 0..7 block 0: ONE pass over the gates (two sigmoids and a tanh: six transcendental instructions and their
    // latencies, the longest dependent chain of the step) serves both blocks instead of one pass per block
    const int blk = NB == 2 ? (c >> 3) & 1 : 0;
    typedef const __attribute__((address_space(1))) f16x8 glb_f16x8_t;
    f16x8 A[NB][3][3];
    float sc[3], bb[3];
    const bool finl = (c & 4) == 0 && (NB == 2 || c < 4);      // the lanes that publish: columns 0..3 (block 0) and, with two blocks, 8..11 (block 1)
    const int ju = 16 * (ub0 + blk) + 4 * g + cs;
#pragma unroll
    for (int k = 0; k < NB; k++)
#pragma unroll
        for (int gate = 0; gate < 3; gate++)
#pragma unroll
            for (int ks = 0; ks < 3; ks++) A[k][gate][ks] = *(glb_f16x8_t *)(whq + (((size_t)ks * 18 + gate * 6 + ub0 + k) * 64 + lane) * 8);
#pragma unroll
    for (int gate = 0; gate < 3; gate++) { sc[gate] = whs[gate * H + ju] * 0x1p-8f; bb[gate] = bhh[gate * H + ju]; }
    float hj = hstate[ju];
    __syncthreads();                                   // (the barrier behind the input projection / fix-up that wrote gi: taken behind the 9 / 18 weight fragments' round trip to L2)
    _Float16 (*hp)[2][H] = (_Float16 (*)[2][H])&sh->hs[0][0];           // [buffer][plane][k]: 2^8 h_{t-1} = hi + lo
    if (finl) { _Float16 a, b; split16_act(hj, a, b); hp[0][0][ju] = a; hp[0][1][ju] = b; }
    const float *gi = &sh->gi[0][0];
    float g0[3];
#pragma unroll
    for (int gate = 0; gate < 3; gate++) g0[gate] = gi[gate * H + ju];
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < Tb; t++) {
        if ((rstmask >> t) & 1u) {                     // uniform over the workgroup
            __syncthreads();
            hj = 0.0f; if (finl) { hp[cur][0][ju] = (_Float16)0.0f; hp[cur][1][ju] = (_Float16)0.0f; }
            __syncthreads();
        }
        const float *gn_ = gi + (size_t)min(t + 1, Tb - 1) * DQ_GIS;
        float g1[3];
#pragma unroll
        for (int gate = 0; gate < 3; gate++) g1[gate] = gn_[gate * H + ju];
        f16x8 bq[3];
#pragma unroll
        for (int ks = 0; ks < 3; ks++) bq[ks] = *(const f16x8 *)&hp[cur][par][32 * ks + 8 * g];
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[NB][3];
#pragma unroll
        for (int k = 0; k < NB; k++)
#pragma unroll
            for (int gate = 0; gate < 3; gate++) acc[k][gate] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int ks = 0; ks < 3; ks++)
#pragma unroll
            for (int k = 0; k < NB; k++)
#pragma unroll
                for (int gate = 0; gate < 3; gate++) acc[k][gate] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[k][gate][ks], bq[ks], acc[k][gate], 0, 0, 0);
        // C layout: this lane holds rows 4 g + 0..3 of each tile for column c: high-plane product in even columns, low-plane product in odd ones
        float s3[3];
#pragma unroll
        for (int gate = 0; gate < 3; gate++) {
            float sr[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float v = NB == 2 ? (blk ? acc[NB - 1][gate][r] : acc[0][gate][r]) : acc[0][gate][r];      // this lane's block
                sr[r] = v + quad_dpp<QUAD_XOR1>(v); asm volatile("" : "+v"(sr[r]));                               // (computed before the select: no branches)
            }
            const float s01 = (cs & 1) ? sr[1] : sr[0], s23 = (cs & 1) ? sr[3] : sr[2];
            s3[gate] = (cs & 2) ? s23 : s01;
        }
        {
            const float r = gate_sigmoid((s3[0] * sc[0] + bb[0]) + g0[0]);
            const float z = gate_sigmoid((s3[1] * sc[1] + bb[1]) + g0[1]);
            const float n = gate_tanh(g0[2] + (s3[2] * sc[2] + bb[2]) * r);
            hj = (hj - n) * z + n;
        }
        if (finl) {
            _Float16 a, b; split16_act(hj, a, b);
            hp[cur ^ 1][0][ju] = a; hp[cur ^ 1][1][ju] = b;
            split16_act(clamp1(hj), a, b);
            sh->hbh[0][dq_hoff(t, ju)] = a; sh->hbl[0][dq_hoff(t, ju)] = b;
        }
#pragma unroll
        for (int gate = 0; gate < 3; gate++) g0[gate] = g1[gate];
        cur ^= 1;
        if (t + 1 < Tb) __syncthreads();               // (the last step's barrier is the consumer's: dq2_gemm_tiles(..., sync_first))
    }
    if (finl) hstate[ju] = hj;
}
__device__ void dq2_scan_mfma(DecShared2 *sh, const unsigned short *whq, const float *whs, const float *bhh, float *hstate, int Tb, unsigned rstmask)
{
    const int wave = rx2_wave();
    if (wave < 2) dq2_scan_mfma_body<2>(sh, whq, whs, bhh, hstate, Tb, rstmask, 2 * wave);
    else dq2_scan_mfma_body<1>(sh, whq, whs, bhh, hstate, Tb, rstmask, 2 + wave);
}

// all decoder layers for rows [0, Tb) (Tb <= 12) of stream b on four wavefronts
__device__ void dq2_layers(DecShared2 *sh, const rd_decs_args &a, int b, const float *z, float *out, int Tb, unsigned rstmask, int census_noscan)
{
    const int tid = rx_tid(), wave = tid >> 6;
    PH2_T0();
    {
        const unsigned *hist = (const unsigned *)(a.x + (size_t)b * a.x_sb - RD_DEC_W);
        constexpr int NH_ = (RD_DEC_W + NT2 - 1) / NT2;
        unsigned hu[NH_];                                       // (all requested before the first LDS store: see rx2_load_rxbuf)
#pragma unroll
        for (int q = 0; q < NH_; q++) hu[q] = hist[min(tid + q * NT2, RD_DEC_W - 1)];
#pragma unroll
        for (int q = 0; q < NH_; q++) {
            const int c = tid + q * NT2; const unsigned u = hu[q];
            if (c < RD_DEC_W) { sh->xh[0][dq_xoff(-1, c)] = __builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu)); sh->xl[0][dq_xoff(-1, c)] = __builtin_bit_cast(_Float16, (unsigned short)(u >> 16)); }
        }
        for (int c = tid; c < DQ_XB * 8; c += NT2) { sh->xh[DQ2_ROWS + 1][c] = (_Float16)0.0f; sh->xl[DQ2_ROWS + 1][c] = (_Float16)0.0f; }
    }
    dq2_dense1(sh, z, a.dense1, Tb);
    DqGemm g;
    // Barriers: every product phase takes the barrier that separates it from the phase before it INSIDE its first dq2_gemm_tiles call (sync_first), behind that call's
    // first weight requests; the recurrences do the same behind their weight fragments.  A wavefront that has no product in a phase takes the barrier bare.
    // 18 column tiles of an input projection over four wavefronts: 5 + 5 + 4 + 4
    const int ct18 = wave < 2 ? 5 * wave : 10 + 4 * (wave - 2);
    g = (DqGemm){ a.gin[0].wa16, 18, a.gin[0].bias, RM_DEC_G, a.gin[0].wscale, 0, 0, 0, 3, 0, DQ_OUT_GI, 0, 0, nullptr, 0 };
    if (wave < 2) dq2_gemm_tiles<5>(sh, g, ct18, Tb, rstmask, 1); else dq2_gemm_tiles<4>(sh, g, ct18, Tb, rstmask, 1);
    PH2(20);
#pragma unroll 1
    for (int l = 0; l < RM_NL; l++) {
        const int in = RM_DEC_GRU_IN(l), cin = RM_DEC_CONV_IN(l);
        if (census_noscan) __syncthreads();
        else if (a.whq[l]) dq2_scan_mfma(sh, a.whq[l], a.whs[l], a.bhh[l], a.h[l] + (size_t)b * RM_DEC_H, Tb, rstmask);
        else dq2_scan(sh, a.whh[l], a.bhh[l], a.h[l] + (size_t)b * RM_DEC_H, Tb, rstmask);
        PH2(21);
        // GLU gates: 6 column tiles, K = 96: 2 + 2 + 1 + 1
        g = (DqGemm){ a.glu[l].wa16, 6, nullptr, RM_DEC_GLU, a.glu[l].wscale, 1, 0, 0, 3, 0, DQ_OUT_X, in, 2, nullptr, 0 };
        if (wave < 2) dq2_gemm_tiles<2>(sh, g, 2 * wave, Tb, rstmask, 1); else dq2_gemm_tiles<1>(sh, g, 2 + wave, Tb, rstmask, 1);
        PH2(22);
        // conv (2 tiles, K = 2 cin) beside the columns of the next product that are already final (K = cin): in units of cin k-steps the
        // conv tiles weigh 2 each, a projection tile 1: wavefronts 0 / 1 = one conv tile + 3 projection tiles, 2 / 3 = 6 projection tiles;
        // behind the last conv the output layer (6 tiles): one conv tile each on 0 / 1, three output tiles each on 2 / 3
        const DqGemm gc = (DqGemm){ a.conv[l].wa16, 2, a.conv[l].bias, RM_DEC_CONV, a.conv[l].wscale, 0, cin / 32, 0, 2 * cin / 32, 0, DQ_OUT_X, cin, 1, nullptr, 0 };
        const bool last = l == RM_NL - 1;
        const rd_lin &nx = last ? a.output : a.gin[l + 1];
        const int nct = last ? 6 : 18;
        const DqGemm gm = (DqGemm){ nx.wa16, nct, nx.bias, last ? a.out_w : RM_DEC_G, nx.wscale, 0, 0, 0, cin / 32, 0, DQ_OUT_GI, 0, 0, nullptr, 0 };
        if (wave < 2) {
            dq2_gemm_tiles<1>(sh, gc, wave, Tb, rstmask, 1);
            if (!last) dq2_gemm_tiles<3>(sh, gm, 3 * wave, Tb, rstmask, 0);
        } else if (last) dq2_gemm_tiles<3>(sh, gm, 3 * (wave - 2), Tb, rstmask, 1);
        else {          // six projection tiles as two calls of three: with six tiles' fragments (4 k-steps x 6 x 4 registers) in flight the K loop spilled -- 20 scratch instructions per k-step
            dq2_gemm_tiles<3>(sh, gm, 6 + 6 * (wave - 2), Tb, rstmask, 1);
            dq2_gemm_tiles<3>(sh, gm, 9 + 6 * (wave - 2), Tb, rstmask, 0);
        }
        PH2(23);
        // fix-up: the conv's 32 new columns (one k-step) added onto the staged sums
        const DqGemm gf = (DqGemm){ nx.wa16, nct, nullptr, last ? a.out_w : RM_DEC_G, nx.wscale, 0, 0, cin / 32, 1, 1, last ? DQ_OUT_GLOBAL : DQ_OUT_GI, 0, 0, out, a.out_w };
        if (last) { if (wave >= 2) dq2_gemm_tiles<3>(sh, gf, 3 * (wave - 2), Tb, rstmask, 1); else __syncthreads(); }
        else if (wave < 2) dq2_gemm_tiles<5>(sh, gf, ct18, Tb, rstmask, 1);
        else dq2_gemm_tiles<4>(sh, gf, ct18, Tb, rstmask, 1);
        PH2(24);
    }
    __syncthreads();                                   // (behind the last fix-up: the history row below reads what the last conv wrote)
    {
        unsigned *hist = (unsigned *)(a.x + (size_t)b * a.x_sb - RD_DEC_W);
        for (int c = tid; c < RD_DEC_W; c += NT2)
            hist[c] = (unsigned)__builtin_bit_cast(unsigned short, sh->xh[0][dq_xoff(Tb - 1, c)]) | ((unsigned)__builtin_bit_cast(unsigned short, sh->xl[0][dq_xoff(Tb - 1, c)]) << 16);
    }
    __syncthreads();
}
