// The FFT-convolution pilot correlator of rounds 2-3 (one forward 2048-point transform of the window, 40 spectral products with
// precomputed pilot spectra, 40 inverse transforms).  Replaced by the matrix-core GEMM form (rx2_detect_mfma) in round 3 and removed
// from the build in round 4; kept here as a record of the measured alternative (DESIGN.md 3.9).  Not compiled.
#define FFT_N 2048
#define FFT_SCR (32 * 66)
__device__ static constexpr float C32[16] = { 1.000000000e+00f, 9.807852804e-01f, 9.238795325e-01f, 8.314696123e-01f, 7.071067812e-01f, 5.555702330e-01f, 3.826834324e-01f, 1.950903220e-01f, 6.123233996e-17f, -1.950903220e-01f, -3.826834324e-01f, -5.555702330e-01f, -7.071067812e-01f, -8.314696123e-01f, -9.238795325e-01f, -9.807852804e-01f };
__device__ static constexpr float S32[16] = { 0.000000000e+00f, 1.950903220e-01f, 3.826834324e-01f, 5.555702330e-01f, 7.071067812e-01f, 8.314696123e-01f, 9.238795325e-01f, 9.807852804e-01f, 1.000000000e+00f, 9.807852804e-01f, 9.238795325e-01f, 8.314696123e-01f, 7.071067812e-01f, 5.555702330e-01f, 3.826834324e-01f, 1.950903220e-01f };
__device__ static constexpr float C64[32] = { 1.000000000e+00f, 9.951847267e-01f, 9.807852804e-01f, 9.569403357e-01f, 9.238795325e-01f, 8.819212643e-01f, 8.314696123e-01f, 7.730104534e-01f, 7.071067812e-01f, 6.343932842e-01f, 5.555702330e-01f, 4.713967368e-01f, 3.826834324e-01f, 2.902846773e-01f, 1.950903220e-01f, 9.801714033e-02f, 6.123233996e-17f, -9.801714033e-02f, -1.950903220e-01f, -2.902846773e-01f, -3.826834324e-01f, -4.713967368e-01f, -5.555702330e-01f, -6.343932842e-01f, -7.071067812e-01f, -7.730104534e-01f, -8.314696123e-01f, -8.819212643e-01f, -9.238795325e-01f, -9.569403357e-01f, -9.807852804e-01f, -9.951847267e-01f };
__device__ static constexpr float S64[32] = { 0.000000000e+00f, 9.801714033e-02f, 1.950903220e-01f, 2.902846773e-01f, 3.826834324e-01f, 4.713967368e-01f, 5.555702330e-01f, 6.343932842e-01f, 7.071067812e-01f, 7.730104534e-01f, 8.314696123e-01f, 8.819212643e-01f, 9.238795325e-01f, 9.569403357e-01f, 9.807852804e-01f, 9.951847267e-01f, 1.000000000e+00f, 9.951847267e-01f, 9.807852804e-01f, 9.569403357e-01f, 9.238795325e-01f, 8.819212643e-01f, 8.314696123e-01f, 7.730104534e-01f, 7.071067812e-01f, 6.343932842e-01f, 5.555702330e-01f, 4.713967368e-01f, 3.826834324e-01f, 2.902846773e-01f, 1.950903220e-01f, 9.801714033e-02f };
__host__ __device__ constexpr int brev5(int x) { return ((x & 1) << 4) | ((x & 2) << 2) | (x & 4) | ((x & 8) >> 2) | ((x & 16) >> 4); }
__device__ __forceinline__ float lane_swap1(float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, true)); }   // quad_perm [1,0,3,2]

__device__ __forceinline__ void dft32_inlane(float2 (&v)[32])
{   // forward DFT, decimation in frequency: output X[q] is left in v[brev5(q)]
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const int half = 16 >> s;
#pragma unroll
        for (int g = 0; g < (1 << s); g++) {
#pragma unroll
            for (int k = 0; k < half; k++) {
                const int i = g * 2 * half + k, j = i + half, e = k << s;
                const float2 x = v[i], y = v[j];
                v[i] = make_float2(x.x + y.x, x.y + y.y);
                const float dr = x.x - y.x, di = x.y - y.y;
                if (e == 0) v[j] = make_float2(dr, di);
                else if (e == 8) v[j] = make_float2(di, -dr);                       // times -j
                else if (e == 4) v[j] = make_float2((dr + di) * C32[4], (di - dr) * C32[4]);
                else if (e == 12) v[j] = make_float2((di - dr) * C32[4], -(dr + di) * C32[4]);
                else v[j] = make_float2(dr * C32[e] + di * S32[e], di * C32[e] - dr * S32[e]);   // times e^{-j2pi e/32}
            }
        }
    }
}

// v[k2] = x[lane + 64 k2] in, X[q + 32(2p + h)] (q = lane>>1, h = lane&1) in v[brev5(p)] out
typedef __attribute__((address_space(3))) float lds_float;
#ifdef RD_FFT_PAD65
#define FFT_WR(q, lane) ((q) * 65 + (lane))
#define FFT_RD(q2, h, l) ((q2) * 65 + 32 * (h) + (l))
#else
#define FFT_WR(q, lane) ((q) * 66 + (lane) + ((lane) >> 5))
#define FFT_RD(q2, h, l) ((q2) * 66 + 33 * (h) + (l))
#endif
typedef __attribute__((address_space(1))) float glb_float;
__device__ __forceinline__ void fft2048_wave(float2 (&v)[32], lds_float *scr, const glb_float *__restrict__ tw, int lane)
{
    // the inter-pass twiddles e^{-j2pi lane q/2048} are fetched before the first in-lane DFT, which hides their L2 round trip
    float2 w1[32];
#pragma unroll
    for (int q = 1; q < 32; q++) w1[q] = make_float2(tw[2 * (q * 64 + lane)], tw[2 * (q * 64 + lane) + 1]);
    __builtin_amdgcn_sched_barrier(0);
    dft32_inlane(v);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 1; q < 32; q++) v[brev5(q)] = cmul(v[brev5(q)], w1[q]);
    const int q2 = lane >> 1, h = lane & 1;
    float ur[32], ui[32];
#pragma unroll
    for (int q = 0; q < 32; q++) scr[FFT_WR(q, lane)] = v[brev5(q)].x;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int l = 0; l < 32; l++) ur[l] = scr[FFT_RD(q2, h, l)];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < 32; q++) scr[FFT_WR(q, lane)] = v[brev5(q)].y;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int l = 0; l < 32; l++) ui[l] = scr[FFT_RD(q2, h, l)];
    __builtin_amdgcn_wave_barrier();
    // radix-2 DIF stage over l <-> l + 32 (the partner lane): even outputs on h = 0, odd outputs (twiddled) on h = 1
    const float sg = h ? -1.0f : 1.0f;
    // h = 0: u + o;  h = 1: (o - u) e^{-j2pi l/64}, the twiddle as a literal (no table fetch inside the transform)
#pragma unroll
    for (int l = 0; l < 32; l++) {
        const float sr = fmaf(ur[l], sg, lane_swap1(ur[l])), si = fmaf(ui[l], sg, lane_swap1(ui[l]));
        if (l == 0) v[l] = make_float2(sr, si);
        else {
            const float2 t = cmul(make_float2(sr, si), make_float2(C64[l], -S64[l]));
            v[l] = h ? t : make_float2(sr, si);
        }
    }
    dft32_inlane(v);
}

// |Dt| surfaces by FFT convolution (see the FFT correlator notes above); runs with its own register allocation.
// pass 0: Dt1 (rx_buf[t + m]) -> buffer oldb, pass 1: Dt2 (rx_buf[Nmf + t + m]) -> buffer newb; cached skips pass 0.
// ---- |Dt| surfaces by FFT convolution (rx_detect_fft on four wavefronts: ten frequencies each; kept for A/B: tools/ab_build.sh fft -DRX2_SEARCH_FFT)
__device__ __forceinline__ void rx2_detect_fft(RxShared2 *sh, const float *G_, const float *tw_, float *cache_, int cached, int oldb, int newb,
                                               float &best, int &bt, int &bfi)
{
    const glb_float *G = (const glb_float *)G_, *tw = (const glb_float *)tw_; glb_float *cache = (glb_float *)cache_;
    const int tid = rx_tid(), wave = tid >> 6, lane = tid & 63, q2 = lane >> 1, h = lane & 1;
    lds_float *scr = (lds_float *)&sh->fftscr[wave][0];
    lds_float *rxf = (lds_float *)&sh->rxb[0], *Xf = (lds_float *)&sh->fftX[0];
    constexpr int NFW = RD_NFC / NW2;                                         // frequencies per wave
#pragma unroll 1
    for (int pass = cached ? 1 : 0; pass < 2; pass++) {
        lds_float *x = rxf + 2 * pass * RD_NMF;
        glb_float *dst = cache + (size_t)(pass ? newb : oldb) * RD_NFC * RD_NMF;
        const glb_float *prev = cache + (size_t)oldb * RD_NFC * RD_NMF;
        float2 v[32];
        float rs[15], mx[15]; unsigned long long argw = 0ull;
#pragma unroll
        for (int p = 0; p < 15; p++) { rs[p] = 0.0f; mx[p] = -1.0f; }
        // fi = -1: forward transform of the window (every wave repeats it and writes the whole spectrum: identical values, so a wave
        // only ever reads what its own lanes -- or another wave, equally -- stored: a wave barrier suffices); fi >= 0: inverse transforms
#pragma unroll 1
        for (int fi = -1; fi < NFW; fi++) {
            const int f = wave * NFW + fi;
            if (fi < 0) {
#pragma unroll
                for (int k2 = 0; k2 < 32; k2++) {
                    const int n = lane + 64 * k2;
                    v[k2] = (k2 < 18 && n < RD_NMF + RD_M - 1) ? make_float2(x[2 * n], x[2 * n + 1]) : make_float2(0.0f, 0.0f);
                }
            } else {
                const glb_float *Gf = G + (size_t)f * FFT_N * 2;
                float2 g[32];
#pragma unroll
                for (int u = 0; u < 32; u++) { const int k = lane + 64 * u; g[u] = make_float2(Gf[2 * k], Gf[2 * k + 1]); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 32; u++) { const int k = lane + 64 * u; const float2 y = cmul(make_float2(Xf[2 * k], Xf[2 * k + 1]), g[u]); v[u] = make_float2(y.y, y.x); }
                __builtin_amdgcn_sched_barrier(0);
            }
            const int t0 = q2 + 32 * h;
            float d1[15];
#pragma unroll
            for (int p = 0; p < 15; p++) d1[p] = (pass && fi >= 0) ? prev[(size_t)f * RD_NMF + t0 + 64 * p] : 0.0f;
            __builtin_amdgcn_sched_barrier(0);
            fft2048_wave(v, scr, tw, lane);
            if (fi < 0) {
#pragma unroll
                for (int p = 0; p < 32; p++) { const int k = q2 + 64 * p + 32 * h; Xf[2 * k] = v[brev5(p)].x; Xf[2 * k + 1] = v[brev5(p)].y; }
                __builtin_amdgcn_wave_barrier();
            } else {
#pragma unroll
                for (int p = 0; p < 15; p++) {
                    const float2 c = v[brev5(p)];
                    const float d = __builtin_amdgcn_sqrtf(fmaf(c.x, c.x, c.y * c.y));
                    dst[(size_t)f * RD_NMF + t0 + 64 * p] = d;
                    rs[p] += d;
                    if (pass) { const float s12 = d1[p] + d; if (s12 > mx[p]) { mx[p] = s12; argw = (argw & ~(15ull << (4 * p))) | ((unsigned long long)fi << (4 * p)); } }
                }
            }
        }
        {
            const int t0 = q2 + 32 * h;
#pragma unroll
            for (int p = 0; p < 15; p++) { scr[t0 + 64 * p] = rs[p]; scr[RD_NMF + t0 + 64 * p] = mx[p]; }
            scr[2 * RD_NMF + 2 * lane] = __uint_as_float((unsigned)argw); scr[2 * RD_NMF + 2 * lane + 1] = __uint_as_float((unsigned)(argw >> 32));
        }
        __syncthreads();
        for (int t = tid; t < RD_NMF; t += NT2) {
            const int ln = 2 * (t & 31) + ((t >> 5) & 1), sh4 = 4 * (t >> 6);
            float sum = 0.0f, lmax = -1.0f; int larg = 0;
#pragma unroll
            for (int w = 0; w < NW2; w++) {
                lds_float *sw = (lds_float *)&sh->fftscr[w][0];
                sum += sw[t];
                const float m = sw[RD_NMF + t];
                if (m > lmax) {
                    const unsigned lo = __float_as_uint(sw[2 * RD_NMF + 2 * ln]), hi = __float_as_uint(sw[2 * RD_NMF + 2 * ln + 1]);
                    const unsigned long long aw = ((unsigned long long)hi << 32) | lo;
                    lmax = m; larg = w * NFW + (int)((aw >> sh4) & 15);
                }
            }
            if (pass) { sh->rowsum2[t] = sum; if (lmax > best) { best = lmax; bt = t; bfi = larg; } }
            else sh->rowsum1[t] = sum;
        }
        __syncthreads();
    }
}


#if 0   /* host side (was rade_host.c): the pilot spectra G[f][k] and the transform twiddles */
/* Tables of the FFT pilot correlator (the retired round-3 kernel, search state).  Dt[t,f] = sum_m conj(rx[t+m]) p_w[m,f]
 * (dsp.py:207-208) is a correlation along t, so |Dt[.,f]| = |IDFT_2048(DFT_2048(rx) . G_f)| with
 * G_f[k] = (1/2048) sum_m conj(p_w[m,f]) e^{+j 2 pi k m/2048}, evaluated here in double from the float32 p_w the
 * reference correlates with.  tw[q][l] = e^{-j 2 pi l q/2048} is the twiddle between the two radix passes. */
#define RD_FFT_TW_FLOATS ((2048 + 64) * 2)
void rd_fft_tables_fill(const rd_tables *T, float *G /* [RD_NFC][2048][2] */, float *tw /* [32][64][2] + [2][32][2] */)
{
    const double w0 = 2.0 * PI_D / 2048.0;
    double cs[2048], sn[2048];
    for (int k = 0; k < 2048; k++) { cs[k] = cos(w0 * k); sn[k] = sin(w0 * k); }
    for (int f = 0; f < RD_NFC; f++)
        for (int k = 0; k < 2048; k++) {
            double ar = 0.0, ai = 0.0;
            for (int m = 0; m < RD_M; m++) {
                const int ph = (k * m) & 2047;
                const double gr = T->p_w[m][f][0], gi = -(double)T->p_w[m][f][1];     /* conj(p_w) */
                ar += gr * cs[ph] - gi * sn[ph]; ai += gr * sn[ph] + gi * cs[ph];
            }
            G[((size_t)f * 2048 + k) * 2] = (float)(ar / 2048.0); G[((size_t)f * 2048 + k) * 2 + 1] = (float)(ai / 2048.0);
        }
    for (int q = 0; q < 32; q++)
        for (int l = 0; l < 64; l++) { tw[(q * 64 + l) * 2] = (float)cs[(l * q) & 2047]; tw[(q * 64 + l) * 2 + 1] = (float)-sn[(l * q) & 2047]; }
    for (int l = 0; l < 32; l++) {          /* cross-lane radix-2 stage: lane h = 0 multiplies by 1, h = 1 by e^{-j 2 pi l/64} */
        tw[(2048 + l) * 2] = 1.0f; tw[(2048 + l) * 2 + 1] = 0.0f;
        tw[(2048 + 32 + l) * 2] = (float)cs[32 * l]; tw[(2048 + 32 + l) * 2 + 1] = (float)-sn[32 * l];
    }
}
#endif
