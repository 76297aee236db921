// rade_irx.h -- the fixed-timing receiver's frame, stated once for its two entries (rade_irx.hip: k_irx_demod, the ideal-timing call, and k_file_demod, the stored-file
// call): the symbols a workgroup demodulates, the pilot estimate of do_pilot_eq (also the SNR estimator's, rade_snr.hip) and the frame body.  Needs rade_devutil.h.
#ifndef RADE_IRX_H
#define RADE_IRX_H
#define IRX_NSYM (RD_NS + 2)   // the frame's pilot and four data symbols, then the pilot of the next frame (the last frame: of the previous one)

// the pilot estimate of carrier c from one received pilot row (do_pilot_eq, radae.py:316-346)
__device__ __forceinline__ float2 irx_pilot(const rd_tables *tab, const float2 *row, int c, int eq)
{
    if (eq == RD_IRX_ALL) {                                          // per_carrier_eq = False: the mean over every carrier
        float2 s = make_float2(0.0f, 0.0f);
        for (int k = 0; k < RD_NC; k++) { const float pp = tab->P[k]; s = cadd(s, make_float2(row[k].x / pp, row[k].y / pp)); }
        return make_float2(s.x / (float)RD_NC, s.y / (float)RD_NC);
    }
    const int cm = c == 0 ? 1 : (c == RD_NC - 1 ? RD_NC - 2 : c);   // edges: carriers 0:3 and Nc-3:Nc
    float2 h[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { const float pp = tab->P[cm - 1 + k]; h[k] = make_float2(row[cm - 1 + k].x / pp, row[cm - 1 + k].y / pp); }
    if (eq == RD_IRX_MEAN6) { const float2 s = cadd(cadd(h[0], h[1]), h[2]); return make_float2(s.x / 3.0f, s.y / 3.0f); }
    // 3-pilot least squares, a = 0.0025 Fs: g = Pmat h, estimate g0 + g1 e^{-j w[c] a} (the streaming receiver's est_pilots, dsp.py:400-433)
    float2 g0 = make_float2(0.0f, 0.0f), g1 = g0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        g0 = cadd(g0, cmul(make_float2(tab->Pmat[c][0][k][0], tab->Pmat[c][0][k][1]), h[k]));
        g1 = cadd(g1, cmul(make_float2(tab->Pmat[c][1][k][0], tab->Pmat[c][1][k][1]), h[k]));
    }
    return cadd(g0, cmul(g1, ld2(tab->eq_rot, c)));
}

// One modem frame of one stream, by a workgroup of 192: cyclic prefix removal at a known timing, the 160 -> 30 DFT, the pilot EQ, the demapper.  rx is the stream's first
// sample, mf the frame, `last` whether it is the stream's last; zf receives the frame's [3][80] latents and *part its sum_c |pilot estimate|^2 (0 without EQ).
// mix(v, n) is the entry's mixer for sample n of the stream, a type so that the sample loop holds no run-time choice between the two.  They are different arithmetic on
// purpose (rade_irx.hip states each once, at its entry):
//   the ideal-timing call   rx * conj(lin_phase) as RADAE.forward forms it (radae.py:594-595): the float32 phase of chan_phase_acc, float sincosf, a float32 product
//   the stored-file call    rx * exp(-1j w n) as rx.py:223-228 forms it: phase, sincos and product in double, rounded once to complex64
template <class Mix>
__device__ __forceinline__ void irx_frame(const rd_tables *tab, const float2 *rx, int mf, bool last, int time_offset, int eq, Mix mix, float *zf, double *part)
{
    __shared__ float2 x[IRX_NSYM][RD_M];
    __shared__ float2 sym[IRX_NSYM][RD_NC];
    __shared__ float2 rp[2][RD_NC];                                  // pilot estimates: this frame's, the other frame's
    const int tid = threadIdx.x;
    // the DFT window [Ncp + time_offset, Ncp + time_offset + M) of every symbol; time_offset in [-Ncp, 0] keeps it inside the symbol, so the
    // last sample read is n_mf * 960 - 1
    for (int i = tid; i < IRX_NSYM * RD_M; i += 192) {
        const int s = i / RD_M, k = i - s * RD_M;
        const int fr = s < RD_NS + 1 ? mf : (last ? mf - 1 : mf + 1);
        const int n = fr * RD_NMF + (s < RD_NS + 1 ? s : 0) * RD_SYM + RD_NCP + time_offset + k;
        x[s][k] = mix(rx[n], n);
    }
    __syncthreads();
    if (tid < IRX_NSYM * RD_NC) {                                    // rx_sym = rx_dash Wfwd
        const int s = tid / RD_NC, c = tid - s * RD_NC;
        float re = 0.0f, im = 0.0f;
        for (int k = 0; k < RD_M; k++) {
            const float2 v = x[s][k], w = ld2(tab->Wfwd[k], c);
            re = fmaf(v.x, w.x, re); re = fmaf(-v.y, w.y, re);
            im = fmaf(v.x, w.y, im); im = fmaf(v.y, w.x, im);
        }
        sym[s][c] = make_float2(re, im);
    }
    __syncthreads();
    if (eq != RD_IRX_NONE && tid < 2 * RD_NC) {
        const int i = tid / RD_NC, c = tid - i * RD_NC;
        rp[i][c] = irx_pilot(tab, sym[i ? RD_NS + 1 : 0], c, eq);
    }
    __syncthreads();
    if (tid == 0) {                                                  // coarse_mag: this frame's share of mean |rx_pilots|^2
        double p = 0.0;
        if (eq != RD_IRX_NONE) for (int c = 0; c < RD_NC; c++) p += (double)rp[0][c].x * rp[0][c].x + (double)rp[0][c].y * rp[0][c].y;
        *part = p;
    }
    if (tid < RD_NS * RD_NC) {
        const int s = tid / RD_NC, c = tid - s * RD_NC;
        float2 v = sym[1 + s][c];
        if (eq != RD_IRX_NONE) {
            // phase-only linear interpolation between this frame's pilot and the next one's, at s + 1 of Ns + 1 (radae.py:350-356); the last frame keeps
            // the slope the loop left behind: carrier Nc - 1's, from frame n_mf - 2, for every carrier (radae.py:358-365)
            const float2 d = last ? make_float2(rp[0][RD_NC - 1].x - rp[1][RD_NC - 1].x, rp[0][RD_NC - 1].y - rp[1][RD_NC - 1].y)
                                  : make_float2(rp[1][c].x - rp[0][c].x, rp[1][c].y - rp[0][c].y);
            const float2 slope = make_float2(d.x / (float)(RD_NS + 1), d.y / (float)(RD_NS + 1));
            const float2 ch = make_float2(slope.x * (float)(s + 1) + rp[0][c].x, slope.y * (float)(s + 1) + rp[0][c].y);
            float sn, cs; sincosf(atan2f(ch.y, ch.x), &sn, &cs);
            v = cmul(v, make_float2(cs, -sn));
        }
        zf[2 * tid] = v.x; zf[2 * tid + 1] = v.y;                    // the inverse of k_ofdm_mod's map
    }
}
#endif
