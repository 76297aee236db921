// rade_irx.h -- what the ideal-timing receiver (rade_irx.hip: k_irx_demod) and the stored-file receiver (rade_file.hip: k_file_demod) share: the symbols a
// workgroup demodulates and the pilot estimate of do_pilot_eq.  Needs rade_devutil.h.
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
#endif
