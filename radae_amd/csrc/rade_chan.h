// rade_chan.h -- the channel simulator and its launch shims; part of rade_kernels.hip (see its inventory).
// Replaces: the rate-Fs channel of RADAE.forward and inference.py (radae.py:529-589, inference.py:263-288), the Watterson model (doppler_spread.m,
// multipath_samples.m), the symbol-domain channels (radae.py:604-634, bbfm.py:157-197).
// Needs rd_chan_args, RD_NEOO, RD_NMF (rade_dev.h); cmul, cadd, chan_phase_acc, philox4x32, gauss_pair (rade_devutil.h).  The LDS reduction trees of
// k_chan_power and k_multipath_gen stay trees: their order of additions is what the goldens pin.
#define CH_NCH 64   // partial-sum chunks per stream (fixed => deterministic reduction order)

__device__ __forceinline__ float2 chan_mp(const float2 *tx, const float2 *G, int i)
{
    if (!G) return tx[i];
    float2 v = cmul(tx[i], G[2 * i]);
    if (i >= 16) v = cadd(v, cmul(tx[i - 16], G[2 * (i - 16) + 1]));
    return v;
}

__global__ __launch_bounds__(256) void k_chan_power(rd_chan_args a, double *part)
{
    __shared__ double red[2][256];
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const float2 *tx = (const float2 *)a.tx + (size_t)b * a.tx_stride;
    const float2 *G = a.G ? (const float2 *)a.G + (size_t)b * a.n_sig * 2 : nullptr;
    const int per = (a.n_sig + CH_NCH - 1) / CH_NCH;
    const int lo = ch * per, hi = min(a.n_sig, lo + per);
    double s0 = 0.0, s1 = 0.0;
    for (int i = lo + tid; i < hi; i += 256) {
        const float2 x = tx[i], m = chan_mp(tx, G, i);
        const float ax = hypotf(x.x, x.y), am = hypotf(m.x, m.y);
        s0 += (double)(ax * ax); s1 += (double)(am * am);
    }
    red[0][tid] = s0; red[1][tid] = s1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; } __syncthreads(); }
    if (tid == 0) { part[((size_t)b * CH_NCH + ch) * 2] = red[0][0]; part[((size_t)b * CH_NCH + ch) * 2 + 1] = red[1][0]; }
}

// (philox4x32 and gauss_pair, the generated noise of every channel kernel: rade_devutil.h)

// per stream, ahead of k_chan_apply: the power-normalising gain and the phase the frequency offset has reached at the end of the signal, from the
// stream's partial power sums (added in their fixed order).  As a prologue of every k_chan_apply workgroup -- one thread, a hundred dependent
// additions, powf and a double-precision sincos while 255 threads wait -- this was a third of that kernel's time.
__global__ __launch_bounds__(64) void k_chan_gain(rd_chan_args a, const double *part, int n_part, float *gf)
{
    __builtin_amdgcn_s_setprio(3);
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double p0 = 0.0, p1 = 0.0;
    for (int c = 0; c < n_part; c++) { p0 += part[((size_t)b * n_part + c) * 2]; p1 += part[((size_t)b * n_part + c) * 2 + 1]; }
    const float tx_power = (float)(p0 / a.n_sig), mp_power = (float)(p1 / a.n_sig);
    const float foff = a.ps ? a.ps[a.B + b] : a.freq_offset, dfdt = a.ps ? a.ps[2 * a.B + b] : a.df_dt;
    float2 fin = make_float2(1.0f, 0.0f);
    if (foff != 0.0f && a.n_sig > 0) { float sn, cs; sincosf((float)chan_phase_acc(a.n_sig - 1, foff, dfdt), &sn, &cs); fin = make_float2(cs, sn); }
    gf[4 * b] = a.G ? powf(tx_power / mp_power, 0.5f) : 1.0f; gf[4 * b + 1] = fin.x; gf[4 * b + 2] = fin.y;
}

__global__ __launch_bounds__(256) void k_chan_apply(rd_chan_args a, const float *gf)
{
    const int b = blockIdx.y;
    const int n_eoo = a.with_eoo ? RD_NEOO : 0;
    const int n_total = a.n_pre + a.n_sig + n_eoo + a.n_post;
    const float gain = gf[4 * b]; const float2 fin = make_float2(gf[4 * b + 1], gf[4 * b + 2]);
    // the stream's channel condition: one uniform load per workgroup when the call gives per-stream values
    const float sigma = a.ps ? a.ps[b] : a.sigma, foff = a.ps ? a.ps[a.B + b] : a.freq_offset, dfdt = a.ps ? a.ps[2 * a.B + b] : a.df_dt;
    const float2 *tx = (const float2 *)a.tx + (size_t)b * a.tx_stride;
    const float2 *G = a.G ? (const float2 *)a.G + (size_t)b * a.n_sig * 2 : nullptr;
    const float2 *noise = a.noise ? (const float2 *)a.noise + (size_t)b * n_total : nullptr;
    const float2 *eoo = (const float2 *)a.eoo + (size_t)b * RD_NEOO;
    float2 *rx = (float2 *)a.rx + (size_t)b * a.rx_stride;
    // two consecutive samples per thread: one Philox4x32 call yields the four uniforms of both (the generator and the Box-Muller
    // transcendentals, not the bytes, are what this kernel's time is made of), and a thread's store is 16 bytes
    auto sample = [&](int j, uint32_t u0, uint32_t u1) -> float2 {
        float2 v = make_float2(0.0f, 0.0f);
        bool real_noise = true;
        const int i = j - a.n_pre;
        if (i >= 0 && i < a.n_sig) {
            real_noise = false;
            const float2 m = a.mp ? ((const float2 *)a.mp)[(size_t)b * a.n_sig + i] : chan_mp(tx, G, i);
            v = make_float2(m.x * gain, m.y * gain);
            if (foff != 0.0f) { float sn, cs; sincosf((float)chan_phase_acc(i, foff, dfdt), &sn, &cs); v = cmul(v, make_float2(cs, sn)); }
        } else if (i >= a.n_sig && i < a.n_sig + n_eoo) {
            real_noise = false;
            const int e = i - a.n_sig;
            float sn, cs; sincosf((float)chan_phase_acc(e, foff, dfdt), &sn, &cs);
            v = cmul(cmul(eoo[e], make_float2(cs, sn)), fin);
        }
        if (noise) { v.x += sigma * noise[j].x; v.y += sigma * noise[j].y; }
        else if (a.seed) {
            const float2 g = gauss_pair(u0, u1);
            if (real_noise) v.x += sigma * g.x;                                    // inference.py:277-284: real-valued randn
            else { v.x += sigma * 0.70710678f * g.x; v.y += sigma * 0.70710678f * g.y; }       // complex randn: 1/2 per component
        }
        if (a.sine_amp != 0.0f) {                                                  // inference.py:285-288, phase taken mod 1 cycle in double
            const double cyc = (double)j * (double)a.sine_freq / 8000.0;
            float sn, cs; sincosf((float)(6.283185307179586 * (cyc - floor(cyc))), &sn, &cs);
            v.x += a.sine_amp * cs; v.y += a.sine_amp * sn;
        }
        return make_float2(v.x * a.rx_gain, v.y * a.rx_gain);
    };
    const int n_pairs = (n_total + 1) >> 1;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += gridDim.x * 256) {
        uint32_t r[4] = { 0u, 0u, 0u, 0u };
        if (!noise && a.seed) philox4x32((uint32_t)p, (uint32_t)b, 0u, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
        const int j = 2 * p;
        const float2 v0 = sample(j, r[0], r[1]);
        if (j + 1 < n_total) {
            const float2 v1 = sample(j + 1, r[2], r[3]);
            if (((uintptr_t)rx & 15) == 0) *(f32x4 *)&rx[j] = (f32x4){ v0.x, v0.y, v1.x, v1.y };
            else { rx[j] = v0; rx[j + 1] = v1; }
        } else rx[j] = v0;
    }
}

// Watterson / Doppler-spread samples (doppler_spread.m:7-50, multipath_samples.m:25-31): one workgroup per stream.
// Low-rate noise -> FIR (double) into LDS, then two sweeps over the Fs-rate interpolation: variance, scaled write.
#define DG_MAXLOW 2048
// ybuf: [B][2][n_low] double2 in HBM for sequences of more than DG_MAXLOW low-rate points (lmr60: 500 low-rate points per second), else NULL (LDS)
__global__ __launch_bounds__(256) void k_multipath_gen(const float *taps, int n_taps, int low_ratio, int n_out, const float2 *noise_low,
                                                       unsigned long long seed, float2 *G, double2 *ybuf)
{
    __shared__ double2 ylds[2][DG_MAXLOW];
    __shared__ double red[256][6];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n_low = max((n_out + low_ratio - 1) / low_ratio, 2), n_x = n_low + n_taps;
    double2 *y = ybuf ? ybuf + (size_t)b * 2 * n_low : &ylds[0][0];
    const int ys = ybuf ? n_low : DG_MAXLOW;
    for (int idx = tid; idx < 2 * n_low; idx += 256) {
        const int p = idx / n_low, i = idx - p * n_low;
        double ar = 0.0, ai = 0.0;
        for (int k = 0; k < n_taps; k++) {                         // np.convolve(x, b)[ntaps:][i] = sum_k b[k] x[i + ntaps - k]
            const int xi = i + n_taps - k;
            float2 x;
            if (noise_low) x = noise_low[((size_t)b * 2 + p) * n_x + xi];
            else { uint32_t r[4]; philox4x32((uint32_t)xi, (uint32_t)(b * 2 + p), 1u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r); x = gauss_pair(r[0], r[1]); }
            ar += (double)taps[k] * x.x; ai += (double)taps[k] * x.y;
        }
        y[p * ys + i] = make_double2(ar, ai);
    }
    __threadfence_block();
    __syncthreads();
    auto interp = [&](int p, int n) {                               // linear interpolation, extrapolating past the last low-rate point
        const double pos = (double)n / (double)low_ratio;
        const int i0 = min((int)pos, n_low - 2);
        const double fr = pos - (double)i0;
        const double2 a0 = y[p * ys + i0], a1 = y[p * ys + i0 + 1];
        return make_double2(a0.x + (a1.x - a0.x) * fr, a0.y + (a1.y - a0.y) * fr);
    };
    double s[6] = { 0, 0, 0, 0, 0, 0 };                             // per path: sum re, sum im, sum |g|^2
    for (int n = tid; n < n_out; n += 256)
        for (int p = 0; p < 2; p++) { const double2 g = interp(p, n); s[3 * p] += g.x; s[3 * p + 1] += g.y; s[3 * p + 2] += g.x * g.x + g.y * g.y; }
    for (int k = 0; k < 6; k++) red[tid][k] = s[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { if (tid < off) for (int k = 0; k < 6; k++) red[tid][k] += red[tid + off][k]; __syncthreads(); }
    double var = 0.0;
    for (int p = 0; p < 2; p++) { const double mr = red[0][3 * p] / n_out, mi = red[0][3 * p + 1] / n_out; var += red[0][3 * p + 2] / n_out - (mr * mr + mi * mi); }
    const double hf_gain = 1.0 / sqrt(var);                         // np.var: population variance of the complex samples
    float2 *Gb = G + (size_t)b * n_out * 2;
    for (int n = tid; n < n_out; n += 256) {
        const double2 g1 = interp(0, n), g2 = interp(1, n);
        Gb[2 * n] = make_float2((float)(hf_gain * g1.x), (float)(hf_gain * g1.y));
        Gb[2 * n + 1] = make_float2((float)(hf_gain * g2.x), (float)(hf_gain * g2.y));
    }
}
extern "C" int rd_multipath_gen_needs_scratch(int low_ratio, int n_out) { return low_ratio >= 1 && (n_out + low_ratio - 1) / low_ratio > DG_MAXLOW; }
extern "C" int rd_launch_multipath_gen(const float *taps_dev, int n_taps, int low_ratio, int n_out, const void *noise_low, unsigned long long seed, void *G, void *ybuf, int B, rd_stream_t s)
{
    if (B <= 0 || n_out <= 0) return 0;
    if (low_ratio < 1 || n_taps < 1 || (!ybuf && (n_out + low_ratio - 1) / low_ratio > DG_MAXLOW)) return -1;
    hipLaunchKernelGGL(k_multipath_gen, dim3(B), dim3(256), 0, (hipStream_t)s, taps_dev, n_taps, low_ratio, n_out, (const float2 *)noise_low, seed, (float2 *)G, (double2 *)ybuf);
    return (int)hipGetLastError();
}

// Rate-Rs channel matrix from the rate-Fs Doppler samples (multipath_samples.m:33-40, :73-80): H[t][c] = G1[t M] + G2[t M] exp(-j 2 pi c d Rs), M = Fs / Rs
// (hf_gain is already in G); magnitudes (the default `.f32` form, what BBFM.forward and the rate-Rs model take) or complex.
__global__ void k_multipath_h(const float2 *G, int n_g, int M, int n_sym, int Nc, float dRs, int want_complex, float *H)
{
    const int b = blockIdx.y;
    const float2 *Gb = G + (size_t)b * n_g * 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)n_sym * Nc; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i / Nc), c = (int)(i - (long)t * Nc);
        const float2 g1 = Gb[2 * (size_t)t * M], g2 = Gb[2 * (size_t)t * M + 1];
        float sn, cs;
        sincosf(-6.283185307179586f * (float)c * dRs, &sn, &cs);
        const float hr = g1.x + g2.x * cs - g2.y * sn, hi = g1.y + g2.x * sn + g2.y * cs;
        if (want_complex) { H[2 * ((size_t)b * n_sym * Nc + i)] = hr; H[2 * ((size_t)b * n_sym * Nc + i) + 1] = hi; }
        else H[(size_t)b * n_sym * Nc + i] = sqrtf(hr * hr + hi * hi);
    }
}
extern "C" int rd_launch_multipath_h(const void *G, int n_g, int M, int n_sym, int Nc, float dRs, int want_complex, float *H, int B, rd_stream_t s)
{
    if (B <= 0 || n_sym <= 0) return 0;
    if (M < 1 || Nc < 1 || (long)(n_sym - 1) * M >= n_g) return -1;
    int gx = (int)(((long)n_sym * Nc + 255) / 256); if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_multipath_h, dim3(gx, B), dim3(256), 0, (hipStream_t)s, (const float2 *)G, n_g, M, n_sym, Nc, dRs, want_complex, H);
    return (int)hipGetLastError();
}

// The generator's two primitives alone, on chosen words (tests/test_device_noise_gpu.py against tests/noise_ref.py): words[i] = philox4x32(ctr[i], key) and
// g[j] = gauss_pair(u[j]); without u, pair j is words 2 (j & 1), 2 (j & 1) + 1 of counter j >> 1 (m <= 2 n).  No caller in the library.
__global__ __launch_bounds__(256) void k_noise_probe(const uint32_t *ctr, uint32_t k0, uint32_t k1, const uint32_t *u, uint32_t *words, float2 *g, int n, int m)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        uint32_t r[4];
        philox4x32(ctr[4 * (size_t)i], ctr[4 * (size_t)i + 1], ctr[4 * (size_t)i + 2], ctr[4 * (size_t)i + 3], k0, k1, r);
        for (int k = 0; k < 4; k++) words[4 * (size_t)i + k] = r[k];
    }
    for (int j = blockIdx.x * 256 + threadIdx.x; j < m; j += gridDim.x * 256) {
        uint32_t u0, u1;
        if (u) { u0 = u[2 * (size_t)j]; u1 = u[2 * (size_t)j + 1]; }
        else {
            const size_t i = (size_t)(j >> 1);
            uint32_t r[4];
            philox4x32(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], k0, k1, r);
            u0 = (j & 1) ? r[2] : r[0]; u1 = (j & 1) ? r[3] : r[1];
        }
        g[j] = gauss_pair(u0, u1);
    }
}
extern "C" int rd_launch_noise_probe(const uint32_t *ctr, uint32_t k0, uint32_t k1, const uint32_t *u, uint32_t *words, float *g, int n, int m, rd_stream_t s)
{
    if (n < 0 || m < 0 || (n > 0 && (!ctr || !words)) || (m > 0 && (!g || (!u && (!ctr || (long)m > 2L * n))))) return -1;
    if (n == 0 && m == 0) return 0;
    int gx = ((n > m ? n : m) + 255) / 256; if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_noise_probe, dim3(gx), dim3(256), 0, (hipStream_t)s, ctr, k0, k1, u, words, (float2 *)g, n, m);
    return (int)hipGetLastError();
}

// Symbol-domain channels of the non-OFDM configurations.
//  mode 0 (rate-Rs, radae.py:604-634, bottleneck 1): QPSK symbol k = (z[2k], z[2k+1]) * H[k] + sigma * CN(0,1)
//  mode 1 (BBFM, bbfm.py:157-197): per real symbol, FM demodulator SNR from the carrier-to-noise ratio:
//          CNRdB = 20log10(H)+CNR ; SNRdB = relu(CNR-12)+12+Gfm - relu(12-CNR)(1+Gfm/3) ; z_hat = clamp(z + N(0,1)/sqrt(SNR))
__global__ void k_chan_symbol(const float *z, const float *H, const float *noise, float *out, long n_real, int mode, float p0, float p1, unsigned long long seed)
{
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_real; i += (long)gridDim.x * blockDim.x) {
        float nz;
        if (noise) nz = noise[i];
        else if (seed) { uint32_t r[4]; philox4x32((uint32_t)(i >> 1), (uint32_t)((i >> 1) >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r); const float2 g = gauss_pair(r[0], r[1]); nz = (i & 1) ? g.y : g.x; if (mode == 0) nz *= 0.70710678f; }
        else nz = 0.0f;
        float v;
        if (mode == 0) { const float h = H ? H[i >> 1] : 1.0f; v = z[i] * h + p0 * nz; }            // p0 = sigma; complex noise: 1/2 per component (explicit tensors already are)
        else {
            const float h = H ? H[i] : 1.0f;
            const float cnr = 20.0f * log10f(h) + p0;                                                 // p0 = CNRdB, p1 = Gfm
            float snr = fmaxf(cnr - 12.0f, 0.0f) + 12.0f + p1;
            snr += -fmaxf(-(cnr - 12.0f), 0.0f) * (1.0f + p1 / 3.0f);
            const float sigma = 1.0f / powf(powf(10.0f, snr / 10.0f), 0.5f);
            v = fminf(fmaxf(z[i] + sigma * nz, -1.0f), 1.0f);
        }
        out[i] = v;
    }
}
extern "C" int rd_launch_chan_symbol(const float *z, const float *H, const float *noise, float *out, long n_real, int mode, float p0, float p1, unsigned long long seed, rd_stream_t s)
{
    if (n_real <= 0) return 0;
    int grid = (int)((n_real + 255) / 256); if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(k_chan_symbol, dim3(grid), dim3(256), 0, (hipStream_t)s, z, H, noise, out, n_real, mode, p0, p1, seed);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_channel(const rd_chan_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    hipStream_t st = (hipStream_t)s;
    float *gf = (float *)a->scratch;                        // scratch: [B][4] floats (gain, final phase), then the partial power sums
    double *part = (double *)a->scratch + 2 * (size_t)a->B;
    const int n_part = a->mp ? a->n_sig / RD_NMF : CH_NCH;
    if (!a->mp) hipLaunchKernelGGL(k_chan_power, dim3(CH_NCH, a->B), dim3(256), 0, st, *a, part);      // a->mp: the modulator left mp and its per-frame power sums (k_ofdm_mod_mp)
    hipLaunchKernelGGL(k_chan_gain, dim3((a->B + 63) / 64), dim3(64), 0, st, *a, (const double *)part, n_part, gf);
    const int n_total = a->n_pre + a->n_sig + (a->with_eoo ? RD_NEOO : 0) + a->n_post;
    int gx = (n_total + 255) / 256; if (gx > 32) gx = 32;          // (16..32 workgroups per stream measure the same; 64: +4 %, 8: +13 %)
    hipLaunchKernelGGL(k_chan_apply, dim3(gx, a->B), dim3(256), 0, st, *a, (const float *)gf);
    return (int)hipGetLastError();
}
