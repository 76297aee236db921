// rade_ofdm_mod.h -- the batched OFDM modulator and the end-of-over frame; part of rade_kernels.hip (see its inventory).
// Replaces: the transmitter's OFDM stage (dsp.py:340-378, radae.py:195-199, :208-219, :441-455, :545-548).
// Needs rd_tables and the RD_* frame geometry (rade_dev.h); cmul, cadd, pa_limit, idft_term, ld2, wave_sum_f64 (rade_devutil.h).
// (The frame synthesis stands in k_ofdm_mod, k_ofdm_mod_mp and k_tx_frame3 (rade_core_step.hip), the prefix store also in k_eoo_build: as one inlined
// function k_ofdm_mod and k_tx_frame3 changed register allocation and store order.  tests/test_hip_parity.py compares their samples bit for bit.)
// one workgroup per (modem frame, stream): 5 symbols x 160 samples, 30-term IDFT per sample
// LINEAR (RADE_BATCH_TX_LINEAR): the bottleneck-1 rate-Fs waveform (radae.py:195-199, :545-548): pilots at unit gain, no limiter
template <bool LINEAR>
__global__ __launch_bounds__(192) void k_ofdm_mod(const rd_tables *tab, const float *z, float2 *tx, long tx_stride, int n_mf)
{
    __shared__ float2 sym[RD_NS + 1][RD_NC];
    const int mf = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *zf = z + ((size_t)b * n_mf + mf) * RD_ZMF;
    const float pg = LINEAR ? 1.0f : tab->pilot_gain;
    if (tid < RD_NC) sym[0][tid] = make_float2(tab->P[tid] * pg, 0.0f * pg);
    if (tid < 120) sym[1 + tid / RD_NC][tid % RD_NC] = make_float2(zf[2 * tid], zf[2 * tid + 1]);
    __syncthreads();
    float2 *out = tx + (size_t)b * tx_stride + (size_t)mf * RD_NMF;
    if (tid < RD_M) {
        f32x2 acc[RD_NS + 1];
#pragma unroll
        for (int s = 0; s <= RD_NS; s++) acc[s] = (f32x2){ 0.0f, 0.0f };
#pragma unroll 6
        for (int c = 0; c < RD_NC; c++) {                 // one Winv load feeds the five symbols of the frame
            const float2 w = ld2(tab->Winv[c], tid);
#pragma unroll
            for (int s = 0; s <= RD_NS; s++) acc[s] = idft_term(acc[s], sym[s][c], w);
        }
#pragma unroll
        for (int s = 0; s <= RD_NS; s++) {
            const float2 v = LINEAR ? make_float2(acc[s][0], acc[s][1]) : pa_limit(make_float2(acc[s][0], acc[s][1]));
            out[s * RD_SYM + RD_NCP + tid] = v;
            if (tid >= RD_M - RD_NCP) out[s * RD_SYM + tid - (RD_M - RD_NCP)] = v;
        }
    }
}
extern "C" int rd_launch_ofdm_mod(const rd_tables *tab, const float *z, void *tx, long tx_stride, int B, int n_mf, int linear, rd_stream_t s)
{
    if (B <= 0 || n_mf <= 0) return 0;
    if (linear) hipLaunchKernelGGL(k_ofdm_mod<true>, dim3(n_mf, B), dim3(192), 0, (hipStream_t)s, tab, z, (float2 *)tx, tx_stride, n_mf);
    else hipLaunchKernelGGL(k_ofdm_mod<false>, dim3(n_mf, B), dim3(192), 0, (hipStream_t)s, tab, z, (float2 *)tx, tx_stride, n_mf);
    return (int)hipGetLastError();
}

// The modulator with the first half of the channel simulator folded in (rade_batch_tx_channel: RADAE.forward goes from latents to received
// samples in one pass too, radae.py:529-589): the workgroup keeps its modem frame's 960 samples in LDS, applies the two-path
// multipath model mp[i] = tx[i] G1[i] + tx[i-16] G2[i-16] while they are there (the 16 samples it needs from the frame before are
// re-synthesised: 16 x 30 terms) and leaves per-frame sums of |tx|^2 and |mp|^2 for the power normalisation.  tx never makes a round
// trip through HBM, k_chan_power disappears, and k_chan_apply reads 8 bytes per sample (mp) instead of 24 (tx + G).
template <bool LINEAR>
__global__ __launch_bounds__(192) void k_ofdm_mod_mp(const rd_tables *tab, const float *z, float2 *tx, long tx_stride, int n_mf, const float2 *G, float2 *mp, double *part)
{
    __shared__ float2 sym[RD_NS + 1][RD_NC];
    __shared__ float2 prevsym[RD_NC];
    __shared__ float2 fr[16 + RD_NMF];                    // [0, 16): tail of the previous frame, then this frame
    __shared__ double red[2][4];
    const int mf = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float *zf = z + ((size_t)b * n_mf + mf) * RD_ZMF;
    const float pg = LINEAR ? 1.0f : tab->pilot_gain;
    if (tid < RD_NC) sym[0][tid] = make_float2(tab->P[tid] * pg, 0.0f * pg);
    if (tid < 120) sym[1 + tid / RD_NC][tid % RD_NC] = make_float2(zf[2 * tid], zf[2 * tid + 1]);
    if (tid >= 128 && tid < 128 + RD_NC && mf > 0) { const int c = tid - 128; prevsym[c] = make_float2(zf[-RD_ZMF + 2 * (90 + c)], zf[-RD_ZMF + 2 * (90 + c) + 1]); }   // last data symbol of frame mf - 1
    __syncthreads();
    if (tid < RD_M) {
        f32x2 acc[RD_NS + 1];
#pragma unroll
        for (int s = 0; s <= RD_NS; s++) acc[s] = (f32x2){ 0.0f, 0.0f };
#pragma unroll 6
        for (int c = 0; c < RD_NC; c++) {
            const float2 w = ld2(tab->Winv[c], tid);
#pragma unroll
            for (int s = 0; s <= RD_NS; s++) acc[s] = idft_term(acc[s], sym[s][c], w);
        }
#pragma unroll
        for (int s = 0; s <= RD_NS; s++) {
            const float2 v = LINEAR ? make_float2(acc[s][0], acc[s][1]) : pa_limit(make_float2(acc[s][0], acc[s][1]));
            fr[16 + s * RD_SYM + RD_NCP + tid] = v;
            if (tid >= RD_M - RD_NCP) fr[16 + s * RD_SYM + tid - (RD_M - RD_NCP)] = v;
        }
    } else if (tid < RD_M + 16) {                          // samples 944..959 of the previous frame = the last 16 of its last symbol
        const int n = RD_M - 16 + (tid - RD_M);
        float2 a = make_float2(0.0f, 0.0f);
        if (mf > 0) { f32x2 ac = { 0.0f, 0.0f }; for (int c = 0; c < RD_NC; c++) ac = idft_term(ac, prevsym[c], ld2(tab->Winv[c], n)); a = LINEAR ? make_float2(ac[0], ac[1]) : pa_limit(make_float2(ac[0], ac[1])); }
        fr[tid - RD_M] = a;                                // frame 0: the signal starts here, nothing before it (chan_mp: i >= 16)
    }
    __syncthreads();
    const size_t base = (size_t)mf * RD_NMF;
    const f32x4 *Gb = (const f32x4 *)G + (size_t)b * n_mf * RD_NMF;      // (G1[i], G2[i]) as one 16-byte load per sample
    // (requesting these before the IDFT instead -- 20 more registers live across it -- made the kernel 5 % slower: 187 -> 196 us; the IDFT and the
    // limiter, not the round trip, are what a workgroup spends its time on)
    float2 *mpo = mp + (size_t)b * n_mf * RD_NMF + base;
    float2 *txo = tx ? tx + (size_t)b * tx_stride + base : nullptr;
    // second path: c2[i + 16] = tx[i] G2[i], written to LDS by the thread that holds G2[i]; the first 16 slots of the frame come from the
    // previous frame's tail (fr[0..16)) and its G2
    __shared__ float2 c2[16 + RD_NMF];
    float2 a1[5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const int i = tid + 192 * q;                       // 960 = 5 x 192
        const f32x4 g = Gb[base + i];
        const float2 x = fr[16 + i];
        a1[q] = cmul(x, make_float2(g[0], g[1]));
        c2[16 + i] = cmul(x, make_float2(g[2], g[3]));
    }
    if (tid < 16) { float2 v = make_float2(0.0f, 0.0f); if (mf > 0) { const f32x4 g = Gb[base - 16 + tid]; v = cmul(fr[tid], make_float2(g[2], g[3])); } c2[tid] = v; }
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const int i = tid + 192 * q;
        const float2 x = fr[16 + i];
        const float2 m = cadd(a1[q], c2[i]);               // c2[i] = tx[base + i - 16] G2[base + i - 16]; zero for the first 16 samples of the signal
        mpo[i] = m;
        if (txo) txo[i] = x;
        const float ax = hypotf(x.x, x.y), am = hypotf(m.x, m.y);
        s0 += (double)(ax * ax); s1 += (double)(am * am);
    }
    // frame sums: inside a wavefront by DPP, the three wavefronts' results through LDS (one barrier; the LDS tree this replaces had eight)
    s0 = wave_sum_f64(s0); s1 = wave_sum_f64(s1);
    if ((tid & 63) == 0) { red[0][tid >> 6] = s0; red[1][tid >> 6] = s1; }
    __syncthreads();
    if (tid == 0) { part[((size_t)b * n_mf + mf) * 2] = (red[0][0] + red[0][1]) + red[0][2]; part[((size_t)b * n_mf + mf) * 2 + 1] = (red[1][0] + red[1][1]) + red[1][2]; }
}
extern "C" int rd_launch_ofdm_mod_mp(const rd_tables *tab, const float *z, void *tx, long tx_stride, int B, int n_mf, const void *G, void *mp, double *part, int linear, rd_stream_t s)
{
    if (B <= 0 || n_mf <= 0) return 0;
    if (linear) hipLaunchKernelGGL(k_ofdm_mod_mp<true>, dim3(n_mf, B), dim3(192), 0, (hipStream_t)s, tab, z, (float2 *)tx, tx_stride, n_mf, (const float2 *)G, (float2 *)mp, part);
    else hipLaunchKernelGGL(k_ofdm_mod_mp<false>, dim3(n_mf, B), dim3(192), 0, (hipStream_t)s, tab, z, (float2 *)tx, tx_stride, n_mf, (const float2 *)G, (float2 *)mp, part);
    return (int)hipGetLastError();
}

// EOO frame per stream: default table copy, optionally with 3 data symbols (90 QPSK) inserted
__global__ __launch_bounds__(192) void k_eoo_build(const rd_tables *tab, const float *bits, float2 *eoo)
{
    __shared__ float2 sym[RD_NS - 1][RD_NC];
    const int b = blockIdx.x, tid = threadIdx.x;
    float2 *out = eoo + (size_t)b * RD_NEOO;
    for (int i = tid; i < RD_NEOO; i += blockDim.x) out[i] = ld2(tab->eoo, i);
    if (!bits) return;
    if (tid < 90) sym[tid / RD_NC][tid % RD_NC] = make_float2(bits[b * RD_NEOOBITS + 2 * tid], bits[b * RD_NEOOBITS + 2 * tid + 1]);
    __syncthreads();
    if (tid < RD_M) {
        for (int s = 0; s < RD_NS - 1; s++) {
            float2 acc = make_float2(0.0f, 0.0f);
            for (int c = 0; c < RD_NC; c++) acc = cadd(acc, cmul(sym[s][c], ld2(tab->Winv[c], tid)));
            const float2 v = pa_limit(make_float2(acc.x * tab->pilot_gain, acc.y * tab->pilot_gain));
            out[(2 + s) * RD_SYM + RD_NCP + tid] = v;
            if (tid >= RD_M - RD_NCP) out[(2 + s) * RD_SYM + tid - (RD_M - RD_NCP)] = v;
        }
    }
}
extern "C" int rd_launch_eoo_build(const rd_tables *tab, const float *bits, float *eoo, int B, rd_stream_t s)
{
    hipLaunchKernelGGL(k_eoo_build, dim3(B), dim3(192), 0, (hipStream_t)s, tab, bits, (float2 *)eoo);
    return (int)hipGetLastError();
}
__global__ void k_copy_eoo(const float2 *eoo, float2 *out, long stride)
{
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < RD_NEOO; i += blockDim.x) out[(size_t)b * stride + i] = eoo[(size_t)b * RD_NEOO + i];
}
extern "C" int rd_launch_copy_eoo(const float *eoo, void *out, long stride, int B, rd_stream_t s)
{
    hipLaunchKernelGGL(k_copy_eoo, dim3(B), dim3(256), 0, (hipStream_t)s, (const float2 *)eoo, (float2 *)out, stride);
    return (int)hipGetLastError();
}
