// rade_irx.hip -- the ideal-timing ("genie") rate-Fs receiver of RADAE.forward / RADAE.receiver (radae.py:312-420, :590-657): known timing,
// optional correction of a known frequency offset, cyclic prefix removal, the 160 -> 30 DFT, the pilot EQ of do_pilot_eq, the QPSK demapper.
//   k_irx_demod   one workgroup per (modem frame, stream), like k_ofdm_mod
//   k_irx_scale   one workgroup per stream: coarse_mag (radae.py:376-381) and the ber_test bit-error count (radae.py:653-657)
// Both are small next to the streaming receiver (genie receiver row); the DFT stays on the vector ALU.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"
#include "rade_irx.h"

__global__ __launch_bounds__(192) void k_irx_demod(rd_irx_args a)
{
    __shared__ float2 x[IRX_NSYM][RD_M];
    __shared__ float2 sym[IRX_NSYM][RD_NC];
    __shared__ float2 rp[2][RD_NC];                                  // pilot estimates: this frame's, the other frame's
    const int mf = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const rd_tables *tab = a.tab;
    const bool last = mf == a.n_mf - 1;
    const float2 *rx = (const float2 *)a.rx + (size_t)b * a.rx_stride;
    const float f0 = a.foff ? a.foff[b] : 0.0f, dfdt = a.foff ? a.foff[a.B + b] : 0.0f;
    // the DFT window [Ncp + time_offset, Ncp + time_offset + M) of every symbol; time_offset in [-Ncp, 0] keeps it inside the symbol, so the
    // last sample read is n_mf * 960 - 1
    for (int i = tid; i < IRX_NSYM * RD_M; i += 192) {
        const int s = i / RD_M, k = i - s * RD_M;
        const int fr = s < RD_NS + 1 ? mf : (last ? mf - 1 : mf + 1);
        const int n = fr * RD_NMF + (s < RD_NS + 1 ? s : 0) * RD_SYM + RD_NCP + a.time_offset + k;
        float2 v = rx[n];
        if (f0 != 0.0f) { float sn, cs; sincosf((float)chan_phase_acc(n, f0, dfdt), &sn, &cs); v = cmul(v, make_float2(cs, -sn)); }   // rx * conj(lin_phase), radae.py:594-595
        x[s][k] = v;
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
    if (a.eq != RD_IRX_NONE && tid < 2 * RD_NC) {
        const int i = tid / RD_NC, c = tid - i * RD_NC;
        rp[i][c] = irx_pilot(tab, sym[i ? RD_NS + 1 : 0], c, a.eq);
    }
    __syncthreads();
    if (tid == 0) {                                                  // coarse_mag: this frame's share of mean |rx_pilots|^2
        double p = 0.0;
        if (a.eq != RD_IRX_NONE) for (int c = 0; c < RD_NC; c++) p += (double)rp[0][c].x * rp[0][c].x + (double)rp[0][c].y * rp[0][c].y;
        a.part[(size_t)b * a.n_mf + mf] = p;
    }
    if (tid < RD_NS * RD_NC) {
        const int s = tid / RD_NC, c = tid - s * RD_NC;
        float2 v = sym[1 + s][c];
        if (a.eq != RD_IRX_NONE) {
            // phase-only linear interpolation between this frame's pilot and the next one's, at s + 1 of Ns + 1 (radae.py:350-356); the last frame keeps
            // the slope the loop left behind: carrier Nc - 1's, from frame n_mf - 2, for every carrier (radae.py:358-365)
            const float2 d = last ? make_float2(rp[0][RD_NC - 1].x - rp[1][RD_NC - 1].x, rp[0][RD_NC - 1].y - rp[1][RD_NC - 1].y)
                                  : make_float2(rp[1][c].x - rp[0][c].x, rp[1][c].y - rp[0][c].y);
            const float2 slope = make_float2(d.x / (float)(RD_NS + 1), d.y / (float)(RD_NS + 1));
            const float2 ch = make_float2(slope.x * (float)(s + 1) + rp[0][c].x, slope.y * (float)(s + 1) + rp[0][c].y);
            float sn, cs; sincosf(atan2f(ch.y, ch.x), &sn, &cs);
            v = cmul(v, make_float2(cs, -sn));
        }
        float *zf = a.z_hat + ((size_t)b * a.n_mf + mf) * RD_ZMF;    // the inverse of k_ofdm_mod's map
        zf[2 * tid] = v.x; zf[2 * tid + 1] = v.y;
    }
}

__global__ __launch_bounds__(256) void k_irx_scale(rd_irx_args a)
{
    __shared__ double red[4];
    __shared__ int cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float mag = 1.0f;
    const bool scale = a.coarse_mag && a.eq != RD_IRX_NONE;
    if (scale) {
        double p = 0.0;
        for (int i = tid; i < a.n_mf; i += 256) p += a.part[(size_t)b * a.n_mf + i];
        p = wave_sum_f64(p);
        if ((tid & 63) == 0) red[tid >> 6] = p;
        __syncthreads();
        const double tot = ((red[0] + red[1]) + red[2]) + red[3];
        mag = sqrtf((float)(tot / ((double)a.n_mf * RD_NC))) * a.mag_scale;
    }
    float *z = a.z_hat + (size_t)b * a.n_mf * RD_ZMF;
    const float *zr = a.z_ref ? a.z_ref + (size_t)b * a.n_mf * RD_ZMF : nullptr;
    int e = 0;
    for (int i = tid; i < a.n_mf * RD_ZMF; i += 256) {
        float v = z[i];
        if (scale) { v = v / mag; z[i] = v; }
        if (zr && -zr[i] * v > 0.0f) e++;                            // torch.sum(-z * z_hat > 0), radae.py:654
    }
    if (!a.n_err) return;
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off);
    if ((tid & 63) == 0) cnt[tid >> 6] = e;
    __syncthreads();
    if (tid == 0) a.n_err[b] = (long long)(((cnt[0] + cnt[1]) + cnt[2]) + cnt[3]);
}

extern "C" int rd_launch_irx(const rd_irx_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    if (a->n_mf < 2 || a->time_offset < -RD_NCP || a->time_offset > 0 || a->eq < RD_IRX_LS || a->eq > RD_IRX_NONE || !a->z_hat || !a->part) return -1;
    hipLaunchKernelGGL(k_irx_demod, dim3(a->n_mf, a->B), dim3(192), 0, (hipStream_t)s, *a);
    if ((a->coarse_mag && a->eq != RD_IRX_NONE) || a->z_ref) hipLaunchKernelGGL(k_irx_scale, dim3(a->B), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
