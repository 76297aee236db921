// rade_snr.hip -- the trials of rade_batch_snr_trials (include/rade_batch.h states the arithmetic, the summation order and the error bound): est_snr.py:45-124 with
// receiver_one.est_pilots (dsp.py:418-435), the six sums of every window of Nw pilot rows x 30 carriers of every stream.
//   k_snr_trials   one wavefront per (window, stream), lane = carrier (30 of 64 lanes work); walks the window's rows once
// Per row: the lane forms its carrier's s = h (pg P), n = sigma g and x = s + n and leaves x in LDS; after the barrier it takes the three neighbours of c_mid from
// there (irx_pilot of rade_irx.h, unchanged: the least-squares estimate of the ideal-timing receiver), e = Im(x conj(r) / |r|) (unit_conj: angle(0) = 0), and leaves
// its six float32 terms in LDS; after the second barrier lane j < 6 adds the 30 terms of sum j in carrier order to its double.  Rows in ascending order, so every sum
// runs row-major over the window, carrier-minor, in one lane: no atomics, no dependence on the grid.  The workgroup is one wavefront, so the two barriers per row
// cost next to nothing; the x of the next row is not written before every lane has passed the second barrier of this one.
// Generated noise: one Philox counter per pair of carriers, q = 15 R + (c >> 1) of the ABSOLUTE row R (both lanes of a pair compute it: the generator is a handful of
// integer multiplies, cheaper than an exchange); words 0-1 the even carrier, 2-3 the odd one.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"
#include "rade_irx.h"

__global__ __launch_bounds__(64) void k_snr_trials(rd_snr_args a)
{
    __shared__ float2 xrow[32];
    __shared__ float term[RD_SNR_NSUM][32];
    const int k = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
    const rd_snr_stream S = a.ps[b];
    if (k >= S.n_win) return;                                                   // the whole workgroup: no barrier is left waiting
    const bool on = c < RD_NC;
    const int Nw = a.Nw;
    const float pgp = on ? a.tab->pilot_gain * a.tab->P[c] : 0.0f;
    const float2 *H = a.H ? (const float2 *)a.H + (size_t)b * a.h_stride : nullptr;
    const float2 *nz = a.noise ? (const float2 *)a.noise + (size_t)b * a.noise_stride : nullptr;
    float2 *nout = a.noise_out ? (float2 *)a.noise_out + (size_t)b * a.noise_stride : nullptr;
    double acc = 0.0;
    for (int i = 0; i < Nw; i++) {
        const long long lr = (long long)k * Nw + i;                             // the row inside the call: < n_win Nw, which the entry checked against the strides
        float2 x = make_float2(0.0f, 0.0f), s = x, n = x;
        if (on) {
            float2 g;
            if (nz) g = nz[(size_t)lr * RD_NC + c];
            else {
                const unsigned long long q = 15ull * (unsigned long long)(S.row0 + lr) + (unsigned)(c >> 1);
                uint32_t w[4];
                philox4x32((uint32_t)q, (uint32_t)b, 4u, (uint32_t)(q >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
                g = (c & 1) ? gauss_pair(w[2], w[3]) : gauss_pair(w[0], w[1]);
                if (nout) nout[(size_t)lr * RD_NC + c] = g;
            }
            const float2 h = H ? H[(size_t)lr * a.h_step * RD_NC + c] : make_float2(1.0f, 0.0f);
            s = make_float2(h.x * pgp, h.y * pgp);
            n = make_float2(S.sigma * g.x, S.sigma * g.y);
            x = cadd(s, n);
            xrow[c] = x;
        }
        __syncthreads();
        if (on) {
            const float2 u = unit_conj(irx_pilot(a.tab, xrow, c, RD_IRX_LS));
            const float e = x.x * u.y + x.y * u.x;                              // Im(x conj(r) / |r|)
            term[0][c] = x.x * x.x + x.y * x.y;
            term[1][c] = s.x * s.x + s.y * s.y;
            term[2][c] = 2.0f * (s.x * n.x - s.y * n.y);                        // 2 Re(s n): no conjugate, as the script has it
            term[3][c] = n.x * n.x + n.y * n.y;
            term[4][c] = n.y * n.y;                                             // Im(|h| pg P + n): the signal term is real
            term[5][c] = e * e;
        }
        __syncthreads();
        if (c < RD_SNR_NSUM)
            for (int j = 0; j < RD_NC; j++) acc += (double)term[c][j];
    }
    if (c < RD_SNR_NSUM) a.sums[((size_t)b * a.max_win + k) * RD_SNR_NSUM + c] = acc;
}

extern "C" int rd_launch_snr_trials(const rd_snr_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_win <= 0) return 0;
    if (a->B > 65535 || a->Nw < 1 || a->Nw > RD_SNR_NW_MAX || a->h_step < 1 || a->h_step > RD_SNR_HSTEP_MAX) return -1;
    if (!a->tab || !a->ps || !a->sums || (!a->noise && !a->seed) || (a->noise && (a->seed || a->noise_out))) return -1;
    hipLaunchKernelGGL(k_snr_trials, dim3(a->max_win, a->B), dim3(64), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
