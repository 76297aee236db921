// rade_rs.hip -- the rate-Rs channel of the bottleneck-3 model, the "hybrid time & frequency domain model" of RADAE.forward (radae.py:603-634):
// every OFDM symbol of the no-pilot, no-prefix numerology (Nc = 20 carriers at DFT bins 20..39, M = 160 samples, Ns = 6) goes through the IDFT, the
// power-amplifier limiter tanh(|tx|) e^{j angle(tx)} and the DFT; phase offset, per-carrier magnitudes H and AWGN are then applied to the symbols.
//   k_rs_pa      one workgroup per (chunk of symbol tiles, stream): RS_SB symbols at a time, both transforms on the vector ALU with the twiddles in LDS
//   k_rs_stats   per stream: the chunks' measurement partials (sum |tx'|^2, max |tx'|, sum |Y|^2) added in their fixed order
// The carriers are bins 5..24 of the 30-carrier rate-Fs waveform (same M, same w), so the twiddles come from rd_tables.Wfwd: the float32 values the
// reference's Winv / Wfwd hold (rade_host.c).
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"

#define RS_NC 20          // carriers
#define RS_C0 5           // first carrier as a column of rd_tables.Wfwd (DFT bin 15 + 5)
#define RS_SB 8           // symbols per tile
#define RS_WG 192         // threads: RS_SB * RS_NC = RD_M = 160 of them work in every phase
#define RS_NP (RD_M / RS_NC)   // the DFT's sum over m in 8 parts of 20 samples
#define RS_ES (RD_M + 1)  // row stride of the twiddle table in LDS: the DFT reads column m of 20 rows at once

static_assert(RS_SB * RS_NC == RD_M && RS_NP * RS_NC == RD_M && RD_M <= RS_WG, "the phases of k_rs_pa share one thread mapping");

// tanh(|x|) e^{j angle(x)} = x tanh(|x|) / |x|.  pa_limit's (1 - e) / (1 + e) cancels below |x| ~ 0.1 (absolute error 3e-8 on the sample whatever its size:
// nothing for a transmitter that fills the amplifier, but this channel is also run in its linear region, inference.py's Eq / PAPR check), so small magnitudes
// take the series of tanh(x) / x (next term 9e-9 at 0.25).  0 gives exactly 0.  A component past 2^40 (where tanh is 1 to the last bit, and the square of
// anything above 1.8e19 would overflow) gives the unit vector, formed from the sample divided by its larger component: magnitude 1 for every finite sample.
__device__ __forceinline__ float2 rs_pa_limit(float2 x)
{
    const float big = fmaxf(fabsf(x.x), fabsf(x.y));
    if (big > 1.0995116e12f) {
        const float sx = x.x / big, sy = x.y / big;
        const float r = __builtin_amdgcn_rsqf(fmaf(sx, sx, sy * sy));
        return make_float2(sx * r, sy * r);
    }
    const float m2 = fmaf(x.x, x.x, x.y * x.y);
    if (m2 == 0.0f) return make_float2(0.0f, 0.0f);
    float g;
    if (m2 < 0.0625f) g = fmaf(m2, fmaf(m2, fmaf(m2, fmaf(m2, 62.0f / 2835.0f, -17.0f / 315.0f), 2.0f / 15.0f), -1.0f / 3.0f), 1.0f);
    else {
        const float mag = __builtin_amdgcn_sqrtf(m2);
        const float e = __builtin_amdgcn_exp2f(-2.88539008177792681f * mag);       // e^{-2 |x|}
        g = (1.0f - e) * __builtin_amdgcn_rcpf((1.0f + e) * mag);
    }
    return make_float2(x.x * g, x.y * g);
}

__global__ __launch_bounds__(RS_WG) void k_rs_pa(rd_rs_args a, int n_chunks)
{
    __shared__ float2 E[RS_NC][RS_ES];               // e^{+j m w_c}
    __shared__ float2 sym[RS_SB][RS_NC];
    __shared__ float2 tx[RS_SB][RD_M];
    __shared__ float2 part[RS_NP][RS_SB][RS_NC];
    __shared__ double red[3][RS_WG / 64];
    const int ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n_sym = 2 * a.n_steps, n_tiles = (n_sym + RS_SB - 1) / RS_SB;
    const size_t row = (size_t)b * n_sym;            // the stream's first symbol
    const float *z = a.z + row * (2 * RS_NC);
    const float *H = a.H ? a.H + row * RS_NC : nullptr;
    const float2 *noise = a.noise ? (const float2 *)a.noise + row * RS_NC : nullptr;
    float *z_hat = a.z_hat + row * (2 * RS_NC);
    const float sigma = a.sigma_b ? a.sigma_b[b] : a.sigma;
    const bool work = tid < RD_M;
    const int k_o = tid / RS_NC, c_o = tid - k_o * RS_NC;      // (symbol of the tile, carrier) when loading and writing; (part, carrier) in the DFT

    for (int i = tid; i < RS_NC * RD_M; i += RS_WG) {
        const int c = i / RD_M, m = i - c * RD_M;
        E[c][m] = make_float2(a.tab->Wfwd[m][RS_C0 + c][0], -a.tab->Wfwd[m][RS_C0 + c][1]);
    }
    double s_tx2 = 0.0, s_sym2 = 0.0;
    float mx2 = 0.0f;
    for (int tile = ch; tile < n_tiles; tile += n_chunks) {
        const int s0 = tile * RS_SB;
        __syncthreads();
        // symbols past the end of the stream are zeros: they pass through every phase as zeros and add nothing to the sums
        if (work) {
            const int s = s0 + k_o;
            sym[k_o][c_o] = s < n_sym ? make_float2(z[(size_t)s * 40 + 2 * c_o], z[(size_t)s * 40 + 2 * c_o + 1]) : make_float2(0.0f, 0.0f);
        }
        __syncthreads();
        if (work) {                                  // tx[m] = (1 / M) sum_c sym[c] e^{+j m w_c} of the tile's symbols, then the limiter
            f32x2 acc[RS_SB];
#pragma unroll
            for (int k = 0; k < RS_SB; k++) acc[k] = (f32x2){ 0.0f, 0.0f };
#pragma unroll 4
            for (int c = 0; c < RS_NC; c++) {
                const float2 e = E[c][tid];
#pragma unroll
                for (int k = 0; k < RS_SB; k++) acc[k] = idft_term(acc[k], sym[k][c], e);
            }
#pragma unroll
            for (int k = 0; k < RS_SB; k++) {
                const float2 v = rs_pa_limit(make_float2(acc[k][0] * (1.0f / RD_M), acc[k][1] * (1.0f / RD_M)));
                tx[k][tid] = v;
                const float p = fmaf(v.x, v.x, v.y * v.y);
                s_tx2 += (double)p; mx2 = fmaxf(mx2, p);
            }
        }
        __syncthreads();
        if (work) {                                  // Y[c] = sum_m tx'[m] e^{-j m w_c}: this thread's 20 samples of carrier c_o for the tile's symbols
            f32x2 acc[RS_SB];
#pragma unroll
            for (int k = 0; k < RS_SB; k++) acc[k] = (f32x2){ 0.0f, 0.0f };
#pragma unroll 4
            for (int i = 0; i < RS_NC; i++) {
                const int m = k_o * RS_NC + i;
                const float2 e = E[c_o][m];
#pragma unroll
                for (int k = 0; k < RS_SB; k++) {
                    const float2 x = tx[k][m];
                    acc[k][0] = fmaf(x.x, e.x, acc[k][0]); acc[k][1] = fmaf(x.y, e.x, acc[k][1]);
                    acc[k][0] = fmaf(x.y, e.y, acc[k][0]); acc[k][1] = fmaf(-x.x, e.y, acc[k][1]);
                }
            }
#pragma unroll
            for (int k = 0; k < RS_SB; k++) part[k_o][k][c_o] = make_float2(acc[k][0], acc[k][1]);
        }
        __syncthreads();
        const int s = s0 + k_o;
        if (work && s < n_sym) {                     // the parts in their order, phase offset, |H|, noise, demap
            float2 y = part[0][k_o][c_o];
#pragma unroll
            for (int p = 1; p < RS_NP; p++) y = cadd(y, part[p][k_o][c_o]);
            if (a.has_phase) y = cmul(y, make_float2(a.ph_re, a.ph_im));
            const size_t i = (size_t)s * RS_NC + c_o;
            if (H) { const float hm = H[i]; y = make_float2(y.x * hm, y.y * hm); }
            s_sym2 += (double)y.x * (double)y.x + (double)y.y * (double)y.y;
            if (noise) { const float2 n = noise[i]; y.x = fmaf(sigma, n.x, y.x); y.y = fmaf(sigma, n.y, y.y); }
            else if (a.seed) {                       // one Philox counter per pair of carriers: words 0-1 the even one, 2-3 the odd one
                uint32_t r[4];
                philox4x32((uint32_t)(i >> 1), (uint32_t)b, 2u, (uint32_t)((i >> 1) >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
                const float2 g = (i & 1) ? gauss_pair(r[2], r[3]) : gauss_pair(r[0], r[1]);
                y.x = fmaf(sigma * 0.70710678f, g.x, y.x); y.y = fmaf(sigma * 0.70710678f, g.y, y.y);
            }
            z_hat[(size_t)s * 40 + 2 * c_o] = y.x; z_hat[(size_t)s * 40 + 2 * c_o + 1] = y.y;
        }
    }
    // the chunk's measurements: inside a wavefront by DPP, the three wavefronts in their order
    s_tx2 = wave_sum_f64(s_tx2); s_sym2 = wave_sum_f64(s_sym2); mx2 = wave_max_f32(mx2);
    if ((tid & 63) == 0) { red[0][tid >> 6] = s_tx2; red[1][tid >> 6] = s_sym2; red[2][tid >> 6] = (double)mx2; }
    __syncthreads();
    if (tid == 0) {
        double *o = a.part + ((size_t)b * RD_RS_NCH + ch) * 4;
        o[0] = (red[0][0] + red[0][1]) + red[0][2]; o[1] = fmax(fmax(red[2][0], red[2][1]), red[2][2]); o[2] = (red[1][0] + red[1][1]) + red[1][2];
    }
}

__global__ __launch_bounds__(64) void k_rs_stats(const double *part, int n_chunks, double *stats, int B)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double t = 0.0, mx = 0.0, y = 0.0;
    for (int c = 0; c < n_chunks; c++) { const double *p = part + ((size_t)b * RD_RS_NCH + c) * 4; t += p[0]; mx = fmax(mx, p[1]); y += p[2]; }
    stats[3 * b] = t; stats[3 * b + 1] = sqrt(mx); stats[3 * b + 2] = y;
}

extern "C" int rd_launch_rs_pa(const rd_rs_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->n_steps <= 0) return 0;
    const int n_tiles = (2 * a->n_steps + RS_SB - 1) / RS_SB;
    const int n_chunks = n_tiles < RD_RS_NCH ? n_tiles : RD_RS_NCH;
    hipLaunchKernelGGL(k_rs_pa, dim3(n_chunks, a->B), dim3(RS_WG), 0, (hipStream_t)s, *a, n_chunks);
    if (a->stats) hipLaunchKernelGGL(k_rs_stats, dim3((a->B + 63) / 64), dim3(64), 0, (hipStream_t)s, (const double *)a->part, n_chunks, a->stats, a->B);
    return (int)hipGetLastError();
}
