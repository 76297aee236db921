// rade_chanp.hip -- the rate-Fs channel and the Doppler generator in pieces, rade_batch_channel_piece / rade_batch_multipath_piece (include/rade_batch.h states the
// arithmetic).  Every output is a pure function of its absolute sample index n and the call's values: no device state, no measured power or variance, no end of the
// sequence.  A stream cut into pieces anywhere equals the stream in one piece, bit for bit.
//   k_dopp_piece   one workgroup per (tile of RD_DOPP_TILE outputs, stream): the tile's low-rate draws once into LDS, the FIR in double from LDS into LDS, then the
//                  linear interpolation to Fs and the store.  A low-rate output y[i] is one sequential sum over k = 0..n_taps-1 whichever tile forms it.
//   k_chan_piece   two consecutive samples (2 P, 2 P + 1: one Philox counter) per thread, the even one and the odd one each at its own place in the code, so a sample
//                  is formed by the same instructions wherever a piece begins; 16-byte stores where the stream's row puts the pair on a 16-byte boundary.
// The whole-utterance kernels (rade_chan.h) are not touched: these take the expected-value hf_gain and a caller's gain instead of measured ones, a 64-bit integer phase
// instead of a float32 one, and never extrapolate.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"

#define DP_WG 256
#define DP_NY (RD_DOPP_TILE + 2)                                     // low-rate points of a tile: (cnt - 1) / low_ratio + 3 at most
#define DP_NX (DP_NY - 1 + RD_DOPP_NTAPS_MAX)                        // draws of a tile and path: y[i] reads x[i + 1 .. i + n_taps]
static_assert(2 * DP_NX * 8 + 2 * DP_NY * 16 + RD_DOPP_NTAPS_MAX * 8 <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(DP_WG) void k_dopp_piece(rd_dopp_args a)
{
    __shared__ float2 xs[2][DP_NX];
    __shared__ double2 ys[2][DP_NY];
    __shared__ double tp[RD_DOPP_NTAPS_MAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    const rd_dopp_stream S = a.ps[b];
    const long long o0 = (long long)blockIdx.x * RD_DOPP_TILE;
    if (o0 >= S.n_out) return;
    const int cnt = min(RD_DOPP_TILE, (int)(S.n_out - o0)), n_taps = a.n_taps;
    const long long nb = S.n0 + o0, r = a.low_ratio;                 // absolute index of the tile's first output
    const long long i_first = nb / r, i_last = (nb + cnt - 1) / r;
    const int ny = (int)(i_last - i_first) + 2, nx = ny - 1 + n_taps;       // y[i_first .. i_last + 1]; x[i_first + 1 .. i_last + 1 + n_taps]
    for (int k = tid; k < n_taps; k += DP_WG) tp[k] = (double)a.taps[k];
    for (int idx = tid; idx < 2 * nx; idx += DP_WG) {                // each draw once per tile
        const int p = idx / nx, j = idx - p * nx;
        const unsigned long long xi = (unsigned long long)(i_first + 1 + j);
        uint32_t w[4];
        philox4x32((uint32_t)xi, (uint32_t)(b * 2 + p), 1u, (uint32_t)(xi >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
        xs[p][j] = gauss_pair(w[0], w[1]);
    }
    __syncthreads();
    for (int idx = tid; idx < 2 * ny; idx += DP_WG) {
        const int p = idx / ny, i = idx - p * ny;
        double ar = 0.0, ai = 0.0;
        for (int k = 0; k < n_taps; k++) {                           // y[i] = sum_k b[k] x[i + n_taps - k], k ascending (k_multipath_gen's expression)
            const float2 x = xs[p][i + n_taps - 1 - k];
            ar += tp[k] * x.x; ai += tp[k] * x.y;
        }
        ys[p][i] = make_double2(ar, ai);
    }
    __syncthreads();
    float2 *Gb = (float2 *)a.G + ((size_t)b * a.g_stride + (size_t)o0) * 2;
    const bool wide = ((uintptr_t)a.G & 15) == 0;                    // a pair is 16 bytes: an aligned base aligns every pair
    for (int j = tid; j < cnt; j += DP_WG) {
        const long long n = nb + j, i0 = n / r;
        const double fr = (double)(n - i0 * r) / (double)r;
        const int li = (int)(i0 - i_first);
        const double2 a0 = ys[0][li], a1 = ys[0][li + 1], c0 = ys[1][li], c1 = ys[1][li + 1];
        const double g1x = a0.x + (a1.x - a0.x) * fr, g1y = a0.y + (a1.y - a0.y) * fr;
        const double g2x = c0.x + (c1.x - c0.x) * fr, g2y = c0.y + (c1.y - c0.y) * fr;
        const float2 G1 = make_float2((float)(a.hf_gain * g1x), (float)(a.hf_gain * g1y)), G2 = make_float2((float)(a.hf_gain * g2x), (float)(a.hf_gain * g2y));
        if (wide) *(f32x4 *)&Gb[2 * j] = (f32x4){ G1.x, G1.y, G2.x, G2.y };
        else { Gb[2 * j] = G1; Gb[2 * j + 1] = G2; }
    }
}

extern "C" int rd_launch_dopp_piece(const rd_dopp_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_out <= 0) return 0;
    if (a->B > 65535 || a->n_taps < 1 || a->n_taps > RD_DOPP_NTAPS_MAX || a->low_ratio < 1) return -1;
    const int n_tiles = (a->max_out + RD_DOPP_TILE - 1) / RD_DOPP_TILE;
    hipLaunchKernelGGL(k_dopp_piece, dim3(n_tiles, a->B), dim3(DP_WG), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void k_chan_piece(rd_chanp_args a)
{
    const int b = blockIdx.y;
    const rd_chanp_stream S = a.ps[b];                               // the stream's record: uniform loads
    if (S.n_out <= 0) return;
    const float sigma = S.sigma, gain = S.gain;
    const float2 *tx = (const float2 *)a.tx + (size_t)b * a.tx_stride;
    const float2 *G = a.G ? (const float2 *)a.G + (size_t)b * a.g_stride * 2 : nullptr;
    const float2 *noise = a.noise ? (const float2 *)a.noise + (size_t)b * a.noise_stride : nullptr;
    float2 *rx = (float2 *)a.rx + (size_t)b * a.rx_stride;
    // transmit sample of absolute index n: zero in front of the stream and outside the row; Doppler sample likewise (the host refuses a row that does not cover the piece)
    auto tx_at = [&](long long n) -> float2 { const long long g = n - S.in_base; return g >= 0 && g < S.n_in ? tx[g] : make_float2(0.0f, 0.0f); };
    auto g_at = [&](long long n, int path) -> float2 { const long long g = n - S.g_base; return g >= 0 && g < S.n_g ? G[2 * g + path] : make_float2(0.0f, 0.0f); };
    auto sample = [&](long long n, uint32_t u0, uint32_t u1) -> float2 {
        float2 m;
        if (!G) m = tx_at(n);
        else {                                                       // chan_mp's expression
            m = cmul(tx_at(n), g_at(n, 0));
            if (n >= 16) m = cadd(m, cmul(tx_at(n - 16), g_at(n - 16, 1)));
        }
        float2 v = make_float2(m.x * gain, m.y * gain);
        if (S.rotate) {                                              // ph[n] = (n + 1) f0q + T(n) dq mod 2^64, T(n) = n (n + 1) / 2: the even factor halved first
            const unsigned long long un = (unsigned long long)n;
            const unsigned long long T = (un & 1) ? un * ((un + 1) >> 1) : (un >> 1) * (un + 1);
            const unsigned long long ph = (un + 1) * S.f0q + T * S.dq;
            v = cmul(v, fm_cis((unsigned)(ph >> 32)));
        }
        if (noise) { const int i = (int)(n - S.n0); v.x += sigma * noise[i].x; v.y += sigma * noise[i].y; }
        else if (a.seed) {
            const float2 g = gauss_pair(u0, u1);
            if (a.noise_mode) v.x += sigma * g.x;                                  // RADE_CHANP_NOISE_REAL: inference.py:277-284
            else { v.x += sigma * 0.70710678f * g.x; v.y += sigma * 0.70710678f * g.y; }       // complex randn: 1/2 per component
        }
        if (a.sine_amp != 0.0f) {                                                  // k_chan_apply's tone, its phase from the absolute index
            const double cyc = (double)n * (double)a.sine_freq / 8000.0;
            float sn, cs; sincosf((float)(6.283185307179586 * (cyc - floor(cyc))), &sn, &cs);
            v.x += a.sine_amp * cs; v.y += a.sine_amp * sn;
        }
        return make_float2(v.x * a.rx_gain, v.y * a.rx_gain);
    };
    const long long n_end = S.n0 + S.n_out, P0 = S.n0 >> 1;
    const long long n_pairs = ((n_end + 1) >> 1) - P0;               // pairs that hold a sample of the piece; the first and the last may hold one
    const bool wide = (((uintptr_t)rx + 8 * (2 * P0 - S.n0)) & 15) == 0;           // the even sample of every pair on a 16-byte boundary
    for (long long q = blockIdx.x * 256 + threadIdx.x; q < n_pairs; q += gridDim.x * 256) {
        const unsigned long long P = (unsigned long long)(P0 + q);
        uint32_t w[4] = { 0u, 0u, 0u, 0u };
        if (!noise && a.seed) philox4x32((uint32_t)P, (uint32_t)b, 0u, (uint32_t)(P >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
        const long long n = 2 * (P0 + q), i = n - S.n0;              // i = -1 for the pair an odd n0 cuts
        const bool has0 = n >= S.n0, has1 = n + 1 < n_end;
        float2 v0 = make_float2(0.0f, 0.0f), v1 = v0;
        if (has0) v0 = sample(n, w[0], w[1]);
        if (has1) v1 = sample(n + 1, w[2], w[3]);
        if (has0 && has1) {
            if (wide) *(f32x4 *)&rx[i] = (f32x4){ v0.x, v0.y, v1.x, v1.y };
            else { rx[i] = v0; rx[i + 1] = v1; }
        } else if (has0) rx[i] = v0;
        else if (has1) rx[i + 1] = v1;
    }
}

extern "C" int rd_launch_chan_piece(const rd_chanp_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_out <= 0) return 0;
    if (a->B > 65535 || (a->noise_mode != 0 && a->noise_mode != 1)) return -1;
    int gx = (a->max_out / 2 + 1 + 255) / 256; if (gx > 32) gx = 32;               // as rd_launch_channel has it
    hipLaunchKernelGGL(k_chan_piece, dim3(gx, a->B), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
