// rade_clk.hip -- sample-clock offset: the fractional resampler of rade_batch_resample (include/rade_batch.h states the arithmetic; dsp.py:564-575 is its linear mode).
//   k_clk_resample   one workgroup per (tiles of RD_CLK_TILE consecutive outputs, stream); a workgroup walks its stream's tiles blockIdx.x, + gridDim.x, ...
// Positions are Q32.32 integers, pos_q = t0_q + n step_q, so an output depends on (t0, ppm, n) and the input alone: no state, and the same bits however a stream is cut
// into calls, tiles or threads (every output is one thread's sum over j = 0..31 in that order, one float32 accumulator per component).
// LDS: the taps once per workgroup, rows CLK_ROW = 36 floats apart -- a thread reads four taps of rows p and p + 1 as 16-byte words; neighbouring outputs differ in mu by the
// fractional step, so the lanes of a wavefront read one row (a broadcast) when |ppm| is small and consecutive rows otherwise, and 36 p mod 64 puts 16 consecutive rows on
// 16 different groups of four banks (a stride of 32 would put every row on the same four) -- and the tile's input window, (cnt - 1) step + 33 samples, zeros where
// the window leaves [in_base, in_base + n_in).  The window is read by consecutive lanes at consecutive samples (8-byte words).
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"

#define CLK_WG 256
#define CLK_ROW 36                           // floats between the rows of the taps in LDS
#define CLK_WIN 1120                         // samples of a tile's window: (RD_CLK_TILE - 1) * 1.05 + 33 < 1108 (the entry refuses |ppm| > 50 000)
static_assert((RD_CLK_TILE - 1) * 1.05 + RD_CLK_TAPS + 1 <= CLK_WIN, "a tile's window fits for every step the entry accepts");
static_assert(RD_CLK_TAPS == 32 && RD_CLK_PHASES == 256, "p = mu >> 24, 32 taps as eight 16-byte words");

__global__ __launch_bounds__(CLK_WG) void k_clk_resample(rd_clk_args a)
{
    __shared__ __attribute__((aligned(16))) float T[(RD_CLK_PHASES + 1) * CLK_ROW];
    __shared__ float2 win[CLK_WIN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const rd_clk_stream S = a.ps[b];
    const int n_tiles = (S.n_out + RD_CLK_TILE - 1) / RD_CLK_TILE;
    if ((int)blockIdx.x >= n_tiles) return;
    const float2 *x = (const float2 *)a.x + (size_t)b * a.x_stride;
    float2 *y = (float2 *)a.y + (size_t)b * a.y_stride;
    if (a.mode == 0)
        for (int i = tid; i < (RD_CLK_PHASES + 1) * RD_CLK_TAPS; i += CLK_WG) T[(i >> 5) * CLK_ROW + (i & 31)] = a.taps[i];
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int o0 = tile * RD_CLK_TILE, cnt = min(RD_CLK_TILE, S.n_out - o0);
        const long long pos_a = S.t0_q + (S.n0 + o0) * S.step_q;                 // position of the tile's first output
        const long long i_lo = (pos_a >> 32) - 15;                               // first sample of its window
        const int len = min((int)(((pos_a + (cnt - 1) * S.step_q) >> 32) + 16 - i_lo) + 1, CLK_WIN);
        __syncthreads();                                                         // the previous tile's window has been read
        for (int k = tid; k < len; k += CLK_WG) {
            const long long g = i_lo + k - S.in_base;                            // index into the stream's row: read inside [0, n_in) only
            win[k] = (g >= 0 && g < S.n_in) ? x[g] : make_float2(0.0f, 0.0f);
        }
        __syncthreads();
        for (int o = tid; o < cnt; o += CLK_WG) {
            const long long pos = pos_a + o * S.step_q;
            const unsigned mu = (unsigned)pos;
            const float2 *xw = win + (int)((pos >> 32) - 15 - i_lo);              // x[i - 15]
            float re, im;
            if (a.mode == 0) {
                const int p = mu >> 24;
                const float w = (float)(mu & 0xffffffu) * (1.0f / 16777216.0f);
                const f32x4 *r0 = (const f32x4 *)(T + p * CLK_ROW), *r1 = (const f32x4 *)(T + (p + 1) * CLK_ROW);
                re = 0.0f; im = 0.0f;
#pragma unroll
                for (int q = 0; q < RD_CLK_TAPS / 4; q++) {
                    const f32x4 t0 = r0[q], t1 = r1[q];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float c = fmaf(w, t1[e] - t0[e], t0[e]);
                        const float2 v = xw[4 * q + e];
                        re = fmaf(c, v.x, re); im = fmaf(c, v.y, im);
                    }
                }
            } else {
                const float f = (float)mu * (1.0f / 4294967296.0f);
                const float2 v0 = xw[15], v1 = xw[16];
                re = fmaf(f, v1.x, (1.0f - f) * v0.x); im = fmaf(f, v1.y, (1.0f - f) * v0.y);
            }
            y[o0 + o] = make_float2(re, im);                                     // one 8-byte store per sample: any y_stride, any parity of n_out
        }
    }
}

extern "C" int rd_launch_clk_resample(const rd_clk_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_out <= 0) return 0;
    if (a->mode != 0 && a->mode != 1) return -1;
    const int n_tiles = (a->max_out + RD_CLK_TILE - 1) / RD_CLK_TILE;
    int gx = 2048 / a->B; if (gx < 1) gx = 1;                                    // about 2048 workgroups per launch: the taps are loaded once per workgroup, not per tile
    if (gx > n_tiles) gx = n_tiles;
    hipLaunchKernelGGL(k_clk_resample, dim3(gx, a->B), dim3(CLK_WG), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
