// rade_spec.hip -- the spectrogram of rade_batch_specgram (include/rade_batch.h states the arithmetic, the order of every sum and the error bound): plot_specgram.m:6-16 at
// Fs = 8000, a 1280-sample Hann window zero-padded to a 2048-point transform every 160 samples, |X[1..1023]| of every slice, the stream's maximum, the 256-step levels.
//   k_specgram     one workgroup per (run of 8 consecutive slices, stream): the run's 2400 samples are loaded once, then its four slice pairs go through the transform.
//                  By its flags a launch writes the magnitudes, folds them into the stream's maximum and / or writes the levels against a peak that is already known.
// Two passes, because the normaliser is a maximum over the whole recording: pass 1 (magnitudes, maximum), pass 2 (levels).  Pass 2 RECOMPUTES the transforms.  The
// alternative, an engine-owned magnitude buffer that pass 2 reads, would be 5.3 GB at 256 x 806,400 samples; the recomputation is the form built, for the memory and not
// for the time: measured on the MI355X (tools/time_specgram.py, profiles/time_specgram.json) a pass is 3.90 ms at that shape and 4.49 ms when it also stores the 5.3 GB
// of magnitudes, so the buffer form would cost about 4.5 + 1.5 ms where the image alone now costs 10.3 ms.  A caller who has the memory can have that form today: ask for
// mag_dev, then call again with peak_in_host -- or take the levels from the magnitudes on the host, they are an exact function of them.  There is one code path for the
// transform, so the image is the same whether or not mag_dev was asked for.  With peak_in_host one launch writes both outputs.
// Measured: 256 x 80,000 samples (126 k slices) image 1.15 ms, magnitudes 0.64 ms, both 1.32 ms; 256 x 806,400 (1.29 M slices) 10.46 / 5.27 / 11.81 ms; 165 M pair
// transforms per second in a pass without stores, 16 T float32 vector instructions per second (about 97 k per pair).  What bounds it, by count: about 250 KB of LDS
// traffic per pair (five stage round trips, the twiddles, the span) are 41 TB/s, half of what 256 CUs move at 128 bytes per clock, in 8-byte accesses with twelve
// barriers per pair and three workgroups per CU to hide them behind; the vector pipe issues at 40 % of its rate.  The stores are hidden (0.6 ms for 5.3 GB).
// Transform: slices (2m, 2m+1) of a stream are the real and the imaginary part of one 2048-point complex transform (an unpaired last slice: imaginary part +0), a Stockham
// autosort decimation in frequency, five radix-4 stages and one radix-2 stage, whose radix-4 butterflies use the exact factors 1, -i, -1, i (additions only) and whose
// twiddles come from the one table t[m] = e^{-2 pi i m / 2048}.  Stage 1 reads the windowed samples straight from the run's span and skips the 768 zeros; the radix-2
// stage and the separation of the two slices are folded into the magnitude step, which forms bins 1..1023 only.
// LDS: the transform buffer 2048 complex64 with 4 of padding behind every 16 (power-of-two strides of the stages' stores would land on one bank: a stage stores to
// q + s (4 p + m), lanes 16 or 64 elements apart; with the padding the stores of stages 2..5 spread over the banks and those of stage 1 are 32 contiguous bytes per
// lane), the table 16 KB, the span 9.4 KB, the window 5 KB, the levels 1 KB: 51.9 KB, three workgroups of 256 threads per CU.  One buffer, not two: a stage reads its
// four inputs into registers, the workgroup meets, and the results go back to the same buffer (two barriers per stage; a second buffer would cost the third workgroup).
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"
#include "rade_fft4.h"

#define SPEC_WG 256
#define SPEC_N RD_SPEC_NFFT
#define SPEC_WIN RD_SPEC_WIN
#define SPEC_STEP RD_SPEC_STEP
#define SPEC_RUN RD_SPEC_RUN
#define SPEC_SPAN (SPEC_WIN + SPEC_STEP * (SPEC_RUN - 1))
#define SPEC_BUF (SPEC_N + SPEC_N / 4)
static_assert(SPEC_N == 2048 && SPEC_WIN == 5 * 256 && SPEC_WG * 2 == SPEC_N / 4 && SPEC_RUN % 2 == 0, "two butterflies per thread and stage; the pruned first stage; whole pairs per run");
static_assert((SPEC_BUF + SPEC_N) * 8 + (SPEC_SPAN + SPEC_WIN + 256 + 8) * 4 <= 160 * 1024 / 3, "three workgroups per CU");

// how many of T[1..255] pk lie at or below m: the thresholds do not decrease with j (one rounded multiply each), so a search finds the count
__device__ __forceinline__ int sp_level(float m, float pk, const float *lev)
{
    if (pk == 0.0f) return 0;
    int lo = 0, hi = 255;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (m >= lev[mid] * pk) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SPEC_WG) void k_specgram(rd_spec_args a)
{
    __shared__ __attribute__((aligned(16))) float2 buf[SPEC_BUF];
    __shared__ float2 tw[SPEC_N];
    __shared__ float span[SPEC_SPAN], win[SPEC_WIN], lev[256], red[SPEC_WG / 64];
    const int run = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = a.n[b];
    const int n_sl = n > SPEC_WIN ? (n - SPEC_WIN + SPEC_STEP - 1) / SPEC_STEP : 0;        // starts 0, 160, .. while start < n - 1280
    const int s0 = run * SPEC_RUN;
    if (s0 >= n_sl) return;
    const int cnt = min(SPEC_RUN, n_sl - s0);
    const int len = SPEC_WIN + SPEC_STEP * (cnt - 1);                                      // s0 160 + len <= (n_sl - 1) 160 + 1280 < n: inside the stream's samples
    const size_t first = (size_t)b * (size_t)a.x_stride + (size_t)s0 * SPEC_STEP;          // in elements of x
    if (a.fmt == RD_SPEC_S16) {
        const short *x = (const short *)a.x + first;
        for (int i = tid; i < len; i += SPEC_WG) span[i] = a.gain * (float)x[i];           // the rule of k_wire_in
    } else {
        const float *x = (const float *)a.x + 2 * first;                                   // the real parts; the imaginary parts are not read
        for (int i = tid; i < len; i += SPEC_WG) span[i] = x[2 * (size_t)i];
    }
    for (int i = tid; i < SPEC_WIN; i += SPEC_WG) win[i] = a.win[i];
    for (int i = tid; i < SPEC_N; i += SPEC_WG) tw[i] = ((const float2 *)a.tw)[i];
    if (tid < 255) lev[tid] = a.lev[tid];
    const float pk = a.img ? a.peak[b] : 0.0f;
    const int k0 = a.k0, k1 = a.k1, n_bins = k1 - k0 + 1;
    float vmax = 0.0f;
    __syncthreads();
    for (int pr = 0; pr < cnt; pr += 2) {
        const bool two = pr + 1 < cnt;
        const float *xa = span + pr * SPEC_STEP, *xb = xa + SPEC_STEP;
        float2 v[2][4];
        // stage 1 (s = 1): z[i] = (x_a[i] w[i], x_b[i] w[i]) for i < 1280, zeros behind: input j of butterfly t is z[t + 512 j]
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int t = tid + u * SPEC_WG;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = t + 512 * j;
                v[u][j] = make_float2(0.0f, 0.0f);
                if (j < 2 || (j == 2 && i < SPEC_WIN)) { const float w = win[i]; v[u][j] = make_float2(xa[i] * w, two ? xb[i] * w : 0.0f); }
            }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) sp_butterfly(buf, tw, v[u], tid + u * SPEC_WG, 0);
        __syncthreads();
        // stages 2..5 (s = 4, 16, 64, 256)
#pragma unroll
        for (int ls = 2; ls <= 8; ls += 2) {
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int j = 0; j < 4; j++) v[u][j] = buf[sp_at(tid + u * SPEC_WG + 512 * j)];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; u++) sp_butterfly(buf, tw, v[u], tid + u * SPEC_WG, ls);
            __syncthreads();
        }
        // the radix-2 stage, Z[k] = y[k] + y[k + 1024] and Z[2048 - k] = y[1024 - k] - y[2048 - k], the two slices A = Z[k] + conj Z[2048 - k] = 2 X_a[k] and
        // D = Z[k] - conj Z[2048 - k] = 2 i X_b[k], and their magnitudes, for k = 1..1023
        const int sa = s0 + pr;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int k = 1 + tid + c * SPEC_WG;
            if (k < SPEC_N / 2) {
                const float2 zk = sp_add(buf[sp_at(k)], buf[sp_at(k + 1024)]), zn = sp_sub(buf[sp_at(1024 - k)], buf[sp_at(2048 - k)]);
                const float ar = 0.5f * (zk.x + zn.x), ai = 0.5f * (zk.y - zn.y), dr = 0.5f * (zk.x - zn.x), di = 0.5f * (zk.y + zn.y);
                const float ma = sqrtf(fmaf(ar, ar, ai * ai)), mb = sqrtf(fmaf(dr, dr, di * di));
                if (a.do_max) vmax = fmaxf(vmax, two ? fmaxf(ma, mb) : ma);
                if (a.mag) {
                    float *m = a.mag + (size_t)b * (size_t)a.mag_stride + (size_t)sa * 1023 + (k - 1);
                    m[0] = ma;
                    if (two) m[1023] = mb;
                }
                if (a.img && k >= k0 && k <= k1) {
                    unsigned char *g = a.img + (size_t)b * (size_t)a.img_stride + (size_t)sa * n_bins + (k - k0);
                    g[0] = (unsigned char)sp_level(ma, pk, lev);
                    if (two) g[n_bins] = (unsigned char)sp_level(mb, pk, lev);
                }
            }
        }
        __syncthreads();                                                                   // the buffer is free for the next pair
    }
    if (a.do_max) {                                                                        // a maximum does not depend on the order: magnitudes are >= 0, their bits order as integers
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
        if ((tid & 63) == 0) red[tid >> 6] = vmax;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < SPEC_WG / 64; w++) vmax = fmaxf(vmax, red[w]);
            atomicMax((unsigned *)a.peak + b, __float_as_uint(vmax));
        }
    }
}

extern "C" int rd_launch_specgram(const rd_spec_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_slices <= 0) return 0;
    if (!a->x || !a->n || !a->tw || !a->win || !a->lev || !a->peak || (a->fmt != RD_SPEC_C64 && a->fmt != RD_SPEC_S16)) return -1;
    if (a->k0 < 1 || a->k0 > a->k1 || a->k1 > SPEC_N / 2 - 1 || (a->do_max && a->img) || !(a->do_max || a->img || a->mag)) return -1;
    hipLaunchKernelGGL(k_specgram, dim3((a->max_slices + SPEC_RUN - 1) / SPEC_RUN, a->B), dim3(SPEC_WG), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
