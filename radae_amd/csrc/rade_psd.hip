// rade_psd.hip -- the Welch periodogram of rade_batch_psd and the power / peak sums of rade_batch_sigstat (include/rade_batch.h states the arithmetic, the order of every
// sum and the error bound): radae_plots.m:53 (pwelch(rx, [], [], 1024, Fs)) and :62-69 (mean power, PAPR, pilot PAPR) for every stream of a batch.
//   k_psd           one workgroup per (run of 32 consecutive segments, stream): each segment is windowed, zero-padded to 1024 points and transformed in LDS, and its
//                   |X[k]|^2 is added to the run's sums, which stay in registers (4 bins per thread) until the run's one row of 1024 floats is stored.
//   k_psd_fold      one thread per (bin, stream): the stream's rows in ascending order in double, one multiply by 1 / (n_seg Fs sum w^2), one rounding.
//   k_sigstat       one workgroup per (chunk of 8192 consecutive samples, stream): |x|^2 as fma(re, re, im im), summed in double and folded into a float32 maximum, for
//                   all samples and for those below `head`.
//   k_sigstat_fold  one thread per stream: the chunks in ascending order.
// Transform: a Stockham autosort decimation in frequency of 1024 = 4^5 points, five radix-4 stages of 256 butterflies, one butterfly per thread and stage; the butterflies
// and the padded LDS buffer are the spectrogram's (rade_fft4.h); the twiddles come from the one table t[m] = e^{-2 pi i m / 1024}.  There is no radix-2 stage: the fifth
// stage leaves X[k] at element k.  Stage 1 reads the samples straight from the stream (each 8-byte sample of a segment once, 2 KB per wavefront and load; neighbouring
// segments overlap in the cache) and skips the inputs i >= win, which are padding zeros.
// LDS: the transform buffer 1024 complex64 with 4 of padding behind every 16 (10 KB), the table 8 KB, the window 4 KB: 22 KB, seven workgroups of 256 threads per CU.
// One buffer, two barriers per stage, as in rade_spec.hip; ten barriers and one more behind the accumulation per segment.
// Measured on the MI355X (tools/time_psd.py, profiles/time_psd.json; host clock around the synchronising call): 256 x 80,000 samples (39,680 transforms) 0.160 ms for the
// spectrum and 0.149 ms for the sums; 256 x 806,400 (402,944 transforms) 0.98 / 0.473 ms, 411 M transforms per second; the device's copy of the same input bytes 0.057 /
// 0.642 ms.  The spectrogram's magnitude pass does 645 k 2048-point pair transforms in 5.27 ms: this call is not slower than that pass, by count or by the clock.
// Runs of 32: the partial rows of 256 x 806,400 samples at step 512 are 50 per stream, 52 MB in all, written once and read once; a stream of one run costs one row.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"
#include "rade_fft4.h"

#define PSD_WG 256
#define PSD_N RD_PSD_NFFT
#define PSD_RUN RD_PSD_RUN
#define PSD_BUF (PSD_N + PSD_N / 4)
#define STAT_WG 256
static_assert(PSD_N == 1024 && PSD_WG == PSD_N / 4, "one butterfly per thread and stage; four bins per thread");
static_assert(RD_STAT_CHUNK % STAT_WG == 0, "whole rounds of the workgroup per chunk");

// sample i of a stream whose first element is x: complex64 as it is, int16 by the rule of k_wire_in (gain (float)s, +0)
__device__ __forceinline__ float2 psd_sample(const void *x, int fmt, float gain, size_t i)
{
    if (fmt == RD_SPEC_S16) return make_float2(gain * (float)((const short *)x)[i], 0.0f);
    return ((const float2 *)x)[i];
}
__device__ __forceinline__ const void *psd_row(const void *x, int fmt, size_t first) { return fmt == RD_SPEC_S16 ? (const void *)((const short *)x + first) : (const void *)((const float2 *)x + first); }

__global__ __launch_bounds__(PSD_WG) void k_psd(rd_psd_args a)
{
    __shared__ __attribute__((aligned(16))) float2 buf[PSD_BUF];
    __shared__ float2 tw[PSD_N];
    __shared__ float win[PSD_N];
    const int run = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int n = a.n[b], W = a.win_len, step = a.step;
    const int n_seg = n >= W ? (n - W) / step + 1 : 0;                                     // starts 0, step, .. while start + win <= n
    const int s0 = run * PSD_RUN;
    if (s0 >= n_seg) return;
    const int cnt = min(PSD_RUN, n_seg - s0);
    for (int i = tid; i < W; i += PSD_WG) win[i] = a.win[i];
    for (int i = tid; i < PSD_N; i += PSD_WG) tw[i] = ((const float2 *)a.tw)[i];
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    __syncthreads();
    for (int r = 0; r < cnt; r++) {
        // (s0 + r) step + win <= (n_seg - 1) step + win <= n: inside the stream's samples
        const void *x = psd_row(a.x, a.fmt, (size_t)b * (size_t)a.x_stride + (size_t)(s0 + r) * (size_t)step);
        float2 v[4];
        // stage 1 (s = 1): z[i] = x[i] w[i] for i < win, zeros behind: input j of butterfly t is z[t + 256 j]
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = tid + 256 * j;
            v[j] = make_float2(0.0f, 0.0f);
            if (i < W) { const float w = win[i]; const float2 s = psd_sample(x, a.fmt, a.gain, (size_t)i); v[j] = make_float2(s.x * w, s.y * w); }
        }
        sp_butterfly(buf, tw, v, tid, 0);
        __syncthreads();
        // stages 2..5 (s = 4, 16, 64, 256)
#pragma unroll
        for (int ls = 2; ls <= 8; ls += 2) {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = buf[sp_at(tid + 256 * j)];
            __syncthreads();
            sp_butterfly(buf, tw, v, tid, ls);
            __syncthreads();
        }
        // X[k] is element k: the segment joins the run's sums in ascending segment order
#pragma unroll
        for (int c = 0; c < 4; c++) { const float2 X = buf[sp_at(tid + c * PSD_WG)]; acc[c] += fmaf(X.x, X.x, X.y * X.y); }
        __syncthreads();                                                                   // the buffer is free for the next segment
    }
    float *row = a.part + ((size_t)b * (size_t)a.max_runs + (size_t)run) * PSD_N;
#pragma unroll
    for (int c = 0; c < 4; c++) row[tid + c * PSD_WG] = acc[c];
}

__global__ __launch_bounds__(PSD_WG) void k_psd_fold(rd_psd_args a)
{
    const int k = blockIdx.x * PSD_WG + threadIdx.x, b = blockIdx.y;
    const int n = a.n[b];
    const int n_seg = n >= a.win_len ? (n - a.win_len) / a.step + 1 : 0;
    if (!n_seg) return;
    const int n_runs = (n_seg + PSD_RUN - 1) / PSD_RUN;                                    // <= max_runs: the rows k_psd wrote
    const float *row = a.part + (size_t)b * (size_t)a.max_runs * PSD_N + k;
    double s = 0.0;
    for (int r = 0; r < n_runs; r++) s += (double)row[(size_t)r * PSD_N];
    a.psd[(size_t)b * (size_t)a.psd_stride + k] = (float)(s * a.scale[b]);
}

__global__ __launch_bounds__(STAT_WG) void k_sigstat(rd_stat_args a)
{
    __shared__ double red[4][STAT_WG / 64];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long long n = a.n[b], base = (long long)c * RD_STAT_CHUNK;
    if (base >= n) return;
    const long long hn = n < a.head ? n : a.head;
    const void *x = psd_row(a.x, a.fmt, (size_t)b * (size_t)a.x_stride);
    double s = 0.0, hs = 0.0;
    float pk = 0.0f, hpk = 0.0f;
    for (int j = 0; j < RD_STAT_CHUNK / STAT_WG; j++) {                                    // a thread's samples in ascending order
        const long long i = base + tid + (long long)j * STAT_WG;
        if (i < n) {
            const float2 v = psd_sample(x, a.fmt, a.gain, (size_t)i);
            const float t = fmaf(v.x, v.x, v.y * v.y);
            s += (double)t; pk = fmaxf(pk, t);
            if (i < hn) { hs += (double)t; hpk = fmaxf(hpk, t); }
        }
    }
    s = wave_sum_f64(s); hs = wave_sum_f64(hs); pk = wave_max_f32(pk); hpk = wave_max_f32(hpk);
    if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = (double)pk; red[2][tid >> 6] = hs; red[3][tid >> 6] = (double)hpk; }
    __syncthreads();
    if (tid == 0) {
        double *p = a.part + ((size_t)b * (size_t)a.max_chunks + (size_t)c) * 4;
        p[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        p[1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
        p[2] = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
        p[3] = fmax(fmax(red[3][0], red[3][1]), fmax(red[3][2], red[3][3]));
    }
}

__global__ __launch_bounds__(64) void k_sigstat_fold(rd_stat_args a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const long long n = a.n[b];
    const int n_ch = (int)((n + RD_STAT_CHUNK - 1) / RD_STAT_CHUNK);                       // <= max_chunks: the records k_sigstat wrote
    double s = 0.0, pk = 0.0, hs = 0.0, hpk = 0.0;
    for (int c = 0; c < n_ch; c++) {
        const double *p = a.part + ((size_t)b * (size_t)a.max_chunks + (size_t)c) * 4;
        s += p[0]; pk = fmax(pk, p[1]); hs += p[2]; hpk = fmax(hpk, p[3]);
    }
    a.out[4 * b] = s; a.out[4 * b + 1] = pk; a.out[4 * b + 2] = hs; a.out[4 * b + 3] = hpk;
}

extern "C" int rd_launch_psd(const rd_psd_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_runs <= 0) return 0;
    if (!a->x || !a->n || !a->scale || !a->tw || !a->win || !a->part || !a->psd || (a->fmt != RD_SPEC_C64 && a->fmt != RD_SPEC_S16)) return -1;
    if (a->win_len < RD_PSD_WIN_MIN || a->win_len > PSD_N || a->step < 1 || a->step > a->win_len || a->psd_stride < PSD_N) return -1;
    hipLaunchKernelGGL(k_psd, dim3(a->max_runs, a->B), dim3(PSD_WG), 0, (hipStream_t)s, *a);
    hipLaunchKernelGGL(k_psd_fold, dim3(PSD_N / PSD_WG, a->B), dim3(PSD_WG), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_sigstat(const rd_stat_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    if (!a->x || !a->n || !a->part || !a->out || a->head < 0 || a->max_chunks < 0 || (a->fmt != RD_SPEC_C64 && a->fmt != RD_SPEC_S16)) return -1;
    if (a->max_chunks) hipLaunchKernelGGL(k_sigstat, dim3(a->max_chunks, a->B), dim3(STAT_WG), 0, (hipStream_t)s, *a);
    hipLaunchKernelGGL(k_sigstat_fold, dim3((a->B + 63) / 64), dim3(64), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
