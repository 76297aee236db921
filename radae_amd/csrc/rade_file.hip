// rade_file.hip -- the stored-file receiver past the acquisition, rx.py:107-114 and :223-276 for every stream of a batch at once (include/rade_batch.h, "stored-file
// receiver: rx.py past the acquisition", states the arithmetic, the contract and the error bound): the whole-file filter of rade_batch_bpf_file.  The demodulator and
// the BER alignment behind it (rade_batch_rx_file, rade_batch_ber_align) are the fixed-timing receiver's, rade_irx.hip.
//   k_file_phase   the mixer's phases e^{-j alpha (i + 1)} of one call: double sincos, rounded once to complex64, one table for all streams
//   k_file_bpf     complex_bpf(101, ..).bpf(x) of a whole file: a workgroup of four wavefronts takes RD_FILE_SPAN consecutive outputs of one stream
// The filter.  The FIR is the project's one FIR arithmetic (rade_bpf_fir.h): per chunk of RD_FILE_CHUNK = 1024 outputs the window [100 earlier baseband samples | the
// chunk mixed down] is staged as binary16 planes (bpf_stage_planes in its first-call form, o = 2: a whole file is ONE call of complex_bpf, whose memory is Ntap - 1
// zeros), each wavefront forms one 256-output tile on the matrix cores (bpf_fir_tile), mixes it back up and stores it.  As in k_bpf_fir the loop is built around the
// memory system: the next chunk's samples and phases are requested before this chunk is staged, and the chunk's last 102 baseband samples reach the next chunk through
// LDS.  What is new here is the power-of-two pre-scale: bpf_stage_planes clamps its block exponent to [2^-95, 2^95] (the receiver's samples never leave that range; a
// stored file's may), so the chunk is first multiplied by the power of two that puts the larger of this chunk's and the previous chunk's largest |component| into
// [1, 2), and the outputs by its inverse.  Both are exact, so a stream scaled by a power of two gives the scaled bits of the unscaled one.
// The phases come from a table made once per call ([max n] complex64, 8 bytes per sample of ONE stream: it stays in the L2 / Infinity Cache while every stream reads
// it), not from a double sincos per sample and stream: 2 x 256 x 806,400 double sincos would cost more than the filter's memory traffic.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"
#include "rade_bpf_fir.h"

#define FILE_NT 256
static_assert(RD_FILE_CHUNK == 4 * 256 && FILE_NT == 256, "one 256-output tile per wavefront and chunk");
static_assert(RD_FILE_CHUNK + 102 + 127 <= BPF_NPL, "the chunk's window inside the planes");

__global__ __launch_bounds__(256) void k_file_phase(rd_file_bpf_args a)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_phase) return;
    double sn, cs; sincos(a.alpha * (double)(i + 1), &sn, &cs);
    a.phase[2 * i] = (float)cs; a.phase[2 * i + 1] = (float)-sn;
}

__device__ __forceinline__ float file_absmax(const float2 (&v)[4]) { return fmaxf(fmaxf(fmaxf(fabsf(v[0].x), fabsf(v[0].y)), fmaxf(fabsf(v[1].x), fabsf(v[1].y))), fmaxf(fmaxf(fabsf(v[2].x), fabsf(v[2].y)), fmaxf(fabsf(v[3].x), fabsf(v[3].y)))); }

__global__ __launch_bounds__(FILE_NT, 4) void k_file_bpf(rd_file_bpf_args a)
{
    __shared__ BpfLds pl;
    __shared__ unsigned maxw;
    __shared__ float2 tailbuf[102];
    __shared__ float cmax[FILE_NT / 64];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long n = a.n[b];
    long long sk = (long long)blockIdx.x * RD_FILE_SPAN;          // the workgroup's first output
    if (sk >= n) return;
    const float2 *x = (const float2 *)a.x + (size_t)b * a.x_stride;
    float2 *y = (float2 *)a.y + (size_t)b * a.y_stride;
    const float2 *ph = (const float2 *)a.phase;                   // [n_phase] entries: every index below the span's end exists
    BpfTaps taps; bpf_load_taps(taps, a.bpf16, lane);
    const int i0 = 256 * wave + 16 * (lane & 15) + 4 * (lane >> 4);      // this lane's four outputs inside a chunk
    int nn = (int)min((long long)RD_FILE_CHUNK, n - sk);
    // first round trip: the first chunk's samples (clamped addresses, values dropped afterwards), their phases, and the 102 samples in front of the chunk
    float2 xb[4], pb[4], head = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int q = 0; q < 4; q++) { xb[q] = x[sk + min(tid + 256 * q, nn - 1)]; pb[q] = ph[sk + tid + 256 * q]; }
    if (tid < 102) { const long long q = sk - 102 + tid; if (q >= 0) head = cmul_nc(x[q], ph[q]); }      // what lies in front of the file is complex_bpf's zero memory
    float m = fmaxf(file_absmax(xb), fmaxf(fabsf(head.x), fabsf(head.y)));
    m = wave_max_f32(m);
    if (lane == 0) cmax[wave] = m;
    __syncthreads();
    float mcur = fmaxf(fmaxf(cmax[0], cmax[1]), fmaxf(cmax[2], cmax[3])), mprev = 0.0f;
    for (int c = 0; c < RD_FILE_NCHUNK; c++) {
        // the pre-scale: the power of two that puts the larger of the two chunks' maxima into [1, 2) (the head is part of the previous chunk)
        const int e = (int)((__float_as_uint(fmaxf(mcur, mprev)) >> 23) & 0xffu), ec = e == 0 ? 127 : min(e, 253);
        const float pre = __uint_as_float((unsigned)(254 - ec) << 23), post = __uint_as_float((unsigned)ec << 23);
        float2 raw[4], body[BPF_NQ];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            raw[q] = cmul_nc(xb[q], pb[q]);
            if (tid + 256 * q >= nn) raw[q] = make_float2(0.0f, 0.0f);
            body[q] = make_float2(raw[q].x * pre, raw[q].y * pre);
        }
        body[4] = make_float2(0.0f, 0.0f);
        const float2 hd = make_float2(head.x * pre, head.y * pre);
        float2 po[4];                                             // the phases of this lane's outputs
#pragma unroll
        for (int r = 0; r < 4; r++) po[r] = ph[sk + i0 + r];
        // the next chunk's samples and phases: in flight from here on
        const long long sk2 = sk + RD_FILE_CHUNK;
        const bool more = c + 1 < RD_FILE_NCHUNK && sk2 < n;      // uniform
        const int n2 = more ? (int)min((long long)RD_FILE_CHUNK, n - sk2) : 1;
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; q++) { xb[q] = x[sk2 + min(tid + 256 * q, n2 - 1)]; pb[q] = ph[sk2 + tid + 256 * q]; }
        }
        const float unsc = bpf_stage_planes(&pl, &maxw, tid, hd, body, 2);
        // this chunk's last 102 baseband samples are the next chunk's head (only a full chunk has a next one)
#pragma unroll
        for (int q = 0; q < 4; q++) { const int ti = tid + 256 * q - (nn - 102); if (ti >= 0 && ti < 102) tailbuf[ti] = raw[q]; }
        if (256 * wave < nn) {
            f32x4 re, im;
            bpf_fir_tile(&pl, taps, wave, lane, re, im);
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (i0 + r < nn) {
                    const float2 v = cmul_nc(make_float2(re[r] * unsc, im[r] * unsc), cconj(po[r]));
                    y[sk + i0 + r] = make_float2(v.x * post, v.y * post);
                }
        }
        if (!more) break;
        m = wave_max_f32(file_absmax(xb));                        // (clamped addresses repeat the chunk's last sample: still the chunk's maximum)
        if (lane == 0) cmax[wave] = m;
        __syncthreads();
        if (tid < 102) head = tailbuf[tid];
        mprev = mcur; mcur = fmaxf(fmaxf(cmax[0], cmax[1]), fmaxf(cmax[2], cmax[3]));
        sk = sk2; nn = n2;
    }
}

extern "C" int rd_launch_file_bpf(const rd_file_bpf_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_n <= 0) return 0;
    if (a->n_phase < a->max_n || a->n_phase % RD_FILE_SPAN) return -1;
    hipLaunchKernelGGL(k_file_phase, dim3((unsigned)((a->n_phase + 255) / 256)), dim3(256), 0, (hipStream_t)s, *a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_file_bpf, dim3((a->max_n + RD_FILE_SPAN - 1) / RD_FILE_SPAN, a->B), dim3(FILE_NT), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
