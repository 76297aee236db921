// rade_wire.hip -- the sound-card wire: int16 in and out of the batch engine (rade_batch_wire_in / rade_batch_wire_out, include/rade_batch.h;
// int16tof32.py:40-50 with --zeropad, f32toint16.py:42-54 with --real).
//   k_wire_in<IQ>          int16 -> complex64, one workgroup per (chunk, stream): chunk ch of a stream takes the 16-byte words ch * 256 + tid, + n_ch * 256, ...
//   k_wire_out<IQ, METER>  complex64 -> int16 with saturation; METER: the chunk's peak, sum of squares, clipped and NaN counts
//   k_wire_meters          per stream: the chunks' partials in their fixed order
// Both kernels see a row as its int16 ELEMENTS (n of them in real mode, 2 n in IQ mode: a component is an element) and the float32 values that belong to them
// (real: two per element, (I, the Q that is written as +0 or read and dropped); IQ: one).  A row is cut where its int16 side crosses 16-byte boundaries:
//     head   the elements in front of the first boundary (0..7, all of a row that reaches none)          by element, chunk 0
//     body   words of 8 elements: one 16-byte access on the int16 side, and 16 (real) or 8 (IQ) consecutive floats on the other side, moved as 16-byte words when
//            the first of them is 16-byte aligned, else as 8-byte words (always possible in real mode: a sample is 8 bytes), else by float (IQ with an odd head)
//     tail   what is left behind the last whole word (0..7)                                               by element, chunk 0
// The int16 side decides the cut because it is the side that has most to lose: a 2-byte access moves an eighth of a 16-byte one per instruction, an 8-byte one half.
// Nothing outside [row, row + n) of either buffer is read or written, and there is no state: a call is a pure function of its arguments.
// Meters: every thread adds v^2 of its components as doubles (the product of two float32 is exact in double) in the order of its words, the 64 lanes of a wavefront
// are added by wave_sum_f64's tree, the four wavefronts and then the chunks in their order.  No atomics: the same call gives the same bits.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"

#define WIRE_WG 256

// NF consecutive floats at p, in the widest words the alignment class al of p (16, 8 or 4: uniform over a row) allows
template <int NF> __device__ __forceinline__ void wire_ld(const float *p, int al, float (&v)[NF])
{
    if (al == 16) {
#pragma unroll
        for (int q = 0; q < NF / 4; q++) { const f32x4 t = ((const f32x4 *)p)[q]; v[4 * q] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3]; }
    } else if (al == 8) {
#pragma unroll
        for (int q = 0; q < NF / 2; q++) { const f32x2 t = ((const f32x2 *)p)[q]; v[2 * q] = t[0]; v[2 * q + 1] = t[1]; }
    } else {
#pragma unroll
        for (int q = 0; q < NF; q++) v[q] = p[q];
    }
}
template <int NF> __device__ __forceinline__ void wire_st(float *p, int al, const float (&v)[NF])
{
    if (al == 16) {
#pragma unroll
        for (int q = 0; q < NF / 4; q++) ((f32x4 *)p)[q] = (f32x4){ v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3] };
    } else if (al == 8) {
#pragma unroll
        for (int q = 0; q < NF / 2; q++) ((f32x2 *)p)[q] = (f32x2){ v[2 * q], v[2 * q + 1] };
    } else {
#pragma unroll
        for (int q = 0; q < NF; q++) p[q] = v[q];
    }
}
__device__ __forceinline__ int wire_align(const void *p) { return ((uintptr_t)p & 15) == 0 ? 16 : ((uintptr_t)p & 7) == 0 ? 8 : 4; }
// the cut of a row of E int16 elements at address p: the head's length; the body is (E - head) >> 3 words
__device__ __forceinline__ int wire_head(const void *p, long long E) { const int h = (int)((16 - ((uintptr_t)p & 15)) & 15) >> 1; return E < h ? (int)E : h; }

template <int IQ> __global__ __launch_bounds__(WIRE_WG) void k_wire_in(rd_wire_args a)
{
    constexpr int FPE = IQ ? 1 : 2;                  // floats per int16 element
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long E = (long long)a.n[b] << IQ;
    const short *in = (const short *)a.i16 + (size_t)b * a.i16_stride;
    float *out = (float *)a.c64 + 2 * (size_t)b * a.c64_stride;
    const float gain = a.k;
    const int h = wire_head(in, E);
    const int n_words = (int)((E - h) >> 3);
    auto one = [&](long long c) {                    // element c on its own
        const float v = gain * (float)in[c];
        if constexpr (IQ) out[c] = v; else *(float2 *)(out + 2 * c) = make_float2(v, 0.0f);
    };
    if (blockIdx.x == 0 && tid < 8) {
        if (tid < h) one(tid);
        const long long c = h + 8LL * n_words + tid;
        if (c < E) one(c);
    }
    const u32x4 *w = (const u32x4 *)(in + h);
    float *og = out + FPE * h;
    const int al = wire_align(og);
    for (int g = blockIdx.x * WIRE_WG + tid; g < n_words; g += gridDim.x * WIRE_WG) {
        const u32x4 x = w[g];
        float v[8 * FPE];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float lo = gain * (float)(short)(x[e] & 0xffffu), hi = gain * (float)(short)(x[e] >> 16);
            if constexpr (IQ) { v[2 * e] = lo; v[2 * e + 1] = hi; }
            else { v[FPE * 2 * e] = lo; v[FPE * 2 * e + 1] = 0.0f; v[FPE * (2 * e + 1)] = hi; v[FPE * (2 * e + 1) + 1] = 0.0f; }
        }
        wire_st<8 * FPE>(og + (size_t)g * (8 * FPE), al, v);
    }
}

struct wire_meter { double s2; float peak; int clipped, nan; };
// v = x * scale rounded once to float32, truncated toward zero; what does not fit saturates, NaN gives 0.  A NaN component is counted and adds to neither the peak
// nor the sum; a clipped one is counted and metered as the value it would have had (+-inf included).
template <bool METER> __device__ __forceinline__ int wire_cvt(float x, float scale, wire_meter &m)
{
    const float v = x * scale;
    int r;
    if (v != v) { if (METER) m.nan++; return 0; }
    if (v >= 32768.0f) { r = 32767; if (METER) m.clipped++; }
    else if (v <= -32769.0f) { r = -32768; if (METER) m.clipped++; }
    else r = (int)v;
    if (METER) { m.peak = fmaxf(m.peak, fabsf(v)); m.s2 += (double)v * (double)v; }
    return r;
}

template <int IQ, bool METER> __global__ __launch_bounds__(WIRE_WG) void k_wire_out(rd_wire_args a)
{
    constexpr int FPE = IQ ? 1 : 2;
    __shared__ double red[4][WIRE_WG / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long long E = (long long)a.n[b] << IQ;
    short *o = (short *)a.i16 + (size_t)b * a.i16_stride;
    const float *x = (const float *)a.c64 + 2 * (size_t)b * a.c64_stride;
    const float scale = a.k;
    const int h = wire_head(o, E);
    const int n_words = (int)((E - h) >> 3);
    wire_meter m = { 0.0, 0.0f, 0, 0 };
    if (blockIdx.x == 0 && tid < 8) {
        if (tid < h) o[tid] = (short)wire_cvt<METER>(x[FPE * tid], scale, m);
        const long long c = h + 8LL * n_words + tid;
        if (c < E) o[c] = (short)wire_cvt<METER>(x[FPE * c], scale, m);
    }
    u32x4 *w = (u32x4 *)(o + h);
    const float *xg = x + FPE * h;
    const int al = wire_align(xg);
    for (int g = blockIdx.x * WIRE_WG + tid; g < n_words; g += gridDim.x * WIRE_WG) {
        float v[8 * FPE];
        wire_ld<8 * FPE>(xg + (size_t)g * (8 * FPE), al, v);
        u32x4 y;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int lo = wire_cvt<METER>(v[FPE * 2 * e], scale, m), hi = wire_cvt<METER>(v[FPE * (2 * e + 1)], scale, m);
            y[e] = ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16);
        }
        w[g] = y;
    }
    if (METER) {                                     // every thread of every chunk arrives here: a chunk without work leaves zeros
        const double s2 = wave_sum_f64(m.s2), nc = wave_sum_f64((double)m.clipped), nn = wave_sum_f64((double)m.nan);
        const float pk = wave_max_f32(m.peak);
        if ((tid & 63) == 0) { red[0][tid >> 6] = (double)pk; red[1][tid >> 6] = s2; red[2][tid >> 6] = nc; red[3][tid >> 6] = nn; }
        __syncthreads();
        if (tid == 0) {
            double *p = a.part + ((size_t)b * gridDim.x + blockIdx.x) * 4;
            p[0] = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
            for (int k = 1; k < 4; k++) p[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
        }
    }
}

__global__ __launch_bounds__(64) void k_wire_meters(const double *part, int n_ch, double *meters, int B)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double pk = 0.0, s2 = 0.0, nc = 0.0, nn = 0.0;
    for (int c = 0; c < n_ch; c++) { const double *p = part + ((size_t)b * n_ch + c) * 4; pk = fmax(pk, p[0]); s2 += p[1]; nc += p[2]; nn += p[3]; }
    meters[4 * b] = pk; meters[4 * b + 1] = s2; meters[4 * b + 2] = nc; meters[4 * b + 3] = nn;
}

extern "C" int rd_launch_wire_in(const rd_wire_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->n_ch <= 0) return 0;
    if (a->mode == 0) hipLaunchKernelGGL(k_wire_in<0>, dim3(a->n_ch, a->B), dim3(WIRE_WG), 0, (hipStream_t)s, *a);
    else if (a->mode == 1) hipLaunchKernelGGL(k_wire_in<1>, dim3(a->n_ch, a->B), dim3(WIRE_WG), 0, (hipStream_t)s, *a);
    else return -1;
    return (int)hipGetLastError();
}

extern "C" int rd_launch_wire_out(const rd_wire_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->n_ch <= 0) return 0;
    if (a->mode != 0 && a->mode != 1) return -1;
    const dim3 grid(a->n_ch, a->B), wg(WIRE_WG);
    if (a->meters) {
        if (!a->part) return -1;
        if (a->mode == 0) hipLaunchKernelGGL((k_wire_out<0, true>), grid, wg, 0, (hipStream_t)s, *a);
        else hipLaunchKernelGGL((k_wire_out<1, true>), grid, wg, 0, (hipStream_t)s, *a);
        hipLaunchKernelGGL(k_wire_meters, dim3((a->B + 63) / 64), dim3(64), 0, (hipStream_t)s, (const double *)a->part, a->n_ch, a->meters, a->B);
    } else {
        if (a->mode == 0) hipLaunchKernelGGL((k_wire_out<0, false>), grid, wg, 0, (hipStream_t)s, *a);
        else hipLaunchKernelGGL((k_wire_out<1, false>), grid, wg, 0, (hipStream_t)s, *a);
    }
    return (int)hipGetLastError();
}
