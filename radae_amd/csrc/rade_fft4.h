// rade_fft4.h -- the radix-4 Stockham butterfly that the spectrogram (rade_spec.hip, 2048 points) and the Welch periodogram (rade_psd.hip, 1024 points) share, stated
// once: the padded transform buffer in LDS, the product form and the butterfly with the exact factors 1, -i, -1, i.  include/rade_batch.h states the arithmetic.
#ifndef RADE_FFT4_H
#define RADE_FFT4_H
#include <hip/hip_runtime.h>

// element i of the transform buffer: 4 of padding behind every 16
__device__ __forceinline__ int sp_at(int i) { return i + ((i >> 4) << 2); }
// y w: one rounded product and one fused multiply-add per component
__device__ __forceinline__ float2 sp_tw(float2 y, float2 w) { return make_float2(fmaf(-y.y, w.y, y.x * w.x), fmaf(y.y, w.x, y.x * w.y)); }
__device__ __forceinline__ float2 sp_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 sp_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// one radix-4 butterfly of the stage with stride s = 1 << ls (butterfly t = q + s p): b_m = sum_j a_j (-i)^(j m) by additions alone, then y[q + s (4 p + m)] = b_m t[m p s]
__device__ __forceinline__ void sp_butterfly(float2 *buf, const float2 *tw, const float2 a[4], int t, int ls)
{
    const int s = 1 << ls, q = t & (s - 1), p = t >> ls;
    const float2 e = sp_add(a[0], a[2]), f = sp_add(a[1], a[3]), g = sp_sub(a[0], a[2]), d = sp_sub(a[1], a[3]);
    const float2 b0 = sp_add(e, f), b2 = sp_sub(e, f);
    const float2 b1 = make_float2(g.x + d.y, g.y - d.x), b3 = make_float2(g.x - d.y, g.y + d.x);       // g - i d, g + i d
    const int o = q + ((4 * p) << ls), w = p << ls;
    buf[sp_at(o)] = b0;
    buf[sp_at(o + s)] = sp_tw(b1, tw[w]);
    buf[sp_at(o + 2 * s)] = sp_tw(b2, tw[2 * w]);
    buf[sp_at(o + 3 * s)] = sp_tw(b3, tw[3 * w]);
}
#endif
