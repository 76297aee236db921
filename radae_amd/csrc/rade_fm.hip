// rade_fm.hip -- the analog FM modulator and demodulator of rade_batch_fm_mod / rade_batch_fm_demod (include/rade_batch.h states the arithmetic): fm.m:74-94
// (analog_fm_mod, with the noise of :171 / :316-322) and fm.m:97-126 (analog_fm_demod), every stream of a batch in one call.  No device state, pieces equal the whole.
//   k_fm_sums<FMT>      one workgroup per (tile of RD_FM_TILE samples, stream): the sum mod 2^32 of the tile's NCO increments
//   k_fm_tile_scan      one workgroup per stream: the tile sums become the phase in front of each tile (exclusive scan, carried from phase0); the final phase
//   k_fm_mod<FMT>       one workgroup per (tile, stream): the scan inside the tile from the phase in front of it, the phasor, the noise, the store
//   k_fm_demod          one workgroup per (tiles of RD_FM_TILE outputs, stream), walking its stream's tiles blockIdx.x, + gridDim.x, ...: mix, input FIR, discriminator,
//                       output FIR, all between LDS arrays
// The three modulator kernels are plain launches in stream order: no workgroup waits for another one (no look-back chain, no flag).  The phase is a 32-bit integer and its
// sums are associative, so the order of the scan leaves no trace in the bits: tiles, workgroups, threads and calls can cut a stream anywhere.
// Phasor (fm_cis, the modulator's carrier and the demodulator's mixer alike): the top two bits of the phase pick the quadrant by swap and negate (exact); the low 30 bits r
// are folded to r' = min(r, 2^30 - r) <= 2^29 (the octant: exact, sine and cosine swapped), the angle (pi / 2) 2^-30 r' is formed in double and rounded once to float32,
// and sincosf of that angle in [0, pi / 4] gives the two components.  r = 0 gives (1, 0) exactly.
// Demodulator LDS (static, 49,280 bytes: three workgroups per CU): the mixed window xm (complex), the filtered baseband bb (complex), the discriminator values (float, in
// xm's place once bb is complete), and the two tap tables.  Every thread forms FOUR consecutive outputs of a FIR at a time: a tap then costs one new sample from LDS
// for four (complex: eight) multiply-adds, the four running samples rotate through registers.  So that lanes four samples apart read consecutive words, each array is
// stored de-interleaved by (index mod 4): sample i at plane i & 3, word i >> 2; the plane and word offset of a tap are the same for all lanes.  The four taps of an
// unrolled step are one 16-byte broadcast read.  Each output is one accumulator per component and fused multiply-adds in the order k = 0..N-1, whichever thread forms it.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"

#define FM_WG 256
#define FM_PER (RD_FM_TILE / FM_WG)                                   // samples per thread of a modulator tile
static_assert(RD_FM_TILE % (4 * FM_WG) == 0, "whole groups of four per thread");

// ---- shared by both directions -----------------------------------------------------------------------------------------------------------------------------------
// (fm_cis, the phasor of a 32-bit phase: rade_devutil.h -- the channel pieces of rade_chanp.hip rotate by it too)

// inclusive scan over the workgroup's 256 threads (integers mod 2^32); ws: 4 words of LDS; total: the sum over all threads
__device__ __forceinline__ unsigned fm_block_scan(unsigned v, unsigned *ws, unsigned &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    if (lane == 63) ws[wv] = v;
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < FM_WG / 64; w++) { const unsigned s = ws[w]; if (w < wv) off += s; tot += s; }
    __syncthreads();                                                  // ws may be written again
    total = tot;
    return v + off;
}

// ---- modulator ---------------------------------------------------------------------------------------------------------------------------------------------------
// inc = (uint32)(int64) rint(fma(m, kd, kc)); a sample that is not finite or lies outside +-2^16 modulates as 0.  |m kd + kc| < 2^48: the conversions are exact.
__device__ __forceinline__ unsigned fm_inc(float m, double kd, double kc)
{
    if (!(fabsf(m) <= 65536.0f)) m = 0.0f;
    return (unsigned)(long long)rint(fma((double)m, kd, kc));
}
template <int FMT> __device__ __forceinline__ float fm_sample(const void *row, int i)
{
    return FMT == 0 ? ((const float *)row)[i] : ((const float2 *)row)[i].x;
}
template <int FMT> __device__ __forceinline__ const void *fm_row(const rd_fm_mod_args &a, int b)
{
    return FMT == 0 ? (const void *)((const float *)a.m + (size_t)b * a.m_stride) : (const void *)((const float2 *)a.m + (size_t)b * a.m_stride);
}

template <int FMT> __global__ __launch_bounds__(FM_WG) void k_fm_sums(rd_fm_mod_args a)
{
    __shared__ unsigned ws[FM_WG / 64];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const int n = a.ps[b].n, i0 = tile * RD_FM_TILE;
    if (i0 >= n) return;
    const void *row = fm_row<FMT>(a, b);
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < FM_PER; j++) { const int i = i0 + j * FM_WG + tid; if (i < n) v += fm_inc(fm_sample<FMT>(row, i), a.kd, a.kc); }
    unsigned total;
    (void)fm_block_scan(v, ws, total);
    if (tid == 0) a.tsum[(size_t)b * a.n_tiles + tile] = total;
}

__global__ __launch_bounds__(FM_WG) void k_fm_tile_scan(rd_fm_mod_args a)
{
    __shared__ unsigned ws[FM_WG / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nt = (a.ps[b].n + RD_FM_TILE - 1) / RD_FM_TILE;
    unsigned *t = a.tsum + (size_t)b * a.n_tiles;
    unsigned carry = a.ps[b].ph0;
    for (int c0 = 0; c0 < nt; c0 += FM_WG) {                          // (nt is the same for every thread: the barriers inside the scan are met by all)
        const int i = c0 + tid;
        const unsigned v = i < nt ? t[i] : 0u;
        unsigned total;
        const unsigned incl = fm_block_scan(v, ws, total);
        if (i < nt) t[i] = carry + (incl - v);                        // the phase in front of tile i
        carry += total;
    }
    if (tid == 0) a.ph_end[b] = carry;
}

// the noise of one sample, unit variance per component: words 0-1 of counter (p, b, 3, p >> 32) for the even sample of pair p = abs >> 1, words 2-3 for the odd one
__device__ __forceinline__ float2 fm_gauss(long long abs_i, int b, unsigned long long seed)
{
    uint32_t r[4];
    const unsigned long long p = (unsigned long long)abs_i >> 1;
    philox4x32((uint32_t)p, (uint32_t)b, 3u, (uint32_t)(p >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return (abs_i & 1) ? gauss_pair(r[2], r[3]) : gauss_pair(r[0], r[1]);
}
// tx + s nz with the product and the sum rounded each on its own: what adding the noise by hand in float32 gives
__device__ __forceinline__ float fm_add_nc(float tx, float s, float nz)
{
#pragma clang fp contract(off)
    const float p = s * nz;
    return tx + p;
}

template <int FMT> __global__ __launch_bounds__(FM_WG) void k_fm_mod(rd_fm_mod_args a)
{
    // the tile's increments, then its phases; read four ways: sample i at word i + (i >> 5) (a thread's FM_PER consecutive words then fall on banks of their own)
    __shared__ unsigned ph[RD_FM_TILE + RD_FM_TILE / 32];
    __shared__ unsigned ws[FM_WG / 64];
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    const rd_fm_stream S = a.ps[b];
    const int n = S.n, i0 = tile * RD_FM_TILE;
    if (i0 >= n) return;
    const void *row = fm_row<FMT>(a, b);
#pragma unroll
    for (int j = 0; j < FM_PER; j++) {
        const int l = j * FM_WG + tid, i = i0 + l;
        ph[l + (l >> 5)] = i < n ? fm_inc(fm_sample<FMT>(row, i), a.kd, a.kc) : 0u;
    }
    __syncthreads();
    unsigned loc[FM_PER], run = 0;
#pragma unroll
    for (int k = 0; k < FM_PER; k++) { const int l = tid * FM_PER + k; run += ph[l + (l >> 5)]; loc[k] = run; }
    unsigned total;
    const unsigned base = a.tsum[(size_t)b * a.n_tiles + tile] + (fm_block_scan(run, ws, total) - run);
#pragma unroll
    for (int k = 0; k < FM_PER; k++) { const int l = tid * FM_PER + k; ph[l + (l >> 5)] = base + loc[k]; }      // inclusive: fm.m adds before it takes the exponential
    __syncthreads();
    float2 *y = (float2 *)a.y + (size_t)b * a.y_stride;
    const float2 *nz = a.noise ? (const float2 *)a.noise + (size_t)b * a.noise_stride : nullptr;
#pragma unroll
    for (int j = 0; j < FM_PER; j++) {
        const int l = j * FM_WG + tid, i = i0 + l;
        if (i >= n) break;
        float2 v = fm_cis(ph[l + (l >> 5)]);
        if (a.noise_on) {
            const float2 g = nz ? nz[i] : fm_gauss(S.n0 + i, b, a.seed);
            v.x = fm_add_nc(v.x, a.sg, g.x);
            if (!a.real_out) v.y = fm_add_nc(v.y, a.sg, g.y);
        }
        if (a.real_out) v.y = 0.0f;
        y[i] = v;
    }
}

template <int FMT> static int fm_mod_launch(const rd_fm_mod_args *a, hipStream_t s)
{
    const dim3 grid(a->n_tiles, a->B);
    hipLaunchKernelGGL(k_fm_sums<FMT>, grid, dim3(FM_WG), 0, s, *a);
    hipLaunchKernelGGL(k_fm_tile_scan, dim3(a->B), dim3(FM_WG), 0, s, *a);
    hipLaunchKernelGGL(k_fm_mod<FMT>, grid, dim3(FM_WG), 0, s, *a);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_fm_mod(const rd_fm_mod_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->n_tiles <= 0) return 0;
    if (a->B > 65535) return -1;
    if (a->fmt == 0) return fm_mod_launch<0>(a, (hipStream_t)s);
    if (a->fmt == 1) return fm_mod_launch<1>(a, (hipStream_t)s);
    return -1;
}

// ---- demodulator -------------------------------------------------------------------------------------------------------------------------------------------------
// the discriminator's angle: atan2 evaluated in double and rounded to float32 (correctly rounded but for the double rounding); d = 0 gives 0 whatever the signs of its
// zeros (fm.m:110 puts a 1 in front; in front of a stream bb[n - 1] = 0 and the product's zeros may be negative, where atan2 would answer +-pi)
__device__ __forceinline__ float fm_angle(float re, float im)
{
    return re == 0.0f && im == 0.0f ? 0.0f : (float)atan2((double)im, (double)re);
}

// capacities, in samples: every array carries FM_LEAD samples in front of its index 0 (the rotation reads up to four samples past a sum's last operand) and is rounded
// up to whole groups of four behind its end
#define FM_LEAD 4
#define FM_XM_CAP (RD_FM_TILE + 2 * RD_FM_NMAX + 2 * FM_LEAD)          // cnt + N1 + N2 - 1 + lead + round-up: 3080
#define FM_BB_CAP (RD_FM_TILE + RD_FM_NMAX + 2 * FM_LEAD)              // cnt + N2 + lead + round-up: 2568
#define FM_XM_PL (FM_XM_CAP / 4)
#define FM_BB_PL (FM_BB_CAP / 4)
static_assert(FM_XM_CAP % 4 == 0 && FM_BB_CAP % 4 == 0, "whole planes");
static_assert((FM_XM_CAP + FM_BB_CAP) * 8 + 2 * RD_FM_NMAX * 4 <= 64 * 1024, "static LDS; at most the rate converter's 80 KB");

__device__ __forceinline__ float fm_fma(float b, float w, float acc) { return fmaf(b, w, acc); }
__device__ __forceinline__ float2 fm_fma(float b, float2 w, float2 acc) { return make_float2(fmaf(b, w.x, acc.x), fmaf(b, w.y, acc.y)); }
__device__ __forceinline__ void fm_zero(float &v) { v = 0.0f; }
__device__ __forceinline__ void fm_zero(float2 &v) { v = make_float2(0.0f, 0.0f); }

// sample i (i >= -FM_LEAD) of an array stored in four planes of PL words
template <int PL> __device__ __forceinline__ int fm_at(int i) { const int u = i + FM_LEAD; return (u & 3) * PL + (u >> 2); }

// out[r] = sum_{k = 0..N-1} taps[k] X[4 g + e + r - k], r = 0..3 (e >= N - 1: every operand has an index >= 0): one accumulator per output and component, k ascending.
// X is stored in planes (fm_at); e and k are the same for all lanes, so the plane and the word offset of every read are scalars and lane g reads word g + offset.
template <class T, int PL> __device__ __forceinline__ void fm_fir4(const T *X, int g, int e, int N, const float *taps, T out[4])
{
    T a0, a1, a2, a3;
    fm_zero(a0); fm_zero(a1); fm_zero(a2); fm_zero(a3);
    const T *Xg = X + g;
    T w0 = Xg[fm_at<PL>(e)], w1 = Xg[fm_at<PL>(e + 1)], w2 = Xg[fm_at<PL>(e + 2)], w3 = Xg[fm_at<PL>(e + 3)];
    int k = 0;
    for (; k + 4 <= N; k += 4) {
        const f32x4 c = *(const f32x4 *)(taps + k);                  // one broadcast read of four taps
        const int p = e - k;                                          // w0 = X[4 g + p], the operand of output 0 at tap k
        const T n1 = Xg[fm_at<PL>(p - 1)], n2 = Xg[fm_at<PL>(p - 2)], n3 = Xg[fm_at<PL>(p - 3)], n4 = Xg[fm_at<PL>(p - 4)];       // p - 4 >= -FM_LEAD
        a0 = fm_fma(c[0], w0, a0); a1 = fm_fma(c[0], w1, a1); a2 = fm_fma(c[0], w2, a2); a3 = fm_fma(c[0], w3, a3);
        a0 = fm_fma(c[1], n1, a0); a1 = fm_fma(c[1], w0, a1); a2 = fm_fma(c[1], w1, a2); a3 = fm_fma(c[1], w2, a3);
        a0 = fm_fma(c[2], n2, a0); a1 = fm_fma(c[2], n1, a1); a2 = fm_fma(c[2], w0, a2); a3 = fm_fma(c[2], w1, a3);
        a0 = fm_fma(c[3], n3, a0); a1 = fm_fma(c[3], n2, a1); a2 = fm_fma(c[3], n1, a2); a3 = fm_fma(c[3], w0, a3);
        w3 = n1; w2 = n2; w1 = n3; w0 = n4;
    }
    for (; k < N; k++) {                                              // the last N mod 4 taps
        const float c = taps[k];
        a0 = fm_fma(c, w0, a0); a1 = fm_fma(c, w1, a1); a2 = fm_fma(c, w2, a2); a3 = fm_fma(c, w3, a3);
        w3 = w2; w2 = w1; w1 = w0; w0 = Xg[fm_at<PL>(e - k - 1)];     // e - k - 1 >= e - N >= -1
    }
    out[0] = a0; out[1] = a1; out[2] = a2; out[3] = a3;
}

__global__ __launch_bounds__(FM_WG) void k_fm_demod(rd_fm_demod_args a)
{
    __shared__ __attribute__((aligned(16))) float2 xm[FM_XM_CAP];
    __shared__ __attribute__((aligned(16))) float2 bb[FM_BB_CAP];
    __shared__ __attribute__((aligned(16))) float tp[2 * RD_FM_NMAX];
    float *ang = (float *)xm;                                         // the discriminator values, FM_XM_PL words per plane like xm: in xm's place once bb is complete
    const int b = blockIdx.y, tid = threadIdx.x;
    const rd_fm_dstream S = a.ps[b];
    const int N1 = a.N1, N2 = a.N2;
    const int n_tiles = (S.n_out + RD_FM_TILE - 1) / RD_FM_TILE;
    if ((int)blockIdx.x >= n_tiles) return;
    for (int i = tid; i < 2 * RD_FM_NMAX; i += FM_WG) tp[i] = i < RD_FM_NMAX ? (i < N1 ? a.taps[i] : 0.0f) : (i - RD_FM_NMAX < N2 ? a.taps[i] : 0.0f);
    const float *t1 = tp, *t2 = tp + RD_FM_NMAX;
    const float2 *x = (const float2 *)a.x + (size_t)b * a.x_stride;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int o0 = tile * RD_FM_TILE, cnt = min(RD_FM_TILE, S.n_out - o0);
        const long long nb = S.n0 + o0;                               // absolute index of the tile's first output
        const int W = cnt + N1 + N2 - 1, V = cnt + N2, U = cnt + N2 - 1;
        const long long lo = nb - N2 - (N1 - 1);                      // absolute index of xm[0]
        __syncthreads();                                              // the taps are there; the previous tile's arrays have been read
        // 0. the mixed window: x[n] cis(-(fcq n mod 2^32)), zeros outside the stream's samples and in front of absolute index 0; zeros in the lead and the round-up
        for (int w = tid - FM_LEAD; w < ((W + 3) & ~3) + FM_LEAD; w += FM_WG) {
            const long long nn = lo + w, gi = nn - S.in_base;
            float2 v = make_float2(0.0f, 0.0f);
            if (w >= 0 && w < W && nn >= 0 && gi >= 0 && gi < S.n_in) {
                const float2 xv = x[gi], c = fm_cis(0u - a.fcq * (unsigned)(unsigned long long)nn);
                v.x = fmaf(xv.x, c.x, -(xv.y * c.y));                 // fc = 0: c = (1, 0) and v = x bit for bit (finite non-zero x)
                v.y = fmaf(xv.x, c.y, xv.y * c.x);
            }
            if (w < FM_XM_CAP - FM_LEAD) xm[fm_at<FM_XM_PL>(w)] = v;
        }
        __syncthreads();
        // 1. bb[v] = sum_k b1[k] xm[v + N1 - 1 - k], v = 0..V-1 (absolute index nb - N2 + v), four at a time
        for (int g = tid; 4 * g < V; g += FM_WG) {
            float2 o[4];
            fm_fir4<float2, FM_XM_PL>(xm, g, N1 - 1, N1, t1, o);
#pragma unroll
            for (int r = 0; r < 4; r++) bb[fm_at<FM_BB_PL>(4 * g + r)] = o[r];
        }
        __syncthreads();                                              // bb complete, xm no longer read
        // 2. the discriminator: ang[u] from bb[u + 1] conj(bb[u]), u = 0..U-1 (absolute index nb - (N2 - 1) + u); zeros around it
        for (int u = tid - FM_LEAD; u < ((U + 3) & ~3) + FM_LEAD; u += FM_WG) {
            float v = 0.0f;
            if (u >= 0 && u < U) {
                const float2 p = bb[fm_at<FM_BB_PL>(u + 1)], q = bb[fm_at<FM_BB_PL>(u)];
                const float re = fmaf(p.x, q.x, p.y * q.y), im = fmaf(p.y, q.x, -(p.x * q.y));
                v = fm_angle(re, im);
                if (!a.dont_limit) v = fminf(fmaxf(v, -a.wd), a.wd);
                v *= a.inv_wd;
            }
            ang[fm_at<FM_XM_PL>(u)] = v;
        }
        if (a.bb_out) {
            float2 *bo = (float2 *)a.bb_out + (size_t)b * a.bb_stride + o0;
            for (int i = tid; i < cnt; i += FM_WG) bo[i] = bb[fm_at<FM_BB_PL>(N2 + i)];
        }
        __syncthreads();
        // 3. y[i] = sum_k b2[k] ang[i + N2 - 1 - k], i = 0..cnt-1
        for (int g = tid; 4 * g < cnt; g += FM_WG) {
            float o[4];
            fm_fir4<float, FM_XM_PL>(ang, g, N2 - 1, N2, t2, o);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = 4 * g + r;
                if (i >= cnt) break;
                if (a.fmt == 0) ((float *)a.y)[(size_t)b * a.y_stride + o0 + i] = o[r];
                else ((float2 *)a.y)[(size_t)b * a.y_stride + o0 + i] = make_float2(o[r], 0.0f);
            }
        }
    }
}

extern "C" int rd_launch_fm_demod(const rd_fm_demod_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_out <= 0) return 0;
    if (a->B > 65535 || a->N1 < 1 || a->N1 > RD_FM_NMAX || a->N2 < 1 || a->N2 > RD_FM_NMAX || (a->fmt != 0 && a->fmt != 1)) return -1;
    const int n_tiles = (a->max_out + RD_FM_TILE - 1) / RD_FM_TILE;
    int gx = 2048 / a->B; if (gx < 1) gx = 1;                         // about 2048 workgroups per launch: the taps are loaded once per workgroup
    if (gx > n_tiles) gx = n_tiles;
    hipLaunchKernelGGL(k_fm_demod, dim3(gx, a->B), dim3(FM_WG), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

// the phasor alone on chosen phases, and atan2 as the discriminator takes it, on chosen pairs (tests/test_fm_gpu.py: EPS_CIS, EPS_ATAN)
__global__ void k_fm_probe(const unsigned *ph, float2 *cis_out, const float2 *d, float *atan_out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (ph && cis_out) cis_out[i] = fm_cis(ph[i]);
    if (d && atan_out) atan_out[i] = fm_angle(d[i].x, d[i].y);
}
extern "C" int rd_launch_fm_probe(const unsigned *ph, void *cis_out, const void *d, float *atan_out, int n, rd_stream_t s)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_fm_probe, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, ph, (float2 *)cis_out, (const float2 *)d, atan_out, n);
    return (int)hipGetLastError();
}
