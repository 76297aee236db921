// rade_loss.hip -- the reference's acceptance metric on the device: loss.py:find_loss (:64-91) over distortion_loss (radae_base.py:50-68, the first
// 20 features), every stream of a batch in one pass (rade_batch_loss, include/rade_batch.h).
//
//   k_loss_offsets   one lane per candidate offset s of a stream, RD_LOSS_WG offsets per workgroup, (offset blocks, B) workgroups.  A lane owns the double
//                    sum over t of distortion_loss(features[s + t], hat[t]) and runs t forward over tiles of LS_TT decoded rows: the tile's hat rows (every
//                    lane reads the same one: a broadcast) and the feature rows of the workgroup's offsets are staged in LDS.  The workgroup's best
//                    (loss, s) goes out.
//   k_loss_pick      per stream, the best of its workgroups' results: find_loss's strict-<, lowest-offset-first scan.
//   k_loss_frames    optional: loss.py:85-90's per-frame curve at the chosen offset, one thread per frame.
//
// Numerical contract: bit-equal to oracle/rade_oracle.c:orc_distortion_loss / orc_find_loss, which is built with -ffp-contract=off.  The frame term is
// float32 in the oracle's order, with no contraction (the pragma below: HIP contracts by default) and the correctly rounded float divide; the frame terms
// of an offset are added in double in frame order and divided by n_hat.  Summing an offset's frames in any other order would not be bit-equal, so the
// parallelism is across offsets and streams only.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "rade_dev.h"

#pragma clang fp contract(off)

#define LS_TT 128      // decoded rows per LDS tile
#define LS_FP 21       // LDS pitch of a staged feature row in floats: odd, so the rows that lanes s and s + 1 read at the same t start in different banks

// distortion_loss of one frame pair with 20 features (radae_base.py:55-63; rade_oracle.c:928-935): y = transmitted row, p = decoded row
__device__ __forceinline__ float ls_frame(const float *y, const float *p)
{
    const float c1 = (float)(3.0 * (10.0 / 18.0)), c2 = (float)(1.0 / 18.0);
    const float pitch = 2.0f * (p[18] - y[18]), corr = p[19] - y[19];
    float pw = y[19] + 0.5f;
    pw = pw > 0.0f ? pw * pw : 0.0f;                                   // relu(.) ** 2
    const float extra = c1 * fabsf(pitch) * pw + c2 * corr * corr;     // (the 21st feature's term is + 0 with 20 features)
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 18; i++) { const float e = p[i] - y[i]; acc += e * e + extra; }
    return acc / 18.0f;
}

// find_loss's scan (loss.py:75-81) as a total order: the lower loss first, then the lower offset.  Nothing compares below a NaN loss at offset 0, so the
// scan keeps it; a NaN at any other offset is never taken.
__device__ __forceinline__ double ls_key(double v, int s) { return v == v ? v : (s == 0 ? -__builtin_inf() : __builtin_inf()); }
__device__ __forceinline__ bool ls_better(double v, int s, double w, int r)
{
    const double kv = ls_key(v, s), kw = ls_key(w, r);
    return kv < kw || (kv == kw && s < r);
}

__global__ __launch_bounds__(RD_LOSS_WG) void k_loss_offsets(rd_loss_args a)
{
    __shared__ float fs[(RD_LOSS_WG + LS_TT) * LS_FP];
    __shared__ float hs[LS_TT * 20];
    __shared__ double rv[RD_LOSS_WG];
    __shared__ int rs[RD_LOSS_WG];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n_in = a.len[b], n_hat = a.len[a.B + b];
    if (n_hat <= 0 || n_hat > n_in) return;
    const int n_off = n_in > n_hat ? n_in - n_hat : 1;                 // s = 0, then s in [0, n_in - n_hat): s = n_in - n_hat is never tried
    const int s0 = blockIdx.x * RD_LOSS_WG;
    if (s0 >= n_off) return;
    const float *F = a.feat + (size_t)b * a.f_stride, *H = a.hat + (size_t)b * a.h_stride;
    const int s = s0 + tid;
    const bool on = s < n_off;
    double tot = 0.0;
    for (int t0 = 0; t0 < n_hat; t0 += LS_TT) {
        const int nt = min(LS_TT, n_hat - t0);
        const int nf = min(RD_LOSS_WG + nt - 1, n_in - s0 - t0);       // feature rows s0 + t0 + [0, nf): every row a lane of this tile reads, none past n_in
        __syncthreads();                                                // (the previous tile is consumed)
        for (int k = tid; k < nt * 20; k += RD_LOSS_WG) { const int r = k / 20, c = k - 20 * r; hs[k] = H[(size_t)(t0 + r) * a.h_row + c]; }
        for (int k = tid; k < nf * 20; k += RD_LOSS_WG) { const int r = k / 20, c = k - 20 * r; fs[r * LS_FP + c] = F[(size_t)(s0 + t0 + r) * a.f_row + c]; }
        __syncthreads();
        if (on)
            for (int t = 0; t < nt; t++) tot += (double)ls_frame(&fs[(tid + t) * LS_FP], &hs[t * 20]);
    }
    rv[tid] = on ? tot / n_hat : __builtin_nan(""); rs[tid] = on ? s : INT_MAX;
    __syncthreads();
    for (int w = RD_LOSS_WG / 2; w > 0; w >>= 1) {
        if (tid < w && ls_better(rv[tid + w], rs[tid + w], rv[tid], rs[tid])) { rv[tid] = rv[tid + w]; rs[tid] = rs[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { a.part_v[(size_t)b * a.n_blk + blockIdx.x] = rv[0]; a.part_s[(size_t)b * a.n_blk + blockIdx.x] = rs[0]; }
}

__global__ __launch_bounds__(64) void k_loss_pick(rd_loss_args a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const int n_in = a.len[b], n_hat = a.len[a.B + b];
    double v = __builtin_nan(""); int s = -1;
    if (n_hat > 0 && n_hat <= n_in) {
        const int nb = ((n_in > n_hat ? n_in - n_hat : 1) + RD_LOSS_WG - 1) / RD_LOSS_WG;
        const double *pv = a.part_v + (size_t)b * a.n_blk; const int *ps = a.part_s + (size_t)b * a.n_blk;
        v = pv[0]; s = ps[0];
        for (int k = 1; k < nb; k++) if (ls_better(pv[k], ps[k], v, s)) { v = pv[k]; s = ps[k]; }
    }
    a.loss[b] = v; a.start[b] = s;
}

__global__ __launch_bounds__(256) void k_loss_frames(rd_loss_args a)
{
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    const int s = a.start[b];
    if (s < 0 || f >= a.len[a.B + b] - s) return;                    // loss.py:86: n_hat - start frames
    a.frame_loss[(size_t)b * a.fl_stride + f] = ls_frame(a.feat + (size_t)b * a.f_stride + (size_t)(s + f) * a.f_row, a.hat + (size_t)b * a.h_stride + (size_t)f * a.h_row);
}

extern "C" int rd_launch_loss(const rd_loss_args *a, rd_stream_t s)
{
    if (a->B <= 0) return 0;
    hipStream_t st = (hipStream_t)s;
    if (a->n_blk > 0) hipLaunchKernelGGL(k_loss_offsets, dim3(a->n_blk, a->B), dim3(RD_LOSS_WG), 0, st, *a);
    hipLaunchKernelGGL(k_loss_pick, dim3((a->B + 63) / 64), dim3(64), 0, st, *a);
    if (a->frame_loss && a->max_hat > 0) hipLaunchKernelGGL(k_loss_frames, dim3((a->max_hat + 255) / 256, a->B), dim3(256), 0, st, *a);
    return (int)hipGetLastError();
}
