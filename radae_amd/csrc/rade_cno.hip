// rade_cno.hip -- the periodograms of rade_batch_cno_est (include/rade_batch.h states the arithmetic, the summation order and the error bound): est_CNo.py:31-45, the
// C + N and No band sums of every N-sample window of every stream, windows 2000 samples apart.
//   k_cno_blocks   one workgroup per (residue r = k mod J, stream); walks the stream's 2000-sample blocks once
//   k_cno_sum      one thread per (window, stream): adds the J residues' partials in the order r = 0..J-1
// With H = 2000, J = N / H and k = J q + r a window's bin is  X_w[k] = sum_{j < J} e^{-2 pi i r j / J} B_{w+j}[k],  B_b[k] = DFT_H(x[b H + n] e^{-2 pi i r n / N})[q]:
// one twiddle and one 2000-point transform per (block, residue), of which only the q inside the two bands are formed, then J terms per bin.  The J-term sum is formed
// afresh for every window from the last J blocks' bins (a ring in LDS); nothing is carried from window to window.
// The 2000-point transform is two dense stages, 2000 = 40 x 50, n = 50 n1 + n2, q = q1 + 40 q2, on the vector unit:
//   Y[n]      = x[b H + n] t[r n]                                                      t[m] = e^{-2 pi i m / N}, the one table of the call (host, double, rounded once)
//   A[q1][n2] = t[J n2 q1] sum_{n1 = 0..39} Y[50 n1 + n2] t[(N / 40)((q1 n1) mod 40)]   every q1, n2
//   B[q]      = sum_{n2 = 0..49} A[q1][n2] t[(N / 50)((q2 n2) mod 50)]                  the wanted q only
//   X_w[k]    = sum_{j = 0..J-1} B_{w+j}[q] t[H ((r j) mod J)]
// Every sum runs in the order written, one float32 accumulator per component, a term = four fused multiply-adds (cmac); a lone product = one multiply and one fused
// multiply-add per component (ctw).  |X|^2 = re re + im im and the band sums are double: a thread's bins in ascending order, the wavefront by wave_sum_f64, the eight
// wavefronts in ascending order -- no atomics, and a stream's sums do not depend on the rest of the batch.
// LDS (dynamic): Y 2000, A 40 x 51 (one sample of padding: the lanes of stage 2 differ in q1), the 40-, 50- and J-point phases, and the ring [J][pitch], complex64 each:
// 33.3 KB + 8 J pitch bytes, 90.9 KB at the defaults (J 16, pitch 450): one workgroup of 512 threads per CU.  Stage 1 gives a thread 4 values of q1 for one n2 (500
// threads, five LDS reads per four terms), stage 2 and the J-term sum one bin per thread and round.
#include <hip/hip_runtime.h>
#include "rade_dev.h"
#include "rade_devutil.h"

#define CNO_WG 512
#define CNO_H RD_CNO_H
#define CNO_APITCH 51
#define CNO_FIXED (CNO_H + 40 * CNO_APITCH + 40 + 50 + RD_CNO_JMAX)          // complex64 in front of the ring
#define CNO_LDS_MAX ((CNO_FIXED + RD_CNO_RING_MAX) * 8)
static_assert(CNO_LDS_MAX + 2 * 8 * 8 <= 160 * 1024, "fixed arrays + the largest ring + the reduction scratch: the LDS of a CU");
static_assert(CNO_H == 40 * 50 && CNO_WG >= 500 && 4 * CNO_WG >= CNO_H, "the two stages and the block load");

// acc += y w: four fused multiply-adds, real part first
__device__ __forceinline__ float2 cmac(float2 acc, float2 y, float2 w)
{
    acc.x = fmaf(y.x, w.x, acc.x); acc.x = fmaf(-y.y, w.y, acc.x);
    acc.y = fmaf(y.x, w.y, acc.y); acc.y = fmaf(y.y, w.x, acc.y);
    return acc;
}
// y w: one rounded product and one fused multiply-add per component
__device__ __forceinline__ float2 ctw(float2 y, float2 w) { return make_float2(fmaf(-y.y, w.y, y.x * w.x), fmaf(y.y, w.x, y.x * w.y)); }

__global__ __launch_bounds__(CNO_WG) void k_cno_blocks(rd_cno_args a)
{
    extern __shared__ __attribute__((aligned(16))) float2 cno_lds[];
    __shared__ double red[2][CNO_WG / 64];
    float2 *Y = cno_lds, *A = Y + CNO_H, *W40 = A + 40 * CNO_APITCH, *W50 = W40 + 40, *PJ = W50 + 50, *ring = PJ + RD_CNO_JMAX;
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int N = a.N, J = a.J, pitch = a.pitch;
    const int n = a.n[b];
    const int n_win = n > N ? (n - N + CNO_H - 1) / CNO_H : 0;                 // st = 0, 2000, .. while st < n - N
    if (!n_win) return;
    const int n_blocks = n_win + J - 1;                                         // (n_win - 1) H + N < n: every block lies inside the stream's n samples
    const float2 *tw = (const float2 *)a.tw;
    const float2 *x = (const float2 *)a.x + (size_t)b * a.x_stride;
    // the wanted q of this residue: k = J q + r inside [flow_bin, fhigh_bin), then inside [noise_st, noise_en); ceil((v - r) / J), 0 where v <= r
    const int qc0 = (max(a.flow_bin - r, 0) + J - 1) / J, qc1 = (max(a.fhigh_bin - r, 0) + J - 1) / J;
    const int qn0 = (max(a.noise_st - r, 0) + J - 1) / J, qn1 = (max(a.noise_en - r, 0) + J - 1) / J;
    const int nc = qc1 - qc0, nw = nc + (qn1 - qn0);                            // nw <= pitch, q < 2000: checked by the entry (noise_en <= N)
    if (tid < 40) W40[tid] = tw[(size_t)tid * (N / 40)];
    else if (tid >= 64 && tid < 64 + 50) W50[tid - 64] = tw[(size_t)(tid - 64) * (N / 50)];
    else if (tid >= 128 && tid < 128 + J) PJ[tid - 128] = tw[(size_t)((r * (tid - 128)) % J) * CNO_H];
    float2 pt[4], it[4], xr[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int i = tid + t * CNO_WG;
        pt[t] = i < CNO_H ? tw[r * i] : make_float2(0.0f, 0.0f);               // r i < J H = N
        xr[t] = i < CNO_H ? x[i] : make_float2(0.0f, 0.0f);
    }
    const int g = tid / 50, n2 = tid - 50 * g;                                  // stage 1: q1 = 4 g .. 4 g + 3 of column n2 (tid < 500)
#pragma unroll
    for (int u = 0; u < 4; u++) it[u] = tid < 500 ? tw[(size_t)(n2 * (4 * g + u)) * J] : make_float2(0.0f, 0.0f);     // n2 q1 < 2000
    double *part = a.part + (((size_t)b * a.max_win) * J + r) * 2;
    for (int blk = 0; blk < n_blocks; blk++) {
#pragma unroll
        for (int t = 0; t < 4; t++) { const int i = tid + t * CNO_WG; if (i < CNO_H) Y[i] = ctw(xr[t], pt[t]); }
        __syncthreads();
        if (blk + 1 < n_blocks) {                                               // the next block's samples: in flight during the two stages
#pragma unroll
            for (int t = 0; t < 4; t++) { const int i = tid + t * CNO_WG; if (i < CNO_H) xr[t] = x[(size_t)(blk + 1) * CNO_H + i]; }
        }
        if (tid < 500) {
            float2 acc[4]; int idx[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { acc[u] = make_float2(0.0f, 0.0f); idx[u] = 0; }
#pragma unroll 4
            for (int n1 = 0; n1 < 40; n1++) {
                const float2 y = Y[50 * n1 + n2];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    acc[u] = cmac(acc[u], y, W40[idx[u]]);
                    idx[u] += 4 * g + u; if (idx[u] >= 40) idx[u] -= 40;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) A[(4 * g + u) * CNO_APITCH + n2] = ctw(acc[u], it[u]);
        }
        __syncthreads();
        float2 *slot = ring + (blk % J) * pitch;
        for (int i = tid; i < nw; i += CNO_WG) {
            const int q = i < nc ? qc0 + i : qn0 + (i - nc);
            const int q2 = q / 40, q1 = q - 40 * q2;
            const float2 *row = A + q1 * CNO_APITCH;
            float2 acc = make_float2(0.0f, 0.0f);
            int idx = 0;
#pragma unroll 5
            for (int m = 0; m < 50; m++) {
                acc = cmac(acc, row[m], W50[idx]);
                idx += q2; if (idx >= 50) idx -= 50;
            }
            slot[i] = acc;
        }
        __syncthreads();
        if (blk >= J - 1) {                                                     // window w = blk - J + 1 is complete: blocks w .. w + J - 1 sit in slots (w + j) mod J
            const int w = blk - J + 1;
            double pc = 0.0, pn = 0.0;
            for (int i = tid; i < nw; i += CNO_WG) {
                float2 X = make_float2(0.0f, 0.0f);
                int s = w % J;
                for (int j = 0; j < J; j++) {
                    X = cmac(X, ring[s * pitch + i], PJ[j]);
                    if (++s == J) s = 0;
                }
                const double p = (double)X.x * (double)X.x + (double)X.y * (double)X.y;
                if (i < nc) pc += p; else pn += p;
            }
            pc = wave_sum_f64(pc); pn = wave_sum_f64(pn);
            if ((tid & 63) == 0) { red[0][tid >> 6] = pc; red[1][tid >> 6] = pn; }
            __syncthreads();
            if (tid == 0) {
                double sc = 0.0, sn = 0.0;
                for (int v = 0; v < CNO_WG / 64; v++) { sc += red[0][v]; sn += red[1][v]; }
                part[(size_t)w * J * 2] = sc; part[(size_t)w * J * 2 + 1] = sn;
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_cno_sum(rd_cno_args a)
{
    const int w = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    const int n = a.n[b];
    const int n_win = n > a.N ? (n - a.N + CNO_H - 1) / CNO_H : 0;
    if (w >= n_win) return;
    const double *p = a.part + (((size_t)b * a.max_win) + w) * a.J * 2;
    double sc = 0.0, sn = 0.0;
    for (int r = 0; r < a.J; r++) { sc += p[2 * r]; sn += p[2 * r + 1]; }
    double *o = a.bands + ((size_t)b * a.max_win + w) * 2;
    o[0] = sc; o[1] = sn;
}

extern "C" int rd_launch_cno(const rd_cno_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_win <= 0) return 0;
    if (a->J < 1 || a->J > RD_CNO_JMAX || a->N != a->J * CNO_H || a->pitch < 1 || (long)a->J * a->pitch > RD_CNO_RING_MAX) return -1;
    if (a->flow_bin < 0 || a->flow_bin >= a->fhigh_bin || a->fhigh_bin > a->noise_st || a->noise_st >= a->noise_en || a->noise_en > a->N) return -1;
    if (a->pitch < rd_cno_pitch(a->J, a->flow_bin, a->fhigh_bin, a->noise_st, a->noise_en)) return -1;
    rd_dyn_lds_once<k_cno_blocks, CNO_LDS_MAX>();
    const size_t lds = sizeof(float2) * ((size_t)CNO_FIXED + (size_t)a->J * a->pitch);
    hipLaunchKernelGGL(k_cno_blocks, dim3(a->J, a->B), dim3(CNO_WG), lds, (hipStream_t)s, *a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_cno_sum, dim3((a->max_win + 63) / 64, a->B), dim3(64), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
