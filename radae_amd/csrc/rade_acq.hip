// rade_acq.hip -- whole-file pilot acquisition, rx.py:146-188 over every hop of every stream at once (include/rade_batch.h states the arithmetic, the order of every
// reduction and the error bound): rade_batch_acq_detect and rade_batch_acq_refine.
//   k_acq_detect    one wavefront per (twentieth of the 960 within-frame timings, stream), eight of them to a workgroup; walks the stream's 960-sample blocks in order
//   k_acq_combine   one thread per (hop, stream): folds the 20 wavefront partials of the hop in ascending order
//   k_acq_refine    one workgroup per event: acquisition.refine's 80 x 3 grid in double
// In a stored file every hop is known up front: hop k's Dt2 is hop k + 1's Dt1, so the surface D[t][f] = sum_m conj(x[t + m]) p_w[m][f] is formed ONCE per timing.  A
// wavefront owns 48 within-frame timings tau (three tiles of 16) for the whole stream: per block k it forms |D[960 k + tau][0..39]|, adds the values of block k - 1 it kept
// in registers (that is |Dt1| + |Dt2| of hop k - 1), and keeps the new ones.  Nothing of the surface goes to memory unless the caller asks for rows of it.
// The product is the two-stage correlator of rade_corr2.h (the algebra, the tables -- the engine's own, the ones the receiver's search uses --, the product order):
// 2 x 10 x 3 + 5 x 5 = 85 matrix instructions per tile of 16 timings, 255 per wavefront and block.  What is acquisition's own: the sample scale comes from the largest
// component of the 208 samples the wavefront reads for the block; the fragment of (timing tile T, k-step s) is the fragment of (T + s, 0), so 12 fragments serve 3 tiles
// x 10 steps; and stage 1 keeps TWO accumulators per (row tile, timing tile): hi x hi (10 instructions) and the cross planes lo x hi, hi x lo (20 instructions, 2^-11
// of the former), joined by one float32 addition per element on the way into stage 2.
// Both tables (50 KB) are copied to LDS by the workgroup and stay there: one workgroup of eight wavefronts per CU, two per SIMD (256 registers each), so that one
// wavefront's fragment reads, sample split and epilogue run under the other's matrix instructions.  After the tables are in place the wavefronts of a workgroup share
// nothing: each has its own sample planes in LDS, written and read by itself alone (a wavefront's LDS accesses complete in the order issued), so the loop over the
// blocks has no workgroup barrier and the eight wavefronts of a workgroup may belong to two or three streams of different length.
#include "rade_corr2.h"

#define ACQ_WAVES 8                                               // wavefronts per workgroup: two per SIMD under the 256 registers a wavefront then has
#define ACQ_WG (64 * ACQ_WAVES)
#define ACQ_RT 3                                                  // timing tiles per wavefront
#define ACQ_NFRAG (ACQ_RT + RD_CORR_NKS - 1)
#define ACQ_SPAN 208                                              // samples a wavefront reads per block: 16 (ACQ_NFRAG - 1) + 31 = 207, rounded up
#define ACQ_TAB_HALVES (RD_CORRQ16_HALFS + RD_CORRA16_HALFS)
#define ACQ_LDS (ACQ_TAB_HALVES * 2 + ACQ_WAVES * 2 * ACQ_SPAN * 4)
static_assert(RD_ACQ_NPART * ACQ_RT * 16 == RD_NMF, "the wavefronts of a stream cover the frame's timings once");
static_assert(16 * (ACQ_NFRAG - 1) + 15 + 12 + 3 < ACQ_SPAN && ACQ_SPAN <= 4 * 64, "the fragments' samples");
static_assert(ACQ_LDS <= 160 * 1024, "table planes + sample planes: the LDS of a CU");

__global__ __launch_bounds__(ACQ_WG) void k_acq_detect(rd_acq_args a)
{
    extern __shared__ __attribute__((aligned(16))) _Float16 acq_lds[];
    _Float16 *tabA = acq_lds;                                     // corrq16 | corra16
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int item = blockIdx.x * ACQ_WAVES + wave;               // (stream, twentieth): the last workgroup may have wavefronts without one
    const int b = item / RD_ACQ_NPART, part = item - b * RD_ACQ_NPART;
    const int n = b < a.B ? a.n[b] : 0;
    const int H = rd_acq_hops(n);
    for (int u = tid; u < ACQ_TAB_HALVES / 8; u += ACQ_WG)           // 16 bytes a thread and round: corrq16, then corra16 behind it
        ((u32x4 *)tabA)[u] = u < RD_CORRQ16_HALFS / 8 ? ((const u32x4 *)a.corrq16)[u] : ((const u32x4 *)a.corra16)[u - RD_CORRQ16_HALFS / 8];
    const _Float16 *tabQ = tabA + (size_t)lane * 8, *tabA2 = tabA + RD_CORRQ16_HALFS + (size_t)lane * 8;
    unsigned *ph = (unsigned *)(acq_lds + ACQ_TAB_HALVES) + wave * 2 * ACQ_SPAN, *pl = ph + ACQ_SPAN;
    const float2 *x = (const float2 *)a.x + (size_t)b * a.x_stride;
    const int T0 = part * ACQ_RT;                                 // the wavefront's first timing tile inside the frame
    float2 xr[4];
    auto load = [&](int blk) {                                    // samples 960 blk + 16 T0 + o, o < 208; the last one needed is 960 H + 1118 < n, what lies behind n reads as 0
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int o = lane + 64 * r; const long long idx = (long long)blk * RD_NMF + 16 * T0 + o;
            xr[r] = (o < ACQ_SPAN && idx < n) ? x[idx] : make_float2(0.0f, 0.0f);
        }
    };
    if (H) load(0);
    float prev[ACQ_RT][2 * RD_CORR_NFT];
#pragma unroll
    for (int rt = 0; rt < ACQ_RT; rt++)
#pragma unroll
        for (int c = 0; c < 2 * RD_CORR_NFT; c++) prev[rt][c] = 0.0f;
    __syncthreads();                                              // the table is whole; from here on a wavefront is on its own
    if (!H) return;
#pragma unroll 1
    for (int blk = 0; blk <= H; blk++) {
        float mx = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; r++) mx = fmaxf(mx, fmaxf(fabsf(xr[r].x), fabsf(xr[r].y)));
        mx = wave_max_f32(mx);
        float sc, unsc;                                           // mx sc in [2^7, 2^8); unsc undoes sc, stage 1's 2^12, the moments' 2^-7 and stage 2's 2^10
        operand_scale<12 + 3>(__float_as_uint(mx), sc, unsc);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int o = lane + 64 * r;
            if (o < ACQ_SPAN) rx2_split16(make_float2(xr[r].x * sc, xr[r].y * sc), ph[o], pl[o]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();      // the planes are the wavefront's own: its reads follow its writes
        if (blk < H) load(blk + 1);                               // in flight during the product
        // the B operand: lane (i, g) of fragment F holds column i (timing 16 F + i), k = 8 g + e: sample 16 F + i + 4 g + e / 2, (re, im) packed in one word
        u32x4 wh[ACQ_NFRAG], wl[ACQ_NFRAG];
#pragma unroll
        for (int F = 0; F < ACQ_NFRAG; F++)
#pragma unroll
            for (int j = 0; j < 4; j++) { wh[F][j] = ph[16 * F + i + 4 * g + j]; wl[F][j] = pl[16 * F + i + 4 * g + j]; }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); __builtin_amdgcn_wave_barrier();
        float lbest = 0.0f; int lkey = 0;
        double dsum = 0.0;
        // ---- stage 1: the 16 complex moments of every timing ----
        f32x4 ahi[ACQ_RT][2], alo[ACQ_RT][2];
#pragma unroll
        for (int rt = 0; rt < ACQ_RT; rt++)
#pragma unroll
            for (int u = 0; u < 2; u++) { ahi[rt][u] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f }; alo[rt][u] = (f32x4){ 0.0f, 0.0f, 0.0f, 0.0f }; }
#pragma unroll
        for (int s = 0; s < RD_CORR_NKS; s++) {
            const f16x8 a0h = *(const f16x8 *)(tabQ + corrq_frag(0, s, 0)), a0l = *(const f16x8 *)(tabQ + corrq_frag(0, s, 1));
            const f16x8 a1h = *(const f16x8 *)(tabQ + corrq_frag(1, s, 0)), a1l = *(const f16x8 *)(tabQ + corrq_frag(1, s, 1));
            corr2_kstep<ACQ_RT>(alo, ahi, a0h, a0l, a1h, a1l, [&](int rt) { return __builtin_bit_cast(f16x8, wh[rt + s]); }, [&](int rt) { return __builtin_bit_cast(f16x8, wl[rt + s]); });
        }
        // ---- stage 2 and the epilogue, one timing tile at a time ----
#pragma unroll
        for (int rt = 0; rt < ACQ_RT; rt++) {
            const int t = 16 * (T0 + rt) + i;
            const MomPlanes mp = mom_split_by([&](int j) { return ahi[rt][j >> 2][j & 3] + alo[rt][j >> 2][j & 3]; });
#pragma unroll
            for (int q = 0; q < RD_CORR_NFT; q++) {
                const f32x4 cc = mom_expand(*(const f16x8 *)(tabA2 + corra_frag(q, 0)), *(const f16x8 *)(tabA2 + corra_frag(q, 1)), mp);
                const int f = 8 * q + 2 * g;
                float c[4];
#pragma unroll
                for (int r = 0; r < 4; r++) c[r] = unsc * cc[r];
                const float d0 = __builtin_amdgcn_sqrtf(fmaf(c[0], c[0], c[1] * c[1])), d1 = __builtin_amdgcn_sqrtf(fmaf(c[2], c[2], c[3] * c[3]));
                if (a.dt) {
                    const long long row = (long long)blk * RD_NMF + t - a.t0;
                    if (row >= 0 && row < a.n_rows) {
                        float2 *o = (float2 *)a.dt + ((size_t)b * a.n_rows + (size_t)row) * RD_NFC + f;
                        o[0] = make_float2(c[0], c[1]); o[1] = make_float2(c[2], c[3]);
                    }
                }
                dsum += (double)d0; dsum += (double)d1;
                // |Dt1| + |Dt2| of hop blk - 1 (block 0 has no hop behind it: prev = 0 and the result is not kept).  The first cell in the script's order wins: smallest t, then f
                const float s0 = prev[rt][2 * q] + d0, s1 = prev[rt][2 * q + 1] + d1;
                const int k0 = (t << 6) | f;
                if (s0 > lbest || (s0 == lbest && k0 < lkey)) { lbest = s0; lkey = k0; }
                if (s1 > lbest || (s1 == lbest && k0 + 1 < lkey)) { lbest = s1; lkey = k0 + 1; }
                prev[rt][2 * q] = d0; prev[rt][2 * q + 1] = d1;
            }
        }
        dsum = wave_sum_f64(dsum);
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const float ov = __shfl_xor(lbest, off); const int ok = __shfl_xor(lkey, off);
            if (ov > lbest || (ov == lbest && ok < lkey)) { lbest = ov; lkey = ok; }
        }
        if (lane == 0) {
            a.psum[((size_t)b * (a.max_hops + 1) + blk) * RD_ACQ_NPART + part] = dsum;
            if (blk) { rd_acq_pmax *o = a.pmax + ((size_t)b * a.max_hops + (blk - 1)) * RD_ACQ_NPART + part; o->best = lbest; o->key = lkey; }
        }
    }
}

__global__ __launch_bounds__(64) void k_acq_combine(rd_acq_args a)
{
    const int hop = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (hop >= rd_acq_hops(a.n[b])) return;
    const rd_acq_pmax *pm = a.pmax + ((size_t)b * a.max_hops + hop) * RD_ACQ_NPART;
    const double *p1 = a.psum + ((size_t)b * (a.max_hops + 1) + hop) * RD_ACQ_NPART, *p2 = p1 + RD_ACQ_NPART;
    float best = 0.0f; int key = 0;
    double S1 = 0.0, S2 = 0.0;
    for (int j = 0; j < RD_ACQ_NPART; j++) {
        if (pm[j].best > best || (pm[j].best == best && pm[j].key < key)) { best = pm[j].best; key = pm[j].key; }
        S1 += p1[j]; S2 += p2[j];
    }
    rd_acq_rec *o = a.rec + (size_t)b * a.max_hops + hop;
    o->best = best; o->key = key; o->S1 = S1; o->S2 = S2;
}

// acquisition.refine (dsp.py:233-270): thread (fi, ti) = (tid / 3, tid % 3) forms Dt1 + Dt2 of frequency fmax - 10 + 0.25 fi and timing t_abs - 1 + ti in double, in
// ascending m; thread 0 takes the maximum by strict > in the script's order (frequency outer, timing inner)
__global__ __launch_bounds__(256) void k_acq_refine(rd_acq_refine_args a)
{
    __shared__ double mag12[3 * RD_ACQ_NFINE], mag1[3 * RD_ACQ_NFINE];
    __shared__ int win_ti;
    const int e = blockIdx.x, tid = threadIdx.x;
    const rd_acq_ev ev = a.ev[e];
    const int n = a.n[ev.stream];
    const float2 *x = (const float2 *)a.x + (size_t)ev.stream * a.x_stride;
    if (tid < 3 * RD_ACQ_NFINE) {
        const int fi = tid / 3, ti = tid - 3 * fi;
        const long long t = ev.t_abs - 1 + ti;
        double v12 = -1.0, v1 = 0.0;
        if (t >= 0 && t + RD_NMF + RD_M <= n) {                   // DEVIATION: the script indexes with t = -1 (the last sample) and fails behind the end
            const double w = (2.0 * PI_D * dgrid_nc(ev.fmax - 10.0, fi, 0.25)) / 8000.0;
            double r1 = 0.0, i1 = 0.0, r2 = 0.0, i2 = 0.0;
            for (int m = 0; m < RD_M; m++) {
                double sn, cs; sincos(w * (double)m, &sn, &cs);   // e^{-j w m} = (cs, -sn)
                const double pr = a.tab->p[m][0], pi = a.tab->p[m][1];
                const double qr = cs * pr - sn * pi, qi = -cs * pi - sn * pr;               // e^{-j w m} conj(p[m])
                const double ar = x[t + m].x, ai = x[t + m].y, br = x[t + RD_NMF + m].x, bi = x[t + RD_NMF + m].y;
                r1 += ar * qr - ai * qi; i1 += ar * qi + ai * qr;
                r2 += br * qr - bi * qi; i2 += br * qi + bi * qr;
            }
            double sn, cs; sincos(w * (double)RD_NMF, &sn, &cs);  // Dt2 carries e^{-j w Nmf}
            const double rr = r2 * cs + i2 * sn, ii = i2 * cs - r2 * sn;
            v12 = hypot(r1 + rr, i1 + ii); v1 = hypot(r1, i1);
        }
        mag12[tid] = v12; mag1[tid] = v1;
    }
    __syncthreads();
    if (tid == 0) {
        double Dmax = 0.0; int k = -1;
        for (int j = 0; j < 3 * RD_ACQ_NFINE; j++) if (mag12[j] > Dmax) { Dmax = mag12[j]; k = j; }
        rd_acq_fine *o = a.out + e;
        o->t = k < 0 ? ev.t_abs : ev.t_abs - 1 + k % 3; o->f = k < 0 ? ev.fmax : dgrid_nc(ev.fmax - 10.0, k / 3, 0.25); o->Dmax = Dmax;
        win_ti = k < 0 ? 0 : k % 3;
    }
    __syncthreads();
    if (tid < RD_ACQ_NFINE) a.dfine[(size_t)e * RD_ACQ_NFINE + tid] = mag1[3 * tid + win_ti];
}

extern "C" int rd_launch_acq_detect(const rd_acq_args *a, rd_stream_t s)
{
    if (a->B <= 0 || a->max_hops <= 0) return 0;
    rd_dyn_lds_once<k_acq_detect, ACQ_LDS>();
    hipLaunchKernelGGL(k_acq_detect, dim3((a->B * RD_ACQ_NPART + ACQ_WAVES - 1) / ACQ_WAVES), dim3(ACQ_WG), ACQ_LDS, (hipStream_t)s, *a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_acq_combine, dim3((a->max_hops + 63) / 64, a->B), dim3(64), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

extern "C" int rd_launch_acq_refine(const rd_acq_refine_args *a, rd_stream_t s)
{
    if (a->n_events <= 0) return 0;
    hipLaunchKernelGGL(k_acq_refine, dim3(a->n_events), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}
