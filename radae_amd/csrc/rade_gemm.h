// rade_gemm.h -- the GEMM family and its launch shim; part of rade_kernels.hip (see its inventory).
// Replaces: every Linear / GRU-input / Conv1d(k=2) / GLU layer of CoreEncoder / CoreDecoder (radae_base.py:260-286, :400-416; src/rade_enc.c:55-114;
// src/rade_dec.c:50-102), for all streams and all time steps of a chunk at once.
// Needs rd_gemm_args (rade_dev.h), g_zero_row (rade_kernels.hip); f32x4 / f32x16 / f16x8, clamp1, sigmoid_f, gate_tanh, gate_sigmoid, split16_act,
// rd_dyn_lds_once (rade_devutil.h).
#include <type_traits>
// (The lane -> operand-row prologue, the accumulator clear and the rr -> (bb, tt) epilogue stand in each kernel: as shared inlined functions they changed its instructions.)
// GEMM: one wavefront = 32 rows x (32*NT) columns; A and packed-W fragments stream straight from
// global/L2 into VGPRs as 16-byte loads (no LDS: each A row is read by exactly one wave, W is
// L2-resident and shared by every wave).  Lane l holds A[row l&31][k = 8kb + 4(l>>5) + s], s=0..3,
// and the packed W holds the matching k for the same lane, so MFMA s contracts k pairs
// {8kb+s, 8kb+4+s}; summation order over k does not matter.
template <int NT>
__global__ __launch_bounds__(64) void k_gemm(rd_gemm_args a)
{
    const int lane = threadIdx.x;
    const int rows = a.B * a.T;
    const int r0 = blockIdx.x * 32;
    const int ntt = (a.N + 31) >> 5;
    const int nt0 = blockIdx.y * NT;
    int r = r0 + (lane & 31);
    if (r >= rows) r = rows - 1;
    const int b = r / a.T, t = r - b * a.T;
    const int half = lane >> 5;
    const float *p1 = a.a1 + b * a.a1_sb + t * a.a1_st + 4 * half;
    const float *p0 = nullptr;
    if (a.K0) {
        const bool rst = a.reset && a.reset[b * a.reset_sb + t];
        p0 = (rst ? g_zero_row : a.a0 + b * a.a0_sb + t * a.a0_st) + 4 * half;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < 16; j++) acc[i][j] = 0.0f;

    const float *wp = a.Wp + ((size_t)nt0 * 64 + lane) * 4;
    const size_t wstep = (size_t)ntt * 256;
#pragma unroll 1
    for (int seg = 0; seg < 2; seg++) {
        const float *p = seg == 0 ? p0 : p1;
        const int nkb = (seg == 0 ? a.K0 : a.K1) >> 3;
        if (nkb == 0) continue;
        f32x4 av = *(const f32x4 *)p;
        f32x4 bv[NT];
#pragma unroll
        for (int i = 0; i < NT; i++) bv[i] = *(const f32x4 *)(wp + i * 256);
        for (int kb = 0; kb < nkb; kb++) {
            f32x4 an = av; f32x4 bn[NT];
#pragma unroll
            for (int i = 0; i < NT; i++) bn[i] = bv[i];
            if (kb + 1 < nkb) {          // prefetch next k-block while the MFMAs of this one run
                an = *(const f32x4 *)(p + (kb + 1) * 8);
#pragma unroll
                for (int i = 0; i < NT; i++) bn[i] = *(const f32x4 *)(wp + wstep + i * 256);
            }
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int i = 0; i < NT; i++)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[i][s], acc[i], 0, 0, 0);
            av = an;
#pragma unroll
            for (int i = 0; i < NT; i++) bv[i] = bn[i];
            wp += wstep;
        }
    }
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int col = (nt0 + i) * 32 + (lane & 31);
        if (col >= a.N) continue;
        const float bias = a.bias ? a.bias[col] : 0.0f;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int rr = r0 + (j & 3) + 8 * (j >> 2) + 4 * half;
            if (rr >= rows) continue;
            const int bb = rr / a.T, tt = rr - bb * a.T;
            if (a.n_rows && tt >= a.n_rows[bb]) continue;
            float v = acc[i][j] + bias;
            if (a.act == 1) v = clamp1(tanhf(v));
            else if (a.act == 2) v = clamp1(a.a1[bb * a.a1_sb + tt * a.a1_st + col] * sigmoid_f(v));
            a.y[bb * a.y_sb + tt * a.y_st + col] = v;
        }
    }
}

// The same GEMM on the f16 matrix cores, operands split in two binary16 planes (see ds_gemm16 below for the
// arithmetic): activations are split on the fly, W comes from rd_pack_weights_f16x2.  K segments are multiples of 16.
template <int NT, int RT>
__global__ __launch_bounds__(64) void k_gemm16(rd_gemm_args a)
{   // one wavefront = RT row tiles of 32 rows x NT column tiles: every W fragment is applied to RT row tiles, so the L2 traffic
    // for the weights (the whole matrix per workgroup) drops RT-fold
    const int lane = threadIdx.x;
    const int rows = a.B * a.T;
    const int r0 = blockIdx.x * 32 * RT;
    const int ntt = (a.N + 31) >> 5;
    const int nt0 = blockIdx.y * NT;
    const int half = lane >> 5;
    const float *p1[RT], *p0[RT];
#pragma unroll
    for (int q = 0; q < RT; q++) {
        int r = r0 + 32 * q + (lane & 31);
        if (r >= rows) r = rows - 1;
        const int b = r / a.T, t = r - b * a.T;
        p1[q] = a.a1 + b * a.a1_sb + t * a.a1_st + 8 * half;
        p0[q] = nullptr;
        if (a.K0) {
            const bool rst = a.reset && a.reset[b * a.reset_sb + t];
            p0[q] = (rst ? g_zero_row : a.a0 + b * a.a0_sb + t * a.a0_st) + 8 * half;
        }
    }
    f32x16 acc[RT][NT];
#pragma unroll
    for (int q = 0; q < RT; q++)
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int j = 0; j < 16; j++) acc[q][i][j] = 0.0f;
    const int nkb0 = a.K0 >> 4, nkb = nkb0 + (a.K1 >> 4);
    const bool single = a.Wscale != nullptr;          // int8-exact layer: the weights are ONE plane of integers (exact in binary16), two products per k-block
    const int planes = single ? 1 : 2;
    const unsigned short *wbase = a.Wp16 + ((size_t)nt0 * planes * 64 + lane) * 8;
    const size_t wstep = (size_t)ntt * planes * 64 * 8;
    f32x4 a4[RT][2]; f16x8 bh[NT], bl[NT];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int q = 0; q < RT; q++) {
            const float *p = kb < nkb0 ? p0[q] + kb * 16 : p1[q] + (kb - nkb0) * 16;
            a4[q][0] = *(const f32x4 *)p; a4[q][1] = *(const f32x4 *)(p + 4);
        }
#pragma unroll
        for (int i = 0; i < NT; i++) { bh[i] = *(const f16x8 *)(wbase + kb * wstep + (size_t)i * planes * 64 * 8); if (!single) bl[i] = *(const f16x8 *)(wbase + kb * wstep + (size_t)i * 2 * 64 * 8 + 64 * 8); }
    };
    fetch(0);
#pragma unroll 1
    for (int kb = 0; kb < nkb; kb++) {
        f16x8 ah[RT], al[RT], ch[NT], cl[NT];
#pragma unroll
        for (int q = 0; q < RT; q++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                _Float16 hi, lo;
                split16_act(a4[q][j >> 2][j & 3], hi, lo);
                ah[q][j] = hi; al[q][j] = lo;
            }
#pragma unroll
        for (int i = 0; i < NT; i++) { ch[i] = bh[i]; cl[i] = bl[i]; }
        if (kb + 1 < nkb) fetch(kb + 1);                    // next k-block's loads fly during the matrix instructions
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < RT; q++)
#pragma unroll
            for (int i = 0; i < NT; i++) {
                acc[q][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[q], ch[i], acc[q][i], 0, 0, 0);
                if (!single) acc[q][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[q], cl[i], acc[q][i], 0, 0, 0);
                acc[q][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[q], ch[i], acc[q][i], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int q = 0; q < RT; q++)
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const int col = (nt0 + i) * 32 + (lane & 31);
            if (col >= a.N) continue;
            const float bias = a.bias ? a.bias[col] : 0.0f;
            const float scl = single ? a.Wscale[col] * 0x1p-8f : 0x1p-18f;       // integers x column scale (rows carry 2^8), or two planes of 2^10 w
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int rr = r0 + 32 * q + (j & 3) + 8 * (j >> 2) + 4 * half;
                if (rr >= rows) continue;
                const int bb = rr / a.T, tt = rr - bb * a.T;
                if (a.n_rows && tt >= a.n_rows[bb]) continue;
                float v = acc[q][i][j] * scl + bias;
                if (a.act == 1) v = clamp1(gate_tanh(v));                 // hardware exp2 / rcp, as in the recurrences
                else if (a.act == 2) v = clamp1(a.a1[bb * a.a1_sb + tt * a.a1_st + col] * gate_sigmoid(v));
                a.y[bb * a.y_sb + tt * a.y_st + col] = v;
            }
        }
}

// The same kernel with two k-blocks of operands in flight and no branch inside the k loop: "one or two weight planes" is a template
// parameter and the k-blocks come in pairs (every layer of the model has an even number), the fetches past the end re-read the last
// block.  With the plane count a run-time flag every matrix instruction sat behind a uniform branch and the loads of the next
// k-block could only be waited for all at once; here the compiler counts them (partial vmcnt waits) and a fetch has two k-blocks of
// matrix work to complete.
// One wavefront per workgroup.  Measured and not kept (round 5, profiles/r05_ab_notes.txt): 2 / 4 / 8 wavefronts per workgroup on ADJACENT row tiles against the same
// column tiles, so that all but the first find the weight fragments in that CU's vector L1, change nothing alone (+2.3 / +0.3 / +7.3 % GEMM time) and nothing
// decidable in the pipeline (-0.2 / +1.3 / -10.5 % frames/s): the weight traffic (3.5 GB of the 5.9 GB a pass moves from L2 to L1) is not what these launches wait for.
template <int NT, int RT, bool SINGLE>
__global__ __launch_bounds__(64) void k_gemm16p(rd_gemm_args a)
{
    const int lane = threadIdx.x & 63;
    const int rows = a.B * a.T;
    const int r0 = (blockIdx.x + (int)(threadIdx.x >> 6)) * 32 * RT;      // threadIdx.x >> 6 is 0; the term keeps r0 a vector value (the measured code)
    if (r0 >= rows) return;
    const int ntt = (a.N + 31) >> 5;
    const int nt0 = blockIdx.y * NT;
    const int half = lane >> 5;
    const float *p1[RT], *p0[RT];
#pragma unroll
    for (int q = 0; q < RT; q++) {
        int r = r0 + 32 * q + (lane & 31);
        if (r >= rows) r = rows - 1;
        const int b = r / a.T, t = r - b * a.T;
        p1[q] = a.a1 + b * a.a1_sb + t * a.a1_st + 8 * half;
        p0[q] = p1[q];
        if (a.K0) {
            const bool rst = a.reset && a.reset[b * a.reset_sb + t];
            p0[q] = (rst ? g_zero_row : a.a0 + b * a.a0_sb + t * a.a0_st) + 8 * half;
        }
    }
    f32x16 acc[RT][NT];
#pragma unroll
    for (int q = 0; q < RT; q++)
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int j = 0; j < 16; j++) acc[q][i][j] = 0.0f;
    const int nkb0 = a.K0 >> 4, nkb = nkb0 + (a.K1 >> 4);
    constexpr int planes = SINGLE ? 1 : 2;
    const unsigned short *wbase = a.Wp16 + ((size_t)nt0 * planes * 64 + lane) * 8;
    const size_t wstep = (size_t)ntt * planes * 64 * 8;
    f32x4 a4[2][RT][2]; f16x8 bh[2][NT], bl[2][NT];
    auto fetch = [&](int st, int kb_) {
        const int kb = min(kb_, nkb - 1);
#pragma unroll
        for (int q = 0; q < RT; q++) {
            const float *p = kb < nkb0 ? p0[q] + kb * 16 : p1[q] + (kb - nkb0) * 16;
            a4[st][q][0] = *(const f32x4 *)p; a4[st][q][1] = *(const f32x4 *)(p + 4);
        }
#pragma unroll
        for (int i = 0; i < NT; i++) {
            bh[st][i] = *(const f16x8 *)(wbase + kb * wstep + (size_t)i * planes * 64 * 8);
            if (!SINGLE) bl[st][i] = *(const f16x8 *)(wbase + kb * wstep + (size_t)i * 2 * 64 * 8 + 64 * 8);
        }
    };
    auto block = [&](int st, int kb_next) {
        f16x8 ah[RT], al[RT], ch[NT], cl[NT];
#pragma unroll
        for (int q = 0; q < RT; q++)
#pragma unroll
            for (int j = 0; j < 8; j++) {
                _Float16 hi, lo;
                split16_act(a4[st][q][j >> 2][j & 3], hi, lo);
                ah[q][j] = hi; al[q][j] = lo;
            }
#pragma unroll
        for (int i = 0; i < NT; i++) { ch[i] = bh[st][i]; cl[i] = bl[st][i]; }
        fetch(st, kb_next);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < RT; q++)
#pragma unroll
            for (int i = 0; i < NT; i++) {
                acc[q][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[q], ch[i], acc[q][i], 0, 0, 0);
                if (!SINGLE) acc[q][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[q], cl[i], acc[q][i], 0, 0, 0);
                acc[q][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[q], ch[i], acc[q][i], 0, 0, 0);
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    fetch(0, 0); fetch(1, 1);
#pragma unroll 1
    for (int kb = 0; kb < nkb; kb += 2) { block(0, kb + 2); block(1, kb + 3); }
    // This kernel's own epilogue: the other three divide by T for every element (in rounds 1-4 a third of a short layer's instructions); here a lane takes its
    // rows once per row tile -- tile row -> (stream, step) by ONE division per wavefront and carries, then the row's output pointer -- and then the column tiles.
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (j & 3) + 8 (j >> 2) + 4 (lane >> 5).
    const int cl0 = nt0 * 32 + (lane & 31);
    float bias[NT], scl[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int col = min(cl0 + 32 * i, a.N - 1);
        bias[i] = a.bias ? a.bias[col] : 0.0f;
        scl[i] = SINGLE ? a.Wscale[col] * 0x1p-8f : 0x1p-18f;
    }
    const int b0 = r0 / a.T, t0 = r0 - b0 * a.T;
#pragma unroll
    for (int q = 0; q < RT; q++)
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int off = 32 * q + (j & 3) + 8 * (j >> 2) + 4 * half;
            int bb = b0, tt = t0 + off;
            while (tt >= a.T) { tt -= a.T; bb++; }               // (a tile spans more than two streams only when T < 32 RT)
            if (r0 + off >= rows || (a.n_rows && tt >= a.n_rows[bb])) continue;
            float *yr = a.y + bb * a.y_sb + tt * a.y_st;
            const float *gr = a.a1 + bb * a.a1_sb + tt * a.a1_st;
#pragma unroll
            for (int i = 0; i < NT; i++) {
                const int col = cl0 + 32 * i;
                if (col >= a.N) continue;
                float v = acc[q][i][j] * scl[i] + bias[i];
                if (a.act == 1) v = clamp1(gate_tanh(v));
                else if (a.act == 2) v = clamp1(gr[col] * gate_sigmoid(v));
                yr[col] = v;
            }
        }
}

// Small-M variant (decoder rounds, single-stream API): the K loop is the latency, so 8 wavefronts of one
// workgroup split it (k-blocks interleaved), partial accumulators meet in LDS, and each wave finishes two of the
// sixteen accumulator registers of every tile (bias / activation / store).
#define SK_WAVES 8
template <int NT>
__global__ __launch_bounds__(64 * SK_WAVES) void k_gemm_splitk(rd_gemm_args a)
{
    extern __shared__ __attribute__((aligned(16))) float sk_red[];       // [SK_WAVES][NT][16][64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = a.B * a.T;
    const int r0 = blockIdx.x * 32;
    const int ntt = (a.N + 31) >> 5;
    const int nt0 = blockIdx.y * NT;
    if (a.n_rows) {                              // decoder rounds: skip tiles whose rows all lie beyond their stream's count
        const int rl = min(r0 + 31, rows - 1);
        bool any = false;
        for (int bb = r0 / a.T; bb <= rl / a.T; bb++) { const int tlo = max(r0 - bb * a.T, 0); any = any || (tlo < a.n_rows[bb]); }
        if (!any) return;
    }
    int r = r0 + (lane & 31);
    if (r >= rows) r = rows - 1;
    const int b = r / a.T, t = r - b * a.T;
    const int half = lane >> 5;
    const float *p1 = a.a1 + b * a.a1_sb + t * a.a1_st + 4 * half;
    const float *p0 = nullptr;
    if (a.K0) {
        const bool rst = a.reset && a.reset[b * a.reset_sb + t];
        p0 = (rst ? g_zero_row : a.a0 + b * a.a0_sb + t * a.a0_st) + 4 * half;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < 16; j++) acc[i][j] = 0.0f;
    const int nkb0 = a.K0 >> 3, nkb = nkb0 + (a.K1 >> 3);
    const float *wbase = a.Wp + ((size_t)nt0 * 64 + lane) * 4;
    const size_t wstep = (size_t)ntt * 256;
#pragma unroll 2
    for (int kb = wave; kb < nkb; kb += SK_WAVES) {
        const float *p = kb < nkb0 ? p0 + kb * 8 : p1 + (kb - nkb0) * 8;
        const f32x4 av = *(const f32x4 *)p;
        f32x4 bv[NT];
#pragma unroll
        for (int i = 0; i < NT; i++) bv[i] = *(const f32x4 *)(wbase + kb * wstep + i * 256);
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int i = 0; i < NT; i++)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[i][s], acc[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < 16; j++) sk_red[((wave * NT + i) * 16 + j) * 64 + lane] = acc[i][j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; i++) {
        const int col = (nt0 + i) * 32 + (lane & 31);
        if (col >= a.N) continue;
        const float bias = a.bias ? a.bias[col] : 0.0f;
#pragma unroll
        for (int jj = 0; jj < 2; jj++) {
            const int j = wave * 2 + jj;
            float v = 0.0f;
#pragma unroll
            for (int w = 0; w < SK_WAVES; w++) v += sk_red[((w * NT + i) * 16 + j) * 64 + lane];
            const int rr = r0 + (j & 3) + 8 * (j >> 2) + 4 * half;
            if (rr >= rows) continue;
            const int bb = rr / a.T, tt = rr - bb * a.T;
            if (a.n_rows && tt >= a.n_rows[bb]) continue;
            v += bias;
            if (a.act == 1) v = clamp1(tanhf(v));
            else if (a.act == 2) v = clamp1(a.a1[bb * a.a1_sb + tt * a.a1_st + col] * sigmoid_f(v));
            a.y[bb * a.y_sb + tt * a.y_st + col] = v;
        }
    }
}

// column tiles per wavefront: three where the tile count allows it, else two, else one; launch(nt) gets the count as an integral constant
template <class F> static inline void gemm_by_col_tiles(int ntt, F launch)
{
    if (ntt % 3 == 0) launch(std::integral_constant<int, 3>());
    else if (ntt % 2 == 0) launch(std::integral_constant<int, 2>());
    else launch(std::integral_constant<int, 1>());
}
extern "C" int rd_launch_gemm(const rd_gemm_args *a, rd_stream_t s)
{
    const int rows = a->B * a->T;
    if (rows <= 0) return 0;
    const int ntt = (a->N + 31) >> 5;
    hipStream_t st = (hipStream_t)s;
    const int gx = (rows + 31) / 32;
    if (rows <= 16384) {                       // too few row tiles to fill the chip: split K inside the workgroup
        gemm_by_col_tiles(ntt, [&](auto nt) {
            constexpr int NT = decltype(nt)::value, lds = SK_WAVES * NT * 16 * 64 * 4;
            rd_dyn_lds_once<k_gemm_splitk<NT>, lds>();
            hipLaunchKernelGGL(k_gemm_splitk<NT>, dim3(gx, ntt / NT), dim3(64 * SK_WAVES), lds, st, *a);
        });
        return (int)hipGetLastError();
    }
    dim3 block(64);
    if (a->Wp16 && (a->K0 & 15) == 0 && (a->K1 & 15) == 0) {          // f16 matrix cores, two-plane operands
        const int gx2 = (rows + 63) / 64;
        if ((((a->K0 + a->K1) >> 4) & 1) == 0 && ((a->K0 >> 4) & 1) == 0 && ntt % 3 == 0) {      // k-blocks in pairs (and the tap boundary on a pair)
            // one 32-row tile per wavefront for the one-plane layers: 96 accumulator registers less, a third wavefront per SIMD
            // (0.711 -> 0.667 ms per step over the encoder's GEMMs); six column tiles per wavefront (activations read once) changed nothing
            if (a->Wscale) { dim3 g1(gx, ntt / 3); hipLaunchKernelGGL((k_gemm16p<3, 1, true>), g1, block, 0, st, *a); return (int)hipGetLastError(); }
            dim3 grid(gx2, ntt / 3);
            hipLaunchKernelGGL((k_gemm16p<3, 2, false>), grid, block, 0, st, *a);
            return (int)hipGetLastError();
        }
        gemm_by_col_tiles(ntt, [&](auto nt) { constexpr int NT = decltype(nt)::value; hipLaunchKernelGGL((k_gemm16<NT, 2>), dim3(gx2, ntt / NT), block, 0, st, *a); });
        return (int)hipGetLastError();
    }
    gemm_by_col_tiles(ntt, [&](auto nt) { constexpr int NT = decltype(nt)::value; hipLaunchKernelGGL(k_gemm<NT>, dim3(gx, ntt / NT), block, 0, st, *a); });
    return (int)hipGetLastError();
}
