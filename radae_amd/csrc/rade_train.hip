// rade_train.hip -- one training step of the decoder on the device (rade_train_*, include/rade_batch.h): the reference's CoreDecoder (radae_base.py:291-354) over whole
// sequences with the activations the backward pass needs, distortion_loss (radae_base.py:50-68) with its gradient, back-propagation through time, and Adam
// (train.py:147-150).  float32 throughout, no f16 / bf16 operand: these are the master weights.  Host sequencing: rade_train.c.
//
//   k_tr_gemm       every feed-forward product, in three forms through one pair of strides per operand (rade_train.h): Y = X W^T + b, dX += dY W, dW = dY^T X.
//                   64 x 64 tile of C per workgroup of 4 wavefronts, one 32 x 32 accumulator each on mfma_f32_32x32x2f32, 16-deep k-steps staged in LDS.  The
//                   instruction is a k-ordered fmaf chain: an element of C is fma(a_K-1, b_K-1, ... fma(a_0, b_0, 0)), whatever tile it falls in, so a row of Y or dX
//                   does not depend on the other rows of the call.  Epilogues: + old C, + bias, tanh, or the GLU (sigmoid saved, product with h).  The dW form sums over
//                   the rows M = B T: blockIdx.z owns a chunk of TR_CHUNK rows and writes its own partial; k_tr_fold adds the partials in chunk order.  No atomics.
//                   8.3 KB LDS (2 x 16 x 65 floats), 16 accumulator and fewer than 64 other VGPRs: 8 workgroups of 256 per CU, the wavefront limit.
//   k_tr_scan_fwd   h_t from gi_t and W_hh h_{t-1} for a tile of TR_SEQ = 16 sequences per workgroup, the tile being the M dimension of mfma_f32_16x16x4f32.
//                   6 wavefronts; wavefront w owns hidden units [16 w, 16 w + 16) of all three gates, its 3 x 16 x 96 slice of W_hh resident in 72 VGPRs per lane,
//                   so W_hh (110 KB) is read once per launch.  The accumulator's lane map (column = unit, 4 registers = 4 sequences) is the gate algebra's, so r, z, n,
//                   hn, h are formed where the products land; h goes to the other wavefronts through LDS, double-buffered: ONE barrier per step.
//                   gi of step t + 1 is fetched under step t's products.  12.8 KB LDS (2 x 16 x 100 floats), 144 VGPRs, one workgroup of 384 per 16 sequences
//                   (6 wavefronts on 4 SIMDs: occupancy is set by the batch, B / 16 workgroups, not by registers or LDS).
//   k_tr_scan_bwd   dh_{t-1} = dh_t z_t + W_hh^T [dr~, dz~, dn~ r] from row T - 1 to row 0, same tile and roles: wavefront w owns dh[16 w ..] and the 288 x 16 slice of
//                   W_hh in 72 VGPRs; the gate-gradient rows go out ([dr~, dz~, dn~] for dW_ih and dX, [dr~, dz~, dn~ r] for dW_hh) and through LDS, one barrier per
//                   step; the saved row of step t - 1 is fetched under step t's products.  The three 24-deep partial chains (one per gate) are added as (r + z) + n.
//                   37.4 KB LDS (2 x 16 x 292 floats), 161 VGPRs, one workgroup of 384 per 16 sequences.
//   k_tr_dtanh, k_tr_glu_bwd   the activation derivatives that no GEMM epilogue can take (they feed two GEMMs each): one pass per layer.
//   k_tr_loss_frames, k_tr_loss_sum   the loss as rade_loss.hip's ls_frame has it, 20 or 21 features, with d total / d features_hat; loss_by_batch in double after
//                   float32 frame terms, in frame order, and total in stream order.
//   k_tr_adam       one elementwise launch over the flat buffers; the bias corrections and the learning rate come from the host, formed in double.
//
// Summation order is fixed everywhere: results depend on B, T and the inputs only.  Rounding (u = 2^-24): an output of a K-deep product carries at most
// (K + 1) u sum|a b|; tanhf / expf are the device library's (<= 2 ulp).  NO end-to-end bound of features_hat or of a gradient is counted here: the per-product figure
// does not carry through five recurrent layers to anything a test could use, so the forward pass and the gradients are held to a measured tolerance instead
// (tests/train_ref.py: TOL, four times what a float32 evaluation in another summation order shows).  Counted and tested per element: Adam,
// m' <= 3 roundings of magnitude |m| + |g|, v' <= 4, the update <= 6 more (sqrt, two products, sum, divide, product) and one for p - update.
//
// Stated deviations from the reference: the uniform +-1/254 noise of n() is left out and the clamp kept -- every n() argument lies in [-1, 1] (tanh, the GLU product and
// the GRU state), so the clamp and its gradient mask are the identity; the GLU's effective weight is trained directly (radae_amd/train.py: weight_norm_grads covers (g, v)).
#include <hip/hip_runtime.h>
#include "rade_train.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define TG_T 64        // tile of C
#define TG_K 16        // k-step
#define TG_P 65        // LDS pitch of a k-row: odd, so a k-fastest fill does not land in one bank

__device__ __forceinline__ float tr_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float tg_a(const tr_gemm_args &a, int i, int k, int k_hi)
{
    if (i >= a.I || k >= k_hi) return 0.0f;
    if (a.a_shift) { if (i % a.T == 0) return 0.0f; i -= 1; }
    return a.A[(long)i * a.a_si + (long)k * a.a_sk];
}

__device__ __forceinline__ float tg_b(const tr_gemm_args &a, int k, int j, int k_hi)
{
    if (j >= a.J || k >= k_hi) return 0.0f;
    if (a.b_shift) { if (k % a.T == 0) return 0.0f; k -= 1; }
    return a.B[(long)k * a.b_sk + (long)j * a.b_sj];
}

__global__ __launch_bounds__(256) void k_tr_gemm(tr_gemm_args a)
{
    __shared__ float As[TG_K][TG_P], Bs[TG_K][TG_P];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wi = (w & 1) * 32, wj = (w >> 1) * 32;
    const int i0 = blockIdx.y * TG_T, j0 = blockIdx.x * TG_T;
    const int k_lo = a.k_chunk > 0 ? (int)blockIdx.z * a.k_chunk : 0;
    const int k_hi = a.k_chunk > 0 ? min(a.K, k_lo + a.k_chunk) : a.K;
    const bool a_kfast = a.a_sk == 1, b_jfast = a.b_sj == 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    for (int kb = k_lo; kb < k_hi; kb += TG_K) {
        __syncthreads();                                              // (the previous k-step is consumed)
#pragma unroll
        for (int e = tid; e < TG_T * TG_K; e += 256) {
            int kk = a_kfast ? (e & 15) : (e >> 6), x = a_kfast ? (e >> 4) : (e & 63);
            As[kk][x] = tg_a(a, i0 + x, kb + kk, k_hi);
            kk = b_jfast ? (e >> 6) : (e & 15); x = b_jfast ? (e & 63) : (e >> 4);
            Bs[kk][x] = tg_b(a, kb + kk, j0 + x, k_hi);
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < TG_K / 2; k2++)                         // lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * k2 + (lane >> 5)][wi + (lane & 31)], Bs[2 * k2 + (lane >> 5)][wj + (lane & 31)], acc, 0, 0, 0);
    }
    float *C = a.k_chunk > 0 ? a.C + (size_t)blockIdx.z * a.I * a.J : a.C;
    const int j = j0 + wj + (lane & 31);
    if (j >= a.J) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {                                    // C: column = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)
        const int i = i0 + wi + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (i >= a.I) continue;
        int ci = i;
        if (a.c_shift) { if (i % a.T == 0) continue; ci = i - 1; }
        float *c = C + (long)ci * a.c_si + (long)j * a.c_sj;
        float v = acc[r];
        if (a.beta) v = *c + v;
        if (a.bias) v += a.bias[j];
        if (a.act == 1) v = tanhf(v);
        else if (a.act == 2) { const float s = tr_sigmoid(v); a.sig[(long)i * a.sig_si + j] = s; v = a.aux[(long)i * a.aux_si + j] * s; }
        *c = v;
    }
}

__global__ __launch_bounds__(256) void k_tr_fold(const float *part, int n_part, int I, int J, float *out, long o_si, long o_sj)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x, n = (long)I * J;
    if (e >= n) return;
    float s = part[e];
    for (int p = 1; p < n_part; p++) s += part[(size_t)p * n + e];
    out[(e / J) * o_si + (e % J) * o_sj] = s;
}

__global__ __launch_bounds__(320) void k_tr_colsum(const float *D, long ld, int M, int N, float *part)
{
    const int j = threadIdx.x, r0 = blockIdx.x * TR_CHUNK, r1 = min(M, r0 + TR_CHUNK);
    if (j >= N) return;
    float s = 0.0f;
    for (int r = r0; r < r1; r++) s += D[(long)r * ld + j];
    part[(size_t)blockIdx.x * N + j] = s;
}

// ---- the recurrence ---------------------------------------------------------------------------------------------------------------------------------------------
#define TS_HP 100      // LDS pitch of a sequence's h: 100 = 4 mod 32, so the 16 x 4 elements a wavefront reads per k-step fall in 32 banks, two lanes each
#define TS_DP 292      // LDS pitch of a sequence's gate-gradient row: 292 = 4 mod 32

__global__ __launch_bounds__(384) void k_tr_scan_fwd(const float *gi, const float *w_hh, const float *b_hh, float *save, int B, int T)
{
    __shared__ float Hs[2][TR_SEQ][TS_HP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
    const int j = 16 * w + c, s0 = blockIdx.x * TR_SEQ;
    float wr[3][24], bh[3], hp[4];
#pragma unroll
    for (int g = 0; g < 3; g++) {                                     // B[k = l >> 4][j = l & 15] = W_hh[g 96 + j][k]
        bh[g] = b_hh[g * TR_H + j];
#pragma unroll
        for (int kk = 0; kk < 24; kk++) wr[g][kk] = w_hh[(size_t)(g * TR_H + j) * TR_H + 4 * kk + q];
    }
#pragma unroll
    for (int r = 0; r < 4; r++) hp[r] = 0.0f;
    for (int e = tid; e < TR_SEQ * TS_HP; e += 384) (&Hs[0][0][0])[e] = 0.0f;
    __syncthreads();
    float gc[4][3], gx[4][3];                                         // gi of this step and of the next: fetched one step ahead, under the products
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int seq = s0 + 4 * q + r;
#pragma unroll
        for (int g = 0; g < 3; g++) gc[r][g] = seq < B ? gi[(size_t)seq * T * TR_G + g * TR_H + j] : 0.0f;
    }
    int cur = 0;
    for (int t = 0; t < T; t++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int seq = s0 + 4 * q + r;
#pragma unroll
            for (int g = 0; g < 3; g++) gx[r][g] = (seq < B && t + 1 < T) ? gi[((size_t)seq * T + t + 1) * TR_G + g * TR_H + j] : 0.0f;
        }
        f32x4 acc[3];
#pragma unroll
        for (int g = 0; g < 3; g++) acc[g] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kk = 0; kk < 24; kk++) {                             // A[i = l & 15][k = l >> 4] = h_{t-1}[sequence i][4 kk + k]
            const float av = Hs[cur][c][4 * kk + q];
#pragma unroll
            for (int g = 0; g < 3; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[g][kk], acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {                                 // C: column = l & 15, row = 4 (l >> 4) + r
            const int seq = s0 + 4 * q + r;
            float h = 0.0f;
            if (seq < B) {
                const size_t row = (size_t)seq * T + t;
                const float rr = tr_sigmoid(gc[r][0] + (acc[0][r] + bh[0]));
                const float zz = tr_sigmoid(gc[r][1] + (acc[1][r] + bh[1]));
                const float hn = acc[2][r] + bh[2];
                const float nn = tanhf(gc[r][2] + rr * hn);
                h = (hp[r] - nn) * zz + nn;
                float *sv = save + row * TR_SAVE + j;
                sv[0] = rr; sv[TR_H] = zz; sv[2 * TR_H] = nn; sv[3 * TR_H] = hn; sv[4 * TR_H] = h;
                hp[r] = h;
            }
            Hs[cur ^ 1][4 * q + r][j] = h;
#pragma unroll
            for (int g = 0; g < 3; g++) gc[r][g] = gx[r][g];
        }
        __syncthreads();                                              // the one hand-over of the step: h_t is in Hs[cur ^ 1]; Hs[cur] is rewritten only after the NEXT barrier
        cur ^= 1;
    }
}

// what the backward step t of one (sequence, unit) reads: r, z, n, hn of row t, h of row t - 1 (zero state ahead of row 0) and the gradient reaching h_t from above
__device__ __forceinline__ void tb_fetch(float *o, const float *save, const float *dh_ext, int seq, int t, int j, int B, int T)
{
    if (seq < B && t >= 0) {
        const size_t row = (size_t)seq * T + t;
        const float *sv = save + row * TR_SAVE + j;
        o[0] = sv[0]; o[1] = sv[TR_H]; o[2] = sv[2 * TR_H]; o[3] = sv[3 * TR_H];
        o[4] = t ? sv[4 * TR_H - TR_SAVE] : 0.0f;
        o[5] = dh_ext[row * TR_H + j];
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = 0.0f;
    }
}

__global__ __launch_bounds__(384) void k_tr_scan_bwd(const float *save, const float *dh_ext, const float *w_hh, float *dg, float *dgh, int B, int T)
{
    __shared__ float Ds[2][TR_SEQ][TS_DP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
    const int j = 16 * w + c, s0 = blockIdx.x * TR_SEQ;
    float wt[72], carry[4];
#pragma unroll
    for (int kk = 0; kk < 72; kk++) wt[kk] = w_hh[(size_t)(4 * kk + q) * TR_H + j];      // B[k = l >> 4][j = l & 15] = W_hh[k][j]
#pragma unroll
    for (int r = 0; r < 4; r++) carry[r] = 0.0f;
    float sc[4][6], sx[4][6];                                         // r, z, n, hn, h_{t-1}, dh of this step and of the next one down: fetched one step ahead
#pragma unroll
    for (int r = 0; r < 4; r++) tb_fetch(sc[r], save, dh_ext, s0 + 4 * q + r, T - 1, j, B, T);
    int cur = 0;
    for (int t = T - 1; t >= 0; t--) {
#pragma unroll
        for (int r = 0; r < 4; r++) tb_fetch(sx[r], save, dh_ext, s0 + 4 * q + r, t - 1, j, B, T);
        float direct[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int seq = s0 + 4 * q + r;
            float drt = 0.0f, dzt = 0.0f, dnr = 0.0f;
            direct[r] = 0.0f;
            if (seq < B) {
                const size_t row = (size_t)seq * T + t;
                const float rr = sc[r][0], zz = sc[r][1], nn = sc[r][2], hn = sc[r][3], hprev = sc[r][4];
                const float dh = sc[r][5] + carry[r];
                const float dnt = dh * (1.0f - zz) * (1.0f - nn * nn);
                dzt = dh * (hprev - nn) * zz * (1.0f - zz);
                drt = dnt * hn * rr * (1.0f - rr);
                dnr = dnt * rr;
                direct[r] = dh * zz;
                float *o = dg + row * TR_G + j, *oh = dgh + row * TR_G + j;
                o[0] = drt; o[TR_H] = dzt; o[2 * TR_H] = dnt;
                oh[0] = drt; oh[TR_H] = dzt; oh[2 * TR_H] = dnr;
            }
            float *d = &Ds[cur][4 * q + r][j];
            d[0] = drt; d[TR_H] = dzt; d[2 * TR_H] = dnr;
        }
        __syncthreads();                                              // the one hand-over of the step; Ds[cur] is rewritten two steps on, behind the next barrier
        f32x4 acc[3];
#pragma unroll
        for (int g = 0; g < 3; g++) acc[g] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kk = 0; kk < 24; kk++)
#pragma unroll
            for (int g = 0; g < 3; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ds[cur][c][g * TR_H + 4 * kk + q], wt[24 * g + kk], acc[g], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            carry[r] = direct[r] + ((acc[0][r] + acc[1][r]) + acc[2][r]);
#pragma unroll
            for (int k = 0; k < 6; k++) sc[r][k] = sx[r][k];
        }
        cur ^= 1;
    }
}

// ---- activation derivatives -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_dtanh(const float *X, const float *dX, int col0, int W, float *D, long n)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long r = e / W; const int c = (int)(e - r * W);
    const float y = X[r * RD_DEC_W + col0 + c];
    D[e] = dX[r * RD_DEC_W + col0 + c] * (1.0f - y * y);
}

__global__ __launch_bounds__(256) void k_tr_glu_bwd(const float *dX, int col0, const float *save, const float *sig, float *da, float *dh, long n)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long r = e / TR_H; const int c = (int)(e - r * TR_H);
    const float g = dX[r * RD_DEC_W + col0 + c], h = save[r * TR_SAVE + 4 * TR_H + c], s = sig[e];
    da[e] = g * h * s * (1.0f - s);
    dh[e] = g * s;
}

// ---- loss -------------------------------------------------------------------------------------------------------------------------------------------------------
// one frame pair (radae_base.py:55-63): y = target row (nf floats), p = decoded row (21 floats); scale = 1 / (B F 18).  The pitch, correlation and data terms are
// added to each of the 18 cepstral columns before the mean, so their gradients carry 18 times the factor: 18 * 3 (10/18) * 2 = 60, 18 * (1/18) * 2 = 2, 18 * (0.5/18) * 2 = 1.
__global__ __launch_bounds__(256) void k_tr_loss_frames(const float *feat, int nf, const float *fhat, float *dfhat, float *frame_loss, long n, float scale)
{
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const float *y = feat + f * nf, *p = fhat + f * (RM_NFEAT + 1);
    float *d = dfhat + f * (RM_NFEAT + 1);
    const float c1 = (float)(3.0 * (10.0 / 18.0)), c2 = (float)(1.0 / 18.0), c3 = (float)(0.5 / 18.0);
    const float pitch = 2.0f * (p[18] - y[18]), corr = p[19] - y[19], data = nf == RM_NFEAT + 1 ? p[RM_NFEAT] - y[RM_NFEAT] : 0.0f;
    float pw = y[19] + 0.5f;
    pw = pw > 0.0f ? pw * pw : 0.0f;                                   // relu(.) ** 2: takes no gradient (it depends on the target alone)
    const float extra = c1 * fabsf(pitch) * pw + c2 * corr * corr + c3 * data * data;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 18; i++) { const float e = p[i] - y[i]; acc += e * e + extra; d[i] = 2.0f * e * scale; }
    frame_loss[f] = acc / 18.0f;
    d[18] = 60.0f * pw * (pitch > 0.0f ? 1.0f : pitch < 0.0f ? -1.0f : 0.0f) * scale;      // sign(0) = 0
    d[19] = 2.0f * corr * scale;
    d[RM_NFEAT] = data * scale;
}

__global__ __launch_bounds__(256) void k_tr_loss_sum(const float *frame_loss, double *loss, int B, int F)
{
    for (int b = threadIdx.x; b < B; b += 256) {
        double s = 0.0;
        for (int f = 0; f < F; f++) s += (double)frame_loss[(size_t)b * F + f];
        loss[b] = s / F;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < B; b++) s += loss[b];
        loss[B] = s / B;
    }
}

// ---- Adam (torch.optim.Adam, betas (0.8, 0.95), eps 1e-8, no weight decay, no amsgrad; train.py:147) ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_adam(float *p, const float *g, float *m, float *v, long n, float step_size, float inv_sqrt_bc2)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float b2 = 0.95f, omb1 = (float)(1.0 - 0.8), omb2 = (float)(1.0 - 0.95), eps = 1e-8f;
    const float gg = g[e];
    const float mm = m[e] + omb1 * (gg - m[e]);
    const float vv = b2 * v[e] + omb2 * gg * gg;
    m[e] = mm; v[e] = vv;
    p[e] = p[e] - step_size * mm / (sqrtf(vv) * inv_sqrt_bc2 + eps);
}

// ---- launch shims -----------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int tr_launch_gemm(const tr_gemm_args *a, rd_stream_t s)
{
    if (a->I <= 0 || a->J <= 0 || a->K <= 0) return 0;
    const int nz = a->k_chunk > 0 ? (a->K + a->k_chunk - 1) / a->k_chunk : 1;
    hipLaunchKernelGGL(k_tr_gemm, dim3((a->J + TG_T - 1) / TG_T, (a->I + TG_T - 1) / TG_T, nz), dim3(256), 0, (hipStream_t)s, *a);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_fold(const float *part, int n_part, int I, int J, float *out, long o_si, long o_sj, rd_stream_t s)
{
    hipLaunchKernelGGL(k_tr_fold, dim3(((long)I * J + 255) / 256), dim3(256), 0, (hipStream_t)s, part, n_part, I, J, out, o_si, o_sj);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_colsum(const float *D, long ld, int M, int N, float *part, rd_stream_t s)
{
    if (N > 320) return -1;
    hipLaunchKernelGGL(k_tr_colsum, dim3((M + TR_CHUNK - 1) / TR_CHUNK), dim3(320), 0, (hipStream_t)s, D, ld, M, N, part);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_scan_fwd(const float *gi, const float *w_hh, const float *b_hh, float *save, int B, int T, rd_stream_t s)
{
    hipLaunchKernelGGL(k_tr_scan_fwd, dim3((B + TR_SEQ - 1) / TR_SEQ), dim3(384), 0, (hipStream_t)s, gi, w_hh, b_hh, save, B, T);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_scan_bwd(const float *save, const float *dh_ext, const float *w_hh, float *dg, float *dgh, int B, int T, rd_stream_t s)
{
    hipLaunchKernelGGL(k_tr_scan_bwd, dim3((B + TR_SEQ - 1) / TR_SEQ), dim3(384), 0, (hipStream_t)s, save, dh_ext, w_hh, dg, dgh, B, T);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_dtanh(const float *X, const float *dX, int col0, int W, float *D, long M, rd_stream_t s)
{
    const long n = M * W;
    hipLaunchKernelGGL(k_tr_dtanh, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, X, dX, col0, W, D, n);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_glu_bwd(const float *dX, int col0, const float *save, const float *sig, float *da, float *dh, long M, rd_stream_t s)
{
    const long n = M * TR_H;
    hipLaunchKernelGGL(k_tr_glu_bwd, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, dX, col0, save, sig, da, dh, n);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_loss(const float *feat, int nf, const float *fhat, float *dfhat, float *frame_loss, double *loss, int B, int F, rd_stream_t s)
{
    const long n = (long)B * F;
    hipLaunchKernelGGL(k_tr_loss_frames, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, feat, nf, fhat, dfhat, frame_loss, n, (float)(1.0 / ((double)n * 18.0)));
    hipLaunchKernelGGL(k_tr_loss_sum, dim3(1), dim3(256), 0, (hipStream_t)s, frame_loss, loss, B, F);
    return (int)hipGetLastError();
}

extern "C" int tr_launch_adam(float *p, const float *g, float *m, float *v, long n, float step_size, float inv_sqrt_bc2, rd_stream_t s)
{
    hipLaunchKernelGGL(k_tr_adam, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, p, g, m, v, n, step_size, inv_sqrt_bc2);
    return (int)hipGetLastError();
}
