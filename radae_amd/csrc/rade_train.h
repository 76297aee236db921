/*
 * rade_train.h -- launch shims between rade_train.c (plain C: the handle, the parameter table, the sequencing of a training step) and rade_train.hip (the kernels).
 * Everything here is POD, as in rade_dev.h.
 */
#ifndef RADE_TRAIN_H
#define RADE_TRAIN_H

#include "rade_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the decoder's shapes under the names the training code uses (rade_model_geom.h); the kernels' tiling assumes them (rade_train.hip) */
#define TR_H        RM_DEC_H        /* GRU hidden units */
#define TR_G        RM_DEC_G        /* three gates, torch's order r, z, n */
#define TR_SAVE     (5 * TR_H)      /* saved planes of a GRU row: r, z, n, hn = W_hn h + b_hn, h */
#define TR_OUT      RM_FEAT_AUX     /* 4 frames x 21 features */
#define TR_NL       RM_NL
#define TR_CONV     RM_DEC_CONV
static_assert(RM_DEC_D1 == TR_H && RM_DEC_GLU == TR_H, "dense1 and the GLU are as wide as a GRU: one TR_H-wide buffer (dc, da, dh) serves each");
#define TR_SEQ      16     /* sequences per workgroup of the scans: the M dimension of mfma_f32_16x16x4f32 */
#define TR_CHUNK    256    /* rows of M = B T per partial sum of a weight gradient */
#define TR_MAX_ROWS (1L << 21) /* rows of a handle: the GEMMs put the 64-row tiles on grid.y (at most 65535), and the workspace is 22 KB per row */

/* C(i, j) (+)= act(sum_k A(i, k) B(k, j) + bias[j]) with every operand reached through two strides, so that the three forms of a layer's feed-forward work
 * are one kernel:   Y = X W^T + b        A = X [M][K],     B(k, j) = W[j][k]
 *                   dX (+)= dY W         A = dY [M][N],    B(k, j) = W[k][j]
 *                   dW = dY^T X          A(i, k) = dY[k][i], B = X [M][K]: the sum runs over M, in chunks of TR_CHUNK rows (k_chunk > 0), one partial per chunk
 * shift: the operand (or C) is taken one row of M earlier, and is zero (dropped) for the first row of a sequence (row % T == 0): the conv's older tap, h_{t-1}.
 * The axis that is M: a_shift on i, b_shift on k, c_shift on i. */
typedef struct {
    const float *A; long a_si, a_sk; int a_shift;
    const float *B; long b_sk, b_sj; int b_shift;
    float *C; long c_si, c_sj; int c_shift;
    const float *bias;                 /* optional [J] */
    const float *aux; long aux_si;     /* act 2: C = aux(i, j) * sigmoid(acc), and the sigmoid goes to sig(i, j) */
    float *sig; long sig_si;
    int I, J, K, T;
    int beta;                          /* 1: the old C is added to the sum before bias and act */
    int act;                           /* 0 none, 1 tanh, 2 GLU */
    int k_chunk;                       /* > 0: blockIdx.z takes k in [z k_chunk, (z + 1) k_chunk) and writes C + z I J as a dense [I][J] */
} tr_gemm_args;
int tr_launch_gemm(const tr_gemm_args *a, rd_stream_t s);
/* out(i, j) = part[0][i][j] + part[1][i][j] + ... in that order (n_part dense [I][J] partials) */
int tr_launch_fold(const float *part, int n_part, int I, int J, float *out, long o_si, long o_sj, rd_stream_t s);
/* part[c][j] = sum over the rows of chunk c of D[row][j], rows in order; D is [M][N] at pitch ld */
int tr_launch_colsum(const float *D, long ld, int M, int N, float *part, rd_stream_t s);
int tr_launch_scan_fwd(const float *gi, const float *w_hh, const float *b_hh, float *save, int B, int T, rd_stream_t s);
int tr_launch_scan_bwd(const float *save, const float *dh_ext, const float *w_hh, float *dg, float *dgh, int B, int T, rd_stream_t s);
/* D[r][c] = dX[r][col0 + c] (1 - X[r][col0 + c]^2), c < W: back through a tanh whose output sits in the concat buffer */
int tr_launch_dtanh(const float *X, const float *dX, int col0, int W, float *D, long M, rd_stream_t s);
/* GLU g = h sigmoid(a): da = dg h s (1 - s), dh = dg s; dg = dX[r][col0 + c] */
int tr_launch_glu_bwd(const float *dX, int col0, const float *save, const float *sig, float *da, float *dh, long M, rd_stream_t s);
/* distortion_loss and its gradient: frame_loss [B][F] float32, dfhat [B][F][21] (column 20 is 0 with 20 features); then loss[b] = the mean of its frames, added in
 * double in frame order, and loss[B] = the mean of loss[0 .. B - 1] in stream order */
int tr_launch_loss(const float *feat, int nf, const float *fhat, float *dfhat, float *frame_loss, double *loss, int B, int F, rd_stream_t s);
int tr_launch_adam(float *p, const float *g, float *m, float *v, long n, float step_size, float inv_sqrt_bc2, rd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
