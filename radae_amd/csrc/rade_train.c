/*
 * rade_train.c -- the rade_train_* section of include/rade_batch.h: the handle that owns the activation workspace of one decoder training step, the table that lays
 * the decoder's parameters out in the caller's flat buffers, and the sequencing of the forward pass, the loss, the backward pass and Adam over the kernels of
 * rade_train.hip.  Rows of every workspace buffer are r = b T + t with the T of the call, dense, so a call below the handle's capacity gives the bits of a handle
 * opened at exactly that size.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rade_batch.h"
#include "rade_train.h"

#define TR_NPARAM (2 + 7 * TR_NL + 2)

typedef struct { char name[32]; long offset; int rows, cols; } tr_param;
static tr_param tr_table[TR_NPARAM];
static long tr_total;

static void tr_build_table(void)
{
    if (tr_total) return;
    int n = 0; long off = 0;
#define ADD(r, c, ...) do { snprintf(tr_table[n].name, sizeof tr_table[n].name, __VA_ARGS__); tr_table[n].offset = off; tr_table[n].rows = (r); tr_table[n].cols = (c); off += (long)(r) * (c); n++; } while (0)
    ADD(TR_H, RD_LATENT, "dec_dense1.w"); ADD(TR_H, 1, "dec_dense1.b");
    for (int l = 0; l < TR_NL; l++) {
        const int kg = RM_DEC_GRU_IN(l);          /* width of the concat buffer the GRU reads; its conv reads TR_H more (the GLU) */
        ADD(TR_G, kg, "dec_gru[%d].w_ih", l); ADD(TR_G, TR_H, "dec_gru[%d].w_hh", l); ADD(TR_G, 1, "dec_gru[%d].b_ih", l); ADD(TR_G, 1, "dec_gru[%d].b_hh", l);
        ADD(TR_H, TR_H, "dec_glu[%d].w", l); ADD(TR_CONV, 2 * (kg + TR_H), "dec_conv[%d].w", l); ADD(TR_CONV, 1, "dec_conv[%d].b", l);
    }
    ADD(TR_OUT, RD_DEC_W, "dec_output.w"); ADD(TR_OUT, 1, "dec_output.b");
#undef ADD
    tr_total = off;
}

/* offsets inside the flat buffers */
enum { P_D1W, P_D1B, P_L0, P_OUTW = 2 + 7 * TR_NL, P_OUTB };
enum { L_WIH, L_WHH, L_BIH, L_BHH, L_GLU, L_CW, L_CB };
static long tr_off(int i) { return tr_table[i].offset; }
static long tr_loff(int l, int k) { return tr_table[P_L0 + 7 * l + k].offset; }

/* phases of a step, as rade_train_profile_get reports them */
enum { PH_FWD_GEMM, PH_FWD_SCAN, PH_LOSS, PH_BWD_SCAN, PH_BWD_GEMM, PH_ADAM, TR_NPHASE };
#define TR_MAXEV 512

struct rade_train {
    int max_B, max_T, nf, device;
    int prof, n_ev, ev_open, ev_made, ev_phase[TR_MAXEV];       /* profiling: pairs of events around each phase's launches, read by rade_train_profile_get */
    hipEvent_t ev0[TR_MAXEV], ev1[TR_MAXEV];
    int B, T;                          /* of the last forward call; 0: none yet */
    int have_loss;
    float *zin, *x, *dx, *gi, *save[TR_NL], *sig[TR_NL], *y, *dy, *dg, *dgh, *da, *dh, *dc, *part, *frame_loss;
};

long rade_train_n_floats(void) { tr_build_table(); return tr_total; }
int rade_train_n_params(void) { return TR_NPARAM; }

int rade_train_param(int i, const char **name, long *offset, int *rows, int *cols)
{
    tr_build_table();
    if (i < 0 || i >= TR_NPARAM) return -1;
    if (name) *name = tr_table[i].name;
    if (offset) *offset = tr_table[i].offset;
    if (rows) *rows = tr_table[i].rows;
    if (cols) *cols = tr_table[i].cols;
    return 0;
}

static float *tr_alloc(size_t n_floats)
{
    void *p = NULL;
    return hipMalloc(&p, sizeof(float) * n_floats) == hipSuccess ? p : NULL;
}

rade_train *rade_train_open(int max_B, int max_T, int n_features, int device)
{
    int ndev = 0;
    if (max_B <= 0 || max_T <= 0 || (n_features != RM_NFEAT && n_features != RM_NFEAT + 1) || device < 0 || (long)max_B * max_T > TR_MAX_ROWS) {
        fprintf(stderr, "rade_train_open: need max_B, max_T > 0, max_B max_T <= 2^21 and 20 or 21 features\n"); return NULL;
    }
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { fprintf(stderr, "rade_train_open: no usable GPU (this library has no CPU path)\n"); return NULL; }
    if (hipSetDevice(device) != hipSuccess) return NULL;
    tr_build_table();
    rade_train *h = calloc(1, sizeof *h);
    if (!h) return NULL;
    h->max_B = max_B; h->max_T = max_T; h->nf = n_features; h->device = device;
    const size_t M = (size_t)max_B * max_T, n_chunk = (M + TR_CHUNK - 1) / TR_CHUNK;
    int ok = 1;
#define GET(field, n) do { h->field = tr_alloc(n); ok = ok && h->field; } while (0)
    GET(zin, M * RD_LATENT); GET(x, M * RD_DEC_W); GET(dx, M * RD_DEC_W); GET(gi, M * TR_G); GET(y, M * TR_OUT); GET(dy, M * TR_OUT);
    GET(dg, M * TR_G); GET(dgh, M * TR_G); GET(da, M * TR_H); GET(dh, M * TR_H); GET(dc, M * TR_H); GET(frame_loss, M * 4);
    GET(part, n_chunk * TR_G * RD_DEC_W);                            /* the largest weight gradient is smaller: TR_G x RM_DEC_GRU_IN(TR_NL - 1) */
    for (int l = 0; l < TR_NL; l++) { GET(save[l], M * TR_SAVE); GET(sig[l], M * TR_H); }
#undef GET
    if (!ok) { rade_train_close(h); return NULL; }
    return h;
}

void rade_train_close(rade_train *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    float *all[] = { h->zin, h->x, h->dx, h->gi, h->y, h->dy, h->dg, h->dgh, h->da, h->dh, h->dc, h->frame_loss, h->part };
    for (size_t i = 0; i < sizeof all / sizeof all[0]; i++) (void)hipFree(all[i]);
    for (int l = 0; l < TR_NL; l++) { (void)hipFree(h->save[l]); (void)hipFree(h->sig[l]); }
    if (h->ev_made) for (int i = 0; i < TR_MAXEV; i++) { (void)hipEventDestroy(h->ev0[i]); (void)hipEventDestroy(h->ev1[i]); }
    free(h);
}

static void ph_begin(rade_train *h, int phase, void *stream)
{
    if (!h->prof || h->n_ev >= TR_MAXEV) return;
    h->ev_phase[h->n_ev] = phase; h->ev_open = 1;
    (void)hipEventRecord(h->ev0[h->n_ev], (hipStream_t)stream);
}

static void ph_end(rade_train *h, void *stream)
{
    if (!h->ev_open) return;
    (void)hipEventRecord(h->ev1[h->n_ev++], (hipStream_t)stream); h->ev_open = 0;
}

int rade_train_profile(rade_train *h, int on)
{
    if (!h) return -1;
    (void)hipSetDevice(h->device);
    if (on && !h->ev_made) {
        for (int i = 0; i < TR_MAXEV; i++) if (hipEventCreate(&h->ev0[i]) != hipSuccess || hipEventCreate(&h->ev1[i]) != hipSuccess) return -2;
        h->ev_made = 1;
    }
    h->prof = on != 0; h->n_ev = 0; h->ev_open = 0;
    return 0;
}

int rade_train_profile_get(rade_train *h, double *ms_out)
{
    if (!h || !ms_out) return -1;
    (void)hipSetDevice(h->device);
    for (int k = 0; k < TR_NPHASE; k++) ms_out[k] = 0.0;
    const int n = h->n_ev;
    for (int i = 0; i < n; i++) {
        float ms = 0.0f;
        if (hipEventSynchronize(h->ev1[i]) != hipSuccess || hipEventElapsedTime(&ms, h->ev0[i], h->ev1[i]) != hipSuccess) return -2;
        ms_out[h->ev_phase[i]] += ms;
    }
    h->n_ev = 0;
    return n;
}

static int aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

/* Y = act(A W^T + b (+ old Y)): A [M][K] at pitch lda (shift: row t - 1), W [N][K] with element (n, k) at W[n w_sn + k w_sk] */
static int fwd_gemm(rd_stream_t s, int M, int T, const float *A, long lda, int shift, const float *W, long w_sn, long w_sk, const float *bias, int N, int K,
                    float *Y, long ldy, int beta, int act, const float *aux, long aux_ld, float *sig)
{
    tr_gemm_args g = { .A = A, .a_si = lda, .a_sk = 1, .a_shift = shift, .B = W, .b_sk = w_sk, .b_sj = w_sn, .C = Y, .c_si = ldy, .c_sj = 1, .bias = bias,
                       .aux = aux, .aux_si = aux_ld, .sig = sig, .sig_si = TR_H, .I = M, .J = N, .K = K, .T = T, .beta = beta, .act = act };
    return tr_launch_gemm(&g, s);
}

/* dX[:, :K] (+)= dY W: dY [M][N] at pitch ldd, W (n, k) at W[n w_sn + k w_sk]; shift: row r's product goes to row r - 1 of the same sequence */
static int dx_gemm(rd_stream_t s, int M, int T, const float *dY, long ldd, int N, const float *W, long w_sn, long w_sk, int K, float *dX, long ldx, int beta, int shift)
{
    tr_gemm_args g = { .A = dY, .a_si = ldd, .a_sk = 1, .B = W, .b_sk = w_sn, .b_sj = w_sk, .C = dX, .c_si = ldx, .c_sj = 1, .c_shift = shift,
                       .I = M, .J = K, .K = N, .T = T, .beta = beta };
    return tr_launch_gemm(&g, s);
}

/* dW = dY^T X in chunks of TR_CHUNK rows, folded in chunk order; dW (n, k) goes to dW[n w_sn + k w_sk]; db = the column sums of dY the same way (db NULL: none) */
static int dw_gemm(rade_train *h, rd_stream_t s, int M, int T, const float *dY, long ldd, int N, const float *X, long ldx, int shift, int K, float *dW, long w_sn, long w_sk, float *db)
{
    const int n_chunk = (M + TR_CHUNK - 1) / TR_CHUNK;
    tr_gemm_args g = { .A = dY, .a_si = 1, .a_sk = ldd, .B = X, .b_sk = ldx, .b_sj = 1, .b_shift = shift, .C = h->part, .c_si = K, .c_sj = 1,
                       .I = N, .J = K, .K = M, .T = T, .k_chunk = TR_CHUNK };
    int rc = tr_launch_gemm(&g, s);
    if (!rc) rc = tr_launch_fold(h->part, n_chunk, N, K, dW, w_sn, w_sk, s);
    if (!rc && db) {
        rc = tr_launch_colsum(dY, ldd, M, N, h->part, s);
        if (!rc) rc = tr_launch_fold(h->part, n_chunk, 1, N, db, 0, 1, s);
    }
    return rc;
}

#define TRY(e) do { int rc_ = (e); if (rc_) return rc_ < 0 ? rc_ : -2; } while (0)

int rade_train_dec_forward(rade_train *h, const float *params_dev, const float *z_hat_dev, int B, int T, float *features_hat_dev, void *stream)
{
    if (!h || !params_dev || !z_hat_dev || B <= 0 || T <= 0 || B > h->max_B || T > h->max_T) return -1;
    if (!aligned4(params_dev) || !aligned4(z_hat_dev) || !aligned4(features_hat_dev)) return -1;
    (void)hipSetDevice(h->device);
    const int M = B * T;
    const float *P = params_dev;
    h->B = 0; h->have_loss = 0;
    ph_begin(h, PH_FWD_GEMM, stream);
    if (hipMemcpyAsync(h->zin, z_hat_dev, sizeof(float) * (size_t)M * RD_LATENT, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return -2;
    TRY(fwd_gemm(stream, M, T, h->zin, RD_LATENT, 0, P + tr_off(P_D1W), RD_LATENT, 1, P + tr_off(P_D1B), TR_H, RD_LATENT, h->x, RD_DEC_W, 0, 1, NULL, 0, NULL));
    for (int l = 0; l < TR_NL; l++) {
        const int kg = RM_DEC_GRU_IN(l), kc = RM_DEC_CONV_IN(l);
        TRY(fwd_gemm(stream, M, T, h->x, RD_DEC_W, 0, P + tr_loff(l, L_WIH), kg, 1, P + tr_loff(l, L_BIH), TR_G, kg, h->gi, TR_G, 0, 0, NULL, 0, NULL));
        ph_end(h, stream); ph_begin(h, PH_FWD_SCAN, stream);
        TRY(tr_launch_scan_fwd(h->gi, P + tr_loff(l, L_WHH), P + tr_loff(l, L_BHH), h->save[l], B, T, stream));
        ph_end(h, stream); ph_begin(h, PH_FWD_GEMM, stream);
        const float *hh = h->save[l] + 4 * TR_H;
        TRY(fwd_gemm(stream, M, T, hh, TR_SAVE, 0, P + tr_loff(l, L_GLU), TR_H, 1, NULL, TR_H, TR_H, h->x + kg, RD_DEC_W, 0, 2, hh, TR_SAVE, h->sig[l]));
        const float *cw = P + tr_loff(l, L_CW);                       /* [TR_CONV][kc][2]: tap 0 is the older row */
        TRY(fwd_gemm(stream, M, T, h->x, RD_DEC_W, 1, cw, 2 * kc, 2, NULL, TR_CONV, kc, h->x + kc, RD_DEC_W, 0, 0, NULL, 0, NULL));
        TRY(fwd_gemm(stream, M, T, h->x, RD_DEC_W, 0, cw + 1, 2 * kc, 2, P + tr_loff(l, L_CB), TR_CONV, kc, h->x + kc, RD_DEC_W, 1, 1, NULL, 0, NULL));
    }
    TRY(fwd_gemm(stream, M, T, h->x, RD_DEC_W, 0, P + tr_off(P_OUTW), RD_DEC_W, 1, P + tr_off(P_OUTB), TR_OUT, RD_DEC_W, h->y, TR_OUT, 0, 0, NULL, 0, NULL));
    if (features_hat_dev && hipMemcpyAsync(features_hat_dev, h->y, sizeof(float) * (size_t)M * TR_OUT, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return -2;
    ph_end(h, stream);
    h->B = B; h->T = T;
    return 0;
}

int rade_train_saved_x(rade_train *h, float *x_out_dev, void *stream)
{
    if (!h || !x_out_dev || !h->B || !aligned4(x_out_dev)) return -1;
    (void)hipSetDevice(h->device);
    return hipMemcpyAsync(x_out_dev, h->x, sizeof(float) * (size_t)h->B * h->T * RD_DEC_W, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int rade_train_loss(rade_train *h, const float *features_dev, float *dfeatures_hat_dev, double *loss_dev, void *stream)
{
    if (!h || !features_dev || !loss_dev || !h->B || !aligned4(features_dev) || !aligned4(dfeatures_hat_dev) || ((uintptr_t)loss_dev & 7)) return -1;
    (void)hipSetDevice(h->device);
    ph_begin(h, PH_LOSS, stream);
    TRY(tr_launch_loss(features_dev, h->nf, h->y, h->dy, h->frame_loss, loss_dev, h->B, 4 * h->T, stream));
    ph_end(h, stream);
    if (dfeatures_hat_dev && hipMemcpyAsync(dfeatures_hat_dev, h->dy, sizeof(float) * (size_t)h->B * h->T * TR_OUT, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return -2;
    h->have_loss = 1;
    return 0;
}

int rade_train_dec_backward(rade_train *h, const float *params_dev, const float *dfeatures_hat_dev, float *grads_dev, float *dz_hat_dev, void *stream)
{
    if (!h || !params_dev || !grads_dev || !h->B || (!dfeatures_hat_dev && !h->have_loss)) return -1;
    if (!aligned4(params_dev) || !aligned4(dfeatures_hat_dev) || !aligned4(grads_dev) || !aligned4(dz_hat_dev)) return -1;
    (void)hipSetDevice(h->device);
    const int B = h->B, T = h->T, M = B * T;
    const float *P = params_dev, *dy = dfeatures_hat_dev ? dfeatures_hat_dev : h->dy;
    float *G = grads_dev;
    ph_begin(h, PH_BWD_GEMM, stream);
    /* output layer: the first writer of every column of dx */
    TRY(dw_gemm(h, stream, M, T, dy, TR_OUT, TR_OUT, h->x, RD_DEC_W, 0, RD_DEC_W, G + tr_off(P_OUTW), RD_DEC_W, 1, G + tr_off(P_OUTB)));
    TRY(dx_gemm(stream, M, T, dy, TR_OUT, TR_OUT, P + tr_off(P_OUTW), RD_DEC_W, 1, RD_DEC_W, h->dx, RD_DEC_W, 0, 0));
    for (int l = TR_NL - 1; l >= 0; l--) {
        const int kg = RM_DEC_GRU_IN(l), kc = RM_DEC_CONV_IN(l);
        /* conv: tap 1 reads row t, tap 0 row t - 1 */
        const float *cw = P + tr_loff(l, L_CW);
        float *gcw = G + tr_loff(l, L_CW);
        TRY(tr_launch_dtanh(h->x, h->dx, kc, TR_CONV, h->dc, M, stream));
        TRY(dw_gemm(h, stream, M, T, h->dc, TR_CONV, TR_CONV, h->x, RD_DEC_W, 1, kc, gcw, 2 * kc, 2, NULL));
        TRY(dw_gemm(h, stream, M, T, h->dc, TR_CONV, TR_CONV, h->x, RD_DEC_W, 0, kc, gcw + 1, 2 * kc, 2, G + tr_loff(l, L_CB)));
        TRY(dx_gemm(stream, M, T, h->dc, TR_CONV, TR_CONV, cw + 1, 2 * kc, 2, kc, h->dx, RD_DEC_W, 1, 0));
        TRY(dx_gemm(stream, M, T, h->dc, TR_CONV, TR_CONV, cw, 2 * kc, 2, kc, h->dx, RD_DEC_W, 1, 1));
        /* GLU */
        const float *hh = h->save[l] + 4 * TR_H;
        TRY(tr_launch_glu_bwd(h->dx, kg, h->save[l], h->sig[l], h->da, h->dh, M, stream));
        TRY(dw_gemm(h, stream, M, T, h->da, TR_H, TR_H, hh, TR_SAVE, 0, TR_H, G + tr_loff(l, L_GLU), TR_H, 1, NULL));
        TRY(dx_gemm(stream, M, T, h->da, TR_H, TR_H, P + tr_loff(l, L_GLU), TR_H, 1, TR_H, h->dh, TR_H, 1, 0));
        /* GRU: back through time, then the products over all rows */
        ph_end(h, stream); ph_begin(h, PH_BWD_SCAN, stream);
        TRY(tr_launch_scan_bwd(h->save[l], h->dh, P + tr_loff(l, L_WHH), h->dg, h->dgh, B, T, stream));
        ph_end(h, stream); ph_begin(h, PH_BWD_GEMM, stream);
        TRY(dw_gemm(h, stream, M, T, h->dg, TR_G, TR_G, h->x, RD_DEC_W, 0, kg, G + tr_loff(l, L_WIH), kg, 1, G + tr_loff(l, L_BIH)));
        TRY(dw_gemm(h, stream, M, T, h->dgh, TR_G, TR_G, hh, TR_SAVE, 1, TR_H, G + tr_loff(l, L_WHH), TR_H, 1, G + tr_loff(l, L_BHH)));
        TRY(dx_gemm(stream, M, T, h->dg, TR_G, TR_G, P + tr_loff(l, L_WIH), kg, 1, kg, h->dx, RD_DEC_W, 1, 0));
    }
    TRY(tr_launch_dtanh(h->x, h->dx, 0, TR_H, h->dc, M, stream));
    TRY(dw_gemm(h, stream, M, T, h->dc, TR_H, TR_H, h->zin, RD_LATENT, 0, RD_LATENT, G + tr_off(P_D1W), RD_LATENT, 1, G + tr_off(P_D1B)));
    if (dz_hat_dev) TRY(dx_gemm(stream, M, T, h->dc, TR_H, TR_H, P + tr_off(P_D1W), RD_LATENT, 1, RD_LATENT, dz_hat_dev, RD_LATENT, 0, 0));
    ph_end(h, stream);
    return 0;
}

int rade_train_adam(rade_train *h, float *params_dev, const float *grads_dev, float *m_dev, float *v_dev, double lr, double bias_correction1, double bias_correction2, void *stream)
{
    if (!h || !params_dev || !grads_dev || !m_dev || !v_dev || !(bias_correction1 > 0) || !(bias_correction2 > 0)) return -1;
    if (!aligned4(params_dev) || !aligned4(grads_dev) || !aligned4(m_dev) || !aligned4(v_dev)) return -1;
    (void)hipSetDevice(h->device);
    ph_begin(h, PH_ADAM, stream);
    TRY(tr_launch_adam(params_dev, grads_dev, m_dev, v_dev, rade_train_n_floats(), (float)(lr / bias_correction1), (float)(1.0 / sqrt(bias_correction2)), stream));
    ph_end(h, stream);
    return 0;
}

int rade_train_dec_step(rade_train *h, float *params_dev, float *grads_dev, float *m_dev, float *v_dev, const float *z_hat_dev, const float *features_dev, int B, int T,
                        double *loss_dev, double lr, double bias_correction1, double bias_correction2, void *stream)
{
    if (!h || !params_dev || !grads_dev || !m_dev || !v_dev || !z_hat_dev || !features_dev || !loss_dev || !(bias_correction1 > 0) || !(bias_correction2 > 0)) return -1;
    if (!aligned4(features_dev) || !aligned4(grads_dev) || !aligned4(m_dev) || !aligned4(v_dev) || ((uintptr_t)loss_dev & 7)) return -1;
    TRY(rade_train_dec_forward(h, params_dev, z_hat_dev, B, T, NULL, stream));
    TRY(rade_train_loss(h, features_dev, NULL, loss_dev, stream));
    TRY(rade_train_dec_backward(h, params_dev, NULL, grads_dev, NULL, stream));
    return rade_train_adam(h, params_dev, grads_dev, m_dev, v_dev, lr, bias_correction1, bias_correction2, stream);
}
