/*
 * rade_host.c -- host-side (plain C) model preparation for the HIP engine:
 *   1. constant tables of the OFDM modem (rd_tables), evaluated with the same float32/float64 steps
 *      NumPy/PyTorch take in the reference so the device kernels see bit-comparable constants;
 *   2. DNNw weight-blob reader -> fp32 matrices (the blob is int8 + per-row scales for most layers);
 *   3. (the weights and constant tables in the matrix cores' fragment order: rade_pack.c)
 *   4. the fractional resampler's Q32.32 time base and its windowed-sinc taps (rade_batch_resample).
 *   5. the rational rate converter's ratio, taps and output count (rade_batch_rate_convert).
 *   6. the analog FM stage's noise level, least-squares filter design and folded de-emphasis (rade_batch_fm_mod / rade_batch_fm_demod).
 *   7. the C/No estimator's plan, table and host arithmetic, and the chirp header (rade_batch_cno_est, rade_chirp).
 *   8. whole-file acquisition: the hop count, the state machine and the --acq_test statistics of rx.py (rade_acq_hops, rade_acq_track, rade_acq_stats).
 *
 * Reference: radae/radae.py:128-234 (numerology/DFT/pilots/EOO), radae/dsp.py:40-61 (BPF),
 * :153-176 (p_w), :400-416 (Pmat); blob format src/write_rade_weights.c:51-74 and
 * weight-exchange/wexchange/c_export/common.py:59-69,140-176,263-271,290-293,307-311,360-368.
 */
#include "rade_host.h"
#include "rade_batch.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define PI_D 3.14159265358979323846

/* ---------------------------------------------------------------------------------------------
 * 1. tables
 * -------------------------------------------------------------------------------------------*/
static void pa_limit_host(float *re, float *im)
{   /* tanh(|x|)*exp(1j*angle(x)) in float32 (radae.py:218) */
    float mag = hypotf(*re, *im), ang = atan2f(*im, *re), t = tanhf(mag);
    *re = t * cosf(ang); *im = t * sinf(ang);
}

void rd_tables_fill(rd_tables *T)
{
    static const float barker13[13] = { 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1 };
    float w[RD_NC];
    memset(T, 0, sizeof *T);
    /* w = 2*pi*(15+arange(30))/160 as float32 tensor arithmetic (radae.py:172-174) */
    const float two_pi = (float)(2.0 * PI_D);
    for (int c = 0; c < RD_NC; c++) w[c] = (two_pi * (float)(15 + c)) / 160.0f;
    for (int c = 0; c < RD_NC; c++)
        for (int n = 0; n < RD_M; n++) {
            const float arg = (float)n * w[c];          /* float32 product, then exp(1j*arg) in float32 */
            const float cs = (float)cos((double)arg), sn = (float)sin((double)arg);
            T->Winv[c][n][0] = cs / 160.0f; T->Winv[c][n][1] = sn / 160.0f;
            T->Wfwd[n][c][0] = cs; T->Wfwd[n][c][1] = -sn;
        }
    const float r2 = (float)sqrt(2.0);
    for (int c = 0; c < RD_NC; c++) { T->P[c] = r2 * barker13[c % 13]; T->Pend[c] = (c & 1) ? -T->P[c] : T->P[c]; }
    for (int n = 0; n < RD_M; n++) {                    /* p = P @ Winv, pend = Pend @ Winv (complex64) */
        float ar = 0, ai = 0, br = 0, bi = 0;
        for (int c = 0; c < RD_NC; c++) {
            const float wr = T->Winv[c][n][0], wi = T->Winv[c][n][1];
            ar += T->P[c] * wr - 0.0f * wi; ai += T->P[c] * wi + 0.0f * wr;
            br += T->Pend[c] * wr - 0.0f * wi; bi += T->Pend[c] * wi + 0.0f * wr;
        }
        T->p[n][0] = ar; T->p[n][1] = ai; T->pend[n][0] = br; T->pend[n][1] = bi;
    }
    T->pilot_gain = (float)(pow(10.0, -2.0 / 20.0) * 160.0 / sqrt(30.0));
    /* default EOO frame: [p_cp][pend_cp][0][0][0][pend_cp] * pilot_gain, PA-limited */
    for (int n = 0; n < RD_SYM; n++) {
        const int src = n < RD_NCP ? RD_M - RD_NCP + n : n - RD_NCP;
        T->eoo[n][0] = T->p[src][0]; T->eoo[n][1] = T->p[src][1];
        T->eoo[RD_SYM + n][0] = T->pend[src][0]; T->eoo[RD_SYM + n][1] = T->pend[src][1];
        T->eoo[RD_NMF + n][0] = T->pend[src][0]; T->eoo[RD_NMF + n][1] = T->pend[src][1];
    }
    for (int n = 0; n < RD_NEOO; n++) { T->eoo[n][0] *= T->pilot_gain; T->eoo[n][1] *= T->pilot_gain; pa_limit_host(&T->eoo[n][0], &T->eoo[n][1]); }
    /* 3-pilot least-squares matrices Pmat[c] = inv(A^T A) A^T with A = [[1, e^{-j w a}]] (plain transpose) */
    for (int c = 0; c < RD_NC; c++) {
        const int cm = c == 0 ? 1 : (c == RD_NC - 1 ? RD_NC - 2 : c);
        double er[3], ei[3];
        for (int k = 0; k < 3; k++) { const float ang = -(w[cm - 1 + k] * 20.0f); er[k] = (float)cos((double)ang); ei[k] = (float)sin((double)ang); }
        double s1r = er[0] + er[1] + er[2], s1i = ei[0] + ei[1] + ei[2], s2r = 0, s2i = 0;
        for (int k = 0; k < 3; k++) { s2r += er[k] * er[k] - ei[k] * ei[k]; s2i += 2 * er[k] * ei[k]; }
        double dr = 3 * s2r - (s1r * s1r - s1i * s1i), di = 3 * s2i - 2 * s1r * s1i;
        double dn = dr * dr + di * di, ir = dr / dn, ii = -di / dn;
        for (int k = 0; k < 3; k++) {
            double a0r = s2r - (s1r * er[k] - s1i * ei[k]), a0i = s2i - (s1r * ei[k] + s1i * er[k]);
            double a1r = 3 * er[k] - s1r, a1i = 3 * ei[k] - s1i;
            T->Pmat[c][0][k][0] = (float)(ir * a0r - ii * a0i); T->Pmat[c][0][k][1] = (float)(ir * a0i + ii * a0r);
            T->Pmat[c][1][k][0] = (float)(ir * a1r - ii * a1i); T->Pmat[c][1][k][1] = (float)(ir * a1i + ii * a1r);
        }
        const float ang = -(w[c] * 20.0f);
        T->eq_rot[c][0] = (float)cos((double)ang); T->eq_rot[c][1] = (float)sin((double)ang);
    }
    /* input band-pass filter: 101-tap sinc low-pass at baseband, float32 like NumPy builds it */
    const float bandwidth = ((1.2f * (w[RD_NC - 1] - w[0])) * 8000.0f) / two_pi;
    const float centre = (((w[RD_NC - 1] + w[0]) * 8000.0f) / two_pi) / 2.0f;
    const float Bn = bandwidth / 8000.0f, alpha = (two_pi * centre) / 8000.0f;
    for (int i = 0; i < RD_NTAP; i++) {
        const float x = (float)(i - 50) * Bn;
        const float y = (float)PI_D * (x == 0.0f ? 1.0e-20f : x);
        T->bpf_h[i] = Bn * ((float)sin((double)y) / y);
    }
    for (int k = 0; k < RD_NEOO; k++) {
        const float arg = (float)((double)alpha * (double)(k + 1));
        T->bpf_E[k][0] = (float)cos((double)arg); T->bpf_E[k][1] = (float)-sin((double)arg);
    }
    /* coarse acquisition grid and frequency-shifted pilot replicas */
    for (int f = 0; f < RD_NFC; f++) {
        T->fcoarse[f] = -50.0 + 2.5 * f;
        const double wf = 2.0 * PI_D * T->fcoarse[f] / 8000.0;
        for (int n = 0; n < RD_M; n++) {
            const double cr = cos(wf * n), ci = sin(wf * n), pr = T->p[n][0], pi = T->p[n][1];
            T->p_w[n][f][0] = (float)(cr * pr - ci * pi); T->p_w[n][f][1] = (float)(cr * pi + ci * pr);
        }
    }
    T->snr_c1 = (float)(10.0 * log10(50.0 * 30 / 3000.0));
    T->snr_c2 = (float)(10.0 * log10(192.0 / 160.0));
}

/* ---------------------------------------------------------------------------------------------
 * 2. DNNw blob
 * -------------------------------------------------------------------------------------------*/
typedef struct { const char *name; int type, size; const unsigned char *data; } dnnw_rec;

static const dnnw_rec *rec_find(const dnnw_rec *r, int n, const char *base, const char *suffix)
{
    char nm[96];
    snprintf(nm, sizeof nm, "%s%s", base, suffix);
    for (int i = 0; i < n; i++) if (!strcmp(r[i].name, nm)) return &r[i];
    return NULL;
}

/* Every record is validated before anything is written: sizes against the shapes they imply, index walks against their
 * array, allocations against NULL.  The blob path comes from rade_open()'s argument or $RADE_MODEL_FILE, i.e. it is
 * untrusted input. */
static int lin_alloc(rd_linear *l)
{
    if (l->n_in <= 0 || l->n_out <= 0 || l->n_in > 65536 || l->n_out > 65536) return -1;
    l->b = malloc(sizeof(float) * (size_t)l->n_out); l->w = calloc((size_t)l->n_in * l->n_out, sizeof(float)); l->row_scale = NULL;
    if (!l->b || !l->w) { free(l->b); free(l->w); l->b = l->w = NULL; return -1; }
    return 0;
}

static int dequant_dense_float(const dnnw_rec *R, int n, const char *name, rd_linear *l)
{
    const dnnw_rec *b = rec_find(R, n, name, "_bias"), *w = rec_find(R, n, name, "_weights_float");
    if (!b || !w || b->size < 4 || b->size % 4 || w->size < 4 || w->size % 4) return -1;
    l->n_out = b->size / 4;
    if ((w->size / 4) % l->n_out) return -1;
    l->n_in = w->size / 4 / l->n_out;
    if (lin_alloc(l)) return -1;
    memcpy(l->b, b->data, sizeof(float) * l->n_out);
    const float *src = (const float *)w->data;                     /* stored as W^T: (n_in, n_out) */
    for (int i = 0; i < l->n_in; i++) for (int o = 0; o < l->n_out; o++) l->w[(size_t)o * l->n_in + i] = src[(size_t)i * l->n_out + o];
    return 0;
}

static int dequant_dense_int8(const dnnw_rec *R, int n, const char *name, rd_linear *l)
{
    const dnnw_rec *b = rec_find(R, n, name, "_bias"), *s = rec_find(R, n, name, "_scale"), *q = rec_find(R, n, name, "_weights_int8");
    if (!b || !s || !q || b->size < 32 || b->size % 32 || s->size != b->size || q->size <= 0) return -1;   /* n_out a multiple of 8 */
    l->n_out = b->size / 4;
    if (q->size % l->n_out) return -1;
    l->n_in = q->size / l->n_out;
    if (l->n_in % 4) return -1;
    if (lin_alloc(l)) return -1;
    memcpy(l->b, b->data, sizeof(float) * l->n_out);
    const float *sc = (const float *)s->data; const signed char *qq = (const signed char *)q->data;
    if ((l->row_scale = malloc(sizeof(float) * (size_t)l->n_out))) for (int o = 0; o < l->n_out; o++) l->row_scale[o] = sc[o] * 127.0f;
    const int blocks_in = l->n_in / 4;
    size_t pos = 0;                                                  /* walk the [n_out/8][n_in/4][8][4] tiles in storage order */
    for (int og = 0; og < l->n_out / 8; og++)
        for (int ib = 0; ib < blocks_in; ib++)
            for (int o8 = 0; o8 < 8; o8++)
                for (int i4 = 0; i4 < 4; i4++, pos++) {
                    const int o = og * 8 + o8;
                    l->w[(size_t)o * l->n_in + ib * 4 + i4] = (float)qq[pos] * (sc[o] * 127.0f);
                }
    return 0;
}

/* n_in comes from the architecture: the blob does not hold it (the reference compiles nb_inputs into linear_init(), wexchange/c_export/common.py:274), and
 * a trailing 4-input block that no output group keeps leaves no trace in the index list (tests/golden/dnnw_export_A.bin has such layers) */
static int dequant_blocksparse_int8(const dnnw_rec *R, int n, const char *name, rd_linear *l, int n_in)
{
    const dnnw_rec *b = rec_find(R, n, name, "_bias"), *s = rec_find(R, n, name, "_scale"), *q = rec_find(R, n, name, "_weights_int8"),
                   *ix = rec_find(R, n, name, "_weights_idx");
    if (!b || !s || !q || !ix || b->size < 32 || b->size % 32 || s->size != b->size || ix->size < 4 || ix->size % 4 || q->size < 0) return -1;
    l->n_out = b->size / 4;
    const int *idx = (const int *)ix->data; const int nidx = ix->size / 4;
    const float *sc = (const float *)s->data; const signed char *qq = (const signed char *)q->data;
    /* first walk: validate every count and column index against n_in, count the 8x4 blocks */
    int p = 0; long nblk = 0;
    if (n_in <= 0 || n_in % 4) return -1;
    for (int g = 0; g < l->n_out / 8; g++) {
        if (p >= nidx) return -1;
        const int cnt = idx[p++];
        if (cnt < 0 || cnt > nidx - p) return -1;
        for (int k = 0; k < cnt; k++, p++) {
            const int j = idx[p];
            if (j < 0 || j % 4 || j + 4 > n_in) return -1;
        }
        nblk += cnt;
    }
    if (nblk * 32 != (long)q->size || p != nidx) return -1;
    l->n_in = n_in;
    if (lin_alloc(l)) return -1;
    memcpy(l->b, b->data, sizeof(float) * l->n_out);
    if ((l->row_scale = malloc(sizeof(float) * (size_t)l->n_out))) for (int o = 0; o < l->n_out; o++) l->row_scale[o] = sc[o] * 127.0f;
    size_t pos = 0;
    p = 0;
    for (int g = 0; g < l->n_out / 8; g++) {
        const int cnt = idx[p++];
        for (int k = 0; k < cnt; k++) {
            const int j = idx[p++];
            for (int o8 = 0; o8 < 8; o8++) for (int i4 = 0; i4 < 4; i4++, pos++) {
                const int o = g * 8 + o8;
                l->w[(size_t)o * l->n_in + j + i4] = (float)qq[pos] * (sc[o] * 127.0f);
            }
        }
    }
    return 0;
}

static void swap_first_two_thirds(float *a, int third)
{   /* exporter wrote gates as z,r,n; torch (and our kernels) use r,z,n */
    for (int i = 0; i < third; i++) { const float t = a[i]; a[i] = a[third + i]; a[third + i] = t; }
}

static int load_gru(const dnnw_rec *R, int n, const char *name, rd_gru *g, int n_in)
{
    char nm[64]; rd_linear in, rec;
    snprintf(nm, sizeof nm, "%s_input", name); if (dequant_blocksparse_int8(R, n, nm, &in, n_in)) return -1;
    snprintf(nm, sizeof nm, "%s_recurrent", name); if (dequant_dense_int8(R, n, nm, &rec)) { free(in.w); free(in.b); free(in.row_scale); return -1; }
    if (rec.n_out != 3 * rec.n_in || in.n_out != rec.n_out) { free(in.w); free(in.b); free(in.row_scale); free(rec.w); free(rec.b); free(rec.row_scale); return -1; }
    g->hid = rec.n_in; g->n_in = in.n_in; g->w_ih = in.w; g->b_ih = in.b; g->w_hh = rec.w; g->b_hh = rec.b; g->s_ih = in.row_scale; g->s_hh = rec.row_scale;
    swap_first_two_thirds(g->w_ih, g->hid * g->n_in); swap_first_two_thirds(g->w_hh, g->hid * g->hid);
    swap_first_two_thirds(g->b_ih, g->hid); swap_first_two_thirds(g->b_hh, g->hid);
    if (g->s_ih) swap_first_two_thirds(g->s_ih, g->hid);
    if (g->s_hh) swap_first_two_thirds(g->s_hh, g->hid);
    return 0;
}

int rd_model_parse(const void *blob, size_t len, rd_model *m)
{
    const unsigned char *p = blob;
    dnnw_rec recs[256]; char names[256][48]; int n = 0;
    size_t off = 0;
    memset(m, 0, sizeof *m);
    while (off + 64 <= len && n < 256) {
        int ver, type, size, block;
        if (memcmp(p + off, "DNNw", 4)) { fprintf(stderr, "rade: bad weight blob (offset %zu)\n", off); return -1; }
        memcpy(&ver, p + off + 4, 4); memcpy(&type, p + off + 8, 4); memcpy(&size, p + off + 12, 4); memcpy(&block, p + off + 16, 4);
        if (ver != 0 || size < 0 || block < size || (size_t)block > len - off - 64) { fprintf(stderr, "rade: corrupt or truncated weight blob (record %d)\n", n); return -1; }
        memset(names[n], 0, 48); memcpy(names[n], p + off + 20, 44);
        recs[n].name = names[n]; recs[n].type = type; recs[n].size = size; recs[n].data = p + off + 64;
        n++; off += 64 + block;
    }
    /* the architecture this engine is built for (radae_base.py:239-251, :377-393; rade_model_geom.h): GRU input widths = the running concat */
    int err = 0;
    err |= dequant_dense_float(recs, n, "enc_dense1", &m->enc_dense1);
    err |= dequant_dense_float(recs, n, "enc_zdense", &m->enc_zdense);
    err |= dequant_dense_float(recs, n, "dec_dense1", &m->dec_dense1);
    err |= dequant_dense_float(recs, n, "dec_output", &m->dec_output);
    for (int i = 0; i < RM_NL && !err; i++) {
        char nm[32];
        snprintf(nm, sizeof nm, "enc_gru%d", i + 1); err |= load_gru(recs, n, nm, &m->enc_gru[i], RM_ENC_GRU_IN(i));
        snprintf(nm, sizeof nm, "dec_gru%d", i + 1); err |= load_gru(recs, n, nm, &m->dec_gru[i], RM_DEC_GRU_IN(i));
        snprintf(nm, sizeof nm, "enc_conv%d", i + 1); err |= dequant_dense_int8(recs, n, nm, &m->enc_conv[i]);
        snprintf(nm, sizeof nm, "dec_conv%d", i + 1); err |= dequant_dense_int8(recs, n, nm, &m->dec_conv[i]);
        snprintf(nm, sizeof nm, "dec_glu%d", i + 1); err |= dequant_dense_int8(recs, n, nm, &m->dec_glu[i]);
    }
    if (err) { fprintf(stderr, "rade: weight blob is missing layers\n"); rd_model_free(m); return -1; }
    /* sanity: every other layer shape of that architecture */
    for (int i = 0; i < RM_NL; i++)
        if (m->enc_gru[i].n_in != RM_ENC_GRU_IN(i) || m->enc_gru[i].hid != RM_ENC_H || m->dec_gru[i].n_in != RM_DEC_GRU_IN(i) || m->dec_gru[i].hid != RM_DEC_H ||
            m->enc_conv[i].n_in != 2 * RM_ENC_CONV_IN(i) || m->enc_conv[i].n_out != RM_ENC_CONV || m->dec_conv[i].n_in != 2 * RM_DEC_CONV_IN(i) || m->dec_conv[i].n_out != RM_DEC_CONV) {
            fprintf(stderr, "rade: unexpected layer shape in weight blob (layer %d)\n", i + 1); rd_model_free(m); return -1;
        }
    for (int i = 0; i < RM_NL; i++)
        if (m->dec_glu[i].n_in != RM_DEC_H || m->dec_glu[i].n_out != RM_DEC_GLU) { fprintf(stderr, "rade: unexpected GLU shape in weight blob (layer %d)\n", i + 1); rd_model_free(m); return -1; }
    /* every dimension the engine's upload (rade_engine.c:upload_lin) hard-codes is checked here: a foreign or crafted blob with smaller
     * layers must not get as far as the packers, which read N x K floats */
    if ((m->enc_dense1.n_in != RM_FEAT_AUX && m->enc_dense1.n_in != RM_FEAT) || m->enc_dense1.n_out != RM_ENC_D1 || m->enc_zdense.n_in != RM_ENC_W || m->enc_zdense.n_out != RM_LATENT ||
        m->dec_dense1.n_in != RM_LATENT || m->dec_dense1.n_out != RM_DEC_D1 || m->dec_output.n_in != RM_DEC_W || m->dec_output.n_out != m->enc_dense1.n_in) {   /* 4 x 21 features (model19, aux symbol) or 4 x 20 (model05, bbfm) */
        fprintf(stderr, "rade: unexpected dense layer shape in weight blob\n"); rd_model_free(m); return -1;
    }
    return 0;
}

static void lin_free(rd_linear *l) { free(l->w); free(l->b); free(l->row_scale); l->w = l->b = l->row_scale = NULL; }
void rd_model_free(rd_model *m)
{
    lin_free(&m->enc_dense1); lin_free(&m->enc_zdense); lin_free(&m->dec_dense1); lin_free(&m->dec_output);
    for (int i = 0; i < RM_NL; i++) {
        free(m->enc_gru[i].w_ih); free(m->enc_gru[i].w_hh); free(m->enc_gru[i].b_ih); free(m->enc_gru[i].b_hh); free(m->enc_gru[i].s_ih); free(m->enc_gru[i].s_hh);
        free(m->dec_gru[i].w_ih); free(m->dec_gru[i].w_hh); free(m->dec_gru[i].b_ih); free(m->dec_gru[i].b_hh); free(m->dec_gru[i].s_ih); free(m->dec_gru[i].s_hh);
        lin_free(&m->enc_conv[i]); lin_free(&m->dec_conv[i]); lin_free(&m->dec_glu[i]);
    }
    memset(m, 0, sizeof *m);
}

/* ---------------------------------------------------------------------------------------------
 * 4. the fractional resampler's time base and taps (include/rade_batch.h: rade_batch_resample; rade_clk.hip)
 * -------------------------------------------------------------------------------------------*/
/* I0 by its power series sum_k ((x / 2)^k / k!)^2: 40 terms are past double precision for x <= 10 */
static double bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 40; k++) { t *= (x * 0.5) / k; s += t * t; }
    return s;
}

/* T[p][j] = g(j - 15 - p / 256) / sum_j g, g(t) = sinc(t) I0(10 sqrt(1 - (t / 16)^2)) / I0(10).  With t = k - f (k = j - 15, f = p / 256, both exact)
 * sin(pi t) = -(-1)^k sin(pi f), and sin(pi f) = sin(pi (1 - f)) keeps it an exact 0 at f = 1 as at f = 0: rows 0 and 256 are exact impulses. */
void rade_resample_taps(float *out /* [257][32] */)
{
    const double i0b = bessel_i0(10.0);
    for (int p = 0; p <= 256; p++) {
        const double f = p / 256.0, sf = sin(PI_D * (p <= 128 ? f : 1.0 - f));
        double g[32], sum = 0.0;
        for (int j = 0; j < 32; j++) {
            const int k = j - 15;
            const double t = (double)k - f, u = t / 16.0;
            const double sinc = t == 0.0 ? 1.0 : ((k & 1) ? sf : -sf) / (PI_D * t);
            g[j] = fabs(t) <= 16.0 ? sinc * bessel_i0(10.0 * sqrt(1.0 - u * u)) / i0b : 0.0;
            sum += g[j];
        }
        for (int j = 0; j < 32; j++) out[p * 32 + j] = (float)(g[j] / sum);
    }
}

/* Q32.32 step and start of a stream; -1 where the header refuses (|ppm| > 50 000, a start that does not fit) */
int rd_resample_q(double t0, double ppm, long long *step_q, long long *t0_q)
{
    if (!(fabs(ppm) <= 50000.0) || !(fabs(t0) <= 536870912.0)) return -1;        /* NaN fails both; |t0| <= 2^29 keeps t0_q + n step_q inside 64 bits */
    *step_q = llrint((1.0 + ppm * 1e-6) * 4294967296.0);
    *t0_q = llrint(t0 * 4294967296.0);
    return 0;
}

long long rade_resample_count(long long in_end, double t0, double ppm)
{
    long long step_q, t0_q;
    if (rd_resample_q(t0, ppm, &step_q, &t0_q)) return -1;
    const __int128 need = ((__int128)in_end << 32) - t0_q;                        /* pos_q(n) < in_end 2^32  <=>  n step_q < need */
    if (need <= 0) return 0;
    const __int128 n = (need + step_q - 1) / step_q;
    return n * step_q > ((__int128)1 << 62) ? -1 : (long long)n;
}

/* ---------------------------------------------------------------------------------------------
 * 5. the rational rate converter's ratio, taps and count (include/rade_batch.h: rade_batch_rate_convert; rade_rate.hip)
 * -------------------------------------------------------------------------------------------*/
/* L / M reduced by their gcd, K = ceil(M / L), T = 32 K; -1 where the header refuses (L or M < 1, K > 8, L T > 16384 floats) */
int rd_rate_reduce(int L, int M, int *Lr, int *Mr, int *T)
{
    if (L < 1 || M < 1) return -1;
    int a = L, b = M;
    while (b) { const int r = a % b; a = b; b = r; }
    L /= a; M /= a;
    const int K = (M + L - 1) / L;
    if (K > RD_RATE_KMAX || (long long)L * 32 * K > RD_RATE_TABLE_MAX) return -1;
    *Lr = L; *Mr = M; *T = 32 * K;
    return 0;
}

/* C[ph][j] = g(t_j) / sum_j g(t_j), t_j = j - (T / 2 - 1) - ph / L, g(t) = sinc(t / W) I0(10 sqrt(1 - (t / H)^2)) / I0(10) for |t| <= H = T / 2, W = max(1, M / L).
 * M <= L (W = 1): sin(pi t) from the fraction f = ph / L alone, as rade_resample_taps forms it: row 0 is the exact unit impulse at j = 15. */
int rade_rate_taps(int L, int M, float *out /* [L][T] of the reduced pair, or NULL */)
{
    int T;
    if (rd_rate_reduce(L, M, &L, &M, &T)) return -1;
    if (!out) return T;
    const double i0b = bessel_i0(10.0), H = T / 2, W = M > L ? (double)M / (double)L : 1.0;
    double g[32 * RD_RATE_KMAX];
    for (int ph = 0; ph < L; ph++) {
        const double f = (double)ph / (double)L, sf = sin(PI_D * (2 * ph <= L ? f : 1.0 - f));
        double sum = 0.0;
        for (int j = 0; j < T; j++) {
            const int k = j - (T / 2 - 1);
            const double t = (double)k - f, u = t / H;
            double sinc;
            if (t == 0.0) sinc = 1.0;
            else if (M <= L) sinc = ((k & 1) ? sf : -sf) / (PI_D * t);
            else sinc = sin(PI_D * t / W) / (PI_D * t / W);
            g[j] = fabs(t) <= H ? sinc * bessel_i0(10.0 * sqrt(1.0 - u * u)) / i0b : 0.0;
            sum += g[j];
        }
        for (int j = 0; j < T; j++) out[(size_t)ph * T + j] = (float)(g[j] / sum);
    }
    return T;
}

/* the number of n >= 0 with n M < in_end L (any common factor of L and M cancels); -1: L or M < 1, or that many outputs pass the 2^62 limit of the call */
long long rade_rate_count(long long in_end, int L, int M)
{
    if (L < 1 || M < 1) return -1;
    if (in_end <= 0) return 0;
    const __int128 n = ((__int128)in_end * L + M - 1) / M;
    return n * M > ((__int128)1 << 62) ? -1 : (long long)n;
}

/* ---------------------------------------------------------------------------------------------
 * 6. the analog FM stage's host side (include/rade_batch.h: rade_batch_fm_mod / rade_batch_fm_demod; rade_fm.hip): the noise level of a C/N, the two
 *    least-squares filters of fm.m:41-47 in closed form, the de-emphasis pole folded into the output filter
 * -------------------------------------------------------------------------------------------*/
/* fm.m:16,162: the sigma of unit-power-carrier noise over the whole band Fs that gives CNdB inside Carson's bandwidth Bfm = 2 (fd + fm_max) */
double rade_fm_sigma(double CNdB, double Fs, double fm_max, double fd)
{
    if (!isfinite(CNdB) || !(Fs > 0.0) || !(fm_max > 0.0) || !(fd > 0.0) || !isfinite(Fs) || !isfinite(fm_max) || !isfinite(fd)) return -1.0;
    return sqrt(Fs / (pow(10.0, CNdB / 10.0) * 2.0 * (fd + fm_max)));
}

/* K of the folded de-emphasis: the first power of a = 1 - 1 / (tc Fs) below 2^-30; 0: no de-emphasis (tc <= 0); -1: a outside (0, 1) or K > RD_FM_NMAX */
int rade_fm_deemph_len(double Fs, double tc)
{
    if (!(tc > 0.0)) return tc == 0.0 ? 0 : -1;
    if (!(Fs > 0.0) || !isfinite(Fs) || !isfinite(tc)) return -1;
    const double a = 1.0 - 1.0 / (tc * Fs);
    if (!(a > 0.0) || !(a < 1.0)) return -1;
    double p = 1.0;
    for (int K = 1; K <= RD_FM_NMAX; K++) { p *= a; if (p < 0x1p-30) return K; }
    return -1;
}

static double fm_sincpi(double x) { return x == 0.0 ? 1.0 : sin(PI_D * x) / (PI_D * x); }

/* firls of a type I filter (n odd) in closed form.  bands [2 nb] are edges in units of the Nyquist rate, amp [2 nb] the desired amplitude at each edge (linear in
 * between), unit weights.  A(f) = sum_{i = 0..M} c_i cos(pi i f), M = (n - 1) / 2; minimising sum_bands int (A - D)^2 df gives Q c = r with
 *     Q[i][j] = 1/2 sum_bands [q(i - j) + q(i + j)],   q(k) = int cos(pi k f) df = f1 sinc(k f1) - f0 sinc(k f0)                (Toeplitz plus Hankel)
 *     r[i]    = sum_bands int (s f + d0) cos(pi i f) df = [(s f + d0) sin(pi i f) / (pi i) + s cos(pi i f) / (pi i)^2]  (i > 0),  [s f^2 / 2 + d0 f]  (i = 0)
 * solved by Gaussian elimination with partial pivoting in double; h[M] = c_0, h[M +- i] = c_i / 2. */
static int fm_firls(int n, int nb, const double *bands, const double *amp, double *h)
{
    const int M = (n - 1) / 2, D = M + 1;
    double *Q = (double *)malloc(sizeof(double) * ((size_t)D * D + D + 2 * (size_t)n));
    if (!Q) return -1;
    double *r = Q + (size_t)D * D, *q = r + D;                      /* q[k], k = 0..2 M */
    for (int k = 0; k <= 2 * M; k++) {
        q[k] = 0.0;
        for (int s = 0; s < nb; s++) q[k] += bands[2 * s + 1] * fm_sincpi(k * bands[2 * s + 1]) - bands[2 * s] * fm_sincpi(k * bands[2 * s]);
    }
    for (int i = 0; i < D; i++) {
        for (int j = 0; j < D; j++) Q[(size_t)i * D + j] = 0.5 * (q[i > j ? i - j : j - i] + q[i + j]);
        r[i] = 0.0;
        for (int s = 0; s < nb; s++) {
            const double f0 = bands[2 * s], f1 = bands[2 * s + 1], sl = (amp[2 * s + 1] - amp[2 * s]) / (f1 - f0), d0 = amp[2 * s] - sl * f0;
            if (i == 0) r[i] += (0.5 * sl * f1 * f1 + d0 * f1) - (0.5 * sl * f0 * f0 + d0 * f0);
            else {
                const double w = PI_D * i;
                r[i] += ((sl * f1 + d0) * sin(w * f1) / w + sl * cos(w * f1) / (w * w)) - ((sl * f0 + d0) * sin(w * f0) / w + sl * cos(w * f0) / (w * w));
            }
        }
    }
    for (int c = 0; c < D; c++) {
        int piv = c;
        for (int i = c + 1; i < D; i++) if (fabs(Q[(size_t)i * D + c]) > fabs(Q[(size_t)piv * D + c])) piv = i;
        if (Q[(size_t)piv * D + c] == 0.0) { free(Q); return -1; }
        if (piv != c) {
            for (int j = 0; j < D; j++) { const double t = Q[(size_t)c * D + j]; Q[(size_t)c * D + j] = Q[(size_t)piv * D + j]; Q[(size_t)piv * D + j] = t; }
            const double t = r[c]; r[c] = r[piv]; r[piv] = t;
        }
        for (int i = c + 1; i < D; i++) {
            const double f = Q[(size_t)i * D + c] / Q[(size_t)c * D + c];
            if (f == 0.0) continue;
            for (int j = c; j < D; j++) Q[(size_t)i * D + j] -= f * Q[(size_t)c * D + j];
            r[i] -= f * r[c];
        }
    }
    for (int i = D - 1; i >= 0; i--) {
        double s = r[i];
        for (int j = i + 1; j < D; j++) s -= Q[(size_t)i * D + j] * r[j];
        r[i] = s / Q[(size_t)i * D + i];
    }
    h[M] = r[0];
    for (int i = 1; i <= M; i++) h[M - i] = h[M + i] = 0.5 * r[i];
    free(Q);
    return 0;
}

/* the two filters of analog_fm_init (fm.m:41-47): bands [0, 0.95 fc, 1.05 fc, 1], amplitudes [1, 1, 0.01, 0.01]; bin: fc = (Bfm / 2) / (Fs / 2), ntaps values;
 * bout: fc = fm_max / (Fs / 2), convolved with a^k, k < K when de_emp_tc > 0: ntaps + K - 1 values (else ntaps).  Returns the length of bout; bin == bout == NULL only
 * queries.  -1: ntaps even or outside 3..RD_FM_NMAX, the folded length above RD_FM_NMAX, a band edge 1.05 fc >= 1, values that are not finite or not positive */
int rade_fm_taps(double Fs, double fm_max, double fd, int ntaps, double de_emp_tc, double *bin, double *bout)
{
    if (!(Fs > 0.0) || !(fm_max > 0.0) || !(fd > 0.0) || !isfinite(Fs) || !isfinite(fm_max) || !isfinite(fd) || !isfinite(de_emp_tc) || de_emp_tc < 0.0) return -1;
    if (ntaps < 3 || ntaps > RD_FM_NMAX || !(ntaps & 1)) return -1;
    const int K = rade_fm_deemph_len(Fs, de_emp_tc);
    if (K < 0) return -1;
    const int N2 = K ? ntaps + K - 1 : ntaps;
    if (N2 > RD_FM_NMAX) return -1;
    const double fc1 = (fd + fm_max) / (Fs / 2.0), fc2 = fm_max / (Fs / 2.0);
    if (!(1.05 * fc1 < 1.0) || !(1.05 * fc2 < 1.0)) return -1;
    if (!bin && !bout) return N2;
    const double amp[4] = { 1.0, 1.0, 0.01, 0.01 };
    if (bin) {
        const double bands[4] = { 0.0, fc1 * (1.0 - 0.05), fc1 * (1.0 + 0.05), 1.0 };
        if (fm_firls(ntaps, 2, bands, amp, bin)) return -1;
    }
    if (bout) {
        const double bands[4] = { 0.0, 0.95 * fc2, 1.05 * fc2, 1.0 };
        double h[RD_FM_NMAX];
        if (fm_firls(ntaps, 2, bands, amp, h)) return -1;
        if (!K) memcpy(bout, h, sizeof(double) * ntaps);
        else {
            const double a = 1.0 - 1.0 / (de_emp_tc * Fs);
            double pw[RD_FM_NMAX];
            pw[0] = 1.0;
            for (int k = 1; k < K; k++) pw[k] = pw[k - 1] * a;
            for (int i = 0; i < N2; i++) {
                double s = 0.0;
                for (int k = 0; k < K; k++) if (i - k >= 0 && i - k < ntaps) s += pw[k] * h[i - k];
                bout[i] = s;
            }
        }
    }
    return N2;
}

/* ---------------------------------------------------------------------------------------------
 * 7. the C/No estimator of est_CNo.py and the chirp of chirp.py (include/rade_batch.h: rade_batch_cno_est, rade_chirp; rade_cno.hip)
 * -------------------------------------------------------------------------------------------*/
/* N, J and the four bin limits with C's truncation toward zero, which is Python's int(); -1 where rade_batch_cno_est refuses */
int rade_cno_plan(const rade_cno_params *p, rade_cno_plan_t *out)
{
    if (!p || !out) return -1;
    if (!isfinite(p->window_time) || !isfinite(p->flow) || !isfinite(p->fhigh)) return -1;
    const double nd = 8000.0 * p->window_time;
    if (!(nd >= 1.0) || nd >= (double)RD_CNO_H * (RD_CNO_JMAX + 1)) return -1;
    const int N = (int)nd;
    if (N % RD_CNO_H || N / RD_CNO_H > RD_CNO_JMAX) return -1;
    const double bph = N / 8000.0, fl = bph * p->flow, fh = bph * p->fhigh;
    if (!(fl > -1.0) || !(fh > -1.0) || fl > (double)N || fh > (double)N) return -1;        /* (int)fl == 0 for -1 < fl < 0, as int() has it */
    rade_cno_plan_t q;
    q.N = N; q.J = N / RD_CNO_H;
    q.flow_bin = (int)fl; q.fhigh_bin = (int)fh;
    const int w = (int)(0.1 * q.fhigh_bin);
    q.noise_st = q.fhigh_bin + w; q.noise_en = q.noise_st + w;
    q.n_bins = q.fhigh_bin - q.flow_bin + w;
    if (q.flow_bin >= q.fhigh_bin || w < 1 || q.noise_en > N) return -1;
    if ((long)q.J * rd_cno_pitch(q.J, q.flow_bin, q.fhigh_bin, q.noise_st, q.noise_en) > RD_CNO_RING_MAX) return -1;
    *out = q;
    return 0;
}

/* t[m] = e^{-2 pi i m / N}, m = 0..N-1: double, rounded once per component */
void rd_cno_table(int N, float *out /* [N][2] */)
{
    for (int m = 0; m < N; m++) {
        const double a = 2.0 * PI_D * (double)m / (double)N;
        out[2 * m] = (float)cos(a); out[2 * m + 1] = (float)(-sin(a));
    }
}

/* est_CNo.py:44-55 and :71 over the band sums of one stream's windows, in the script's operation order */
void rd_cno_finish(const rade_cno_plan_t *q, const rade_cno_params *p, const double *bands /* [n_windows][2] */, int n_windows, rade_cno_result *res)
{
    const double bins_per_Hz = q->N / 8000.0;
    const double Nbw = (q->noise_en - q->noise_st) / bins_per_Hz;
    rade_cno_result r = { n_windows, 0, 0, 0.0, 0.0 };
    for (int w = 0; w < n_windows; w++) {
        const double C_plus_N = bands[2 * w], No = bands[2 * w + 1] / Nbw;
        const double C = C_plus_N - No * (p->fhigh - p->flow);
        if (C > 0) {
            const double CdB = 10 * log10(C), NodB = 10 * log10(No);
            const double CNodB = CdB - NodB;
            if (CNodB > r.max_CNodB) { r.max_CNodB = CNodB; r.max_st = (long long)w * RD_CNO_H; }
            r.n_positive++;
        }
    }
    r.max_SNRdB = r.max_CNodB - 10 * log10(3000);
    *res = r;
}

/* chirp.py:50-65 */
int rade_chirp(float *iq_out, int nsam, double flow, double fhigh, double amp)
{
    if (!iq_out || nsam < 0 || !isfinite(flow) || !isfinite(fhigh) || !isfinite(amp)) return -1;
    const double Fs = 8000;
    double freq = flow, delta_freq = (fhigh - flow) / Fs, phase = 0;
    for (int n = 0; n < nsam; n++) {
        phase += 2 * PI_D * freq / Fs;
        phase -= 2 * PI_D * (int)(phase / (2 * PI_D));
        freq += delta_freq;
        if (freq > fhigh) delta_freq = -(fhigh - flow) / Fs;
        if (freq < flow) delta_freq = (fhigh - flow) / Fs;
        iq_out[2 * n] = (float)(amp * cos(phase)); iq_out[2 * n + 1] = (float)(amp * sin(phase));
    }
    return 0;
}

/* ---------------------------------------------------------------------------------------------
 * 8. the spectrogram of plot_specgram.m (include/rade_batch.h: rade_batch_specgram; rade_spec.hip): the display band, the slice count, the window, the thresholds
 * -------------------------------------------------------------------------------------------*/
/* k0 = max(1, ceil(fmin 2048 / 8000)), k1 = min(1023, floor(fmax 2048 / 8000)); -1 where rade_batch_specgram refuses the parameters */
int rade_specgram_plan(const rade_specgram_params *p, rade_specgram_plan_t *out)
{
    if (!p || !out) return -1;
    if (!isfinite(p->fmin) || !isfinite(p->fmax) || !isfinite(p->lo) || !isfinite(p->hi)) return -1;
    if (p->fmin > p->fmax || !(0.0 < p->lo && p->lo < p->hi && p->hi <= 1.0)) return -1;
    const double half = RD_SPEC_NFFT / 2;
    double c0 = ceil(p->fmin * RD_SPEC_NFFT / 8000.0), c1 = floor(p->fmax * RD_SPEC_NFFT / 8000.0);
    if (c0 < 1.0) c0 = 1.0;
    if (c1 > half - 1.0) c1 = half - 1.0;
    if (c0 > c1) return -1;
    rade_specgram_plan_t q = { (int)c1 - (int)c0 + 1, (int)c0, (int)c1, RD_SPEC_WIN, RD_SPEC_STEP, RD_SPEC_NFFT };
    *out = q;
    return 0;
}

/* len(1 : 160 : n - 1280): starts 0, 160, .. while start < n - 1280 */
long long rade_specgram_slices(long long n)
{
    return n > RD_SPEC_WIN ? (n - RD_SPEC_WIN + RD_SPEC_STEP - 1) / RD_SPEC_STEP : 0;
}

/* hanning(1280): 0.5 - 0.5 cos(2 pi (i + 1) / 1281) in double, rounded once */
void rade_specgram_window(float *out /* [1280] */)
{
    for (int i = 0; i < RD_SPEC_WIN; i++) out[i] = (float)(0.5 - 0.5 * cos(2.0 * PI_D * (double)(i + 1) / (double)(RD_SPEC_WIN + 1)));
}

/* T[j] = lo (hi / lo)^((j - 0.5) / 255), j = 1..255 -> out[j - 1]: double, rounded once */
int rade_specgram_levels(double lo, double hi, float *out /* [255] */)
{
    if (!out || !isfinite(lo) || !isfinite(hi) || !(0.0 < lo && lo < hi && hi <= 1.0)) return -1;
    for (int j = 1; j <= 255; j++) out[j - 1] = (float)(lo * pow(hi / lo, ((double)j - 0.5) / 255.0));
    return 0;
}

/* ---------------------------------------------------------------------------------------------
 * 8. whole-file pilot acquisition: the hop count, the state machine and the statistics of rx.py (include/rade_batch.h: rade_batch_acq_detect; rade_acq.hip)
 * -------------------------------------------------------------------------------------------*/
/* hops of `while len(rx) >= 2 Nmf + M + Ncp: ...; rx = rx[Nmf:-1]` */
int rade_acq_hops(long long n) { return rd_acq_hops(n); }

/* fcoarse_range[f_ind_max]; the script's fmax stays the integer 0 where no cell exceeded 0 */
double rade_acq_fmax(const rade_acq_hop *hop) { return hop && hop->Dtmax12 > 0.0f ? -50.0 + 2.5 * hop->f_ind : 0.0; }

/* rx.py:151-188 */
int rade_acq_track(const rade_acq_hop *hops, int n_hops, int acq_test, rade_acq_event *events, int max_events, rade_acq_log *log_out)
{
    if (n_hops < 0 || max_events < 0 || (n_hops && !hops) || (max_events && !events)) return -1;
    int state = 0, tmax_candidate = 0, valid_count = 0, n_ev = 0;
    for (int k = 0; k < n_hops; k++) {
        if (log_out) { log_out[k].state = state; log_out[k].tmax_candidate = tmax_candidate; log_out[k].valid_count = valid_count; }
        int next = state;
        if (state == 0) {
            if (hops[k].candidate) { next = 1; tmax_candidate = hops[k].tmax; valid_count = 1; }
        } else if (hops[k].candidate && fabs((double)(hops[k].tmax - tmax_candidate)) < 0.02 * RD_M) {
            if (++valid_count > 3) {
                if (n_ev < max_events) { events[n_ev].hop = k; events[n_ev].tmax = hops[k].tmax; events[n_ev].f_ind = hops[k].f_ind; }
                n_ev++;
                if (!acq_test) return n_ev;
                next = 0;
            }
        } else next = 0;
        state = next;
    }
    return n_ev;
}

/* rx.py:134, :170-171, :190-195 */
int rade_acq_stats(const rade_acq_event *events, const rade_acq_refined *refined, int n_events, int n_hops, int Ntap, double fmax_target, double acq_time_target,
                   rade_acq_result *out)
{
    if (!out || n_events < 0 || n_hops < 0 || (n_events && (!events || !refined)) || !isfinite(fmax_target)) return -1;
    const double target = RD_NCP + Ntap / 2.0;
    rade_acq_result r = { 0, 0, 0, 0.0, INFINITY };
    for (int e = 0; e < n_events; e++) {
        const double t = (double)(refined[e].t - (long long)RD_NMF * events[e].hop);
        if (fabs(t - target) < 0.0025 * 8000.0 && fabs(refined[e].f - fmax_target) <= 5.0) r.passes++; else r.fails++;
    }
    if (r.passes + r.fails) r.pfail = (double)r.fails / (double)(r.passes + r.fails);
    if (r.passes) r.mean_acq_time = ((double)RD_NMF * (double)(n_hops + 1) / 8000.0) / (double)r.passes;
    r.passed = r.pfail < 0.2 && r.mean_acq_time < acq_time_target;
    *out = r;
    return 0;
}

/* ---------------------------------------------------------------------------------------------
 * 9. the Welch periodogram and the 99 % bandwidth of radae_plots.m (include/rade_batch.h: rade_batch_psd, rade_batch_sigstat; rade_psd.hip): the geometry, the segment
 *    count, the window, pwelch's recalled defaults, bandwidth() / spec_power() as written
 * -------------------------------------------------------------------------------------------*/
/* -1 where rade_batch_psd refuses the geometry */
int rade_psd_plan(int win, int step, rade_psd_plan_t *out)
{
    if (!out || win < RD_PSD_WIN_MIN || win > RD_PSD_NFFT || step < 1 || step > win) return -1;
    rade_psd_plan_t q = { RD_PSD_NFFT, win, step, RD_PSD_RUN };
    *out = q;
    return 0;
}

/* len(0 : step : n - win): starts 0, step, .. while start + win <= n */
long long rade_psd_segments(long long n, int win, int step)
{
    return win >= 1 && step >= 1 && n >= win ? (n - win) / step + 1 : 0;
}

/* hamming(win): 0.54 - 0.46 cos(2 pi i / (win - 1)) in double, rounded once */
int rade_psd_window(int win, float *out /* [win] */)
{
    if (!out || win < RD_PSD_WIN_MIN || win > RD_PSD_NFFT) return -1;
    for (int i = 0; i < win; i++) out[i] = (float)(0.54 - 0.46 * cos(2.0 * PI_D * (double)i / (double)(win - 1)));
    return 0;
}

/* RECALLED, NOT VERIFIED: pwelch(x, [], []) takes a Hamming window of 2^ceil(log2(sqrt(n / 0.5))) samples at 50 % overlap */
int rade_psd_octave_default(long long n, int *win, int *step)
{
    if (!win || !step || n < 1 || n > (1LL << 40)) return -1;
    int w = 1;
    while ((double)w < sqrt((double)n / 0.5)) w *= 2;
    *win = w; *step = w - w / 2;
    return 0;
}

/* bandwidth() and spec_power() of radae_plots.m:92-116, one-based as written; round() is half away from zero in C as in Octave.  -1: `en` passes the last bin before
 * the fraction is reached (the script's index error), or the arguments are refused */
int rade_psd_bandwidth(const double *P, int nfft, double Fs, double centre_hz, double frac, double *bw_hz, double *ratio)
{
    if (!P || !bw_hz || !ratio || nfft < 2 || !(Fs > 0.0) || !isfinite(Fs) || !isfinite(centre_hz) || !isfinite(frac)) return -1;
    double total = 0.0;
    for (int k = 0; k < nfft; k++) total += P[k];
    const double centre = round((double)nfft * centre_hz / Fs);
    if (!(centre >= 1.0 && centre <= (double)nfft)) return -1;
    for (int bw = 2; ; bw++) {
        double st = round(centre - bw / 2.0);
        const double en = round(centre + bw / 2.0);
        if (st < 1.0) st = 1.0;
        if (en > (double)nfft) return -1;
        double p = 0.0;
        for (int k = (int)st; k <= (int)en; k++) p += P[k - 1];
        if (p > frac * total) { *bw_hz = bw * Fs / nfft; *ratio = p / total; return 0; }
    }
}
