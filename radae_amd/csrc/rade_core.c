/*
 * rade_core.c -- include/rade_core.h on the single-stream HIP kernels (rade_core_step.hip): one device-resident state per encoder /
 * decoder state, one 40 ms step per call (the call granularity of /root/reference/src/rade_enc.c:55-114 and
 * rade_dec.c:50-102), host buffers in and out.  The step itself is one launch of k_core_enc_step / k_core_dec_step.
 */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "rade_core.h"
#include "rade_host.h"
#include "rade_dev.h"
static_assert(RADE_LATENT_DIM == RM_LATENT, "the public header's latent width is the model's");

/* hidden record BEHIND the NULL terminator of every list rade_parse_weights() returns: where the blob lives.  *list is the
 * malloc'ed pointer itself, so the reference harnesses' free(list) (test_rade_enc.c:115, test_rade_dec.c:115) is valid. */
#define RD_LIST_MAGIC "__rade_blob__"
/* the reference links compiled-in weights under these names; here they stand for "the default blob" */
const WeightArray radeenc_arrays[1] = { { NULL, -1, 0, NULL } };
const WeightArray radedec_arrays[1] = { { NULL, -1, 0, NULL } };

int rade_parse_weights(WeightArray **list, const void *data, int len)
{
    if (!list || !data || len < 64) return -1;
    const unsigned char *p = data;
    int n = 0;
    for (size_t off = 0; off + 64 <= (size_t)len; n++) {       /* first pass: count and validate the record headers */
        int size, block;
        if (memcmp(p + off, "DNNw", 4)) return -1;
        memcpy(&size, p + off + 12, 4); memcpy(&block, p + off + 16, 4);
        if (size < 0 || block < size || (size_t)block > (size_t)len - off - 64 || p[off + 63] != 0) return -1;
        off += 64 + (size_t)block;
    }
    WeightArray *l = calloc((size_t)n + 2, sizeof *l);
    if (!l) return -1;
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        int type, size, block;
        memcpy(&type, p + off + 8, 4); memcpy(&size, p + off + 12, 4); memcpy(&block, p + off + 16, 4);
        l[i].name = (const char *)(p + off + 20); l[i].type = type; l[i].size = size; l[i].data = p + off + 64;
        off += 64 + (size_t)block;
    }
    /* l[n] is the NULL terminator (calloc); the blob record sits behind it, out of reach of a walk over the list */
    l[n + 1].name = RD_LIST_MAGIC; l[n + 1].size = len; l[n + 1].data = data;
    *list = l;
    return n;
}

static int find_array(const WeightArray *a, const char *name)
{
    for (int i = 0; a[i].name; i++) if (!strcmp(a[i].name, name)) return a[i].size;
    return -1;
}

/* resolves a list to (blob, len); the default lists map the default blob file into memory once */
static int list_blob(const WeightArray *arrays, const void **blob, int *len)
{
    static void *def_blob; static int def_len;
    if (arrays && arrays != radeenc_arrays && arrays != radedec_arrays) {
        const WeightArray *hdr = arrays;
        while (hdr->name) hdr++;                               /* the terminator; the blob record follows it */
        hdr++;
        if (!hdr->name || strcmp(hdr->name, RD_LIST_MAGIC)) { fprintf(stderr, "rade_core: weight list was not made by rade_parse_weights()\n"); return -1; }
        *blob = hdr->data; *len = hdr->size;
        return 0;
    }
    if (!def_blob) {
        char buf[4096];
        const char *path = rd_find_default_model(NULL, buf, sizeof buf);
        FILE *f = path ? fopen(path, "rb") : NULL;
        if (!f) { fprintf(stderr, "rade_core: no default weight blob ($RADE_MODEL_FILE, weights/model19_check3.bin)\n"); return -1; }
        fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
        void *b = n > 0 ? malloc((size_t)n) : NULL;
        if (!b || fread(b, 1, (size_t)n, f) != (size_t)n) { fclose(f); free(b); return -1; }
        fclose(f);
        def_blob = b; def_len = (int)n;
    }
    *blob = def_blob; *len = def_len;
    return 0;
}

static int init_model(const WeightArray *arrays, int dim, const void **blob, int *len)
{
    if (list_blob(arrays, blob, len)) return 1;
    WeightArray *l = NULL;
    if (rade_parse_weights(&l, *blob, *len) < 0) return 1;
    /* the dimension the blob was exported with: enc_dense1 is (input_dim x RM_ENC_D1) floats, dec_output has output_dim biases */
    const int w = find_array(l, "enc_dense1_weights_float"), b = find_array(l, "dec_output_bias");
    free(l);
    if (w != dim * RM_ENC_D1 * 4 || b != dim * 4) return 1;
    return 0;
}

int init_radeenc(RADEEnc *model, const WeightArray *arrays, int input_dim)
{
    if (!model || (input_dim != RM_FEAT && input_dim != RM_FEAT_AUX)) return 1;
    memset(model, 0, sizeof *model);
    if (init_model(arrays, input_dim, &model->blob, &model->blob_len)) return 1;
    model->input_dim = input_dim; model->nb_z = RADE_LATENT_DIM;
    return 0;
}

int init_radedec(RADEDec *model, const WeightArray *arrays, int output_dim)
{
    if (!model || (output_dim != RM_FEAT && output_dim != RM_FEAT_AUX)) return 1;
    memset(model, 0, sizeof *model);
    if (init_model(arrays, output_dim, &model->blob, &model->blob_len)) return 1;
    model->output_dim = output_dim; model->nb_z = RADE_LATENT_DIM;
    return 0;
}

/* ---- device side of one state ------------------------------------------------------------------------------------
 * One step = ONE launch of k_core_enc_step / k_core_dec_step (rade_core_step.hip): the whole layer stack for the stream's next 40 ms
 * in a single workgroup, weights chunk-major in HBM / L2 (int8 layers as one binary16 plane of integers + row scales), GRU and conv state in
 * HBM between calls, input and output in pinned host memory the kernel reads / writes directly (no copy nodes). */
#define CORE_MAXBUF 64
typedef struct {
    int dim;
    rd_core_args a; void *bufs[CORE_MAXBUF]; int n_bufs; hipStream_t gs; float *h_in, *h_out; int device;
} core_dev;

static void *core_upload(core_dev *d, const void *src, size_t bytes)
{
    void *p = NULL;
    if (d->n_bufs >= CORE_MAXBUF || hipMalloc(&p, bytes) != hipSuccess) return NULL;
    if (src ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess : hipMemset(p, 0, bytes) != hipSuccess) { hipFree(p); return NULL; }
    d->bufs[d->n_bufs++] = p;
    return p;
}
/* one layer, chunk-major [Kpad / 8][Npad][8] (rade_core_step.hip): the integers of an int8 layer as a binary16 plane + row scales
 * when `want_q` (the kernel's product for this layer is the binary16 one), float32 otherwise */
static int core_layer(core_dev *d, rd_mv *L, const float *w, const float *bias, const float *row_scale, int N, int K, int want_q)
{
    const int Kpad = (K + 7) & ~7, Npad = (N + 63) & ~63;
    memset(L, 0, sizeof *L);
    L->N = N; L->K = Kpad;
    if (want_q) {
        /* a float layer where the kernel expects integers cannot be represented: every GRU / conv / GLU layer of the blob format is int8 */
        unsigned short *q = malloc(sizeof(unsigned short) * (size_t)Npad * Kpad);
        float *sc = calloc(Npad, sizeof(float));
        if (!q || !sc || rd_chunkmajor_q16(w, row_scale, N, K, Kpad, Npad, q)) { fprintf(stderr, "rade_core: a GRU / conv / GLU layer of the blob is not int8 x row scale\n"); free(q); free(sc); return -1; }
        memcpy(sc, row_scale, sizeof(float) * N);
        L->wq = core_upload(d, q, sizeof(unsigned short) * (size_t)Npad * Kpad);
        L->scale = core_upload(d, sc, sizeof(float) * Npad);
        free(q); free(sc);
        if (!L->wq || !L->scale) return -1;
    } else {
        float *f = malloc(sizeof(float) * (size_t)Npad * Kpad);
        if (!f) return -1;
        rd_chunkmajor_f32(w, N, K, Kpad, Npad, f);
        L->wf = core_upload(d, f, sizeof(float) * (size_t)Npad * Kpad);
        free(f);
        if (!L->wf) return -1;
    }
    if (bias) {
        float *bp = calloc(Npad, sizeof(float));
        if (!bp) return -1;
        memcpy(bp, bias, sizeof(float) * N);
        L->bias = core_upload(d, bp, sizeof(float) * Npad);
        free(bp);
        if (!L->bias) return -1;
    }
    return 0;
}

static void dev_close(core_dev *d)
{
    if (!d) return;
    if (d->h_in) hipHostFree(d->h_in);
    if (d->h_out) hipHostFree(d->h_out);
    if (d->gs) hipStreamDestroy(d->gs);
    for (int i = 0; i < d->n_bufs; i++) hipFree(d->bufs[i]);
    free(d);
}

static core_dev *dev_open(const void *blob, int len, int dim, int enc)
{
    core_dev *d = calloc(1, sizeof *d);
    if (!d) return NULL;
    const char *dv = getenv("RADE_DEVICE");
    d->device = dv ? atoi(dv) : 0; d->dim = dim;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fprintf(stderr, "rade_core: no HIP device available -- this library has no CPU fallback\n"); free(d); return NULL; }
    rd_model m;
    if (hipSetDevice(d->device) != hipSuccess || rd_model_parse(blob, (size_t)len, &m)) { free(d); return NULL; }
    rd_core_args *a = &d->a;
    int e = 0;
    a->is_enc = enc;
    if (enc) {
        a->n_in = dim; a->n_out = RADE_LATENT_DIM; a->W = RM_ENC_W; a->H = RM_ENC_H; a->in0 = RM_ENC_D1; a->conv_out = RM_ENC_CONV;
        e |= core_layer(d, &a->dense1, m.enc_dense1.w, m.enc_dense1.b, NULL, RM_ENC_D1, m.enc_dense1.n_in, 0);
        e |= core_layer(d, &a->out, m.enc_zdense.w, m.enc_zdense.b, NULL, RM_LATENT, RM_ENC_W, 0);
        for (int l = 0; l < RM_NL && !e; l++) {
            a->dil[l] = RM_ENC_DIL(l);
            e |= core_layer(d, &a->gin[l], m.enc_gru[l].w_ih, m.enc_gru[l].b_ih, m.enc_gru[l].s_ih, RM_ENC_G, m.enc_gru[l].n_in, 1);
            e |= core_layer(d, &a->ghh[l], m.enc_gru[l].w_hh, m.enc_gru[l].b_hh, m.enc_gru[l].s_hh, RM_ENC_G, RM_ENC_H, 1);
            e |= core_layer(d, &a->conv[l], m.enc_conv[l].w, m.enc_conv[l].b, m.enc_conv[l].row_scale, RM_ENC_CONV, m.enc_conv[l].n_in, 1);
        }
    } else {
        a->n_in = RADE_LATENT_DIM; a->n_out = dim; a->W = RM_DEC_W; a->H = RM_DEC_H; a->in0 = RM_DEC_D1; a->conv_out = RM_DEC_CONV;
        e |= core_layer(d, &a->dense1, m.dec_dense1.w, m.dec_dense1.b, NULL, RM_DEC_D1, RM_LATENT, 0);
        e |= core_layer(d, &a->out, m.dec_output.w, m.dec_output.b, NULL, m.dec_output.n_out, RM_DEC_W, 0);
        for (int l = 0; l < RM_NL && !e; l++) {
            a->dil[l] = 1;
            e |= core_layer(d, &a->gin[l], m.dec_gru[l].w_ih, m.dec_gru[l].b_ih, m.dec_gru[l].s_ih, RM_DEC_G, m.dec_gru[l].n_in, 1);
            e |= core_layer(d, &a->ghh[l], m.dec_gru[l].w_hh, m.dec_gru[l].b_hh, m.dec_gru[l].s_hh, RM_DEC_G, RM_DEC_H, 1);
            e |= core_layer(d, &a->glu[l], m.dec_glu[l].w, NULL, m.dec_glu[l].row_scale, RM_DEC_GLU, RM_DEC_H, 1);
            e |= core_layer(d, &a->conv[l], m.dec_conv[l].w, m.dec_conv[l].b, m.dec_conv[l].row_scale, RM_DEC_CONV, m.dec_conv[l].n_in, 1);
        }
    }
    if (!e && (enc ? m.enc_dense1.n_in : m.dec_output.n_out) != dim) e = -1;
    rd_model_free(&m);
    a->hist = core_upload(d, NULL, sizeof(float) * 2 * a->W);          /* zero state = rade_init_encoder / rade_init_decoder */
    a->h = core_upload(d, NULL, sizeof(float) * RM_NL * a->H);
    if (e || !a->hist || !a->h || hipStreamCreate(&d->gs) != hipSuccess ||
        hipHostMalloc((void **)&d->h_in, sizeof(float) * 96, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostMalloc((void **)&d->h_out, sizeof(float) * 128, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&a->in, d->h_in, 0) != hipSuccess || hipHostGetDevicePointer((void **)&a->out_vec, d->h_out, 0) != hipSuccess) {
        fprintf(stderr, "rade_core: device set-up failed\n"); dev_close(d); return NULL;
    }
    memset(d->h_out, 0, sizeof(float) * 128);
    a->done = (unsigned *)(a->out_vec + 96);
    return d;
}

/* Completion of a single-stream launch: the kernel writes `seq` into a word of pinned, host-coherent memory after its outputs.  Polling that word returns
 * as soon as the result is there (a stream synchronisation goes through the runtime's interrupt path: ~100 us of wake-up for a 40 us kernel), but a polling
 * thread owns a core: so the spin is bounded by RD_POLL_US (a few kernel durations) and then the stream is waited for the ordinary way, which yields the
 * core and surfaces device errors.  $RADE_CORE_NO_POLL=1: never spin (hosts with fewer cores than single-stream states). */
#define RD_POLL_US 1000.0
static int wait_done(volatile unsigned *done, unsigned seq, hipStream_t st)
{
    static int no_poll = -1;
    if (no_poll < 0) no_poll = getenv("RADE_CORE_NO_POLL") ? 1 : 0;
    if (!no_poll) {
        struct timespec t0, t1; clock_gettime(CLOCK_MONOTONIC, &t0);
        for (unsigned spins = 0; *done != seq; spins++) {
            if ((spins & 255u) == 255u) {
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1e6 + (t1.tv_nsec - t0.tv_nsec) * 1e-3 > RD_POLL_US) break;
            }
        }
    }
    if (*done != seq && (hipStreamSynchronize(st) != hipSuccess || *done != seq)) return -1;
    __sync_synchronize();
    return 0;
}

/* ---- internal (rade_api.c): rade_tx() on the single-stream kernels -- one launch per modem frame (k_tx_frame3: three encoder steps + the OFDM
 * modulator), features and samples in pinned host memory the kernel reads / writes directly, completion by a polled word ------------------------- */
typedef struct { core_dev *d; float *h_in, *h_iq; unsigned *done; rd_core_args *a_dev; } tx_dev;
void rd_core_tx_close(void *p)
{
    tx_dev *t = p;
    if (!t) return;
    if (t->h_in) hipHostFree(t->h_in);
    if (t->h_iq) hipHostFree(t->h_iq);
    if (t->a_dev) hipFree(t->a_dev);
    if (t->d) dev_close(t->d);
    free(t);
}
void *rd_core_tx_open(const void *blob, int len, const rd_tables *d_tab)
{
    tx_dev *t = calloc(1, sizeof *t);
    if (!t) return NULL;
    t->d = dev_open(blob, len, RM_FEAT_AUX, 1);
    if (!t->d || hipHostMalloc((void **)&t->h_in, sizeof(float) * 3 * RM_FEAT_AUX, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostMalloc((void **)&t->h_iq, sizeof(float) * 2 * RD_NMF + 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { rd_core_tx_close(t); (void)hipGetLastError(); return NULL; }
    rd_core_args *a = &t->d->a;
    void *dp = NULL;
    if (hipHostGetDevicePointer(&dp, t->h_in, 0) != hipSuccess) { rd_core_tx_close(t); return NULL; }
    a->in = dp;
    if (hipHostGetDevicePointer(&dp, t->h_iq, 0) != hipSuccess) { rd_core_tx_close(t); return NULL; }
    a->iq_out = dp; a->tab = d_tab;
    t->done = (unsigned *)(t->h_iq + 2 * RD_NMF); *t->done = 0;
    a->done = (unsigned *)((float *)dp + 2 * RD_NMF);
    /* the kernel reads the layer table through a pointer: the record goes to device memory once (every pointer in it is fixed from here on) */
    if (hipMalloc((void **)&t->a_dev, sizeof *a) != hipSuccess || hipMemcpy(t->a_dev, a, sizeof *a, hipMemcpyHostToDevice) != hipSuccess) { rd_core_tx_close(t); return NULL; }
    return t;
}
/* features_in: 12 frames x RM_FILE_FRAME floats (rade_api.c:426-434 packs the first RM_NFEAT of each + the aux symbol -1 into three rows of 4 x 21); tx_out: 960 complex samples */
int rd_core_tx_frame(void *p, const float *features_in, float *tx_out)
{
    tx_dev *t = p; core_dev *d = t->d;
    if (hipSetDevice(d->device) != hipSuccess) return -1;
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < RM_STEP_FRAMES; i++) {
            float *row = t->h_in + c * RM_FEAT_AUX + i * (RM_NFEAT + 1);
            memcpy(row, features_in + (c * RM_STEP_FRAMES + i) * RM_FILE_FRAME, sizeof(float) * RM_NFEAT);
            row[RM_NFEAT] = -1.0f;
        }
    volatile unsigned *done = (volatile unsigned *)t->done;
    d->a.seq++;
    if (rd_launch_tx_frame(t->a_dev, d->a.seq, d->gs)) return -1;
    if (wait_done(done, d->a.seq, d->gs)) return -1;
    memcpy(tx_out, t->h_iq, sizeof(float) * 2 * RD_NMF);
    return 0;
}

void rade_init_encoder(RADEEncState *s) { memset(s, 0, sizeof *s); }     /* rade_enc.c:39-43: the caller's memory may be uninitialised */
void rade_init_decoder(RADEDecState *s) { memset(s, 0, sizeof *s); }
void rade_free_encoder(RADEEncState *s) { if (s && s->initialized) dev_close(s->dev); if (s) memset(s, 0, sizeof *s); }
void rade_free_decoder(RADEDecState *s) { if (s && s->initialized) dev_close(s->dev); if (s) memset(s, 0, sizeof *s); }

/* additive: back to the zero state without releasing the device side (weights stay uploaded) */
static void core_reset(int *initialized, void **dev)
{
    core_dev *d = *initialized ? *dev : NULL;
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipMemsetAsync(d->a.hist, 0, sizeof(float) * 2 * d->a.W, d->gs);
    (void)hipMemsetAsync(d->a.h, 0, sizeof(float) * RM_NL * d->a.H, d->gs);
    (void)hipStreamSynchronize(d->gs);
}
void rade_reset_encoder(RADEEncState *s) { if (s) core_reset(&s->initialized, &s->dev); }
void rade_reset_decoder(RADEDecState *s) { if (s) core_reset(&s->initialized, &s->dev); }

/* one step: in[n_in] (host) -> out[n_out] (host) */
static int core_step(core_dev *d, const float *in, int n_in, float *out, int n_out)
{
    if (hipSetDevice(d->device) != hipSuccess) return -1;
    memcpy(d->h_in, in, sizeof(float) * n_in);
    volatile unsigned *done = (volatile unsigned *)(d->h_out + 96);
    d->a.seq++;
    if (rd_launch_core_step(&d->a, d->gs)) return -1;
    if (wait_done(done, d->a.seq, d->gs)) return -1;        /* the completion word the kernel writes after the output */
    memcpy(out, d->h_out, sizeof(float) * n_out);
    return 0;
}

static void die(const char *what) { fprintf(stderr, "%s: device error (this library has no CPU fallback)\n", what); exit(1); }

void rade_core_encoder(RADEEncState *s, const RADEEnc *model, float *z, const float *features, int arch, int bottleneck)
{
    (void)arch;
    if (!s->initialized) {                        /* first step after rade_init_encoder(): zero state = a fresh device state */
        s->dev = dev_open(model->blob, model->blob_len, model->input_dim, 1);
        if (!s->dev) die("rade_core_encoder");
        s->initialized = 1;
    }
    core_dev *d = s->dev;
    if (core_step(d, features, d->dim, z, RADE_LATENT_DIM)) die("rade_core_encoder");
    if (bottleneck == 1) for (int i = 0; i < RADE_LATENT_DIM; i++) z[i] = tanhf(z[i]);      /* rade_enc.c:113 / radae_base.py:281-284 */
}

void rade_core_decoder(RADEDecState *s, const RADEDec *model, float *features, const float *z_hat, int arch)
{
    (void)arch;
    if (!s->initialized) {
        s->dev = dev_open(model->blob, model->blob_len, model->output_dim, 0);
        if (!s->dev) die("rade_core_decoder");
        s->initialized = 1;
    }
    core_dev *d = s->dev;
    if (core_step(d, z_hat, RADE_LATENT_DIM, features, d->dim)) die("rade_core_decoder");
}
