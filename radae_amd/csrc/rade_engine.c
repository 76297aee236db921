/*
 * rade_engine.c -- batched RADE engine (plain C host code driving the HIP kernels through the
 * launch shims in rade_dev.h).  Implements include/rade_batch.h.
 *
 * Execution model: the encoder / decoder are evaluated layer by layer over
 * ALL streams and ALL time steps of a chunk: the feed-forward part of every layer is one skinny-N
 * f32-MFMA GEMM with M = B*T rows, and only the 64/96-wide GRU recurrences run as serial scans.
 * The receiver runs one workgroup per stream for a whole rade_batch_rx call; the sync state machine consumes the
 * decoder's aux bits (UW errors, radae_rxe.py:220-224, :306-312), so the decoder runs inside that workgroup
 * right before every unique-word decision (k_rx_sync2 -> rx2_decode_pending, rade_rx.hip).
 *
 * This file: the engine (struct rade_batch in rade_engine.h: open, close, the owner of all its memory), the profiler, transmit, channel, receive and scoring.  The
 * front-end stage calls -- the rate-Rs channel, resampler, wire, rate converter, analog FM and C/No -- and all the state they keep live in rade_stages.c.
 */
#define _GNU_SOURCE          /* sched_getaffinity / CPU_COUNT */

#include <pthread.h>
#include <time.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <math.h>

#include "rade_batch.h"
#include "rade_api.h"
#include "rade_host.h"
#include "rade_engine.h"
#include "rade_pack.h"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "rade: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); goto fail; } } while (0)

/* ---- how rade_batch_rx waits for its stream (the one blocking call of the batched API) -----------------------------------------------------
 * hipStreamSynchronize spins by default: right for one engine per core, wrong when the host has fewer cores than engines in flight -- 8 GPUs x 3
 * batches in flight are 24 host threads, and a container's CPU quota may be 16 (seen on the 1-GPU lease) -- the spinning threads then take the
 * cores the other engines' launch paths need.  Policy: spin while the engines open in this process fit the CPUs the process may use, otherwise
 * sleep until the launch is done (sleep_until_event below: naps between hipEventQuery calls -- waiting on a hipEventBlockingSync event does not sleep on this runtime).
 * $RADE_SYNC=spin|block overrides. */
static int g_engines_open;                 /* engines alive in this process (atomic) */
double rade_host_cpu_quota(void)
{   /* CPUs this process may use: the smaller of its affinity mask and the cgroup v2 quota (cpu.max = "quota period" or "max period") */
    cpu_set_t set; double n = 1.0;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = (double)CPU_COUNT(&set);
    FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (f) {
        char q[64]; double per = 0.0;
        if (fscanf(f, "%63s %lf", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0.0) { const double c = atof(q) / per; if (c > 0.0 && c < n) n = c; }
        fclose(f);
    }
    return n;
}
/* 1 = sleep (sleep_until_event), 0 = spin: a pure function of the two counts (tests/test_host_cpu.py) */
int rade_sync_policy(int engines_open, double cpu_quota) { return (double)engines_open > cpu_quota; }
/* $RADE_SYNC_PEERS = processes that share this process's CPUs and hold as many engines each (one process per GPU under torchrun: the quota is the
 * container's, the engine count this process's -- bench.py sets it to LOCAL_WORLD_SIZE): the policy then compares engines x peers with the quota */
static int g_sync_mode = 2, g_sync_peers = 1; static double g_sync_quota = 1.0;    /* written once (pthread_once), read by every engine's host thread */
static pthread_once_t g_sync_once = PTHREAD_ONCE_INIT;
static void sync_policy_init(void)
{
    const char *e = getenv("RADE_SYNC"), *p = getenv("RADE_SYNC_PEERS");
    g_sync_quota = rade_host_cpu_quota(); g_sync_peers = p && atoi(p) > 1 ? atoi(p) : 1;
    g_sync_mode = e && !strcmp(e, "block") ? 1 : (e && !strcmp(e, "spin") ? 0 : 2);
}
static int sync_blocking_now(void)
{
    pthread_once(&g_sync_once, sync_policy_init);
    return g_sync_mode == 2 ? rade_sync_policy(__atomic_load_n(&g_engines_open, __ATOMIC_RELAXED) * g_sync_peers, g_sync_quota) : g_sync_mode;
}

/* samples per stream of tx_raw, the modulator's output ahead of the Tx band-pass filter (>= the 1152-sample end-of-over frame) */
static long tx_raw_stride(const rade_batch *h) { return (long)(h->max_tx_mf > 2 ? h->max_tx_mf : 2) * RD_NMF; }

/* ---- the engine's memory: every allocation is recorded on the engine (own), and rade_batch_close releases what was recorded ------------------------ */
struct owned { struct owned *next; void *p; int pinned; };
static void *own(rade_batch *h, void *p, int pinned)
{
    struct owned *o = p ? malloc(sizeof *o) : NULL;
    if (p && !o) { if (pinned) hipHostFree(p); else hipFree(p); return NULL; }
    if (o) { o->next = h->owned; o->p = p; o->pinned = pinned; h->owned = o; }
    return p;
}
void disown(rade_batch *h, void *p)       /* release one recorded allocation */
{
    for (struct owned **q = &h->owned; *q; q = &(*q)->next)
        if ((*q)->p == p) { struct owned *o = *q; *q = o->next; if (o->pinned) hipHostFree(p); else hipFree(p); free(o); return; }
}
/* The non-sticky allocators: NULL is the caller's to handle (an optional buffer, or a call after the open that returns -1).  zero = 0: left as allocated.
 * The zeros are complete before returning: the memset runs on the null stream, which is not ordered against a caller's non-blocking stream (a buffer
 * allocated on first use inside a stream-ordered call would otherwise be zeroed on top of what that call's kernels wrote). */
static void *dev_alloc_opt(rade_batch *h, size_t bytes, int zero)
{
    void *d = NULL;
    if (hipMalloc(&d, bytes) != hipSuccess) return NULL;
    if (zero && (hipMemset(d, 0, bytes) != hipSuccess || hipStreamSynchronize(NULL) != hipSuccess)) { hipFree(d); return NULL; }
    return own(h, d, 0);
}
void *dev_upload_opt(rade_batch *h, const void *src, size_t bytes)
{
    void *d = dev_alloc_opt(h, bytes, 0);
    if (d && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) { disown(h, d); return NULL; }
    return d;
}
void *pinned_alloc_opt(rade_batch *h, size_t bytes) { void *p = NULL; return hipHostMalloc(&p, bytes, 0) == hipSuccess ? own(h, p, 1) : NULL; }
static void *must(rade_batch *h, void *p) { if (!p) h->alloc_failed = 1; return p; }      /* the open's: what the engine cannot do without */
static void *dev_upload(rade_batch *h, const void *src, size_t bytes) { return must(h, dev_upload_opt(h, src, bytes)); }
static void *dev_zeros(rade_batch *h, size_t bytes) { return must(h, dev_alloc_opt(h, bytes, 1)); }

/* Scratch that follows the largest call seen: the pointer at ptr_addr (of any object type) holds `need` elements of elem_bytes afterwards (*cap = need; cap = NULL:
 * a fixed size, allocated on first use).  A buffer it replaces is released only once the device is idle: queued work may still read it.  zeroed = 0: left as allocated,
 * for buffers whose every entry is written on the caller's stream before it is read (the receiver's pre-pass): a memset on the null stream could land on top of that. */
int dev_grow(rade_batch *h, void *ptr_addr, long *cap, long need, size_t elem_bytes, int zeroed)
{
    void *p;
    memcpy(&p, ptr_addr, sizeof p);
    if (p && (!cap || need <= *cap)) return 0;
    if (p) { if (hipDeviceSynchronize() != hipSuccess) return -1; disown(h, p); }
    p = dev_alloc_opt(h, elem_bytes * (size_t)need, zeroed);
    memcpy(ptr_addr, &p, sizeof p);
    if (cap) *cap = p ? need : 0;
    return p ? 0 : -1;
}

/* One operand form of W[N][K] on the device: the pointer at plane_addr (of any object type) and *scales.  RD_FRAG_F32: the float32 fragments of k_gemm, no scales.
 * The binary16 layouts: an int8-exact layer (row scales, every w = q row_scale[n]) as ONE plane of the integers q plus its scales -- exact, and half the bytes to
 * stream --, any other layer as two planes of 2^10 w without scales.  optional: the one-plane form or nothing, and the engine can do without the device memory.
 * Returns 0 = packed and uploaded, 1 = the layer has no such form (K is no whole number of k-steps, or optional and not int8-exact): both stay NULL,
 * -1 = a weight does not fit the planes, -2 = no host memory. */
static int upload_form(rade_batch *h, const rd_frag *L, const float *w, const float *row_scale, int N, int K, int optional, void *plane_addr, float **scales)
{
    const int f32 = L == &RD_FRAG_F32, ks = rd_frag_kstep(L), tiles = rd_frag_tiles(L, N);
    const size_t elem = f32 ? sizeof(float) : sizeof(unsigned short);
    void *d = NULL;
    memcpy(plane_addr, &d, sizeof d); *scales = NULL;
    if (!f32 && K % ks) return 1;
    void *p = malloc(elem * (size_t)rd_frag_size(L, tiles, (K + ks - 1) / ks));
    float *sc = malloc(sizeof(float) * (size_t)tiles * L->R);
    if (!p || !sc) { free(p); free(sc); return -2; }
    long n = f32 ? rd_pack_weights(w, N, K, p) : rd_pack_int8(L, w, row_scale, N, K, p, sc);
    const int exact = !f32 && n > 0;
    if (!f32 && !exact && !optional) n = rd_pack_split(L, w, N, K, p);
    if (n > 0) {
        d = optional ? dev_upload_opt(h, p, elem * (size_t)n) : dev_upload(h, p, elem * (size_t)n);
        memcpy(plane_addr, &d, sizeof d);
        if (exact) *scales = optional ? dev_upload_opt(h, sc, sizeof(float) * (size_t)tiles * L->R) : dev_upload(h, sc, sizeof(float) * (size_t)tiles * L->R);
    }
    free(p); free(sc);
    return n > 0 ? 0 : (optional ? 1 : -1);
}

/* W[N][K] (K padded up to Kpad with zero columns) in its three operand forms, and the bias; -1 = a weight does not fit the planes, or no memory */
static int upload_lin(rade_batch *h, dev_lin *d, const float *w, const float *b, const float *row_scale, int N, int K, int Kpad)
{
    float *tmp = NULL, *none;
    if (Kpad != K) {
        if (!(tmp = calloc((size_t)N * Kpad, sizeof(float)))) { h->alloc_failed = 1; return -1; }
        for (int o = 0; o < N; o++) memcpy(tmp + (size_t)o * Kpad, w + (size_t)o * K, sizeof(float) * K);
        w = tmp;
    }
    d->N = N; d->K = Kpad;
    int r = upload_form(h, &RD_FRAG_F32, w, NULL, N, Kpad, 0, &d->wp, &none);
    d->bias = b ? dev_upload(h, b, sizeof(float) * N) : NULL;
    if (r >= 0) r = upload_form(h, &RD_FRAG_B16, w, row_scale, N, Kpad, 0, &d->wp16, &d->wscale16);     /* k_gemm16, k_encf_gemm */
    if (r == -1) fprintf(stderr, "rade: a weight exceeds the range of the split-binary16 operand planes (|w| < 63.9)\n");
    if (r >= 0) r = upload_form(h, &RD_FRAG_A16, w, row_scale, N, Kpad, 0, &d->wa16, &d->wscale);        /* the in-kernel decoder's 16x16x32 products */
    free(tmp);
    if (r == -2) h->alloc_failed = 1;
    return (r >= 0 && d->wp && (!b || d->bias)) ? 0 : -1;
}

/* start-of-utterance state, ONE launch (k_batch_reset) for the directions asked for; the trace buffers and the Tx filter state only where they exist */
static void reset_on(rade_batch *h, int tx, int rx, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    rd_reset_args r;
    memset(&r, 0, sizeof r);
    r.B = h->B;
    if (rx) {
        r.st = h->rx_st; r.seeds = h->d_lcg_seeds; r.foff_err = (h->flags & RADE_FOFF_TEST) ? 10.0 : 0.0;   /* rade_api.c:263-264 */
        r.dec_h = h->dec_h[0];                             /* the five layers' states are one allocation */
        /* only a stream's history row has to start from zero: every other row of dec_x is written before it is read */
        r.dec_x = h->dec_x; r.dec_x_sb = (long)(1 + h->dec_rows) * RD_DEC_W;
        if (h->trace) { hipMemsetAsync(h->trace, 0, sizeof(rd_rx_trace) * (size_t)h->B * h->trace_cap, st); hipMemsetAsync(h->trace_z, 0, sizeof(float) * (size_t)h->B * h->trace_cap * RD_ZMF, st); }
    }
    if (tx) {
        h->enc_hist_frag = 0;
        if (h->tx_bpf) hipMemcpyAsync(h->tx_bpf, h->tx_bpf_init, sizeof(rd_bpf_state) * h->B, hipMemcpyDeviceToDevice, st);
        r.enc_h = h->enc_h[0];
        /* the two history rows of each stream (conv taps before the first frame); rows 2.. are written layer by layer before they are read */
        r.enc_x = h->enc_x; r.enc_x_sb = (long)(2 + h->Tcap) * RD_ENC_W;
    }
    rd_launch_reset(&r, st);
}

void rade_batch_rx_reset(rade_batch *h) { ON_DEV(h); reset_on(h, 0, 1, NULL); hipDeviceSynchronize(); }

/* stream-ordered reset of both directions (start of a new batch of utterances) */
void rade_batch_reset(rade_batch *h, void *stream) { ON_DEV(h); reset_on(h, 1, 1, stream); }

void rade_batch_rx_set_lcg(rade_batch *h, const unsigned *seeds_host)
{
    ON_DEV(h);
    if (!h) return;
    for (int b = 0; b < h->B; b++) h->lcg_seeds[b] = seeds_host ? seeds_host[b] : 1u;
    hipMemcpy(h->d_lcg_seeds, h->lcg_seeds, sizeof(unsigned) * h->B, hipMemcpyHostToDevice);
    rade_batch_rx_reset(h);
}

void rade_batch_tx_reset(rade_batch *h) { ON_DEV(h); reset_on(h, 1, 0, NULL); hipDeviceSynchronize(); }

rade_batch *rade_batch_open_mem(const void *blob, size_t blob_len, const rade_batch_config *cfg)
{
    rade_batch *h = NULL;
    rd_model m; int have_model = 0;
    if (!cfg || cfg->n_streams <= 0 || cfg->max_tx_mf <= 0) { fprintf(stderr, "rade: bad batch config\n"); return NULL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "rade: no HIP device available -- this library has no CPU fallback\n");
        return NULL;
    }
    CHK(hipSetDevice(cfg->device));
    if (rd_model_parse(blob, blob_len, &m)) return NULL;
    have_model = 1;
    h = calloc(1, sizeof *h);
    if (!h) { rd_model_free(&m); return NULL; }
    __atomic_add_fetch(&g_engines_open, 1, __ATOMIC_RELAXED);
    h->B = cfg->n_streams; h->max_tx_mf = cfg->max_tx_mf; h->device = cfg->device; h->flags = cfg->flags;
    h->trace_cap = cfg->rx_trace_calls; h->Tcap = 3 * cfg->max_tx_mf;
    h->unsync_off_after = cfg->disable_unsync != 0.0f ? (int)((double)cfg->disable_unsync * 8000.0 / RD_NMF) : -1;    /* radae_rxe.py:279-280 */
    const size_t B = (size_t)h->B, T = (size_t)h->Tcap;
    /* do_radae_rx calls per stream and launch (the per-launch bookkeeping arrays hold RD_RX_ROUND_MAX); RADE_ROUND_CALLS
     * lowers it for tests: the call loop then takes several launches with identical results */
    h->R = getenv("RADE_ROUND_CALLS") ? atoi(getenv("RADE_ROUND_CALLS")) : RD_RX_ROUND_MAX;
    if (h->R < 1) h->R = 1;
    if (h->R > RD_RX_ROUND_MAX) h->R = RD_RX_ROUND_MAX;
    /* rows a stream may hold before its decoder stage runs: 8 frames wait for a unique-word check, up to 7 more can be
     * left over from before a loss of sync */
    h->dec_rows = getenv("RADE_DEC_ROWS") ? atoi(getenv("RADE_DEC_ROWS")) : 48;
    if (h->dec_rows < 3) h->dec_rows = 3;
    if (h->dec_rows > 63) h->dec_rows = 63;            /* the stage's LDS row flags hold DQ_PEND_MAX = 64 entries (rade_kernels.hip) */
    const size_t DR = (size_t)h->dec_rows;

    {   /* the constant tables, and the four of them that are matrix-core operands (rade_pack.c), through one host buffer */
        _Static_assert(RD_CORRQ16_HALFS >= RD_CORRA16_HALFS && RD_CORRQ16_HALFS >= RD_WFWD16_HALFS && RD_CORRQ16_HALFS >= RD_BPF16_HALFS, "t16 holds the largest table");
        rd_tables *tab = malloc(sizeof *tab); rd_corr_basis *basis = malloc(sizeof *basis);
        unsigned short *t16 = malloc(sizeof(unsigned short) * RD_CORRQ16_HALFS);
        if (tab && basis && t16) {
            rd_tables_fill(tab);
            h->d_tab = dev_upload(h, tab, sizeof *tab);
            /* the pilot correlator in two stages: 16 polynomial moments, then their expansion to the 40 frequencies; one basis serves both */
            rd_corr_basis_fill(tab, basis);
            rd_corrq16_fill(tab, basis, t16); h->corrq16 = dev_upload(h, t16, sizeof(unsigned short) * RD_CORRQ16_HALFS);
            rd_corra16_fill(tab, basis, t16); h->corra16 = dev_upload(h, t16, sizeof(unsigned short) * RD_CORRA16_HALFS);
            rd_wfwd16_table_fill(tab, t16); h->wfwd16 = dev_upload(h, t16, sizeof(unsigned short) * RD_WFWD16_HALFS);    /* the demodulator DFT matrix (k_rx_sync2) */
            rd_bpf16_table_fill(tab, t16); h->bpf16 = dev_upload(h, t16, sizeof(unsigned short) * RD_BPF16_HALFS);       /* the band-pass taps (k_bpf_fir) */
        } else h->alloc_failed = 1;
        free(tab); free(basis); free(t16);
    }
    {   /* ((n - 79.5) / 80)^m, m = 0..7, by repeated multiplication (the order the kernels build their LDS copy in) */
        double vm[8][RD_M];
        for (int n = 0; n < RD_M; n++) { const double nu = ((double)n - 79.5) / 80.0; double v = 1.0; for (int m = 0; m < 8; m++) { vm[m][n] = v; v *= nu; } }
        h->vm = dev_upload(h, vm, sizeof vm);
    }
    /* the receiver kernel asks for more dynamic LDS than the 64 KB default: raised here, once per engine and before any launch (the
     * attribute belongs to the device's code object; setting it again from another engine's thread is harmless) */
    h->rx_lds = rd_rx_sync_prepare();
    h->rx_census = getenv("RADE_RX2_CENSUS") ? atoi(getenv("RADE_RX2_CENSUS")) : 0;      /* only acts in -DRX2_CENSUS builds */
    if (h->alloc_failed || h->rx_lds <= 0) goto fail;

    int err = 0;
    h->feat_in = m.enc_dense1.n_in; h->enc_kpad = (h->feat_in + 15) & ~15; h->bottleneck1 = (cfg->flags & RADE_BATCH_BOTTLENECK1) != 0;
    err |= upload_lin(h, &h->enc_dense1, m.enc_dense1.w, m.enc_dense1.b, NULL, RM_ENC_D1, h->feat_in, h->enc_kpad);
    err |= upload_lin(h, &h->enc_zdense, m.enc_zdense.w, m.enc_zdense.b, NULL, RM_LATENT, RM_ENC_W, RM_ENC_W);
    err |= upload_lin(h, &h->dec_dense1, m.dec_dense1.w, m.dec_dense1.b, NULL, RM_DEC_D1, RM_LATENT, RM_LATENT);
    err |= upload_lin(h, &h->dec_output, m.dec_output.w, m.dec_output.b, NULL, h->feat_in, RM_DEC_W, RM_DEC_W);
    for (int l = 0; l < RM_NL && !err; l++) {
        err |= upload_lin(h, &h->enc_gin[l], m.enc_gru[l].w_ih, m.enc_gru[l].b_ih, m.enc_gru[l].s_ih, RM_ENC_G, RM_ENC_GRU_IN(l), RM_ENC_GRU_IN(l));
        err |= upload_lin(h, &h->dec_gin[l], m.dec_gru[l].w_ih, m.dec_gru[l].b_ih, m.dec_gru[l].s_ih, RM_DEC_G, RM_DEC_GRU_IN(l), RM_DEC_GRU_IN(l));
        err |= upload_lin(h, &h->enc_conv[l], m.enc_conv[l].w, m.enc_conv[l].b, m.enc_conv[l].row_scale, RM_ENC_CONV, m.enc_conv[l].n_in, m.enc_conv[l].n_in);
        err |= upload_lin(h, &h->dec_conv[l], m.dec_conv[l].w, m.dec_conv[l].b, m.dec_conv[l].row_scale, RM_DEC_CONV, m.dec_conv[l].n_in, m.dec_conv[l].n_in);
        err |= upload_lin(h, &h->dec_glu[l], m.dec_glu[l].w, NULL, m.dec_glu[l].row_scale, RM_DEC_GLU, RM_DEC_H, RM_DEC_H);
        h->enc_whh[l] = dev_upload(h, m.enc_gru[l].w_hh, sizeof(float) * RM_ENC_G * RM_ENC_H);
        h->enc_bhh[l] = dev_upload(h, m.enc_gru[l].b_hh, sizeof(float) * RM_ENC_G);
        h->dec_whh[l] = dev_upload(h, m.dec_gru[l].w_hh, sizeof(float) * RM_DEC_G * RM_DEC_H);
        h->dec_bhh[l] = dev_upload(h, m.dec_gru[l].b_hh, sizeof(float) * RM_DEC_G);
        (void)upload_form(h, &RD_FRAG_A16, m.dec_gru[l].w_hh, m.dec_gru[l].s_hh, RM_DEC_G, RM_DEC_H, 1, &h->dec_whq[l], &h->dec_whs[l]);   /* int8-exact, or k_rx_sync2 scans in float32 */
    }
    if (err || h->alloc_failed) { fprintf(stderr, "rade: weight upload failed\n"); goto fail; }

    h->enc_xin = dev_zeros(h, sizeof(float) * B * T * RD_ENC_IN);
    h->enc_x = dev_zeros(h, sizeof(float) * B * (2 + T) * RD_ENC_W);
    h->enc_gi = dev_zeros(h, sizeof(float) * B * T * RM_ENC_G);
    h->enc_nq = 1 + (h->Tcap + 31) / 32;
    h->enc_seq_taps = getenv("RADE_ENCF_SEQ_TAPS") != NULL;    /* developer switches, read per engine (rade_enc.hip: k_encf_gemm) */
    h->enc_no_pair = getenv("RADE_ENCF_NO_PAIR") != NULL;
    if (B * T > 16384 && !getenv("RADE_ENC_ROWS")) {       /* $RADE_ENC_ROWS: the float32-row path (k_gemm16p) for every size: A/B and the equality test */
        h->enc_xf = dev_alloc_opt(h, sizeof(unsigned short) * B * h->enc_nq * RD_EF_TILE, 1);   /* (NULL = no memory for it: the float32-row kernels serve every call) */
        if (!h->enc_xf && !getenv("RADE_VERBOSE_0"))
            fprintf(stderr, "rade: no device memory for the encoder's fragment buffer (%.1f MB): the float32-row kernels serve every call (slower encoder GEMMs, same results to the last bits documented in rade_batch.h)\n",
                    1e-6 * sizeof(unsigned short) * (double)B * h->enc_nq * RD_EF_TILE);
    }
    h->enc_z = dev_zeros(h, sizeof(float) * B * T * RD_LATENT);
    h->eoo = dev_zeros(h, sizeof(float) * B * RD_NEOO * 2);
    h->eoo_bits = dev_zeros(h, sizeof(float) * B * RD_NEOOBITS);
    h->bypass_dec = (cfg->flags & RADE_BATCH_BYPASS_DEC) != 0;
    h->tx_linear = (cfg->flags & RADE_BATCH_TX_LINEAR) != 0;
    if (h->tx_linear && (cfg->flags & RADE_BATCH_TX_BPF)) { fprintf(stderr, "rade: RADE_BATCH_TX_LINEAR cannot be combined with RADE_BATCH_TX_BPF (the filter clips)\n"); goto fail; }
    if (cfg->flags & RADE_BATCH_TX_BPF) {
        rd_bpf_state *init = calloc(B, sizeof *init);
        if (!init) goto fail;
        for (size_t b = 0; b < B; b++) { init[b].mem_len = 100; init[b].phase[0] = 1.0f; }    /* complex_bpf.__init__: dsp.py:54-60 */
        h->tx_bpf_init = dev_upload(h, init, sizeof(rd_bpf_state) * B); h->tx_bpf = dev_upload(h, init, sizeof(rd_bpf_state) * B);
        free(init);
        h->tx_raw = dev_zeros(h, sizeof(float) * 2 * B * tx_raw_stride(h));
        h->tx_chain = dev_zeros(h, sizeof(float) * 2 * B * (cfg->max_tx_mf + 8));
        h->eoo_filt = dev_zeros(h, sizeof(float) * 2 * B * RD_NEOO);
    }
    h->chan_scratch = dev_zeros(h, sizeof(double) * B * (1 + (cfg->max_tx_mf > 64 ? cfg->max_tx_mf : 64)) * 2);   /* rd_chan_args.scratch */
    /* one allocation each: the five layers' states; progress word, per-stream counters and status, in the order of the host copy (rade_batch_rx: one transfer back per invocation) */
    h->enc_h[0] = dev_zeros(h, sizeof(float) * RM_NL * B * RM_ENC_H); h->dec_h[0] = dev_zeros(h, sizeof(float) * RM_NL * B * RM_DEC_H);
    h->dec2_h[0] = dev_zeros(h, sizeof(float) * RM_NL * B * RM_DEC_H);
    h->rx_progress = dev_zeros(h, sizeof(int) * (8 + B * 8));
    if (h->alloc_failed) { fprintf(stderr, "rade: device allocation failed\n"); goto fail; }
    for (int l = 1; l < RM_NL; l++) { h->enc_h[l] = h->enc_h[0] + (size_t)l * B * RM_ENC_H; h->dec_h[l] = h->dec_h[0] + (size_t)l * B * RM_DEC_H; }
    for (int l = 1; l < RM_NL; l++) h->dec2_h[l] = h->dec2_h[0] + (size_t)l * B * RM_DEC_H;
    h->rx_acc = h->rx_progress + 8; h->rx_status = h->rx_progress + 8 + 4 * B;
    h->rx_st = dev_zeros(h, sizeof(rd_rx_stream) * B);
    h->rx_round = dev_zeros(h, sizeof(rd_rx_round) * B);
    h->rx_avail = dev_zeros(h, sizeof(int) * B);
    h->wg_cycles = dev_zeros(h, sizeof(long long) * B);
    h->zrows = dev_zeros(h, sizeof(float) * B * DR * RD_LATENT);
    h->dec_x = dev_zeros(h, sizeof(float) * B * (1 + DR) * RD_DEC_W);
    h->dec_gi = dev_zeros(h, sizeof(float) * B * DR * RM_DEC_G);
    h->dec_hbuf = dev_zeros(h, sizeof(float) * B * DR * RM_DEC_H);
    h->feat84 = dev_zeros(h, sizeof(float) * B * DR * RM_FEAT_AUX);
    h->dec2_x = dev_zeros(h, sizeof(float) * B * (1 + T) * RD_DEC_W);
    h->dec2_gi = dev_zeros(h, sizeof(float) * B * T * RM_DEC_G);
    h->dec2_hbuf = dev_zeros(h, sizeof(float) * B * T * RM_DEC_H);
    h->dtcache = dev_zeros(h, sizeof(float) * B * 2 * RD_NMF * RD_NFC);
    if (h->trace_cap > 0) {
        h->trace = dev_zeros(h, sizeof(rd_rx_trace) * B * h->trace_cap);
        h->trace_z = dev_zeros(h, sizeof(float) * B * h->trace_cap * RD_ZMF);
    }
    h->h_small = must(h, pinned_alloc_opt(h, sizeof(int) * (8 + B * 8)));
    h->lcg_seeds = malloc(sizeof(unsigned) * B);
    for (size_t b = 0; b < B; b++) h->lcg_seeds[b] = 1u;
    h->d_lcg_seeds = dev_upload(h, h->lcg_seeds, sizeof(unsigned) * B);
    if (h->alloc_failed) { fprintf(stderr, "rade: device allocation failed\n"); goto fail; }
    for (int i = 0; i < 2 * RADE_PROF_MAXEV; i++) CHK(hipEventCreate(&h->prof_ev[i]));
    CHK(hipEventCreateWithFlags(&h->ev_block, hipEventBlockingSync | hipEventDisableTiming));
    rade_batch_rx_reset(h);
    if (rd_launch_eoo_build(h->d_tab, NULL, h->eoo, h->B, NULL)) goto fail;
    CHK(hipDeviceSynchronize());
    rd_model_free(&m);
    return h;
fail:
    if (have_model) rd_model_free(&m);
    if (h) rade_batch_close(h);
    return NULL;
}

rade_batch *rade_batch_open(const char *blob_path, const rade_batch_config *cfg)
{
    FILE *f = blob_path ? fopen(blob_path, "rb") : NULL;
    if (!f) { fprintf(stderr, "rade: cannot open weight blob %s\n", blob_path ? blob_path : "(null)"); return NULL; }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    void *buf = malloc(n);
    if (fread(buf, 1, n, f) != (size_t)n) { fclose(f); free(buf); return NULL; }
    fclose(f);
    rade_batch *h = rade_batch_open_mem(buf, n, cfg);
    free(buf);
    return h;
}

void rade_batch_close(rade_batch *h)
{
    if (!h) return;
    ON_DEV(h);
    while (h->owned) disown(h, h->owned->p);
    if (h->ev_block) hipEventDestroy(h->ev_block);
    if (h->stages) rd_stages_free(h->stages);
    __atomic_sub_fetch(&g_engines_open, 1, __ATOMIC_RELAXED);
    for (int i = 0; i < 2 * RADE_PROF_MAXEV; i++) if (h->prof_ev[i]) hipEventDestroy(h->prof_ev[i]);
    free(h->lcg_seeds);
    free(h);
}

int rade_batch_n_streams(const rade_batch *h) { return h->B; }
const rd_tables *rd_batch_tables(const rade_batch *h) { return h->d_tab; }
int rd_batch_has_tx_bpf(const rade_batch *h) { return h->tx_bpf != NULL; }

/* ---- per-kernel-class timing (HIP events on the launch stream) -------------------------------- */
/* Events are only recorded while the work is queued and read back afterwards (prof_drain): a profiled step runs back to
 * back like a timed one, without a host synchronisation (and the clock ramp-down that follows it) after every kernel. */
void prof_drain(rade_batch *h)
{
    for (int i = 0; i < h->prof_cnt; i++) {
        float ms = 0;
        if (hipEventSynchronize(h->prof_ev[2 * i + 1]) == hipSuccess && hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]) == hipSuccess) {
            h->prof_ms[h->prof_cls[i]] += ms; h->prof_flops[h->prof_cls[i]] += h->prof_fl[i]; h->prof_n[h->prof_cls[i]]++;
            float t0 = 0;
            if (h->prof_ref && h->iv_n < RADE_PROF_MAXIV && hipEventElapsedTime(&t0, h->prof_ref, h->prof_ev[2 * i]) == hipSuccess) {
                h->iv_cls[h->iv_n] = h->prof_cls[i]; h->iv_t0[h->iv_n] = t0; h->iv_t1[h->iv_n] = t0 + ms; h->iv_n++;
            }
        }
    }
    h->prof_cnt = 0;
}

void rade_batch_profile(rade_batch *h, int enable)
{
    ON_DEV(h);
    if (!enable && h->prof_on) prof_drain(h);
    h->prof_on = enable;
    if (enable) { h->prof_cnt = 0; h->iv_n = 0; memset(h->prof_ms, 0, sizeof h->prof_ms); memset(h->prof_flops, 0, sizeof h->prof_flops); memset(h->prof_n, 0, sizeof h->prof_n); }
}
/* launches of class `cls` since profiling was enabled as [start, end] in ms after `ref_event` (a hipEvent_t of the caller, recorded and
 * complete before the first launch): call rade_batch_profile_ref before enabling, read the intervals after disabling */
void rade_batch_profile_ref(rade_batch *h, void *ref_event) { h->prof_ref = (hipEvent_t)ref_event; }
int rade_batch_profile_intervals(rade_batch *h, int cls, float *t0_ms, float *t1_ms, int max)
{
    ON_DEV(h);
    prof_drain(h);
    int n = 0;
    for (int i = 0; i < h->iv_n && n < max; i++) if (h->iv_cls[i] == cls) { t0_ms[n] = h->iv_t0[i]; t1_ms[n] = h->iv_t1[i]; n++; }
    return n;
}
int rade_batch_profile_get(rade_batch *h, int cls, double *ms, double *work, long *launches)
{
    ON_DEV(h);
    if (cls < 0 || cls >= RADE_PROF_NCLASS) return -1;
    prof_drain(h);
    *ms = h->prof_ms[cls]; *work = h->prof_flops[cls]; *launches = h->prof_n[cls];
    return 0;
}

/* The caller's buffers that a kernel reads or writes as 16-byte words (include/rade_batch.h, "Buffers, strides and alignment"): refused on the host, before
 * any launch, when they are not 16-byte aligned.  Every other caller buffer is accessed element by element. */
static int misaligned16(const void *p) { return ((uintptr_t)p & 15) != 0; }

/* ---- one GEMM launch helper ------------------------------------------------------------------ */
static int gemm(rade_batch *hh, const dev_lin *w, const float *a1, long a1_sb, long a1_st, int K1, const float *a0, long a0_sb, long a0_st, int K0,
                float *y, long y_sb, long y_st, int B, int T, int act, void *stream)
{
    rd_gemm_args g;
    memset(&g, 0, sizeof g);
    g.a1 = a1; g.a1_sb = a1_sb; g.a1_st = a1_st; g.K1 = K1; g.a0 = a0; g.a0_sb = a0_sb; g.a0_st = a0_st; g.K0 = K0;
    g.Wp = w->wp; g.Wp16 = w->wp16; g.Wscale = w->wp16 ? w->wscale16 : NULL; g.bias = w->bias; g.y = y; g.y_sb = y_sb; g.y_st = y_st; g.N = w->N; g.B = B; g.T = T; g.act = act;
    if (K0 + K1 != w->K) { fprintf(stderr, "rade: internal GEMM shape error (%d+%d != %d)\n", K0, K1, w->K); return -1; }
    PROF_BEGIN(hh, stream);
    const int rc = rd_launch_gemm(&g, stream);
    PROF_END(hh, stream, RADE_PROF_GEMM, 2.0 * (double)B * T * (K0 + K1) * w->N);
    return rc;
}

/* ---- CoreEncoderStatefull.forward over T steps for all streams (radae_base.py:260-286); xin = [B][T][enc_kpad] ----
 * Layer by layer over all B x T rows, in one pass on the caller's stream: the feed-forward pieces are GEMMs, the five W_hh recurrences
 * serial scans (one workgroup of four wavefronts per stream: latency-bound, most of the chip idle).  Measured and not kept
 * (profiles/r03_tx_side_ab.json): the steps cut into two time chunks on two HIP streams, one recurrence apart, gain 3 % with one batch
 * in flight and lose 7 % with two. */
/* The same pass with the concat buffer kept as matrix-core operand fragments (rade_enc.hip): taken when the call has enough rows for the batched GEMMs
 * (the float32-row path below serves short calls with k_gemm_splitk); the conv history crosses calls in enc_x's two float32 rows either way.  conv_l and
 * the product behind it are separate launches: one fused launch was slower in the pipelined bench. */
static int encf_gemm(rade_batch *h, const dev_lin *w, int K1, int K0, int dil, float *y, long y_sb, long y_st, int ycol, int T, int act, void *stream)
{
    rd_encf_args g;
    memset(&g, 0, sizeof g);
    g.xf = h->enc_xf; g.NQ = h->enc_nq; g.B = h->B; g.T = T; g.K0 = K0; g.K1 = K1; g.dil = dil;
    g.Wp16 = w->wp16; g.Wscale = w->wscale16; g.bias = w->bias; g.N = w->N; g.act = act;
    g.y = y; g.y_sb = y_sb; g.y_st = y_st; if (!y) { g.yf = h->enc_xf; g.ycol = ycol; }
    g.seq_taps = h->enc_seq_taps; g.no_pair = h->enc_no_pair;
    if (K0 + K1 != w->K || !w->wp16) { fprintf(stderr, "rade: internal GEMM shape error (%d+%d != %d)\n", K0, K1, w->K); return -1; }
    PROF_BEGIN(h, stream);
    const int rc = rd_launch_encf_gemm(&g, stream);
    PROF_END(h, stream, RADE_PROF_GEMM, 2.0 * (double)h->B * T * (K0 + K1) * w->N);
    return rc;
}
static int encode_core_frag(rade_batch *h, int T, float *z, void *stream)
{
    const int B = h->B;
    /* history rows: float32 -> planes only when the float32 rows are the newer ones (after a reset or a short call).  After a fragment pass the tile already holds the
     * planes themselves: rebuilding them from 2^-8 (hi + lo) would re-split a pair whose low plane is exactly half an ulp of the high one differently (round to even) --
     * the same sum, other partial products, last-bit differences against the float32-row kernels in about one stream of 400 per call */
    int e = h->enc_hist_frag ? 0 : rd_launch_encf_hist(h->enc_xf, h->enc_nq, h->enc_x, (long)(2 + h->Tcap) * RD_ENC_W, B, T, 0, stream);
    {
        rd_encf_args g;
        memset(&g, 0, sizeof g);
        g.xf = h->enc_xf; g.NQ = h->enc_nq; g.B = B; g.T = T; g.bias = h->enc_dense1.bias; g.N = RM_ENC_D1; g.act = 1; g.yf = h->enc_xf; g.ycol = 0;
        g.xin = h->enc_xin; g.Kin = h->enc_kpad; g.Wp = h->enc_dense1.wp;
        PROF_BEGIN(h, stream); e |= rd_launch_encf_dense1(&g, stream); PROF_END(h, stream, RADE_PROF_GEMM, 2.0 * (double)B * T * h->enc_kpad * RM_ENC_D1);
    }
    e |= encf_gemm(h, &h->enc_gin[0], RM_ENC_GRU_IN(0), 0, 0, h->enc_gi, (long)T * RM_ENC_G, RM_ENC_G, 0, T, 0, stream);
    for (int l = 0; l < RM_NL && !e; l++) {
        const int in = RM_ENC_GRU_IN(l), cin = RM_ENC_CONV_IN(l);
        rd_scan_args s = { h->enc_gi, (long)T * RM_ENC_G, RM_ENC_G, h->enc_whh[l], h->enc_bhh[l], h->enc_h[l], NULL, 0, 0, NULL, 0, NULL, B, T, RM_ENC_H, h->enc_xf, h->enc_nq, in };
        PROF_BEGIN(h, stream); e |= rd_launch_gru_scan(&s, stream); PROF_END(h, stream, RADE_PROF_SCAN, 2.0 * B * T * RM_ENC_G * RM_ENC_H);
        e |= encf_gemm(h, &h->enc_conv[l], cin, cin, RM_ENC_DIL(l), NULL, 0, 0, cin, T, 1, stream);
        if (l + 1 < RM_NL) e |= encf_gemm(h, &h->enc_gin[l + 1], RM_ENC_GRU_IN(l + 1), 0, 0, h->enc_gi, (long)T * RM_ENC_G, RM_ENC_G, 0, T, 0, stream);
        else e |= encf_gemm(h, &h->enc_zdense, RM_ENC_W, 0, 0, z, (long)T * RD_LATENT, RD_LATENT, 0, T, h->bottleneck1 ? 1 : 0, stream);
    }
    e |= rd_launch_encf_hist(h->enc_xf, h->enc_nq, h->enc_x, (long)(2 + h->Tcap) * RD_ENC_W, B, T, 1, stream);
    h->enc_hist_frag = !e;
    return e;
}

static int encode_core(rade_batch *h, int T, float *z, void *stream)
{
    const int B = h->B, W = RD_ENC_W;
    if (h->enc_xf && (long)B * T > 16384) return encode_core_frag(h, T, z, stream);
    h->enc_hist_frag = 0;
    const long xsb = (long)(2 + h->Tcap) * W;
    float *x0 = h->enc_x + 2 * W;              /* time row 0 of each stream; rows -2,-1 hold the conv history */
    int e = 0;
    /* dense1 reads raw features: the one encoder operand that is not tanh-bounded, so it stays on the f32 matrix cores
     * (the 2^8-scaled binary16 planes of the split-f16 kernels overflow beyond +-255.9) */
    dev_lin d1 = h->enc_dense1; d1.wp16 = NULL; d1.wscale16 = NULL;
    e |= gemm(h, &d1, h->enc_xin, (long)T * h->enc_kpad, h->enc_kpad, h->enc_kpad, NULL, 0, 0, 0, x0, xsb, W, B, T, 1, stream);
    for (int l = 0; l < RM_NL && !e; l++) {
        const int in = RM_ENC_GRU_IN(l), cin = RM_ENC_CONV_IN(l);
        e |= gemm(h, &h->enc_gin[l], x0, xsb, W, in, NULL, 0, 0, 0, h->enc_gi, (long)T * RM_ENC_G, RM_ENC_G, B, T, 0, stream);
        rd_scan_args s = { h->enc_gi, (long)T * RM_ENC_G, RM_ENC_G, h->enc_whh[l], h->enc_bhh[l], h->enc_h[l], x0 + in, xsb, W, NULL, 0, NULL, B, T, RM_ENC_H };
        PROF_BEGIN(h, stream); e |= rd_launch_gru_scan(&s, stream); PROF_END(h, stream, RADE_PROF_SCAN, 2.0 * B * T * RM_ENC_G * RM_ENC_H);
        e |= gemm(h, &h->enc_conv[l], x0, xsb, W, cin, x0 - (long)RM_ENC_DIL(l) * W, xsb, W, cin, x0 + cin, xsb, W, B, T, 1, stream);
    }
    /* bottleneck 1: z = tanh(z_dense) (radae_base.py:281-284); bottleneck 3: linear */
    e |= gemm(h, &h->enc_zdense, x0, xsb, W, W, NULL, 0, 0, 0, z, (long)T * RD_LATENT, RD_LATENT, B, T, h->bottleneck1 ? 1 : 0, stream);
    e |= rd_launch_carry_rows(h->enc_x, B, h->Tcap, W, 2, T, NULL, stream);
    return e;
}

/* the optional Tx band-pass filter + magnitude clip (radae_txe.py:130-132, :141-143) over the n samples the modulator left in tx_raw: the receiver's
 * filtering pass with frames as blocks (len0 = the first frame: 960, or the 1152-sample end-of-over frame), every sample consumed (advance = 0: the filter state is left as it was) */
static int tx_bpf_pass(rade_batch *h, int n, int len0, void *out, long out_stride, void *stream, int advance)
{
    rd_bpf_args ba;
    memset(&ba, 0, sizeof ba);
    ba.state = h->tx_bpf; ba.state_stride = sizeof(rd_bpf_state); ba.len0_const = len0; ba.avail_const = n;
    ba.tab = h->d_tab; ba.bpf16 = h->bpf16; ba.x = h->tx_raw; ba.x_stride = tx_raw_stride(h); ba.y = out; ba.y_stride = out_stride;
    ba.chain = h->tx_chain; ba.chain_stride = h->max_tx_mf + 8; ba.n_blocks = 1 + (n > len0 ? (n - len0 + RD_NMF - 1) / RD_NMF : 0); ba.B = h->B; ba.clip = 1; ba.advance = advance;
    PROF_BEGIN(h, stream);
    const int rc = rd_launch_bpf(&ba, stream);
    PROF_END(h, stream, RADE_PROF_BPF, 8.0 * 101.0 * (double)h->B * n);
    return rc;
}

/* the transmitter's front: the features packed into the encoder's input rows (enc_xin), then the core encoder */
static int encode_features(rade_batch *h, const float *features_dev, int T, float *z, void *stream)
{
    const int e = rd_launch_enc_pack(features_dev, h->enc_xin, h->B, T, stream);
    return e | encode_core(h, T, z, stream);
}
/* and its tail: the modulator, into tx_raw and through the Tx band-pass filter where the engine has one */
static int modulate(rade_batch *h, const float *z, int n_mf, void *iq_out, long iq_stride, void *stream)
{
    void *mod_out = h->tx_bpf ? h->tx_raw : iq_out; const long mod_stride = h->tx_bpf ? tx_raw_stride(h) : iq_stride;
    PROF_BEGIN(h, stream);
    int e = rd_launch_ofdm_mod(h->d_tab, z, mod_out, mod_stride, h->B, n_mf, h->tx_linear, stream);
    PROF_END(h, stream, RADE_PROF_MOD, 8.0 * h->B * n_mf * 5 * 30 * 160);
    if (h->tx_bpf) e |= tx_bpf_pass(h, n_mf * RD_NMF, RD_NMF, iq_out, iq_stride, stream, 1);
    return e;
}

/* ---- transmit (radae_txe.py:108-135 for n_mf modem frames and B streams at once) -------------- */
int rade_batch_tx(rade_batch *h, const float *features_dev, int n_mf, void *iq_out_dev, long iq_stride, float *z_out_dev, void *stream)
{
    ON_DEV(h);
    if (!h || !features_dev || !iq_out_dev || n_mf <= 0 || n_mf > h->max_tx_mf || h->feat_in != RM_FEAT_AUX) return -1;
    if (misaligned16(z_out_dev)) return -1;           /* encf_emit (rade_enc.hip) stores the latents of a large call as f32x4 */
    float *z = z_out_dev ? z_out_dev : h->enc_z;
    int e = encode_features(h, features_dev, 3 * n_mf, z, stream);
    e |= modulate(h, z, n_mf, iq_out_dev, iq_stride, stream);
    return e ? -1 : n_mf * RD_NMF;
}

/* radae_txe.py --bypass_enc (:124-126): latents in, the modulator (+ Tx band-pass filter) as rade_batch_tx runs it */
int rade_batch_tx_latents(rade_batch *h, const float *z_dev, int n_mf, void *iq_out_dev, long iq_stride, void *stream)
{
    ON_DEV(h);
    if (!h || !z_dev || !iq_out_dev || n_mf <= 0 || n_mf > h->max_tx_mf) return -1;
    return modulate(h, z_dev, n_mf, iq_out_dev, iq_stride, stream) ? -1 : n_mf * RD_NMF;
}

/* ---- core encoder / decoder alone (the rade_core_encoder / rade_core_decoder level, src/rade_core.h:42-46) ---- */
int rade_batch_encode(rade_batch *h, const float *features_dev, int n_steps, float *z_out_dev, void *stream)
{
    ON_DEV(h);
    if (!h || !features_dev || n_steps <= 0 || n_steps > h->Tcap || !z_out_dev) return -1;
    if (misaligned16(z_out_dev)) return -1;           /* encf_emit (rade_enc.hip) stores the latents of a large call as f32x4 */
    int e = rd_launch_pad_rows(features_dev, h->enc_xin, (long)h->B * n_steps, h->feat_in, h->enc_kpad, stream);
    e |= encode_core(h, n_steps, z_out_dev, stream);
    return e ? -1 : n_steps;
}

int rade_batch_tx_set_eoo_bits(rade_batch *h, const float *bits_host)
{
    ON_DEV(h);
    if (bits_host && hipMemcpy(h->eoo_bits, bits_host, sizeof(float) * h->B * RD_NEOOBITS, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (rd_launch_eoo_build(h->d_tab, bits_host ? h->eoo_bits : NULL, h->eoo, h->B, NULL)) return -1;
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

int rade_batch_tx_eoo(rade_batch *h, void *iq_out_dev, long iq_stride, void *stream)
{
    if (!h || !iq_out_dev) return -1;
    ON_DEV(h);
    if (h->tx_linear) return -1;           /* the end-of-over frame is built with the bottleneck-3 pilot gain and limiter */
    if (!h->tx_bpf) return rd_launch_copy_eoo(h->eoo, iq_out_dev, iq_stride, h->B, stream) ? -1 : RD_NEOO;
    int e = rd_launch_copy_eoo(h->eoo, h->tx_raw, tx_raw_stride(h), h->B, stream);
    e |= tx_bpf_pass(h, RD_NEOO, RD_NEOO, iq_out_dev, iq_stride, stream, 1);
    return e ? -1 : RD_NEOO;
}

/* ---- channel ----------------------------------------------------------------------------------- */
float rade_sigma_from_EbNodB(float EbNodB)
{   /* radae.py:567-573 (bottleneck 3): sigma = sqrt(Fs/(EbNo*Rb)), Rb = latent_dim/Tz */
    const float EbNo = powf(10.0f, EbNodB / 10.0f), Rb = (float)(80.0 / (0.01 * 4));
    return powf(8000.0f / (EbNo * Rb), 0.5f);
}

float rade_sigma_from_EbNodB_bn1(float EbNodB)
{   /* radae.py:574-576 (bottleneck 1): sigma = (EbNo*M)^-0.5 */
    const float EbNo = powf(10.0f, EbNodB / 10.0f);
    return powf(EbNo * (float)RD_M, -0.5f);
}

float rade_sigma_from_EbNodB_rs3(float EbNodB)
{   /* radae.py:627-630 (rate Rs, bottleneck 3): sigma = M / sqrt(2 Nc EbNo) / sqrt(2), Nc = 20 carriers of the no-pilot numerology */
    const float EbNo = powf(10.0f, EbNodB / 10.0f);
    return ((float)RD_M / powf(2.0f * 20.0f * EbNo, 0.5f)) / powf(2.0f, 0.5f);
}

/* `rows` arrays of B 4-byte values (row r: src[r], or fill[r] where that is NULL, 0 without fill) to `dev` through their pinned staging copy *stage ([rows][B], allocated
 * on first use); wait = 0: the caller synchronises before it returns, since the next call refills the staging copy */
static int stage_rows(rade_batch *h, void **stage, void *dev, int rows, const void *const *src, const float *fill, int wait, hipStream_t st)
{
    if (!*stage && !(*stage = pinned_alloc_opt(h, sizeof(float) * rows * h->B))) return -1;
    float *f = *stage;
    for (int r = 0; r < rows; r++, f += h->B)
        if (src[r]) memcpy(f, src[r], sizeof(float) * h->B);
        else for (int b = 0; b < h->B; b++) f[b] = fill ? fill[r] : 0.0f;
    if (hipMemcpyAsync(dev, *stage, sizeof(float) * rows * h->B, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    return wait && hipStreamSynchronize(st) != hipSuccess ? -1 : 0;
}

/* Results on their way to the caller: `bytes` at `dev` into the engine's pinned landing area, and the stream waited for.  One area serves every call that reads
 * results back (it grows to the largest seen): each of them has waited by the time it returns, so the area is free whenever the next one starts. */
const void *read_back(rade_batch *h, const void *dev, size_t bytes, hipStream_t st)
{
    if (bytes > h->rb_cap) {
        if (h->rb_host) disown(h, h->rb_host);
        h->rb_cap = (h->rb_host = pinned_alloc_opt(h, bytes)) ? bytes : 0;
        if (!h->rb_host) return NULL;
    }
    if (hipMemcpyAsync(h->rb_host, dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return NULL;
    return h->rb_host;
}

/* the [3][B] per-stream sigma, freq_offset, df_dt of a call on the device (rd_chan_args.ps), a NULL member filled with p's scalar; *out = NULL when ps gives none */
static int chan_streams_upload(rade_batch *h, const rade_channel_params *p, const rade_channel_streams *ps, void *stream, const float **out)
{
    *out = NULL;
    if (!ps || (!ps->sigma && !ps->freq_offset && !ps->df_dt)) return 0;
    if (dev_grow(h, &h->chan_ps, NULL, 3 * h->B, sizeof(float), 1)) return -1;
    const void *src[3] = { ps->sigma, ps->freq_offset, ps->df_dt };
    const float fill[3] = { p->sigma, p->freq_offset, p->df_dt };
    if (stage_rows(h, &h->chan_ps_host, h->chan_ps, 3, src, fill, 1, (hipStream_t)stream)) return -1;
    *out = h->chan_ps;
    return 0;
}

/* one k_channel launch: the signal from tx, or from mp where the fused modulator (k_ofdm_mod_mp) left its multipath output; eoo = the end-of-over frame as transmitted */
static int channel_launch(rade_batch *h, const rade_channel_params *p, const float *ps_dev, const void *tx, long tx_stride, const void *mp, const float *eoo, void *rx, long rx_stride, void *stream)
{
    rd_chan_args a;
    memset(&a, 0, sizeof a);
    a.tab = h->d_tab; a.tx = tx; a.tx_stride = tx_stride; a.rx = rx; a.rx_stride = rx_stride; a.G = p->G_dev; a.noise = p->noise_dev; a.mp = mp;
    a.eoo = eoo; a.scratch = h->chan_scratch; a.B = h->B; a.n_sig = p->n_sig; a.n_pre = p->n_pre; a.n_post = p->n_post; a.with_eoo = p->with_eoo;
    a.sigma = p->sigma; a.freq_offset = p->freq_offset; a.df_dt = p->df_dt; a.seed = p->seed; a.ps = ps_dev;
    a.sine_amp = p->sine_amp; a.sine_freq = p->sine_freq; a.rx_gain = p->rx_gain != 0.0f ? p->rx_gain : 1.0f;
    PROF_BEGIN(h, stream);
    if (rd_launch_channel(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, 0.0);
    return p->n_pre + p->n_sig + (p->with_eoo ? RD_NEOO : 0) + p->n_post;
}

/* rade_batch_channel_streams with the per-stream values already on the device (ps_dev, or NULL) */
static int channel_dev(rade_batch *h, const void *tx_dev, long tx_stride, void *rx_out_dev, long rx_stride, const rade_channel_params *p, const float *ps_dev, void *stream)
{
    if (h->tx_linear && p->with_eoo) return -1;
    const float *eoo = h->eoo;
    if (h->tx_bpf && p->with_eoo) {        /* what radae_tx --txbpf transmits after the last frame: the end-of-over frame through the Tx band-pass filter and the clip,
                                            * the filter state carried on from the frames before it (radae_txe.py:138-144) */
        /* a pure channel call: the filter state is READ, not advanced (two passes over the same tx -- two SNR points, a two-pass bench -- see the same EOO);
         * tx_raw is the modulator's scratch and holds nothing a caller can see */
        if (rd_launch_copy_eoo(h->eoo, h->tx_raw, tx_raw_stride(h), h->B, stream) || tx_bpf_pass(h, RD_NEOO, RD_NEOO, h->eoo_filt, RD_NEOO, stream, 0)) return -1;
        eoo = h->eoo_filt;
    }
    return channel_launch(h, p, ps_dev, tx_dev, tx_stride, NULL, eoo, rx_out_dev, rx_stride, stream);
}

int rade_batch_channel_streams(rade_batch *h, const void *tx_dev, long tx_stride, void *rx_out_dev, long rx_stride,
                               const rade_channel_params *p, const rade_channel_streams *ps, void *stream)
{
    ON_DEV(h);
    const float *ps_dev;
    if (chan_streams_upload(h, p, ps, stream, &ps_dev)) return -1;
    return channel_dev(h, tx_dev, tx_stride, rx_out_dev, rx_stride, p, ps_dev, stream);
}

int rade_batch_channel(rade_batch *h, const void *tx_dev, long tx_stride, void *rx_out_dev, long rx_stride, const rade_channel_params *p, void *stream)
{
    return rade_batch_channel_streams(h, tx_dev, tx_stride, rx_out_dev, rx_stride, p, NULL, stream);
}

/* ---- transmit + channel in one pass (RADAE.forward, radae.py:529-589: latents -> OFDM -> multipath -> noise) -------------------
 * The modulator applies the two-path model while a frame's samples are in LDS and leaves the power sums, so tx is never re-read and
 * k_chan_power does not run; without G (AWGN only) it is the two calls back to back. */
int rade_batch_tx_channel_streams(rade_batch *h, const float *features_dev, int n_mf, void *iq_out_dev, long iq_stride, void *rx_out_dev, long rx_stride,
                                  const rade_channel_params *p, const rade_channel_streams *ps, void *stream)
{
    ON_DEV(h);
    if (!h || !p || n_mf <= 0 || n_mf > h->max_tx_mf || h->feat_in != RM_FEAT_AUX || p->n_sig != n_mf * RD_NMF || !rx_out_dev || (h->tx_linear && p->with_eoo)) return -1;
    if (!features_dev || misaligned16(p->G_dev)) return -1;      /* k_ofdm_mod_mp reads (G1[i], G2[i]) as one f32x4 */
    const float *ps_dev;                   /* (uploaded ahead of the transmit launches: its synchronisation waits only for what the stream held before this call) */
    if (chan_streams_upload(h, p, ps, stream, &ps_dev)) return -1;
    if (!p->G_dev || h->tx_bpf) {          /* (the Tx band-pass filter sits between the modulator and the channel: the two calls back to back) */
        if (!iq_out_dev) return -1;
        if (rade_batch_tx(h, features_dev, n_mf, iq_out_dev, iq_stride, NULL, stream) != p->n_sig) return -1;
        return channel_dev(h, iq_out_dev, iq_stride, rx_out_dev, rx_stride, p, ps_dev, stream);
    }
    if (dev_grow(h, &h->chan_mp, NULL, (long)h->B * h->max_tx_mf * RD_NMF, sizeof(float) * 2, 1)) return -1;
    const int B = h->B;
    int e = encode_features(h, features_dev, 3 * n_mf, h->enc_z, stream);
    PROF_BEGIN(h, stream);
    e |= rd_launch_ofdm_mod_mp(h->d_tab, h->enc_z, iq_out_dev, iq_stride, B, n_mf, p->G_dev, h->chan_mp, (double *)h->chan_scratch + 2 * (size_t)B, h->tx_linear, stream);
    PROF_END(h, stream, RADE_PROF_MOD, 8.0 * B * n_mf * 5 * 30 * 160);
    if (e) return -1;
    return channel_launch(h, p, ps_dev, NULL, 0, h->chan_mp, h->eoo, rx_out_dev, rx_stride, stream);
}

int rade_batch_tx_channel(rade_batch *h, const float *features_dev, int n_mf, void *iq_out_dev, long iq_stride, void *rx_out_dev, long rx_stride,
                          const rade_channel_params *p, void *stream)
{
    return rade_batch_tx_channel_streams(h, features_dev, n_mf, iq_out_dev, iq_stride, rx_out_dev, rx_stride, p, NULL, stream);
}

int rade_batch_multipath_gen(rade_batch *h, const float *fir_taps_host, int n_taps, int low_ratio, int n_out,
                             const void *noise_low_dev, unsigned long long seed, void *G_out_dev, void *stream)
{
    ON_DEV(h);
    if (!h || !fir_taps_host || n_taps <= 0 || n_taps > 1024 || !G_out_dev) return -1;
    float *taps = NULL;                                 /* (the call's two buffers live for the call only: not recorded on the engine) */
    if (hipMalloc((void **)&taps, sizeof(float) * n_taps) != hipSuccess || hipMemcpy(taps, fir_taps_host, sizeof(float) * n_taps, hipMemcpyHostToDevice) != hipSuccess) { hipFree(taps); return -1; }
    void *ybuf = NULL;                                  /* more low-rate points than the kernel keeps in LDS (lmr60: Fs / 16): they live in HBM for the call */
    if (rd_multipath_gen_needs_scratch(low_ratio, n_out)) {
        const size_t n_low = (size_t)(n_out + low_ratio - 1) / low_ratio;
        if (hipMalloc(&ybuf, sizeof(double) * 2 * 2 * n_low * h->B) != hipSuccess) { hipFree(taps); return -1; }
    }
    const int rc = rd_launch_multipath_gen(taps, n_taps, low_ratio, n_out, noise_low_dev, seed, G_out_dev, ybuf, h->B, stream);
    hipStreamSynchronize((hipStream_t)stream);          /* the call's two buffers are released right away */
    hipFree(taps);
    if (ybuf) hipFree(ybuf);
    return rc ? -1 : n_out;
}

/* multipath_samples.m:33-40: the rate-Rs channel matrix from rate-Fs Doppler samples */
int rade_batch_multipath_h(rade_batch *h, const void *G_dev, int n_g, int fs_over_rs, int n_sym, int Nc, float delay_s, float Rs, int want_complex, float *H_out_dev, void *stream)
{
    ON_DEV(h);
    if (!h || !G_dev || !H_out_dev) return -1;
    return rd_launch_multipath_h(G_dev, n_g, fs_over_rs, n_sym, Nc, delay_s * Rs, want_complex, H_out_dev, h->B, stream) ? -1 : n_sym;
}

/* ---- receive ----------------------------------------------------------------------------------- */
/* CoreDecoderStatefull.forward (radae_base.py:400-416) over T time slots of every stream, on the engine's dec2_* buffers: dec2_x = [B][1+Tcap][RD_DEC_W]
 * (slot 0 = conv history), z and out dense [B][T][.] */
static int decoder_layers(rade_batch *h, const float *z, int T, float *out, void *stream)
{
    const int B = h->B, W = RD_DEC_W, G = RM_DEC_G, H = RM_DEC_H;
    const long xsb = (long)(1 + h->Tcap) * W;
    float *x = h->dec2_x + W, *gi = h->dec2_gi, *hbuf = h->dec2_hbuf;
    int e = 0;
    dev_lin d1 = h->dec_dense1; d1.wp16 = NULL; d1.wscale16 = NULL;       /* z_hat is unbounded: f32 matrix cores (see encode_core) */
    e |= gemm(h, &d1, z, (long)T * RD_LATENT, RD_LATENT, RD_LATENT, NULL, 0, 0, 0, x, xsb, W, B, T, 1, stream);
    for (int l = 0; l < RM_NL && !e; l++) {
        const int in = RM_DEC_GRU_IN(l), cin = RM_DEC_CONV_IN(l);
        e |= gemm(h, &h->dec_gin[l], x, xsb, W, in, NULL, 0, 0, 0, gi, (long)T * G, G, B, T, 0, stream);
        rd_scan_args s = { gi, (long)T * G, G, h->dec_whh[l], h->dec_bhh[l], h->dec2_h[l], hbuf, (long)T * H, H, NULL, 0, NULL, B, T, H };
        PROF_BEGIN(h, stream); e |= rd_launch_gru_scan(&s, stream); PROF_END(h, stream, RADE_PROF_SCAN, 2.0 * B * T * G * H);
        e |= gemm(h, &h->dec_glu[l], hbuf, (long)T * H, H, H, NULL, 0, 0, 0, x + in, xsb, W, B, T, 2, stream);
        e |= gemm(h, &h->dec_conv[l], x, xsb, W, cin, x - W, xsb, W, cin, x + cin, xsb, W, B, T, 1, stream);
    }
    e |= gemm(h, &h->dec_output, x, xsb, W, W, NULL, 0, 0, 0, out, (long)T * h->feat_in, h->feat_in, B, T, 0, stream);
    return e;
}

/* pointers of the receiver's in-kernel decoder stage (rx2_decode_pending -> dq2_layers) */
static void fill_dec_args(const rade_batch *h, rd_decs_args *d)
{
    memset(d, 0, sizeof *d);
    const long DR = h->dec_rows;
    d->z = h->zrows; d->z_sb = DR * RD_LATENT; d->x = h->dec_x + RD_DEC_W; d->x_sb = (1 + DR) * RD_DEC_W;
    d->gi = h->dec_gi; d->gi_sb = DR * RM_DEC_G; d->hbuf = h->dec_hbuf; d->hb_sb = DR * RM_DEC_H;
    d->out = h->feat84; d->out_sb = DR * h->feat_in; d->out_w = h->feat_in;
    d->B = h->B;
#define LIN(dst, src) do { (dst).wp = (src).wp; (dst).bias = (src).bias; (dst).wp16 = (src).wp16; (dst).wa16 = (src).wa16; (dst).wscale = (src).wscale; (dst).N = (src).N; (dst).K = (src).K; } while (0)
    LIN(d->dense1, h->dec_dense1); LIN(d->output, h->dec_output);
    for (int l = 0; l < RM_NL; l++) { LIN(d->gin[l], h->dec_gin[l]); LIN(d->glu[l], h->dec_glu[l]); LIN(d->conv[l], h->dec_conv[l]); d->whh[l] = h->dec_whh[l]; d->bhh[l] = h->dec_bhh[l]; d->h[l] = h->dec_h[l];
                                  d->whq[l] = (h->dec_whq[l] && h->dec_whs[l]) ? h->dec_whq[l] : NULL; d->whs[l] = h->dec_whs[l]; }
#undef LIN
}

int rade_batch_decode(rade_batch *h, const float *z_dev, int n_steps, float *features_out_dev, int reset_state, void *stream)
{
    ON_DEV(h);
    if (!h || !z_dev || n_steps <= 0 || n_steps > h->Tcap || !features_out_dev) return -1;
    if (misaligned16(z_dev)) return -1;               /* the GEMMs read their A rows as f32x4 (rade_gemm.h), and dense1's rows are z_dev's */
    hipStream_t st = (hipStream_t)stream;
    if (reset_state) {
        hipMemsetAsync(h->dec2_h[0], 0, sizeof(float) * RM_NL * h->B * RM_DEC_H, st);
        hipMemsetAsync(h->dec2_x, 0, sizeof(float) * (size_t)h->B * (1 + h->Tcap) * RD_DEC_W, st);
    }
    int e = decoder_layers(h, z_dev, n_steps, features_out_dev, stream);
    e |= rd_launch_carry_rows(h->dec2_x, h->B, h->Tcap, RD_DEC_W, 1, n_steps, NULL, stream);
    return e ? -1 : n_steps;
}

/* ---- loss.py:find_loss of every stream (rade_loss.hip) ------------------------------------------------------------------------ */
int rade_batch_loss(rade_batch *h, const float *features_dev, long f_stride, int f_row, const int *n_in_host,
                    const float *hat_dev, long h_stride, int h_row, const int *n_hat_host,
                    double *loss_host, int *start_host, float *frame_loss_dev, long fl_stride, void *stream)
{
    ON_DEV(h);
    if (!h || !features_dev || !hat_dev || !n_in_host || !n_hat_host || !loss_host || !start_host || f_row < 20 || h_row < 20 || f_stride < 0 || h_stride < 0) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    int n_blk = 0, max_hat = 0, n_scored = 0;
    for (int b = 0; b < B; b++) {
        const int n = n_in_host[b], m = n_hat_host[b];
        if (m <= 0 || m > n) continue;
        const int nb = ((n > m ? n - m : 1) + RD_LOSS_WG - 1) / RD_LOSS_WG;
        if (nb > n_blk) n_blk = nb;
        if (m > max_hat) max_hat = m;
        if (frame_loss_dev && fl_stride < m) return -1;   /* a stream's curve has at most n_hat frames */
        n_scored++;
    }
    if (dev_grow(h, &h->loss_len, NULL, 2 * B, sizeof(int), 1) || dev_grow(h, &h->loss_res, NULL, B, sizeof(double) + sizeof(int), 1)) return -1;
    if (n_blk > h->loss_part_cap && dev_grow(h, &h->loss_part, &h->loss_part_cap, n_blk, (sizeof(double) + sizeof(int)) * B, 1)) return -1;
    const void *len[2] = { n_in_host, n_hat_host };        /* not waited for here: the results are read back below */
    if (stage_rows(h, &h->loss_len_host, h->loss_len, 2, len, NULL, 0, st)) return -1;
    rd_loss_args a;
    memset(&a, 0, sizeof a);
    a.feat = features_dev; a.f_stride = f_stride; a.f_row = f_row; a.hat = hat_dev; a.h_stride = h_stride; a.h_row = h_row; a.len = h->loss_len;
    a.part_v = h->loss_part; a.part_s = h->loss_part ? (int *)(h->loss_part + (size_t)B * h->loss_part_cap) : NULL; a.n_blk = n_blk;
    a.loss = h->loss_res; a.start = (int *)(h->loss_res + B);
    a.frame_loss = frame_loss_dev; a.fl_stride = fl_stride; a.max_hat = max_hat; a.B = B;
    if (rd_launch_loss(&a, stream)) return -1;
    const double *res = read_back(h, h->loss_res, (sizeof(double) + sizeof(int)) * B, st);      /* [B] doubles, then [B] ints */
    if (!res) return -1;
    const int *rs = (const int *)(res + B);
    for (int b = 0; b < B; b++) { loss_host[b] = res[b]; start_host[b] = rs[b]; }
    return n_scored;
}

int rade_batch_channel_symbol(rade_batch *h, const float *z_dev, const float *H_dev, const float *noise_dev, float *z_hat_dev, int n_steps,
                              int mode, float p0, float p1, unsigned long long seed, void *stream)
{
    ON_DEV(h);
    if (!h || n_steps <= 0 || (mode != 0 && mode != 1)) return -1;
    return rd_launch_chan_symbol(z_dev, H_dev, noise_dev, z_hat_dev, (long)h->B * n_steps * RD_LATENT, mode, p0, p1, seed, stream) ? -1 : n_steps;
}

/* The wait of rade_batch_rx when the host is short of CPUs (sync_blocking_now): SLEEP until the receiver launch is done.  hipEventSynchronize on a
 * hipEventBlockingSync event does not do that on this runtime -- measured (tools/host_threads_cpu.py, round 5): a lane thread sitting in it burns its whole
 * wall time, 3.0 cores busy for three engines against 3.8 with hipStreamSynchronize -- so the thread sleeps itself: through three quarters of what the last
 * measured waits took (a receiver launch lasts milliseconds and as long as the one before it), then in short naps between hipEventQuery calls.  A nap costs a wake-up,
 * not a core; the launch's end is noticed at most one nap (plus the timer slack) late, which the other engines' batches in flight cover. */
static double now_us(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec; }
static void nap_us(double us) { if (us > 0.0) { struct timespec t = { (time_t)(us / 1e6), (long)(1e3 * (us - 1e6 * (double)(time_t)(us / 1e6))) }; nanosleep(&t, NULL); } }
/* The estimate must not feed on its own nap: a wait that ends INSIDE the long nap says only "the launch took at most the nap", so the estimate is halved (not
 * averaged with a dt that is mostly the nap -- that form decayed 6 % per call and an outlier cost seconds of oversleeping); only a wait whose first query after the nap
 * still found the launch running measures the launch, and only those are averaged in, an outlier counted as at most 8x the present estimate.  The long nap is capped
 * (a receiver launch lasts milliseconds), and the engine's first wait -- lazy code-object load included -- does not seed the estimate. */
#define RADE_NAP_CAP_US 20000.0
static int sleep_until_event(rade_batch *h, hipEvent_t ev)
{
    const double t0 = now_us();
    int overslept = 0;
    hipError_t e = hipEventQuery(ev);
    if (e == hipErrorNotReady && h->wait_est_us > 150.0) {
        const double nap = 0.75 * h->wait_est_us;
        nap_us(nap < RADE_NAP_CAP_US ? nap : RADE_NAP_CAP_US); e = hipEventQuery(ev); overslept = e == hipSuccess;
    }
    while (e == hipErrorNotReady) { nap_us(40.0); e = hipEventQuery(ev); }
    if (e != hipSuccess) { fprintf(stderr, "rade: %s while waiting for the receiver launch\n", hipGetErrorString(e)); return -1; }
    double dt = now_us() - t0;
    if (overslept) h->wait_est_us *= 0.5;
    else if (h->n_sync_block > 0) {
        if (h->wait_est_us > 0.0 && dt > 8.0 * h->wait_est_us) dt = 8.0 * h->wait_est_us;
        h->wait_est_us = h->wait_est_us > 0.0 ? 0.75 * h->wait_est_us + 0.25 * dt : dt;
    }
    return 0;
}
/* test hook (tests/test_host_cpu.py): the estimate's update rule driven with synthetic waits -- `ready_after_us` is when the launch really ends; returns the
 * time this wait would have kept the thread beyond that (the oversleep) and updates *est like sleep_until_event does */
double rade_wait_model_step(double *est, double ready_after_us, int first)
{
    double t = 0.0; int overslept = 0;
    if (ready_after_us > 0.0 && *est > 150.0) { const double nap = 0.75 * *est; t = nap < RADE_NAP_CAP_US ? nap : RADE_NAP_CAP_US; overslept = t >= ready_after_us; }
    while (t < ready_after_us) t += 40.0;
    double dt = t;
    if (overslept) *est *= 0.5;
    else if (!first) { if (*est > 0.0 && dt > 8.0 * *est) dt = 8.0 * *est; *est = *est > 0.0 ? 0.75 * *est + 0.25 * dt : dt; }
    return t - ready_after_us;
}

int rade_batch_rx(rade_batch *h, const void *rx_dev, long rx_stride, const int *n_avail_host, int max_calls,
                  float *features_out_dev, long feat_stride, float *eoo_out_dev, rade_rx_status *status_host, void *stream)
{
    ON_DEV(h);
    const int row_floats = h && h->bypass_dec ? RD_ZMF : RD_FEAT_MF;       /* RADE_BATCH_BYPASS_DEC: 240 latents per valid modem frame instead of 432 feature floats */
    if (!h || !n_avail_host || max_calls <= 0 || h->feat_in != RM_FEAT_AUX || !features_out_dev || feat_stride < row_floats) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    int *hs = h->h_small;
    /* complex_bpf.bpf for every sample of this invocation, ahead of the receiver launches (rade_rx.hip: k_bpf_chain + k_bpf_fir).  The buffers follow the
     * largest invocation seen (a few times the input: 8 bytes per sample and stream); growing them waits for the device. */
    int max_avail = 0;
    for (int b = 0; b < B; b++) if (n_avail_host[b] > max_avail) max_avail = n_avail_host[b];
    if (max_avail > 0 && !rx_dev) return -1;
    const int n_blocks = max_avail > 0 ? 2 + (max_avail - 1) / 800 : 0;          /* blocks of >= 800 samples (a first block after a slip), the tail included */
    if (max_avail > h->filt_cap || n_blocks + 3 > h->chain_stride) {
        CHK(hipDeviceSynchronize());
        const long cap = ((long)max_avail + 1023) & ~1023L;       /* not zeroed: every entry that is read is written by the pre-pass first (dev_grow) */
        const int e = dev_grow(h, &h->rx_filt, &h->filt_cap, cap, sizeof(float) * 2 * B, 0) || dev_grow(h, &h->bpf_chain, &h->chain_stride, cap / 800 + 8, sizeof(float) * 2 * B, 0);
        if (e) { fprintf(stderr, "rade: device allocation failed (receiver pre-pass buffers)\n"); return -1; }
    }
    CHK(hipMemcpyAsync(h->rx_avail, n_avail_host, sizeof(int) * B, hipMemcpyHostToDevice, st));
    PROF_BEGIN(h, st);
    {
        rd_bpf_args ba;
        memset(&ba, 0, sizeof ba);
        ba.state = &h->rx_st->bpf; ba.state_stride = sizeof(rd_rx_stream); ba.len0 = &h->rx_st->nin; ba.len0_stride = sizeof(rd_rx_stream); ba.avail = h->rx_avail;
        ba.tab = h->d_tab; ba.bpf16 = h->bpf16; ba.x = rx_dev; ba.x_stride = rx_stride; ba.y = h->rx_filt; ba.y_stride = h->filt_cap;
        ba.chain = h->bpf_chain; ba.chain_stride = h->chain_stride; ba.n_blocks = n_blocks; ba.B = B;
        ba.zero_acc = h->rx_acc; ba.zero_progress = h->rx_progress;        /* the invocation's counters are cleared by the pre-pass's first kernel */
        if (rd_launch_bpf(&ba, st)) goto fail;
    }
    PROF_END(h, st, RADE_PROF_BPF, 8.0 * 101.0 * (double)B * max_avail);
    int counters_clear = n_blocks > 0;
    if (!counters_clear) CHK(hipMemsetAsync(h->rx_acc, 0, sizeof(int) * B * 4, st));
    rd_sync_args sa;
    memset(&sa, 0, sizeof sa);
    sa.tab = h->d_tab; sa.st = h->rx_st; sa.round = h->rx_round; sa.rx = rx_dev; sa.rx_stride = rx_stride; sa.rxf = h->rx_filt; sa.rxf_stride = h->filt_cap; sa.bpf16 = h->bpf16; sa.bpf_chain = h->bpf_chain; sa.chain_stride = h->chain_stride; sa.avail = h->rx_avail; sa.acc = h->rx_acc;
    sa.max_calls = max_calls; sa.round_calls = h->R; sa.dec_rows = h->dec_rows; sa.unsync_off_after = h->unsync_off_after;
    sa.corrq16 = h->corrq16; sa.corra16 = h->corra16; sa.zrows = h->zrows; sa.status = h->rx_status; sa.eoo_out = eoo_out_dev; sa.dtcache = h->dtcache;
    sa.trace = h->trace; sa.trace_z = h->trace_z; sa.trace_cap = h->trace_cap; sa.progress = h->rx_progress; sa.wg_cycles = h->wg_cycles; sa.B = B; sa.vm = h->vm; sa.wfwd16 = h->wfwd16; sa.variant = h->rx_census << 8; sa.lds_bytes = h->rx_lds;
    fill_dec_args(h, &sa.dec); sa.features_out = features_out_dev; sa.feat_stride = feat_stride;
    sa.bypass_dec = h->bypass_dec;
    sa.feat_cap = (int)(feat_stride / row_floats);      /* the kernel never writes past the caller's rows: a stream pauses once its buffer is full (status.consumed tells how far it got) */
    /* one launch normally takes every stream through all of its samples (calls, decoder, output); the loop only
     * continues when a stream ran into the per-launch call limit */
    for (;;) {
        if (!counters_clear) CHK(hipMemsetAsync(h->rx_progress, 0, sizeof(int) * 4, st));
        counters_clear = 0;
        PROF_BEGIN(h, st);
        if (rd_launch_rx_sync(&sa, st)) goto fail;
        PROF_END(h, st, RADE_PROF_SYNC, 0.0);
        /* progress word and (normally final) per-stream results come back in one transfer (one device block in the host copy's order) */
        CHK(hipMemcpyAsync(hs, h->rx_progress, sizeof(int) * (status_host ? 8 + 8 * (size_t)B : 4), hipMemcpyDeviceToHost, st));
        if (sync_blocking_now()) { CHK(hipEventRecord(h->ev_block, st)); if (sleep_until_event(h, h->ev_block)) goto fail; h->n_sync_block++; }
        else { CHK(hipStreamSynchronize(st)); h->n_sync_spin++; }
        if (hs[0] == 0 || hs[1] == 0) break;    /* nothing done, or no stream stopped at the per-launch limit */
    }
    if (status_host) {
        const int *acc = hs + 8, *sts = hs + 8 + 4 * B;
        for (int b = 0; b < B; b++) {
            rade_rx_status *s = status_host + b;
            s->consumed = acc[4 * b]; s->n_calls = acc[4 * b + 1]; s->n_valid = acc[4 * b + 2]; s->has_eoo = acc[4 * b + 3] > 0;
            s->nin = sts[4 * b]; s->sync = sts[4 * b + 1]; s->snr_dB = sts[4 * b + 2]; s->state = sts[4 * b + 3];
        }
    }
    return 0;
fail:
    return -1;
}

/* how many of this engine's rade_batch_rx waits slept / spun (measurement aid) */
void rade_batch_sync_counts(const rade_batch *h, long *blocking, long *spinning) { if (blocking) *blocking = h->n_sync_block; if (spinning) *spinning = h->n_sync_spin; }

/* shader-clock cycles every stream's workgroup spent in the most recent receiver launch (measurement aid: the launch lasts as
 * long as its slowest stream) */
int rade_batch_rx_stream_cycles(rade_batch *h, long long *out_host)
{
    if (!h || !out_host || !h->wg_cycles) return -1;
    ON_DEV(h);
    return hipMemcpy(out_host, h->wg_cycles, sizeof(long long) * h->B, hipMemcpyDeviceToHost) == hipSuccess ? h->B : -1;
}

/* test / measurement aid: the band-pass filtered samples (complex_bpf.bpf, dsp.py:63-102) the most recent rade_batch_rx invocation's receiver read
 * for stream b, first n of them -> out_host [n] complex64; returns the count copied */
int rade_batch_rx_filtered(rade_batch *h, int b, void *out_host, int n)
{
    if (!h || b < 0 || b >= h->B || !out_host || !h->rx_filt) return -1;
    ON_DEV(h);
    if (n > h->filt_cap) n = (int)h->filt_cap;
    if (n <= 0) return 0;
    return hipMemcpy(out_host, (const char *)h->rx_filt + sizeof(float) * 2 * (size_t)b * h->filt_cap, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? n : -1;
}

int rade_batch_rx_get_trace(rade_batch *h, int b, rade_rx_trace *out, float *z_hat_out, int max_calls)
{
    ON_DEV(h);
    if (!h || !h->trace || b < 0 || b >= h->B) return -1;
    rd_rx_stream *tmp = malloc(sizeof *tmp);
    hipMemcpy(tmp, h->rx_st + b, sizeof *tmp, hipMemcpyDeviceToHost);
    int n = tmp->mf - 1;
    free(tmp);
    if (n > h->trace_cap) n = h->trace_cap;
    if (n > max_calls) n = max_calls;
    if (n <= 0) return 0;
    if (out) hipMemcpy(out, h->trace + (size_t)b * h->trace_cap, sizeof(rd_rx_trace) * n, hipMemcpyDeviceToHost);
    if (z_hat_out) hipMemcpy(z_hat_out, h->trace_z + (size_t)b * h->trace_cap * RD_ZMF, sizeof(float) * n * RD_ZMF, hipMemcpyDeviceToHost);
    return n;
}
