/*
 * rade_stages.c -- the front-end stage calls of the batched engine (include/rade_batch.h): the rate-Rs channel, the fractional resampler, the int16 wire, the rational
 * rate converter, analog FM, the channel and the Doppler generator in pieces, the chirp header's C/No, the trials of the pilot SNR estimator, the spectrogram, the whole-file pilot acquisition, the stored-file receiver behind it and the ideal-timing receiver that shares its demodulator.  Plain C host code: each entry point checks every stream, puts the call's per-stream values on the device and
 * launches its kernel through the shim in rade_dev.h.  What these calls keep between calls is struct rd_stages, made by the first of them and opaque to rade_engine.c;
 * its device and pinned memory is on the engine's own list (rade_engine.h).
 *
 * The rules of that plumbing are stated once each, below: the record pair, the cached table and the span check here, the read-back in rade_engine.c (read_back).
 * Every refusal happens before any launch and writes nothing.
 */
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <math.h>

#include "rade_engine.h"

/* ---- the record pair: [B] per-stream values of a call on the device and their pinned staging copy, both allocated on first use -----------------------------------
 * The rule: the staging copy is not refilled until the device has read it.  A call fills pair_host() while it checks its streams and then pushes; with wait = 1 the
 * push waits for the stream, since the next call refills the staging copy (and may refill a staging table queued ahead of it); with wait = 0 the call itself waits
 * before it returns (settle, or a read-back). */
typedef struct { void *host, *dev; } rd_pair;
static int settle(hipStream_t st) { return hipStreamSynchronize(st) == hipSuccess ? 0 : -1; }
static void *pair_host(rade_batch *h, rd_pair *p, size_t bytes)
{
    if (!p->host) p->host = pinned_alloc_opt(h, bytes);
    return p->host;
}
static int pair_push(rade_batch *h, rd_pair *p, size_t bytes, int wait, hipStream_t st)
{
    if (dev_grow(h, &p->dev, NULL, 1, bytes, 1)) return -1;
    if (hipMemcpyAsync(p->dev, p->host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    return wait ? settle(st) : 0;
}

/* ---- the cached table: a table on the device that is a function of a key, made again only when a call brings another key ------------------------------------------
 * Both buffers hold the largest table the stage admits and are allocated on first use.  The protocol: a call whose key is not table_is() fills t->host and calls
 * table_upload, which clears the key BEFORE it queues the copy behind what the stream holds; table_commit sets the key only AFTER the call has waited for the stream.
 * A call that fails in between leaves the key cleared, so the next call makes the table again; and the staging table is never refilled while a copy of it is queued.
 * keep_last: t->last holds the bytes of the committed upload, for a key that includes the table's contents (the FM demodulator's taps). */
typedef struct { float *host, *dev, *last; size_t cap; int key[2], pending[2]; } rd_table;
static int table_alloc(rade_batch *h, rd_table *t, size_t cap, int keep_last)
{
    if (!t->host) {
        if (!(t->host = pinned_alloc_opt(h, sizeof(float) * cap * (keep_last ? 2 : 1)))) return -1;
        t->cap = cap;
        if (keep_last) { t->last = t->host + cap; memset(t->last, 0, sizeof(float) * cap); }
    }
    return dev_grow(h, &t->dev, NULL, (long)cap, sizeof(float), 1);
}
static int table_is(const rd_table *t, int k0, int k1) { return t->key[0] == k0 && t->key[1] == k1; }
static int table_upload(rd_table *t, int k0, int k1, size_t n, hipStream_t st)
{
    t->key[0] = t->key[1] = 0; t->pending[0] = k0; t->pending[1] = k1;
    return hipMemcpyAsync(t->dev, t->host, sizeof(float) * n, hipMemcpyHostToDevice, st) == hipSuccess ? 0 : -1;
}
static void table_commit(rd_table *t)       /* after the wait; nothing to do for a call that found its table on the device */
{
    if (!t->pending[0]) return;
    if (t->last) memcpy(t->last, t->host, sizeof(float) * t->cap);
    t->key[0] = t->pending[0]; t->key[1] = t->pending[1]; t->pending[0] = t->pending[1] = 0;
}

/* ---- the span check of a stream that reads n_in elements of a row of x_stride and writes n_out of a row of y_stride: the counts against the strides, the index n0
 * of its first output (>= n0_min) and the absolute index in_base of its first input, both within +-2^62 ----------------------------------------------------------- */
static int span_bad(long n_in, long x_stride, long n_out, long y_stride, long long n0, long long n0_min, long long in_base)
{
    if (n_in < 0 || n_out < 0 || n_in > x_stride || n_out > y_stride || n0 < n0_min) return 1;
    return n0 > (1LL << 62) || in_base > (1LL << 62) || in_base < -(1LL << 62);
}

#define RD_WIRE_SLOTS 8
struct rd_stages {
    /* rade_batch_channel_rs_pa: [B] per-stream sigma; [B][RD_RS_NCH][4] measurement partials, [B][3] measurements */
    rd_pair rs_sigma; double *rs_part, *rs_stats;
    /* rade_batch_resample: the taps [257][32] (made once); [B] per-stream records */
    float *clk_taps; rd_pair clk_ps;
    /* rade_batch_wire_in / _out: the [B] sample counts of the last RD_WIRE_SLOTS calls on the device and their pinned staging copies, one slot per call in turn (a call
     * does not wait for its stream: it waits for the call that used its slot RD_WIRE_SLOTS calls ago); [B][RD_WIRE_NCH_MAX][4] meter partials, [B][4] meters */
    int *wire_n, *wire_n_host; hipEvent_t wire_ev[RD_WIRE_SLOTS]; unsigned wire_used, wire_seq; double *wire_part, *wire_meters;
    /* rade_batch_rate_convert: the [L][T] table, key = the reduced ratio (L, M); [B] per-stream records */
    rd_table rate_taps; rd_pair rate_ps;
    /* rade_batch_fm_mod: [B] per-stream records; [B][fm_tsum_cap / B] tile sums; [B] final phases.
     * rade_batch_fm_demod: its [B] records; the two tap tables [2][RD_FM_NMAX], key = (N1, N2) and the bytes they were made from */
    rd_pair fm_ps; unsigned *fm_tsum; long fm_tsum_cap; unsigned *fm_ph_end;
    rd_pair fm_dps; rd_table fm_taps;
    /* rade_batch_multipath_piece: [B] per-stream records; the taps [RD_DOPP_NTAPS_MAX], key = n_taps and the bytes they were made from.
     * rade_batch_channel_piece: its [B] records */
    rd_pair dopp_ps; rd_table dopp_taps; rd_pair chanp_ps;
    /* rade_batch_cno_est: the table e^{-2 pi i m / N}, key = the window length N; the [B] sample counts; [B][cno_cap][RD_CNO_JMAX][2] partial and [B][cno_bands_cap][2]
     * band sums, grown with the call */
    rd_table cno_tw; rd_pair cno_n; double *cno_part, *cno_bands; long cno_cap, cno_bands_cap;
    /* rade_batch_snr_trials: [B] per-stream records; [B][snr_cap][RD_SNR_NSUM] sums, grown with the call */
    rd_pair snr_ps; double *snr_sums; long snr_cap;
    /* rade_batch_specgram: the table e^{-2 pi i m / 2048} and the window behind it (made once); per call [B] counts, [255] thresholds and [B] given peaks in one
     * record; the [B] peaks */
    float *spec_tab; rd_pair spec_rec; float *spec_peak;
    /* rade_batch_psd: the table e^{-2 pi i m / 1024} and the window behind it, key = the window length; per call [B] scales (double) and [B] counts in one record;
     * [B][psd_cap][1024] partial rows, grown with the call.  rade_batch_sigstat: the [B] counts; [B][stat_cap][4] chunk records, grown with the call; [B][4] results */
    rd_table psd_tab; rd_pair psd_rec; float *psd_part; long psd_cap;
    rd_pair stat_n; double *stat_part; long stat_cap; double *stat_out;
    /* rade_batch_acq_detect / _refine: the [B] sample counts; [B][acq_cap + 1][RD_ACQ_NPART] block sums, [B][acq_cap][RD_ACQ_NPART] best cells and [B][acq_cap] hop
     * records, grown with the call; a chunk of RD_ACQ_EV_CHUNK events, their results and their fine rows */
    rd_pair acq_n; double *acq_psum; rd_acq_pmax *acq_pmax; rd_acq_rec *acq_rec; long acq_cap, acq_cap1, acq_cap2;
    rd_pair acq_ev; rd_acq_fine *acq_fine; double *acq_dfine;
    /* rade_batch_bpf_file: the [B] sample counts; the call's mixer phases [file_phase_cap][2], grown with the call (scratch: made again by every call).
     * rade_batch_rx_file: the [B] stream records; [B][file_part_cap] pilot powers.  rade_batch_ber_align: the [B] lengths; [B][RD_FILE_NSHIFT] counts.
     * rade_batch_rx_ideal: the [2][B] frequency offsets and drifts; [B][irx_part_cap] pilot powers; [B] error counts */
    rd_pair file_n; float *file_phase; long file_phase_cap;
    rd_pair file_rx; double *file_part; long file_part_cap;
    rd_pair file_ber; long long *file_err;
    rd_pair irx_foff; double *irx_part; long irx_part_cap; long long *irx_err;
};
static struct rd_stages *stages_of(rade_batch *h)
{
    if (!h->stages) h->stages = calloc(1, sizeof *h->stages);
    return h->stages;
}
void rd_stages_free(struct rd_stages *s)
{
    for (int i = 0; i < RD_WIRE_SLOTS; i++) if (s->wire_ev[i]) hipEventDestroy(s->wire_ev[i]);
    free(s);
}

/* ---- the rate-Rs channel of the bottleneck-3 model (radae.py:603-634; rade_rs.hip) ------------------------------------------------------------ */
int rade_batch_channel_rs_pa(rade_batch *h, const float *z_dev, const float *H_dev, const void *noise_dev, float *z_hat_dev, int n_steps, float sigma,
                             const float *sigma_streams_host, float phase_offset, unsigned long long seed, double *stats_host, void *stream)
{
    ON_DEV(h);
    if (!h || !z_dev || !z_hat_dev || n_steps <= 0) return -1;
    if (((uintptr_t)z_dev | (uintptr_t)H_dev | (uintptr_t)z_hat_dev) & 3 || ((uintptr_t)noise_dev & 7)) return -1;   /* element alignment is all the kernel needs */
    struct rd_stages *s = stages_of(h);
    if (!s) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    if (dev_grow(h, &s->rs_part, NULL, (long)B * RD_RS_NCH * 4, sizeof(double), 1) || dev_grow(h, &s->rs_stats, NULL, 3L * B, sizeof(double), 1)) return -1;
    if (sigma_streams_host) {
        float *sg = pair_host(h, &s->rs_sigma, sizeof(float) * B);
        if (!sg) return -1;
        memcpy(sg, sigma_streams_host, sizeof(float) * B);
        if (pair_push(h, &s->rs_sigma, sizeof(float) * B, 1, st)) return -1;
    }
    rd_rs_args a;
    memset(&a, 0, sizeof a);
    a.tab = h->d_tab; a.z = z_dev; a.H = H_dev; a.noise = noise_dev; a.z_hat = z_hat_dev; a.B = B; a.n_steps = n_steps;
    a.sigma = sigma; a.sigma_b = sigma_streams_host ? s->rs_sigma.dev : NULL; a.seed = seed;
    a.has_phase = phase_offset != 0.0f; a.ph_re = cosf(phase_offset); a.ph_im = sinf(phase_offset);      /* radae.py:616-619 */
    a.part = s->rs_part; a.stats = stats_host ? s->rs_stats : NULL;
    PROF_BEGIN(h, stream);
    if (rd_launch_rs_pa(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, 8.0 * B * 2.0 * n_steps * 2 * 20 * RD_M);
    if (stats_host) {
        const void *res = read_back(h, s->rs_stats, sizeof(double) * 3 * B, st);
        if (!res) return -1;
        memcpy(stats_host, res, sizeof(double) * 3 * B);
    }
    return n_steps;
}

/* ---- sample-clock offset: the fractional resampler (rade_clk.hip) ------------------------------------------------------------------------------ */
int rade_batch_resample(rade_batch *h, const void *x_dev, long x_stride, const int *n_in_host, void *y_dev, long y_stride, const int *n_out_host,
                        const rade_resample_params *p, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !y_dev || !n_in_host || !n_out_host || !p) return -1;
    if (((uintptr_t)x_dev | (uintptr_t)y_dev) & 7) return -1;
    if (p->mode != RADE_RESAMPLE_SINC32 && p->mode != RADE_RESAMPLE_LINEAR) return -1;
    struct rd_stages *s = stages_of(h);
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    rd_clk_stream *ps = s ? pair_host(h, &s->clk_ps, sizeof(rd_clk_stream) * B) : NULL;
    if (!ps) return -1;
    int max_out = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched */
        rd_clk_stream *r = &ps[b];
        r->n_in = n_in_host[b]; r->n_out = n_out_host[b];
        r->n0 = p->n0_host ? p->n0_host[b] : 0; r->in_base = p->in_base_host ? p->in_base_host[b] : 0;
        if (span_bad(r->n_in, x_stride, r->n_out, y_stride, r->n0, 0, r->in_base)) return -1;
        if (rd_resample_q(p->t0_host ? p->t0_host[b] : 0.0, p->ppm_host ? p->ppm_host[b] : p->ppm, &r->step_q, &r->t0_q)) return -1;
        if (((__int128)r->n0 + r->n_out) * r->step_q > ((__int128)1 << 62)) return -1;
        if (r->n_out > max_out) max_out = r->n_out;
        work += (p->mode == RADE_RESAMPLE_SINC32 ? 4.0 * 2 * RD_CLK_TAPS : 6.0) * r->n_out;
    }
    if (!max_out) return 0;
    if (!s->clk_taps) {
        float *t = malloc(sizeof(float) * (RD_CLK_PHASES + 1) * RD_CLK_TAPS);
        if (t) { rade_resample_taps(t); s->clk_taps = dev_upload_opt(h, t, sizeof(float) * (RD_CLK_PHASES + 1) * RD_CLK_TAPS); }
        free(t);
        if (!s->clk_taps) return -1;
    }
    if (pair_push(h, &s->clk_ps, sizeof(rd_clk_stream) * B, 1, st)) return -1;       /* the one small copy ahead of the launch */
    rd_clk_args a;
    memset(&a, 0, sizeof a);
    a.x = x_dev; a.x_stride = x_stride; a.y = y_dev; a.y_stride = y_stride; a.ps = s->clk_ps.dev; a.taps = s->clk_taps; a.mode = p->mode; a.B = B; a.max_out = max_out;
    PROF_BEGIN(h, stream);
    if (rd_launch_clk_resample(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    return 0;
}

/* ---- the sound-card wire: int16 <-> complex64 (rade_wire.hip) ---------------------------------------------------------------------------------- */
/* Checks every stream, then puts the counts on the device in the call's slot and fills the launch record; 1 = nothing to do (no stream has a sample), -1 = refused */
static int wire_prepare(rade_batch *h, const void *i16, long i16_stride, const void *c64, long c64_stride, const int *n_host, int mode, float k, rd_wire_args *a, int *slot, hipStream_t st)
{
    if (!h || !i16 || !c64 || !n_host) return -1;
    if (((uintptr_t)i16 & 1) || ((uintptr_t)c64 & 7)) return -1;
    if ((mode != RADE_WIRE_REAL && mode != RADE_WIRE_IQ) || !isfinite(k)) return -1;
    const int B = h->B;
    int max_n = 0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched */
        const int n = n_host[b];
        if (n < 0 || n > c64_stride || (long)n << mode > i16_stride) return -1;
        if (n > max_n) max_n = n;
    }
    struct rd_stages *w = stages_of(h);
    if (!w) return -1;
    if (!w->wire_n_host && !(w->wire_n_host = pinned_alloc_opt(h, sizeof(int) * RD_WIRE_SLOTS * B))) return -1;
    if (dev_grow(h, &w->wire_n, NULL, (long)RD_WIRE_SLOTS * B, sizeof(int), 1)) return -1;
    const int s = (int)(w->wire_seq++ % RD_WIRE_SLOTS);
    if (!w->wire_ev[s] && hipEventCreateWithFlags(&w->wire_ev[s], hipEventDisableTiming) != hipSuccess) { w->wire_ev[s] = NULL; return -1; }
    if ((w->wire_used >> s & 1) && hipEventSynchronize(w->wire_ev[s]) != hipSuccess) return -1;     /* the slot's previous call has read its counts */
    w->wire_used &= ~(1u << s);
    memcpy(w->wire_n_host + (size_t)s * B, n_host, sizeof(int) * B);
    if (hipMemcpyAsync(w->wire_n + (size_t)s * B, w->wire_n_host + (size_t)s * B, sizeof(int) * B, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    memset(a, 0, sizeof *a);
    a->i16 = (void *)i16; a->i16_stride = i16_stride; a->c64 = (void *)c64; a->c64_stride = c64_stride; a->n = w->wire_n + (size_t)s * B;
    a->mode = mode; a->B = B; a->k = k;
    a->n_ch = 4096 / B < 4 ? 4 : 4096 / B > RD_WIRE_NCH_MAX ? RD_WIRE_NCH_MAX : 4096 / B;      /* a function of B alone: a stream's meter sums do not depend on the other streams */
    *slot = s;
    return max_n ? 0 : 1;
}
/* the slot is busy until what was queued on st up to here has run */
static int wire_done(rade_batch *h, int slot, hipStream_t st)
{
    if (hipEventRecord(h->stages->wire_ev[slot], st) != hipSuccess) return -1;
    h->stages->wire_used |= 1u << slot;
    return 0;
}

int rade_batch_wire_in(rade_batch *h, const void *in_dev, long in_stride, const int *n_host, int mode, float gain, void *out_dev, long out_stride, void *stream)
{
    ON_DEV(h);
    hipStream_t st = (hipStream_t)stream;
    rd_wire_args a; int slot;
    const int r = wire_prepare(h, in_dev, in_stride, out_dev, out_stride, n_host, mode, gain, &a, &slot, st);
    if (r < 0) return -1;
    if (r == 0) {
        PROF_BEGIN(h, stream);
        if (rd_launch_wire_in(&a, stream)) return -1;
        PROF_END(h, stream, RADE_PROF_CHAN, 0.0);
    }
    return wire_done(h, slot, st);
}

int rade_batch_wire_out(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int mode, float scale, void *out_dev, long out_stride, double *meters_host, void *stream)
{
    ON_DEV(h);
    hipStream_t st = (hipStream_t)stream;
    rd_wire_args a; int slot;
    const int r = wire_prepare(h, out_dev, out_stride, x_dev, x_stride, n_host, mode, scale, &a, &slot, st);
    if (r < 0) return -1;
    struct rd_stages *w = h->stages;
    const int B = h->B;
    if (meters_host) {
        if (dev_grow(h, &w->wire_part, NULL, (long)B * RD_WIRE_NCH_MAX * 4, sizeof(double), 1) || dev_grow(h, &w->wire_meters, NULL, 4L * B, sizeof(double), 1)) return -1;
        a.part = w->wire_part; a.meters = w->wire_meters;
    }
    if (r == 0) {
        PROF_BEGIN(h, stream);
        if (rd_launch_wire_out(&a, stream)) return -1;
        PROF_END(h, stream, RADE_PROF_CHAN, 0.0);
    }
    if (wire_done(h, slot, st)) return -1;
    if (meters_host) {                     /* straight into the caller's array, and the stream waited for */
        if (r) { memset(meters_host, 0, sizeof(double) * 4 * B); return 0; }     /* no stream has a sample: nothing was launched */
        if (hipMemcpyAsync(meters_host, w->wire_meters, sizeof(double) * 4 * B, hipMemcpyDeviceToHost, st) != hipSuccess || settle(st)) return -1;
    }
    return 0;
}

/* ---- the rational rate converter: 48 / 44.1 kHz <-> 8 kHz (rade_rate.hip) ------------------------------------------------------------------------------ */
int rade_batch_rate_convert(rade_batch *h, const void *x_dev, long x_stride, const int *n_in_host, int format, float gain, void *y_dev, long y_stride,
                            const int *n_out_host, const rade_rate_params *p, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !y_dev || !n_in_host || !n_out_host || !p) return -1;
    if (format != RADE_RATE_C64 && format != RADE_RATE_S16_REAL && format != RADE_RATE_S16_IQ) return -1;
    if (((uintptr_t)x_dev & (format == RADE_RATE_C64 ? 7 : 1)) || ((uintptr_t)y_dev & 7)) return -1;
    if (format != RADE_RATE_C64 && !isfinite(gain)) return -1;
    int L, M, T;
    if (rd_rate_reduce(p->L, p->M, &L, &M, &T)) return -1;
    struct rd_stages *s = stages_of(h);
    const int B = h->B, per = format == RADE_RATE_S16_IQ ? 2 : 1;         /* elements of x per sample */
    hipStream_t st = (hipStream_t)stream;
    rd_rate_stream *ps = s ? pair_host(h, &s->rate_ps, sizeof(rd_rate_stream) * B) : NULL;
    if (!ps) return -1;
    int max_out = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched */
        rd_rate_stream *r = &ps[b];
        r->n_in = n_in_host[b]; r->n_out = n_out_host[b];
        r->n0 = p->n0_host ? p->n0_host[b] : 0; r->in_base = p->in_base_host ? p->in_base_host[b] : 0;
        if (span_bad((long)r->n_in * per, x_stride, r->n_out, y_stride, r->n0, 0, r->in_base)) return -1;
        if (((__int128)r->n0 + r->n_out) * M > ((__int128)1 << 62)) return -1;
        if (r->n_out > max_out) max_out = r->n_out;
        work += (format == RADE_RATE_S16_REAL ? 2.0 : 4.0) * T * r->n_out;
    }
    if (!max_out) return 0;
    if (table_alloc(h, &s->rate_taps, RD_RATE_TABLE_MAX, 0)) return -1;
    if (!table_is(&s->rate_taps, L, M) && (rade_rate_taps(L, M, s->rate_taps.host) != T || table_upload(&s->rate_taps, L, M, (size_t)L * T, st))) return -1;
    if (pair_push(h, &s->rate_ps, sizeof(rd_rate_stream) * B, 1, st)) return -1;     /* the one small copy ahead of the launch */
    table_commit(&s->rate_taps);
    rd_rate_args a;
    memset(&a, 0, sizeof a);
    a.x = x_dev; a.x_stride = x_stride; a.y = y_dev; a.y_stride = y_stride; a.ps = s->rate_ps.dev; a.taps = s->rate_taps.dev;
    a.L = L; a.M = M; a.T = T; a.tile = rd_rate_tile(L, M, T); a.fmt = format; a.B = B; a.max_out = max_out; a.gain = gain;
    PROF_BEGIN(h, stream);
    if (rd_launch_rate_convert(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    return 0;
}

/* ---- the analog FM modulator and demodulator (rade_fm.hip) -------------------------------------------------------------------------------------------------- */
static int fm_rates_ok(double Fs, double fc, double fd)
{
    return isfinite(Fs) && isfinite(fc) && isfinite(fd) && Fs > 0.0 && fabs(fc) <= Fs / 2.0 && fd > 0.0 && fd <= Fs / 2.0;
}

int rade_batch_fm_mod(rade_batch *h, const void *m_dev, long m_stride, const int *n_host, void *y_dev, long y_stride, const rade_fm_mod_params *p, void *stream)
{
    ON_DEV(h);
    if (!h || !m_dev || !y_dev || !n_host || !p) return -1;
    if (p->in_format != RADE_FM_F32 && p->in_format != RADE_FM_C64) return -1;
    if (p->out_mode != RADE_FM_OUT_COMPLEX && p->out_mode != RADE_FM_OUT_REAL) return -1;
    if (((uintptr_t)m_dev & (p->in_format == RADE_FM_C64 ? 7 : 3)) || ((uintptr_t)y_dev & 7) || ((uintptr_t)p->noise_dev & 7)) return -1;
    if (!fm_rates_ok(p->Fs, p->fc, p->fd) || !isfinite(p->sigma) || p->sigma < 0.0) return -1;
    const int noise_on = p->sigma > 0.0;
    if (noise_on && !p->noise_dev && !p->seed) return -1;             /* a noise level without a source of noise */
    struct rd_stages *s = stages_of(h);
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    rd_fm_stream *ps = s ? pair_host(h, &s->fm_ps, sizeof(rd_fm_stream) * B) : NULL;
    if (!ps) return -1;
    int max_n = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched */
        rd_fm_stream *r = &ps[b];
        r->n = n_host[b]; r->n0 = p->n0_host ? p->n0_host[b] : 0; r->ph0 = p->phase0_host ? p->phase0_host[b] : 0u;
        if (r->n < 0 || r->n > m_stride || r->n > y_stride || r->n0 < 0 || r->n0 > (1LL << 62)) return -1;
        if (r->n > max_n) max_n = r->n;
        work += 8.0 * r->n;
    }
    if (!max_n) {                                                     /* nothing to modulate: the phase stays where it was */
        if (p->phase_end_host) for (int b = 0; b < B; b++) p->phase_end_host[b] = ps[b].ph0;
        return 0;
    }
    const int n_tiles = (max_n + RD_FM_TILE - 1) / RD_FM_TILE;
    if (dev_grow(h, &s->fm_ph_end, NULL, B, sizeof(unsigned), 1) || dev_grow(h, &s->fm_tsum, &s->fm_tsum_cap, (long)B * n_tiles, sizeof(unsigned), 1)) return -1;
    if (pair_push(h, &s->fm_ps, sizeof(rd_fm_stream) * B, 1, st)) return -1;         /* the one small copy ahead of the launches */
    rd_fm_mod_args a;
    memset(&a, 0, sizeof a);
    a.m = m_dev; a.m_stride = m_stride; a.y = y_dev; a.y_stride = y_stride; a.noise = noise_on ? p->noise_dev : NULL; a.noise_stride = max_n;
    a.ps = s->fm_ps.dev; a.tsum = s->fm_tsum; a.ph_end = s->fm_ph_end;
    a.kc = p->fc / p->Fs * 4294967296.0; a.kd = p->fd / p->Fs * 4294967296.0; a.seed = p->seed;
    a.sg = (float)(a.noise || p->out_mode == RADE_FM_OUT_REAL ? p->sigma : p->sigma / sqrt(2.0));
    a.fmt = p->in_format; a.real_out = p->out_mode == RADE_FM_OUT_REAL; a.noise_on = noise_on; a.B = B; a.n_tiles = n_tiles;
    PROF_BEGIN(h, stream);
    if (rd_launch_fm_mod(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    if (p->phase_end_host) {                                          /* the call then waits for `stream` once more */
        const void *end = read_back(h, s->fm_ph_end, sizeof(unsigned) * B, st);
        if (!end) return -1;
        memcpy(p->phase_end_host, end, sizeof(unsigned) * B);
    }
    return 0;
}

int rade_batch_fm_demod(rade_batch *h, const void *x_dev, long x_stride, const int *n_in_host, void *y_dev, long y_stride, const int *n_out_host,
                        const rade_fm_demod_params *p, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !y_dev || !n_in_host || !n_out_host || !p || !p->b1 || !p->b2) return -1;
    if (p->out_format != RADE_FM_F32 && p->out_format != RADE_FM_C64) return -1;
    if (((uintptr_t)x_dev & 7) || ((uintptr_t)y_dev & (p->out_format == RADE_FM_C64 ? 7 : 3)) || ((uintptr_t)p->bb_out_dev & 7)) return -1;
    if (!fm_rates_ok(p->Fs, p->fc, p->fd)) return -1;
    if (p->N1 < 1 || p->N1 > RD_FM_NMAX || p->N2 < 1 || p->N2 > RD_FM_NMAX) return -1;
    for (int k = 0; k < p->N1; k++) if (!isfinite(p->b1[k])) return -1;
    for (int k = 0; k < p->N2; k++) if (!isfinite(p->b2[k])) return -1;
    struct rd_stages *s = stages_of(h);
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    rd_fm_dstream *ps = s ? pair_host(h, &s->fm_dps, sizeof(rd_fm_dstream) * B) : NULL;
    if (!ps) return -1;
    int max_out = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched */
        rd_fm_dstream *r = &ps[b];
        r->n_in = n_in_host[b]; r->n_out = n_out_host[b];
        r->in_base = p->in_base_host ? p->in_base_host[b] : 0; r->n0 = p->n0_host ? p->n0_host[b] : r->in_base;
        if (span_bad(r->n_in, x_stride, r->n_out, y_stride, r->n0, -(1LL << 62), r->in_base) || (p->bb_out_dev && r->n_out > p->bb_stride)) return -1;
        if (r->n_out > max_out) max_out = r->n_out;
        work += (4.0 * p->N1 + 2.0 * p->N2) * r->n_out;
    }
    if (!max_out) return 0;
    rd_table *t = &s->fm_taps;             /* [2][RD_FM_NMAX]: b1, b2, zeros behind each */
    if (table_alloc(h, t, 2 * RD_FM_NMAX, 1)) return -1;
    if (!table_is(t, p->N1, p->N2) || memcmp(t->last, p->b1, sizeof(float) * p->N1) || memcmp(t->last + RD_FM_NMAX, p->b2, sizeof(float) * p->N2)) {
        memset(t->host, 0, sizeof(float) * 2 * RD_FM_NMAX);
        memcpy(t->host, p->b1, sizeof(float) * p->N1); memcpy(t->host + RD_FM_NMAX, p->b2, sizeof(float) * p->N2);
        if (table_upload(t, p->N1, p->N2, 2 * RD_FM_NMAX, st)) return -1;
    }
    if (pair_push(h, &s->fm_dps, sizeof(rd_fm_dstream) * B, 1, st)) return -1;       /* the one small copy ahead of the launch */
    table_commit(t);
    const double wd = 2.0 * M_PI * p->fd / p->Fs;
    rd_fm_demod_args a;
    memset(&a, 0, sizeof a);
    a.x = x_dev; a.x_stride = x_stride; a.y = y_dev; a.y_stride = y_stride; a.bb_out = p->bb_out_dev; a.bb_stride = p->bb_stride;
    a.ps = s->fm_dps.dev; a.taps = t->dev;
    a.fcq = (unsigned)(long long)llrint(p->fc / p->Fs * 4294967296.0);
    a.wd = (float)wd; a.inv_wd = (float)(1.0 / wd);
    a.N1 = p->N1; a.N2 = p->N2; a.fmt = p->out_format; a.dont_limit = p->ph_dont_limit != 0; a.B = B; a.max_out = max_out;
    PROF_BEGIN(h, stream);
    if (rd_launch_fm_demod(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    return 0;
}

/* ---- the channel and the Doppler generator in pieces (rade_chanp.hip) ---------------------------------------------------------------------------------------- */
double rade_multipath_gain(const float *taps, int n_taps)
{
    if (!taps || n_taps < 1 || n_taps > RD_DOPP_NTAPS_MAX) return -1.0;
    double R0 = 0.0, R1 = 0.0;             /* of one path's low-rate sequence: E |y[i]|^2 and E y[i] conj(y[i + 1]), the draws having unit variance per component */
    for (int k = 0; k < n_taps; k++) {
        if (!isfinite(taps[k])) return -1.0;
        R0 += 2.0 * (double)taps[k] * (double)taps[k];
        if (k + 1 < n_taps) R1 += 2.0 * (double)taps[k] * (double)taps[k + 1];
    }
    const double var = 2.0 * ((2.0 / 3.0) * R0 + (1.0 / 3.0) * R1);      /* two paths, the interpolation weights averaged over a low-rate step */
    return var > 0.0 ? 1.0 / sqrt(var) : -1.0;
}

int rade_batch_multipath_piece(rade_batch *h, const float *fir_taps_host, int n_taps, int low_ratio, double hf_gain, unsigned long long seed,
                               const long long *n0_host, const int *n_out_host, void *G_out_dev, long g_stride, void *stream)
{
    ON_DEV(h);
    if (!h || !fir_taps_host || !n_out_host || !G_out_dev || ((uintptr_t)G_out_dev & 7)) return -1;
    if (n_taps < 1 || n_taps > RD_DOPP_NTAPS_MAX || low_ratio < 1 || !isfinite(hf_gain) || hf_gain < 0.0) return -1;
    if (hf_gain == 0.0 && (hf_gain = rade_multipath_gain(fir_taps_host, n_taps)) <= 0.0) return -1;      /* (also: taps that are not finite) */
    for (int k = 0; k < n_taps; k++) if (!isfinite(fir_taps_host[k])) return -1;
    struct rd_stages *s = stages_of(h);
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    rd_dopp_stream *ps = s ? pair_host(h, &s->dopp_ps, sizeof(rd_dopp_stream) * B) : NULL;
    if (!ps) return -1;
    int max_out = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched */
        rd_dopp_stream *r = &ps[b];
        r->n0 = n0_host ? n0_host[b] : 0; r->n_out = n_out_host[b]; r->pad = 0;
        if (r->n_out < 0 || r->n_out > g_stride || r->n0 < 0 || r->n0 > (1LL << 62) || r->n0 + r->n_out > (1LL << 62)) return -1;
        if (r->n_out > max_out) max_out = r->n_out;
        work += (4.0 * n_taps / low_ratio + 16.0) * r->n_out;
    }
    if (!max_out) return 0;
    rd_table *t = &s->dopp_taps;
    if (table_alloc(h, t, RD_DOPP_NTAPS_MAX, 1)) return -1;
    if (!table_is(t, n_taps, 1) || memcmp(t->last, fir_taps_host, sizeof(float) * n_taps)) {
        memset(t->host, 0, sizeof(float) * RD_DOPP_NTAPS_MAX);
        memcpy(t->host, fir_taps_host, sizeof(float) * n_taps);
        if (table_upload(t, n_taps, 1, RD_DOPP_NTAPS_MAX, st)) return -1;
    }
    if (pair_push(h, &s->dopp_ps, sizeof(rd_dopp_stream) * B, 1, st)) return -1;     /* the one small copy ahead of the launch */
    table_commit(t);
    rd_dopp_args a;
    memset(&a, 0, sizeof a);
    a.taps = t->dev; a.n_taps = n_taps; a.low_ratio = low_ratio; a.hf_gain = hf_gain; a.seed = seed;
    a.G = G_out_dev; a.g_stride = g_stride; a.ps = s->dopp_ps.dev; a.B = B; a.max_out = max_out;
    PROF_BEGIN(h, stream);
    if (rd_launch_dopp_piece(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    return 0;
}

/* The frequency offset in turns per sample, the rate rade_batch_channel turns at (chan_phase_acc, rade_devutil.h): without a drift that is the reference's FLOAT32
 * omega = ((f0 * 2) * pi) / 8000 (radae.py: the tensor it sums is float32), 5e-8 relative from f0 / 8000 at 10 Hz -- which is 8e-7 rad after 1,920 samples, more than
 * the float32 phase's own rounding there; with a drift it is the closed form's double f0 / 8000.  A piece and the whole call then differ by roundings that do not grow
 * with the sample index on the piece's side. */
static double piece_turns(float f0, float df_dt)
{
    if (df_dt != 0.0f) return (double)f0 / 8000.0;
    const float om = ((f0 * 2.0f) * (float)M_PI) / 8000.0f;
    return (double)om / (2.0 * M_PI);
}

/* a scalar of the structure or stream b's entry of its [B] array */
#define PIECE_VAL(p, name, b) ((p)->name##_host ? (p)->name##_host[b] : (p)->name)
int rade_batch_channel_piece(rade_batch *h, const void *tx_dev, long tx_stride, const int *n_in_host, void *rx_out_dev, long rx_stride, const int *n_out_host,
                             const rade_channel_piece_params *p, void *stream)
{
    ON_DEV(h);
    if (!h || !tx_dev || !rx_out_dev || !n_in_host || !n_out_host || !p || (p->G_dev && !p->n_g_host)) return -1;
    if (((uintptr_t)tx_dev | (uintptr_t)rx_out_dev | (uintptr_t)p->G_dev | (uintptr_t)p->noise_dev) & 7) return -1;
    if (p->noise_mode != RADE_CHANP_NOISE_COMPLEX && p->noise_mode != RADE_CHANP_NOISE_REAL) return -1;
    if (!isfinite(p->sine_amp) || !isfinite(p->sine_freq) || !isfinite(p->rx_gain)) return -1;
    struct rd_stages *s = stages_of(h);
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    rd_chanp_stream *ps = s ? pair_host(h, &s->chanp_ps, sizeof(rd_chanp_stream) * B) : NULL;
    if (!ps) return -1;
    int max_out = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched */
        rd_chanp_stream *r = &ps[b];
        const float sigma = PIECE_VAL(p, sigma, b), f0 = PIECE_VAL(p, freq_offset, b), dd = PIECE_VAL(p, df_dt, b), gain = PIECE_VAL(p, gain, b);
        if (!isfinite(sigma) || sigma < 0.0f || !isfinite(f0) || fabsf(f0) > 2000.0f || !isfinite(dd) || fabsf(dd) > 2000.0f * 8000.0f || !isfinite(gain)) return -1;
        r->n0 = PIECE_VAL(p, n0, b); r->in_base = PIECE_VAL(p, in_base, b); r->g_base = p->G_dev ? PIECE_VAL(p, g_base, b) : 0;
        r->n_in = n_in_host[b]; r->n_out = n_out_host[b]; r->n_g = p->G_dev ? p->n_g_host[b] : 0;
        if (span_bad(r->n_in, tx_stride, r->n_out, rx_stride, r->n0, 0, r->in_base) || r->in_base < 0 || r->n0 + r->n_out > (1LL << 62)) return -1;
        if (p->G_dev) {
            if (r->n_g < 0 || r->n_g > p->g_stride || r->g_base < 0 || r->g_base > (1LL << 62)) return -1;
            if (r->n_out > 0 && (r->g_base > (r->n0 > 16 ? r->n0 - 16 : 0) || r->g_base + r->n_g < r->n0 + r->n_out)) return -1;      /* [max(0, n0 - 16), n0 + n_out) */
        }
        r->sigma = sigma; r->gain = gain == 0.0f ? 1.0f : gain;
        r->rotate = f0 != 0.0f || dd != 0.0f;
        r->f0q = (unsigned long long)llrint(piece_turns(f0, dd) * 18446744073709551616.0);
        r->dq = (unsigned long long)llrint((double)dd / 64000000.0 * 18446744073709551616.0);
        if (r->n_out > max_out) max_out = r->n_out;
        work += (p->G_dev ? 30.0 : 14.0) * r->n_out;
    }
    if (!max_out) return 0;
    if (pair_push(h, &s->chanp_ps, sizeof(rd_chanp_stream) * B, 1, st)) return -1;   /* the one small copy ahead of the launch */
    rd_chanp_args a;
    memset(&a, 0, sizeof a);
    a.tx = tx_dev; a.tx_stride = tx_stride; a.G = p->G_dev; a.g_stride = p->g_stride; a.noise = p->noise_dev; a.noise_stride = max_out;
    a.rx = rx_out_dev; a.rx_stride = rx_stride; a.ps = s->chanp_ps.dev; a.seed = p->seed;
    a.sine_amp = p->sine_amp; a.sine_freq = p->sine_freq; a.rx_gain = p->rx_gain == 0.0f ? 1.0f : p->rx_gain;
    a.noise_mode = p->noise_mode; a.B = B; a.max_out = max_out;
    PROF_BEGIN(h, stream);
    if (rd_launch_chan_piece(&a, stream)) return -1;
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    return 0;
}

/* ---- C/No of the chirp header: est_CNo.py over every stream (rade_cno.hip; the arithmetic behind the band sums: rade_host.c) ------------------------------ */
int rade_batch_cno_est(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, const rade_cno_params *p, double *bands_host, int max_windows,
                       rade_cno_result *result_host, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !n_host || !p || !result_host || ((uintptr_t)x_dev & 7)) return -1;
    rade_cno_plan_t q;
    if (rade_cno_plan(p, &q)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    int max_win = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        const int n = n_host[b];
        if (n < 0 || n > x_stride || n < q.N) return -1;
        const int nw = n > q.N ? (n - q.N + RD_CNO_H - 1) / RD_CNO_H : 0;
        if (nw > max_win) max_win = nw;
        if (nw) work += 8.0 * (40.0 + 50.0 * 0.225 + 0.225 * q.J) * RD_CNO_H * (nw + q.J - 1) * q.J;
    }
    if (bands_host && max_windows < max_win) return -1;
    const double *bands_all = NULL;        /* [B][max_win][2], read back */
    if (max_win) {
        struct rd_stages *s = stages_of(h);
        int *n_stage = s ? pair_host(h, &s->cno_n, sizeof(int) * B) : NULL;
        if (!n_stage || table_alloc(h, &s->cno_tw, 2L * RD_CNO_H * RD_CNO_JMAX, 0)) return -1;
        if (dev_grow(h, &s->cno_part, &s->cno_cap, max_win, sizeof(double) * 2 * RD_CNO_JMAX * B, 1)) return -1;
        if (dev_grow(h, &s->cno_bands, &s->cno_bands_cap, max_win, sizeof(double) * 2 * B, 1)) return -1;
        if (!table_is(&s->cno_tw, q.N, 0)) {
            rd_cno_table(q.N, s->cno_tw.host);
            if (table_upload(&s->cno_tw, q.N, 0, 2 * (size_t)q.N, st)) return -1;
        }
        memcpy(n_stage, n_host, sizeof(int) * B);
        if (pair_push(h, &s->cno_n, sizeof(int) * B, 0, st)) return -1;              /* not waited for here: the call waits at its end */
        rd_cno_args a;
        memset(&a, 0, sizeof a);
        a.x = x_dev; a.x_stride = x_stride; a.n = s->cno_n.dev; a.tw = s->cno_tw.dev; a.part = s->cno_part; a.bands = s->cno_bands;
        a.N = q.N; a.J = q.J; a.B = B; a.max_win = max_win;
        a.flow_bin = q.flow_bin; a.fhigh_bin = q.fhigh_bin; a.noise_st = q.noise_st; a.noise_en = q.noise_en;
        a.pitch = rd_cno_pitch(q.J, q.flow_bin, q.fhigh_bin, q.noise_st, q.noise_en);
        PROF_BEGIN(h, stream);
        const int e = rd_launch_cno(&a, stream);
        PROF_END(h, stream, RADE_PROF_CHAN, work);
        /* the band sums come back and the stream is waited for (also where the launch failed: the staging copies above are then free again) */
        if (e || !(bands_all = read_back(h, s->cno_bands, sizeof(double) * 2 * B * max_win, st))) { settle(st); return -1; }
        table_commit(&s->cno_tw);
    } else if (settle(st)) return -1;
    for (int b = 0; b < B; b++) {
        const int nw = n_host[b] > q.N ? (n_host[b] - q.N + RD_CNO_H - 1) / RD_CNO_H : 0;
        const double *bands = nw ? bands_all + (size_t)b * max_win * 2 : NULL;
        rd_cno_finish(&q, p, bands, nw, &result_host[b]);
        if (bands_host && nw) memcpy(bands_host + (size_t)b * max_windows * 2, bands, sizeof(double) * 2 * nw);
    }
    return 0;
}

/* ---- trials of the pilot SNR estimator: est_snr.py over every stream (rade_snr.hip); the script's formulas behind the sums, host only ------------------------- */
int rade_batch_snr_trials(rade_batch *h, const int *n_windows_host, const rade_snr_params *p, rade_snr_sums *out_host, int max_windows, void *stream)
{
    ON_DEV(h);
    if (!h || !n_windows_host || !p || !p->sigma_host || !out_host) return -1;
    if (p->Nw < 1 || p->Nw > RD_SNR_NW_MAX || p->h_step < 1 || p->h_step > RD_SNR_HSTEP_MAX) return -1;
    if ((p->noise_dev != NULL) == (p->seed != 0) || (p->noise_out_dev && !p->seed)) return -1;          /* exactly one source of noise */
    if (((uintptr_t)p->H_dev | (uintptr_t)p->noise_dev | (uintptr_t)p->noise_out_dev) & 7) return -1;
    struct rd_stages *s = stages_of(h);
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    rd_snr_stream *ps = s ? pair_host(h, &s->snr_ps, sizeof(rd_snr_stream) * B) : NULL;
    if (!ps) return -1;
    int max_win = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        rd_snr_stream *r = &ps[b];
        r->n_win = n_windows_host[b]; r->sigma = p->sigma_host[b]; r->row0 = p->row0_host ? p->row0_host[b] : 0;
        if (r->n_win < 0 || r->n_win > max_windows || !isfinite(r->sigma) || r->sigma < 0.0f || r->row0 < 0 || r->row0 > (1LL << 40)) return -1;
        const long long rows = (long long)r->n_win * p->Nw;
        if (rows) {
            if (p->H_dev && ((rows - 1) * p->h_step + 1) * RD_NC > p->h_stride) return -1;
            if ((p->noise_dev || p->noise_out_dev) && rows * RD_NC > p->noise_stride) return -1;
        }
        if (r->n_win > max_win) max_win = r->n_win;
        work += (p->noise_dev ? 60.0 : 160.0) * RD_NC * (double)rows;
    }
    if (!max_win) return settle(st) ? -1 : 0;
    if (dev_grow(h, &s->snr_sums, &s->snr_cap, max_win, sizeof(double) * RD_SNR_NSUM * B, 1)) return -1;
    if (pair_push(h, &s->snr_ps, sizeof(rd_snr_stream) * B, 0, st)) return -1;           /* not waited for here: the call waits at its end */
    rd_snr_args a;
    memset(&a, 0, sizeof a);
    a.tab = h->d_tab; a.H = p->H_dev; a.h_stride = p->h_stride; a.h_step = p->h_step;
    a.noise = p->noise_dev; a.noise_out = p->noise_out_dev; a.noise_stride = p->noise_stride;
    a.ps = s->snr_ps.dev; a.seed = p->seed; a.sums = s->snr_sums; a.Nw = p->Nw; a.B = B; a.max_win = max_win;
    PROF_BEGIN(h, stream);
    const int e = rd_launch_snr_trials(&a, stream);
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    /* the sums come back and the stream is waited for (also where the launch failed: the staging copy above is then free again) */
    const double *all = NULL;              /* [B][max_win][RD_SNR_NSUM], read back */
    if (e || !(all = read_back(h, s->snr_sums, sizeof(double) * RD_SNR_NSUM * B * max_win, st))) { settle(st); return -1; }
    for (int b = 0; b < B; b++)
        if (ps[b].n_win) memcpy(out_host + (size_t)b * max_windows, all + (size_t)b * max_win * RD_SNR_NSUM, sizeof(rade_snr_sums) * ps[b].n_win);
    return 0;
}

/* sum (pg P[c])^2 / Nc with the float32 products k_snr_trials forms (rd_tables_fill: P = +-(float)sqrt 2, pilot_gain): every carrier has the same square */
static double snr_Es(void)
{
    const float pgp = (float)(pow(10.0, -2.0 / 20.0) * 160.0 / sqrt(30.0)) * (float)sqrt(2.0);
    return (double)pgp * (double)pgp;
}

double rade_snr_sigma(double snrdB)
{
    return sqrt(snr_Es() / pow(10.0, snrdB / 10.0)) / sqrt(2.0);
}

/* est_snr.py:107-109 / dsp.py:444-447: S1 / (2 S2) - 1, 0.1 where that is <= 0 (a NaN passes, as in the script) */
static double snr_est_of(double S1, double S2)
{
    const double v = S1 / (2.0 * S2) - 1.0;
    return v <= 0.0 ? 0.1 : v;
}

int rade_snr_finish(const rade_snr_sums *s, int eq_ls, double c, double m, rade_snr_point *out)
{
    if (!s || !out || !isfinite(c) || !isfinite(m) || m == 0.0) return -1;
    out->snrdB_genie = 10.0 * log10(s->S1_sig / s->S1_noise);
    out->snrdB_est = (10.0 * log10(snr_est_of(s->S1, eq_ls ? s->S2_est : s->S2_genie)) - c) / m;
    out->NdB_genie = 10.0 * log10(2.0 * s->S2_genie);
    out->NdB_est = 10.0 * log10(2.0 * s->S2_est);
    return 0;
}

int rade_snr_fit(const double *x, const double *y, int n, double *m, double *c)
{
    if (!x || !y || !m || !c || n < 2) return -1;
    double mx = 0.0, my = 0.0, sxx = 0.0, sxy = 0.0;
    for (int i = 0; i < n; i++) { mx += x[i]; my += y[i]; }
    mx /= n; my /= n;
    for (int i = 0; i < n; i++) { sxx += (x[i] - mx) * (x[i] - mx); sxy += (x[i] - mx) * (y[i] - my); }
    if (!(sxx > 0.0) || !isfinite(sxx) || !isfinite(sxy)) return -1;
    *m = sxy / sxx; *c = my - *m * mx;
    return 0;
}

int rade_snr_track(const rade_snr_sums *sums, int n, double c, double m, double *state, double *out)
{
    if (!sums || !state || n < 0 || !isfinite(c) || !isfinite(m) || m == 0.0) return -1;
    const double bw_3k = 10.0 * log10((8000.0 / RD_M) * RD_NC / 3000.0), cp = 10.0 * log10((double)(RD_M + RD_NCP) / RD_M);
    for (int i = 0; i < n; i++) {
        const double snrdB_est = (10.0 * log10(snr_est_of(sums[i].S1, sums[i].S2_est + 1e-12)) - c) / m;
        *state = 0.9 * *state + 0.1 * (snrdB_est + bw_3k + cp);
        if (out) out[i] = *state;
    }
    return 0;
}

/* ---- the spectrogram: plot_specgram.m over every stream (rade_spec.hip; the band, the window and the thresholds: rade_host.c) ------------------------------ */
int rade_batch_specgram(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int format, float gain, const rade_specgram_params *p,
                        unsigned char *img_dev, long img_stride, float *mag_dev, long mag_stride, float *peak_host, int *n_slices_host, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !n_host || !p || !peak_host || !n_slices_host) return -1;
    if (format != RADE_SPEC_C64 && format != RADE_SPEC_S16_REAL) return -1;
    if (((uintptr_t)x_dev & (format == RADE_SPEC_C64 ? 7 : 1)) || ((uintptr_t)mag_dev & 3) || !isfinite(gain)) return -1;
    if (p->peak_in_host && !img_dev && !mag_dev) return -1;               /* nothing is left to compute */
    rade_specgram_plan_t q;
    if (rade_specgram_plan(p, &q)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    long long max_sl = 0, pairs = 0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        const int n = n_host[b];
        if (n < 0 || n > x_stride || n <= RD_SPEC_WIN) return -1;
        const long long ns = rade_specgram_slices(n);
        if ((img_dev && ns * q.n_bins > img_stride) || (mag_dev && ns * (RD_SPEC_NFFT / 2 - 1) > mag_stride)) return -1;
        if (p->peak_in_host && !(p->peak_in_host[b] >= 0.0f && isfinite(p->peak_in_host[b]))) return -1;
        if (ns > max_sl) max_sl = ns;
        pairs += (ns + 1) / 2;
    }
    struct rd_stages *s = stages_of(h);
    if (!s) return -1;
    const size_t tab_floats = 2 * RD_SPEC_NFFT + RD_SPEC_WIN, rec_bytes = sizeof(int) * B + sizeof(float) * (256 + B);
    if (!s->spec_tab) {
        float *t = malloc(sizeof(float) * tab_floats);
        if (t) { rd_cno_table(RD_SPEC_NFFT, t); rade_specgram_window(t + 2 * RD_SPEC_NFFT); s->spec_tab = dev_upload_opt(h, t, sizeof(float) * tab_floats); }
        free(t);
        if (!s->spec_tab) return -1;
    }
    int *rec = pair_host(h, &s->spec_rec, rec_bytes);                    /* [B] counts, [256] thresholds (255 used), [B] given peaks */
    if (!rec || dev_grow(h, &s->spec_peak, NULL, B, sizeof(float), 1)) return -1;
    float *lev = (float *)(rec + B), *pin = lev + 256;
    memcpy(rec, n_host, sizeof(int) * B);
    lev[255] = 0.0f;
    if (rade_specgram_levels(p->lo, p->hi, lev)) return -1;
    for (int b = 0; b < B; b++) pin[b] = p->peak_in_host ? p->peak_in_host[b] : 0.0f;
    if (pair_push(h, &s->spec_rec, rec_bytes, 0, st)) return -1;         /* not waited for here: the call waits at its end */
    rd_spec_args a;
    memset(&a, 0, sizeof a);
    a.x = x_dev; a.x_stride = x_stride; a.n = s->spec_rec.dev; a.tw = s->spec_tab; a.win = s->spec_tab + 2 * RD_SPEC_NFFT; a.lev = (const float *)((const int *)s->spec_rec.dev + B);
    a.gain = gain; a.fmt = format; a.k0 = q.k0; a.k1 = q.k1; a.B = B; a.max_slices = (int)max_sl;
    a.img_stride = img_stride; a.mag_stride = mag_stride;
    const double work = 10.0 * RD_SPEC_NFFT * 11;                        /* of a pair's transform: 5 N log2 N, the textbook count */
    int e = 0, passes = 0;
    PROF_BEGIN(h, stream);
    if (p->peak_in_host) {                                                /* one pass against the given peaks */
        a.peak = (float *)a.lev + 256; a.img = img_dev; a.mag = mag_dev;
        e = rd_launch_specgram(&a, stream); passes = 1;
    } else {
        a.peak = s->spec_peak; a.mag = mag_dev; a.do_max = 1;             /* pass 1: magnitudes and the maximum */
        e = hipMemsetAsync(s->spec_peak, 0, sizeof(float) * B, st) != hipSuccess || rd_launch_specgram(&a, stream); passes = 1;
        if (!e && img_dev) { a.mag = NULL; a.do_max = 0; a.img = img_dev; e = rd_launch_specgram(&a, stream); passes = 2; }     /* pass 2: the levels */
    }
    PROF_END(h, stream, RADE_PROF_CHAN, work * pairs * passes);
    /* the peaks come back and the stream is waited for (also where a launch failed: the staging copy above is then free again) */
    const float *pk = NULL;
    if (e || (!p->peak_in_host && !(pk = read_back(h, s->spec_peak, sizeof(float) * B, st))) || (p->peak_in_host && settle(st))) { settle(st); return -1; }
    for (int b = 0; b < B; b++) {
        peak_host[b] = p->peak_in_host ? p->peak_in_host[b] : pk[b];
        n_slices_host[b] = (int)rade_specgram_slices(n_host[b]);
    }
    return 0;
}

/* ---- the Welch periodogram and the power / peak sums: radae_plots.m's do_plots over every stream (rade_psd.hip; the geometry, the window and the bandwidth:
 * rade_host.c) ------------------------------------------------------------------------------------------------------------------------------------------------ */
static int psd_input_bad(const void *x_dev, int format, float gain)
{
    if (format != RADE_SPEC_C64 && format != RADE_SPEC_S16_REAL) return 1;
    return ((uintptr_t)x_dev & (format == RADE_SPEC_C64 ? 7 : 1)) || !isfinite(gain) || !(gain > 0.0f);
}

int rade_batch_psd(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int format, float gain, int win, int step, double Fs,
                   float *psd_dev, long psd_stride, int *n_seg_host, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !n_host || !psd_dev || !n_seg_host) return -1;
    if (psd_input_bad(x_dev, format, gain) || ((uintptr_t)psd_dev & 3) || !isfinite(Fs) || !(Fs > 0.0) || psd_stride < RD_PSD_NFFT) return -1;
    rade_psd_plan_t q;
    if (rade_psd_plan(win, step, &q)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    long long max_seg = 0, segs = 0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        const int n = n_host[b];
        if (n < 0 || n > x_stride || n < win) return -1;
        const long long ns = rade_psd_segments(n, win, step);
        if (ns > max_seg) max_seg = ns;
        segs += ns;
    }
    struct rd_stages *s = stages_of(h);
    const size_t rec_bytes = (sizeof(double) + sizeof(int)) * B;
    double *rec = s ? pair_host(h, &s->psd_rec, rec_bytes) : NULL;     /* [B] scales, [B] counts */
    const int max_runs = (int)((max_seg + RD_PSD_RUN - 1) / RD_PSD_RUN);
    if (!rec || table_alloc(h, &s->psd_tab, 3L * RD_PSD_NFFT, 0)) return -1;
    if (dev_grow(h, &s->psd_part, &s->psd_cap, max_runs, sizeof(float) * RD_PSD_NFFT * B, 0)) return -1;
    float w[RD_PSD_NFFT];
    double sw2 = 0.0;                      /* of the float32 window, in double, in ascending order */
    rade_psd_window(win, w);
    for (int i = 0; i < win; i++) sw2 += (double)w[i] * (double)w[i];
    if (!table_is(&s->psd_tab, win, 0)) {
        rd_cno_table(RD_PSD_NFFT, s->psd_tab.host);
        memcpy(s->psd_tab.host + 2 * RD_PSD_NFFT, w, sizeof(float) * win);
        if (table_upload(&s->psd_tab, win, 0, 2 * RD_PSD_NFFT + (size_t)win, st)) return -1;
    }
    for (int b = 0; b < B; b++) rec[b] = 1.0 / ((double)rade_psd_segments(n_host[b], win, step) * Fs * sw2);
    memcpy(rec + B, n_host, sizeof(int) * B);
    if (pair_push(h, &s->psd_rec, rec_bytes, 0, st)) { settle(st); return -1; }      /* not waited for here: the call waits at its end */
    rd_psd_args a;
    memset(&a, 0, sizeof a);
    a.x = x_dev; a.x_stride = x_stride; a.scale = s->psd_rec.dev; a.n = (const int *)((const double *)s->psd_rec.dev + B);
    a.tw = s->psd_tab.dev; a.win = s->psd_tab.dev + 2 * RD_PSD_NFFT; a.part = s->psd_part; a.psd = psd_dev; a.psd_stride = psd_stride;
    a.gain = gain; a.fmt = format; a.win_len = win; a.step = step; a.B = B; a.max_runs = max_runs;
    PROF_BEGIN(h, stream);
    const int e = rd_launch_psd(&a, stream);
    PROF_END(h, stream, RADE_PROF_CHAN, 5.0 * RD_PSD_NFFT * 10 * (double)segs);      /* 5 N log2 N per segment, the textbook count */
    /* the stream is waited for (also where the launch failed: the staging copies above are then free again) */
    if (settle(st) || e) return -1;
    table_commit(&s->psd_tab);
    for (int b = 0; b < B; b++) n_seg_host[b] = (int)rade_psd_segments(n_host[b], win, step);
    return 0;
}

int rade_batch_sigstat(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int format, float gain, int head, rade_sigstat_result *result_host,
                       void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !n_host || !result_host || head < 0 || psd_input_bad(x_dev, format, gain)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    long long max_n = 0, total = 0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        const int n = n_host[b];
        if (n < 0 || n > x_stride) return -1;
        if (n > max_n) max_n = n;
        total += n;
    }
    struct rd_stages *s = stages_of(h);
    int *n_stage = s ? pair_host(h, &s->stat_n, sizeof(int) * B) : NULL;
    const int max_chunks = (int)((max_n + RD_STAT_CHUNK - 1) / RD_STAT_CHUNK);
    if (!n_stage || dev_grow(h, &s->stat_part, &s->stat_cap, max_chunks ? max_chunks : 1, sizeof(double) * 4 * B, 0)) return -1;
    if (dev_grow(h, &s->stat_out, NULL, 4L * B, sizeof(double), 1)) return -1;
    memcpy(n_stage, n_host, sizeof(int) * B);
    if (pair_push(h, &s->stat_n, sizeof(int) * B, 0, st)) { settle(st); return -1; } /* not waited for here: the read-back waits */
    rd_stat_args a;
    memset(&a, 0, sizeof a);
    a.x = x_dev; a.x_stride = x_stride; a.n = s->stat_n.dev; a.part = s->stat_part; a.out = s->stat_out; a.gain = gain; a.fmt = format; a.head = head; a.B = B;
    a.max_chunks = max_chunks;
    PROF_BEGIN(h, stream);
    const int e = rd_launch_sigstat(&a, stream);
    PROF_END(h, stream, RADE_PROF_CHAN, 4.0 * (double)total);
    const double *r = NULL;
    if (e || !(r = read_back(h, s->stat_out, sizeof(double) * 4 * B, st))) { settle(st); return -1; }
    for (int b = 0; b < B; b++) {
        rade_sigstat_result o = { r[4 * b], r[4 * b + 1], r[4 * b + 2], r[4 * b + 3], n_host[b] };
        result_host[b] = o;
    }
    return 0;
}

/* ---- whole-file pilot acquisition: every hop of rx.py's frame loop, and acquisition.refine for a list of events (rade_acq.hip; the state machine and the statistics:
 * rade_host.c) ---------------------------------------------------------------------------------------------------------------------------------------------------- */
int rade_batch_acq_detect(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, double Pacq_error1, rade_acq_hop *hops_host, int max_hops, int *n_hops_host,
                          void *dt_dev, long long t0, int n_rows, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !n_host || !hops_host || !n_hops_host || (((uintptr_t)x_dev | (uintptr_t)dt_dev) & 7)) return -1;
    if (!(Pacq_error1 > 0.0 && Pacq_error1 < 5.0)) return -1;
    if (dt_dev && (t0 < 0 || n_rows < 1 || t0 + n_rows > x_stride)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    int maxh = 0;
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        const int n = n_host[b];
        if (n < 0 || n > x_stride) return -1;
        const int nh = rd_acq_hops(n);
        if (nh > max_hops) return -1;
        if (nh > maxh) maxh = nh;
        if (nh) work += 2.0 * 16 * 16 * 32 * 85 * (RD_NMF / 16) * (nh + 1.0);      /* 85 matrix instructions per tile of 16 timings and block */
    }
    const rd_acq_rec *rec = NULL;          /* [B][maxh], read back */
    if (maxh) {
        struct rd_stages *s = stages_of(h);
        int *n_stage = s ? pair_host(h, &s->acq_n, sizeof(int) * B) : NULL;
        if (!n_stage) return -1;
        if (dev_grow(h, &s->acq_psum, &s->acq_cap, maxh, sizeof(double) * RD_ACQ_NPART * B * 2, 1)) return -1;      /* maxh + 1 <= 2 maxh blocks */
        if (dev_grow(h, &s->acq_pmax, &s->acq_cap1, maxh, sizeof(rd_acq_pmax) * RD_ACQ_NPART * B, 1)) return -1;
        if (dev_grow(h, &s->acq_rec, &s->acq_cap2, maxh, sizeof(rd_acq_rec) * B, 1)) return -1;
        memcpy(n_stage, n_host, sizeof(int) * B);
        if (pair_push(h, &s->acq_n, sizeof(int) * B, 0, st)) return -1;              /* not waited for here: the call waits at its end */
        rd_acq_args a;
        memset(&a, 0, sizeof a);
        a.corrq16 = h->corrq16; a.corra16 = h->corra16; a.x = x_dev; a.x_stride = x_stride; a.n = s->acq_n.dev; a.psum = s->acq_psum; a.pmax = s->acq_pmax; a.rec = s->acq_rec;
        a.dt = dt_dev; a.t0 = t0; a.n_rows = n_rows; a.B = B; a.max_hops = maxh;
        PROF_BEGIN(h, stream);
        const int e = rd_launch_acq_detect(&a, stream);
        PROF_END(h, stream, RADE_PROF_CHAN, work);         /* booked with the other front-end stages, as C/No and the spectrogram are: the profile's classes are the
                                                            * benchmark's (rade_batch_profile), and a run that mixes channel and acquisition calls sees both under `channel` */
        /* the records come back and the stream is waited for (also where the launch failed: the staging copy above is then free again) */
        if (e || !(rec = read_back(h, s->acq_rec, sizeof(rd_acq_rec) * B * maxh, st))) { settle(st); return -1; }
    } else if (settle(st)) return -1;
    const double k = 2.0 * sqrt(-log(Pacq_error1 / 5.0));
    for (int b = 0; b < B; b++) {
        const int nh = rd_acq_hops(n_host[b]);
        n_hops_host[b] = nh;
        for (int j = 0; j < nh; j++) {
            const rd_acq_rec *r = &rec[(size_t)b * maxh + j];
            rade_acq_hop *o = &hops_host[(size_t)b * max_hops + j];
            const double sigma_r = (r->S1 + r->S2) / (double)(RD_NMF * RD_NFC) / sqrt(M_PI / 2.0) / 2.0;
            o->Dtmax12 = r->best; o->Dthresh = k * sigma_r; o->tmax = r->key >> 6; o->f_ind = r->key & 63; o->candidate = (double)r->best > o->Dthresh;
            o->S1 = r->S1; o->S2 = r->S2;
        }
    }
    return 0;
}

int rade_batch_acq_refine(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, const rade_acq_refine_in *events_host, int n_events,
                          rade_acq_refined *out_host, double *dfine_host, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !n_host || n_events < 0 || (n_events && (!events_host || !out_host)) || ((uintptr_t)x_dev & 7)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < B; b++) if (n_host[b] < 0 || n_host[b] > x_stride) return -1;
    for (int e = 0; e < n_events; e++) {   /* every event is checked before anything is launched or written */
        const rade_acq_refine_in *v = &events_host[e];
        if (v->stream < 0 || v->stream >= B || v->t_abs > (1LL << 40) || v->t_abs < -(1LL << 40) || !isfinite(v->fmax)) return -1;
    }
    if (!n_events) return settle(st);
    struct rd_stages *s = stages_of(h);
    int *n_stage = s ? pair_host(h, &s->acq_n, sizeof(int) * B) : NULL;
    rd_acq_ev *ev = s ? pair_host(h, &s->acq_ev, sizeof(rd_acq_ev) * RD_ACQ_EV_CHUNK) : NULL;
    if (!n_stage || !ev) return -1;
    if (dev_grow(h, &s->acq_fine, NULL, RD_ACQ_EV_CHUNK, sizeof(rd_acq_fine), 1) || dev_grow(h, &s->acq_dfine, NULL, (long)RD_ACQ_EV_CHUNK * RD_ACQ_NFINE, sizeof(double), 1)) return -1;
    memcpy(n_stage, n_host, sizeof(int) * B);
    if (pair_push(h, &s->acq_n, sizeof(int) * B, 0, st)) return -1;
    for (int e0 = 0; e0 < n_events; e0 += RD_ACQ_EV_CHUNK) {                         /* a chunk per launch; each chunk's read-back waits for the stream */
        const int ne = n_events - e0 < RD_ACQ_EV_CHUNK ? n_events - e0 : RD_ACQ_EV_CHUNK;
        memset(ev, 0, sizeof(rd_acq_ev) * RD_ACQ_EV_CHUNK);
        for (int e = 0; e < ne; e++) { ev[e].t_abs = events_host[e0 + e].t_abs; ev[e].fmax = events_host[e0 + e].fmax; ev[e].stream = events_host[e0 + e].stream; ev[e].pad = 0; }
        if (pair_push(h, &s->acq_ev, sizeof(rd_acq_ev) * RD_ACQ_EV_CHUNK, 0, st)) { settle(st); return -1; }      /* the whole chunk: the device copy is sized by its first push */
        rd_acq_refine_args a;
        memset(&a, 0, sizeof a);
        a.tab = h->d_tab; a.x = x_dev; a.x_stride = x_stride; a.n = s->acq_n.dev; a.ev = s->acq_ev.dev; a.out = s->acq_fine; a.dfine = s->acq_dfine; a.n_events = ne;
        PROF_BEGIN(h, stream);
        const int err = rd_launch_acq_refine(&a, stream);
        PROF_END(h, stream, RADE_PROF_CHAN, 8.0 * 2 * RD_M * 3 * RD_ACQ_NFINE * ne);
        const rd_acq_fine *res = err ? NULL : read_back(h, s->acq_fine, sizeof(rd_acq_fine) * ne, st);
        if (!res) { settle(st); return -1; }
        for (int e = 0; e < ne; e++) { out_host[e0 + e].t = res[e].t; out_host[e0 + e].f = res[e].f; out_host[e0 + e].Dmax = res[e].Dmax; }
        if (dfine_host) {
            const double *d = read_back(h, s->acq_dfine, sizeof(double) * RD_ACQ_NFINE * ne, st);
            if (!d) { settle(st); return -1; }
            memcpy(dfine_host + (size_t)e0 * RD_ACQ_NFINE, d, sizeof(double) * RD_ACQ_NFINE * ne);
        }
    }
    return 0;
}

/* ---- the stored-file receiver past the acquisition: the whole-file band-pass (rade_file.hip) and the plan of rx.py; its ragged demodulator and BER alignment follow with
 * the fixed-timing receiver (include/rade_batch.h states the arithmetic) --------------------------------------------------------------------------------------------------------------------- */
_Static_assert(RADE_FILE_BPF_SPAN == RD_FILE_SPAN && RD_FILE_CHUNK == 1024, "the header's span is the kernel's (rade_file.hip: a chunk is four tiles of 256)");
/* complex_bpf's mixer step as rd_tables_fill forms it (rade_host.c: float32 like NumPy), as a double */
static double file_bpf_alpha(void)
{
    const float two_pi = (float)(2.0 * M_PI), w0 = (two_pi * 15.0f) / 160.0f, w1 = (two_pi * (float)(15 + RD_NC - 1)) / 160.0f;
    const float centre = (((w1 + w0) * 8000.0f) / two_pi) / 2.0f;
    return (double)((two_pi * centre) / 8000.0f);
}

int rade_batch_bpf_file(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, void *y_dev, long y_stride, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !y_dev || !n_host || (((uintptr_t)x_dev | (uintptr_t)y_dev) & 7) || x_stride < 0 || y_stride < 0) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    int maxn = 0;
    long long lo = -1, hi = 0;             /* the samples any stream touches, relative to either base: [lo, hi) */
    double work = 0.0;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        const int n = n_host[b];
        if (n < 0 || n > x_stride || n > y_stride) return -1;
        if (n > maxn) maxn = n;
        work += 2.0 * 16 * 16 * 32 * 24 * ((n + 255) / 256);
    }
    if (!maxn) return 0;
    for (int b = 0; b < B; b++) if (n_host[b]) { if (lo < 0) lo = b; hi = b; }
    {   /* y overlapping x: the extents from the first non-empty stream's first sample to the last one's last, held against each other */
        const uintptr_t x0 = (uintptr_t)x_dev + 8 * (uintptr_t)(lo * x_stride), x1 = (uintptr_t)x_dev + 8 * (uintptr_t)(hi * x_stride + n_host[hi]);
        const uintptr_t y0 = (uintptr_t)y_dev + 8 * (uintptr_t)(lo * y_stride), y1 = (uintptr_t)y_dev + 8 * (uintptr_t)(hi * y_stride + n_host[hi]);
        if (x0 < y1 && y0 < x1) return -1;
    }
    struct rd_stages *s = stages_of(h);
    int *n_stage = s ? pair_host(h, &s->file_n, sizeof(int) * B) : NULL;
    if (!n_stage) return -1;
    const long n_phase = ((long)maxn + RD_FILE_SPAN - 1) / RD_FILE_SPAN * RD_FILE_SPAN;
    if (dev_grow(h, &s->file_phase, &s->file_phase_cap, n_phase, 2 * sizeof(float), 0)) return -1;
    memcpy(n_stage, n_host, sizeof(int) * B);
    if (pair_push(h, &s->file_n, sizeof(int) * B, 0, st)) return -1;       /* not waited for here: the call waits at its end */
    rd_file_bpf_args a;
    memset(&a, 0, sizeof a);
    a.bpf16 = h->bpf16; a.x = x_dev; a.x_stride = x_stride; a.y = y_dev; a.y_stride = y_stride; a.n = s->file_n.dev; a.phase = s->file_phase; a.n_phase = n_phase;
    a.alpha = file_bpf_alpha(); a.B = B; a.max_n = maxn;
    PROF_BEGIN(h, stream);
    const int e = rd_launch_file_bpf(&a, stream);
    PROF_END(h, stream, RADE_PROF_CHAN, work);
    return (settle(st) || e) ? -1 : 0;     /* the staging copy of the counts is free again */
}

int rade_file_plan(long long n, int hop, long long t, double f, const double *freq_override, rade_file_plan_out *out)
{
    if (!out || n < 0 || !isfinite(f) || (freq_override && !isfinite(*freq_override))) return -1;
    out->start = 0; out->n_mf = 0; out->freq = freq_override ? *freq_override : f;
    if (hop < 0) { out->status = RADE_FILE_NOT_ACQUIRED; return 0; }
    const long long base = (long long)RD_NMF * (hop + 1), len = n - (hop + 1);      /* rx = rx[Nmf:-1] once more after the acquiring hop (rx.py:186-187) */
    if (t < 0 || t + RD_NMF + RD_M > len) { out->status = RADE_FILE_REFINE_OUTSIDE; return 0; }
    if (t - base < RD_NCP) { out->status = RADE_FILE_EARLY; return 0; }             /* rx[tmax - Ncp:] with a negative index would wrap to the tail */
    out->start = t - RD_NCP;
    const long long n_left = len - out->start;
    out->n_mf = (int)((n_left / (RD_M + RD_NCP)) / (RD_NS + 1));
    if (out->n_mf < 2) { out->start = 0; out->n_mf = 0; out->status = RADE_FILE_SHORT; return 0; }
    out->status = RADE_FILE_OK;
    return 0;
}

/* ---- the fixed-timing receiver (radae.py:312-420, :590-657; rade_irx.hip): the ideal-timing call and the stored-file call side by side.  What the two share -------- */
/* what both refuse: a DFT window outside its symbol, an unknown EQ and, where the call decodes, more rows than the decoder holds or a z_hat_dev the decoder cannot read
 * (as rade_batch_decode does: f32x4 A rows) */
static int fixed_rx_bad(const rade_batch *h, int n_mf, int time_offset, int eq, const float *z_hat_dev, const float *features_out_dev)
{
    if (time_offset < -RD_NCP || time_offset > 0 || eq < RADE_EQ_LS || eq > RADE_EQ_NONE) return 1;
    return features_out_dev && (3 * n_mf > h->Tcap || ((uintptr_t)z_hat_dev & 15));
}
/* the coarse_mag factor: |P[0]| / pilot_gain (radae.py:196-199, :379-380), 1 for the bottleneck-1 waveform */
static float fixed_rx_mag_scale(const rade_batch *h)
{
    return h->tx_linear ? 1.0f : (float)(sqrt(2.0) / ((pow(10.0, -2.0 / 20.0) * RD_M) / sqrt((double)RD_NC)));
}
/* the decode tail: every stream's 3 n_mf rows of z_hat through the stateless decoder, from a zero state */
static int fixed_rx_decode(rade_batch *h, const float *z_hat_dev, int n_mf, float *features_out_dev, void *stream)
{
    return rade_batch_decode(h, z_hat_dev, 3 * n_mf, features_out_dev, 1, stream) == 3 * n_mf ? 0 : -1;
}

/* waits for the stream only where a BER count is read back (and, ahead of the launch, where per-stream offsets are put on the device) */
int rade_batch_rx_ideal(rade_batch *h, const void *rx_dev, long rx_stride, int n_mf, const rade_ideal_rx_params *p,
                        float *z_hat_dev, float *features_out_dev, void *stream)
{
    ON_DEV(h);
    if (!h || !rx_dev || !p || !z_hat_dev || n_mf < 2 || rx_stride < (long)n_mf * RD_NMF || (p->n_errors_host && !p->z_ref_dev)) return -1;
    if (fixed_rx_bad(h, n_mf, p->time_offset, p->eq, z_hat_dev, features_out_dev)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    struct rd_stages *s = stages_of(h);
    if (!s || dev_grow(h, &s->irx_part, &s->irx_part_cap, n_mf, sizeof(double) * B, 1) || dev_grow(h, &s->irx_err, NULL, B, sizeof(long long), 1)) return -1;
    if (p->freq_offset_host) {             /* [2][B]: freq_offset, then df_dt (zeros without) */
        float *fo = pair_host(h, &s->irx_foff, sizeof(float) * 2 * B);
        if (!fo) return -1;
        memcpy(fo, p->freq_offset_host, sizeof(float) * B);
        if (p->df_dt_host) memcpy(fo + B, p->df_dt_host, sizeof(float) * B); else memset(fo + B, 0, sizeof(float) * B);
        if (pair_push(h, &s->irx_foff, sizeof(float) * 2 * B, 1, st)) return -1;
    }
    rd_irx_args a;
    memset(&a, 0, sizeof a);
    a.tab = h->d_tab; a.rx = rx_dev; a.rx_stride = rx_stride; a.foff = p->freq_offset_host ? s->irx_foff.dev : NULL;
    a.n_mf = n_mf; a.time_offset = p->time_offset; a.eq = p->eq; a.coarse_mag = p->coarse_mag; a.B = B;
    a.mag_scale = fixed_rx_mag_scale(h);
    a.z_hat = z_hat_dev; a.part = s->irx_part; a.z_ref = p->z_ref_dev; a.n_err = p->z_ref_dev ? s->irx_err : NULL;
    if (rd_launch_irx(&a, stream)) return -1;
    if (p->n_errors_host) {
        const long long *e = read_back(h, s->irx_err, sizeof(long long) * B, st);
        if (!e) return -1;
        for (int b = 0; b < B; b++) p->n_errors_host[b] = (long)e[b];
    }
    if (features_out_dev && fixed_rx_decode(h, z_hat_dev, n_mf, features_out_dev, stream)) return -1;
    return n_mf;
}

/* always settles: the staging copy of the stream records is free again when it returns */
int rade_batch_rx_file(rade_batch *h, const void *x_dev, long x_stride, const rade_file_rx_in *in_host, int max_mf, int time_offset, int eq, int coarse_mag,
                       float *z_hat_dev, float *features_out_dev, void *stream)
{
    ON_DEV(h);
    if (!h || !x_dev || !in_host || !z_hat_dev || max_mf < 1 || x_stride < 0 || ((uintptr_t)x_dev & 7) || ((uintptr_t)z_hat_dev & 3) || ((uintptr_t)features_out_dev & 3)) return -1;
    if (fixed_rx_bad(h, max_mf, time_offset, eq, z_hat_dev, features_out_dev)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < B; b++) {          /* every stream is checked before anything is launched or written */
        const rade_file_rx_in *v = &in_host[b];
        if (v->n_mf < 0 || v->n_mf == 1 || v->n_mf > max_mf || v->start < 0 || !isfinite(v->freq)) return -1;      /* the demodulator needs two pilots; 0 = a stream of zeros */
        if (v->start > x_stride || v->start + (long long)RD_NMF * v->n_mf > x_stride) return -1;
    }
    struct rd_stages *s = stages_of(h);
    rd_file_rx_rec *rec = s ? pair_host(h, &s->file_rx, sizeof(rd_file_rx_rec) * B) : NULL;
    if (!rec) return -1;
    if (dev_grow(h, &s->file_part, &s->file_part_cap, max_mf, sizeof(double) * B, 1)) return -1;
    for (int b = 0; b < B; b++) {
        rec[b].start = in_host[b].start; rec[b].n_mf = in_host[b].n_mf; rec[b].pad = 0;
        rec[b].w = in_host[b].freq == 0.0 ? 0.0 : 2.0 * M_PI * in_host[b].freq / 8000.0;
    }
    if (pair_push(h, &s->file_rx, sizeof(rd_file_rx_rec) * B, 0, st)) return -1;
    rd_file_rx_args a;
    memset(&a, 0, sizeof a);
    a.tab = h->d_tab; a.x = x_dev; a.x_stride = x_stride; a.rec = s->file_rx.dev; a.max_mf = max_mf; a.time_offset = time_offset; a.eq = eq; a.coarse_mag = coarse_mag; a.B = B;
    a.mag_scale = fixed_rx_mag_scale(h);
    a.z_hat = z_hat_dev; a.part = s->file_part;
    PROF_BEGIN(h, stream);
    int e = rd_launch_file_rx(&a, stream);
    PROF_END(h, stream, RADE_PROF_CHAN, 8.0 * RD_M * RD_NC * (RD_NS + 2) * (double)max_mf * B);
    if (!e && features_out_dev) e = fixed_rx_decode(h, z_hat_dev, max_mf, features_out_dev, stream);
    return (settle(st) || e) ? -1 : max_mf;
}

int rade_batch_ber_align(rade_batch *h, const float *z_ref_dev, long ref_stride, const long *n_ref_host, const float *z_hat_dev, long hat_stride, const long *n_hat_host,
                         long *n_errors_host, void *stream)
{
    ON_DEV(h);
    if (!h || !z_ref_dev || !z_hat_dev || !n_ref_host || !n_hat_host || !n_errors_host || (((uintptr_t)z_ref_dev | (uintptr_t)z_hat_dev) & 3)) return -1;
    const int B = h->B;
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < B; b++) if (n_ref_host[b] < 0 || n_ref_host[b] > ref_stride || n_hat_host[b] < 0 || n_hat_host[b] > hat_stride) return -1;
    struct rd_stages *s = stages_of(h);
    rd_file_ber_rec *rec = s ? pair_host(h, &s->file_ber, sizeof(rd_file_ber_rec) * B) : NULL;
    if (!rec) return -1;
    if (dev_grow(h, &s->file_err, NULL, (long)B * RD_FILE_NSHIFT, sizeof(long long), 1)) return -1;
    for (int b = 0; b < B; b++) { rec[b].n_ref = n_ref_host[b]; rec[b].n_hat = n_hat_host[b]; }
    if (pair_push(h, &s->file_ber, sizeof(rd_file_ber_rec) * B, 0, st)) return -1;
    rd_file_ber_args a;
    memset(&a, 0, sizeof a);
    a.z_ref = z_ref_dev; a.ref_stride = ref_stride; a.z_hat = z_hat_dev; a.hat_stride = hat_stride; a.rec = s->file_ber.dev; a.n_err = s->file_err; a.B = B;
    const int e = rd_launch_file_ber(&a, stream);
    const long long *res = e ? NULL : read_back(h, s->file_err, sizeof(long long) * B * RD_FILE_NSHIFT, st);
    if (!res) { settle(st); return -1; }
    for (int i = 0; i < B * RD_FILE_NSHIFT; i++) n_errors_host[i] = (long)res[i];
    return 0;
}

int rade_ber_best(const long *n_errors, long n_ref, double *ber_out)
{
    if (!n_errors || n_ref < 0) return -1;
    double best = 1.0;
    int at = -1;
    for (int f = 0; f < RD_FILE_NSHIFT; f++) {
        const long n_bits = n_ref - (long)RD_ZMF * f;      /* the script's own denominator: what is left of the reference, not the symbols compared */
        if (n_bits <= 0 || n_errors[f] < 0) break;
        const double ber = (double)n_errors[f] / (double)n_bits;
        if (ber < best) { best = ber; at = f; }
    }
    if (ber_out) *ber_out = best;
    return at;
}
