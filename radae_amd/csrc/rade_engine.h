/*
 * rade_engine.h -- private to the batched engine's host files: what rade_stages.c (the front-end stage calls) needs of rade_engine.c (the engine itself).
 *
 * The stage file reads B, device and d_tab of an engine, keeps its own state behind h->stages, allocates through the engine's owner functions (everything a stage
 * allocates stays on the engine's own list and is released by rade_batch_close), reads results back with read_back and brackets its launches with PROF_BEGIN /
 * PROF_END.  The other members of struct rade_batch are rade_engine.c's.  The functions declared here cross files inside the library only: hidden visibility.
 */
#ifndef RADE_ENGINE_H
#define RADE_ENGINE_H
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "rade_batch.h"
#include "rade_host.h"

#define RD_HIDDEN __attribute__((visibility("hidden")))

typedef struct { float *wp, *bias; unsigned short *wp16, *wa16; float *wscale, *wscale16; int N, K; } dev_lin;   /* wscale16: column scales when wp16 is one plane of integers */

/* every public entry point runs on its engine's device, whatever device the calling thread had current (one host thread may
 * drive several engines, and an engine may be called from a thread other than the one that opened it) */
#define ON_DEV(h) do { if (h) (void)hipSetDevice((h)->device); } while (0)

#define RADE_PROF_MAXEV 256   /* launches recorded per profiled interval before the events are drained */
#define RADE_PROF_MAXIV 4096  /* launch intervals kept per profiling session (rade_batch_profile_intervals) */
struct rd_stages;             /* the state of the front-end stage calls (rade_stages.c), made by the first of them */
struct rade_batch {
    struct owned *owned;                  /* every device / pinned allocation of the engine (own): rade_batch_close frees exactly these */
    int alloc_failed;                     /* sticky: an allocation the engine cannot do without failed (rade_batch_open_mem checks it) */
    int B, max_tx_mf, device, flags, trace_cap, Tcap;
    int R, dec_rows;                      /* do_radae_rx calls per stream per sync launch; 3R decoder slots */
    int unsync_off_after;                 /* int(disable_unsync * Fs / Nmf) or -1 */
    unsigned short *corrq16, *corra16, *wfwd16, *bpf16; double *vm; int rx_lds, rx_census;   /* dynamic LDS of a receiver launch; phase mask of the -DRX2_CENSUS developer build */
    int feat_in, enc_kpad, bottleneck1;   /* 84 (model19: 4x21) or 80 (model05/bbfm: 4x20); tanh on z when bottleneck 1 */
    float *dec2_x, *dec2_gi, *dec2_hbuf, *dec2_h[5];   /* stand-alone decoder (rade_batch_decode) */
    rd_tables *d_tab;
    /* weights */
    dev_lin enc_dense1, enc_zdense, dec_dense1, dec_output, enc_gin[5], dec_gin[5], enc_conv[5], dec_conv[5], dec_glu[5];
    float *enc_whh[5], *enc_bhh[5], *dec_whh[5], *dec_bhh[5];
    unsigned short *dec_whq[5]; float *dec_whs[5];      /* decoder W_hh as matrix-core fragments (int8-exact) + row scales; NULL when the blob's recurrent weights are not int8 x scale */
    /* transmit side */
    float *enc_xin, *enc_x, *enc_gi, *enc_h[5], *enc_z, *eoo, *eoo_bits;
    unsigned short *enc_xf; int enc_nq, enc_seq_taps, enc_no_pair;
    int enc_hist_frag;                   /* the history tile of enc_xf holds what enc_x's two float32 history rows hold (set by a fragment pass, cleared by a reset or a float32-row pass) */   /* the concat buffer as matrix-core operand fragments (rade_enc.hip: [B][enc_nq][RD_EF_TILE] binary16), engines with enough rows for the batched GEMMs only */
    /* optional Tx band-pass filter + clip (RADE_BATCH_TX_BPF; radae_txe.py:74-83): filter state per stream, its initial value, the modulator's raw output, block phases */
    int bypass_dec;                          /* RADE_BATCH_BYPASS_DEC */
    int tx_linear;                           /* RADE_BATCH_TX_LINEAR */
    rd_bpf_state *tx_bpf, *tx_bpf_init; void *tx_raw; float *tx_chain; float *eoo_filt;   /* eoo_filt [B][Neoo] c64: the end-of-over frame as transmitted (filtered + clipped) for the channel's with_eoo */
    void *chan_scratch; void *chan_mp;        /* chan_mp [B][max_tx_mf * 960] c64: multipath output of the fused modulator (rade_batch_tx_channel), allocated on first use */
    float *chan_ps; void *chan_ps_host;       /* rade_channel_streams: [3][B] sigma, freq_offset, df_dt on the device and its pinned staging copy, allocated on first use */
    int *loss_len; void *loss_len_host; double *loss_res, *loss_part; long loss_part_cap;   /* rade_batch_loss: [2][B] n_in, n_hat and their pinned staging copy; [B] losses + [B] starts; [B][cap] block partials (doubles, then ints) */
    struct rd_stages *stages;                 /* rade_stages.c: everything the front-end stage calls keep between calls; NULL until the first of them */
    void *rb_host; size_t rb_cap;             /* read_back: the pinned area results land in on their way to the caller, grown to the largest read-back seen */
    /* receive side */
    rd_rx_stream *rx_st; rd_rx_round *rx_round;
    int *rx_avail, *rx_acc, *rx_progress, *rx_status;
    float *zrows, *dec_x, *dec_gi, *dec_hbuf, *dec_h[5], *feat84, *dtcache;
    void *rx_filt; float *bpf_chain; long filt_cap, chain_stride;   /* band-pass pre-pass of an invocation: filtered samples [B][filt_cap] c64 and block phases [B][chain_stride] c64, grown on demand */
    rd_rx_trace *trace; float *trace_z;
    long long *wg_cycles;            /* [B] per-stream cycles of the last receiver launch */
    int *h_small;                    /* rade_batch_rx's pinned scratch: the progress word and the per-stream results of a launch (8 + 8 B ints) */
    unsigned *lcg_seeds;             /* host copy for resets */
    unsigned *d_lcg_seeds;
    /* optional per-kernel-class timing with HIP events (bench.py roofline leg; never on in timed runs) */
    int prof_on, prof_cnt; hipEvent_t prof_ev[2 * RADE_PROF_MAXEV]; int prof_cls[RADE_PROF_MAXEV]; double prof_fl[RADE_PROF_MAXEV];
    double prof_ms[RADE_PROF_NCLASS], prof_flops[RADE_PROF_NCLASS]; long prof_n[RADE_PROF_NCLASS];
    /* optional: absolute start / end of every profiled launch relative to a caller-supplied event (launches of several engines on one time axis) */
    hipEvent_t prof_ref; int iv_n; int iv_cls[RADE_PROF_MAXIV]; float iv_t0[RADE_PROF_MAXIV], iv_t1[RADE_PROF_MAXIV];
    hipEvent_t ev_block;             /* the event rade_batch_rx sleeps on (sleep_until_event) when the host has fewer CPUs than engines (sync_blocking_now) */
    long n_sync_block, n_sync_spin;  /* waits of either kind so far (rade_batch_sync_counts) */
    double wait_est_us;              /* how long the sleeping wait of rade_batch_rx lasted lately (running average): the next one sleeps through most of that before it polls */
};

/* ---- the engine's memory (rade_engine.c): every allocation is recorded on the engine, and rade_batch_close releases what was recorded ---- */
RD_HIDDEN void *pinned_alloc_opt(rade_batch *h, size_t bytes);
RD_HIDDEN void *dev_upload_opt(rade_batch *h, const void *src, size_t bytes);
RD_HIDDEN int dev_grow(rade_batch *h, void *ptr_addr, long *cap, long need, size_t elem_bytes, int zeroed);
RD_HIDDEN void disown(rade_batch *h, void *p);
/* `bytes` of results at `dev` through the engine's pinned landing area, waited for: where they landed (valid until the engine's next read-back), NULL = failed */
RD_HIDDEN const void *read_back(rade_batch *h, const void *dev, size_t bytes, hipStream_t st);
/* rade_stages.c: what rade_batch_close owes the stage state (its device and pinned memory is on the engine's list) */
RD_HIDDEN void rd_stages_free(struct rd_stages *s);

/* ---- per-kernel-class timing (rade_engine.c: HIP events on the launch stream, read back by prof_drain) ---- */
RD_HIDDEN void prof_drain(rade_batch *h);
#define PROF_BEGIN(h, st) do { if ((h)->prof_on) { if ((h)->prof_cnt >= RADE_PROF_MAXEV) prof_drain(h); hipEventRecord((h)->prof_ev[2 * (h)->prof_cnt], (hipStream_t)(st)); } } while (0)
#define PROF_END(h, st, cls, fl) do { if ((h)->prof_on) { hipEventRecord((h)->prof_ev[2 * (h)->prof_cnt + 1], (hipStream_t)(st)); \
    (h)->prof_cls[(h)->prof_cnt] = (cls); (h)->prof_fl[(h)->prof_cnt] = (fl); (h)->prof_cnt++; } } while (0)

#endif
