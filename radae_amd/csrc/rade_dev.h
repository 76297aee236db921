/*
 * rade_dev.h -- data layouts shared by the C host (rade_engine.c / rade_tables.c) and the HIP
 * kernels (rade_kernels.hip), and the thin launch shims the host calls ("FFI" between plain C and
 * device code).  Everything here is POD; float2-like pairs are spelled as float[2] so that plain C
 * can fill them.
 */
#ifndef RADE_DEV_H
#define RADE_DEV_H

#include <stdint.h>
#include "rade_model_geom.h"         /* the encoder's and decoder's layer shapes (RM_*), with the asserts that tie them */

#ifdef __cplusplus
extern "C" {
#endif

/* numerology of RADE V1 / model19_check3 (radae/radae.py:128-234) */
#define RD_M        160   /* samples per OFDM symbol body */
#define RD_NCP      32    /* cyclic prefix */
#define RD_SYM      192
#define RD_NC       30    /* carriers */
#define RD_NS       4     /* data symbols per modem frame */
#define RD_NMF      960   /* samples per modem frame */
#define RD_NEOO     1152
#define RD_RXBUF    2112  /* 2*Nmf + M + Ncp */
#define RD_NFC      40    /* coarse frequency bins */
#define RD_NQ       16    /* polynomial moments of the two-stage pilot correlator (rade_pack.c: rd_corrq16_table_fill) */
#define RD_NTAP     101
#define RD_NINMAX   1120
#define RD_LATENT   RM_LATENT
#define RD_ZMF      240   /* latent floats per modem frame */
#define RD_FEAT_MF  432   /* 12 frames x 36 */
#define RD_NEOOBITS 180
#define RD_ENC_W    RM_ENC_W   /* encoder concat width */
#define RD_DEC_W    RM_DEC_W
#define RD_ENC_IN   RM_FEAT_PAD /* 84 padded to a multiple of 16 (k-block of the f16 matrix instructions) */
#define RD_RX_ROUND_MAX 128   /* capacity: do_radae_rx calls per stream per sync-kernel launch (engine picks R <= this) */
#define RD_DEC_ROWS_MAX (3 * RD_RX_ROUND_MAX)
/* geometry of the two-stage pilot correlator's operand tables (rade_corr2.h explains them and checks the divisions; rade_pack.c fills them).  A fragment plane is what
 * the 64 lanes of one v_mfma_f32_16x16x32_f16 operand hold, 8 binary16 each; every table entry is two of them (hi, lo) */
#define RD_FRAG_HALFS (64 * 8)
#define RD_CORR_NRT (2 * RD_NQ / 16)                            /* stage 1, row tiles: 16 of the rows (moment, re | im) */
#define RD_CORR_NKS (2 * RD_M / 32)                             /* stage 1, k-steps: 32 of the columns (sample, re | im) */
#define RD_CORR_NFT (2 * RD_NFC / 16)                           /* stage 2, frequency tiles: 16 of the rows (frequency, re | im); below: the binary16 values each of the four operand tables holds */
#define RD_CORRQ16_HALFS (RD_CORR_NRT * RD_CORR_NKS * 2 * RD_FRAG_HALFS)      /* [row tile][k-step][plane][lane][8] */
#define RD_CORRA16_HALFS (RD_CORR_NFT * 2 * RD_FRAG_HALFS)                    /* [frequency tile][plane][lane][8] */
#define RD_WFWD16_HALFS  (2 * RD_CORR_NKS * 2 * RD_FRAG_HALFS)                /* the demodulator DFT: 32 carrier rows over the same K axis */
#define RD_BPF16_HALFS   (4 * 2 * RD_FRAG_HALFS)

/* constant tables, one copy in HBM (filled by rade_tables.c) */
typedef struct {
    float Winv[RD_NC][RD_M][2];        /* radae.py:175-178 */
    float Wfwd[RD_M][RD_NC][2];        /* :179 */
    float P[RD_NC], Pend[RD_NC];       /* real parts (imag = 0), :182-185 */
    float p[RD_M][2], pend[RD_M][2];   /* :183,:186 */
    float eoo[RD_NEOO][2];             /* default EOO frame :208-219 */
    float Pmat[RD_NC][2][3][2];        /* dsp.py:400-412 */
    float eq_rot[RD_NC][2];            /* exp(-1j*w[c]*20), dsp.py:433 */
    float bpf_h[RD_NTAP + 3];          /* dsp.py:46-49 */
    float bpf_E[RD_NEOO][2];           /* phase_vec_exp, dsp.py:61: exp(-j alpha (i + 1)); 1152 entries (the transmit filter also takes the end-of-over frame) */
    float p_w[RD_M][RD_NFC][2];        /* acquisition.p_w, dsp.py:166-173 */
    double fcoarse[RD_NFC];            /* dsp.py:163 */
    float pilot_gain;                  /* radae.py:196-199 */
    float snr_c1, snr_c2;              /* 10log10(Rs*Nc/3000), 10log10((M+Ncp)/M)  dsp.py:453 */
    float pad;
} rd_tables;

/* what complex_bpf carries from call to call (dsp.py:54-61, :96-99): one record per stream and filter (receiver input filter; transmit filter) */
typedef struct {
    int mem_len;                        /* samples of memory: Ntap - 1 = 100 before the first call, Ntap + 1 = 102 afterwards (dsp.py:55 against :96) */
    int grid_off;                       /* receiver: the stream left the block grid of the invocation's pre-pass (a timing slip inside the invocation) and filters its own samples until the invocation ends */
    float phase[2];                     /* the complex64 mixer phase after the last sample filtered */
    float mem[102][2];                  /* the last mem_len baseband samples, oldest first */
} rd_bpf_state;

/* per-stream receiver state (HBM, one record per stream, touched by exactly one workgroup) */
typedef struct {
    int state, nin, tmax, tmax_candidate, valid_count, uw_errors, synced_count, mf;
    int f_ind_max, dec_reset_pending, n_out_frames, pad0;
    uint32_t lcg; int has_eoo, dt_valid;
    int pad1;
    double fmax, foff_err, rx_phase[2];
    double rx_theta;                 /* k_rx_sync2 keeps rx_phase as its angle (rx_phase = e^{j rx_theta}); carried exactly, so results do not depend on how calls are cut into launches */
    double Dthresh, Dtmax12, Dtmax12_eoo;
    float snr_est, pad2[3];
    unsigned rxmax[4];                  /* float bits: largest |re|,|im| of the filtered samples of the last three calls (check_pilots operand scale) */
    long long consumed;                 /* samples consumed since reset */
    rd_bpf_state bpf;                   /* input band-pass filter (radae_rxe.py:104-109, :194-195) */
    float rx_buf[RD_RXBUF][2];
    float rowsum1[RD_NMF], rowsum2[RD_NMF];   /* sum_f |Dt1[t,f]|, |Dt2[t,f]|: all check_pilots ever reads back */
} rd_rx_stream;

/* per-stream, per-launch bookkeeping of the receiver kernel (row flags for its decoder stage, per-call trace indices) */
typedef struct {
    int n_calls;                        /* calls made this round */
    int n_rows;                         /* decoder steps emitted (3 per valid call) */
    int uw_from_row;                    /* aux-bit errors count from this row on (sync entry resets) */
    int consumed;                       /* samples consumed this round */
    int row_reset[RD_DEC_ROWS_MAX];     /* 1: decoder state is reset before this step */
    int call_ret[RD_RX_ROUND_MAX];      /* bit0 valid bit1 eoo */
    int call_row_lo[RD_RX_ROUND_MAX], call_row_hi[RD_RX_ROUND_MAX]; /* trace patching of uw_errors */
    int call_trace_idx[RD_RX_ROUND_MAX];
    int out_base;                       /* valid frames of this invocation written to features_out so far */
    int pad[3];
} rd_rx_round;

/* same layout as rade_rx_trace in include/rade_batch.h */
typedef struct {
    int state_before, state_after, nin_before, nin_after, ret, tmax, f_ind_max, valid_count;
    int uw_errors, synced_count, snr_int, pad;
    double fmax, Dthresh, Dtmax12, Dtmax12_eoo;
    float snrdB_3k_est; float pad2;
} rd_rx_trace;

/* ---- launch shims (defined in rade_kernels.hip and its stage headers / rade_rx.hip) -------------------------------------------- */
typedef void *rd_stream_t;

/* Y[r, n] = act(sum_k A[r,k] W[n,k] + bias[n]) on f32 MFMA; rows r = b*T + t.
 * A row (b,t) = [tap0 | tap1]: tap1 at a1 + b*a1_sb + t*a1_st (K1 floats), tap0 (K0 floats, may be 0)
 * at a0 + b*a0_sb + t*a0_st, or the zero row when reset[b*reset_sb+t] != 0.  Wp = packed weights
 * (rd_pack_weights).  act: 0 none, 1 tanh+clamp, 2 GLU (y = a1[r][n] * sigmoid(acc), clamp). */
typedef struct {
    const float *a1; long a1_sb, a1_st; int K1;
    const float *a0; long a0_sb, a0_st; int K0;
    const int *reset; int reset_sb;    /* optional [B][reset_sb] (reset_sb >= T) */
    const int *n_rows;                 /* optional [B]: rows t >= n_rows[b] are skipped */
    const float *Wp; const float *bias;
    const unsigned short *Wp16;        /* optional rd_pack_weights_f16x2 copy: used for large row counts when K0, K1 are multiples of 16 */
    const float *Wscale;               /* non-NULL: Wp16 is ONE plane of integers (rd_pack_weights_q16, int8-exact layer) and Wscale[n] the column's scale */
    float *y; long y_sb, y_st; int N;  /* N valid outputs (<= 32*NT) */
    int B, T, act;
} rd_gemm_args;
int rd_launch_gemm(const rd_gemm_args *a, rd_stream_t s);
/* packs W[N][K] (row-major) into the fragment order the GEMM kernel streams; returns #floats (K,N padded) */
long rd_pack_weights(const float *W, int N, int K, float *out);
long rd_packed_size(int N, int K);

/* GRU recurrence over T steps, one workgroup per stream.  gi[b][t][3H] = W_ih x + b_ih (from the GEMM).
 * h state [B][H] in/out.  Writes clamp(h_t) to out + b*out_sb + t*out_st. */
typedef struct {
    const float *gi; long gi_sb, gi_st;
    const float *Whh; const float *bhh;   /* [3H][H], [3H], torch gate order r,z,n */
    float *h;                             /* [B][H] */
    float *out; long out_sb, out_st;
    const int *reset; int reset_sb;       /* optional [B][reset_sb]: zero h before step */
    const int *n_rows;                    /* optional [B] */
    int B, T, H;
    unsigned short *outf; int outf_NQ, outf_col;   /* optional (rade_enc.hip): clamp(h_t) as two binary16 planes into columns outf_col.. of the encoder's fragment buffer instead of out */
} rd_scan_args;
int rd_launch_gru_scan(const rd_scan_args *a, rd_stream_t s);

/* ---- the batched encoder on activations stored as matrix-core operand fragments (rade_enc.hip) ----
 * xf [B][NQ][RD_EF_TILE] binary16: per stream a history tile (rows 30, 31 = steps -2, -1) and one tile per 32 steps, a tile = [col / 16][plane hi / lo][(col % 16) / 8][t % 32][col % 8]
 * of 2^8 x = hi + lo.  Y^T = W X^T: K0 columns of the rows dil steps earlier (0: none), then K1 columns of the rows themselves; outputs as float32 rows (y) or into columns ycol.. of
 * the same kind of buffer (yf). */
#define RD_EF_KB   (RD_ENC_W / 16)
#define RD_EF_TILE (RD_EF_KB * 1024)
typedef struct {
    const unsigned short *xf; int NQ;
    int B, T, K0, K1, dil;
    const unsigned short *Wp16; const float *Wscale; const float *bias; int N, act;   /* as rd_gemm_args; act 0 none, 1 tanh + clamp */
    float *y; long y_sb, y_st;
    unsigned short *yf; int ycol;
    int seq_taps, no_pair;                          /* developer switches: conv taps one after the other (the float32-row kernels' summation order); no XCD pairing of column groups */
    int pair;                                       /* set by rd_launch_encf_gemm: the two column groups of a 192-column product as blocks i, i + 8 of a 1-D grid (same XCD) */
    const float *xin; int Kin; const float *Wp;     /* rd_launch_encf_dense1 only: float32 input rows [B][T][Kin], rd_pack_weights copy of dense_1 */
} rd_encf_args;
int rd_launch_encf_gemm(const rd_encf_args *a, rd_stream_t s);
int rd_launch_encf_dense1(const rd_encf_args *a, rd_stream_t s);
/* conv history between calls: dir 0 = the float32 history rows (x32 + b * x32_sb, 2 x RD_ENC_W) -> the history tile; dir 1 = steps T - 2, T - 1 -> history tile and float32 rows */
int rd_launch_encf_hist(unsigned short *xf, int NQ, float *x32, long x32_sb, int B, int T, int dir, rd_stream_t s);

/* encoder input packing: features [B][T*4][36] -> [B][T][88] = 4 x (20 feats, aux -1), zero pad */
int rd_launch_enc_pack(const float *features, float *xin, int B, int T, rd_stream_t s);
int rd_launch_pad_rows(const float *src, float *dst, long R, int K, int Kpad, rd_stream_t s);
int rd_launch_chan_symbol(const float *z, const float *H, const float *noise, float *out, long n_real, int mode, float p0, float p1, unsigned long long seed, rd_stream_t s);
/* x is [B][nhist+Tcap][W]: copy time rows [T, T+nhist) (or [n_rows[b], ..)) of each stream to rows [0, nhist); a stream with n_rows[b] <= 0 is left alone.
 * -1, and nothing launched, for nhist < 1 or nhist * W > 2048 (what a workgroup holds in registers) */
int rd_launch_carry_rows(float *x, int B, int Tcap, int W, int nhist, int T, const int *n_rows, rd_stream_t s);
/* z [B][n_mf*3][80] -> tx [b*stride + mf*960 ...] (transmitter_one, dsp.py:340-378); linear: the bottleneck-1 waveform (unit pilot gain, no limiter) */
int rd_launch_ofdm_mod(const rd_tables *tab, const float *z, void *tx, long tx_stride, int B, int n_mf, int linear, rd_stream_t s);
/* the same with the two-path multipath model applied on the way out: mp [B][n_mf*960] c64, part [B][n_mf][2] sums of |tx|^2, |mp|^2; tx optional */
int rd_launch_ofdm_mod_mp(const rd_tables *tab, const float *z, void *tx, long tx_stride, int B, int n_mf, const void *G, void *mp, double *part, int linear, rd_stream_t s);
/* EOO data symbols: bits [B][180] -> eoo frames [B][1152] (radae.py:441-455); bits NULL = defaults */
int rd_launch_eoo_build(const rd_tables *tab, const float *bits, float *eoo, int B, rd_stream_t s);
int rd_launch_copy_eoo(const float *eoo, void *out, long stride, int B, rd_stream_t s);

/* the fixed-timing receiver of RADAE.forward / RADAE.receiver (rade_irx.hip; the frame body both entries share: irx_frame of rade_irx.h).
 * rd_irx_args, the ideal-timing call: k_irx_demod per (modem frame, stream), then k_irx_scale per stream when coarse_mag (eq != NONE) or a BER count is asked for.
 * rd_file_rx_args, the stored-file call (rade_batch_rx_file): k_file_demod + k_file_scale, the same with each stream's own start, frame count and frequency.
 * rd_file_ber_args (rade_batch_ber_align): k_file_ber, one workgroup per (shift, stream). */
enum { RD_IRX_LS = 0, RD_IRX_MEAN6 = 1, RD_IRX_ALL = 2, RD_IRX_NONE = 3 };
typedef struct {
    const rd_tables *tab; const void *rx; long rx_stride;      /* complex64, stream b at rx + b * rx_stride samples, n_mf * 960 readable */
    const float *foff;                                           /* optional [2][B]: freq_offset, df_dt per stream (Hz, Hz/s); a stream with freq_offset 0 is not corrected */
    int n_mf, time_offset, eq, coarse_mag, B;
    float mag_scale;                                             /* coarse_mag factor: |P[0]| / pilot_gain (bottleneck 3) or 1 */
    float *z_hat;                                                /* [B][n_mf * 3][80] */
    double *part;                                                /* [B][n_mf] sum_c |pilot estimate|^2 */
    const float *z_ref; long long *n_err;                        /* optional BER count: [B][n_mf * 3][80] reference latents, [B] errors */
} rd_irx_args;
int rd_launch_irx(const rd_irx_args *a, rd_stream_t s);
#define RD_FILE_NSHIFT 20                                        /* rx.py:268: the shifts of the BER alignment, in modem frames */
typedef struct { long long start; double w; int n_mf, pad; } rd_file_rx_rec;     /* w = 2 pi freq / 8000, 0: the stream is not mixed */
typedef struct {
    const rd_tables *tab; const void *x; long x_stride;         /* complex64; stream b reads [start, start + 960 n_mf) of its row */
    const rd_file_rx_rec *rec;                                  /* device [B] */
    int max_mf, time_offset, eq, coarse_mag, B;
    float mag_scale;
    float *z_hat;                                               /* [B][3 max_mf][80]; rows past 3 n_mf are written as zeros */
    double *part;                                               /* [B][max_mf] */
} rd_file_rx_args;
int rd_launch_file_rx(const rd_file_rx_args *a, rd_stream_t s);
typedef struct { long long n_ref, n_hat; } rd_file_ber_rec;     /* floats of either side */
typedef struct {
    const float *z_ref; long ref_stride; const float *z_hat; long hat_stride;      /* float32, stream b at + b * stride floats */
    const rd_file_ber_rec *rec;                                 /* device [B] */
    long long *n_err;                                           /* device [B][RD_FILE_NSHIFT] */
    int B;
} rd_file_ber_args;
int rd_launch_file_ber(const rd_file_ber_args *a, rd_stream_t s);

/* time-aligned distortion loss of every stream (rade_loss.hip: loss.py:find_loss :64-91 over distortion_loss, radae_base.py:50-68, first 20 features):
 * k_loss_offsets per (block of RD_LOSS_WG offsets, stream), k_loss_pick per stream, k_loss_frames per (256 frames, stream) when frame_loss is given */
#define RD_LOSS_WG 64
typedef struct {
    const float *feat; long f_stride; int f_row;     /* stream b at feat + b * f_stride, rows f_row floats apart */
    const float *hat; long h_stride; int h_row;
    const int *len;                                  /* device [2][B]: n_in, n_hat */
    double *part_v; int *part_s; int n_blk;          /* [B][n_blk]: best (loss, offset) of each block of offsets; n_blk = 0: no stream is scored */
    double *loss; int *start;                        /* [B] results: NaN / -1 for a stream without 0 < n_hat <= n_in */
    float *frame_loss; long fl_stride; int max_hat;  /* optional [B][fl_stride] per-frame curve at the chosen offset; max_hat = largest scored n_hat */
    int B;
} rd_loss_args;
int rd_launch_loss(const rd_loss_args *a, rd_stream_t s);

/* the rate-Rs channel of the bottleneck-3 model (rade_rs.hip; radae.py:603-634): IDFT, limiter, DFT per OFDM symbol of the no-pilot numerology (20 carriers, 160 samples),
 * then phase offset, |H|, noise.  Every buffer dense: z, z_hat [B][n_steps][80], H [B][2 n_steps][20] float, noise [B][2 n_steps][20] complex64. */
#define RD_RS_NCH 8                                              /* chunks of symbol tiles per stream: the measurement partials are added in this fixed order */
typedef struct {
    const rd_tables *tab; const float *z, *H; const void *noise; float *z_hat;
    int B, n_steps, has_phase; float sigma, ph_re, ph_im;        /* e^{j phase_offset}, applied when has_phase */
    const float *sigma_b;                                        /* optional [B]: sigma of every stream, read in place of the scalar */
    unsigned long long seed;                                     /* noise NULL: Philox keyed by (seed, stream); 0 = no noise */
    double *part;                                                /* [B][RD_RS_NCH][4]: sum |tx'|^2, max |tx'|^2, sum |Y|^2 of each chunk */
    double *stats;                                               /* optional [B][3]: sum |tx'|^2, max |tx'|, sum |Y|^2 (k_rs_stats) */
} rd_rs_args;
int rd_launch_rs_pa(const rd_rs_args *a, rd_stream_t s);

/* the fractional resampler of rade_batch_resample (rade_clk.hip; include/rade_batch.h states the arithmetic): k_clk_resample, one workgroup per (tiles of RD_CLK_TILE
 * consecutive outputs, stream), the tile's input window and the taps in LDS */
#define RD_CLK_TILE 1024
#define RD_CLK_PHASES 256
#define RD_CLK_TAPS 32
typedef struct { long long step_q, t0_q, n0, in_base; int n_in, n_out; } rd_clk_stream;      /* one record per stream; Q32.32 step and start */
typedef struct {
    const void *x; long x_stride; void *y; long y_stride;       /* complex64, stream b at + b * stride samples */
    const rd_clk_stream *ps;                                    /* device [B] */
    const float *taps;                                          /* device [RD_CLK_PHASES + 1][RD_CLK_TAPS] (rade_resample_taps) */
    int mode, B, max_out;                                       /* 0 sinc, 1 linear; max_out = the largest n_out of the call */
} rd_clk_args;
int rd_launch_clk_resample(const rd_clk_args *a, rd_stream_t s);

/* the sound-card wire of rade_batch_wire_in / rade_batch_wire_out (rade_wire.hip): int16 rows on one side, complex64 rows on the other; k_wire_in reads i16 and writes
 * c64, k_wire_out the other way round.  One workgroup per (chunk, stream), n_ch chunks per stream */
#define RD_WIRE_NCH_MAX 64
typedef struct {
    void *i16; long i16_stride;                                 /* stream b at + b * i16_stride int16 elements */
    void *c64; long c64_stride;                                 /* stream b at + b * c64_stride samples */
    const int *n;                                               /* device [B]: samples of every stream */
    int mode, B, n_ch;                                          /* 0 real (one int16 per sample), 1 IQ (two) */
    float k;                                                    /* gain (in) or scale (out) */
    double *part, *meters;                                      /* k_wire_out, optional: [B][n_ch][4] partials and [B][4] = peak |v|, sum v^2, clipped, NaN components */
} rd_wire_args;
int rd_launch_wire_in(const rd_wire_args *a, rd_stream_t s);
int rd_launch_wire_out(const rd_wire_args *a, rd_stream_t s);

/* the rational rate converter of rade_batch_rate_convert (rade_rate.hip; include/rade_batch.h states the arithmetic): k_rate_convert, one workgroup per (tiles of
 * consecutive outputs, stream), the [L][T] table and the tile's input window in LDS.  The window's capacity is fixed (RD_RATE_WIN samples: with the largest table the
 * header admits, rows one float apart from T, a complex window fills 80 KB exactly); the tile follows from it: rd_rate_tile outputs, whose windows span at most
 * (tile - 1) M / L + 1 + T <= RD_RATE_WIN - K + 1 samples for every phase of the tile's first output. */
#define RD_RATE_KMAX 8                                           /* ceil(M / L) of the reduced ratio */
#define RD_RATE_TABLE_MAX 16384                                  /* floats of the table, L T */
#define RD_RATE_WIN 1792                                         /* samples of a tile's window */
#define RD_RATE_TILE_MAX 2048
static inline int rd_rate_tile(int L, int M, int T)              /* of a reduced ratio the entry admits: a multiple of 64, 192 or more */
{
    const int K = (M + L - 1) / L;
    long long t = (long long)(RD_RATE_WIN - T - K) * L / M + 1;
    if (t > RD_RATE_TILE_MAX) t = RD_RATE_TILE_MAX;
    return (int)(t / 64 * 64);
}
typedef struct { long long n0, in_base; int n_in, n_out; } rd_rate_stream;    /* one record per stream */
typedef struct {
    const void *x; long x_stride;                               /* complex64 or int16, stream b at + b * x_stride elements of the buffer */
    void *y; long y_stride;                                     /* complex64 */
    const rd_rate_stream *ps;                                   /* device [B] */
    const float *taps;                                          /* device [L][T] (rade_rate_taps) */
    int L, M, T, tile;                                          /* the reduced ratio, its taps per phase, rd_rate_tile */
    int fmt, B, max_out;                                        /* RADE_RATE_C64 / _S16_REAL / _S16_IQ = 0, 1, 2; max_out = the largest n_out of the call */
    float gain;                                                 /* of the int16 formats */
} rd_rate_args;
int rd_launch_rate_convert(const rd_rate_args *a, rd_stream_t s);

/* the analog FM modulator and demodulator of rade_batch_fm_mod / rade_batch_fm_demod (rade_fm.hip; include/rade_batch.h states the arithmetic).  Modulator: three plain
 * launches (k_fm_sums, k_fm_tile_scan, k_fm_mod) over tiles of RD_FM_TILE samples; demodulator: k_fm_demod, one workgroup per (tiles of RD_FM_TILE outputs, stream),
 * the mixed window, the filtered baseband, the discriminator values and both tap tables in LDS. */
#define RD_FM_TILE 2048                                          /* samples of a tile, both directions */
#define RD_FM_NMAX 512                                           /* taps of either demodulator filter */
typedef struct { long long n0; unsigned ph0; int n; } rd_fm_stream;           /* modulator: absolute index of the first sample (the noise counter), phase in front of it, count */
typedef struct {
    const void *m; long m_stride;                               /* float32 or complex64 (real part used), stream b at + b * m_stride elements */
    void *y; long y_stride;                                     /* complex64 */
    const void *noise; long noise_stride;                       /* complex64 [B][noise_stride] or NULL (generated) */
    const rd_fm_stream *ps;                                     /* device [B] */
    unsigned *tsum;                                             /* device [B][n_tiles]: tile sums, then the phase in front of each tile */
    unsigned *ph_end;                                           /* device [B]: the phase behind the last sample */
    double kc, kd;                                              /* fc / Fs 2^32, fd / Fs 2^32 */
    unsigned long long seed;
    float sg;                                                   /* what multiplies the unit noise: sigma / sqrt 2 (generated, complex), sigma (generated real; explicit) */
    int fmt, real_out, noise_on, B, n_tiles;                    /* fmt: RADE_FM_F32 / RADE_FM_C64 = 0, 1; n_tiles of the longest stream */
} rd_fm_mod_args;
int rd_launch_fm_mod(const rd_fm_mod_args *a, rd_stream_t s);
typedef struct { long long n0, in_base; int n_in, n_out; } rd_fm_dstream;     /* demodulator: absolute index of the first output, of x[b][0]; counts */
typedef struct {
    const void *x; long x_stride;                               /* complex64 */
    void *y; long y_stride;                                     /* float32 or complex64 (imaginary part +0) */
    void *bb_out; long bb_stride;                               /* complex64 or NULL: the filtered baseband of the outputs */
    const rd_fm_dstream *ps;                                    /* device [B] */
    const float *taps;                                          /* device [2][RD_FM_NMAX]: b1, b2 */
    unsigned fcq;                                               /* (uint32) llrint(fc / Fs 2^32) */
    float wd, inv_wd;                                           /* (float)(2 pi fd / Fs), (float)(1 / wd) */
    int N1, N2, fmt, dont_limit, B, max_out;                    /* fmt of y: RADE_FM_F32 / RADE_FM_C64 = 0, 1 */
} rd_fm_demod_args;
int rd_launch_fm_demod(const rd_fm_demod_args *a, rd_stream_t s);
/* tests only: the phasor on n phases (ph, cis_out complex64) and / or the discriminator's atan2 on n complex64 pairs (d, atan_out float32); device pointers, NULL skips */
int rd_launch_fm_probe(const unsigned *ph, void *cis_out, const void *d, float *atan_out, int n, rd_stream_t s);

/* the periodograms of rade_batch_cno_est (rade_cno.hip; include/rade_batch.h states the arithmetic): k_cno_blocks, one workgroup per (residue k mod J, stream), the
 * wanted bins of the last J blocks in LDS, [J][pitch] complex64; k_cno_sum adds the residues.  pitch = the most wanted bins any residue has (rd_cno_pitch). */
#define RD_CNO_H 2000                                            /* the hop, Fs // 4, and the length of a block */
#define RD_CNO_JMAX 32                                           /* blocks per window */
#define RD_CNO_RING_MAX 16000                                    /* complex64 of the ring, J x pitch */
static inline int rd_cno_pitch(int J, int flow_bin, int fhigh_bin, int noise_st, int noise_en)
{   /* a band [lo, hi) holds ceil((hi - r) / J) - ceil((lo - r) / J) bins of residue r (each ceil 0 where its argument is negative): at most ceil((hi - lo) / J) */
    return (fhigh_bin - flow_bin + J - 1) / J + (noise_en - noise_st + J - 1) / J;
}
typedef struct {
    const void *x; long x_stride;                               /* complex64, stream b at + b * x_stride samples */
    const int *n;                                               /* device [B] sample counts */
    const float *tw;                                            /* device [N][2]: e^{-2 pi i m / N} */
    double *part;                                               /* device [B][max_win][J][2]: a residue's band sums of a window */
    double *bands;                                              /* device [B][max_win][2] */
    int N, J, B, max_win;                                       /* max_win: the most windows any stream of the call has; the row length of part and bands */
    int flow_bin, fhigh_bin, noise_st, noise_en, pitch;
} rd_cno_args;
int rd_launch_cno(const rd_cno_args *a, rd_stream_t s);

/* the estimator trials of rade_batch_snr_trials (rade_snr.hip; include/rade_batch.h states the arithmetic): k_snr_trials, one wavefront per (window, stream), lane =
 * carrier, the row and its six terms per carrier in LDS, one lane per sum. */
#define RD_SNR_NW_MAX 66                                         /* pilot rows per window: est_snr.py -T up to 8 s */
#define RD_SNR_HSTEP_MAX 5                                       /* Ns + 1: a rate-Rs file */
#define RD_SNR_NSUM 6                                            /* doubles of rade_snr_sums */
typedef struct { long long row0; int n_win; float sigma; } rd_snr_stream;     /* absolute index of the first pilot row, windows, noise level */
typedef struct {
    const rd_tables *tab;                                       /* P, pilot_gain, Pmat, eq_rot */
    const void *H; long h_stride; int h_step;                   /* complex64 [rows][30] per stream or NULL */
    const void *noise; void *noise_out; long noise_stride;      /* complex64 [n_win Nw][30] per stream; noise NULL: generated from seed */
    const rd_snr_stream *ps;                                    /* device [B] */
    unsigned long long seed;
    double *sums;                                               /* device [B][max_win][RD_SNR_NSUM] */
    int Nw, B, max_win;                                         /* max_win: the most windows any stream of the call has */
} rd_snr_args;
int rd_launch_snr_trials(const rd_snr_args *a, rd_stream_t s);

/* the spectrogram of rade_batch_specgram (rade_spec.hip; include/rade_batch.h states the arithmetic): k_specgram, one workgroup per (run of RD_SPEC_RUN consecutive
 * slices, stream).  A launch does what its three flags say: mag != NULL writes |X[1..1023]|, do_max folds them into peak[b] (cleared by the caller; not together with
 * img), img != NULL writes the levels of bins k0..k1 against peak[b]. */
#define RD_SPEC_WIN 1280
#define RD_SPEC_STEP 160
#define RD_SPEC_NFFT 2048
#define RD_SPEC_RUN 8
enum { RD_SPEC_C64 = 0, RD_SPEC_S16 = 1 };                      /* RADE_SPEC_C64 / RADE_SPEC_S16_REAL */
typedef struct {
    const void *x; long x_stride;                               /* complex64 or int16, stream b at + b * x_stride elements of the buffer */
    const int *n;                                               /* device [B] sample counts */
    const float *tw, *win, *lev;                                /* device: e^{-2 pi i m / 2048} [2048][2], the window [1280], the thresholds T[1..255] */
    float *peak;                                                /* device [B] */
    unsigned char *img; long img_stride;                        /* [B][slices][k1 - k0 + 1] or NULL; bytes per stream */
    float *mag; long mag_stride;                                /* [B][slices][1023] or NULL; floats per stream */
    float gain;                                                 /* of the int16 format */
    int fmt, k0, k1, do_max, B, max_slices;                     /* max_slices: the most slices any stream of the call has */
} rd_spec_args;
int rd_launch_specgram(const rd_spec_args *a, rd_stream_t s);

/* the Welch periodogram of rade_batch_psd (rade_psd.hip; include/rade_batch.h states the arithmetic): k_psd, one workgroup per (run of RD_PSD_RUN consecutive segments,
 * stream), leaves one row of 1024 float32 sums per run; k_psd_fold adds a stream's rows in ascending order in double and scales.  The formats are rd_spec_args'. */
#define RD_PSD_NFFT 1024
#define RD_PSD_WIN_MIN 16
#define RD_PSD_RUN 32
typedef struct {
    const void *x; long x_stride;                               /* complex64 or int16, stream b at + b * x_stride elements of the buffer */
    const int *n;                                               /* device [B] sample counts */
    const double *scale;                                        /* device [B]: 1 / (n_seg Fs sum w^2) */
    const float *tw, *win;                                      /* device: e^{-2 pi i m / 1024} [1024][2], the window [win] */
    float *part;                                                /* device [B][max_runs][1024] */
    float *psd; long psd_stride;                                /* [B][1024]; floats per stream */
    float gain;                                                 /* of the int16 format */
    int fmt, win_len, step, B, max_runs;                        /* max_runs: the most runs any stream of the call has; the row count of part per stream */
} rd_psd_args;
int rd_launch_psd(const rd_psd_args *a, rd_stream_t s);

/* power and peak of rade_batch_sigstat (rade_psd.hip): k_sigstat, one workgroup per (chunk of RD_STAT_CHUNK consecutive samples, stream), leaves (sum, peak, sum and
 * peak over the samples below head) per chunk; k_sigstat_fold adds a stream's chunks in ascending order. */
#define RD_STAT_CHUNK 8192
typedef struct {
    const void *x; long x_stride;                               /* as rd_psd_args */
    const int *n;                                               /* device [B] sample counts */
    double *part;                                               /* device [B][max_chunks][4] */
    double *out;                                                /* device [B][4]: sum2, peak2, head_sum2, head_peak2 */
    float gain;
    int fmt, head, B, max_chunks;                               /* max_chunks: the most chunks any stream of the call has */
} rd_stat_args;
int rd_launch_sigstat(const rd_stat_args *a, rd_stream_t s);

/* whole-file pilot acquisition, rade_batch_acq_detect / _refine (rade_acq.hip; include/rade_batch.h states the arithmetic): k_acq_detect, one wavefront
 * per (RD_ACQ_NPART-th of the 960 within-frame timings, stream), eight to a workgroup, walks the stream's 960-sample blocks and leaves per (block, wavefront) one double sum of |D| and per (hop,
 * wavefront) one best cell; k_acq_combine folds the RD_ACQ_NPART partials of a hop in ascending order.  k_acq_refine: one workgroup per event. */
#define RD_ACQ_NPART 20                                          /* wavefronts per stream (48 timings each) = partials per block and per hop */
#define RD_ACQ_HOP 961                                           /* rx = rx[Nmf:-1]: a hop costs the script 961 samples of its length */
#define RD_ACQ_NFINE 80                                          /* np.arange(fmax - 10, fmax + 10, 0.25) */
#define RD_ACQ_EV_CHUNK 1024                                     /* events per launch of k_acq_refine */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int rd_acq_hops(long long n) { return n < RD_RXBUF ? 0 : (int)((n - RD_RXBUF) / RD_ACQ_HOP) + 1; }
typedef struct { float best; int key; double S1, S2; } rd_acq_rec;          /* a hop as the device leaves it: Dtmax12, (tmax << 6) | f_ind, the two surface sums */
typedef struct { float best; int key; } rd_acq_pmax;
typedef struct {
    const unsigned short *corrq16, *corra16;                    /* the two tables of the two-stage pilot correlator (rade_host.c), as the receiver has them */
    const void *x; long x_stride;                               /* complex64, stream b at + b * x_stride samples */
    const int *n;                                               /* device [B] sample counts */
    double *psum;                                               /* device [B][max_hops + 1][RD_ACQ_NPART]: a wavefront's sum of |D| over its cells of a block */
    rd_acq_pmax *pmax;                                          /* device [B][max_hops][RD_ACQ_NPART]: a wavefront's best cell of a hop */
    rd_acq_rec *rec;                                            /* device [B][max_hops] */
    void *dt; long long t0; int n_rows;                         /* complex64 [B][n_rows][40] or NULL: D[t0 .. t0 + n_rows) */
    int B, max_hops;                                            /* max_hops: the most hops any stream of the call has */
} rd_acq_args;
int rd_launch_acq_detect(const rd_acq_args *a, rd_stream_t s);
typedef struct { long long t_abs; double fmax; int stream, pad; } rd_acq_ev;
typedef struct { long long t; double f, Dmax; } rd_acq_fine;
typedef struct {
    const rd_tables *tab;                                       /* p */
    const void *x; long x_stride;
    const int *n;                                               /* device [B] */
    const rd_acq_ev *ev;                                        /* device [n_events] */
    rd_acq_fine *out;                                           /* device [n_events] */
    double *dfine;                                              /* device [n_events][RD_ACQ_NFINE]: |Dt1| of the winning timing */
    int n_events;
} rd_acq_refine_args;
int rd_launch_acq_refine(const rd_acq_refine_args *a, rd_stream_t s);

/* the whole-file band-pass of the stored-file receiver, rade_batch_bpf_file (rade_file.hip; include/rade_batch.h states the arithmetic).
 * k_file_phase + k_file_bpf: complex_bpf.bpf of a whole file; a workgroup of four wavefronts takes RD_FILE_SPAN consecutive outputs of one stream, RD_FILE_CHUNK at a
 * time (one 256-output tile of rade_bpf_fir.h per wavefront).  The demodulator and the BER alignment behind it: rd_file_rx_args, rd_file_ber_args above. */
#define RD_FILE_CHUNK 1024
#define RD_FILE_NCHUNK 8
#define RD_FILE_SPAN (RD_FILE_CHUNK * RD_FILE_NCHUNK)
typedef struct {
    const unsigned short *bpf16;                                /* rd_bpf16_table_fill(): the taps as matrix-core operands */
    const void *x; long x_stride; void *y; long y_stride;       /* complex64, stream b at + b * stride samples */
    const int *n;                                               /* device [B] sample counts */
    float *phase; long n_phase;                                 /* device [n_phase][2], n_phase = max_n rounded up to RD_FILE_SPAN: made by k_file_phase, read by k_file_bpf */
    double alpha;                                               /* the mixer's step (rd_tables_fill: the float32 value, as a double) */
    int B, max_n;
} rd_file_bpf_args;
int rd_launch_file_bpf(const rd_file_bpf_args *a, rd_stream_t s);

typedef struct {
    const rd_tables *tab; const void *tx; long tx_stride; void *rx; long rx_stride;
    const void *G; const void *noise; const float *eoo; void *scratch; /* >= B * (1 + max(64, n_sig / 960)) * 2 doubles: [B][4] floats (gain, final phase), then the partial power sums */
    const void *mp;                    /* optional [B][n_sig] c64: the multipath output k_ofdm_mod_mp left (scratch then holds its n_sig / 960 per-frame power sums per stream) */
    int B, n_sig, n_pre, n_post, with_eoo; float sigma, freq_offset, df_dt; unsigned long long seed;
    float sine_amp, sine_freq, rx_gain;
    const float *ps;                   /* optional [3][B]: sigma, freq_offset, df_dt of every stream (rade_channel_streams), read in place of the three scalars */
} rd_chan_args;
int rd_launch_channel(const rd_chan_args *a, rd_stream_t s);
/* Doppler-spread generator: taps_dev [n_taps] f32, noise optional, G [B][n_out][2] c64 */
int rd_launch_multipath_gen(const float *taps_dev, int n_taps, int low_ratio, int n_out, const void *noise_low, unsigned long long seed, void *G, void *ybuf, int B, rd_stream_t s);
int rd_multipath_gen_needs_scratch(int low_ratio, int n_out);
/* the noise generator's primitives on chosen words (k_noise_probe; tests only): words[i] = Philox4x32-10(ctr[i], (k0, k1)), g[j] = gauss_pair(u[j]); u NULL: pair j is
 * words 2 (j & 1), 2 (j & 1) + 1 of counter j >> 1, m <= 2 n.  All pointers device memory, 4-byte aligned (g: 8) */
int rd_launch_noise_probe(const uint32_t *ctr /*[n][4]*/, uint32_t k0, uint32_t k1, const uint32_t *u /*[m][2] or NULL*/, uint32_t *words /*[n][4]*/,
                          float *g /*[m][2]*/, int n, int m, rd_stream_t s);
int rd_launch_multipath_h(const void *G, int n_g, int M, int n_sym, int Nc, float dRs, int want_complex, float *H, int B, rd_stream_t s);

/* the channel and the Doppler generator in pieces, rade_batch_channel_piece / rade_batch_multipath_piece (rade_chanp.hip; include/rade_batch.h states the arithmetic):
 * every output is a pure function of its absolute sample index, no device state.  k_dopp_piece: one workgroup per (tile of RD_DOPP_TILE outputs, stream), the tile's
 * draws and its low-rate FIR outputs in LDS; k_chan_piece: two samples (one Philox counter) per thread. */
#define RD_DOPP_TILE 1024                                        /* outputs of a generator tile */
#define RD_DOPP_NTAPS_MAX 256
typedef struct { long long n0; int n_out, pad; } rd_dopp_stream;              /* absolute index of the first output, count */
typedef struct {
    const float *taps; int n_taps, low_ratio;                   /* device [n_taps] */
    double hf_gain; unsigned long long seed;
    void *G; long g_stride;                                     /* complex64 pairs (G1, G2): stream b at + b * g_stride pairs */
    const rd_dopp_stream *ps;                                   /* device [B] */
    int B, max_out;
} rd_dopp_args;
int rd_launch_dopp_piece(const rd_dopp_args *a, rd_stream_t s);
typedef struct {
    long long n0, in_base, g_base;                              /* absolute index of the first output, of tx[b][0], of G[b][0] */
    unsigned long long f0q, dq;                                 /* (uint64) llrint(turns per sample 2^64) (rade_stages.c: piece_turns), (uint64) llrint(df_dt / 8000^2 2^64) */
    int n_in, n_g, n_out, rotate;                               /* rotate: f0 != 0 or df_dt != 0 */
    float sigma, gain;
} rd_chanp_stream;
typedef struct {
    const void *tx; long tx_stride;                             /* complex64 */
    const void *G; long g_stride;                               /* complex64 pairs or NULL */
    const void *noise; long noise_stride;                       /* complex64 [B][noise_stride] unit noise or NULL */
    void *rx; long rx_stride;                                   /* complex64 */
    const rd_chanp_stream *ps;                                  /* device [B] */
    unsigned long long seed;                                    /* generated noise when noise is NULL and seed != 0 */
    float sine_amp, sine_freq, rx_gain;
    int noise_mode, B, max_out;                                 /* RADE_CHANP_NOISE_COMPLEX / _REAL = 0, 1 */
} rd_chanp_args;
int rd_launch_chan_piece(const rd_chanp_args *a, rd_stream_t s);

/* CoreDecoderStatefull.forward (radae_base.py:388-430) for the pending rows of one stream, run inside the receiver
 * kernel by the stream's own workgroup (rx2_decode_pending -> dq2_layers): buffers and weights of that stage. */
typedef struct { const float *wp, *bias; const unsigned short *wp16, *wa16; const float *wscale; int N, K; } rd_lin;
/* wp16: rd_pack_weights_f16x2; wa16 (in-kernel decoder): rd_pack_weights_q16_a16 when wscale != NULL (int8-exact layer: one plane of
 * integers + per-column scales), else rd_pack_weights_f16x2_a16 (two planes) */
typedef struct {
    const float *z; long z_sb;                 /* [B][.][80] latent rows */
    float *x; long x_sb;                       /* [B][1 + Tcap][736]; x points at row 0 of stream 0, row -1 = conv history (the in-kernel stage keeps every other row in LDS) */
    float *gi; long gi_sb;                     /* [B][.][288] */
    float *hbuf; long hb_sb;                   /* [B][.][96] */
    float *h[5];                               /* GRU states [B][96] */
    float *out; long out_sb; int out_w;        /* [B][.][84] */
    rd_lin dense1, gin[5], glu[5], conv[5], output;
    const float *whh[5], *bhh[5];
    const unsigned short *whq[5]; const float *whs[5];   /* W_hh as int8-exact A-operand fragments (rd_pack_weights_q16_a16) + row scales, or NULL: k_rx_sync2 runs the recurrence on the matrix cores (dq2_scan_mfma) */
    int B;
} rd_decs_args;

typedef struct {
    const rd_tables *tab; rd_rx_stream *st; rd_rx_round *round;
    const void *rx; long rx_stride; const int *avail;   /* [B] samples readable at rx + b*stride (raw input: the receiver only reads it to rebuild the filter memory) */
    void *rxf; long rxf_stride;                          /* band-pass filtered samples of the invocation (k_bpf_fir), same indexing as rx */
    const unsigned short *bpf16;                         /* rd_bpf16_table_fill(): [4][2][64][8] binary16, the band-pass taps as matrix-core A operands */
    const void *bpf_chain; int chain_stride;             /* [B][chain_stride] float2: (nin0, mem_len0) + the block phases of the pre-pass */
    int *acc;                                            /* [B][4] this invocation: consumed, calls, valid, eoo */
    int max_calls;                                       /* call budget per stream per invocation */
    int unsync_off_after;                                /* radae_rxe.py:277-281: synced_count beyond which the unsync paths are disabled; < 0 = never */
    int round_calls, dec_rows;                           /* R calls per stream per launch (<= RD_RX_ROUND_MAX), 3R decoder slots */
    rd_decs_args dec;                                    /* the decoder runs inside the stream's workgroup (rx2_decode_pending) */
    float *features_out; long feat_stride;               /* [B][cap][432] */
    int feat_cap;                                        /* valid modem frames features_out holds per stream: a stream stops making calls once it has produced that many */
    int bypass_dec;                                      /* radae_rxe.py --bypass_dec (:300-302, :315): rows of features_out are the 240 latents of a valid modem frame, no decoder, no UW accounting */
    const unsigned short *corrq16, *corra16;             /* rd_corrq16_table_fill() [2][10][2][64][8] / rd_corra16_table_fill() [5][2][64][8]: the two-stage pilot correlator */
    float *zrows;                                        /* [B][dec_rows][80] */
    float *dtcache;                                      /* [B][960][40] |Dt2| surface of the previous detect_pilots call */
    int *status;                                         /* [B][4]: nin, sync, snr_int, state */
    float *eoo_out;                                      /* [B][180] or NULL */
    rd_rx_trace *trace; float *trace_z; int trace_cap;   /* optional */
    int *progress;                                       /* [4]: calls made by this launch, unused x3 */
    long long *wg_cycles;                                /* [B] shader-clock cycles each stream's workgroup spent in the launch (or NULL) */
    const unsigned short *wfwd16;                        /* [2][10][2][64][8] binary16: the forward DFT matrix (wr, -wi rows) as matrix-core A operands (rd_wfwd16_table_fill; k_rx_sync2's demodulator) */
    const double *vm;                                    /* [8][160] ((n - 79.5) / 80)^m: refine()'s moment powers (k_rx_sync2 reads them from L2) */
    int variant;                                         /* bits 8..: phase mask of the -DRX2_CENSUS developer build (tools/rx2_census.sh); 0 otherwise */
    int lds_bytes;                                       /* dynamic LDS of the launch: what rd_rx_sync_prepare() returned */
    int B;
} rd_sync_args;
int rd_launch_rx_sync(const rd_sync_args *a, rd_stream_t s);
/* once per device before the first launch (rade_batch_open): raises the kernel's dynamic-LDS limit; returns the bytes to launch with, < 0 on error */
int rd_rx_sync_prepare(void);

/* complex_bpf.bpf (dsp.py:63-102) over n samples of every stream in one pass (rade_rx.hip: k_bpf_chain + k_bpf_fir [+ k_bpf_advance]): the receiver's
 * input filter ahead of the receiver launches of an invocation, and the transmitter's optional output filter (radae_txe.py:74-83).  Streams are cut into
 * blocks as the reference cuts them into calls: the first block len0 samples, every later one 960.
 * Contract (tests/test_bpf_units_gpu.py): stream b's y[0, avail) is written, whole blocks and a partial last one alike, and nothing else of y; x is read inside [0, avail)
 * only.  1 <= len0 <= 1152; a stream with len0 <= 0 or avail <= 0 writes nothing.  chain[b][0] = (len0, mem_len) as integer bits, chain[b][1 + k] = the phase block k
 * starts from, up to and including the first block beyond the input (every block steps the phase by its WHOLE length, a partial last one too); nothing behind that
 * and nothing at or past chain_stride is written.  grid_off is cleared for every stream.  advance = 0: nothing else of the state record is written.  advance = 1:
 * mem <- the last 102 baseband samples of [0, avail), phase <- the chain's entry behind the last block, mem_len <- 102 -- what complex_bpf holds after these calls when
 * the last block is whole; with avail < 102 or len0 <= 0 the record stays as it was (the reference would shift such a call into its memory: no caller makes one).
 * One invocation over n blocks and n invocations over one block each, advance = 1, give the same bits in y and in the record. */
typedef struct {
    rd_bpf_state *state; long state_stride;      /* record of stream b at (char *)state + b * state_stride */
    const int *len0; long len0_stride;           /* first block length of stream b at (char *)len0 + b * len0_stride (the receiver: its nin), or NULL: len0_const */
    int len0_const;
    const int *avail; int avail_const;           /* samples of stream b: device array, or NULL: avail_const for every stream */
    const rd_tables *tab; const unsigned short *bpf16;   /* rd_bpf16_table_fill(): the taps as matrix-core operands */
    const void *x; long x_stride; void *y; long y_stride;   /* complex64 in / out, stream b at + b * stride (samples); must not overlap */
    void *chain; int chain_stride;               /* [B][chain_stride] float2 scratch, chain_stride >= n_blocks + 3: (len0, mem_len) + the block phases */
    int n_blocks;                                /* blocks of the longest stream */
    int B;
    int clip;                                    /* 1: magnitude limited to 1 after the filter (radae_txe.py:132) */
    int advance;                                 /* 1: every sample is consumed -- leave the state complex_bpf would hold (the receiver kernel does that itself, by what it consumed) */
    int *zero_acc, *zero_progress;               /* optional: [B][4] / [4] ints that k_bpf_chain clears on its way (the receiver's per-invocation counters: two memsets less in the stream) */
} rd_bpf_args;
int rd_launch_bpf(const rd_bpf_args *a, rd_stream_t s);
/* start-of-utterance state of every stream in ONE launch (one workgroup per stream): the receiver record (radae_rxe.py:128-142) when st != NULL, and any of
 * the GRU states [5][B][H] / conv history rows that are given (NULL = leave alone) */
typedef struct {
    rd_rx_stream *st; const unsigned *seeds; double foff_err;
    float *dec_h; float *dec_x; long dec_x_sb;      /* [5][B][96]; history row of stream b at dec_x + b * dec_x_sb, RD_DEC_W floats */
    float *enc_h; float *enc_x; long enc_x_sb;      /* [5][B][64]; the two history rows of stream b at enc_x + b * enc_x_sb, 2 * RD_ENC_W floats */
    int B;
} rd_reset_args;
int rd_launch_reset(const rd_reset_args *a, rd_stream_t s);

/* ---- one core encoder / decoder step of ONE stream as one launch (rade_core_step.hip; include/rade_core.h) ----
 * A layer = row-major W[N][K] (K a multiple of 8, zero padded): wq != NULL: ONE binary16 plane of the integers q of an int8 layer
 * (w = q * scale[n], exact); else float32 wf (scale NULL). */
typedef struct { const unsigned short *wq; const float *wf; const float *scale; const float *bias; int N, K; } rd_mv;
typedef struct {
    rd_mv dense1, gin[5], ghh[5], glu[5], conv[5], out;
    int is_enc, n_in, n_out;           /* floats in / out per step (80 or 84 features, 80 latents) */
    int W, H, in0, conv_out;           /* concat width 864 / 736, GRU width 64 / 96, dense1 outputs 64 / 96, conv outputs 96 / 32 */
    int dil[5];                        /* conv dilation (1 or 2): tap 0 reads row t - dil */
    float *hist;                       /* [2][W]: concat rows t-1, t-2 of the previous steps */
    float *h;                          /* [5][H] GRU states */
    const float *in; float *out_vec;   /* device-visible buffers (pinned host memory in rade_core.c) */
    unsigned *done; unsigned seq;      /* optional completion word (device-visible host memory): set to seq after out_vec is written */
    const rd_tables *tab; float *iq_out;   /* rd_launch_tx_frame only: the constant tables and the 960 complex output samples (device-visible) */
} rd_core_args;
int rd_launch_core_step(const rd_core_args *a, rd_stream_t s);
/* a whole modem frame of the transmitter in one launch: in = 3 x n_in packed feature rows -> three encoder steps -> OFDM modulator -> iq_out[960] */
int rd_launch_tx_frame(const rd_core_args *a_dev /* the record in DEVICE memory */, unsigned seq, rd_stream_t s);


#ifdef __cplusplus
}
#endif
#endif
