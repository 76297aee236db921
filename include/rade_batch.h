/*
 * rade_batch.h -- batched (many independent streams) form of the RADE hot path, C ABI.
 *
 * Additive extension of rade_api.h: the single-stream API cannot express "256 utterances on one
 * MI355X", which is the workload BASELINE.json names.  Every call processes the same step for all
 * B streams; streams never exchange data, so sharding across GPUs is one
 * engine per device with a disjoint set of streams.
 *
 * All *_dev pointers are device (HBM) addresses; `stream` is a hipStream_t passed as void*
 * (NULL = the legacy default stream).  No torch / C++ types cross this boundary.
 *
 * Reference behaviour implemented per entry point:
 *   rade_batch_tx          radae_txe.py:108-135 (do_radae_tx) + rade_api.c:403-445, n_mf modem frames at once,
 *                          encoder state carried across calls (radae_base.py:97-129)
 *   rade_batch_tx_eoo      radae_txe.py:138-144, radae.py:208-219, :441-455
 *   rade_batch_channel     radae.py:529-589 (rate-Fs multipath, offsets, AWGN; power normalised per
 *                          stream = the reference's batch-1 behaviour) + inference.py:263-284 (EOO / noise framing)
 *   rade_batch_rx          radae_rxe.py:171-330 (do_radae_rx) looped like radae_rxe.py:349-356 /
 *                          src/radae_rx.c:42-53, incl. rade_api.c:480-513 decoder + UW accounting
 *   rade_batch_rx_ideal    radae.py:312-420, :590-657 (the ideal-timing receiver of RADAE.forward / RADAE.receiver, ber_test)
 *   rade_batch_channel_rs_pa  radae.py:603-634 with bottleneck 3 (the rate-Rs "hybrid time & frequency domain" channel: IDFT, PA limiter, DFT, |H|, AWGN) +
 *                          inference.py:213-229 (its Eq / PAPR measurements)
 *   rade_batch_resample    dsp.py:564-575 (sample_clock_offset, the linear mode) and what the ctests radae_rx_dfs / radae_rx_slip_* do with `sox -r 8000 .. -r 8020`:
 *                          the receiver's sound card running at another rate than the transmitter's, per stream
 *   rade_batch_wire_in     int16tof32.py:40-50 (with --zeropad: a real channel becomes IQ with Q = 0), what every streaming ctest puts in front of the receiver
 *   rade_batch_wire_out    f32toint16.py:42-54 (--real --scale 8192 feeds the radio), with saturation and level meters
 *   rade_batch_rate_convert  the `sox .. -r 8000` stage in front of int16tof32.py in every off-air and sound-card pipeline (radae_rx.sh:33,39, README.md:570, evaluate.sh:119,
 *                          analog_bbfm.sh:37,43): 48 or 44.1 kHz <-> the modem's 8 kHz, a polyphase L / M converter whose anti-alias filter scales with the ratio
 *   rade_batch_fm_mod      fm.m:74-94 (analog_fm_mod) with the noise of fm.m:171 / :316-322: the analog-FM baseline every BBFM result is compared with (analog_bbfm.sh:37-43)
 *   rade_batch_fm_demod    fm.m:97-126 (analog_fm_demod): mix, input filter, discriminator, output filter (de-emphasis folded into it)
 *   rade_batch_cno_est     est_CNo.py:23-73 as ota_test.sh:136-148 (process_rx) runs it over the first 10 s of every stored off-air file: the C/No of the 400-2000 Hz chirp
 *                          header and the time at which it starts; rade_chirp: chirp.py:50-65, the header itself
 *   rade_batch_snr_trials  est_snr.py:45-124 with receiver_one.est_pilots (dsp.py:418-435): the trials of the pilot SNR estimator behind the receiver's correction
 *                          constants, every set point of every channel in one call; rade_snr_finish / _fit / _track: the script's formulas, its np.polyfit, dsp.py:438-456
 *   rade_batch_specgram    plot_specgram.m:6-16 as ota_test.sh:130-134 and evaluate.sh:112, :153 draw it: the spectrogram of every recording, |X| of a 1280-sample Hann
 *                          window every 160 samples, normalised by the recording's maximum, as 256 grey levels
 *   rade_batch_psd         radae_plots.m:53 (do_plots): the Welch power spectrum of every stream; rade_batch_sigstat :62-69: mean power, PAPR and the pilot symbol's
 *                          PAPR; rade_psd_bandwidth :100-116: the 99 % power bandwidth
 */
#ifndef RADE_BATCH_H
#define RADE_BATCH_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rade_batch rade_batch;
#define RADE_BATCH_BOTTLENECK1 0x100
/* Accepted and ignored since round 4: the receiver kernel (k_rx_sync2: 256 threads and at most 80 KB of LDS per stream, so that the
 * workgroups of two launches share a CU) is the only one; rounds 2-3 selected it with this flag beside a one-stream-per-CU kernel. */
#define RADE_BATCH_RX_TWO_PER_CU 0x200

/* Tx band-pass filter + magnitude clip on every transmitted frame and the end-of-over frame: radae_tx(..., txbpf_en=True) / `radae_tx.py --txbpf`
 * (radae_txe.py:74-83, :130-132, :141-143; ctest radae_tx_basic).  Off by default, as in the reference. */
#define RADE_BATCH_TX_BPF 0x400

/* Receiver without the core decoder: `radae_rxe.py --bypass_dec` (radae_rxe.py:67, :113-123, :300-302, :315), the mode the reference's rade_api.c drives when an
 * external C decoder follows (rade_api.c:491-513).  Every valid modem frame appends its 240 equalised latents (3 x 80, what receiver_one returned) to
 * features_out instead of 432 feature floats -- rows are 240 floats, feat_stride / 240 is the capacity -- and, as in the reference, the aux-bit (UW) errors are
 * never summed in this mode (sum_uw_errors sits behind the decoder), so a UW failure cannot end sync; everything else of do_radae_rx is unchanged. */
#define RADE_BATCH_BYPASS_DEC 0x800

/* The bottleneck-1 rate-Fs waveform (model05 numerology, radae.py:195-199, :545-548): rade_batch_tx, rade_batch_tx_latents and rade_batch_tx_channel send the pilots at
 * unit gain and skip the tanh limiter, and rade_batch_rx_ideal scales coarse_mag without the bottleneck-3 factor.  Paths that cannot honour it fail instead of limiting:
 * rade_batch_open with RADE_BATCH_TX_BPF, rade_open (rade_api.h: single-stream frame kernels), rade_batch_tx_eoo and rade_batch_channel with_eoo.
 * Noise for this waveform: rade_sigma_from_EbNodB_bn1. */
#define RADE_BATCH_TX_LINEAR 0x1000

typedef struct {
    int n_streams;        /* B */
    int max_tx_mf;        /* largest n_mf a single rade_batch_tx call may carry */
    int device;           /* HIP device ordinal */
    int flags;            /* RADE_FOFF_TEST from rade_api.h is honoured; RADE_BATCH_BOTTLENECK1: z = tanh(.) (model05, bbfm); RADE_BATCH_TX_BPF; RADE_BATCH_BYPASS_DEC; RADE_BATCH_TX_LINEAR */
    int rx_trace_calls;   /* >0: keep a per-call trace of this many do_radae_rx calls per stream (tests) */
    float disable_unsync; /* test mode of radae_rxe.py --disable_unsync (:277-281, :337): after this many seconds in sync the receiver no longer
                           * drops back to search (pilot loss, end-of-over, UW failure); 0 = normal operation */
} rade_batch_config;

/* blob = DNNw weight file (weights/model19_check3.bin).  Returns NULL on failure (message on stderr). */
rade_batch *rade_batch_open(const char *blob_path, const rade_batch_config *cfg);
rade_batch *rade_batch_open_mem(const void *blob, size_t blob_len, const rade_batch_config *cfg);
void rade_batch_close(rade_batch *h);
int rade_batch_n_streams(const rade_batch *h);

/* ---- Buffers, strides and alignment (pinned by tests/test_buffer_contract_gpu.py) ------------------------------------------------------------------------------
 * Strides are counted in ELEMENTS of the buffer they belong to: complex64 samples for iq_stride, tx_stride, rx_stride (rade_batch_* and rade_sc_*), floats for
 * feat_stride, f_stride / f_row, h_stride / h_row and fl_stride.  Stream b's row starts at base + b * stride; stride >= the row length of the call is all a stride
 * has to satisfy (no multiple of anything; an odd stride is fine) unless an entry below says more.  Buffers without a stride argument are dense:
 * [B][rows of this call][width], whatever the engine's capacity (max_tx_mf) is.
 * Writes: a call writes the row [b * stride, b * stride + row) of each output it documents and NOTHING else of the caller's memory -- not the gap up to the next
 * row, not a byte before row 0 or behind the last row, and never an input buffer.  Inside a row it writes exactly the documented extent: n_total samples of
 * rx_out, n_valid * 432 (240) floats of features_out, n_hat - start floats of a scored stream's frame_loss row; the rest of the row keeps what it held.
 * Alignment: every pointer is aligned to its ELEMENT (4 bytes for float buffers, 8 bytes for complex64 buffers, G_dev and noise_low_dev included), and that is
 * enough -- base pointers at odd element offsets are fine -- except for the four buffers that kernels access as 16-byte words.  Those must be 16-byte aligned,
 * and the entry returns -1 on the host, before any launch and with nothing written, when they are not:
 *     rade_batch_tx, rade_batch_encode          z_out_dev     (rade_enc.hip stores the latents of a call of more than 16384 rows as f32x4; refused for every size)
 *     rade_batch_decode                         z_dev         (the GEMMs read their A rows as f32x4, and the first layer's rows are the caller's)
 *     rade_batch_rx_ideal                       z_hat_dev     when features_out_dev is given (the decoder then reads it like rade_batch_decode's z_dev)
 *     rade_batch_tx_channel(_streams)           p->G_dev      (the fused modulator reads (G1[i], G2[i]) as one 16-byte word; rade_batch_channel reads it by element: 8 bytes)
 * Rows of these buffers are 320 (z) or 16 (G) bytes, so an aligned base aligns every stream.  Handled inside the kernel instead: rx_out_dev of the channel calls
 * (k_chan_apply stores two samples as one 16-byte word where the stream's row allows it, else as two 8-byte words; any rx_stride, n_pre, n_total parity).
 * Host arrays ([B] ints, floats, doubles, longs, status records) are read or written for exactly B entries.
 * Per entry, buffer (element; stride) -- all natural alignment unless listed above:
 *   rade_batch_tx / _tx_latents / _tx_eoo   features_dev, z_dev (float; dense) in; iq_out_dev (complex64; iq_stride >= 960 n_mf, 1152 for _tx_eoo), z_out_dev (float; dense, 16 B)
 *   rade_batch_encode / _decode             features / z in (float; dense; _decode's z_dev 16 B); z_out_dev (16 B) / features_out_dev (float; dense)
 *   rade_batch_channel(_streams)            tx_dev (complex64; tx_stride >= n_sig), G_dev [B][n_sig][2], noise_dev [B][n_total] (complex64; dense) in; rx_out_dev (complex64; rx_stride >= n_total)
 *   rade_batch_tx_channel(_streams)         as the two above; iq_out_dev optional with G_dev (16 B)
 *   rade_batch_channel_symbol               z_dev, H_dev, noise_dev in, z_hat_dev out (float; dense)
 *   rade_batch_channel_rs_pa                z_dev [B][n_steps][80], H_dev [B][2 n_steps][20] (float; dense), noise_dev [B][2 n_steps][20] (complex64; dense) in; z_hat_dev
 *                                           [B][n_steps][80] (float; dense).  Element alignment suffices for all four (the kernel reads and writes z, H, z_hat by float,
 *                                           noise by complex64); a pointer that is not even that returns -1 before any launch
 *   rade_batch_multipath_gen / _h           noise_low_dev, G_dev in (complex64; dense); G_out_dev (complex64 [B][n_out][2], n_out >= 1; one sample has no variance to
 *                                           normalise by: n_out = 1 writes its two values, not finite), H_out_dev (float; dense)
 *   rade_batch_rx                           rx_dev (complex64; rx_stride >= every n_avail) in; features_out_dev (float; feat_stride >= 432 or 240, capacity = the floor of
 *                                           feat_stride / that), eoo_out_dev (float [B][180], written only for a stream with has_eoo)
 *   rade_batch_rx_ideal                     rx_dev (complex64; rx_stride >= 960 n_mf, checked), z_ref_dev in; z_hat_dev (16 B with features_out_dev), features_out_dev (float; dense)
 *   rade_batch_loss                         features_dev (float; f_stride >= n_in f_row), hat_dev (float; h_stride >= n_hat h_row) in; frame_loss_dev (float; fl_stride >= n_hat, checked)
 *   rade_batch_resample                     x_dev (complex64; x_stride >= every n_in, checked) in; y_dev (complex64; y_stride >= every n_out, checked): n_out[b] samples of row b are written,
 *                                           8 bytes at a time (any y_stride, any parity of n_out, element alignment); x is read inside [b x_stride, b x_stride + n_in[b]) only
 *   rade_batch_wire_in                      in_dev (int16; in_stride >= n or 2 n int16, checked; 2-byte alignment) in; out_dev (complex64; out_stride >= n, checked): n[b] samples of row b
 *   rade_batch_wire_out                     x_dev (complex64; x_stride >= n, checked) in; out_dev (int16; out_stride >= n or 2 n int16, checked; 2-byte alignment): n[b] samples of row b.
 *                                           Both move 16-byte words where the int16 row crosses 16-byte boundaries and single elements in front of the first and behind the
 *                                           last (rade_wire.hip): any stride, any count, element alignment
 *   rade_batch_rate_convert                 x_dev (complex64, or int16 with one or two elements per sample; x_stride >= n_in, 2 n_in for int16 IQ, in elements of x, checked; 8- or
 *                                           2-byte alignment) in; y_dev (complex64; y_stride >= every n_out, checked): n_out[b] samples of row b are written, 8 bytes at a time (any
 *                                           y_stride, any parity of n_out, element alignment); x is read inside the n_in[b] samples of row b only
 *   rade_batch_fm_mod                       m_dev (float32 or complex64; m_stride >= n, checked; 4- or 8-byte alignment) in; y_dev (complex64; y_stride >= n, checked): n[b]
 *                                           samples of row b are written, 8 bytes at a time; p->noise_dev (complex64) is dense [B][max n]
 *   rade_batch_fm_demod                     x_dev (complex64; x_stride >= n_in, checked) in; y_dev (float32 or complex64; y_stride >= n_out, checked; 4- or 8-byte alignment)
 *                                           and p->bb_out_dev (complex64; bb_stride >= n_out, checked): n_out[b] samples of row b are written, one element at a time
 *   rade_batch_channel_piece                tx_dev (complex64; tx_stride >= every n_in, checked), p->G_dev (complex64 pairs; g_stride >= every n_g, checked) in, read inside the
 *                                           stream's n_in / n_g elements only; p->noise_dev (complex64) dense [B][max n_out]; rx_out_dev (complex64; rx_stride >= every n_out,
 *                                           checked): n_out[b] samples of row b are written, 16 bytes at a time where the row allows it, single samples at an odd head or tail
 *                                           (any rx_stride, any parity of n0 and n_out, element alignment)
 *   rade_batch_multipath_piece              G_out_dev (complex64 pairs; g_stride >= every n_out, checked; 8-byte alignment): n_out[b] pairs of row b are written
 *   rade_batch_cno_est                      x_dev (complex64; x_stride >= every n, checked) in, read inside the n[b] samples of row b only and never written; the results go to
 *                                           host memory
 *   rade_batch_snr_trials                   p->H_dev (complex64; h_stride >= the rows a stream reads x 30, checked), p->noise_dev (complex64; noise_stride >= n_windows Nw 30,
 *                                           checked) in, never written; p->noise_out_dev (complex64; the same noise_stride): the n_windows Nw 30 elements of row b are written,
 *                                           8 bytes at a time; the sums go to host memory
 *   rade_batch_specgram                     x_dev (complex64 or int16; x_stride >= every n, checked) in, read inside the n[b] samples of row b only; img_dev (bytes; img_stride
 *                                           >= n_slices n_bins, checked; any alignment) and mag_dev (float; mag_stride >= 1023 n_slices, checked): a stream's own rows only
 *   rade_batch_psd / rade_batch_sigstat     x_dev (complex64 or int16; x_stride >= every n, checked) in, read inside the n[b] samples of row b only; psd_dev (float;
 *                                           psd_stride >= 1024, checked): the 1024 floats of row b; rade_batch_sigstat's results go to host memory
 *   rade_sc_tx / rade_sc_rx                 symbs_dev (float; dense), rx_dev (complex64; rx_stride >= n_avail, checked) in; iq_out_dev (complex64; iq_stride >= 384 n_frames, checked),
 *                                           payload / zhat / frames [B][max_frames][..] dense: frames past status.n_frames are not written */

/* Arithmetic of the encoder depends on the SIZE of the call, in the last bits only: calls with more than 16384 rows (B x 3 n_mf) run the batched kernels on operand
 * fragments (rade_enc.hip), whose two conv taps alternate per k-block -- another summation order of the same float32 partial products than the float32-row kernels that
 * serve smaller calls ($RADE_ENCF_SEQ_TAPS restores the sequential order, $RADE_ENC_ROWS the row kernels for every size).  Both are inside every parity bar (latents
 * < 2e-5 of full scale against the float32 oracle, tests/test_hip_parity.py), but the same stream encoded in a batch of 32 and in a batch of 256 is not bit-identical.
 * The batched path also keeps one bit of HOST state per engine (whether the history tile of its fragment buffer is current): rade_batch_tx / rade_batch_encode are
 * stream-ordered but not capturable into a hipGraph that is replayed across resets or mixed with short calls (rade_tx() of rade_api.h, which IS captured on a handle
 * opened with the Tx band-pass filter, always takes the row path). */
/* ---- transmit ------------------------------------------------------------------------------
 * features_dev : [B][n_mf*12][36] float32 (first 20 of each 36 used; aux symbol -1 added inside)
 * iq_out_dev   : stream b written at iq_out_dev + b*iq_stride (units: complex samples), n_mf*960 samples
 * z_out_dev    : optional [B][n_mf*3][80] latents (NULL to skip)
 * returns n_mf*960 or <0 on error */
int rade_batch_tx(rade_batch *h, const float *features_dev, int n_mf, void *iq_out_dev, long iq_stride,
                  float *z_out_dev, void *stream);
/* `radae_txe.py --bypass_enc` (radae_txe.py:124-126; rade_api.c with RADE_USE_C_ENCODER): latents from an external core encoder, z_dev [B][3 n_mf][80] float32,
 * straight into the OFDM modulator (and the Tx band-pass filter when the engine has it).  The engine's own encoder state is not touched.  Returns n_mf * 960. */
int rade_batch_tx_latents(rade_batch *h, const float *z_dev, int n_mf, void *iq_out_dev, long iq_stride, void *stream);
/* bits_host: [B][180] +-1 floats, or NULL to restore the default (all-zero data symbols) EOO frame */
int rade_batch_tx_set_eoo_bits(rade_batch *h, const float *bits_host);
/* writes the 1152-sample end-of-over frame of every stream; returns 1152 */
int rade_batch_tx_eoo(rade_batch *h, void *iq_out_dev, long iq_stride, void *stream);
void rade_batch_tx_reset(rade_batch *h);

/* ---- core encoder / decoder alone ---------------------------------------------------------------
 * The rade_core_encoder / rade_core_decoder level (src/rade_core.h:42-46, test_rade_enc.c / test_rade_dec.c),
 * and what the non-OFDM configurations (inference.py rate-Rs, bbfm.py) run.  The feature width comes from
 * the blob: 4 x 21 (model19: caller supplies the aux symbol) or 4 x 20 (model05, bbfm).
 * features_dev: [B][n_steps][4*feat_dim] -> z_out_dev [B][n_steps][80]; state carried across calls
 * (rade_batch_tx_reset clears it).  rade_batch_decode: z [B][n_steps][80] -> features [B][n_steps][4*feat_dim]. */
int rade_batch_encode(rade_batch *h, const float *features_dev, int n_steps, float *z_out_dev, void *stream);
int rade_batch_decode(rade_batch *h, const float *z_dev, int n_steps, float *features_out_dev, int reset_state, void *stream);
/* symbol-domain channels: mode 0 = rate-Rs AWGN/multipath magnitudes (radae.py:604-634; H_dev [B][n_steps*40] per
 * QPSK symbol or NULL, p0 = sigma); mode 1 = BBFM FM-demodulator SNR model (bbfm.py:157-197; H_dev [B][n_steps*80]
 * or NULL, p0 = CNRdB, p1 = Gfm dB).  noise_dev: [B][n_steps*80] float32 (already scaled per component) or NULL -> Philox(seed).
 * The generated draw runs over the WHOLE call, not per stream: real symbol i of the flat [B][n_steps][80] index takes counter (i >> 1, 0, 0, 0), words 0-1 only,
 * the first Gaussian for even i and the second for odd i (mode 0: times 1 / sqrt(2)).  So stream b continues where stream b - 1 ended, a stream's draw depends on B
 * and n_steps, and with one seed the call draws the words of stream 0 of the rate-Fs channel (third counter word 0 in both): give the two different seeds. */
int rade_batch_channel_symbol(rade_batch *h, const float *z_dev, const float *H_dev, const float *noise_dev, float *z_hat_dev, int n_steps,
                              int mode, float p0, float p1, unsigned long long seed, void *stream);

/* The rate-Rs channel of the bottleneck-3 model, RADAE.forward without rate_Fs (radae.py:603-634; what model19 was trained under, and what inference.py runs without
 * --rate_Fs).  Numerology of RADAE(..., bottleneck = 3) without pilots or cyclic prefix: Nc = 20 carriers at DFT bins 20..39, M = 160, Ns = 6 (the pilot numerology
 * does not run in the reference without rate_Fs and is not offered).  Latent row r of a stream (80 floats) is 40 QPSK symbols q[k] = z[2k] + j z[2k+1]; OFDM symbol
 * s = 2r + (k >= 20) takes carriers c = k mod 20, i.e. symbol s is floats [40 s, 40 s + 40) of the stream.  Per symbol:
 *     tx[m]  = (1/160) sum_c sym[c] e^{+j m w_c}, w_c = 2 pi (20 + c) / 160          tx'[m] = tanh(|tx[m]|) tx[m] / |tx[m]|   (0 -> exactly 0; any finite tx, however large -> magnitude 1)
 *     Y[c]   = sum_m tx'[m] e^{-j m w_c}                                             Y[c]  *= e^{j phase_offset} H[b][s][c]   (H real magnitudes; NULL = 1)
 *     R[c]   = Y[c] + sigma_b n[b][s][c]                                             z_hat[40 s + 2c], [40 s + 2c + 1] = Re R[c], Im R[c]
 * noise_dev: complex, unit variance in total (1/2 per component, torch.randn_like of a complex tensor), or NULL: generated, Philox4x32-10 keyed by (seed, stream) with
 *   one counter per pair of carriers (words 0-1 -> the even carrier, 2-3 -> the odd one), Box-Muller on the hardware units; seed 0 = no noise.  As for the rate-Fs
 *   channel the generated sequence is a property of the BUILD; a stream's draw does not depend on B; anything comparable across builds passes noise_dev.
 * sigma_streams_host: [B] or NULL = `sigma` for every stream.  Stream b gets what a call with the scalar set to its value gives it, bit for bit (the rule of
 *   rade_channel_streams); the values are copied to the device ahead of the launch (the call synchronises `stream` once for that).
 * stats_host: [B][3] doubles or NULL: sum |tx'|^2 and max |tx'| over the stream's 320 n_steps samples, sum |Y|^2 over its 40 n_steps symbols after phase and H -- what
 *   inference.py:215-227 measures (Eq = sum |Y|^2 / (40 n_steps), S = sum |tx'|^2 / (320 n_steps), PAPR = max^2 / S).  Sums are doubles added in a fixed order (no atomics):
 *   two identical calls give identical bits.  With stats_host the call synchronises `stream`.
 * Any n_steps >= 1, any engine (the model is not used; no encoder or receiver state is touched).  Returns n_steps or < 0.  Noise level: rade_sigma_from_EbNodB_rs3. */
int rade_batch_channel_rs_pa(rade_batch *h, const float *z_dev, const float *H_dev, const void *noise_dev, float *z_hat_dev, int n_steps, float sigma,
                             const float *sigma_streams_host, float phase_offset, unsigned long long seed, double *stats_host, void *stream);

/* ---- channel simulator ---------------------------------------------------------------------- */
typedef struct {
    int n_sig;            /* signal samples per stream (multiple of 960) */
    int n_pre, n_post;    /* noise-only samples before / after (inference.py --prepend_noise/--append_noise) */
    int with_eoo;         /* append the stream's EOO frame, phase-continued (inference.py --end_of_over).  On an engine with RADE_BATCH_TX_BPF the appended frame is the EOO
                           * through the Tx band-pass filter + clip, continuing from the filter state the transmitted frames left (radae_txe.py:138-144); the channel call
                           * only READS that state (calling it twice gives the same samples).  Do not call rade_batch_tx_eoo first: that advances the state past the EOO. */
    float sigma;          /* AWGN std-dev, see rade_sigma_from_EbNodB */
    float freq_offset;    /* Hz */
    float df_dt;          /* Hz/s */
    const void *G_dev;    /* [B][n_sig][2] complex64 Doppler samples (G1,G2) or NULL = (1,0) */
    const void *noise_dev;/* [B][n_total] complex64, unit variance, or NULL: generate (Philox) from seed; seed 0 = no noise.
                           * The generated sequence is a property of the BUILD, not of the seed alone: Philox4x32-10 keyed by (seed, stream) with one counter per
                           * PAIR of samples (words 0-1 -> sample 2p, 2-3 -> sample 2p + 1; round 3: one counter per sample), Box-Muller on the hardware
                           * log2 / sqrt / sin / cos units (round 4).  Seeded statistics are reproducible within a build; anything that must be comparable
                           * across builds (parity tests) passes noise_dev.
                           * Inside the signal and the EOO frame the generated sample is complex, sigma / sqrt(2) per component.  In n_pre and n_post it is REAL-valued:
                           * the full sigma on the real part (the pair's first Gaussian), imaginary part exactly 0 (inference.py:277-284 adds a real randn there).  An
                           * explicit noise_dev is added as complex, sigma x noise, everywhere.
                           * The generated draw, pinned sample by sample by tests/test_device_noise_gpu.py against tests/noise_ref.py: key (seed & 0xffffffff,
                           * seed >> 32); counter (p, b, 0, 0).  The third counter word names the consumer: 0 here and in rade_batch_channel_symbol, 1 in
                           * rade_batch_multipath_gen (counter (x, 2 b + path, 1, 0), words 0-1 -> complex low-rate sample x), 2 in rade_batch_channel_rs_pa (counter
                           * (i >> 1, b, 2, 0), i = 20 s + c).  Uniforms (float(u) + 0.5) 2^-32; (sqrt(-2 ln a) cos 2 pi q, sqrt(-2 ln a) sin 2 pi q). */
    unsigned long long seed;
    float sine_amp, sine_freq;   /* complex tone added over the whole output, inference.py:285-288 (--sine_amp/--sine_freq); 0 = none */
    float rx_gain;               /* final scale, inference.py:289 (--rx_gain); 0 is taken as 1 */
} rade_channel_params;
/* n_total = n_pre + n_sig + (with_eoo ? 1152 : 0) + n_post samples written per stream; returns n_total */
int rade_batch_channel(rade_batch *h, const void *tx_dev, long tx_stride, void *rx_out_dev, long rx_stride,
                       const rade_channel_params *p, void *stream);

/* transmit and channel in one pass (what RADAE.forward does, radae.py:529-589): features [B][12 n_mf][36] -> received samples, with
 * p->n_sig == 960 n_mf.  With p->G_dev the modulator applies the two-path model itself and leaves the power sums (no second pass over
 * tx and G); iq_out_dev (the clean transmit samples) is then optional.  Returns n_total like rade_batch_channel, or <0. */
int rade_batch_tx_channel(rade_batch *h, const float *features_dev, int n_mf, void *iq_out_dev, long iq_stride, void *rx_out_dev, long rx_stride,
                          const rade_channel_params *p, void *stream);

/* per-stream values of rade_channel_params: [B] host arrays; a NULL member = p's scalar for every stream.
 * Stream b of a call gives what a call with p->sigma, freq_offset, df_dt set to stream b's values gives for stream b, bit for bit (Philox noise is keyed by
 * (seed, stream)), so a loss-vs-Eb/No curve (points x channels x utterances) is one batch.  The values are copied to the device ahead of the launches (the call
 * synchronises `stream` once for that); rade_batch_channel / rade_batch_tx_channel are these calls with ps = NULL. */
typedef struct { const float *sigma, *freq_offset, *df_dt; } rade_channel_streams;
int rade_batch_channel_streams(rade_batch *h, const void *tx_dev, long tx_stride, void *rx_out_dev, long rx_stride,
                               const rade_channel_params *p, const rade_channel_streams *ps, void *stream);
int rade_batch_tx_channel_streams(rade_batch *h, const float *features_dev, int n_mf, void *iq_out_dev, long iq_stride,
                                  void *rx_out_dev, long rx_stride, const rade_channel_params *p, const rade_channel_streams *ps, void *stream);

/* ---- sample-clock offset: a fractional resampler, every stream in one launch (rade_clk.hip) -----------------------------------------------
 * Output n of stream b (absolute index, n0 <= n < n0 + n_out) is the input interpolated at pos(n) = t0 + n step input samples, step = 1 + ppm 1e-6 (dsp.py:574's
 * convention: ppm > 0 reads the input faster, fewer outputs per input).  Time base: Q32.32 integers made on the host in double and rounded once,
 *     step_q = llrint((1 + ppm 1e-6) 2^32)    t0_q = llrint(t0 2^32)    pos_q = t0_q + n step_q (signed 64 bit)    i = pos_q >> 32 (arithmetic)    mu = pos_q & 0xffffffff
 * so an output's position is a pure function of (t0, ppm, n): the call keeps no state on the device, and a stream resampled in pieces equals the stream resampled
 * whole, bit for bit, when every piece is handed the inputs its windows cover.  in_base is the absolute index of x[b][0]; input samples outside
 * [in_base, in_base + n_in) read as zero, at both ends and at negative indices, and nothing outside [b x_stride, b x_stride + n_in) is read.
 *   RADE_RESAMPLE_LINEAR  dsp.py:569-572: y = (1 - f) x[i] + f x[i + 1], f = mu 2^-32 rounded to float32.
 *   RADE_RESAMPLE_SINC32  32-tap Kaiser-windowed sinc, 256 phases, linear interpolation between neighbouring phases:
 *       p = mu >> 24    w = (mu & 0xffffff) 2^-24 (exact in float32)    c[j] = T[p][j] + w (T[p + 1][j] - T[p][j])    y = sum_{j = 0..31} c[j] x[i + j - 15]
 *     T [257][32] float32, made on the host in double (rade_resample_taps): T[p][j] = g(j - 15 - p / 256) / sum_j g(.), g(t) = sinc(t) I0(10 sqrt(1 - (t / 16)^2)) / I0(10)
 *     for |t| <= 16, else 0, sinc(t) = sin(pi t) / (pi t).  Every row sums to 1; row 0 is exactly the unit impulse at j = 15 and row 256 the one at j = 16, so ppm = 0 with
 *     an integer t0 is a bit-exact delay in both modes.  The terms are added in the order j = 0..31 into one float32 accumulator per component (fused multiply-adds).
 *     Worst error of the definition on unit tones |f| <= 2700 Hz at 8 kHz: 2e-5 (the modem's carriers: 700..2300 Hz).
 * ppm / t0 / n0 / in_base: [B] host arrays, or NULL = the scalar ppm, 0, 0, 0 for every stream.  Stream b of a call with arrays is what the call with its values as
 * scalars gives for it, bit for bit (the rule of rade_channel_streams).  The per-stream values are copied to the device in one record per stream ahead of the launch:
 * the call synchronises `stream` once for that.
 * Refused with -1 on the host, before any launch and with nothing written: NULL or misaligned (8 bytes) x_dev / y_dev, NULL counts or p, a negative count or n0, a
 * stride shorter than the row, an unknown mode, |ppm| > 50 000, |t0| > 2^29 or |in_base| > 2^62 (or not a number), (n0 + n_out) step_q past 2^62 (37 h at 8 kHz).
 * Returns 0.  Any engine (the model is not used; no encoder or receiver state is touched). */
enum { RADE_RESAMPLE_SINC32 = 0, RADE_RESAMPLE_LINEAR = 1 };
typedef struct {
    int mode;
    double ppm;  const double *ppm_host;          /* [B] or NULL = ppm for every stream */
    const double *t0_host;                        /* [B] position of output 0 in input samples (fractional, may be negative), NULL = 0 */
    const long long *n0_host;                     /* [B] index of the first output sample this call writes, NULL = 0 */
    const long long *in_base_host;                /* [B] absolute index of x[b][0], NULL = 0 */
} rade_resample_params;
int rade_batch_resample(rade_batch *h, const void *x_dev, long x_stride, const int *n_in_host, void *y_dev, long y_stride, const int *n_out_host,
                        const rade_resample_params *p, void *stream);
/* host only: the number of n >= 0 with pos(n) < in_end, i.e. the outputs whose centre tap lies inside an input of in_end samples (-1: ppm or t0 refused as above, or
 * that many outputs pass the 2^62 limit) */
long long rade_resample_count(long long in_end, double t0, double ppm);
/* host only, no handle, no GPU: the table T */
void rade_resample_taps(float *out /* [257][32] */);

/* ---- the sound-card wire: int16 samples in and out, every stream in one launch (rade_wire.hip) -------------------------------------------
 * Counts are in SAMPLES: stream b converts n_host[b] of them.  RADE_WIRE_REAL: one int16 per sample; RADE_WIRE_IQ: two (I, Q).  Strides of the int16 buffers are in int16
 * elements.  (int16tof32.py drops a trailing odd int16 of a FILE, a property of its 4-byte reads; radae_amd/wire.py keeps that, these calls have no such rule.)
 * rade_batch_wire_in: out = (gain (float)s, +0.0f) in real mode (`int16tof32.py --zeropad`), (gain (float)I, gain (float)Q) in IQ mode; one float32 multiply per component,
 *   so gain = 1 gives the bytes of the reference script.
 * rade_batch_wire_out: per written component v = x * scale (one float32 multiply, rounded once), then
 *       v is NaN -> 0        v >= 32768 -> 32767        v <= -32769 -> -32768        else (int16)v truncated toward zero (f32toint16.py:48-49; -32768.99 gives -32768: it fits)
 *   RADE_WIRE_REAL writes (and meters) the I component only (`f32toint16.py --real`), RADE_WIRE_IQ both.
 *   meters_host [B][4] doubles or NULL, per stream over its written components: [0] the largest |v| (before saturation, +inf included; what an operator sets the drive by),
 *   [1] sum of v^2 (each v^2 exact in double; RMS = sqrt([1] / components)), [2] components that saturated, [3] NaN components (counted, and in neither [0] nor [1]).
 *   The sums are added in a fixed order (fixed chunks per stream -- their number depends on B alone --, a tree inside a chunk, no atomics): two identical calls give
 *   identical bits, and a stream's meters do not depend on the other streams.  With meters_host the call synchronises `stream`; without it, it does not.
 * Neither call keeps state on the device: a call is a pure function of its arguments (the rule of rade_batch_resample).  The counts travel in one small copy ahead of the
 * launch, from one of eight staging records used in turn: a call waits for the call eight before it, not for its stream.
 * Refused with -1 on the host, before any launch and with nothing written: NULL or misaligned pointers (2 bytes for int16, 8 for complex64), NULL counts, a negative count,
 * a stride shorter than the row, an unknown mode, a gain or scale that is not finite.  Return 0.  Any engine (the model is not used; no encoder or receiver state is touched). */
enum { RADE_WIRE_REAL = 0, RADE_WIRE_IQ = 1 };
int rade_batch_wire_in (rade_batch *h, const void *in_dev, long in_stride, const int *n_host, int mode, float gain,
                        void *out_dev, long out_stride, void *stream);
int rade_batch_wire_out(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int mode, float scale,
                        void *out_dev, long out_stride, double *meters_host /* [B][4] or NULL */, void *stream);

/* ---- sample-rate conversion by a ratio L / M: 48 / 44.1 kHz <-> 8 kHz, every stream in one launch (rade_rate.hip) ---------------------------------------
 * Every stream of a call is converted by the same ratio L / M (L up, M down, both >= 1; 1 / 6: 48 k -> 8 k, 80 / 441: 44.1 k -> 8 k).  The host reduces L and M by their gcd;
 * everything below is about the reduced pair.
 * Time base: output n of a stream (absolute index, n0 <= n < n0 + n_out) sits at input position n M / L:
 *     i = floor(n M / L)    ph = (n M) mod L        64-bit integers, no rounding anywhere
 * so an output's position is a pure function of (L, M, n): the call keeps no state on the device, and a stream converted in pieces equals the stream converted whole, bit
 * for bit, when every piece is handed the inputs its windows cover.
 * Filter: K = ceil(M / L) (integer), W = max(1, M / L) (real), T = 32 K taps per phase, H = 16 K;
 *     t_j = j - (T / 2 - 1) - ph / L        g(t) = sinc(t / W) I0(10 sqrt(1 - (t / H)^2)) / I0(10) for |t| <= H, else 0        sinc(u) = sin(pi u) / (pi u)
 *     C[ph][j] = g(t_j) / sum_j g(t_j)      made on the host in double and rounded once to float32; layout [L][T] (rade_rate_taps)
 *   the Kaiser-windowed sinc of rade_batch_resample with its cut-off at the lower of the two Nyquist rates and its length stretched by the same factor.  For M <= L (W = 1)
 *   sin(pi t) is formed from the fraction ph / L alone, as rade_resample_taps forms it: row 0 is then exactly the unit impulse at j = 15, L = M = 1 is a bit-exact copy, and
 *   up-sampling reproduces x[k] at y[k L] bit for bit for finite non-zero samples; with L = M = 1 the table is row 0 of rade_resample_taps.  Every row sums to 1.
 *   Unit tones |f| <= 2700 Hz are reproduced within 2e-5 at every phase for 1/6, 6/1, 80/441, 441/80, 1/2, 2/3, and the prototype is below -95 dB from 0.6 x the lower of
 *   the two rates upward (tests/test_rate_host.py).
 * Sum: y[n] = sum_{j = 0..T-1} C[ph][j] x[i + j - (T / 2 - 1)], one float32 accumulator per component, fused multiply-adds in the order j = 0..T-1.  in_base is the
 *   absolute index of x[b][0]; samples outside [in_base, in_base + n_in) read as zero, at both ends and at negative indices, and nothing outside the stream's n_in samples
 *   is read.
 * Input format: RADE_RATE_C64 complex64; RADE_RATE_S16_REAL one int16 per sample; RADE_RATE_S16_IQ two (I, Q).  The two int16 formats take `gain` (ignored for complex64):
 *   the operand is gain (float)s, one float32 multiply -- the rule of rade_batch_wire_in, so the fused call equals rade_batch_wire_in followed by the complex64 call, bit for
 *   bit.  In the real format the output's imaginary part is exactly +0.0f; it is not computed.  Output: complex64, written in 8-byte stores.
 * n_in_host, n_out_host: [B] counts; p->n0_host [B]: index of the first output written; p->in_base_host [B]; NULL = 0 for every stream.  Strides are in elements of their
 *   own buffer (int16 IQ: x_stride >= 2 n_in); pointers are aligned to their element.  The per-stream values are copied to the device in one record per stream ahead of the
 *   launch (the call synchronises `stream` once for that).  The table lives in the engine's device memory, keyed by the reduced (L, M), and is re-made by an upload on
 *   `stream` when a call asks for another ratio: calls on one stream may alternate between ratios freely.
 * Refused with -1 on the host, before any launch and with nothing written: NULL or misaligned pointers (8 bytes complex64, 2 bytes int16), NULL counts or p, a negative
 *   count or n0, a stride shorter than its row, an unknown format, a gain that is not finite (int16 formats), L or M < 1, reduced K > 8, reduced L T > 16384 floats,
 *   |in_base| > 2^62, (n0 + n_out) M past 2^62.  Admitted: 1/6 and 6/1 (T 192 and 32: 192 floats each), 80/441 (T 192: 15 360 floats), 441/80 (T 32: 14 112), 1/2, 2/3, 3/2.
 * Returns 0.  Any engine (the model is not used; no encoder or receiver state is touched). */
enum { RADE_RATE_C64 = 0, RADE_RATE_S16_REAL = 1, RADE_RATE_S16_IQ = 2 };
typedef struct {
    int L, M;                                     /* the ratio: output rate / input rate = L / M */
    const long long *n0_host;                     /* [B] index of the first output sample this call writes, NULL = 0 */
    const long long *in_base_host;                /* [B] absolute index of x[b][0], NULL = 0 */
} rade_rate_params;
int rade_batch_rate_convert(rade_batch *h, const void *x_dev, long x_stride, const int *n_in_host, int format, float gain, void *y_dev, long y_stride,
                            const int *n_out_host, const rade_rate_params *p, void *stream);
/* host only: the number of n >= 0 with n M < in_end L, i.e. the outputs whose centre tap lies inside an input of in_end samples (-1: L or M < 1, or that many outputs pass
 * the 2^62 limit) */
long long rade_rate_count(long long in_end, int L, int M);
/* host only, no handle, no GPU: the table C [L][T] of the reduced pair.  Returns T (-1: a ratio the call refuses); out == NULL only queries */
int rade_rate_taps(int L, int M, float *out);

/* ---- analog FM: modulator and demodulator of fm.m, every stream in one call (rade_fm.hip) ----------------------------------------------------------------
 * Both calls work on any engine (the model is not used; no encoder or receiver state is touched), keep no state on the device, and obey the buffer rules above.
 *
 * The phasor cis(ph) of a 32-bit phase ph (one turn = 2^32), used by both calls: the top two bits of ph choose the quadrant by swapping and negating the two components,
 * which is exact; the low 30 bits r give an angle in [0, pi / 2): r' = min(r, 2^30 - r) (exact; the two components swapped when the complement was taken), the angle
 * (pi / 2) 2^-30 r' formed in double and rounded once to float32, sine and cosine of it in float32.  r = 0 gives exactly (1, 0): a carrier at Fs / 4 with no modulation
 * is exactly (0, 1), (-1, 0), (0, -1), (1, 0), ..  The deviation from the exact phasor measured on the MI355X is 7.8e-8 at worst (EPS_CIS_MEASURED in tests/test_fm_gpu.py).
 *
 * rade_batch_fm_mod (fm.m:74-94).  Per stream n[b] modulating samples m (RADE_FM_F32: float32; RADE_FM_C64: complex64 whose real part is used, what
 *   rade_batch_rate_convert and rade_batch_wire_in hand over) -> complex64.  The phase is a 32-bit NCO, not a float accumulator: with kc = fc / Fs 2^32 and
 *   kd = fd / Fs 2^32 (doubles made on the host)
 *       inc[k] = (uint32)(int64) rint(fma((double)m[k], kd, kc))          ph[i] = ph0[b] + sum_{k <= i} inc[k]  mod 2^32          tx[i] = cis(ph[i])
 *   The sum is inclusive (fm.m:90-92 adds before it takes the exponential).  A sample that is not finite or whose |m| > 2^16 modulates as 0; finite samples are otherwise
 *   used as they are (|m| > 1 over-deviates, as in fm.m).  Integer sums are associative: a stream modulated in pieces equals the stream modulated whole, bit for bit, when
 *   each piece is given the phase the previous one ended on (phase0_host [B] or NULL = 0; phase_end_host [B] out or NULL: when given, the call also waits for its own
 *   kernels, as the wire meters do; like rade_batch_rate_convert, both calls always wait once ahead of their launches for the copy of the per-stream records, and so
 *   for the work queued on `stream` in front of them).  Against fm.m's float64 accumulate-and-wrap on the same float32 input the phasor differs by 3.4e-9 after 1 s at 48 kHz (tests/test_fm_host.py).
 *   Three plain launches (tile sums, their scan, apply); no workgroup waits for another.
 *   Noise, when sigma > 0: from noise_dev (complex64, dense [B][max n]: row b at + b max n, max n the largest count of the call) or, when that is NULL, generated from
 *   `seed` (non-zero): Philox keyed as in rade_channel_params, counter (p, b, 3, p >> 32) with p = (n0[b] + i) >> 1, words 0-1 for the even sample of the pair and words
 *   2-3 for the odd one, Box-Muller as everywhere (g0, g1 of unit variance).  (The fourth word carries p >> 32, as the rate-Rs channel's does: it is 0, the counter
 *   (p, b, 3, 0), for every n0 + i below 2^33, and keeps the draws distinct up to the 2^62 the call admits.)  n0_host [B] is the absolute index of the piece's first sample (NULL = 0), so pieces equal the
 *   whole bit for bit with noise on as well.
 *       RADE_FM_OUT_COMPLEX   generated: tx + (float)(sigma / sqrt 2) (g0 + j g1) (fm.m:171);  explicit: tx + (float)sigma noise
 *       RADE_FM_OUT_REAL      generated: (Re tx + (float)sigma g0, +0.0f) (fm.m:321-324: real noise, the real part kept);  explicit: (Re tx + (float)sigma Re noise, +0.0f)
 *   each component one float32 product and one float32 sum, rounded separately.  RADE_FM_OUT_REAL is applied with and without noise.  The call does not refuse fc = 0 in
 *   real mode, but a real signal only carries the modulation when fc >= Bfm / 2.
 *   Pre-emphasis (fm.m:80-83: a two-tap FIR and a whole-signal peak normalisation) is NOT on the device; radae_amd.engine.fm_pre_emphasis does it on the host.
 *   Refused (-1, nothing written): NULL or misaligned pointers, a negative count, a stride shorter than its row, an unknown format or mode, Fs <= 0, |fc| > Fs / 2,
 *   fd <= 0 or fd > Fs / 2, a sigma that is negative or not finite, sigma > 0 with neither noise_dev nor a seed, n0 negative or above 2^62, values that are not finite.
 *
 * rade_batch_fm_demod (fm.m:97-126).  complex64 in (a real signal arrives as (x, +0) from rade_batch_wire_in); out float32 (RADE_FM_F32) or complex64 with +0.0f imaginary
 *   (RADE_FM_C64: feeds rade_batch_rate_convert / rade_batch_wire_out directly); optional second output bb_out_dev (complex64): the filtered baseband of the same samples,
 *   analog_fm_demod's rx_bb.  x[b][g] is the sample of absolute index in_base[b] + g, 0 <= g < n_in[b]; output i of row b is the sample of absolute index n = n0[b] + i,
 *   0 <= i < n_out[b] (n0_host NULL: n0 = in_base, one output per input).  Every step is a pure function of n:
 *     1. mix down    xm[n] = x[n] cis(-(fcq n mod 2^32)), fcq = (uint32) llrint(fc / Fs 2^32): re = fma(x.re, c.re, -(x.im c.im)), im = fma(x.re, c.im, x.im c.re).
 *                    fc = 0: the factor is exactly (1, 0).  Samples in front of absolute index 0 and samples outside [in_base, in_base + n_in) are zero; nothing outside
 *                    the stream's n_in samples is read.
 *     2. input FIR   bb[n] = sum_{k = 0..N1-1} b1[k] xm[n - k] (filter(bin, 1, .), causal): one float32 accumulator per component, fused multiply-adds in the order
 *                    k = 0..N1-1.
 *     3. discriminator  d = bb[n] conj(bb[n - 1]): re = fma(p.re, q.re, p.im q.im), im = fma(p.im, q.re, -(p.re q.im)); a = atan2(im, re) evaluated in double and
 *                    rounded to float32; d = 0 gives a = 0 whatever the signs of its zeros (bb[-1] = 0: sample 0 of a stream gives angle 0, fm.m:110); unless ph_dont_limit, a clamped to [-wd, wd], wd = (float)(2 pi fd / Fs);
 *                    then one multiply by (float)(1 / wd).
 *     4. output FIR  y[n] = sum_{k = 0..N2-1} b2[k] a[n - k], ordered like 2.
 *   b1, b2: host float32 arrays given per call, 1 <= N1, N2 <= 512; they are uploaded into engine memory and uploaded again only when their bytes change.  A one-tap
 *   table {1.0f} is an exact pass-through (fm.m's output_filter = 0).  The summation order is stated so that a vector-unit form and an f32 matrix-core form over a Toeplitz
 *   tile would give the same bits; the kernel is the vector-unit form.
 *   Output n depends on inputs n - (N1 + N2 - 1) .. n: a piece handed that much history (through in_base / n0) equals the whole, bit for bit.
 *   De-emphasis (fm.m:123-125, filter(1, prede, .)) is a one-pole recurrence and would need state; it is folded into b2 on the host instead (rade_fm_taps):
 *   b2 = conv(bout, a^k for k < K), a = 1 - 1 / (tc Fs), K the first power with a^K < 2^-30 (39 at 48 kHz, 90 at 96 kHz).  DEVIATION from fm.m: the tail of the
 *   recurrence below 1e-9 is cut off.
 *   Refused: what rade_batch_fm_mod refuses of pointers, counts, strides, formats and rates, plus NULL taps, N1 or N2 outside 1..512, taps that are not finite,
 *   |in_base| or |n0| > 2^62.
 * Both return 0. */
enum { RADE_FM_F32 = 0, RADE_FM_C64 = 1 };
enum { RADE_FM_OUT_COMPLEX = 0, RADE_FM_OUT_REAL = 1 };
typedef struct {
    double Fs, fc, fd;                            /* sample rate, carrier, peak deviation, Hz */
    int in_format, out_mode;                      /* RADE_FM_F32 / RADE_FM_C64; RADE_FM_OUT_COMPLEX / RADE_FM_OUT_REAL */
    double sigma;                                 /* 0: no noise */
    unsigned long long seed;                      /* of the generated noise (used when sigma > 0 and noise_dev is NULL) */
    const void *noise_dev;                        /* complex64 [B][max n] unit noise, or NULL */
    const unsigned *phase0_host;                  /* [B] phase in front of the first sample, NULL = 0 */
    unsigned *phase_end_host;                     /* [B] out: phase behind the last sample, or NULL */
    const long long *n0_host;                     /* [B] absolute index of the first sample (the noise counter), NULL = 0 */
} rade_fm_mod_params;
int rade_batch_fm_mod(rade_batch *h, const void *m_dev, long m_stride, const int *n_host, void *y_dev, long y_stride, const rade_fm_mod_params *p, void *stream);
typedef struct {
    double Fs, fc, fd;
    int out_format, ph_dont_limit;                /* RADE_FM_F32 / RADE_FM_C64; non-zero: no clamp of the discriminator's angle */
    const float *b1; int N1;                      /* input filter, host */
    const float *b2; int N2;                      /* output filter, host */
    const long long *in_base_host;                /* [B] absolute index of x[b][0], NULL = 0 */
    const long long *n0_host;                     /* [B] absolute index of the first output written, NULL = in_base */
    void *bb_out_dev; long bb_stride;             /* complex64 [B][bb_stride] or NULL */
} rade_fm_demod_params;
int rade_batch_fm_demod(rade_batch *h, const void *x_dev, long x_stride, const int *n_in_host, void *y_dev, long y_stride, const int *n_out_host,
                        const rade_fm_demod_params *p, void *stream);
/* host only, no handle, no GPU.
 * rade_fm_sigma: sqrt(Fs / (CN Bfm)), CN = 10^(CNdB / 10), Bfm = 2 (fd + fm_max) (fm.m:16,162): the sigma that gives a unit carrier the C/N inside Carson's bandwidth.
 *   -1: values that are not finite or not positive.
 * rade_fm_deemph_len: K of the folded de-emphasis (0 for tc = 0; -1: tc < 0, a outside (0, 1), K > 512).
 * rade_fm_taps: the two least-squares designs of fm.m:41-47 (firls, bands [0, 0.95 fc, 1.05 fc, 1], amplitudes [1, 1, 0.01, 0.01], unit weights; fc = (Bfm / 2) / (Fs / 2)
 *   for bin, fm_max / (Fs / 2) for bout) in closed form: sinc integrals for the Toeplitz-plus-Hankel normal matrix, linear-ramp integrals for the right side, a dense
 *   solve in double.  ntaps is odd (type I), 3..511; bin gets ntaps values, bout ntaps + K - 1 (the de-emphasis of time constant de_emp_tc folded in; de_emp_tc = 0:
 *   ntaps).  Returns the length of bout (-1: refused); bin == bout == NULL only queries.  The default of the callers is 201 taps, the ncoeffs that fm.m:27 computes and
 *   uses as the filters' delay.  Octave's firls(201, ..) takes its first argument as an ORDER; whether it returns 201, 202 or 203 taps could not be checked (no Octave
 *   where this was written).  The kernel takes any length.  Equal to scipy.signal.firls(201, ..) within 1e-12 (tests/test_fm_host.py). */
double rade_fm_sigma(double CNdB, double Fs, double fm_max, double fd);
int rade_fm_deemph_len(double Fs, double tc);
int rade_fm_taps(double Fs, double fm_max, double fd, int ntaps, double de_emp_tc, double *bin, double *bout);

/* ---- C/No of the chirp header and where it starts: est_CNo.py on the device, every stream in one call (rade_cno.hip) -------------------------------------
 * ota_test.sh:136-148 cuts the first 10 s of a stored off-air file, runs est_CNo.py over them and trims the file at the time of the best window.  With Fs = 8000 and
 * hop = Fs // 4 = 2000 (est_CNo.py:23-73):
 * Windows: N = (int)(8000 window_time) samples, starting at st = 0, 2000, .. while st < n - N (np.arange(0, len - N, hop)): n = N has no window, N + 1 .. N + 2000 one,
 *   N + 2001 two.
 * Bins: bph = N / 8000.0 (double); flow_bin = (int)(bph flow), fhigh_bin = (int)(bph fhigh), noise_st = fhigh_bin + (int)(0.1 fhigh_bin), noise_en = noise_st +
 *   (int)(0.1 fhigh_bin): C truncation toward zero, which is Python's int() (rade_cno_plan; n_bins = the bins of both bands together).
 * Device: per window two numbers, S_c = sum |X[k]|^2 over [flow_bin, fhigh_bin) and S_n over [noise_st, noise_en), X the N-point DFT of the window's complex64 samples.
 * Host, in double after the read-back, written as the script writes it (the logarithms are the host's libm):
 *     No = S_n / ((noise_en - noise_st) / bph)      C = S_c - No (fhigh - flow)      for C > 0: CNodB = 10 log10(C) - 10 log10(No)
 *   the maximum over the windows with C > 0 by strict >, from max_CNodB = 0 and max_st = 0 (the script's max_time is max_st / 8000); max_SNRdB = max_CNodB - 10 log10(3000).
 *   bands_host, when given, receives (S_c, S_n) of window w of stream b at [b][w][0..1], rows max_windows windows apart; windows past a stream's own are not written.
 * How the device forms X (H = 2000, J = N / H, k = J q + r; t[m] = e^{-2 pi i m / N}, ONE table of N complex64 made on the host in double and rounded once per
 *   component, kept in the engine's device memory and re-made when N changes):
 *     Y[n]      = x[b H + n] t[r n]                                                       block b, residue r; n = 50 n1 + n2, q = q1 + 40 q2
 *     A[q1][n2] = t[J n2 q1] sum_{n1 = 0..39} Y[50 n1 + n2] t[(N / 40)((q1 n1) mod 40)]
 *     B_b[k]    = sum_{n2 = 0..49} A[q1][n2] t[(N / 50)((q2 n2) mod 50)]                   = sum_{n < H} x[b H + n] e^{-2 pi i k n / N}, for the k of the two bands only
 *     X_w[k]    = sum_{j = 0..J-1} B_{w+j}[k] t[H ((r j) mod J)]                           formed afresh for every window: nothing is carried from window to window
 *   Summation order: every sum in the order written, one float32 accumulator per component starting from 0, a term acc += y w as four fused multiply-adds (re += y.re w.re,
 *   re -= y.im w.im, im += y.re w.im, im += y.im w.re); a lone product y w as one rounded multiply and one fused multiply-add per component.  |X|^2 = re re + im im and
 *   everything behind it in double: per residue a thread adds its bins (i, i + 512, ..) in ascending order, the 64 lanes of a wavefront are added by a fixed exchange
 *   pattern, the 8 wavefronts in ascending order, and a second launch adds the residues r = 0..J-1 in ascending order.  No atomics: identical calls give identical bits, and
 *   a stream's numbers do not depend on the other streams of the batch.
 * Error bound, counted from these roundings (u = 2^-24; every coefficient has modulus 1, so errors propagate through the later stages unamplified): a table entry is off by at
 *   most u; a lone product adds 2 roundings per component, at most 4 u of the operand's modulus; a sum of m terms is, per component, a 2 m-term real dot product of fused
 *   multiply-adds, off by at most 2 m u sqrt 2 sum |y_i| per component, 4 m u sum |y_i| in modulus.  Along the path of a bin: (1 + 4) + (1 + 160) + (1 + 4) + (1 + 200) + (1 + 4 J)
 *   = (372 + 4 J) u, times 1.01 for the terms of second order:
 *     |X^ - X| <= 1.01 (372 + 4 J) u sum_n |x_n| <= gamma ||x_w||_2,   gamma = 1.01 (372 + 4 J) 2^-24 sqrt N        (J = 16: 2.63e-5 sqrt N)
 *   and for a band of nb bins with exact sum S: |dS| <= 2 e sqrt(nb S) + nb e^2, e = gamma ||x_w||_2 (Cauchy-Schwarz over the band).  The double sums add nothing that counts
 *   (nb 2^-53).  A worst-case bound: tests/test_cno_gpu.py records how far below it the device stays.
 * Input: complex64, 8-byte aligned, x_stride >= every n_host[b]; not written; nothing outside a stream's n_host[b] samples is read (of those, the samples of its windows).
 * The call copies the counts to the device, launches, reads the band sums back and SYNCHRONISES `stream` before the host arithmetic, as the metered rade_batch_wire_out
 *   does.  Any engine (the model is not used; no encoder or receiver state is touched); the device memory (table, counts, partial and band sums) belongs to the engine and is
 *   sized on first use and when a call needs more.
 * Refused with -1 before any launch and with nothing written: NULL h, x_dev, n_host, p or result_host; x_dev not 8-byte aligned; a negative count or one above x_stride; any
 *   n_host[b] < N (the script asserts it); values of p that are not finite; DEVIATION from the script, which takes any window length: N must be a positive multiple of 2000 with
 *   J = N / 2000 <= 32 (window_time a multiple of 0.25 s up to 8 s); flow_bin < 0 (a negative slice index means something else in Python), flow_bin >= fhigh_bin,
 *   (int)(0.1 fhigh_bin) < 1, noise_en > N (the script would silently sum a clipped slice and still divide by the full width); max_windows smaller than the largest window
 *   count when bands_host is given; and, a limit of the kernel's LDS ring, J (ceil((fhigh_bin - flow_bin) / J) + ceil((noise_en - noise_st) / J)) > 16000 (the defaults need
 *   450 J, so every admitted window length passes; it refuses bands that are together wider than about 2000 Hz at J = 32, 4000 Hz at J = 16).
 * rade_cno_plan: host only; the numbers above for a parameter set, -1 where the call would refuse it.
 * rade_chirp: host only; chirp.py:50-65 restated in C: freq = flow, delta = (fhigh - flow) / 8000, phase = 0 in double; per sample phase += 2 pi freq / 8000 (the script's
 *   operation order: (2 pi freq) / 8000), phase -= 2 pi (int)(phase / (2 pi)), freq += delta, then the two turn-around tests (freq > fhigh: delta = -(fhigh - flow) / 8000;
 *   freq < flow: delta = +(fhigh - flow) / 8000), then iq_out[n] = (amp cos(phase), amp sin(phase)) rounded once to float32.  A sequential recurrence of 36000 steps for the
 *   header of ota_test.sh:336, whose only per-stream parameter is amp: it stays on the host, as the FM block's pre-emphasis does.  -1: NULL, nsam < 0, values that
 *   are not finite.  libm's cos / sin against NumPy's may differ in the last place of the double: at most one float32 ulp per component (tests/test_cno_host.py counts them). */
typedef struct {
    double window_time;        /* seconds; N = (int)(8000 * window_time)          (est_CNo.py:25) */
    double flow, fhigh;        /* Hz, the C+N band                                (est_CNo.py:19-20) */
} rade_cno_params;
typedef struct { int N, J, n_bins, flow_bin, fhigh_bin, noise_st, noise_en; } rade_cno_plan_t;
typedef struct {
    int n_windows, n_positive;                  /* windows evaluated; those with C > 0 */
    long long max_st;                           /* start sample of the best window (0 when none) */
    double max_CNodB, max_SNRdB;                /* est_CNo.py:52-55, :71 */
} rade_cno_result;
int rade_cno_plan(const rade_cno_params *p, rade_cno_plan_t *out);
int rade_batch_cno_est(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, const rade_cno_params *p,
                       double *bands_host /* [B][max_windows][2] = (C+N, band sum of No) or NULL */, int max_windows,
                       rade_cno_result *result_host /* [B] */, void *stream);
int rade_chirp(float *iq_out /* [nsam][2] */, int nsam, double flow, double fhigh, double amp);

/* ---- trials of the pilot SNR estimator: est_snr.py on the device, every set point of every channel in one call (rade_snr.hip) --------------------------------
 * est_snr.py is the experiment behind the two constants the live receiver corrects its reported SNR with (m = 0.8070, c = 2.513, dsp.py:415-416; the mean of the
 * straight-line fits est_snr_curves.sh makes over AWGN, MPG and MPP).  A trial is one window of Nw pilot rows x 30 carriers of one stream.  PINNED: the estimator's
 * arithmetic -- receiver_one.est_pilots (dsp.py:418-435) and the script's own formulas (est_snr.py:45-124) as written.  NOT pinned: the script's np.random draws; the
 * noise here is the engine's Philox / Box-Muller generator (or the caller's), so single points differ from a run of the script.
 * Constants, all from the engine's tables: P[c] the pilot row (float32 sqrt 2 times the Barker sign), pg the model's pilot_gain, Pmat[c] the 3-pilot least-squares
 *   matrices (plain transpose) and e^{-j w[c] a}, a = 0.0025 Fs = 20, w[c] and w[c] a formed in float32 as the reference forms them; c_mid = clamp(c, 1, 28).
 * Per pilot row i and carrier c of window k of stream b, every product and sum in float32:
 *     s   = h (pg P[c])                          h = H[(k Nw + i) h_step][c], or 1 without H                                  (est_snr.py:63)
 *     n   = sigma_b g                            g the unit-variance noise of the element
 *     x   = s + n
 *     q_j = x[c_mid - 1 + j] / P[c_mid - 1 + j]  j = 0, 1, 2, same row
 *     r   = (Pmat[c] q)_0 + (Pmat[c] q)_1 e^{-j w[c] a}                                                                        (dsp.py:431-433)
 *     e   = Im(x conj(r) / |r|)                  = Im(x e^{-j angle r});  |r|^2 = 0 in float32 (r = 0) gives angle 0, as numpy does
 *   and six sums per window, rade_snr_sums: S1 = sum |x|^2, S1_sig = sum |s|^2, S1_cross = sum 2 Re(s n) (as the script has it, WITHOUT a conjugate),
 *   S1_noise = sum |n|^2, S2_genie = sum Im(|h| pg P + n)^2 (= sum Im(n)^2: the signal term is real), S2_est = sum e^2.  Every term is formed in float32 and added in
 *   double in one fixed order: row-major over the window, carrier-minor, by one lane per sum.  No atomics: a window's six values do not depend on B, on the grid or on
 *   which other windows are in the call; identical calls give identical bits.
 * Noise, one of two modes (as rade_batch_fm_mod has them):
 *   given      noise_dev, complex64 [B][n_windows Nw][30] at noise_stride elements per stream, unit variance per component; seed = 0
 *   generated  seed != 0, noise_dev NULL: Philox4x32-10 keyed (seed & 0xffffffff, seed >> 32) as rade_channel_params' seed is, counter (q & 0xffffffff, b, 4, q >> 32)
 *              with q = 15 R + (c >> 1), R = row0[b] + k Nw + i the ABSOLUTE pilot row; words 0-1 make the even carrier's g, words 2-3 the odd one's (gauss_pair).  The
 *              draw is a function of R: a stream computed in pieces (the caller advances row0 and the H pointer) gives the bits of the whole.  noise_out_dev, when
 *              given, receives g in the given-noise layout (same noise_stride); a given-noise call fed with it repeats the generated call bit for bit.
 * Error bound, counted from these roundings (u = 2^-24; tests/snr_ref.py: bounds() restates it, tests/test_snr_est_gpu.py records how far below it the device stays).
 *   Per element, in modulus: pg P one rounding, s one more: |ds| <= 2 u |s|; |dn| <= u |n| (+ sqrt 2 sigma dg where the noise itself is off by dg per component:
 *   the generated draws against the float64 Box-Muller); x one rounding: e_x = 2 u |s| + u |n| + u |x| (+ sqrt 2 sigma dg).  A square-and-add is two roundings.  So
 *     |dS1| <= sum 2 u |x|^2 + 2 |x| e_x + e_x^2          |dS1_sig| <= sum 6 u |s|^2          |dS1_noise| <= sum 2 u |n|^2 + 2 |n| e_n + e_n^2
 *     |dS1_cross| <= sum 2 (2 u |s| |n| + e_s |n| + e_n |s| + e_s e_n)          |dS2_genie| <= sum u n_y^2 + 2 |n_y| e_ny + e_ny^2
 *   r: a table entry is off by u, a quotient by at most 3 u (that covers a hardware reciprocal), a complex product by 3 u, a sum by u: along g_0 (1 + 3 + 3) + 2 = 9 u,
 *   along g_1 another product by a table entry and the last sum: 14 u, and the g_0 terms see the last sum too: 10 u; the errors of x enter through the same weights:
 *     e_r = u sum_j (10 |Pmat_0j| + 14 |Pmat_1j|) |q_j| + sum_j (|Pmat_0j| + |Pmat_1j|) e_x[j] / |P_j|
 *   The angle of r is then off by at most (pi / 2) e_r / |r| (nothing is claimed where e_r >= |r|: the term's error is then bounded by 2 |x|); |r|^2 (2 u), its root
 *   (u + a hardware square root's 2 u), the reciprocal (3 u) and the two products (u) leave the unit phasor's modulus off by 7 u and its angle by u; the last two
 *   products and their sum add 2 u |x|:      e_e = e_x + |x| (pi / 2) e_r / |r| + 10 u |x|,      |dS2_est| <= sum u e^2 + 2 |e| e_e + e_e^2
 *   each bound times 1.01 for the terms of second order.  The double sums add nothing that counts (1980 terms at most: 2^-42).
 * Inputs per stream: H_dev complex64 [rows][30] at h_stride elements per stream, row (k Nw + i) h_step used -- h_step = 1, or Ns + 1 = 5 for a rate-Rs file, which
 *   the script decimates with h[::Ns+1] -- NULL: h = 1 (AWGN); n_windows_host[B] (0 is allowed); sigma_host[B] float32 (0 is allowed: rade_snr_sigma); row0_host[B]
 *   the absolute index of the stream's first pilot row, 0 .. 2^40, NULL: 0.  Nothing outside a stream's rows is read or written; inputs are never written.
 * out_host: rade_snr_sums [B][max_windows], host memory; entries at or beyond a stream's window count are not written.  The call copies the per-stream values to the
 *   device, launches once, reads the sums back and SYNCHRONISES `stream`, as rade_batch_cno_est does.  Any engine (of the model only the constant tables are used).
 * Refused with -1 before any launch and with nothing written: NULL h, p, n_windows_host, sigma_host or out_host; Nw outside 1..66 (est_snr.py -T up to 8 s; the
 *   default -T 1.0 gives 8); h_step outside 1..5; neither a seed nor noise_dev, or both; noise_out_dev without a seed; a pointer that is not 8-byte aligned; a negative
 *   count; max_windows below a stream's count; a sigma that is negative or not finite; row0 outside 0 .. 2^40; h_stride (with H_dev) below the
 *   ((n_windows Nw - 1) h_step + 1) 30 elements a stream reads, noise_stride (with noise_dev or noise_out_dev) below its n_windows Nw 30.
 * Host only, double arithmetic, no device:
 *   rade_snr_sigma(snrdB)   sqrt(Es / 10^(snrdB / 10)) / sqrt 2, Es = sum (pg P[c])^2 / 30 with the float32 products the kernel uses (est_snr.py:57-59)
 *   rade_snr_finish         est_snr.py:96-122 over one window's sums: snr_est = S1 / (2 S2) - 1 with S2 = S2_est (eq_ls) or S2_genie, a value <= 0 becomes 0.1;
 *                           snrdB_genie = 10 log10(S1_sig / S1_noise), snrdB_est = (10 log10 snr_est - c) / m, NdB_genie = 10 log10(2 S2_genie), NdB_est =
 *                           10 log10(2 S2_est).  The script has no guard for S2 = 0 and neither has this: IEEE arithmetic, snr_est = +inf (NaN for 0 / 0, which the
 *                           clamp does not catch either) and NdB = -inf.  -1: NULL, m = 0 or values that are not finite.
 *   rade_snr_fit            the degree-1 least-squares line y = m x + c of np.polyfit(x, y, 1) (est_snr.py:178), by centred sums.  -1: NULL, n < 2, constant x.
 *   rade_snr_track          what the live receiver does with one frame's sums (dsp.py:438-456) for n windows of Nw = 1 in turn: S2 = S2_est + 1e-12, snr_est =
 *                           S1 / (2 S2) - 1, <= 0 becomes 0.1, (10 log10 snr_est - c) / m, + 10 log10(Rs Nc / 3000) + 10 log10((M + Ncp) / M) with Rs = 50,
 *                           Nc = 30, M = 160, Ncp = 32, then *state = 0.9 *state + 0.1 of it; out[i] = *state after frame i: the figure rade_snrdB_3k_est reports
 *                           before its rounding, in double where the reference's tensors are float32.  -1: NULL sums or state, n < 0, m = 0. */
typedef struct { double S1, S1_sig, S1_cross, S1_noise, S2_genie, S2_est; } rade_snr_sums;
typedef struct {
    int Nw, h_step;                             /* pilot rows per window, 1..66; rows of H_dev per pilot row, 1..5 */
    const void *H_dev; long h_stride;           /* complex64 [rows][30] per stream or NULL (h = 1) */
    const float *sigma_host;                    /* [B] */
    const long long *row0_host;                 /* [B] or NULL (0) */
    const void *noise_dev;                      /* complex64 [n_windows Nw][30] per stream, or NULL with a seed */
    void *noise_out_dev;                        /* optional, with a seed: the generated draws in the same layout */
    long noise_stride;                          /* elements per stream of noise_dev / noise_out_dev */
    unsigned long long seed;
} rade_snr_params;
typedef struct { double snrdB_genie, snrdB_est, NdB_genie, NdB_est; } rade_snr_point;
int rade_batch_snr_trials(rade_batch *h, const int *n_windows_host /* [B] */, const rade_snr_params *p, rade_snr_sums *out_host /* [B][max_windows] */, int max_windows,
                          void *stream);
double rade_snr_sigma(double snrdB);
int rade_snr_finish(const rade_snr_sums *s, int eq_ls, double c, double m, rade_snr_point *out);
int rade_snr_fit(const double *x, const double *y, int n, double *m, double *c);
int rade_snr_track(const rade_snr_sums *sums, int n, double c, double m, double *state, double *out /* [n] or NULL */);

/* ---- the spectrogram of a recording: plot_specgram.m on the device, every stream in one call (rade_spec.hip) ------------------------------------------------
 * ota_test.sh:130-134 draws plot_specgram(s, 8000, 200, 3000) of every stored off-air file, evaluate.sh:112, :153 (utils.sh:66-68) plot_specgram(rx, 8000, 0, 3000).  With
 * Fs = 8000 (plot_specgram.m:6-16): step = 160 (20 ms; the comment there says 5), window = 1280, fftn = 2048, S = abs(specgram(x, 2048, 8000, 1280, 1120)(2:1024, :)),
 * S / max(S(:)), clipped to [10^(-20/10), 10^(-3/10)], shown as imagesc(log(S)).
 * RECALLED, NOT VERIFIED (the signal package's specgram.m and hanning.m were not at hand where this was written): hanning(m) = 0.5 - 0.5 cos(2 pi (1:m)' / (m + 1)), no
 *   zero end points; specgram turns a scalar window into hanning(window), starts its slices at the one-based offsets 1 : step : length(x) - window, multiplies each by the
 *   window, zero-pads to the transform and returns rows 1 : n / 2 (bins 0..1023); length(x) <= window is an error.
 * Geometry: win 1280, step 160, nfft 2048.  DEVIATION: plot_specgram takes any Fs; only the 8 kHz geometry is built.
 * Slices: starts s = 0, 160, .. while s < n - 1280 (np.arange(0, n - 1280, 160)): n = 1281 .. 1440 one slice, 1441 two (rade_specgram_slices).
 * Display band: k0 = max(1, ceil(fmin 2048 / 8000)), k1 = min(1023, floor(fmax 2048 / 8000)), n_bins = k1 - k0 + 1 (0-3000 Hz: 1..768; 200-3000 Hz: 52..768).  The band
 *   only crops the image: the maximum is taken over bins 1..1023 of every slice, as the script takes it.
 * Window: w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 1281), host, double, rounded once to float32, kept in the engine's device memory (rade_specgram_window).
 * Operand: v[i] = x.re w[i], one rounded float32 multiply.  The imaginary part of a complex64 input is not read.  Int16 input is gain (float)s first, the rule of
 *   rade_batch_wire_in: the fused call equals wire_in followed by the complex64 call, bit for bit.
 * Transform: X_s[k] = sum_{i < 1280} v[i] e^{-2 pi i k i / 2048}, k = 1..1023.  How the device forms it (t[m] = e^{-2 pi i m / 2048}: ONE table of 2048 complex64, host,
 *   double, rounded once per component):
 *     z[i] = (v_a[i], v_b[i]) for i < 1280, 0 behind         slices a = 2 m and b = 2 m + 1 of ONE stream are the two parts of one complex transform; a last slice
 *                                                            without a partner has v_b = +0
 *     five radix-4 stages, s = 1, 4, 16, 64, 256; butterfly t = q + s p (q < s, t < 512) of a stage reads a_j = y[t + 512 j], j = 0..3 (stage 1: y = z), and writes
 *       y'[q + s (4 p + m)] = b_m t[m p s], m = 0..3 (m = 0: b_0 itself, no product), where
 *       e = a_0 + a_2, f = a_1 + a_3, g = a_0 - a_2, d = a_1 - a_3;  b_0 = e + f, b_2 = e - f, b_1 = g - i d = (g.re + d.im, g.im - d.re), b_3 = g + i d = (g.re - d.im, g.im + d.re)
 *       and a product y w = (fma(-y.im, w.im, y.re w.re), fma(y.im, w.re, y.re w.im)): one rounded multiply and one fused multiply-add per component
 *     the radix-2 stage: Z[k] = y[k] + y[k + 1024], Z[2048 - k] = y[1024 - k] - y[2048 - k]
 *     the two slices: X_a[k] = 0.5 (Z[k] + conj Z[2048 - k]): re = 0.5 (Z[k].re + Z[2048 - k].re), im = 0.5 (Z[k].im - Z[2048 - k].im)
 *                     |X_b[k]| from 0.5 (Z[k] - conj Z[2048 - k]): re = 0.5 (Z[k].re - Z[2048 - k].re), im = 0.5 (Z[k].im + Z[2048 - k].im)     (= i X_b[k]: same modulus)
 *     mag = sqrtf(fma(re, re, im im)): im im rounded, then one fused multiply-add, then the correctly rounded square root.
 *   Every addition is one rounded float32 addition per component in the order written.  The zeros of the padding take part as zeros.  A slice's bits are a function of its
 *   stream's samples, its index and whether it has a partner (n_slices odd and the slice the last) -- not of the batch size, the other streams, the strides or which
 *   outputs were asked for.  No atomics for the values: identical calls give identical bits.
 * Error bound, counted from these roundings (u = 2^-24; every factor has modulus 1 and a butterfly's outputs are bounded by the sum of its inputs' moduli, so the errors
 *   of the stages add, each relative to S = sum_i |z[i]| = sum_i sqrt(v_a[i]^2 + v_b[i]^2)): the window entry u and the operand's multiply u; per radix-4 stage the two
 *   levels of additions 2 u, the table entry u and the lone product 4 u: 7 u, five stages 35 u; the radix-2 stage u; the separating addition u; the magnitude (a product,
 *   a fused multiply-add, a square root: relative 2.5 u) 3 u.  42 u, times 1.01 for the terms of second order and rounded up:
 *     | mag^ - |X_s[k]| | <= 44 u S,   S <= sum_i |v_a[i]| + sum_i |v_b[i]| <= sqrt(1280) sqrt(||v_a||^2 + ||v_b||^2)
 *   against the float64 X of the double window (tests/specgram_ref.py); barring underflow.  A worst-case bound: tests/test_specgram_gpu.py records how far below it the
 *   device stays.
 * Peak: peak[b] = the maximum of the float32 mag over all slices and k = 1..1023 (a maximum does not depend on the order it is taken in; the kernel folds the
 *   workgroups' maxima with an integer atomic maximum on the bits, which order as the values do).  With peak_in_host the given values are used instead and peak_host
 *   returns them.
 * Levels: T[j] = lo (hi / lo)^((j - 0.5) / 255), j = 1..255, double, rounded once to float32 (rade_specgram_levels: out[j - 1]); the level of a cell is the number of j
 *   with mag >= T[j] peak, T[j] peak one rounded float32 multiply -- no logarithm on the device.  This is what imagesc(log(min(max(S / max, lo), hi))) shows on a
 *   256-step grey scale when both clips are reached.  The image is an exact function of (mag, peak, table).  A peak of 0 (silence; NaN in the script): every cell is
 *   level 0 and peak_host[b] = 0.
 *   DEVIATION: imagesc scales to the data's own minimum and maximum, and the renderer's colour map and the JPEG coding are not reproduced.
 * Layout: img[b][s][k - k0] at img_dev + b img_stride + s n_bins + (k - k0) bytes; mag[b][s][k - 1] at mag_dev + b mag_stride + 1023 s + (k - 1) floats; rows contiguous.
 *   n_slices_host[b] is always written.  Nothing outside a stream's n_slices n_bins bytes or n_slices 1023 floats is written and nothing outside its n_host[b] samples is
 *   read.  img_dev may have any alignment (byte stores), mag_dev is 4-byte aligned, x_dev aligned to its element (8 bytes complex64, x_stride in samples; 2 bytes int16,
 *   x_stride in int16).  Strides are at least the stream's own extent.
 * Two passes, because the normaliser is a maximum over the whole recording: transform, magnitude and maximum; then the levels, for which the transforms are computed
 *   again (rade_spec.hip says why).  With peak_in_host one pass.
 * Refused with -1 before any launch and with nothing written: NULL h, x_dev, n_host, p, peak_host or n_slices_host; both outputs NULL while peak_in_host is given; misaligned
 *   pointers; a negative count or one above x_stride; any n_host[b] <= 1280 (specgram raises an error); a stride shorter than the stream's output; an unknown format; a
 *   gain, fmin, fmax, lo or hi that is not finite; fmin > fmax; k0 > k1; not 0 < lo < hi <= 1; a peak_in_host value that is negative or not finite.
 * The call copies the counts (and the thresholds) to the device, launches, reads peak back and SYNCHRONISES `stream`, as rade_batch_cno_est does.  Any engine (the model is
 *   not used; no encoder or receiver state is touched); the device memory (tables, counts, peaks) belongs to the engine and is sized on first use.
 * rade_specgram_plan, _slices, _window, _levels: host only; the numbers above, -1 where the call would refuse the parameters. */
enum { RADE_SPEC_C64 = 0, RADE_SPEC_S16_REAL = 1 };
typedef struct {
    double fmin, fmax;            /* Hz: the displayed band (plot_specgram's 3rd and 4th argument) */
    double lo, hi;                /* clips on |X| / peak: 10^(-20/10), 10^(-3/10) */
    const float *peak_in_host;    /* [B] normaliser per stream, or NULL = the stream's own maximum (the reference) */
} rade_specgram_params;
typedef struct { int n_bins, k0, k1, win, step, nfft; } rade_specgram_plan_t;   /* k0..k1 inclusive */
int rade_specgram_plan(const rade_specgram_params *p, rade_specgram_plan_t *out);
long long rade_specgram_slices(long long n);                       /* host only: slices of an n-sample stream, 0 for n <= 1280 */
void rade_specgram_window(float *out /* [1280] */);                /* host only */
int rade_specgram_levels(double lo, double hi, float *out /* [255] */);   /* host only */
int rade_batch_specgram(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int format, float gain,
                        const rade_specgram_params *p,
                        unsigned char *img_dev, long img_stride,    /* [B][slices][n_bins] levels, img_stride in bytes per stream; or NULL */
                        float *mag_dev, long mag_stride,            /* [B][slices][1023] |X[1..1023]|, mag_stride in floats per stream; or NULL */
                        float *peak_host /* [B] */, int *n_slices_host /* [B] */, void *stream);

/* ---- the waveform itself: Welch power spectrum, 99 % bandwidth, mean power and PAPR of every stream (rade_psd.hip) --------------------------------------------
 * radae_plots.m: do_plots (:34-72) takes the --write_rx / --write_tx file of a run: y = pwelch(rx, [], [], 1024, Fs) (:53), max and mean of |rx|^2, their ratio in dB
 * over the file and over its first 160 samples (:62-69), and bandwidth() (:100-116): the smallest bw whose bins round(centre -+ bw / 2) hold more than 99 % of sum(y).
 * RECALLED, NOT VERIFIED (pwelch.m was not at hand where this was written): with an empty window and overlap pwelch takes a Hamming window of
 *   2^ceil(log2(sqrt(n / 0.5))) samples at 50 % overlap.  rade_psd_octave_default(n, &win, &step) returns that recalled rule (win may exceed 1024) and nothing here
 *   depends on it: DEVIATION: the stage takes win and step explicitly.
 * DEVIATION: bandwidth() asks for Nfft = 1204; by its centre formula round(Nfft 1500 / Fs) and its frequency axis that is a slip for 1024.  Only nfft = 1024 is built.
 * DEVIATION: the density scaling 1 / (n_seg Fs sum w^2) and the symmetric window are pinned against scipy.signal.welch (tests/test_psd_host.py), not against Octave.
 * rade_batch_psd
 * Geometry: nfft 1024; the window length 16 <= win <= 1024, each segment zero-padded to 1024; the hop 1 <= step <= win.  Segments start at s = 0, step, 2 step, .. while
 *   s + win <= n; a tail that does not fill a segment is not used (rade_psd_segments: 0 for n < win).
 * Window: w[i] = 0.54 - 0.46 cos(2 pi i / (win - 1)), Octave's hamming(win), scipy's get_window('hamming', win, fftbins=False): host, double, rounded once to float32,
 *   kept in the engine's device memory for the last win used (rade_psd_window).
 * Operand: z[i] = (x.re w[i], x.im w[i]), one rounded float32 multiply per component.  RADE_SPEC_S16_REAL: x = (gain (float)s, +0), the rule of rade_batch_wire_in: the
 *   fused call equals wire_in followed by the complex64 call, bit for bit.  Two real segments are not paired into one transform.
 * Transform: X_s[k] = sum_{i < win} z[i] e^{-2 pi i k i / 1024}, k = 0..1023.  How the device forms it (t[m] = e^{-2 pi i m / 1024}: ONE table of 1024 complex64, host,
 *   double, rounded once per component): five radix-4 stages, s = 1, 4, 16, 64, 256; butterfly t = q + s p (q < s, t < 256) of a stage reads a_j = y[t + 256 j], j = 0..3
 *   (stage 1: y = z, zeros for i >= win), and writes y'[q + s (4 p + m)] = b_m t[m p s], m = 0..3 -- the butterfly b_m and the product form of rade_batch_specgram
 *   above, one rounded multiply and one fused multiply-add per component.  1024 = 4^5: there is no radix-2 stage and the fifth stage leaves X_s[k] at element k.
 * Accumulation: p_s[k] = fma(re, re, im im) in float32, im im rounded.  A workgroup owns a run of R = 32 consecutive segments of one stream (rade_psd_plan returns R) and
 *   adds their p_s[k] to 0 in ascending segment order in float32; the runs of a stream are added in ascending order in double, multiplied once by the double
 *   1 / (n_seg Fs sum_i w[i]^2) (the sum over the float32 window, formed on the host in double in ascending order) and rounded once to float32: P[b][k], the two-sided
 *   density.  No atomics for the values: identical calls give identical bits, and a stream's bits are a function of its own samples, its length, win, step and Fs -- not
 *   of the batch size, the other streams or the strides.
 * Error bound, counted from these roundings (u = 2^-24; every factor has modulus 1, so the stages' errors add, each relative to S_s = sum_i |x[s + i] w[i]|, w the
 *   double window): the window entry u, the operand's multiply u, 7 u per radix-4 stage (two levels of additions 2 u, the table entry u, the lone product 4 u): 37 u on
 *   X_s[k], so 74 u S_s^2 on |X_s[k]|^2 <= S_s^2; the square (a product and a fused multiply-add) 2 u; the run's R - 1 float32 additions (R - 1) u of the run's sum; the
 *   fold in double below u 2^-20; sum w^2 of the float32 window 2 u; the last rounding u.  78 + R, times 1.01 for the terms of second order:
 *     | P^[b][k] - P[b][k] | <= (80 + R) u sum_s S_s^2 / (n_seg Fs sum w^2) = 112 u sum_s S_s^2 / (n_seg Fs sum w^2)
 *   against the float64 P of the double window (tests/psd_ref.py); barring underflow.  A worst-case bound: tests/test_psd_gpu.py records how far below it the device stays.
 * Layout: P[b][k] at psd_dev + b psd_stride + k floats, k = 0..1023 in natural order, 0 .. Fs 1023 / 1024, as pwelch returns for complex input.  n_seg_host[b] is always
 *   written.  Nothing outside a stream's 1024 floats is written and nothing outside its n_host[b] samples is read.  psd_dev is 4-byte aligned, psd_stride >= 1024; x_dev
 *   aligned to its element (8 bytes complex64, x_stride in samples; 2 bytes int16, x_stride in int16).
 * Refused with -1 before any launch and with nothing written: NULL h, x_dev, n_host, psd_dev or n_seg_host; misaligned pointers; a negative count, one above x_stride or
 *   any n_host[b] < win; psd_stride < 1024; win outside 16..1024; step outside 1..win; an unknown format; a gain or Fs that is not finite or not positive.
 * The call copies the counts and scales to the device, launches twice and SYNCHRONISES `stream`, as rade_batch_specgram does.  Any engine; the device memory (table,
 *   window, counts, the partial rows: 4 KB per run of 32 segments) belongs to the engine and grows with the call.
 * rade_batch_sigstat
 *   Per stream sum2 = sum |x|^2 and peak2 = max |x|^2 over its n_host[b] samples, and head_sum2, head_peak2 over its first min(n, head) (the script's 160: one OFDM
 *   symbol, the pilot).  Every term is t = fma(re, re, im im) in float32 (im im rounded; int16 input by the rule above).  Sums: a chunk is 8192 consecutive samples;
 *   thread j of 256 adds the chunk's samples j, j + 256, .. as doubles in ascending order, the 64 lanes of a wavefront are added by a fixed tree, the four wavefronts in
 *   order (level 1); the chunks of a stream are added in ascending order (level 2).  Peaks: float32 maxima of t, which do not depend on the order.  Each term carries at
 *   most 2 u relative error and the double sums add below u 2^-20: sum2 is within 2.02 u of the sum of the exact squares.  n = 0 gives zeros.  The bits of a stream do not
 *   depend on the batch.  Mean power is sum2 / n, PAPR 10 log10(peak2 n / sum2) (inference.py:201, :211: 20 log10(max |tx| / sqrt(S))); silence is 0 / 0.
 *   Refused with -1 before any launch and with nothing written: NULL h, x_dev, n_host or result_host; a misaligned x_dev; a negative count or one above x_stride; a
 *   negative head; an unknown format; a gain that is not finite or not positive.  The call reads the results back and SYNCHRONISES `stream`.
 * rade_psd_bandwidth: bandwidth() / spec_power() as written, on the host in double, P[0..nfft-1] as one-based y: centre = round(nfft centre_hz / Fs); for bw = 2, 3, ..:
 *   st = max(1, round(centre - bw / 2)), en = round(centre + bw / 2), p = sum P(st..en); stop at the first bw with p > frac sum P and report bw Fs / nfft and p / sum P.
 *   round is half away from zero, as Octave's.  -1 where en would pass the last bin (the script raises an index error there) or an argument is refused.
 * rade_psd_plan, _segments, _window, _octave_default, _bandwidth: host only. */
typedef struct { int nfft, win, step, run; } rade_psd_plan_t;       /* run: R, the segments whose |X|^2 a workgroup adds in float32 */
typedef struct { double sum2, peak2, head_sum2, head_peak2; long long n; } rade_sigstat_result;
int rade_psd_plan(int win, int step, rade_psd_plan_t *out);         /* -1 where rade_batch_psd refuses win or step */
long long rade_psd_segments(long long n, int win, int step);       /* host only: segments of an n-sample stream, 0 for n < win */
int rade_psd_window(int win, float *out /* [win] */);               /* host only */
int rade_psd_octave_default(long long n, int *win, int *step);     /* host only: RECALLED, NOT VERIFIED */
int rade_psd_bandwidth(const double *P, int nfft, double Fs, double centre_hz, double frac, double *bw_hz, double *ratio);
int rade_batch_psd(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int format, float gain, int win, int step, double Fs,
                   float *psd_dev, long psd_stride,                 /* [B][1024] density, psd_stride in floats per stream */
                   int *n_seg_host /* [B] */, void *stream);
int rade_batch_sigstat(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int format, float gain, int head,
                       rade_sigstat_result *result_host /* [B] */, void *stream);

/* ---- whole-file pilot acquisition: rx.py's frame loop (rx.py:146-188, --acq_test :164-178, :190-195) over every hop of every stream (rade_acq.hip) -------------------
 * rx.py walks a stored recording one modem frame at a time: acquisition.detect_pilots (dsp.py:178-231) over 2 Nmf + M + Ncp = 2112 samples, a small state machine, and
 * acquisition.refine (dsp.py:233-270) where it acquires.  Here every hop of every stream is one call.  Geometry: model19_check3's only, Fs 8000, M 160, Ncp 32, Nmf 960,
 * the 40 coarse frequencies -50 .. +47.5 Hz in steps of 2.5; p and p_w are the engine's own tables (dsp.py:166-173).
 * Surface: D[t][f] = sum_{m < 160} conj(x[t + m]) p_w[m][f], x the stream's n complex64 samples.
 * Hops: hop k exists while n - 961 k >= 2112 (the script drops one tail sample per hop, rx = rx[Nmf:-1]): n = 2111 none, 2112 .. 3072 one, 3073 two (rade_acq_hops).
 *   DEVIATION: with between 2 Nmf + M and 2 Nmf + M + Ncp samples left the script trips detect_pilots' assert; the loop here stops one hop earlier.
 *   Hop k starts at sample 960 k: Dt1 = D[960 k + t], Dt2 = D[960 (k + 1) + t], t = 0..959.  Hop k's Dt2 is hop k + 1's Dt1: every row of D is formed once.
 * Per hop: Dtmax12 = max over (t, f) of |Dt1[t][f]| + |Dt2[t][f]| (one rounded float32 addition of the two float32 magnitudes), tmax and f_ind the cell that has it; of
 *   equal cells the first in the script's order wins (smallest t, then smallest f: its comparison is a strict >, from 0).  An all-zero hop has Dtmax12 0, tmax 0,
 *   f_ind 0 and, as in the script, fmax 0.0 (rade_acq_fmax; otherwise fmax = -50 + 2.5 f_ind).
 *   S1 = sum |Dt1|, S2 = sum |Dt2| over the 38400 cells, in double: a lane adds its 30 cells of a block, the 64 lanes are added by a fixed exchange pattern, and a
 *   second launch adds the 20 wavefronts of a block in ascending order.  No atomics: identical calls give identical bits, and a stream's results do not depend on the
 *   other streams of the batch, on B or on the strides.
 *   Host, in double after the read-back: sigma_r = (S1 + S2) / 38400 / sqrt(pi / 2) / 2, Dthresh = 2 sigma_r sqrt(-ln(Pacq_error1 / 5)), candidate = Dtmax12 > Dthresh.
 *   (The script's float32 means differ from these double sums by a few 1e-7 of Dthresh.)
 * How the device forms D: the two-stage correlator of the receiver's search (rade_pack.c, rd_corrq16_table_fill), with the engine's own two tables.  p_w[m][f] = sum_{r < 16}
 *   alpha[r][f] s_r[m], s_r[m] = p[m] q_r(x_m), q_r the 16 polynomials orthonormal on x_m = (m - 79.5) / 80, alpha[r][f] = sum_m q_r(x_m) e^{j w_f m}; so
 *   D[t][f] = sum_r alpha[r][f] Mom_r[t], Mom_r[t] = sum_m conj(x[t + m]) s_r[m].  Stage 1, the moments: a real GEMM, rows (r, re | im), K = (m, re | im), columns t, on
 *   v_mfma_f32_16x16x32_f16.  Both operands are two binary16 planes, v = hi + lo with hi = fl16(v), lo = fl16(v - hi), under a power-of-two scale: 2^12 for s_r, and for
 *   the samples the power of two that puts the largest |component| of the 208 samples a wavefront reads for a block (48 timings) into [2^7, 2^8).  hi x hi is accumulated by
 *   10 instructions (K = 32 each) into one float32 accumulator, lo x hi and hi x lo by 20 into a second, lo x lo is dropped; one float32 addition joins the two.  Stage 2:
 *   the joined moments times 2^-7 in three binary16 planes (33 bits) against the two planes of 2^10 alpha, five instructions (K = 32: the 16 complex moments) into one
 *   accumulator, smallest partial products first.  The power-of-two scales are undone exactly, and |D| = sqrt(fma(re, re, im im)) on the hardware square root (1 ulp).
 *   85 matrix instructions per 16 timings, where the 80 rows of p_w itself take 150.
 * Error bound, counted from these roundings.  The matrix instruction's own rounding is not documented; ASSUMED: each instruction returns its 33-term sum within 2^-23 of the
 *   sum of the terms' moduli (two float32 roundings).  Stage 1, per real component of Mom_r relative to B_r = sum_m |x[t + m]| |p[m]| |q_r(x_m)|: the two planes of either
 *   operand leave 2^-22 each and the dropped product 2^-22, the hi x hi chain adds 10 x 2^-23, the cross chain 20 x 2^-23 x 2^-10, the joining addition 2^-24: e1 = (0.75 +
 *   1.25 + 0.02 + 0.0625) 2^-20 = 2.09 x 2^-20, sqrt 2 e1 B_r in modulus.  Stage 2 multiplies the moment r by alpha[r][f], so these errors reach D[t][f] as sqrt 2 e1 sum_r
 *   |alpha[r][f]| B_r = sqrt 2 e1 A[t][f], with
 *       A[t][f] = sum_{m < 160} |x[t + m]| |p[m]| G[f][m],   G[f][m] = sum_r |alpha[r][f]| |q_r(x_m)|     (the moment form's gain: 1 at 0 Hz, up to 4.4 at -50 Hz)
 *   Stage 2's own roundings, relative to sum_r |alpha[r][f]| |Mom_r| <= A[t][f]: the planes of alpha 2^-22 (the moments' three planes and the dropped product: below 2^-32),
 *   the chain 5 x 2^-23: sqrt 2 (0.25 + 0.625) 2^-20 = 1.24 x 2^-20 in modulus.  The magnitude (a product, a fused multiply-add, the square root): 3 x 2^-24 |D| <= 0.19 x
 *   2^-20 A.  Sum 4.39, with 1.01 for the terms of second order and rounded up: RADE_ACQ_EPS = 4.5 x 2^-20 = 4.29e-6.  Last, the two tables' product is p_w only within
 *   RADE_ACQ_TAB = 1e-8 per entry (16 moments of a band-limited phase: 4.8e-9 as built; rd_corr_tables_check, tests/test_host_cpu.py), which adds RADE_ACQ_TAB sum_m |x[t + m]|:
 *       | |D|^ - |D| | <= RADE_ACQ_EPS A[t][f] + RADE_ACQ_TAB sum_{m < 160} |x[t + m]|
 *   and the same bound holds for the complex value in dt_dev; barring underflow (a low plane below 2^-24 of the scaled maximum: 2^-32 of the block's largest component
 *   per term).  Dtmax12's cell: the bounds of its two cells + 2^-24 Dtmax12; S1: the sum of the bounds of the block's 38400 cells (the double sums add nothing that
 *   counts).  A worst-case bound under the stated assumption: tests/test_acq_gpu.py records how far below it the device stays (under 2 %).
 * dt_dev (optional): complex64 [B][n_rows][40], D[t0 + r][f] of every stream at [b][r][f], in the script's convention (a hop's 960 rows are what --write_Dt writes).
 *   Only the rows the hops use exist: t < 960 (n_hops + 1).  Rows beyond that are not written.
 * Input: complex64, 8-byte aligned, x_stride >= every n_host[b]; not written; nothing outside a stream's n_host[b] samples is read.  Streams with no hop are not an error
 *   (n_hops 0, nothing written for them).  The call copies the counts to the device, launches, reads the hop records back and SYNCHRONISES `stream` before the host
 *   arithmetic, as rade_batch_cno_est does.  Any engine (the model is not used; no encoder or receiver state is touched); the device memory (counts, partials, records)
 *   belongs to the engine and is sized on first use and when a call needs more.
 * Refused with -1 before any launch and with nothing written: NULL h, x_dev, n_host, hops_host or n_hops_host; x_dev or dt_dev not 8-byte aligned; a negative count or one
 *   above x_stride; max_hops smaller than the largest hop count; with dt_dev, t0 < 0, n_rows < 1 or t0 + n_rows > x_stride; Pacq_error1 not inside (0, 5).
 * rade_acq_track: host only; the state machine of rx.py:151-188 over one stream's hop records.  A candidate in `search` moves to `candidate` and stores tmax_candidate with
 *   valid_count 1; a further candidate with |tmax - tmax_candidate| < 0.02 M increments the count, and when it exceeds 3 the hop is an event {hop, tmax, f_ind}; anything
 *   else returns to `search`.  acq_test 0: stop at the first event (the script's normal run); 1: go back to `search` and collect every event.  log_out[k] (optional) is
 *   what the script prints in hop k's line: the state (0 search, 1 candidate), tmax_candidate and valid_count BEFORE the hop's update (0 until first set).  Returns the
 *   number of events (those beyond max_events are counted, not stored), -1: NULL hops with n_hops > 0, NULL events with max_events > 0, negative counts.
 * rade_batch_acq_refine: acquisition.refine for a list of (stream, t_abs = 960 hop + tmax, fmax), one workgroup per event.  For the 80 frequencies fmax - 10 + 0.25 i and the
 *   timings t_abs - 1 .. t_abs + 1: Dt1 = sum_m x[t + m] e^{-j w m} conj(p[m]), Dt2 the same at t + 960 times e^{-j w 960}, w = 2 pi f / 8000; the maximum of
 *   |Dt1 + Dt2| by strict > from 0 in the script's order (frequency outer, timing inner).  Everything in double, in ascending m.  DIFFERENCE: the script multiplies
 *   complex64 samples by complex128 phasors and rounds each dot product to complex64 before it adds and compares (relative 6e-8); near-equal cells may order otherwise.
 *   DEVIATION: the script hands refine the hop's slice x[960 k : n - k] and the timing inside it; here the timing is absolute and its windows are held against the whole
 *   stream's n (the same samples: a hop's windows always lie inside its slice).  DEVIATION: a timing whose windows leave [0, n) is skipped (the script reads x[-1] for t = -1 and fails behind the end); with no timing left, or an all-zero window,
 *   t = t_abs, f = fmax, Dmax = 0.  dfine_host (optional) [n_events][80]: |Dt1| of the winning timing over the 80 frequencies (|acq.D_fine|).  Synchronises `stream`.
 *   Refused: NULLs, misaligned x_dev, n_events < 0, a count outside [0, x_stride], an event whose stream is outside [0, B), whose |t_abs| exceeds 2^40 or whose fmax is
 *   not finite.
 * rade_acq_stats: host only; rx.py:134, :170-171, :190-195.  An event passes when |(t - 960 hop) - (Ncp + Ntap / 2)| < 0.0025 Fs and |f - fmax_target| <= 5 (t, f refined;
 *   Ntap 101 with the input band-pass, 0 without; Ntap / 2 is 50.5).  pfail = fails / (passes + fails) (0 with no event, where the script divides by zero);
 *   mean_acq_time = (960 (n_hops + 1) / 8000) / passes (the script's mf counter ends one above the hop count), infinity with no pass; passed = pfail < 0.2 and
 *   mean_acq_time < acq_time_target. */
#define RADE_ACQ_EPS (4.5 / 1048576.0)
#define RADE_ACQ_TAB 1e-8
typedef struct { float Dtmax12; double Dthresh; int tmax, f_ind, candidate; double S1, S2; } rade_acq_hop;
typedef struct { int hop, tmax, f_ind; } rade_acq_event;
typedef struct { int state, tmax_candidate, valid_count; } rade_acq_log;
typedef struct { int stream; long long t_abs; double fmax; } rade_acq_refine_in;
typedef struct { long long t; double f, Dmax; } rade_acq_refined;
typedef struct { int passes, fails, passed; double pfail, mean_acq_time; } rade_acq_result;
int rade_acq_hops(long long n);                                    /* host only */
double rade_acq_fmax(const rade_acq_hop *hop);                     /* host only */
int rade_batch_acq_detect(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, double Pacq_error1 /* the script's 1e-5 */,
                          rade_acq_hop *hops_host /* [B][max_hops] */, int max_hops, int *n_hops_host /* [B] */,
                          void *dt_dev /* complex64 [B][n_rows][40] or NULL */, long long t0, int n_rows, void *stream);
int rade_acq_track(const rade_acq_hop *hops, int n_hops, int acq_test, rade_acq_event *events, int max_events, rade_acq_log *log_out /* [n_hops] or NULL */);
int rade_batch_acq_refine(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, const rade_acq_refine_in *events_host, int n_events,
                          rade_acq_refined *out_host /* [n_events] */, double *dfine_host /* [n_events][80] or NULL */, void *stream);
int rade_acq_stats(const rade_acq_event *events, const rade_acq_refined *refined, int n_events, int n_hops, int Ntap, double fmax_target, double acq_time_target,
                   rade_acq_result *out);

/* ---- stored-file receiver: rx.py past the acquisition (rx.py:107-114 the input band-pass, :197-228 the normal run's refine, trim and mix, :253 the receiver, :260-276 the
 * BER alignment), every stream of a batch in one call each (rade_file.hip, rade_irx.hip).  Geometry: model19_check3's only, as for the acquisition. ------------------------
 * rade_batch_bpf_file: complex_bpf(101, Fs, bandwidth, centre, len(x)).bpf(x) of a whole file (dsp.py:63-102, its first and only call): zero memory of 100 samples;
 *   y[i] = conj(E[i]) sum_{t < 101} h[t] (x E)[i - 100 + t], E[i] = e^{-j alpha (i + 1)}, h and alpha the engine's own (rd_tables_fill: bpf_h; float32 as NumPy forms them).
 *   DEVIATION: E[i] is the complex64 nearest to e^{-j alpha (i + 1)} with the argument formed in double (as radae_amd/acq.py: complex_bpf and tests/acq_ref.py: bpf have
 *   it); the script forms the argument in float32 (np.exp(.., dtype = complex64)), which jitters the phase by up to an ulp of alpha i on long files.  Not reproduced.
 *   The mixers are complex64 products with every operation rounded on its own.  The FIR is the engine's one FIR arithmetic (rade_bpf_fir.h, shared with the receiver's input
 *   filter): per chunk of 1024 outputs the baseband window in two binary16 planes per component (hi + lo, 22 bits) under the power of two that puts the chunk's largest
 *   |component| into [2^7, 2^8), against the two planes of 2^10 h, on v_mfma_f32_16x16x32_f16: hi hi + hi lo + lo hi, each chain of four instructions (K = 32) in its own
 *   float32 accumulator, joined by two float32 additions.  Ahead of that a chunk is multiplied by the power of two that puts the larger of its own and the previous
 *   chunk's largest |component| into [1, 2), and its outputs by the inverse: both exact, so that 2^k x gives 2^k y bit for bit (barring overflow and underflow of
 *   binary32 itself) whatever the file's level.  A workgroup takes 8 chunks of one stream; the phases are a table made once per call for all streams.
 *   Error bound, counted from these roundings, per output against the exact value, relative to S[i] = sum_t |h[t]| |x[i - 100 + t]|.  ASSUMED, as for the acquisition: a
 *   matrix instruction returns its 33-term sum within 2^-23 of the sum of the terms' moduli.  The down mixer: E[i] within sqrt 2 x 2^-25, the product's six roundings 2 sqrt
 *   2 x 2^-24: 3.54 x 2^-24 = 0.22 x 2^-20.  The samples' two planes 2^-22, the taps' two planes 2^-22, the dropped lo lo product 2^-22: 0.75 x 2^-20 (component errors
 *   eps sum |h| |re|, eps sum |h| |im| give eps S in modulus).  The hi hi chain 4 x 2^-23 = 0.5 x 2^-20, the cross chains 8 x 2^-23 x 2^-10 = 0.001, the joining additions
 *   2 x 2^-24 = 0.125.  The up mixer, on |y| <= S: 0.22 again.  Sum 1.82, with 1.01 for the terms of second order and rounded up:
 *       |y^[i] - y[i]| <= RADE_FILE_BPF_EPS S[i] + RADE_FILE_BPF_TINY X,   RADE_FILE_BPF_EPS = 2 x 2^-20 = 1.9e-6,   X = the stream's largest |component|
 *   The second term is what binary16 underflow leaves: a plane entry below 2^-14 is rounded to a multiple of 2^-24, at most 2^-25 x 2^-7 = 2^-32 of the window's largest
 *   component per sample (sqrt 2 sum |h| = 2.9 of them) and 2^-25 x 2^-10 per tap (101 of them): under 2^-28 X; RADE_FILE_BPF_TINY = 2^-27.  tests/test_rx_file_gpu.py
 *   records how far below the bound the device stays.
 *   Contract: no device state (the phase table and the counts are scratch of the call, the engine's memory, sized on first use and when a call needs more); no atomics
 *   on outputs (identical calls give identical bits, and a stream's bits do not depend on the batch); y of stream b is written for exactly n_host[b] samples; x is read
 *   inside [0, n_host[b]) of the stream's row only and not written; both bases 8-byte aligned; any strides >= the counts.  The call SYNCHRONISES `stream` before it
 *   returns.  Refused with -1 before any launch and with nothing written: NULL h, x_dev, y_dev or n_host; a base not 8-byte aligned; a count negative or above either
 *   stride; y overlapping x (the extents first non-empty stream's first sample .. last non-empty stream's last sample of the two buffers intersect).
 * rade_file_plan: host only; where the script's normal run starts to demodulate.  The script advances one more frame after the acquiring hop k (rx = rx[Nmf:-1]; mf += 1,
 *   rx.py:186-187) BEFORE acquisition.refine: refine is called with t_abs = 960 (k + 1) + tmax and the stream length n - (k + 1) (every hop drops one tail sample).  [This
 *   is not radae_amd/acq.py: acquire(acq_test = False), which refines at 960 k + tmax, the --acq_test placement.]  With refine's absolute t and f: start = t - Ncp,
 *   n_left = n - (k + 1) - start, n_mf = (n_left // 192) // 5 (RADAE.receiver), freq = f or *freq_override (--freq_offset, rx.py:224-226).  Status: RADE_FILE_OK;
 *   RADE_FILE_NOT_ACQUIRED (hop < 0); RADE_FILE_REFINE_OUTSIDE (t < 0 or t + 960 + 160 > n - (k + 1): refine had no window inside the stream); RADE_FILE_EARLY
 *   (t - 960 (k + 1) < 32; DEVIATION: the script's negative slice start would wrap to the file's tail; not decoded); RADE_FILE_SHORT (n_mf < 2; DEVIATION: the
 *   demodulator needs two pilots; not decoded).  Every status but OK gives start 0, n_mf 0.  Returns -1 for NULL out, n < 0 or a value that is not finite.
 * rade_batch_rx_file: rx.py:223-253 with one fixed estimate per stream.  Stream b: samples from in_host[b].start; multiplied by e^{-j w m}, w = 2 pi freq / 8000 in double,
 *   m counted from start, phase and product formed in double and rounded once to complex64 (the script multiplies complex64 by complex128 and converts afterwards); a
 *   stream with freq == 0 is not touched.  Then exactly the arithmetic of rade_batch_rx_ideal (below) over the stream's own n_mf frames: the DFT window
 *   [Ncp + time_offset, + M), the same float32 DFT, do_pilot_eq, the last frame's slope, coarse_mag over the stream's own frames; with start 0, freq 0 and equal n_mf the
 *   two calls give the same bits.  z_hat_dev [B][3 max_mf][80]: rows past a stream's 3 n_mf are written as zeros, a stream with n_mf 0 gets all zeros.  features_out_dev
 *   (optional) [B][3 max_mf][feat]: rade_batch_decode over 3 max_mf steps after a reset; the decoder is causal, so a stream's rows below 3 n_mf do not depend on its zero
 *   tail (the rows behind are the decoder's answer to zeros).  Synchronises `stream`.  Returns max_mf.  Refused with -1, nothing written: NULLs; x_dev not 8-byte, z_hat_dev
 *   not 4-byte (with features_out_dev: 16-byte) aligned; max_mf < 1; with features_out_dev, 3 max_mf above the engine's decoder rows; time_offset outside [-Ncp, 0]; eq
 *   outside RADE_EQ_*; a stream with n_mf < 0, == 1 or > max_mf, start < 0, start + 960 n_mf > x_stride, or a freq that is not finite.
 * rade_batch_ber_align: rx.py:260-276.  Per stream and shift f = 0..19: z_f = z_ref[240 f:], n_syms = min(len(z_f), len(z_hat)), n_errors = #(-z_f z_hat > 0) over
 *   n_syms; one launch, grid (shift, stream), integer counts added in a fixed order.  n_errors_host [B][20]; -1 for a shift that leaves no reference symbol (DEVIATION:
 *   the script divides by zero there).  Lengths in floats.  Synchronises `stream`.  Refused: NULLs, a base not 4-byte aligned, a length negative or above its stride.
 * rade_ber_best: host only; BER_f = n_errors[f] / n_bits, n_bits = len(z_f) = n_ref - 240 f (the script's own denominator: what is left of the reference, NOT n_syms);
 *   the best is the first strict minimum below 1.  Returns its shift (-1: none) and its BER in *ber_out (1 when none). */
#define RADE_FILE_BPF_EPS (2.0 / 1048576.0)
#define RADE_FILE_BPF_TINY (1.0 / 134217728.0)
#define RADE_FILE_BPF_SPAN 8192                                   /* outputs per workgroup of the filter kernel: where its tests put their edge cases */
enum { RADE_FILE_OK = 0, RADE_FILE_NOT_ACQUIRED = 1, RADE_FILE_REFINE_OUTSIDE = 2, RADE_FILE_EARLY = 3, RADE_FILE_SHORT = 4 };
typedef struct { long long start; int n_mf; double freq; } rade_file_rx_in;
typedef struct { long long start; int n_mf; double freq; int status; } rade_file_plan_out;
int rade_batch_bpf_file(rade_batch *h, const void *x_dev, long x_stride, const int *n_host /* [B] */, void *y_dev, long y_stride, void *stream);
int rade_file_plan(long long n, int hop, long long t, double f, const double *freq_override /* or NULL */, rade_file_plan_out *out);      /* host only */
int rade_batch_rx_file(rade_batch *h, const void *x_dev, long x_stride, const rade_file_rx_in *in_host /* [B] */, int max_mf, int time_offset, int eq, int coarse_mag,
                       float *z_hat_dev /* [B][3 max_mf][80] */, float *features_out_dev /* [B][3 max_mf][feat] or NULL */, void *stream);
int rade_batch_ber_align(rade_batch *h, const float *z_ref_dev, long ref_stride, const long *n_ref_host /* [B] */, const float *z_hat_dev, long hat_stride,
                         const long *n_hat_host /* [B] */, long *n_errors_host /* [B][20] */, void *stream);
int rade_ber_best(const long *n_errors /* [20] */, long n_ref, double *ber_out /* or NULL */);      /* host only */

/* ---- Watterson / Doppler-spread sample generator on the device (doppler_spread.m:7-50, multipath_samples.m:10-31):
 * per stream two independent paths G1, G2 = complex Gaussian noise at the low rate Fs/low_ratio through the
 * n_taps Gaussian-PSD FIR (taps designed by the caller, e.g. radae_amd/channel_tools.py), linearly interpolated to
 * Fs, scaled by hf_gain = 1/sqrt(var G1 + var G2).
 * noise_low_dev : optional [B][2][n_low + n_taps] complex64 unit-variance-per-component input noise with
 *                 n_low = max(ceil(n_out / low_ratio), 2); NULL: Philox from seed
 * G_out_dev     : [B][n_out][2] complex64, the layout rade_channel_params.G_dev takes.  Returns n_out or <0. */
int rade_batch_multipath_gen(rade_batch *h, const float *fir_taps_host, int n_taps, int low_ratio, int n_out,
                             const void *noise_low_dev, unsigned long long seed, void *G_out_dev, void *stream);
/* The rate-Rs channel matrix multipath_samples.m:33-40 derives from the same Doppler samples (what `multipath_samples("lmr60", 8000, 2000, 1, ...)` writes for the
 * BBFM model, BBFM.md:37, and the `h_*.f32` files of the rate-Rs RADE model): H[b][t][c] = G1[t M] + G2[t M] exp(-j 2 pi c delay Rs), M = Fs / Rs = fs_over_rs,
 * as magnitudes (float32 [B][n_sym][Nc], the default file form) or complex (want_complex: [B][n_sym][Nc][2]).  G_dev [B][n_g][2] complex64 as
 * rade_batch_multipath_gen leaves it (hf_gain included), n_g > (n_sym - 1) M.  Returns n_sym or <0. */
int rade_batch_multipath_h(rade_batch *h, const void *G_dev, int n_g, int fs_over_rs, int n_sym, int Nc, float delay_s, float Rs, int want_complex,
                           float *H_out_dev, void *stream);

/* ---- the channel and the Doppler generator in pieces: endless streams through fixed-size calls (rade_chanp.hip) ------------------------------------------------
 * rade_batch_channel and rade_batch_multipath_gen above need a whole utterance: they normalise by a power / a variance measured over all of it.  The two calls below
 * are separate entry points with their own arithmetic, in which every quantity is a pure function of the ABSOLUTE sample index n (>= 0, up to 2^62): they keep no
 * state on the device, and a stream cut into pieces anywhere equals the stream in one piece, bit for bit.  Nothing of the whole-utterance calls changes.
 * DEVIATIONS from the reference (multipath_samples.m, radae.py:529-589), all three so that a piece needs nothing it cannot know:
 *   1. hf_gain is the EXPECTED value 1 / sqrt(E var G1 + E var G2) (rade_multipath_gain), not 1 / sqrt of the variance realised by one sequence; and the channel
 *      multiplies by a gain the caller gives (1 by default) instead of sqrt(tx power / multipath power) measured over the utterance.  With the expected hf_gain
 *      E |G1|^2 + E |G2|^2 = 1, so no power pass is needed.  Over 10 s the realised gain scatters by +-10 % (mpp) and up to a factor of 2 (mpg) around the expected
 *      one -- which is why a piece cannot measure it; over 8 seeds x 1200 s the mean ratio of realised to expected was 0.9993 (mpg), 1.0017 (mpp), 1.0022 (mpd).
 *   2. the phase of the frequency offset is a 64-bit integer fraction of a turn, not a float32 angle: its accuracy does not decay with n.
 *   3. the Doppler sequence has no end: no clamp of the interpolation index, no extrapolation of a last block.
 *
 * rade_batch_multipath_piece: (G1, G2) of absolute indices [n0[b], n0[b] + n_out[b]) into G_out_dev [B][g_stride][2] complex64 (g_stride in pairs, >= every n_out).
 *   Draws     x_p[xi] = Box-Muller of words 0-1 of Philox4x32-10, counter (xi & 0xffffffff, 2 b + p, 1, xi >> 32), key as in rade_channel_params: path p of stream b,
 *             low-rate index xi >= 0 (64 bit).  This is rade_batch_multipath_gen's draw for xi < 2^32.
 *   FIR       y_p[i] = sum_{k = 0..n_taps-1} (double)taps[k] x_p[i + n_taps - k], in double, k ascending (rade_batch_multipath_gen's expression).
 *   To Fs     i0 = n div low_ratio (integers), fr = (double)(n - i0 low_ratio) / (double)low_ratio, g_p[n] = y_p[i0] + (y_p[i0 + 1] - y_p[i0]) fr,
 *             G_p[n] = (float)(hf_gain g_p[n]) per component.
 *   hf_gain   a double given by the caller; 0 = rade_multipath_gain(taps, n_taps) = 1 / sqrt(2 ((2/3) R0 + (1/3) R1)), R0 = 2 sum t_k^2, R1 = 2 sum t_k t_{k+1}, t the
 *             float32 taps widened to double: the expected variance of two independent linearly interpolated paths (the interpolation weights (1 - fr, fr) average to
 *             E[(1 - fr)^2 + fr^2] = 2/3 and E[2 fr (1 - fr)] = 1/3 over a low-rate step).
 *   1 <= n_taps <= 256, low_ratio >= 1 (the presets give 16 (lmr60), 400, 800, 8000).  Returns 0.
 *   Refused (-1, before any launch, nothing written): NULL or misaligned (8 bytes) pointers, n_taps or low_ratio out of range, taps or hf_gain not finite, hf_gain < 0,
 *   a negative count or n0, n0 + n_out above 2^62, g_stride shorter than a row.
 *
 * rade_batch_channel_piece: output i of row b of rx_out_dev is the received sample of absolute index n = n0[b] + i, 0 <= i < n_out[b].
 *   tx[b][g] is the transmit sample of absolute index in_base[b] + g, 0 <= g < n_in[b]; transmit samples in front of index 0 or outside the row read as zero, and
 *   nothing outside the row is read.  G[b][g] is (G1, G2) of absolute index g_base[b] + g, 0 <= g < n_g[b] (G_dev [B][g_stride][2]); with G_dev the row must cover
 *   [max(0, n0 - 16), n0 + n_out), else the call is refused.
 *     m[n]  = tx[n] G1[n] + tx[n - 16] G2[n - 16] (the second term when n >= 16; the complex products and the sum of rade_batch_channel); m = tx[n] without G_dev
 *     v     = m gain_b                                                 (float32; 0 is taken as 1)
 *     v     = v cis(ph[n] >> 32) when freq_offset != 0 or df_dt != 0:  ph[n] = (n + 1) f0q + T(n) dq mod 2^64, T(n) = n (n + 1) / 2 with the even factor halved first
 *             (exact mod 2^64 for every n < 2^62), f0q = (uint64) llrint(turns 2^64), dq = (uint64) llrint(df_dt / 8000^2 2^64), both made on the host in double; the sum
 *             is inclusive (the reference's cumsum); cis is the 32-bit phasor of rade_batch_fm_mod.  turns, the offset in turns per sample, is the rate rade_batch_channel
 *             turns at: with a drift freq_offset / 8000 in double (its closed form), WITHOUT one the reference's float32 omega = ((freq_offset * 2) * (float)pi) / 8000
 *             over 2 pi (radae.py sums a float32 tensor) -- up to 2e-7 relative from freq_offset / 8000 (5e-8 at 10 Hz: 8e-7 rad after 1,920 samples, which would separate
 *             a piece from the whole call by more than the float32 rounding of the whole call's phase)
 *     v    += sigma_b noise[b][i]                                      explicit: noise_dev complex64, dense [B][max n_out]
 *     or    generated (noise_dev NULL, seed != 0): Philox counter (P & 0xffffffff, b, 0, P >> 32), P = n >> 1, words 0-1 for even n and 2-3 for odd n (rade_batch_channel's
 *             draw for n < 2^33); RADE_CHANP_NOISE_COMPLEX: sigma_b 0.70710678f g per component; RADE_CHANP_NOISE_REAL: sigma_b g.x on the real part only (the rule of
 *             inference.py:277-284 for the noise-only lead and tail)
 *     v    += sine_amp cis(2 pi frac(n sine_freq / 8000)), then v rx_gain  (as rade_batch_channel; rx_gain 0 is taken as 1)
 *   Silence between overs, the EOO frame (rade_batch_tx_eoo) and lead-in noise are the CALLER's transmit samples and piece boundaries: there is no n_pre, n_post or
 *   with_eoo here.  rade_batch_channel with generated noise, no G and no frequency offset equals three piece calls bit for bit (real noise over the lead, complex over
 *   the signal with in_base = n_pre, real over the tail).
 *   sigma, freq_offset, df_dt, gain, n0, in_base, g_base: the scalar of the structure for every stream, or a [B] host array when the _host member is not NULL; stream b
 *   of a call with arrays gets what a call with its values as scalars gives it, bit for bit.  The per-stream records are copied to the device ahead of the launch (the
 *   call synchronises `stream` once for that).  Any engine; no model, encoder or receiver state is touched.  Returns 0.
 *   Refused (-1, before any launch, nothing written): NULL or misaligned (8 bytes) pointers, negative counts, n0, in_base or g_base, any of those (or n0 + n_out) above
 *   2^62, a stride shorter than its row, a G row that does not cover its window, values that are not finite, |freq_offset| > 2000, |df_dt| > 2000 * 8000, an unknown
 *   noise mode, sigma < 0.
 * Buffers: tx_dev (complex64; tx_stride >= every n_in, checked) and p->G_dev (complex64 pairs; g_stride >= every n_g, checked) in, read inside the stream's n_in / n_g
 *   elements only and never written; p->noise_dev (complex64) dense [B][max n_out]; rx_out_dev (complex64; rx_stride >= every n_out, checked): n_out[b] samples of row b
 *   are written and nothing else, two samples as one 16-byte word where the row puts an even-n sample on a 16-byte boundary, single samples otherwise and at an odd head
 *   or tail (any rx_stride, any parity of n0 and n_out, element alignment).  rade_batch_multipath_piece's G_out_dev: n_out[b] pairs of row b, 16-byte words when the base
 *   is 16-byte aligned, else 8-byte ones. */
enum { RADE_CHANP_NOISE_COMPLEX = 0, RADE_CHANP_NOISE_REAL = 1 };
typedef struct {
    float sigma, freq_offset, df_dt, gain;                      /* every stream's value where the _host array below is NULL; Hz, Hz / s; gain 0 = 1 */
    long long n0, in_base, g_base;                              /* likewise: absolute index of the first output, of tx[b][0], of G[b][0] */
    const float *sigma_host, *freq_offset_host, *df_dt_host, *gain_host;          /* [B] or NULL */
    const long long *n0_host, *in_base_host, *g_base_host;      /* [B] or NULL */
    const void *G_dev; long g_stride; const int *n_g_host;      /* complex64 [B][g_stride][2] and the [B] pairs each row holds, or NULL: no two-path model */
    const void *noise_dev;                                      /* complex64 [B][max n_out] unit noise, or NULL: generated from seed; seed 0 = no noise */
    unsigned long long seed;
    int noise_mode;                                             /* RADE_CHANP_NOISE_COMPLEX / _REAL (generated noise only) */
    float sine_amp, sine_freq, rx_gain;
} rade_channel_piece_params;
int rade_batch_multipath_piece(rade_batch *h, const float *fir_taps_host, int n_taps, int low_ratio, double hf_gain, unsigned long long seed,
                               const long long *n0_host /* [B] or NULL = 0 */, const int *n_out_host /* [B] */, void *G_out_dev, long g_stride, void *stream);
int rade_batch_channel_piece(rade_batch *h, const void *tx_dev, long tx_stride, const int *n_in_host, void *rx_out_dev, long rx_stride, const int *n_out_host,
                             const rade_channel_piece_params *p, void *stream);
double rade_multipath_gain(const float *fir_taps, int n_taps);      /* host only; -1: NULL, n_taps outside 1..256, taps that are not finite or all zero */
float rade_sigma_from_EbNodB(float EbNodB);
/* bottleneck 1 (radae.py:574-576): sigma = (EbNo M)^-0.5, M = 160 */
float rade_sigma_from_EbNodB_bn1(float EbNodB);
/* rate Rs, bottleneck 3 (radae.py:627-630): sigma = M / sqrt(2 Nc EbNo) / sqrt(2), M = 160, Nc = 20 (12.66 at 3 dB: the encoder drives |tx_sym| to about M / sqrt(Nc)) */
float rade_sigma_from_EbNodB_rs3(float EbNodB);

/* ---- receive --------------------------------------------------------------------------------
 * rx_dev + b*rx_stride points at the first sample stream b has NOT yet consumed; n_avail_host[b]
 * samples are readable there.  Each stream consumes whole do_radae_rx calls (rade_nin() samples
 * each) while enough samples remain and fewer than max_calls calls were made in this invocation.
 * features_out_dev: stream b at + b*feat_stride floats; each valid modem frame appends 432 floats.  feat_stride / 432 is the
 *   stream's capacity in frames: a stream that has filled it makes no further call in this invocation (status consumed < available),
 *   so nothing is ever written past a stream's rows; the caller continues from rx_dev + consumed with fresh rows.
 * eoo_out_dev: [B][180] soft bits of the most recent end-of-over frame (NULL to skip).
 * status_host: [B] records filled on return (the call synchronises `stream`). */
typedef struct {
    int consumed;         /* samples consumed by this invocation */
    int n_calls;          /* do_radae_rx calls made */
    int n_valid;          /* calls that produced features (432 floats each) */
    int has_eoo;          /* an end-of-over frame was decoded */
    int nin;              /* samples the next call needs (rade_nin) */
    int sync;             /* rade_sync */
    int snr_dB;           /* rade_snrdB_3k_est */
    int state;            /* 0 search 1 candidate 2 sync */
} rade_rx_status;
int rade_batch_rx(rade_batch *h, const void *rx_dev, long rx_stride, const int *n_avail_host, int max_calls,
                  float *features_out_dev, long feat_stride, float *eoo_out_dev, rade_rx_status *status_host,
                  void *stream);
void rade_batch_rx_reset(rade_batch *h);
/* stream-ordered reset of encoder and receiver state of every stream (a new batch of utterances starts) */
void rade_batch_reset(rade_batch *h, void *stream);
/* seed of the documented LCG that picks the 48 rows check_pilots refreshes (dsp.py:291-295 uses an
 * unseeded np.random.randint); seeds_host[B] or NULL for all-ones */
void rade_batch_rx_set_lcg(rade_batch *h, const unsigned *seeds_host);

/* ---- the ideal-timing ("genie") receiver of RADAE.forward / RADAE.receiver (radae.py:312-420, :590-657) -------------------------------
 * Known timing: every stream's n_mf modem frames start at rx_dev + b * rx_stride (n_mf * 960 samples readable, n_mf >= 2).  Per stream the known frequency offset is
 * optionally removed (rx * conj(lin_phase), the phase recurrence of rade_batch_channel, so that its output cancels), the DFT window [Ncp + time_offset, Ncp + time_offset + M)
 * of each symbol goes through the 160 -> 30 DFT, the pilots are estimated (eq) and interpolated in phase between a frame's pilot and the next one's (the last frame
 * keeps the reference's last slope), and the data symbols are demapped to z_hat_dev [B][3 n_mf][80].  coarse_mag divides by the RMS pilot magnitude (times
 * |P[0]| / pilot_gain unless the engine has RADE_BATCH_TX_LINEAR).  With z_ref_dev ([B][3 n_mf][80]) n_errors_host[b] = #(-z * z_hat > 0) (ber_test; the call then
 * synchronises `stream`).  features_out_dev [B][3 n_mf][feature width of the blob]: the stateless decoder (rade_batch_decode with reset_state = 1; 3 n_mf <= 3 max_tx_mf),
 * or NULL.  The streaming receiver's state is not touched.  Returns n_mf or <0. */
enum { RADE_EQ_LS = 0, RADE_EQ_MEAN6 = 1, RADE_EQ_MEAN_ALL = 2, RADE_EQ_NONE = 3 };
typedef struct {
    int time_offset;                  /* samples, -32..0 (inference.py --time_offset) */
    int eq;                           /* RADE_EQ_LS (--eq_ls), RADE_EQ_MEAN6 (the default of RADAE), RADE_EQ_MEAN_ALL (per_carrier_eq = False), RADE_EQ_NONE (no --pilot_eq) */
    int coarse_mag;                   /* --coarse_mag (ignored with RADE_EQ_NONE, as in the reference) */
    const float *freq_offset_host, *df_dt_host;   /* [B] Hz, Hz/s: --correct_freq_offset; NULL = no correction (df_dt NULL = 0); a stream with freq_offset 0 is not corrected */
    const float *z_ref_dev; long *n_errors_host;  /* optional BER count */
} rade_ideal_rx_params;
int rade_batch_rx_ideal(rade_batch *h, const void *rx_dev, long rx_stride, int n_mf, const rade_ideal_rx_params *p,
                        float *z_hat_dev, float *features_out_dev, void *stream);

/* ---- scoring ----------------------------------------------------------------------------------
 * loss.py:find_loss (:64-91) over distortion_loss (radae_base.py:50-68, first 20 features), every stream in one launch.
 * features_dev + b*f_stride: n_in_host[b] rows of f_row floats (f_row >= 20), the transmitted features;
 * hat_dev + b*h_stride: n_hat_host[b] rows of h_row floats (h_row >= 20), the decoded features
 *   (rade_batch_rx's features_out is h_row = 36 with 12 rows per valid modem frame).
 * For a stream with 0 < n_hat <= n_in: loss_host[b] = min of distortion_loss(features[s : s + n_hat], hat) over s = 0 and
 *   s in [0, n_in - n_hat), the reference's range: s = n_in - n_hat is never tried. The first of equal values wins.
 *   start_host[b] = that s (acq_time = 0.01 s * start). Any other stream: loss NaN, start -1.
 *   Bit-equal to the reference's float32 frame terms summed in double in frame order (rade_loss.hip).
 * frame_loss_dev, optional, [B][fl_stride] float32: loss.py:83-88's per-frame curve, distortion_loss(features[s + f], hat[f])
 *   for f in [0, n_hat - s) (fl_stride >= every scored n_hat; other entries are not written).
 * Synchronises `stream`. Returns the number of streams scored, or < 0 on bad arguments. */
int rade_batch_loss(rade_batch *h, const float *features_dev, long f_stride, int f_row, const int *n_in_host,
                    const float *hat_dev, long h_stride, int h_row, const int *n_hat_host,
                    double *loss_host, int *start_host, float *frame_loss_dev, long fl_stride, void *stream);

/* per-call trace record (tests): mirrors what radae_rxe.py prints per frame at -v 2 */
typedef struct {
    int state_before, state_after, nin_before, nin_after, ret, tmax, f_ind_max, valid_count;
    int uw_errors, synced_count, snr_int, pad;
    double fmax, Dthresh, Dtmax12, Dtmax12_eoo;
    float snrdB_3k_est; float pad2;
} rade_rx_trace;
/* copies up to max_calls records + 240-float z_hat rows per call of stream b to host; returns #calls traced */
int rade_batch_rx_get_trace(rade_batch *h, int b, rade_rx_trace *out, float *z_hat_out, int max_calls);

/* Host-side wait policy of rade_batch_rx (the one call that waits for its stream): hipStreamSynchronize spins, which is right while every engine's
 * host thread has a core; when more engines are open in the process than the process has CPUs (affinity mask and cgroup quota: 8 GPUs x 3 batches
 * in flight = 24 threads under a 16-core quota) the wait SLEEPS instead (naps between hipEventQuery calls: rade_engine.c sleep_until_event; hipEventSynchronize on a hipEventBlockingSync event was measured to burn a core per waiting thread on this runtime).  $RADE_SYNC=spin|block overrides; $RADE_SYNC_PEERS=n: n processes with as many engines each share these CPUs (one process per GPU: the count is engines x n).
 * rade_sync_policy is the rule itself (1 = block); rade_host_cpu_quota what it is fed with; rade_batch_sync_counts what an engine did so far. */
double rade_host_cpu_quota(void);
int rade_sync_policy(int engines_open, double cpu_quota);
void rade_batch_sync_counts(const rade_batch *h, long *blocking, long *spinning);
/* test aid: the band-pass filtered samples (complex_bpf.bpf, dsp.py:63-102) the receiver of the most recent rade_batch_rx invocation read for
 * stream b -> out_host [n] complex64 (host memory); returns the number copied, < 0 on error */
int rade_batch_rx_filtered(rade_batch *h, int b, void *out_host, int n);
/* measurement aid: shader-clock cycles each stream's workgroup spent in the most recent receiver launch -> out_host[B]; returns B */
int rade_batch_rx_stream_cycles(rade_batch *h, long long *out_host);

/* ---- measurement hook (bench.py): per-kernel-class HIP-event timing, off by default ---------- */
enum { RADE_PROF_GEMM = 0, RADE_PROF_SCAN, RADE_PROF_MOD, RADE_PROF_CHAN, RADE_PROF_SYNC, RADE_PROF_BPF, RADE_PROF_NCLASS };
void rade_batch_profile(rade_batch *h, int enable);
/* accumulated since enable: device milliseconds, algorithmic FLOPs, launches */
int rade_batch_profile_get(rade_batch *h, int cls, double *ms, double *work, long *launches);
/* every profiled launch of a class as [start, end] in ms after a caller-supplied hipEvent_t (so that launches of several engines, which
 * may overlap on the device, can be put on one time axis): set the reference before enabling, read after disabling; returns the count */
void rade_batch_profile_ref(rade_batch *h, void *ref_event);
int rade_batch_profile_intervals(rade_batch *h, int cls, float *t0_ms, float *t1_ms, int max);

/* ---- several GPUs from one host process (BASELINE.json configs[3]: 2048 utterances over 8 MI355X) -------------------
 * The n_streams_total independent utterances are sharded contiguously over the devices of device_mask (bit g = HIP device g),
 * ceil(total / n_dev) per device; there is no data-path collective.  rade_multi_open reads the DNNw blob once, moves it to the
 * other devices with ONE ncclBroadcast (RCCL over xGMI; librccl.so is bound at run time and only required for n_dev > 1) and opens
 * one engine per device (one host thread each).  Per-device work is driven through the ordinary rade_batch_* calls on
 * rade_multi_engine(m, i); rade_multi_foreach runs a callback on one host thread per device; rade_multi_allreduce_sum adds job
 * statistics (frames, loss sums, bit errors) with ONE ncclAllReduce.  NULL / <0 on failure, message on stderr. */
typedef struct rade_multi rade_multi;
typedef int (*rade_multi_fn)(int i, rade_batch *engine, int first_stream, int n_streams, void *arg);
rade_multi *rade_multi_open(const char *blob_path, int n_streams_total, int max_tx_mf, unsigned long long device_mask, int flags);
void rade_multi_close(rade_multi *m);
int rade_multi_n_devices(const rade_multi *m);
const char *rade_multi_transport(const rade_multi *m);            /* "rccl" or "none (single device)" */
rade_batch *rade_multi_engine(rade_multi *m, int i, int *device, int *first_stream, int *n_streams);
void rade_multi_shard(int n_total, int n_dev, int i, int *first, int *count);      /* the sharding rule, also usable on its own */
int rade_multi_foreach(rade_multi *m, rade_multi_fn fn, void *arg);
int rade_multi_allreduce_sum(rade_multi *m, const double *per_device /* [n_dev][n] */, int n, double *out /* [n] */);

/* ---- single-carrier modem for BBFM symbols ------------------------------------------------
 * Batched form of the reference's `single_carrier` class (radae/dsp.py:579-860; drivers sc_tx.py:58-75,
 * sc_rx.py:83-112): BPSK at Rs symbols/s, Fs = 4 Rs, 16-symbol frame-sync word + 80 payload symbols per frame,
 * 24-tap root-Nyquist filters (gen_rn_coeffs, dsp.py:532-562), fine timing from the symbol-rate line of the
 * envelope, squared-symbol phase tracker, frame-sync state machine.  One independent modem per stream; all state
 * lives on the device between calls. */
typedef struct rade_sc rade_sc;
typedef struct {          /* end-of-call state of one stream */
    int n_frames;         /* frames demodulated by this call */
    int consumed;         /* samples consumed */
    int state;            /* 0 search, 1 sync */
    int nin;              /* samples the next frame needs: 96 M - 1, 96 M or 96 M + 1 (dsp.py:697-702) */
    int fs_s;             /* frame-sync position inside the two-frame symbol buffer */
    float g;              /* amplitude normalisation from the sync word (dsp.py:805-806) */
    float max_cs_re, max_cs_im, norm_rx_timing, phase_ambiguity;
} rade_sc_status;
typedef struct {          /* per-frame record, what sc_rx.py prints at -v 2 */
    int state, nin, fs_s, pad;
    float norm_rx_timing, g, max_cs_re, max_cs_im, phase_ambiguity, pad2[3];
} rade_sc_frame;
/* Rs, Fs, fcentreHz, alpha as single_carrier.__init__ (dsp.py:581); Fs must equal 4 Rs.  NULL without a GPU. */
rade_sc *rade_sc_open(int n_streams, double Rs, double Fs, double fcentreHz, double alpha, int device);
void rade_sc_close(rade_sc *h);
void rade_sc_reset(rade_sc *h);
int rade_sc_n_streams(const rade_sc *h);
int rade_sc_n_tx_out(const rade_sc *h);       /* 384 samples per frame */
int rade_sc_nin_max(const rade_sc *h);        /* 385 */
int rade_sc_n_payload(const rade_sc *h);      /* 80 */
void rade_sc_rrc(const rade_sc *h, double *taps_out /* [24] */);
/* single_carrier.tx (dsp.py:636-662) for n_frames frames per stream: symbs_dev [B][n_frames][80] float ->
 * iq_out_dev [B][iq_stride] complex64, n_frames * 384 samples each.  Returns samples per stream or -1. */
int rade_sc_tx(rade_sc *h, const float *symbs_dev, int n_frames, void *iq_out_dev, long iq_stride, void *stream);
/* single_carrier.rx (dsp.py:773-829) over every whole frame in the first n_avail samples of each stream (at most
 * max_frames): payload_out_dev [B][max_frames][80] complex64 = the returned symbols, zhat_out_dev [B][max_frames][80]
 * = g * Re(payload) where the modem is in sync after the frame, else 0 (sc_rx.py:99-101); frames_out_dev
 * [B][max_frames]; any of the three may be NULL.  status_host[B] is filled after a stream synchronisation. */
int rade_sc_rx(rade_sc *h, const void *rx_dev, long rx_stride, int n_avail, int max_frames, void *payload_out_dev, float *zhat_out_dev,
               rade_sc_frame *frames_out_dev, rade_sc_status *status_host, void *stream);

/* ---- training the decoder (radae_amd/csrc/rade_train.hip, rade_train.c) ------------------------------------------------------------------------------------------
 * One training step of the reference's CoreDecoder (radae_base.py:291-354, the stateless whole-sequence form train.py:257-263 uses) for B sequences of T latent rows
 * at once, in float32: forward with saved activations, distortion_loss (radae_base.py:50-68) and its gradient, back-propagation through time, and Adam
 * (train.py:147-150: betas (0.8, 0.95), eps 1e-8).  Zero GRU state and zero conv history at the start of every sequence.  A handle of its own, like rade_sc: it needs
 * no engine and no blob, and owns the activation workspace for max_B x max_T rows.  The CALLER owns four flat float32 device buffers -- parameters, gradients, Adam's
 * m and v -- of rade_train_n_floats() floats each, laid out by the table rade_train_param returns: entry i has a name (that of dnnw.Model's decoder member:
 * "dec_dense1.w", "dec_gru[0].w_ih", "dec_glu[0].w", "dec_conv[0].w", "dec_output.b", ...), an offset in floats and a row-major shape rows x cols in torch's orientation
 * ([out][in]; gate order r, z, n; a conv weight [32][in][2] has cols = 2 in, tap 0 the older row; a bias has cols = 1).
 * Deviations from the reference, as everywhere in this library: the uniform +-1/254 noise of n() is left out and its clamp kept (the identity here: every argument lies
 * in [-1, 1]); the GLU's effective weight is the parameter.  The encoder and the channel's backward pass are not here: dz_hat is what they would be handed.
 * Buffers: all dense, element (4-byte) alignment, loss_dev 8-byte; z_hat_dev [B][T][80], features_hat_dev / dfeatures_hat_dev [B][4 T][21] (= [B][T][84]),
 * features_dev [B][4 T][n_features], dz_hat_dev [B][T][80], loss_dev [B + 1] doubles: loss_by_batch, then their mean.  A call writes the documented extent of its
 * outputs and nothing else of the caller's memory, never an input.  Every call is stream-ordered on `stream` and returns 0, -1 for an argument it refuses (NULL, B or T
 * outside [1, max], a misaligned pointer, a call out of sequence) before any launch and with nothing written, -2 for a failed launch.  Results depend on B, T and the
 * inputs only (fixed summation order, no atomics): two runs give the same bits, sequence b's features_hat and dz_hat rows do not depend on the other sequences of the
 * batch, and a call below the handle's capacity gives the bits of a handle opened at that size. */
typedef struct rade_train rade_train;
rade_train *rade_train_open(int max_B, int max_T, int n_features /* 20 | 21 */, int device);      /* NULL without a GPU or for a bad argument; max_B max_T <= 2^21 */
void rade_train_close(rade_train *h);
long rade_train_n_floats(void);
int rade_train_n_params(void);
int rade_train_param(int i, const char **name, long *offset, int *rows, int *cols);                 /* any output may be NULL; -1 for i outside the table */
/* forward: saves the concat buffer and per GRU layer r, z, n, W_hn h + b_hn, h and the GLU's sigmoid.  features_hat_dev may be NULL (the handle keeps its own copy). */
int rade_train_dec_forward(rade_train *h, const float *params_dev, const float *z_hat_dev, int B, int T, float *features_hat_dev, void *stream);
/* the saved concat buffer x [B][T][736] of the last forward call (layout: tests/core_ref.py:8-9) */
int rade_train_saved_x(rade_train *h, float *x_out_dev, void *stream);
/* the loss of the last forward call's features_hat against features_dev, and d total / d features_hat (kept in the handle; dfeatures_hat_dev may be NULL).
 * loss_by_batch[b] is the mean of its frames' float32 terms, added in double in frame order; total is the mean of loss_by_batch in stream order. */
int rade_train_loss(rade_train *h, const float *features_dev, float *dfeatures_hat_dev, double *loss_dev, void *stream);
/* backward of the last forward call: grads_dev (all of it is written) and dz_hat_dev (may be NULL).  dfeatures_hat_dev NULL: the gradient rade_train_loss left. */
int rade_train_dec_backward(rade_train *h, const float *params_dev, const float *dfeatures_hat_dev, float *grads_dev, float *dz_hat_dev, void *stream);
/* one Adam update of all rade_train_n_floats() elements.  The caller forms in double lr = lr0 / (1 + decay step) and the corrections 1 - beta^step (step from 1). */
int rade_train_adam(rade_train *h, float *params_dev, const float *grads_dev, float *m_dev, float *v_dev, double lr, double bias_correction1, double bias_correction2, void *stream);
/* forward, loss, backward and Adam in one call */
int rade_train_dec_step(rade_train *h, float *params_dev, float *grads_dev, float *m_dev, float *v_dev, const float *z_hat_dev, const float *features_dev, int B, int T,
                        double *loss_dev, double lr, double bias_correction1, double bias_correction2, void *stream);
/* Time per phase by HIP events (tools/time_train.py).  rade_train_profile(h, 1) starts recording a pair of events around each phase's launches (at most 512 pairs
 * between two reads), 0 stops it; rade_train_profile_get waits for the recorded work, adds the milliseconds per phase into ms_out[6] -- forward GEMMs, forward scans,
 * loss, backward scans, backward GEMMs with the activation derivatives and the folds, Adam -- starts over, and returns the number of intervals read. */
int rade_train_profile(rade_train *h, int on);
int rade_train_profile_get(rade_train *h, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif
