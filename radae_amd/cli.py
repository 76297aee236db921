"""stdin / stdout filters with the command lines of the reference's Python tools:

    python -m radae_amd.cli txe [--txbpf] [--bypass_enc] [--eoo_data_test] [--model_name BLOB] [--fs HZ] [--int16_real SCALE]
                                                                                                     features.f32 (or z.f32) -> IQ.f32 (or I.int16)  /root/reference/radae_txe.py:146-180
    python -m radae_amd.cli rxe [--bypass_dec] [--disable_unsync S] [--foff_err HZ] [--eoo_data_test] [--no_stdout] [-v N] [--model_name BLOB] [--fs HZ] [--int16 | --int16_iq]
                                                                                                     IQ.f32 (or .int16) -> features.f32 (or z_hat.f32)  /root/reference/radae_rxe.py:332-371

    python -m radae_amd.cli inference MODEL features.f32 features_hat.f32 --rate_Fs --EbNodB .. [--g_file g.f32] --write_rx rx.f32 [...]    the channel-simulation run of inference.py (rate Fs)
    python -m radae_amd.cli inference MODEL features.f32 features_hat.f32 --bottleneck 3 --auxdata --EbNodB .. [--h_file h.f32] [--mp_test] [--phase_offset rad]          the same without --rate_Fs: the rate-Rs channel
    python -m radae_amd.cli multipath_samples mpp 8000 50 30 10 h.f32 g.f32                                                      multipath_samples.m
    python -m radae_amd.cli bbfm_inference MODEL features.f32 features_hat.f32 [--CNRdB ..] [--h_file h_lmr60.f32] [--write_latent z.f32]    bbfm_inference.py
    python -m radae_amd.cli analog_fm IN.s16 OUT.s16 CNRdB [--seed N]                                                             analog_bbfm.sh:37-43 from the 8 kHz int16 file onward
    python -m radae_amd.cli est_cno RX.f32 [--window_time S] [--flow HZ] [--fhigh HZ]                                              est_CNo.py (without --plots); the periodograms on the device
    python -m radae_amd.cli est_snr [--snrdB X] [--single | --sequence] [--h_file F] [-T S] [--Nt N] [--test_S1] [--eq_ls] [-c C] [-m M] [--save_text F] [--seed N]    est_snr.py (without --plots): every trial in one device call
    python -m radae_amd.cli rx RX.f32 [--no_bpf] [--acq_test] [--fmax_target HZ] [--acq_time_target S] [--write_Dt FILE]             rx.py --pilots up to the acquisition (no decoding): every frame's pilot search in one device call
    python -m radae_amd.cli chirp OUT.f32 NSEC [--flow HZ] [--fhigh HZ] [--amp A]                                                  chirp.py (host)
    python -m radae_amd.cli specgram IN OUT.png [--fmin HZ] [--fmax HZ]                                                            plot_specgram.m at 8 kHz: the transforms and levels on the device, a grey-scale PNG
    python -m radae_amd.cli train_decoder MODEL z_hat.f32 features.f32 OUT.bin [--sequence-length 256] [--batch-size 32] [--epochs N] [--lr] [--lr-decay-factor] [--auxdata] [--seed N]
                                                                                                     the decoder's half of train.py on received latents: forward, loss, BPTT and Adam on the device (rade_train_*)
    python -m radae_amd.cli do_plots RX.f32 [--win N --step N] [--int16 GAIN] [--save_text F]                                      radae_plots.m: do_plots' two printed lines: Pav, PAPR, pilot PAPR, 99 % bandwidth (Welch spectrum and sums on the device)

so that the reference's shell pipelines (`cat features_in.f32 | python3 radae_txe.py > rx.f32`, `cat rx.f32 | python3 radae_rxe.py > features_out.f32`: CMakeLists.txt:300-420) run with
`python3 -m radae_amd.cli txe|rxe` in their place; `--fs 48000` (or 44100, ..) takes the place of the `sox .. -r 8000` stage of the off-air pipelines (radae_rx.sh:33,39): the
rate conversion runs on the device (rade_batch_rate_convert).  Everything computes in libradehip.so on the GPU (radae_amd/api.py over include/rade_api.h; the bypass modes over a one-stream
batched engine); `--model_name` takes a DNNw blob (the reference's `.pth` checkpoints are not in its tree), default weights/model19_check3.bin.  `--noauxdata` is not offered: model19_check3 has the aux symbol.
"""
from __future__ import annotations

import argparse
import struct
import sys

import numpy as np

from . import api


def _ratio(fs_out: int, fs_in: int):
    """(L, M) of a conversion from fs_in to fs_out Hz, reduced"""
    from math import gcd
    if fs_out < 1 or fs_in < 1:
        raise SystemExit("radae_amd.cli: --fs takes a sample rate in Hz")
    g = gcd(fs_out, fs_in)
    return fs_out // g, fs_in // g


class _RateIn:
    """stdin at another rate than the modem's: reads what the next receiver call needs, converts it on the device (engine.RateConverter) and hands out 8 kHz samples"""

    def __init__(self, eng, inp, fs, int16, int16_iq):
        import torch
        from . import engine
        self.torch, self.inp = torch, inp
        self.L, self.M = _ratio(8000, fs)
        self.rc = engine.RateConverter(eng, self.L, self.M)
        self.dtype, self.per = (np.int16, 2) if int16_iq else (np.int16, 1) if int16 else (np.complex64, 1)
        self.iq16 = int16_iq
        self.buf = torch.zeros((1, 0), dtype=torch.complex64, device="cuda")
        self.eof = False

    def _take(self, y, n):
        if y is not None and n[0]:
            self.buf = self.torch.cat([self.buf, y[:, :n[0]]], dim=1)

    def read(self, nin):
        """nin samples at 8 kHz as a device tensor [1, nin], or None once stdin cannot supply them"""
        size = np.dtype(self.dtype).itemsize * self.per
        while self.buf.shape[1] < nin and not self.eof:
            want = max(-(-(nin - self.buf.shape[1]) * self.M // self.L), 1)
            raw = self.inp.read(want * size)
            n = len(raw) // size
            if n:
                x = np.frombuffer(raw[:n * size], self.dtype)
                self._take(*self.rc.feed(self.torch.tensor(x.reshape(1, n, 2) if self.iq16 else x[None], device="cuda")))
            if n < want:
                self.eof = True
                self._take(*self.rc.flush())
        if self.buf.shape[1] < nin:
            return None
        x, self.buf = self.buf[:, :nin].contiguous(), self.buf[:, nin:]
        return x


def _txe(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli txe", description="RADAE streaming transmitter, features.f32 on stdin, IQ.f32 on output")
    ap.add_argument("--model_name", type=str, default="", help="DNNw weight blob (default: weights/model19_check3.bin)")
    ap.add_argument("--txbpf", action="store_true", help="enable Tx BPF")
    ap.add_argument("--bypass_enc", action="store_true", help="Bypass core encoder, read z from stdin")
    ap.add_argument("--eoo_data_test", action="store_true", help="experimental EOO data test - tx test frame")
    ap.add_argument("--int16_real", type=float, default=None, metavar="SCALE", help="write int16(I * SCALE) instead of IQ.f32 (`| f32toint16.py --real --scale SCALE`), converted on "
                    "the device; prints `peak: .. rms: .. clipped: ..` of the written samples on stderr")
    ap.add_argument("--fs", type=int, default=8000, metavar="HZ", help="sample rate written (default 8000: no conversion); another rate is made on the device, ahead of --int16_real")
    args = ap.parse_args(argv)
    eng = None
    if (args.int16_real is not None or args.fs != 8000) and not args.bypass_enc:  # the last metre to the radio runs on the device (rade_batch_wire_out): any engine serves, the bypass transmitter
        from . import engine                                 # has one; this one is opened ahead of the rade_api.h handle, whose library must find torch's HIP runtime loaded
        eng = engine.BatchEngine(1, max_tx_mf=1, blob=args.model_name or None)
    tx = api.radae_tx_bypass_enc(args.model_name, txbpf_en=args.txbpf) if args.bypass_enc else api.radae_tx(args.model_name, txbpf_en=args.txbpf)
    if args.eoo_data_test:                                  # radae_txe.py:157-163: the seeded bits the receiver side regenerates
        rng = np.random.default_rng(65647)
        bits = np.sign(rng.random(tx.get_Neoo_bits()) - 0.5).astype(np.float32)
        tx.set_eoo_bits(bits)
        bits.tofile("eoo_tx.f32")
    n_in = tx.get_n_floats_in()
    tx_out = np.zeros(tx.get_Nmf(), np.complex64)
    inp, out = sys.stdin.buffer, sys.stdout.buffer
    emit = lambda iq, last=False: out.write(iq.tobytes())
    if args.int16_real is not None or args.fs != 8000:
        import torch
        from . import engine
        eng = eng or tx.eng
        level = {"peak": 0.0, "s2": 0.0, "n": 0, "clipped": 0}
        rc = engine.RateConverter(eng, *_ratio(args.fs, 8000)) if args.fs != 8000 else None

        def emit(iq, last=False):
            x = torch.tensor(iq[None], device="cuda")
            for y, n_y in ([rc.feed(x)] + ([rc.flush()] if last else [])) if rc else [(x, [iq.size])]:
                if not n_y[0]:
                    continue
                y = y[:, :n_y[0]].contiguous()
                if args.int16_real is None:
                    out.write(y.cpu().numpy().tobytes())
                    continue
                s, m = eng.wire_out(y, scale=args.int16_real, meters=True)
                out.write(s.cpu().numpy().tobytes())
                n = int(n_y[0]) - int(m.nan[0])
                level["peak"] = max(level["peak"], float(m.peak[0])); level["s2"] += float(m.rms[0]) ** 2 * n; level["n"] += n; level["clipped"] += int(m.clipped[0])
    while True:
        buf = inp.read(n_in * struct.calcsize("f"))
        if len(buf) != n_in * struct.calcsize("f"):
            break
        tx.do_radae_tx(np.frombuffer(buf, np.float32), tx_out)
        emit(tx_out)
    eoo = np.zeros(tx.get_Neoo(), np.complex64)
    tx.do_eoo(eoo)
    emit(eoo, last=True)
    out.flush()
    if args.int16_real is not None:
        print(f"peak: {level['peak']:.1f} rms: {np.sqrt(level['s2'] / max(level['n'], 1)):.1f} clipped: {level['clipped']}", file=sys.stderr)
    return 0


def _rxe(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli rxe", description="RADAE streaming receiver, IQ.f32 on stdin to features.f32 on stdout")
    ap.add_argument("--model_name", type=str, default="", help="DNNw weight blob (default: weights/model19_check3.bin)")
    ap.add_argument("-v", type=int, default=2, help="Verbose level (default 2)")
    ap.add_argument("--disable_unsync", type=float, default=0.0, help="test mode: disable auxdata based unsyncs after this many seconds (default disabled)")
    ap.add_argument("--no_stdout", action="store_false", dest="use_stdout", help="disable the use of stdout")
    ap.add_argument("--foff_err", type=float, default=0.0, help="Artifical freq offset error after first sync to test false sync (the C ABI offers the 10 Hz test only)")
    ap.add_argument("--bypass_dec", action="store_true", help="Bypass core decoder, write z_hat to stdout")
    ap.add_argument("--eoo_data_test", action="store_true", help="experimental EOO data test - count bit errors")
    ap.add_argument("--int16", action="store_true", help="stdin is int16 samples of one real channel (what `int16tof32.py --zeropad` is piped in for), converted on the device")
    ap.add_argument("--int16_iq", action="store_true", help="stdin is int16 ..IQIQ.. (`int16tof32.py`), converted on the device")
    ap.add_argument("--fs", type=int, default=8000, metavar="HZ", help="sample rate of stdin (default 8000: no conversion); another rate, e.g. 48000 or 44100, is brought to 8000 "
                    "on the device, in place of a `sox .. -r 8000` stage; with --int16, --int16_iq or float IQ")
    ap.set_defaults(use_stdout=True)
    args = ap.parse_args(argv)
    if args.int16 and args.int16_iq:
        raise SystemExit("radae_amd.cli rxe: --int16 (one real channel) or --int16_iq, not both")
    wire16 = args.int16 or args.int16_iq                     # the conversion is a call of the batched engine (rade_batch_wire_in)
    if args.bypass_dec or args.disable_unsync or wire16 or args.fs != 8000:   # all are switches or calls of the batched engine (rade_api.h has none of them)
        cls = api.radae_rx_bypass_dec if args.bypass_dec else api.radae_rx_engine
        rx = cls(args.model_name, foff_err=args.foff_err, disable_unsync=args.disable_unsync)
    else:
        rx = api.radae_rx(args.model_name, foff_err=args.foff_err)
    floats_out = np.zeros(rx.get_n_floats_out(), np.float32)
    inp, out = sys.stdin.buffer, sys.stdout.buffer
    mf = 0
    rate_in = _RateIn(rx.eng, inp, args.fs, args.int16, args.int16_iq) if args.fs != 8000 else None
    while True:
        nin = rx.get_nin()
        if rate_in:
            x = rate_in.read(nin)
            if x is None:
                break
            ret = rx._rx_dev(x, floats_out)
        else:
            n_bytes = nin * struct.calcsize("hh" if args.int16_iq else "h" if args.int16 else "ff")
            buf = inp.read(n_bytes)
            if len(buf) != n_bytes:
                break
            ret = rx.do_radae_rx_int16(np.frombuffer(buf, np.int16), floats_out, iq=args.int16_iq) if wire16 else rx.do_radae_rx(np.frombuffer(buf, np.complex64), floats_out)
        mf += 1
        if args.v >= 2:
            print(f"{mf:3d} sync: {int(rx.get_sync())} nin: {rx.get_nin():4d} SNRdB: {rx.get_snrdB_3k_est():3d} ret: {ret}", file=sys.stderr)
        if (ret & 1) and args.use_stdout:
            out.write(floats_out.tobytes())
        if (ret & 2) and args.eoo_data_test:                # radae_rxe.py:359-368
            rng = np.random.default_rng(65647)
            tx_bits = np.sign(rng.random(rx.get_Neoo_bits()) - 0.5)
            n_bits = len(tx_bits)
            n_errors = int(np.sum(floats_out[:n_bits] * tx_bits < 0))
            ber = n_errors / n_bits
            print(f"EOO data n_bits: {n_bits} n_errors: {n_errors} BER: {ber:5.2f}", file=sys.stderr)
            if ber < 0.05:
                print("PASS", file=sys.stderr)
    out.flush()
    if args.v >= 1:
        print(f"state: {'sync' if rx.get_sync() else 'search'}", file=sys.stderr)       # what the ctest radae_rx_slip_plus_drops greps for
    return 0


def _inference(argv):
    """inference.py's rate-Fs channel-simulation run as the streaming ctests use it (`inference.sh model wav /dev/null --EbNodB .. --freq_offset .. [--df_dt ..] [--g_file g.f32]
    --rate_Fs --pilots --pilot_eq --eq_ls --cp 0.004 --bottleneck 3 --time_offset -16 --auxdata --write_rx rx.f32 [--prepend_noise s] [--append_noise s] [--end_of_over]
    [--sine_amp a --sine_freq f] [--rx_gain g] [--write_tx tx.f32]`, CMakeLists.txt:300-420; inference.py:43-79, :253-300): encoder + OFDM modulator, the two-path Doppler
    channel from a `g_file` (multipath_samples' format: gain sample, then ..G1G2..), AWGN at the Eb/No, frequency offset / drift, the write_rx tail.  The model-shape switches
    (--rate_Fs --pilots --pilot_eq --eq_ls --cp --bottleneck --time_offset --auxdata --correct_freq_offset --coarse_mag --latent-dim) are accepted and must describe model19_check3's
    waveform, the only one this path implements.  `features_hat` receives what the STREAMING receiver (radae_rxe's) decodes from the written samples -- the reference runs its
    stateless receiver with ideal timing there; the ctests of this path pass /dev/null.  Noise: the device's Philox generator (--seed), not torch's.

    The reference's ideal-timing receiver (radae.py:312-420, :590-657; rade_batch_rx_ideal) runs on the signal part of the channel output when asked for: `--ideal_rx` takes
    features_hat and the loss from it, honouring --pilot_eq / --eq_ls / --coarse_mag / --time_offset / --correct_freq_offset; `--ber_test` sends random +-1 latents instead
    of the encoder's and prints `n_bits: N BER: x.xxx` (radae.py:653-657); `--write_latent` writes its z_hat.  `--bottleneck 1` takes a bottleneck-1 blob (weights/model05.bin):
    the linear rate-Fs waveform (RADE_BATCH_TX_LINEAR) at sigma = (EbNo M)^-0.5, received by the ideal-timing receiver (the streaming one is model19_check3's).

    Without `--rate_Fs` and with `--bottleneck 3` the run is inference.py's rate-Rs one (_inference_rate_rs below): the channel model19 was trained under."""
    import torch
    from . import engine, wire
    from .loss import distortion_loss, find_loss
    ap = argparse.ArgumentParser(prog="radae_amd.cli inference")
    ap.add_argument("model_name"); ap.add_argument("features"); ap.add_argument("features_hat")
    ap.add_argument("--EbNodB", type=float, default=100.0); ap.add_argument("--g_file", type=str, default=""); ap.add_argument("--write_rx", type=str, default="")
    ap.add_argument("--rx_gain", type=float, default=1.0); ap.add_argument("--write_tx", type=str, default=""); ap.add_argument("--freq_offset", type=float, default=0.0)
    ap.add_argument("--df_dt", type=float, default=0.0); ap.add_argument("--prepend_noise", type=float, default=0.0); ap.add_argument("--append_noise", type=float, default=0.0)
    ap.add_argument("--end_of_over", action="store_true"); ap.add_argument("--sine_amp", type=float, default=0.0); ap.add_argument("--sine_freq", type=float, default=1000.0)
    ap.add_argument("--loss_test", type=float, default=0.0); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--write_latent", type=str, default="", help="z_hat of the ideal-timing receiver, .f32")
    for flag in ("--rate_Fs", "--pilots", "--pilot_eq", "--eq_ls", "--auxdata", "--correct_freq_offset", "--coarse_mag", "--ber_test", "--ideal_rx"):
        ap.add_argument(flag, action="store_true")
    ap.add_argument("--cp", type=float, default=0.004); ap.add_argument("--bottleneck", type=int, default=3); ap.add_argument("--time_offset", type=int, default=-16)
    ap.add_argument("--latent-dim", type=int, default=80)
    ap.add_argument("--h_file", type=str, default="", help="rate-Rs run: per-carrier magnitudes, float32 [.][20]"); ap.add_argument("--mp_test", action="store_true")
    ap.add_argument("--phase_offset", type=float, default=0.0, help="rate-Rs run: phase offset in rads")
    args = ap.parse_args(argv)
    if args.pilots and not args.rate_Fs:
        raise SystemExit("radae_amd.cli inference: --pilots needs --rate_Fs: the rate-Rs channel has no pilot numerology (the reference does not run this combination "
                         "either: RADAE.forward fails on tx_sym * H, 5 n_mf against 4 n_mf symbols)")
    if not args.rate_Fs and args.bottleneck == 3:
        return _inference_rate_rs(args)
    genie = args.ideal_rx or args.ber_test or bool(args.write_latent) or args.bottleneck == 1
    if args.bottleneck not in (1, 3) or abs(args.cp - 0.004) > 1e-9 or args.latent_dim != 80 or not -32 <= args.time_offset <= 0 or \
            (args.time_offset != -16 and not genie):
        raise SystemExit("radae_amd.cli inference: only the waveforms of model19_check3 (--rate_Fs --pilots --pilot_eq --eq_ls --cp 0.004 --bottleneck 3 --time_offset -16 --auxdata) "
                         "and of a bottleneck-1 blob (--bottleneck 1, ideal-timing receiver, --time_offset -32..0) are implemented")
    if args.bottleneck == 1 and args.end_of_over:
        raise SystemExit("radae_amd.cli inference: --end_of_over needs the bottleneck-3 waveform")
    blob = args.model_name if args.model_name.endswith(".bin") else None
    if args.bottleneck == 1 and not blob:
        raise SystemExit("radae_amd.cli inference: --bottleneck 1 needs a bottleneck-1 DNNw blob, e.g. weights/model05.bin")
    feats = wire.read_features(args.features)
    n_mf = len(feats) // 12                                   # whole modem frames (radae.py:303-310)
    feats = np.ascontiguousarray(feats[:12 * n_mf])
    if genie and n_mf < 2:
        raise SystemExit("radae_amd.cli inference: the ideal-timing receiver needs at least two modem frames")
    dev = torch.device("cuda", 0)
    bn1 = args.bottleneck == 1
    eng = engine.BatchEngine(1, max_tx_mf=n_mf, blob=blob, flags=(engine.BOTTLENECK1 | engine.TX_LINEAR) if bn1 else 0)
    feat_dim = 20 if bn1 else 21
    z = None
    if args.ber_test:                                         # radae.py:477-478: random +-1 latents in place of the encoder's
        g = torch.Generator().manual_seed(args.seed)
        z = torch.sign(torch.rand((1, 3 * n_mf, 80), generator=g) - 0.5).to(dev)
        iq = eng.tx_latents(z)
    elif bn1:                                                 # model05: 4 x 20 features per latent, tanh bottleneck (RADE_BATCH_BOTTLENECK1)
        iq = eng.tx_latents(eng.encode(torch.tensor(np.ascontiguousarray(feats[:, :20]).reshape(1, 3 * n_mf, 80), device=dev)))
    else:
        iq = eng.tx(torch.tensor(feats[None], device=dev))
    n_sig = n_mf * engine.NMF
    G = None
    if args.g_file:
        g = np.fromfile(args.g_file, np.complex64).reshape(-1, 2)
        mp_gain = np.real(g[0, 0]); g = (mp_gain * g[1:]).astype(np.complex64)          # inference.py:160-171
        if len(g) < n_sig:
            raise SystemExit("Multipath Doppler spread file too short")
        G = torch.tensor(np.ascontiguousarray(g[:n_sig])[None], device=dev)
    sigma = engine.sigma_from_EbNodB(args.EbNodB, bottleneck=args.bottleneck)
    n_pre, n_post = int(8000 * args.prepend_noise), int(8000 * args.append_noise)
    rx = eng.channel(iq, sigma, args.freq_offset, n_pre=n_pre, n_post=n_post, with_eoo=args.end_of_over, G=G, seed=args.seed, df_dt=args.df_dt,
                     sine_amp=args.sine_amp, sine_freq=args.sine_freq, rx_gain=args.rx_gain)
    tx = iq.cpu().numpy()[0]
    S = float(np.mean(np.abs(tx) ** 2)); N = sigma ** 2
    EbNo = 10 ** (args.EbNodB / 10); Rb, Bw = 2000.0, 3000.0
    print("          Eb/No   C/No     SNR3k  Rb'    Eq     PAPR")
    print(f"Target..: {args.EbNodB:6.2f}  {10 * np.log10(EbNo * Rb):6.2f}  {10 * np.log10(EbNo * Rb / Bw):6.2f}  {2400:d}")
    cno = 10 * np.log10(S * 8000.0 / N)
    print(f"Measured: {cno + 10 * np.log10(160 / (8000.0 * 30 * 2)):6.2f}  {cno:6.2f}  {cno - 10 * np.log10(Bw):6.2f}                {20 * np.log10(np.max(np.abs(tx)) / np.sqrt(S)):5.2f}")
    if args.write_rx:
        rx.cpu().numpy()[0].astype(np.complex64).tofile(args.write_rx)
    if args.write_tx:
        tx.astype(np.complex64).tofile(args.write_tx)
    if genie:                                                 # the ideal-timing receiver inside RADAE.forward sees the signal before the write_rx tail
        rs = rx[:, n_pre:n_pre + n_sig]
        if args.rx_gain != 1.0:
            rs = rs / args.rx_gain
        fo_ = (args.freq_offset, args.df_dt) if args.correct_freq_offset else (None, None)
        fi, z_hat, n_err = eng.rx_ideal(rs.contiguous(), n_mf, time_offset=args.time_offset, eq="ls" if args.eq_ls else ("mean6" if args.pilot_eq else "none"),
                                        coarse_mag=args.coarse_mag, freq_offset=fo_[0], df_dt=fo_[1], z_ref=z, feat_width=4 * feat_dim)
        if args.ber_test:
            n_bits = 3 * n_mf * 80
            print(f"n_bits: {n_bits:d} BER: {int(n_err[0]) / n_bits:5.3f}")
        if args.write_latent:
            z_hat.cpu().numpy()[0].astype(np.float32).tofile(args.write_latent)
    if genie and (args.ideal_rx or bn1):
        fh = fi.cpu().numpy()[0].reshape(-1, feat_dim)
        out = np.zeros((len(fh), 36), np.float32); out[:, :20] = fh[:, :20]          # inference.py:234-236
        if args.features_hat != "/dev/null":
            out.tofile(args.features_hat)
        if not args.ber_test:
            ft = feats[:, :21].copy()
            if not bn1:
                ft[:, 20] = -1.0                              # the aux symbol the transmitter appended
            loss = distortion_loss(ft[:, :feat_dim], fh)
            print(f"loss: {loss:5.3f} (ideal-timing receiver)")
            if args.loss_test > 0.0:
                print("PASS" if loss < args.loss_test else "FAIL")
        eng.close()
        return 0
    fo, st, _ = eng.rx(rx if args.rx_gain == 1.0 else rx.clone())
    nv = st[0].n_valid
    fh = fo.cpu().numpy()[0, :nv].reshape(-1, 36)
    if args.features_hat != "/dev/null":
        fh.astype(np.float32).tofile(args.features_hat)
    if nv:
        loss, start = find_loss(feats, fh)
        print(f"loss: {loss:5.3f} (streaming receiver: {12 * nv} frames decoded, aligned at frame {start})")
        if args.loss_test > 0.0:
            print("PASS" if loss < args.loss_test else "FAIL")
    else:
        print("loss: n/a (the streaming receiver decoded nothing)")
    eng.close()
    return 0


def _inference_rate_rs(args):
    """inference.py without --rate_Fs on a bottleneck-3 model (inference.py:127-153, :213-229; radae.py:603-634): features (+ the aux symbol) -> core encoder -> the rate-Rs
    channel (IDFT, PA limiter, DFT per OFDM symbol of the no-pilot numerology Nc = 20, M = 160; phase offset, per-carrier magnitudes H, AWGN: rade_batch_channel_rs_pa) ->
    core decoder -> features_hat.  Needs --auxdata (the blob's 21 features); refuses the options only the rate-Fs run has.  Honours --EbNodB, --h_file (float32 [.][20]), --mp_test, --phase_offset, --write_latent, --loss_test, --ber_test, --seed; prints the
    reference's Target / Measured lines (Eq/No - 3 dB, SNR3k, Eq, PAPR).  Noise: the device's Philox generator (--seed), not torch's."""
    import torch
    from . import engine, wire
    from .loss import distortion_loss
    if args.latent_dim != 80:
        raise SystemExit("radae_amd.cli inference: only --latent-dim 80 is implemented")
    # what only the rate-Fs run can honour is refused, not ignored: the sample-rate channel, its files and its receivers do not exist at rate Rs
    fs_only = [("--g_file", args.g_file), ("--write_rx", args.write_rx), ("--write_tx", args.write_tx), ("--freq_offset", args.freq_offset), ("--df_dt", args.df_dt),
               ("--prepend_noise", args.prepend_noise), ("--append_noise", args.append_noise), ("--end_of_over", args.end_of_over), ("--sine_amp", args.sine_amp),
               ("--rx_gain", args.rx_gain != 1.0), ("--ideal_rx", args.ideal_rx), ("--correct_freq_offset", args.correct_freq_offset)]
    given = [name for name, v in fs_only if v]
    if given:
        raise SystemExit(f"radae_amd.cli inference: {', '.join(given)} need(s) --rate_Fs: without it the run is the rate-Rs channel (one sample per QPSK symbol), "
                         "which has no sample-rate signal to write, offset or receive")
    if not args.auxdata:
        raise SystemExit("radae_amd.cli inference: the rate-Rs run needs --auxdata: model19_check3's encoder takes 21 features per frame (the aux symbol is appended here, "
                         "inference.py:115-123)")
    blob = args.model_name if args.model_name.endswith(".bin") else None
    feats = wire.read_features(args.features)
    n_mf = len(feats) // 12                                   # whole modem frames (radae.py:303-310)
    if n_mf < 1:
        raise SystemExit("radae_amd.cli inference: less than one modem frame of features")
    feats = np.ascontiguousarray(feats[:12 * n_mf])
    print(f"Processing: {12 * n_mf} feature vectors")
    rows, n_sym, Nc, Rs = 3 * n_mf, 6 * n_mf, 20, 50.0
    H = None
    if args.mp_test:                                          # inference.py:134-142: peaks and notches between 2 and 0, constant over time
        H = np.tile(np.abs(1.0 + np.exp(-2j * np.pi * np.arange(Nc) * 0.002 * Rs)).astype(np.float32), (n_sym, 1))
    if args.h_file:
        H = np.fromfile(args.h_file, np.float32).reshape(-1, Nc)
        if len(H) < n_sym:
            raise SystemExit("Multipath H file too short")
        H = np.ascontiguousarray(H[:n_sym])
    dev = torch.device("cuda", 0)
    eng = engine.BatchEngine(1, max_tx_mf=n_mf, blob=blob)
    ft = np.ascontiguousarray(feats[:, :21]); ft[:, 20] = -1.0           # inference.py:115-123: the aux symbol
    z = eng.encode(torch.tensor(ft.reshape(1, rows, 84), device=dev))
    if args.ber_test:                                         # radae.py:477-478 (BER 0.5 in this mode: the noise is scaled for the encoder's symbols of magnitude M / sqrt(Nc))
        g = torch.Generator().manual_seed(args.seed)
        z = torch.sign(torch.rand((1, rows, 80), generator=g) - 0.5).to(dev)
    sigma = engine.sigma_from_EbNodB(args.EbNodB, rate_Fs=False)
    z_hat, st = eng.channel_rs_pa(z, sigma, H=torch.tensor(H[None], device=dev) if H is not None else None, phase_offset=args.phase_offset, seed=args.seed, want_stats=True)
    if args.ber_test:
        print(f"n_bits: {rows * 80:d} BER: {int(torch.sum(-z * z_hat > 0)) / (rows * 80):5.3f}")
    fh = eng.decode(z_hat, 84).cpu().numpy()[0].reshape(-1, 21)
    EbNo = 10 ** (args.EbNodB / 10); Rb, Bw = 2000.0, 3000.0
    print("          Eb/No   C/No     SNR3k  Rb'    Eq     PAPR")
    print(f"Target..: {args.EbNodB:6.2f}  {10 * np.log10(EbNo * Rb):6.2f}  {10 * np.log10(EbNo * Rb / Bw):6.2f}  {int(Rb):d}")
    Eq = st[0, 2] / (n_sym * Nc); S = st[0, 0] / (n_sym * 160)
    EqNo = 10 * np.log10(Eq / sigma ** 2)
    print(f"Measured: {EqNo - 3:6.2f}          {EqNo + 10 * np.log10(Rs * Nc / Bw):6.2f}       {Eq:7.2f} {20 * np.log10(st[0, 1] / np.sqrt(S)):5.2f}")
    out = np.zeros((len(fh), 36), np.float32); out[:, :20] = fh[:, :20]              # inference.py:231-234
    if args.features_hat != "/dev/null":
        out.tofile(args.features_hat)
    if args.write_latent:
        z_hat.cpu().numpy()[0].astype(np.float32).tofile(args.write_latent)
    loss = distortion_loss(ft, fh)
    ber = float(np.mean(ft[:, 20] * fh[:, 20] < 0))
    print(f"loss: {loss:5.3f} Auxdata BER: {ber:5.3f}")
    if args.loss_test > 0.0:
        print("PASS" if loss < args.loss_test else "FAIL")
    eng.close()
    return 0


def _multipath_samples(argv):
    """multipath_samples.m's command line: `multipath_samples(ch, Fs, Rs, Nc, Nseconds, H_fn, G_fn="", H_complex=0)` -> the rate-Rs `H` file (magnitudes, or complex with
    --complex) and the rate-Fs `G` file (gain sample, then ..G1G2.. complex64) that inference.py's --h_file / --g_file read.  numpy's generator instead of Octave's randn('seed', 1)."""
    from .channel_tools import PRESETS
    ap = argparse.ArgumentParser(prog="radae_amd.cli multipath_samples")
    ap.add_argument("ch", choices=sorted(PRESETS)); ap.add_argument("Fs", type=int); ap.add_argument("Rs", type=int); ap.add_argument("Nc", type=int)
    ap.add_argument("Nseconds", type=float); ap.add_argument("H_fn"); ap.add_argument("G_fn", nargs="?", default="")
    ap.add_argument("--complex", action="store_true", dest="h_complex"); ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    import math
    from .channel_tools import doppler_spread
    nsam = int(args.Fs * args.Nseconds)
    rng = np.random.default_rng(args.seed)
    g1 = doppler_spread(PRESETS[args.ch][0], args.Fs, nsam, rng); g2 = doppler_spread(PRESETS[args.ch][0], args.Fs, nsam, rng)      # the draws of channel_tools.multipath_g
    hf_gain = 1.0 / math.sqrt(np.var(g1) + np.var(g2))                                 # multipath_samples.m:31
    m = args.Fs // args.Rs
    d = PRESETS[args.ch][1]
    H = hf_gain * (g1[::m, None] + g2[::m, None] * np.exp(-2j * np.pi * np.arange(args.Nc)[None, :] * d * args.Rs))      # :33-40
    (H.astype(np.complex64) if args.h_complex else np.abs(H).astype(np.float32)).tofile(args.H_fn)
    if args.G_fn:                                                                      # :92-103: four floats of hf_gain, then ..G1G2.. UN-scaled (inference.py:160-171 multiplies)
        out = np.concatenate([np.full((1, 2), hf_gain * (1 + 1j), np.complex64), np.stack([g1, g2], axis=1).astype(np.complex64)])
        out.tofile(args.G_fn)
    print(f"{args.ch}: Doppler spread {PRESETS[args.ch][0]:g} Hz, path delay {d * 1e3:g} ms, {len(H)} x {args.Nc} H samples" + (f", {nsam} G samples" if args.G_fn else ""))
    return 0


def _bbfm_inference(argv):
    """bbfm_inference.py (:43-170): features -> core encoder (bottleneck 1) -> the analog-FM channel model (bbfm.py:157-197: per-symbol CNR = 20 log10 |H| + CNRdB, FM demodulator SNR
    with its threshold at 12 dB, noise, clamp) -> core decoder -> features_hat; `--h_file` = rate-Rs fading magnitudes (multipath_samples("lmr60", 8000, 2000, 1, ...)), `--write_latent`,
    `--write_CNRdB`, `--loss_test`, `--passthru`.  `model_name`: a DNNw blob of the BBFM architecture (default weights/bbfm_random_seed20240501.bin: no trained BBFM weights exist in the
    reference tree).  Noise: the device's Philox generator (--seed)."""
    import math
    import os
    import torch
    from . import engine, wire
    from .loss import distortion_loss
    ap = argparse.ArgumentParser(prog="radae_amd.cli bbfm_inference")
    ap.add_argument("model_name"); ap.add_argument("features"); ap.add_argument("features_hat")
    ap.add_argument("--latent-dim", type=int, default=80); ap.add_argument("--write_latent", type=str, default=""); ap.add_argument("--CNRdB", type=float, default=100.0)
    ap.add_argument("--passthru", action="store_true"); ap.add_argument("--h_file", type=str, default=""); ap.add_argument("--write_CNRdB", type=str, default="")
    ap.add_argument("--loss_test", type=float, default=0.0); ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    feats = wire.read_features(args.features)
    T = len(feats) // 4                                      # encoder steps of four frames (bbfm.py / radae_base.py:158)
    feats = np.ascontiguousarray(feats[:4 * T])
    if args.passthru:
        feats.astype(np.float32).tofile(args.features_hat); return 0
    blob = args.model_name if args.model_name.endswith(".bin") else os.path.join(os.path.dirname(engine.DEFAULT_BLOB), "bbfm_random_seed20240501.bin")
    dev = torch.device("cuda", 0)
    Tc = 3 * ((T + 2) // 3)
    eng = engine.BatchEngine(1, max_tx_mf=Tc // 3, blob=blob, flags=engine.BOTTLENECK1)
    x = np.zeros((1, Tc, 80), np.float32); x[0, :T] = feats[:, :20].reshape(T, 80)
    z = eng.encode(torch.tensor(x, device=dev))
    nsym = Tc * 80
    H = None; Hn = np.ones(nsym, np.float32)
    if args.h_file:
        h = np.fromfile(args.h_file, np.float32)
        if h.size < T * 80:
            raise SystemExit("Multipath H file too short")
        Hn[:T * 80] = h[:T * 80]; H = torch.tensor(Hn[None], device=dev)
    Gfm = 10 * math.log10(3 * (5000 / 3000) ** 2 * (5000 / 3000 + 1))       # bbfm.py:78-80, fd 5000 Hz, fm 3000 Hz
    zh = eng.channel_symbol(z, "bbfm", args.CNRdB, Gfm, H=H, seed=args.seed)
    fh = eng.decode(zh, 80).cpu().numpy()[0, :T].reshape(4 * T, 20)
    cnr = 20 * np.log10(Hn[:T * 80]) + args.CNRdB
    snr = np.maximum(cnr - 12, 0) + 12 + Gfm - np.maximum(-(cnr - 12), 0) * (1 + Gfm / 3)      # bbfm.py:178-179
    zhn = zh.cpu().numpy()[0, :T].ravel()
    print(f"SNRdB Measured: {10 * np.log10(np.mean(zhn ** 2) / np.mean(10 ** (-snr / 10))):6.2f}")
    out = np.zeros((4 * T, 36), np.float32); out[:, :20] = fh
    if args.features_hat != "/dev/null":
        out.tofile(args.features_hat)
    loss = distortion_loss(feats[:, :20], fh)
    print(f"loss: {loss:5.3f}")
    if args.loss_test > 0.0:
        print("PASS" if loss < args.loss_test else "FAIL")
    if args.write_latent:
        zhn.astype(np.float32).tofile(args.write_latent)
    if args.write_CNRdB:
        cnr.astype(np.float32).tofile(args.write_CNRdB)
    eng.close()
    return 0


FM_FS, FM_FC, FM_FD, FM_FMAX = 48000, 12000.0, 5000.0, 3000.0           # fm_mod_file / fm_demod_file (fm.m:292-300, :337-346)


def analog_fm_chain(eng, x16, CNRdB: float, seed: int = 1):
    """The analog-FM baseline of analog_bbfm.sh:37-43 on the device, from 8 kHz int16 speech to 8 kHz int16 speech: x16 cuda int16 [B, n] -> int16 [B, n].
    rate_convert 8 k -> 48 k (the int16 samples scaled by 1 / 32767 as fm_mod_file reads them), fm_mod (fc 12 kHz, fd 5 kHz, real output with real noise at CNRdB),
    int16(tx x 16384) and back (the file between fm_mod_file and fm_demod_file), fm_demod (de-emphasis folded in), rate_convert 48 k -> 8 k, int16(y x 20000).
    Deviations from the script: no int16 file at 48 kHz in front of the modulator and behind the demodulator (the samples stay float32 there), and int16 conversion
    truncates toward zero where Octave's fwrite rounds."""
    from . import engine
    sigma = engine.fm_sigma(CNRdB, FM_FS, FM_FMAX, FM_FD)
    b1, b2 = engine.fm_taps(FM_FS, FM_FMAX, FM_FD, 201, engine.FM_DE_EMP_TC)
    up, n_up = eng.rate_convert(x16, 6, 1, gain=1.0 / 32767.0)
    tx, _ = eng.fm_mod(up, FM_FS, FM_FC, FM_FD, n=n_up, real=True, sigma=sigma, seed=seed, want_phase=False)
    rx = eng.wire_in(eng.wire_out(tx, n=n_up, real=True, scale=16384.0), n=n_up)
    y, _, n_y = eng.fm_demod(rx, FM_FS, FM_FC, FM_FD, b1, b2, n_in=n_up, complex_out=True)
    down, n_down = eng.rate_convert(y, 1, 6, n_in=n_y)
    return eng.wire_out(down, n=n_down, real=True, scale=20000.0), n_down


def _analog_fm(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli analog_fm", description="analog FM baseline (analog_bbfm.sh): 8 kHz int16 speech through an FM modulator, noise at a C/N "
                                 "and an FM demodulator at 48 kHz, all on the device")
    ap.add_argument("input", help="8 kHz int16 mono samples (what the sox and `ch` stages of analog_bbfm.sh:37 deliver)")
    ap.add_argument("output", help="8 kHz int16 mono samples")
    ap.add_argument("CNRdB", type=float, help="carrier to noise ratio in Carson's bandwidth, dB")
    ap.add_argument("--seed", type=int, default=1, help="seed of the generated noise (non-zero)")
    args = ap.parse_args(argv)
    import torch
    from . import engine
    x = np.fromfile(args.input, np.int16)
    if not x.size:
        np.zeros(0, np.int16).tofile(args.output)
        return 0
    eng = engine.BatchEngine(1, max_tx_mf=1)
    y, n = analog_fm_chain(eng, torch.tensor(x[None], device="cuda"), args.CNRdB, args.seed)
    y.cpu().numpy()[0, :int(n[0])].tofile(args.output)
    eng.close()
    return 0


def _est_cno(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli est_cno", description="Estimate C/No from a file of samples (est_CNo.py): C+N in a band that holds the signal, No in an "
                                 "adjacent band, the window with the highest C/No; the periodograms run on the device (rade_batch_cno_est)")
    ap.add_argument("rx", type=str, help="path to signal + noise input file of rate Fs rx samples in ..IQIQ...f32 format")
    ap.add_argument("--window_time", type=float, default=4.0, help="size of time domain window (seconds) used for SNR measurement, a multiple of 0.25 up to 8 (default 4.0)")
    ap.add_argument("--flow", type=float, default=400.0, help="lower freq limit for C+N band (default 400 Hz)")
    ap.add_argument("--fhigh", type=float, default=2000.0, help="upper limit for C+N band (default 2000 Hz)")
    args = ap.parse_args(argv)
    import torch
    from . import engine
    Fs = engine.CNO_FS
    rx = np.fromfile(args.rx, dtype=np.csingle)
    q = engine.cno_plan(args.window_time, args.flow, args.fhigh)
    assert len(rx) >= q.N
    eng = engine.BatchEngine(1, max_tx_mf=1)
    (res,), bands = eng.cno_est(torch.tensor(rx[None], device="cuda"), window_time=args.window_time, flow=args.flow, fhigh=args.fhigh, bands=True)
    eng.close()
    bins_per_Hz = q.N / Fs
    Nbw = (q.noise_en - q.noise_st) / bins_per_Hz
    for w in range(res.n_windows):                           # the script's per-window lines, from the band sums by the script's own arithmetic
        st = w * engine.CNO_HOP
        No = bands[0, w, 1] / Nbw
        C = bands[0, w, 0] - No * (args.fhigh - args.flow)
        if C > 0:
            CNodB = 10 * np.log10(C) - 10 * np.log10(No)
            print(f"time: {st:8d} {st/Fs:5.2f} CNodB: {CNodB:5.2f}")
    print(f"           Time   C/No    SNR3k")
    print(f"Measured: {res.max_st/Fs:5.2f}  {res.max_CNodB:6.2f}  {res.max_SNRdB:6.2f}")
    return 0


def _est_snr(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli est_snr", description="Trials of the pilot SNR estimator (est_snr.py): the default run sweeps the set points -5 .. 19 dB, "
                                 "every trial of every set point in one device call (rade_batch_snr_trials).  The estimator's arithmetic is the script's; the noise is the "
                                 "engine's generator (--seed), not np.random, so single points differ from a run of the script.  --plots and --plots2 are not offered")
    ap.add_argument("--snrdB", type=float, default=10.0, help="snrdB set point")
    ap.add_argument("--single", action="store_true", help="single snrdB test")
    ap.add_argument("--sequence", action="store_true", help="run over a sequence of timesteps")
    ap.add_argument("--h_file", type=str, default="", help="path to rate Rs multipath samples, rate Rs time steps by Nc carriers .f32 format")
    ap.add_argument("-T", type=float, default=1.0, help="length of time window for estimate (default 1.0 sec)")
    ap.add_argument("--Nt", type=int, default=1, help="number of analysis time windows to test across (default 1)")
    ap.add_argument("--test_S1", action="store_true", help="calculate S1 two ways to check S1 expression")
    ap.add_argument("--eq_ls", action="store_true", help="est phase from received pilots using least square (default genie phase)")
    ap.add_argument("--save_text", type=str, default="", help="path to text file to save test points")
    ap.add_argument("-c", type=float, default=0.0, help="y offset correction in dB (default 0)")
    ap.add_argument("-m", type=float, default=1.0, help="gradient correction in dB (default 1.0)")
    ap.add_argument("--seed", type=int, default=1, help="seed of the device noise generator, not 0 (default 1)")
    args = ap.parse_args(argv)
    import torch
    from . import engine
    Nw = engine.snr_windows_rows(args.T)
    h = None
    if args.h_file:                                          # the script's h[::Ns+1][:Nw*Nt]: the rows stay where they are, the device steps over them
        h = np.fromfile(args.h_file, dtype=np.complex64).reshape(-1, engine.SNR_NC)[:(Nw * args.Nt - 1) * (engine.SNR_NS + 1) + 1]
    if args.single or args.sequence:
        Nt = 1 if args.single else args.Nt
        eng = engine.BatchEngine(1, max_tx_mf=1)
        sums = eng.snr_trials(Nt, Nw, engine.snr_sigma(args.snrdB), H=None if h is None else torch.tensor(h[None], device="cuda"), h_step=engine.SNR_NS + 1,
                              seed=args.seed)[0]
        eng.close()
        pts = engine.snr_finish(sums, args.eq_ls, args.c, args.m)
        for s, p in zip(sums, pts):
            if args.single:
                if args.test_S1:
                    print(f"S1_first: {s['S1_sig']:5.2f} S1_second: {s['S1_cross']:5.2f} S1_third: {s['S1_noise']:5.2f}")
                    print(f"S1: {s['S1']:5.2f} S1_sum: {s['S1_sig'] + s['S1_cross'] + s['S1_noise']:5.2f}")
                print(f"setpoint snrdB: {args.snrdB:5.2f} snrdB_genie: {p['snrdB_genie']:5.2f} snrdB_est: {p['snrdB_est']:5.2f}")
            else:
                print(f"setpoint snrdB: {args.snrdB:5.2f} snrdB_genie: {p['snrdB_genie']:5.2f} snrdB_est: {p['snrdB_est']:5.2f} NdB: {p['NdB_genie']:5.2f} {p['NdB_est']:5.2f}")
        return 0
    r = engine.snr_sweep([h], args.Nt, args.T, eq_ls=args.eq_ls, c=args.c, m=args.m, seed=args.seed)
    for i, sp in enumerate(range(-5, 20)):
        for k in range(args.Nt):
            j = i * args.Nt + k
            print(f"setpoint snrdB: {sp:5.2f} snrdB_genie: {r.snrdB_genie[0, j]:5.2f} snrdB_est: {r.snrdB_est[0, j]:5.2f} NdB: {r.NdB_genie[0, j]:5.2f} {r.NdB_est[0, j]:5.2f}")
    print(r.fit[0])
    if args.save_text:                                       # the two columns radae_plots.m: est_snr_plot loads
        np.savetxt(args.save_text, np.transpose(np.array((r.snrdB_genie[0], r.snrdB_est[0]))), delimiter="\t")
    return 0


def _rx(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli rx", description="Pilot acquisition of a stored recording (rx.py --pilots): the input band-pass, detect_pilots over every "
                                 "modem frame in one device call (rade_batch_acq_detect), the script's state machine and refine; with --acq_test the pass / fail statistics.  "
                                 "With --decode the script's normal run goes on past the acquisition, on the device: refine one frame later, trim, mix down, the "
                                 "fixed-timing demodulator, the decoder, and --ber_test's alignment (rx.py:197-276).  --rx_one, --stateful and --plots are not offered")
    ap.add_argument("rx", type=str, help="path to input file of rate Fs rx samples in ..IQIQ...f32 format")
    ap.add_argument("model_name", nargs="?", default=None, help="accepted and ignored (the script's first argument): the geometry is model19_check3's")
    ap.add_argument("features_hat", nargs="?", default=None, help="with --decode: path to the output feature file (float32, 36 per frame); ignored otherwise")
    ap.add_argument("--no_bpf", dest="bpf", action="store_false", help="disable the input band-pass filter")
    ap.add_argument("--acq_test", action="store_true", help="search again after every acquisition and report passes, fails, P(fail) and the mean acquisition time")
    ap.add_argument("--fmax_target", type=float, default=0.0, help="acquisition test mode freq offset target (default 0.0)")
    ap.add_argument("--acq_time_target", type=float, default=1.0, help="acquisition test mode mean acquisition time target (default 1.0)")
    ap.add_argument("--write_Dt", type=str, default="", help="write Dt1 of every frame, complex64 [frames][960][40]")
    ap.add_argument("--decode", action="store_true", help="go on past the acquisition as the script's normal run does and write features_hat (not with --acq_test / --write_Dt)")
    ap.add_argument("--write_latent", type=str, default="", help="with --decode: path to output file of latent vectors z[latent_dim] in .f32 format")
    ap.add_argument("--ber_test", type=str, default="", help="with --decode: symbols are PSK bits, compare to z.f32 file to calculate BER")
    ap.add_argument("--freq_offset", type=float, default=None, help="with --decode: manually specify frequency offset")
    # the script's waveform flags, accepted where they describe model19_check3
    ap.add_argument("--pilots", action="store_true"); ap.add_argument("--pilot_eq", action="store_true"); ap.add_argument("--coarse_mag", action="store_true")
    ap.add_argument("--auxdata", action="store_true"); ap.add_argument("--bottleneck", type=int, default=3); ap.add_argument("--cp", type=float, default=0.004)
    ap.add_argument("--latent-dim", type=int, default=80); ap.add_argument("--time_offset", type=int, default=-16)
    ap.add_argument("--eq_ls", action="store_true", help="accepted and ignored (an option of inference.py, not of rx.py): with --decode, --pilot_eq alone selects the least-squares equaliser, as in the script")
    args = ap.parse_args(argv)
    if args.bottleneck != 3 or args.cp != 0.004 or args.latent_dim != 80:
        raise SystemExit("radae_amd.cli rx: only model19_check3's waveform (--bottleneck 3 --cp 0.004 --latent-dim 80) is built")
    if args.decode and (args.acq_test or args.write_Dt or not args.features_hat):
        raise SystemExit("radae_amd.cli rx --decode: needs FEATURES_HAT and is the script's normal run (no --acq_test, no --write_Dt)")
    import torch
    from . import acq, engine, stages
    rx = np.fromfile(args.rx, dtype=np.csingle)
    print(f"samples: {len(rx):d} Nmf: {acq.NMF:d} modem frames: {len(rx)/acq.NMF}")
    if args.decode:
        return _rx_decode(args, rx)
    eng = engine.BatchEngine(1, max_tx_mf=1)
    x = torch.tensor(rx[None], device="cuda")
    n_hops = stages.acq_hops(len(rx))
    res = acq.acquire(eng, x, bpf=args.bpf, acq_test=args.acq_test, fmax_target=args.fmax_target, acq_time_target=args.acq_time_target,
                      dt_rows=(0, acq.NMF * n_hops) if args.write_Dt and n_hops else None)
    (r,) = res[0] if isinstance(res, tuple) else res
    if isinstance(res, tuple):
        res[1][0].cpu().numpy().tofile(args.write_Dt)             # Dt1 of every frame, from the one detect call
    eng.close()
    at = {int(e["hop"]): i for i, e in enumerate(r.events)}
    for k, (h, fm, lg) in enumerate(zip(r.hops, r.fmax, r.log)):         # the script's per-frame line, then what it prints when the frame acquires
        state = ("search", "candidate")[lg["state"]]
        print(f"{k + 1:2d} state: {state:10s} Dthresh: {h['Dthresh']:8.2f} Dtmax12: {h['Dtmax12']:8.2f} tmax: {h['tmax']:4d} tmax_candidate: {lg['tmax_candidate']:4d} fmax: {fm:6.2f}")
        if k in at and args.acq_test:
            t, f = int(r.refined[at[k]]["t"]) - acq.NMF * k, float(r.refined[at[k]]["f"])
            t_ok = abs(t - (acq.NCP + (acq.NTAP if args.bpf else 0) / 2)) < 0.0025 * acq.FS
            f_ok = abs(f - args.fmax_target) <= 5.0
            print(f"Acquired! Timing: {t_ok:d} Freq: {f_ok:d} " + ("" if t_ok and f_ok else f"fmax: {f:6.2f} targ: {args.fmax_target:6.2f}"))
        elif k in at:
            print("Acquired!")
    if args.acq_test:
        s = r.stats
        print(f"Acq Test Passes: {s.passes:d} Fails: {s.fails:d} Pfail: {s.pfail:5.2f} Mean Acq time: {s.mean_acq_time:5.2f} s")
        if s.passed:
            print("PASS")
    if args.acq_test or not len(r.events):                             # --acq_test never sets the script's `acquired`: it always ends here, as the script does
        print("Acquisition failed....")
    else:
        print(f"refined fmax: {float(r.refined[0]['f']):f}")
    return 0


def _rx_decode(args, rx):
    """rx.py's normal run past the acquisition (radae_amd.acq.receive): what the script prints, the feature file as `inference` writes its own, --write_latent, --ber_test"""
    import torch
    from . import acq, engine
    from .abi import FILE_STATUS
    eng = engine.BatchEngine(1, max_tx_mf=max(len(rx) // acq.NMF, 2))
    z_ref = None
    if args.ber_test:
        z = np.fromfile(args.ber_test, dtype=np.float32)
        z_ref = torch.tensor(z[None] if len(z) else np.zeros((1, 1), np.float32), device="cuda"), len(z)
    eq = "ls" if args.pilot_eq else "none"                            # the script builds its model with eq_mean6 = False (rx.py:81-84): --pilot_eq IS the least-squares equaliser
    (r,) = acq.receive(eng, torch.tensor(rx[None], device="cuda"), bpf=args.bpf, freq_offset=args.freq_offset, time_offset=args.time_offset, eq=eq,
                       coarse_mag=args.coarse_mag, z_ref=z_ref)
    a = r.acq
    for k, (h, fm, lg) in enumerate(zip(a.hops, a.fmax, a.log)):
        if len(a.events) and k > int(a.events[0]["hop"]):
            break                                                      # the script's loop ends with the frame that acquires
        state = ("search", "candidate")[lg["state"]]
        print(f"{k + 1:2d} state: {state:10s} Dthresh: {h['Dthresh']:8.2f} Dtmax12: {h['Dtmax12']:8.2f} tmax: {h['tmax']:4d} tmax_candidate: {lg['tmax_candidate']:4d} fmax: {fm:6.2f}")
    if not len(a.events):
        print("Acquisition failed....")
        eng.close()
        return 0
    print("Acquired!")
    print(f"refined fmax: {float(a.refined[0]['f']):f}")
    if args.freq_offset is not None:
        print(args.freq_offset)
    if r.plan.status:
        print(f"not decoded: {FILE_STATUS[r.plan.status]}")
        eng.close()
        return 1
    z_hat = r.z_hat.cpu().numpy().astype(np.float32).ravel()
    if r.n_errors is not None:
        best, n_ref = 1.0, z_ref[1]
        for f in range(20):                                            # the script's lines: a shift is printed when it improves on the best so far
            n_bits = n_ref - 240 * f
            if n_bits <= 0 or r.n_errors[f] < 0:
                break
            if r.n_errors[f] / n_bits < best:
                best = r.n_errors[f] / n_bits
                print(f"f: {f:2d} n_bits: {n_bits:d} n_errors: {int(r.n_errors[f]):d} BER: {best:5.3f}")
    fh = r.features.cpu().numpy().reshape(-1, 21)
    out = np.zeros((len(fh), 36), np.float32); out[:, :20] = fh[:, :20]
    out.tofile(args.features_hat)
    if args.write_latent:
        z_hat.tofile(args.write_latent)
    eng.close()
    return 0


def _chirp(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli chirp", description="Generates a .f32 IQIQI chirp file for HF channel SNR measurement (chirp.py)")
    ap.add_argument("f32", type=str, help="path to output IQ .f32 file")
    ap.add_argument("Nsec", type=float, help="output file length in seconds")
    ap.add_argument("--flow", type=float, default=400.0, help="lower freq limit for chirp (default 400 Hz)")
    ap.add_argument("--fhigh", type=float, default=2000.0, help="upper limit for chirp (default 2000 Hz)")
    ap.add_argument("--amp", type=float, default=0.25, help="magnitude of chirp (default 0.25)")
    args = ap.parse_args(argv)
    from . import engine
    engine.chirp(args.Nsec, args.flow, args.fhigh, args.amp).tofile(args.f32)
    return 0


def _specgram(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli specgram", description="Spectrogram of an 8 kHz recording (plot_specgram.m: 160 ms Hann window every 20 ms, normalised by "
                                 "the recording's maximum, clipped 20 dB and 3 dB below it) as a grey-scale PNG, time to the right and frequency upward; the transforms and "
                                 "the 256 levels run on the device (rade_batch_specgram).  No axes, colour map or JPEG")
    ap.add_argument("input", type=str, help="raw int16 mono (.s16 / .raw, what load_raw reads), ..IQIQ.. .f32 (the real part is drawn) or a 16-bit mono .wav (read through the "
                    "wave module; load_raw would plot its 44 header bytes as 22 samples)")
    ap.add_argument("png", type=str, help="path to the output .png")
    ap.add_argument("--fmin", type=float, default=0.0, help="lower edge of the displayed band (default 0 Hz)")
    ap.add_argument("--fmax", type=float, default=3000.0, help="upper edge of the displayed band (default 3000 Hz)")
    args = ap.parse_args(argv)
    import torch
    from . import engine, ota
    name = args.input.lower()
    if name.endswith(".wav"):
        import wave
        with wave.open(args.input, "rb") as wf:
            if wf.getsampwidth() != 2 or wf.getnchannels() != 1 or wf.getframerate() != engine.CNO_FS:
                raise SystemExit("radae_amd.cli specgram: a .wav must be 16-bit mono at 8000 Hz")
            x = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2").astype(np.int16)
    elif name.endswith(".f32"):
        x = np.fromfile(args.input, dtype=np.csingle)
    else:
        x = np.fromfile(args.input, dtype=np.int16)
    if len(x) <= engine.SPEC_WIN:
        raise SystemExit(f"radae_amd.cli specgram: {len(x)} samples; more than {engine.SPEC_WIN} are needed (specgram raises an error)")
    eng = engine.BatchEngine(1, max_tx_mf=1)
    img, ns, peak = eng.specgram(torch.tensor(x[None], device="cuda"), fmin=args.fmin, fmax=args.fmax)
    ota.write_png(args.png, img[0], ns[0])
    eng.close()
    print(f"{int(ns[0])} slices x {img.shape[2]} bins, peak {float(peak[0]):.6g}", file=sys.stderr)
    return 0


def _do_plots(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli do_plots", description="radae_plots.m: do_plots on a --write_rx / --write_tx file at 8 kHz: the Welch power spectrum "
                                 "(Hamming window, 1024-point transform), mean power, PAPR, the PAPR of the first 160 samples and the 99 % power bandwidth around "
                                 "1500 Hz; the transforms and the sums run on the device (rade_batch_psd, rade_batch_sigstat).  Prints the script's two lines; no plots")
    ap.add_argument("rx", type=str, help="..IQIQ.. float32 samples (what --write_rx writes), or with --int16 raw int16 mono")
    ap.add_argument("--win", type=int, default=0, help="window length, 16..1024 (default: what pwelch is recalled to take for an empty window, "
                    "2^ceil(log2(sqrt(2 n))), at most 1024)")
    ap.add_argument("--step", type=int, default=0, help="hop between segments, 1..win (default: 50 %% overlap)")
    ap.add_argument("--int16", type=float, default=None, metavar="GAIN", help="the file is raw int16 mono, scaled by GAIN as int16tof32.py scales it")
    ap.add_argument("--save_text", type=str, default="", help="write two columns, frequency in Hz and 10 log10 P minus its maximum (the curve of the script's figure 8)")
    args = ap.parse_args(argv)
    import torch
    from . import engine
    x = np.fromfile(args.rx, dtype=np.int16 if args.int16 is not None else np.csingle)
    win = args.win or min(engine.psd_octave_default(max(len(x), 1))[0], engine.PSD_NFFT)
    step = args.step or win - win // 2
    if len(x) < win:
        raise SystemExit(f"radae_amd.cli do_plots: {len(x)} samples; at least the window's {win} are needed")
    eng = engine.BatchEngine(1, max_tx_mf=1)
    xt = torch.tensor(x[None], device="cuda")
    kw = {} if args.int16 is None else {"gain": args.int16}
    P, _ = eng.psd(xt, win=win, step=step, **kw)
    st = eng.sigstat(xt, **kw)
    eng.close()
    P = P[0].cpu().numpy().astype(np.float64)
    print("Pav: %f PAPRdB: %5.2f PilotPAPRdB: %5.2f" % (st.Pav[0], st.PAPRdB[0], st.PilotPAPRdB[0]))
    bw = engine.psd_bandwidth(P)
    if bw is None:
        raise SystemExit("radae_amd.cli do_plots: 99 % of the power is not reached inside the spectrum (the script's index error)")
    print("bandwidth (Hz): %f power/total_power: %f" % bw)
    if args.save_text:
        with np.errstate(divide="ignore"):
            dB = 10 * np.log10(P)
        np.savetxt(args.save_text, np.column_stack([np.arange(len(P)) * engine.PSD_FS / len(P), dB - dB.max()]), fmt="%.6f")
    return 0


def _train_decoder(argv):
    ap = argparse.ArgumentParser(prog="radae_amd.cli train_decoder", description="train.py for the decoder alone, on latents that were received (--write_latent of `rx` and "
                                 "`inference`) and the features that were sent: sequences of --sequence-length frames as dataset.py cuts them, shuffled batches with the "
                                 "last ragged one dropped, distortion_loss, Adam with betas (0.8, 0.95) and lr / (1 + decay step); every step runs on the device "
                                 "(rade_train_dec_step).  Writes a DNNw blob that `rx --decode` and `inference` load.  The shuffle and the aux bits are seeded (the "
                                 "reference draws them unseeded); no checkpoints, no plots.  NO QUANTISATION NOISE in training: the float weights are quantised to "
                                 "int8 only when the blob is written, which moves the decoder's output (by about 7 %% of full scale after ten steps from a perturbed "
                                 "model19), and weights that were exactly 0 move too, so the blob loses the input matrices' block sparsity and grows")
    ap.add_argument("model", type=str, help="DNNw blob to start from")
    ap.add_argument("z_hat", type=str, help="received latents, float32 [rows, 80]: one row per 4 feature frames")
    ap.add_argument("features", type=str, help="the transmitted features, float32 [frames, 36]")
    ap.add_argument("out", type=str, help="path of the trained DNNw blob")
    ap.add_argument("--sequence-length", type=int, default=256, help="feature frames per sequence (a multiple of 4), default 256")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--lr-decay-factor", type=float, default=2.5e-5)
    ap.add_argument("--auxdata", action="store_true", help="train the 21st feature on a +-1 symbol held over 4 frames")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    from . import train
    try:
        z, f = train.load_sequences(args.z_hat, args.features, args.sequence_length, args.auxdata, args.seed)
        train.train_decoder(args.model, z, f, args.out, args.batch_size, args.epochs, args.lr, args.lr_decay_factor, args.seed, log=lambda m: print(m, file=sys.stderr))
    except ValueError as e:
        raise SystemExit(f"radae_amd.cli train_decoder: {e}")
    return 0


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    cmds = {"txe": _txe, "rxe": _rxe, "inference": _inference, "multipath_samples": _multipath_samples, "bbfm_inference": _bbfm_inference, "analog_fm": _analog_fm,
            "est_cno": _est_cno, "est_snr": _est_snr, "rx": _rx, "chirp": _chirp, "specgram": _specgram, "do_plots": _do_plots, "train_decoder": _train_decoder}
    if not argv or argv[0] not in cmds:
        print(__doc__, file=sys.stderr)
        return 2
    return cmds[argv[0]](argv[1:])


if __name__ == "__main__":
    raise SystemExit(main())
