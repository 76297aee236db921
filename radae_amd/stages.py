"""The front-end stages of the batched engine, the Python mirror of radae_amd/csrc/rade_stages.c: rate-Rs channel, resampler, sound-card wire, rate converter, analog FM,
the channel and the Doppler generator in pieces, C/No of the chirp header, the trials of the pilot SNR estimator, the spectrogram and the whole-file pilot acquisition (its driver: radae_amd/acq.py).

Three layers: the host-only helpers of each stage (`*_count`, `*_taps`, `*_plan`, ..: no handle, no GPU); BatchStages, the plain base class that gives BatchEngine one
method per stage call (it uses only self.lib, self.h, self.B and self.device, so this module does not import engine.py); and the classes that apply a stateless stage to
streams that arrive in pieces.  The row / count / stride helpers every stage method checks its tensors with are stated once, ahead of the class.  torch is imported inside
the functions that need it, as in engine.py.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from .abi import (FM_C64, FM_F32, FM_OUT_COMPLEX, FM_OUT_REAL, RATE_C64, RATE_S16_IQ, RATE_S16_REAL, RESAMPLE_MODES, SPEC_C64, SPEC_S16_REAL, WIRE_IQ, WIRE_REAL, AcqEvent, AcqHop, AcqLog, EQ_MODES, FilePlan, FileRxIn,
                  AcqRefined, AcqRefineIn, AcqResult, CnoParams, CnoPlan, CnoResult, FmDemodParams, FmModParams, RateParams, PsdPlan, ResampleParams, SigstatResult, SnrParams, SnrPoint, SnrSums, SpecgramParams, SpecgramPlan, load_library)


class WireMeters(NamedTuple):
    """Level of what wire_out wrote, one value per stream: the largest |x scale| (before saturation), the RMS of x scale over the written components (NaN components
    excluded), and how many components saturated / were NaN."""
    peak: np.ndarray
    rms: np.ndarray
    clipped: np.ndarray
    nan: np.ndarray


RESAMPLE_PPM_MAX = 50000.0

def ppm_from_rates(fs_tx: float, fs_rx: float) -> float:
    """The clock offset in ppm of a receiver sampling at fs_rx what was sent at fs_tx (`sox -r 8000 .. -r 8020`): step = fs_tx / fs_rx input samples per output
    sample, so ppm = (fs_tx / fs_rx - 1) 1e6 (dsp.py:574's convention); ppm_from_rates(8000, 8020) = -2493.77."""
    return (float(fs_tx) / float(fs_rx) - 1.0) * 1e6


def resample_count(in_end: int, t0: float = 0.0, ppm: float = 0.0) -> int:
    """rade_resample_count: how many outputs n >= 0 have their position t0 + n (1 + ppm 1e-6) below in_end input samples."""
    n = int(load_library().rade_resample_count(int(in_end), float(t0), float(ppm)))
    if n < 0:
        raise ValueError(f"rade_resample_count refuses ppm {ppm!r}, t0 {t0!r}, in_end {in_end!r} (|ppm| <= 50000, |t0| <= 2^29, outputs x step <= 2^62)")
    return n


def resample_taps() -> np.ndarray:
    """rade_resample_taps: the float32 [257, 32] Kaiser-windowed sinc table of the sinc32 mode (host only)."""
    t = np.zeros((257, 32), np.float32)
    load_library().rade_resample_taps(t.ctypes.data)
    return t



def rate_count(in_end: int, L: int, M: int) -> int:
    """rade_rate_count: how many outputs n >= 0 have their position n M / L below in_end input samples."""
    n = int(load_library().rade_rate_count(int(in_end), int(L), int(M)))
    if n < 0:
        raise ValueError(f"rade_rate_count refuses L {L!r}, M {M!r}, in_end {in_end!r} (L, M >= 1, outputs x M <= 2^62)")
    return n


def rate_taps(L: int, M: int) -> np.ndarray:
    """rade_rate_taps: the float32 [L', T] Kaiser-windowed sinc table of the ratio L / M reduced to L' / M' (host only), T = 32 ceil(M' / L')."""
    lib = load_library()
    T = int(lib.rade_rate_taps(int(L), int(M), None))
    if T < 0:
        raise ValueError(f"rade_rate_taps refuses the ratio {L!r} / {M!r} (L, M >= 1; reduced: ceil(M / L) <= 8, L T <= 16384)")
    t = np.zeros((int(L) // int(np.gcd(int(L), int(M))), T), np.float32)
    assert lib.rade_rate_taps(int(L), int(M), t.ctypes.data) == T
    return t


FM_DE_EMP_TC = 50e-6                                                               # fm.m:17


def fm_sigma(CNdB: float, Fs: float, fm_max: float, fd: float) -> float:
    """rade_fm_sigma: sqrt(Fs / (CN Bfm)), Bfm = 2 (fd + fm_max): the noise sigma that gives a unit carrier the C/N CNdB inside Carson's bandwidth (fm.m:16,162)."""
    v = float(load_library().rade_fm_sigma(float(CNdB), float(Fs), float(fm_max), float(fd)))
    if v < 0:
        raise ValueError(f"rade_fm_sigma refuses CNdB {CNdB!r}, Fs {Fs!r}, fm_max {fm_max!r}, fd {fd!r} (finite, rates > 0)")
    return v


def fm_deemph_len(Fs: float, tc: float = FM_DE_EMP_TC) -> int:
    """rade_fm_deemph_len: K of the folded de-emphasis, the first power of a = 1 - 1 / (tc Fs) below 2^-30."""
    K = int(load_library().rade_fm_deemph_len(float(Fs), float(tc)))
    if K < 0:
        raise ValueError(f"rade_fm_deemph_len refuses Fs {Fs!r}, tc {tc!r}")
    return K


def fm_taps(Fs: float, fm_max: float, fd: float, ntaps: int = 201, de_emp_tc: float = 0.0):
    """rade_fm_taps: (bin, bout) as float64 arrays, the two least-squares filters of fm.m:41-47; with de_emp_tc > 0 the de-emphasis pole is folded into bout
    (ntaps + K - 1 values).  Host only.  fm_demod takes them rounded to float32."""
    lib = load_library()
    N2 = int(lib.rade_fm_taps(float(Fs), float(fm_max), float(fd), int(ntaps), float(de_emp_tc), None, None))
    if N2 < 0:
        raise ValueError(f"rade_fm_taps refuses Fs {Fs!r}, fm_max {fm_max!r}, fd {fd!r}, ntaps {ntaps!r}, de_emp_tc {de_emp_tc!r} (ntaps odd, 3..511; at most 512 taps folded)")
    b1, b2 = np.zeros(int(ntaps), np.float64), np.zeros(N2, np.float64)
    assert lib.rade_fm_taps(float(Fs), float(fm_max), float(fd), int(ntaps), float(de_emp_tc), b1.ctypes.data, b2.ctypes.data) == N2
    return b1, b2


def fm_pre_emphasis(mod: np.ndarray, Fs: float, tc: float = FM_DE_EMP_TC) -> np.ndarray:
    """fm.m:80-83 on the host (not on the device: the normalisation needs the whole signal): filter([1, -(1 - 1 / (tc Fs))], 1, mod) / max of it, per row."""
    mod = np.asarray(mod, np.float64)
    a = 1.0 - 1.0 / (tc * Fs)
    y = mod.copy()
    y[..., 1:] -= a * mod[..., :-1]
    return y / y.max(axis=-1, keepdims=True)


def multipath_gain(taps) -> float:
    """rade_multipath_gain: 1 / sqrt(2 ((2/3) R0 + (1/3) R1)), R0 = 2 sum t^2, R1 = 2 sum t[k] t[k + 1] of the float32 taps: the hf_gain that gives the two linearly
    interpolated Doppler paths unit power in expectation (host only; what multipath_piece uses unless it is given one)."""
    t = np.ascontiguousarray(taps, dtype=np.float32)
    v = float(load_library().rade_multipath_gain(t.ctypes.data, t.size))
    if v <= 0:
        raise ValueError("rade_multipath_gain refuses the taps (1..256 finite values, not all zero)")
    return v


CNO_FS, CNO_HOP = 8000, 2000                                                     # est_CNo.py:23, :31 (Fs // 4)


def cno_plan(window_time: float = 4.0, flow: float = 400.0, fhigh: float = 2000.0) -> CnoPlan:
    """rade_cno_plan: N, J = N / 2000, the bins of both bands together and the four bin limits of est_CNo.py:25-42 (host only).  Refused: what rade_batch_cno_est refuses."""
    q = CnoPlan()
    if load_library().rade_cno_plan(C.byref(CnoParams(float(window_time), float(flow), float(fhigh))), C.byref(q)):
        raise ValueError(f"rade_cno_plan refuses window_time {window_time!r}, flow {flow!r}, fhigh {fhigh!r} (window_time a multiple of 0.25 s up to 8 s -- the one deviation "
                         "from est_CNo.py, which takes any; 0 <= flow_bin < fhigh_bin, a noise band of at least one bin that ends inside the window's N bins)")
    return q


def cno_windows(n: int, N: int) -> int:
    """len(np.arange(0, n - N, 2000)): the windows est_CNo.py evaluates in n samples"""
    return max(-(-(int(n) - int(N)) // CNO_HOP), 0)


def chirp(nsec: float, flow: float = 400.0, fhigh: float = 2000.0, amp: float = 0.25) -> np.ndarray:
    """rade_chirp: chirp.py:50-65 on the host, int(nsec * 8000) complex64 samples of the triangular flow .. fhigh sweep."""
    x = np.zeros(int(nsec * CNO_FS), np.complex64)
    if load_library().rade_chirp(x.ctypes.data, x.size, float(flow), float(fhigh), float(amp)):
        raise ValueError(f"rade_chirp refuses flow {flow!r}, fhigh {fhigh!r}, amp {amp!r} (finite values)")
    return x


SNR_NC, SNR_NS, SNR_TMF = 30, 4, 0.12                                              # carriers; data symbols per modem frame; a modem frame in seconds (model.Tmf)
SNR_M, SNR_C = 0.8070, 2.513                                                       # dsp.py:415-416: the receiver's correction, est_snr_curves.sh's -m / -c


def snr_windows_rows(T: float = 1.0) -> int:
    """est_snr.py:230: Nw = int(T // Tmf), the pilot rows of a window of T seconds (8 at the default -T 1.0)"""
    return int(float(T) // SNR_TMF)


def snr_sigma(snrdB: float) -> float:
    """rade_snr_sigma: sqrt(Es / 10^(snrdB / 10)) / sqrt 2, Es = sum (pg P)^2 / Nc: the noise per component at a set point (est_snr.py:57-59; host only)"""
    return float(load_library().rade_snr_sigma(float(snrdB)))


def _snr_sums(sums) -> np.ndarray:
    return np.ascontiguousarray(sums, np.dtype(SnrSums))


def snr_finish(sums, eq_ls: bool = False, c: float = 0.0, m: float = 1.0) -> np.ndarray:
    """rade_snr_finish over an array of abi.SnrSums records (any shape): a record array of abi.SnrPoint of the same shape (snrdB_genie, snrdB_est, NdB_genie, NdB_est;
    est_snr.py:96-122).  S2 = 0 follows IEEE, as the script does: +inf.  Host only."""
    a = _snr_sums(sums)
    out = np.zeros(a.shape, np.dtype(SnrPoint))
    lib = load_library()
    ap, op = C.cast(a.ctypes.data, C.POINTER(SnrSums)), C.cast(out.ctypes.data, C.POINTER(SnrPoint))
    for i in range(a.size):
        if lib.rade_snr_finish(C.byref(ap[i]), int(bool(eq_ls)), float(c), float(m), C.byref(op[i])):
            raise ValueError(f"rade_snr_finish refuses c {c!r}, m {m!r} (finite, m != 0)")
    return out


def snr_fit(x, y):
    """rade_snr_fit: (m, c) of the least-squares line y = m x + c, np.polyfit(x, y, 1) (est_snr.py:178).  Host only."""
    x = np.ascontiguousarray(x, np.float64).ravel(); y = np.ascontiguousarray(y, np.float64).ravel()
    if x.shape != y.shape:
        raise ValueError("snr_fit: x and y of one length")
    m, c = C.c_double(0.0), C.c_double(0.0)
    if load_library().rade_snr_fit(x.ctypes.data, y.ctypes.data, x.size, C.byref(m), C.byref(c)):
        raise ValueError("rade_snr_fit refuses the points (at least two, x not constant, finite values)")
    return m.value, c.value


def snr_track(sums, c: float = SNR_C, m: float = SNR_M, state: float = 0.0) -> np.ndarray:
    """rade_snr_track over the sums of n windows of Nw = 1 (a 1-D array of abi.SnrSums) in turn: float64 [n], the smoothed 3 kHz SNR the live receiver holds after
    each frame (dsp.py:438-456), from `state` before the first.  Host only."""
    a = _snr_sums(sums).ravel()
    out = np.zeros(a.size, np.float64)
    st = C.c_double(float(state))
    if load_library().rade_snr_track(a.ctypes.data, a.size, float(c), float(m), C.byref(st), out.ctypes.data):
        raise ValueError(f"rade_snr_track refuses c {c!r}, m {m!r} (finite, m != 0)")
    return out


class SnrSweep(NamedTuple):
    """snr_sweep: per channel, in the order est_snr.py's sweep appends them (set point major, window minor)"""
    snrdB_genie: np.ndarray  # float64 [n_channels, n_set_points * Nt]: the x of the script's plot and of its --save_text
    snrdB_est: np.ndarray    # the y
    NdB_genie: np.ndarray
    NdB_est: np.ndarray
    fit: np.ndarray          # float64 [n_channels, 2]: (m, c) of np.polyfit(snrdB_genie, snrdB_est, 1)
    sums: np.ndarray         # abi.SnrSums [n_channels, n_set_points, Nt]


def snr_sweep(channels, Nt: int, T: float = 1.0, set_points=range(-5, 20), eq_ls: bool = False, c: float = 0.0, m: float = 1.0, seed: int = 1, h_step: int = SNR_NS + 1,
              engine=None) -> SnrSweep:
    """est_snr.py's sweep for several channels in ONE device call: one stream per (channel, set point), Nt windows of Nw = int(T // 0.12) pilot rows each, generated
    noise from `seed`.  channels: a sequence whose entries are None (AWGN, h = 1) or the channel's H as complex64 [rows, 30] (numpy or cuda), of which row
    (k Nw + i) h_step is used: h_step = 5 for a rate-Rs file as the script decimates it (h[::Ns+1]), 1 for one row per modem frame; all set points of a channel use
    the same H windows, as the script does.  engine: a BatchEngine of len(channels) * len(set_points) streams (default: one is opened for the call and closed).
    The estimator's arithmetic is the script's; the noise is the engine's generator, not np.random, so single points differ from a run of the script."""
    import torch
    set_points = [float(v) for v in set_points]
    Nw, n_ch, n_sp = snr_windows_rows(T), len(channels), len(set_points)
    if Nw < 1 or Nt < 1 or not n_ch or not n_sp:
        raise ValueError("snr_sweep: T of at least one modem frame (0.12 s), Nt >= 1, at least one channel and one set point")
    B = n_ch * n_sp
    own = engine is None
    if own:
        from .engine import BatchEngine
        engine = BatchEngine(B, max_tx_mf=1)
    try:
        if engine.B != B:
            raise ValueError(f"snr_sweep: the engine has {engine.B} streams, {n_ch} channels x {n_sp} set points need {B}")
        rows = (Nt * Nw - 1) * h_step + 1
        H = None
        if any(ch is not None for ch in channels):
            H = torch.ones((n_ch, rows, SNR_NC), dtype=torch.complex64, device=engine.device)
            for j, ch in enumerate(channels):
                if ch is not None:
                    t = torch.as_tensor(ch).to(device=engine.device, dtype=torch.complex64)
                    if t.dim() != 2 or t.shape[1] != SNR_NC or t.shape[0] < rows:
                        raise ValueError(f"snr_sweep: channel {j} needs H of at least {rows} rows x {SNR_NC} carriers, got {tuple(t.shape)}")
                    H[j] = t[:rows]
            H = H[:, None].expand(n_ch, n_sp, rows, SNR_NC).reshape(B, rows, SNR_NC).contiguous()      # stream = channel * n_set_points + set point
        sigma = np.array([snr_sigma(v) for v in set_points] * n_ch, np.float32)
        sums = engine.snr_trials(Nt, Nw, sigma, H=H, h_step=h_step, seed=seed).reshape(n_ch, n_sp, Nt)
    finally:
        if own:
            engine.close()
    pts = snr_finish(sums, eq_ls, c, m).reshape(n_ch, n_sp * Nt)
    fit = np.array([snr_fit(pts["snrdB_genie"][j], pts["snrdB_est"][j]) for j in range(n_ch)], np.float64)
    return SnrSweep(pts["snrdB_genie"].copy(), pts["snrdB_est"].copy(), pts["NdB_genie"].copy(), pts["NdB_est"].copy(), fit, sums)


SPEC_WIN, SPEC_STEP, SPEC_NFFT = 1280, 160, 2048                                   # plot_specgram.m:6-10 at Fs = 8000
SPEC_LO, SPEC_HI = 10.0 ** (-20 / 10), 10.0 ** (-3 / 10)                           # plot_specgram.m:13-14


def specgram_plan(fmin: float = 0.0, fmax: float = 3000.0, lo: float = SPEC_LO, hi: float = SPEC_HI) -> SpecgramPlan:
    """rade_specgram_plan: the display band k0..k1 (inclusive) of a 2048-point transform at 8 kHz, n_bins = k1 - k0 + 1, and the fixed geometry (host only)."""
    q = SpecgramPlan()
    if load_library().rade_specgram_plan(C.byref(SpecgramParams(float(fmin), float(fmax), float(lo), float(hi), None)), C.byref(q)):
        raise ValueError(f"rade_specgram_plan refuses fmin {fmin!r}, fmax {fmax!r}, lo {lo!r}, hi {hi!r} (finite, fmin <= fmax with a bin of 1..1023 between them, 0 < lo < hi <= 1)")
    return q


def specgram_slices(n: int) -> int:
    """rade_specgram_slices: len(np.arange(0, n - 1280, 160)), the slices specgram makes of n samples"""
    return int(load_library().rade_specgram_slices(int(n)))


def specgram_window() -> np.ndarray:
    """rade_specgram_window: hanning(1280) = 0.5 - 0.5 cos(2 pi (i + 1) / 1281) as float32 (host only)"""
    w = np.zeros(SPEC_WIN, np.float32)
    load_library().rade_specgram_window(w.ctypes.data)
    return w


def specgram_levels(lo: float = SPEC_LO, hi: float = SPEC_HI) -> np.ndarray:
    """rade_specgram_levels: the 255 thresholds T[j] = lo (hi / lo)^((j - 0.5) / 255), j = 1..255, as float32 (host only)"""
    t = np.zeros(255, np.float32)
    if load_library().rade_specgram_levels(float(lo), float(hi), t.ctypes.data):
        raise ValueError(f"rade_specgram_levels refuses lo {lo!r}, hi {hi!r} (0 < lo < hi <= 1)")
    return t


PSD_NFFT, PSD_FS, PSD_HEAD = 1024, 8000.0, 160                                     # radae_plots.m:53, :66: pwelch(.., 1024, Fs), rx(1:160)


class SigStat(NamedTuple):
    """BatchStages.sigstat: per stream, numpy arrays [B]; a stream without power (or without samples) has nan where the script's 0 / 0 has"""
    n: np.ndarray            # int64: samples
    sum2: np.ndarray         # float64: sum |x|^2
    peak2: np.ndarray        # float64: max |x|^2
    head_sum2: np.ndarray    # the same two over the first min(n, head) samples
    head_peak2: np.ndarray
    Pav: np.ndarray          # sum2 / n
    PAPRdB: np.ndarray       # 10 log10(peak2 / Pav)
    PilotPAPRdB: np.ndarray  # 10 log10(head_peak2 / (head_sum2 / min(n, head)))


def psd_plan(win: int = 1024, step: int = 512) -> PsdPlan:
    """rade_psd_plan: (nfft, win, step, run) of rade_batch_psd, run = the segments a workgroup adds in float32 before the sums go on in double (host only)"""
    q = PsdPlan()
    if load_library().rade_psd_plan(int(win), int(step), C.byref(q)):
        raise ValueError(f"rade_psd_plan refuses win {win!r}, step {step!r} (16 <= win <= 1024, 1 <= step <= win)")
    return q


def psd_segments(n: int, win: int, step: int) -> int:
    """rade_psd_segments: len(range(0, n - win + 1, step)), the whole segments of n samples"""
    return int(load_library().rade_psd_segments(int(n), int(win), int(step)))


def psd_window(win: int) -> np.ndarray:
    """rade_psd_window: hamming(win) = 0.54 - 0.46 cos(2 pi i / (win - 1)) as float32 (host only)"""
    w = np.zeros(max(int(win), 0), np.float32)
    if load_library().rade_psd_window(int(win), w.ctypes.data):
        raise ValueError(f"rade_psd_window refuses win {win!r} (16 <= win <= 1024)")
    return w


def psd_octave_default(n: int):
    """rade_psd_octave_default: (win, step) that pwelch(x, [], []) is RECALLED (not verified) to take for n samples: 2^ceil(log2(sqrt(n / 0.5))) at 50 % overlap"""
    w, s = C.c_int(0), C.c_int(0)
    if load_library().rade_psd_octave_default(int(n), C.byref(w), C.byref(s)):
        raise ValueError(f"rade_psd_octave_default refuses n {n!r}")
    return w.value, s.value


def psd_bandwidth(P, fs: float = PSD_FS, centre_hz: float = 1500.0, frac: float = 0.99):
    """rade_psd_bandwidth: radae_plots.m's bandwidth() on one spectrum P[0..N-1] (any float type; the sums are formed in double): (bandwidth in Hz, power / total power),
    or None where the fraction is not reached before the band passes the last bin (the script's index error)"""
    P = np.ascontiguousarray(np.asarray(P.detach().cpu().numpy() if hasattr(P, "detach") else P, np.float64))
    assert P.ndim == 1
    bw, ratio = C.c_double(0.0), C.c_double(0.0)
    if load_library().rade_psd_bandwidth(P.ctypes.data, len(P), float(fs), float(centre_hz), float(frac), C.byref(bw), C.byref(ratio)):
        return None
    return bw.value, ratio.value


def acq_hops(n: int) -> int:
    """rade_acq_hops: the frames rx.py's loop visits in n samples (hop k while n - 961 k >= 2112)."""
    return int(load_library().rade_acq_hops(int(n)))


def acq_fmax(hops: np.ndarray) -> np.ndarray:
    """rade_acq_fmax of every record: -50 + 2.5 f_ind, and the script's 0.0 where no cell exceeded 0."""
    return np.where(hops["Dtmax12"] > 0, -50.0 + 2.5 * hops["f_ind"], 0.0)


def acq_track(hops: np.ndarray, acq_test: bool = False):
    """rade_acq_track over one stream's hop records (a 1-D record array of abi.AcqHop): (events, log), record arrays of abi.AcqEvent (hop, tmax, f_ind) and of
    abi.AcqLog [n_hops] (state 0 search / 1 candidate, tmax_candidate, valid_count as the script prints them in the hop's line).  Host only."""
    hops = np.ascontiguousarray(hops, np.dtype(AcqHop))
    assert hops.ndim == 1
    ev = np.zeros(max(len(hops), 1), np.dtype(AcqEvent))
    log = np.zeros(max(len(hops), 1), np.dtype(AcqLog))
    k = load_library().rade_acq_track(hops.ctypes.data, len(hops), int(bool(acq_test)), ev.ctypes.data, len(ev), log.ctypes.data)
    if k < 0:
        raise ValueError("rade_acq_track refused its arguments")
    return ev[:k], log[:len(hops)]


def acq_stats(events: np.ndarray, refined: np.ndarray, n_hops: int, ntap: int = 101, fmax_target: float = 0.0, acq_time_target: float = 1.0) -> AcqResult:
    """rade_acq_stats: passes, fails, pfail, mean_acq_time and passed of rx.py --acq_test (host only).  ntap: 101 with the input band-pass, 0 without."""
    events = np.ascontiguousarray(events, np.dtype(AcqEvent)); refined = np.ascontiguousarray(refined, np.dtype(AcqRefined))
    assert events.ndim == 1 and events.shape == refined.shape
    r = AcqResult()
    if load_library().rade_acq_stats(events.ctypes.data, refined.ctypes.data, len(events), int(n_hops), int(ntap), float(fmax_target), float(acq_time_target), C.byref(r)):
        raise ValueError("rade_acq_stats refused its arguments")
    return r


def file_plan(n: int, hop: int, t: int, f: float, freq_offset=None) -> FilePlan:
    """rade_file_plan: where rx.py's normal run starts to demodulate a stream of n samples that acquired at hop `hop` (-1: not acquired) and whose refine -- called
    one frame later, at 960 (hop + 1) + tmax in a stream of n - (hop + 1) samples -- returned the absolute timing t and frequency f.  -> abi.FilePlan (start, n_mf,
    freq, status: an index into abi.FILE_STATUS).  freq_offset: the --freq_offset override.  Host only."""
    out = FilePlan()
    fo = None if freq_offset is None else C.byref(C.c_double(float(freq_offset)))
    if load_library().rade_file_plan(int(n), int(hop), int(t), float(f), fo, C.byref(out)):
        raise ValueError("rade_file_plan refused its arguments")
    return out


def ber_best(n_errors, n_ref: int):
    """rade_ber_best over one stream's 20 counts: (shift, BER) of the first strict minimum below 1, (-1, 1.0) when there is none.  Host only."""
    e = np.ascontiguousarray(n_errors, np.int64)
    assert e.shape == (20,)
    ber = C.c_double(1.0)
    return int(load_library().rade_ber_best(e.ctypes.data, int(n_ref), C.byref(ber))), float(ber.value)


def _per_stream(B: int, v, dtype, what: str) -> np.ndarray:
    """a scalar (every stream) or B per-stream values -> a contiguous [B] array"""
    a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=dtype)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
        raise ValueError(f"{what}: a scalar or {B} per-stream values, got shape {a.shape}")
    return np.ascontiguousarray(np.broadcast_to(a, (B,)))


def _scalar_or_streams(B: int, v, what: str):
    """a scalar -> (its float, None); B per-stream values -> (0.0, float32 [B]): the two forms of a value that a call takes as a scalar or as a per-stream host array"""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return (float(v), None) if np.ndim(v) == 0 else (0.0, _per_stream(B, v, np.float32, what))


def _is_rows(t, B: int, dtype) -> bool:
    """2-D device rows [B, N] of `dtype` with unit inner stride (a row of at most one sample may carry any)"""
    return t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[0] == B and (t.stride(1) == 1 or t.shape[1] <= 1)


def _is_i16_rows(t, B: int) -> bool:
    """device int16 rows [B, N] (one channel, or ..IQIQ..) or [B, N, 2] (I, Q) with unit inner strides (a [B, N, 2] row of at most one sample may carry any)"""
    import torch
    return t.is_cuda and t.dtype == torch.int16 and t.shape[0] == B and (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 2)) and t.stride(-1) == 1 \
        and (t.dim() == 2 or t.stride(1) == 2 or t.shape[1] <= 1)


def _counts(B: int, v, N: int, what: str) -> np.ndarray:
    """per-stream counts within a row of N samples (None: the whole row of every stream) -> int32 [B]"""
    n = _per_stream(B, N if v is None else v, np.int32, what)
    if n.min() < 0 or n.max() > N:
        raise ValueError(f"{what}: between 0 and the {N} samples of a row")
    return n


def _row_stride(t, row: int) -> int:
    """the row stride of a [B, ..] tensor in elements; a one-row tensor may carry any stride in its first dimension (0 from numpy's [None]): its row of `row` elements"""
    return t.stride(0) if t.shape[0] > 1 else row


def _out_rows(out, B: int, n, width: int, device):
    """complex64 output rows of at least max n: the caller's `out`, checked, or zeros [B, max(width, 1)]"""
    import torch
    if out is None:
        out = torch.zeros((B, max(int(width), 1)), dtype=torch.complex64, device=device)
    assert out.is_cuda and out.dtype == torch.complex64 and out.dim() == 2 and out.shape[0] == B and out.stride(1) == 1 and out.shape[1] >= n.max()
    return out


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class BatchStages:
    """The stage calls of a batched engine: every method is one call of rade_batch.h on every stream of the engine that inherits it."""

    def channel_rs_pa(self, z, sigma, H=None, noise=None, phase_offset: float = 0.0, seed: int = 0, want_stats: bool = False):
        """The rate-Rs channel of the bottleneck-3 model (rade_batch_channel_rs_pa; radae.py:603-634): z cuda float32 [B, n_steps, 80] -> z_hat of the same shape.
        Every OFDM symbol (40 floats of z: 20 carriers) through IDFT, PA limiter and DFT, then e^{j phase_offset}, H (float32 [B, 2 n_steps, 20] magnitudes or
        None = 1) and sigma times noise (complex64 [B, 2 n_steps, 20], unit variance; None -> Philox(seed), seed 0 = no noise).  sigma: a scalar for every
        stream or B per-stream values (sigma_from_EbNodB(.., rate_Fs=False)).  want_stats: also returns float64 [B, 3] = sum |tx'|^2, max |tx'|, sum |Y|^2 per
        stream (inference.py:215-227's Eq and PAPR; the call then synchronises)."""
        import torch
        assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.dim() == 3 and z.shape[0] == self.B and z.shape[2] == 80 and z.shape[1] >= 1
        n = z.shape[1]
        sigma, per = _scalar_or_streams(self.B, sigma, "sigma")
        if H is not None:
            assert H.is_cuda and H.dtype == torch.float32 and H.is_contiguous() and tuple(H.shape) == (self.B, 2 * n, 20)
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.complex64 and noise.is_contiguous() and tuple(noise.shape) == (self.B, 2 * n, 20)
        out = torch.empty_like(z)
        stats = np.zeros((self.B, 3), np.float64) if want_stats else None
        r = self.lib.rade_batch_channel_rs_pa(self.h, z.data_ptr(), H.data_ptr() if H is not None else None, noise.data_ptr() if noise is not None else None,
                                              out.data_ptr(), n, sigma, None if per is None else per.ctypes.data, phase_offset, seed,
                                              stats.ctypes.data if want_stats else None, _stream_ptr())
        if r != n:
            raise RuntimeError("rade_batch_channel_rs_pa failed")
        return (out, stats) if want_stats else out

    # ---- sample-clock offset -----------------------------------------------------------------
    def resample(self, x, ppm, t0=0.0, mode: str = "sinc32", n_out=None, n_in=None, n0=0, in_base=0, out=None):
        """The fractional resampler (rade_batch_resample): x cuda complex64 [B, N] -> (y complex64 [B, max n_out], n_out int32 [B]).  Output n of a stream sits at
        t0 + n (1 + ppm 1e-6) input samples: ppm_from_rates(8000, 8020) stretches the signal as a sound card at 8020 Hz does.  ppm, t0, n_out, n_in (readable samples of
        each row, default N), n0 (index of the first output written) and in_base (absolute index of x[b, 0]): scalars or B per-stream values.  n_out defaults to
        rade_resample_count(in_base + n_in, t0, ppm) - n0: every output whose position lies inside the input.  mode "sinc32" or "linear" (dsp.py:564-575).  Samples
        of y past a stream's n_out are zeros (left alone in a caller's `out`)."""
        import torch
        B = self.B
        assert _is_rows(x, B, torch.complex64)
        ppm = _per_stream(B, ppm, np.float64, "ppm"); t0 = _per_stream(B, t0, np.float64, "t0")
        n0 = _per_stream(B, n0, np.int64, "n0"); in_base = _per_stream(B, in_base, np.int64, "in_base")
        n_in = _counts(B, n_in, x.shape[1], "n_in")
        if n_out is None:
            n_out = np.array([max(resample_count(int(in_base[b]) + int(n_in[b]), t0[b], ppm[b]) - int(n0[b]), 0) for b in range(B)], np.int32)
        else:
            n_out = _per_stream(B, n_out, np.int32, "n_out")
        out = _out_rows(out, B, n_out, n_out.max(), x.device)
        p = ResampleParams(RESAMPLE_MODES[mode], 0.0, ppm.ctypes.data, t0.ctypes.data, n0.ctypes.data, in_base.ctypes.data)
        if self.lib.rade_batch_resample(self.h, x.data_ptr(), _row_stride(x, x.shape[1]), n_in.ctypes.data, out.data_ptr(), _row_stride(out, out.shape[1]), n_out.ctypes.data,
                                        C.byref(p), _stream_ptr()):
            raise RuntimeError("rade_batch_resample failed (|ppm| <= 50000, n0 >= 0, n_out <= the row of out)")
        return out, n_out

    # ---- sample-rate conversion --------------------------------------------------------------
    def rate_convert(self, x, L: int, M: int, n_out=None, n_in=None, n0=0, in_base=0, gain: float = 1.0, out=None):
        """The rational rate converter (rade_batch_rate_convert): output rate = input rate x L / M (L = 1, M = 6: 48 kHz -> 8 kHz).  x: cuda complex64 [B, N], int16 [B, N]
        (one real channel: the imaginary part of the output is +0) or int16 [B, N, 2] (I, Q); the int16 forms are scaled by `gain` as wire_in does.  Returns
        (y complex64 [B, max n_out], n_out int32 [B]).  Output n of a stream sits at input position n M / L.  n_out, n_in (readable samples of each row, default N), n0
        (index of the first output written) and in_base (absolute index of x[b, 0]): scalars or B per-stream values.  n_out defaults to
        rade_rate_count(in_base + n_in, L, M) - n0: every output whose position lies inside the input.  Samples of y past a stream's n_out are zeros (left alone in a
        caller's `out`)."""
        import torch
        B = self.B
        assert x.is_cuda and x.shape[0] == B
        if x.dtype == torch.complex64:
            assert _is_rows(x, B, torch.complex64)
            fmt, per = RATE_C64, 1
        else:
            assert _is_i16_rows(x, B)
            fmt, per = (RATE_S16_REAL, 1) if x.dim() == 2 else (RATE_S16_IQ, 2)
        N = x.shape[1]
        n0 = _per_stream(B, n0, np.int64, "n0"); in_base = _per_stream(B, in_base, np.int64, "in_base")
        n_in = _counts(B, n_in, N, "n_in")
        if n_out is None:
            n_out = np.array([max(rate_count(int(in_base[b]) + int(n_in[b]), L, M) - int(n0[b]), 0) for b in range(B)], np.int32)
        else:
            n_out = _per_stream(B, n_out, np.int32, "n_out")
        out = _out_rows(out, B, n_out, n_out.max(), x.device)
        p = RateParams(int(L), int(M), n0.ctypes.data, in_base.ctypes.data)
        if self.lib.rade_batch_rate_convert(self.h, x.data_ptr(), _row_stride(x, N * per), n_in.ctypes.data, fmt, gain, out.data_ptr(), _row_stride(out, out.shape[1]),
                                            n_out.ctypes.data, C.byref(p), _stream_ptr()):
            raise RuntimeError("rade_batch_rate_convert failed (L, M >= 1 with ceil(M / L) <= 8 and L T <= 16384 after reduction, a finite gain, n0 >= 0, n_out <= the row of out)")
        return out, n_out

    # ---- C/No of the chirp header ---------------------------------------------------------------
    def cno_est(self, x, n=None, window_time: float = 4.0, flow: float = 400.0, fhigh: float = 2000.0, bands: bool = False):
        """est_CNo.py over every stream (rade_batch_cno_est).  x: cuda complex64 [B, S] at 8 kHz; n: samples of each stream (a scalar or B values, default S), each at
        least N = int(8000 window_time).  Returns a list of B CnoResult (n_windows, n_positive, max_st, max_CNodB, max_SNRdB; the script's max_time is max_st / 8000); with
        bands=True also a float64 array [B, W, 2] of (C + N, band sum of No) per window, W = the most windows any stream has, zeros past a stream's own.  window_time must
        be a multiple of 0.25 s up to 8 s: the one deviation from the script.  The call synchronises the current stream."""
        import torch
        B = self.B
        assert _is_rows(x, B, torch.complex64)
        S = x.shape[1]
        n = _counts(B, n, S, "n")
        q = cno_plan(window_time, flow, fhigh)
        W = max(max(cno_windows(v, q.N) for v in n), 1)
        bh = np.zeros((B, W, 2), np.float64) if bands else None
        res = (CnoResult * B)()
        p = CnoParams(float(window_time), float(flow), float(fhigh))
        if self.lib.rade_batch_cno_est(self.h, x.data_ptr(), _row_stride(x, S), n.ctypes.data, C.byref(p), bh.ctypes.data if bands else None, W, C.byref(res), _stream_ptr()):
            raise RuntimeError(f"rade_batch_cno_est failed (every stream needs at least N = {q.N} samples)")
        out = list(res)
        return (out, bh) if bands else out

    # ---- trials of the pilot SNR estimator ------------------------------------------------------
    def snr_trials(self, n_windows, Nw: int, sigma, H=None, h_step: int = 1, noise=None, seed: int = 0, row0=0, want_noise: bool = False):
        """est_snr.py's trial over every window of every stream (rade_batch_snr_trials).  n_windows: windows of each stream (a scalar or B values, 0 allowed); Nw:
        pilot rows per window (1..66); sigma: the noise per component (a scalar or B values: snr_sigma(snrdB)); H: cuda complex64 [B, rows, 30] or None (h = 1), of which
        row (k Nw + i) h_step is used; noise: cuda complex64 [B, >= n_windows Nw, 30], unit variance per component, or None with a seed (generated: a function of
        seed, stream and the absolute row row0 + k Nw + i, so a stream in pieces gives the bits of the whole); row0: a scalar or B values.  Returns a numpy record array
        [B, W] of abi.SnrSums (S1, S1_sig, S1_cross, S1_noise, S2_genie, S2_est), W = the most windows any stream has (at least 1), zeros past a stream's own; with
        want_noise also the generated draws, cuda complex64 [B, W Nw, 30].  The call synchronises the current stream."""
        import torch
        B = self.B
        nw = _per_stream(B, n_windows, np.int32, "n_windows")
        sg = _per_stream(B, sigma, np.float32, "sigma")
        r0 = _per_stream(B, row0, np.int64, "row0")
        W = max(int(nw.max()), 1)
        rows = W * int(Nw)
        for t, what in ((H, "H"), (noise, "noise")):
            if t is not None:
                assert t.is_cuda and t.dtype == torch.complex64 and t.dim() == 3 and t.shape[0] == B and t.shape[2] == SNR_NC and t.stride(2) == 1 \
                    and (t.stride(1) == SNR_NC or t.shape[1] <= 1), f"{what}: cuda complex64 [B, rows, 30] with dense rows"
        if want_noise and (noise is not None or not seed):
            raise ValueError("snr_trials: want_noise goes with a seed")
        nout = torch.zeros((B, rows, SNR_NC), dtype=torch.complex64, device=self.device) if want_noise else None
        p = SnrParams(int(Nw), int(h_step), H.data_ptr() if H is not None else None, _row_stride(H, H.shape[1] * SNR_NC) if H is not None else 0, sg.ctypes.data,
                      r0.ctypes.data, noise.data_ptr() if noise is not None else None, nout.data_ptr() if want_noise else None,
                      _row_stride(noise, noise.shape[1] * SNR_NC) if noise is not None else rows * SNR_NC, int(seed))
        out = np.zeros((B, W), np.dtype(SnrSums))
        if self.lib.rade_batch_snr_trials(self.h, nw.ctypes.data, C.byref(p), out.ctypes.data, W, _stream_ptr()):
            raise RuntimeError("rade_batch_snr_trials failed (Nw 1..66, h_step 1..5, a seed or a noise tensor and not both, sigma >= 0, 0 <= row0 <= 2^40, H and noise "
                               "long enough for every stream's windows)")
        return (out, nout) if want_noise else out

    # ---- the spectrogram ------------------------------------------------------------------------
    def specgram(self, x, n=None, fmin: float = 0.0, fmax: float = 3000.0, lo: float = SPEC_LO, hi: float = SPEC_HI, peak=None, mag: bool = False, fmt=None,
                 gain: float = 1.0, img: bool = True):
        """plot_specgram.m over every stream (rade_batch_specgram).  x: cuda complex64 [B, S] at 8 kHz (the real part is used) or int16 [B, S] (scaled by `gain` as wire_in
        does); n: samples of each stream (a scalar or B values, default S), each above 1280.  Returns (img, n_slices, peak[, mag]): img uint8 [B, W, n_bins], the levels
        0..255 of bins k0..k1 (specgram_plan(fmin, fmax)) of every slice, W = the most slices any stream has, zeros past a stream's own (None with img=False); n_slices
        int32 [B]; peak float32 [B], each stream's largest |X| over bins 1..1023 -- or the values given as `peak` (a scalar or B values), which then normalise the image;
        with mag=True also float32 [B, W, 1023], |X[1..1023]|.  fmt: SPEC_C64 / SPEC_S16_REAL, default by x's dtype.  The call synchronises the current stream."""
        import torch
        B = self.B
        if fmt is None:
            fmt = SPEC_S16_REAL if x.dtype == torch.int16 else SPEC_C64
        assert _is_rows(x, B, torch.int16 if fmt == SPEC_S16_REAL else torch.complex64)
        S = x.shape[1]
        n = _counts(B, n, S, "n")
        q = specgram_plan(fmin, fmax, lo, hi)
        W = max(max(specgram_slices(v) for v in n), 1)
        im = torch.zeros((B, W, q.n_bins), dtype=torch.uint8, device=x.device) if img else None
        mg = torch.zeros((B, W, SPEC_NFFT // 2 - 1), dtype=torch.float32, device=x.device) if mag else None
        pin = None if peak is None else _per_stream(B, peak, np.float32, "peak")
        pk, ns = np.zeros(B, np.float32), np.zeros(B, np.int32)
        p = SpecgramParams(float(fmin), float(fmax), float(lo), float(hi), None if pin is None else pin.ctypes.data)
        if self.lib.rade_batch_specgram(self.h, x.data_ptr(), _row_stride(x, S), n.ctypes.data, fmt, gain, C.byref(p), im.data_ptr() if img else None, W * q.n_bins,
                                        mg.data_ptr() if mag else None, W * (SPEC_NFFT // 2 - 1), pk.ctypes.data, ns.ctypes.data, _stream_ptr()):
            raise RuntimeError("rade_batch_specgram failed (every stream needs more than 1280 samples; a finite gain; given peaks finite and >= 0; an output to write)")
        return (im, ns, pk, mg) if mag else (im, ns, pk)

    # ---- the waveform itself: Welch spectrum, power and peak -------------------------------------------
    def _psd_input(self, x, n, fmt):
        import torch
        if fmt is None:
            fmt = SPEC_S16_REAL if x.dtype == torch.int16 else SPEC_C64
        assert _is_rows(x, self.B, torch.int16 if fmt == SPEC_S16_REAL else torch.complex64)
        return fmt, _counts(self.B, n, x.shape[1], "n")

    def psd(self, x, n=None, win: int = 1024, step: int = 512, fs: float = PSD_FS, fmt=None, gain: float = 1.0):
        """radae_plots.m's pwelch(rx, [], [], 1024, Fs) over every stream (rade_batch_psd).  x: cuda complex64 [B, S] or int16 [B, S] (scaled by `gain` as wire_in does,
        imaginary part +0); n: samples of each stream (a scalar or B values, default S), each at least win.  A symmetric Hamming window of `win` samples (16..1024) every
        `step` (1..win), zero-padded to 1024 points.  Returns (P, n_seg): P cuda float32 [B, 1024], the two-sided density of bins 0 .. fs 1023 / 1024 in natural order;
        n_seg int32 [B].  pwelch's own defaults are psd_octave_default(n) (recalled, not verified).  The call synchronises the current stream."""
        import torch
        B = self.B
        fmt, n = self._psd_input(x, n, fmt)
        psd_plan(win, step)
        P = torch.zeros((B, PSD_NFFT), dtype=torch.float32, device=x.device)
        ns = np.zeros(B, np.int32)
        if self.lib.rade_batch_psd(self.h, x.data_ptr(), _row_stride(x, x.shape[1]), n.ctypes.data, fmt, gain, int(win), int(step), float(fs), P.data_ptr(), PSD_NFFT,
                                   ns.ctypes.data, _stream_ptr()):
            raise RuntimeError(f"rade_batch_psd failed (every stream needs at least win = {win} samples; a gain and fs that are finite and positive)")
        return P, ns

    def sigstat(self, x, n=None, head: int = PSD_HEAD, fmt=None, gain: float = 1.0) -> SigStat:
        """radae_plots.m:62-69 over every stream (rade_batch_sigstat): sum and maximum of |x|^2 over each stream and over its first min(n, head) samples, and from them the
        script's Pav, PAPRdB and PilotPAPRdB (nan for silence, as its 0 / 0).  x, n, fmt, gain as psd takes them; n = 0 is allowed.  The call synchronises the stream."""
        B = self.B
        fmt, n = self._psd_input(x, n, fmt)
        res = (SigstatResult * B)()
        if self.lib.rade_batch_sigstat(self.h, x.data_ptr(), _row_stride(x, x.shape[1]), n.ctypes.data, fmt, gain, int(head), C.byref(res), _stream_ptr()):
            raise RuntimeError("rade_batch_sigstat failed (head >= 0; a gain that is finite and positive)")
        r = np.array([(v.sum2, v.peak2, v.head_sum2, v.head_peak2) for v in res], np.float64).reshape(B, 4)
        cnt = np.array([v.n for v in res], np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            pav, hav = r[:, 0] / cnt, r[:, 2] / np.minimum(cnt, int(head))
            papr, ppapr = 10 * np.log10(r[:, 1] / pav), 10 * np.log10(r[:, 3] / hav)
        return SigStat(cnt, r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy(), pav, papr, ppapr)

    # ---- whole-file pilot acquisition ---------------------------------------------------------------
    def acq_detect(self, x, n=None, pacq_error1: float = 1e-5, dt_rows=None):
        """detect_pilots over every hop of every stream (rade_batch_acq_detect, rx.py:146-150).  x: cuda complex64 [B, S]; n: samples of each stream (a scalar or B values,
        default S).  Returns (hops, n_hops): hops a numpy record array [B, H] of abi.AcqHop (Dtmax12, Dthresh, tmax, f_ind, candidate, S1, S2), H = the most hops any
        stream has (at least 1), n_hops int32 [B].  dt_rows=(t0, n_rows): also the complex64 surface D[t0 .. t0 + n_rows) of every stream as a third value, cuda
        [B, n_rows, 40], zeros where a stream has no such row.  The call synchronises the current stream."""
        import torch
        B = self.B
        assert _is_rows(x, B, torch.complex64)
        S = x.shape[1]
        n = _counts(B, n, S, "n")
        H = max(max(acq_hops(v) for v in n), 1)
        hops = np.zeros((B, H), np.dtype(AcqHop))
        nh = np.zeros(B, np.int32)
        dt, t0, nr = None, 0, 0
        if dt_rows is not None:
            t0, nr = int(dt_rows[0]), int(dt_rows[1])
            dt = torch.zeros((B, max(nr, 1), 40), dtype=torch.complex64, device=x.device)
        if self.lib.rade_batch_acq_detect(self.h, x.data_ptr(), _row_stride(x, S), n.ctypes.data, float(pacq_error1), hops.ctypes.data, H, nh.ctypes.data,
                                          dt.data_ptr() if dt is not None else None, t0, nr, _stream_ptr()):
            raise RuntimeError("rade_batch_acq_detect failed (0 < pacq_error1 < 5; with dt_rows, t0 >= 0, n_rows >= 1 and t0 + n_rows within the row of x)")
        return (hops, nh) if dt is None else (hops, nh, dt)

    def acq_refine(self, x, events, n=None, want_dfine: bool = False):
        """acquisition.refine for a list of events (rade_batch_acq_refine).  x: cuda complex64 [B, S]; events: a sequence of (stream, t_abs = 960 hop + tmax, fmax).
        Returns a numpy record array [E] of abi.AcqRefined (t, f, Dmax); with want_dfine also float64 [E, 80], |Dt1| of the winning timing.  Synchronises the stream."""
        import torch
        B = self.B
        assert _is_rows(x, B, torch.complex64)
        S = x.shape[1]
        n = _counts(B, n, S, "n")
        E = len(events)
        ev = np.zeros(max(E, 1), np.dtype(AcqRefineIn))
        for i, (b, t, f) in enumerate(events):
            ev[i] = (int(b), int(t), float(f))
        out = np.zeros(max(E, 1), np.dtype(AcqRefined))
        df = np.zeros((max(E, 1), 80), np.float64) if want_dfine else None
        if self.lib.rade_batch_acq_refine(self.h, x.data_ptr(), _row_stride(x, S), n.ctypes.data, ev.ctypes.data, E, out.ctypes.data,
                                          df.ctypes.data if want_dfine else None, _stream_ptr()):
            raise RuntimeError("rade_batch_acq_refine failed (an event's stream inside the batch, |t_abs| <= 2^40, a finite fmax)")
        return (out[:E], df[:E]) if want_dfine else out[:E]

    acq_hops = staticmethod(lambda n: acq_hops(n))
    acq_track = staticmethod(lambda hops, acq_test=False: acq_track(hops, acq_test))
    acq_stats = staticmethod(lambda events, refined, n_hops, ntap=101, fmax_target=0.0, acq_time_target=1.0: acq_stats(events, refined, n_hops, ntap, fmax_target,
                                                                                                                      acq_time_target))

    # ---- the stored-file receiver past the acquisition ------------------------------------------------------------------------
    def bpf_file(self, x, n=None, out=None):
        """complex_bpf(101, ..).bpf(x) of whole files (rade_batch_bpf_file, rx.py:107-114).  x: cuda complex64 [B, S]; n: samples of each stream (a scalar or B values,
        default S).  Returns y complex64 [B, S]: a stream's first n samples filtered, zeros behind them (left alone in a caller's `out`).  Synchronises the stream."""
        import torch
        B = self.B
        assert _is_rows(x, B, torch.complex64)
        S = x.shape[1]
        n = _counts(B, n, S, "n")
        out = _out_rows(out, B, n, S, x.device)
        if self.lib.rade_batch_bpf_file(self.h, x.data_ptr(), _row_stride(x, S), n.ctypes.data, out.data_ptr(), _row_stride(out, out.shape[1]), _stream_ptr()):
            raise RuntimeError("rade_batch_bpf_file failed (8-byte aligned rows, counts within both rows, an output that does not overlap the input)")
        return out

    def rx_file(self, x, plans, max_mf=None, time_offset: int = -16, eq: str = "ls", coarse_mag: bool = True, feat_width: int = 84):
        """The fixed-timing demodulator and decoder of rx.py:223-253 (rade_batch_rx_file).  x: cuda complex64 [B, S]; plans: B (start, n_mf, freq) -- or objects with those
        attributes, as file_plan returns; a stream with n_mf 0 gives zeros.  max_mf: rows of the result in modem frames (default: the largest n_mf, at least 1).
        feat_width: the blob's decoder output per step (84 model19_check3), 0 = no decoder.  Returns (features [B, 3 max_mf, feat_width] or None, z_hat [B, 3 max_mf, 80]);
        rows past a stream's 3 n_mf are zeros in z_hat.  Synchronises the stream."""
        import torch
        B = self.B
        assert _is_rows(x, B, torch.complex64) and len(plans) == B
        rec = np.zeros(B, np.dtype(FileRxIn))
        for b, p in enumerate(plans):
            rec[b] = (int(p.start), int(p.n_mf), float(p.freq)) if hasattr(p, "n_mf") else (int(p[0]), int(p[1]), float(p[2]))
        max_mf = max(int(rec["n_mf"].max()), 1) if max_mf is None else int(max_mf)
        z_hat = torch.empty((B, 3 * max_mf, 80), dtype=torch.float32, device=x.device)
        feats = torch.empty((B, 3 * max_mf, feat_width), dtype=torch.float32, device=x.device) if feat_width else None
        r = self.lib.rade_batch_rx_file(self.h, x.data_ptr(), _row_stride(x, x.shape[1]), rec.ctypes.data, max_mf, int(time_offset), EQ_MODES[eq], int(coarse_mag),
                                        z_hat.data_ptr(), feats.data_ptr() if feats is not None else None, _stream_ptr())
        if r != max_mf:
            raise RuntimeError("rade_batch_rx_file failed (n_mf 0 or 2 .. max_mf, start >= 0 and start + 960 n_mf inside the row, time_offset in [-32, 0], "
                               "3 max_mf <= 3 max_tx_mf with decode)")
        return feats, z_hat

    def ber_align(self, z_ref, z_hat, n_ref=None, n_hat=None):
        """The BER alignment of rx.py:260-276 (rade_batch_ber_align).  z_ref, z_hat: cuda float32 [B, N] / [B, M] (or [B, rows, 80]); n_ref, n_hat: floats of each stream
        (scalars or B values, default the whole row).  Returns n_errors np.int64 [B, 20]: the sign errors at shifts of 0..19 modem frames (240 floats) of the reference,
        -1 where the shift leaves no reference.  ber_best(n_errors[b], n_ref[b]) gives the script's best shift and BER.  Synchronises the stream."""
        import torch
        B = self.B
        z_ref, z_hat = (t.reshape(B, -1) for t in (z_ref, z_hat))
        assert _is_rows(z_ref, B, torch.float32) and _is_rows(z_hat, B, torch.float32)
        n_ref = _per_stream(B, z_ref.shape[1] if n_ref is None else n_ref, np.int64, "n_ref"); n_hat = _per_stream(B, z_hat.shape[1] if n_hat is None else n_hat, np.int64, "n_hat")
        err = np.zeros((B, 20), np.int64)      # C long
        if self.lib.rade_batch_ber_align(self.h, z_ref.data_ptr(), _row_stride(z_ref, z_ref.shape[1]), n_ref.ctypes.data, z_hat.data_ptr(), _row_stride(z_hat, z_hat.shape[1]),
                                         n_hat.ctypes.data, err.ctypes.data, _stream_ptr()):
            raise RuntimeError("rade_batch_ber_align failed (lengths within the rows)")
        return err

    file_plan = staticmethod(lambda n, hop, t, f, freq_offset=None: file_plan(n, hop, t, f, freq_offset))
    ber_best = staticmethod(lambda n_errors, n_ref: ber_best(n_errors, n_ref))

    # ---- analog FM ----------------------------------------------------------------------------------------------------------
    def fm_mod(self, m, Fs: float, fc: float, fd: float, n=None, real: bool = False, sigma: float = 0.0, seed: int = 0, noise=None, phase0=0, n0=0, out=None,
               want_phase: bool = True):
        """The analog FM modulator (rade_batch_fm_mod, fm.m:74-94).  m: cuda float32 [B, N], or complex64 [B, N] whose real part is used.  Returns
        (tx complex64 [B, N], phase_end uint32 [B] or None): tx[i] = cis(phase0 + sum_{k <= i} inc[k]), a 32-bit NCO.  n: samples of each row (default N); phase0: the
        phase in front of the first sample, n0: its absolute index (what the generated noise is counted by): scalars or B per-stream values.  sigma > 0 adds noise:
        `noise` (cuda complex64 [B, N], unit) or generated from `seed`; real: (Re tx + sigma g, +0) instead of tx + sigma / sqrt 2 (g0 + j g1).  Samples past a
        stream's n are zeros (left alone in a caller's `out`).  want_phase=False skips the read-back and the wait behind the kernels (the call still waits once, ahead of its launches, for the copy of its per-stream records and so for the work queued in front of it)."""
        import torch
        B = self.B
        assert m.dtype in (torch.float32, torch.complex64) and _is_rows(m, B, m.dtype)
        N = m.shape[1]
        n = _counts(B, n, N, "n")
        ph0 = _per_stream(B, phase0, np.uint32, "phase0"); n0 = _per_stream(B, n0, np.int64, "n0")
        ph_end = np.zeros(B, np.uint32) if want_phase else None
        out = _out_rows(out, B, n, N, m.device)
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.complex64 and noise.dim() == 2 and noise.shape[0] == B and noise.shape[1] >= n.max()
            noise = noise[:, :int(n.max())].contiguous()              # dense [B][max n]
        p = FmModParams(float(Fs), float(fc), float(fd), FM_F32 if m.dtype == torch.float32 else FM_C64, FM_OUT_REAL if real else FM_OUT_COMPLEX, float(sigma), int(seed),
                        noise.data_ptr() if noise is not None else None, ph0.ctypes.data, ph_end.ctypes.data if want_phase else None, n0.ctypes.data)
        if self.lib.rade_batch_fm_mod(self.h, m.data_ptr(), _row_stride(m, N), n.ctypes.data, out.data_ptr(), _row_stride(out, out.shape[1]), C.byref(p), _stream_ptr()):
            raise RuntimeError("rade_batch_fm_mod failed (Fs > 0, |fc| <= Fs / 2, 0 < fd <= Fs / 2, sigma >= 0 with a seed or a noise tensor, n0 >= 0)")
        return out, ph_end

    def fm_demod(self, x, Fs: float, fc: float, fd: float, b1, b2, n_in=None, n_out=None, in_base=0, n0=None, complex_out: bool = False, ph_dont_limit: bool = False,
                 want_bb: bool = False):
        """The analog FM demodulator (rade_batch_fm_demod, fm.m:97-126): mix down by fc, input FIR b1, discriminator (clamped to the deviation unless ph_dont_limit),
        output FIR b2.  x: cuda complex64 [B, N]; b1, b2: host arrays (rounded to float32), 1..512 taps each.  Returns (y float32 [B, max n_out] -- complex64 with +0
        imaginary parts when complex_out --, bb complex64 [B, max n_out] or None, n_out int32 [B]).  x[b, g] is the sample of absolute index in_base + g; output i is the
        sample of absolute index n0 + i (default n0 = in_base, n_out = n_in: one output per input).  Samples past a stream's n_out are zeros."""
        import torch
        B = self.B
        assert _is_rows(x, B, torch.complex64)
        N = x.shape[1]
        b1 = np.ascontiguousarray(b1, dtype=np.float32); b2 = np.ascontiguousarray(b2, dtype=np.float32)
        n_in = _counts(B, n_in, N, "n_in")
        in_base = _per_stream(B, in_base, np.int64, "in_base")
        n0 = in_base.copy() if n0 is None else _per_stream(B, n0, np.int64, "n0")
        if n_out is None:
            n_out = np.maximum(in_base + n_in - n0, 0).astype(np.int32)
        else:
            n_out = _per_stream(B, n_out, np.int32, "n_out")
        W = max(int(n_out.max()), 1)
        y = torch.zeros((B, W), dtype=torch.complex64 if complex_out else torch.float32, device=x.device)
        bb = torch.zeros((B, W), dtype=torch.complex64, device=x.device) if want_bb else None
        p = FmDemodParams(float(Fs), float(fc), float(fd), FM_C64 if complex_out else FM_F32, int(bool(ph_dont_limit)), b1.ctypes.data, b1.size, b2.ctypes.data, b2.size,
                          in_base.ctypes.data, n0.ctypes.data, bb.data_ptr() if want_bb else None, W)
        if self.lib.rade_batch_fm_demod(self.h, x.data_ptr(), _row_stride(x, N), n_in.ctypes.data, y.data_ptr(), W, n_out.ctypes.data, C.byref(p), _stream_ptr()):
            raise RuntimeError("rade_batch_fm_demod failed (Fs > 0, |fc| <= Fs / 2, 0 < fd <= Fs / 2, 1..512 finite taps per filter)")
        return y, bb, n_out

    # ---- the channel and the Doppler generator in pieces -----------------------------------------------------------------
    def multipath_piece(self, taps, low_ratio: int, n_out, n0=0, seed: int = 1, hf_gain: float = 0.0, out=None):
        """Doppler samples of absolute indices [n0, n0 + n_out) of every stream (rade_batch_multipath_piece): returns (G complex64 [B, max n_out, 2], n_out int32 [B]).
        taps: the host FIR taps (rounded to float32, 1..256), low_ratio: Fs over the low rate (channel_tools.doppler_plan gives both); n_out, n0: scalars or B
        per-stream values; hf_gain 0 = multipath_gain(taps), the expected-value normalisation.  Every sample is a pure function of (seed, stream, absolute index): pieces
        equal the whole, bit for bit.  Pairs past a stream's n_out are zeros (left alone in a caller's `out`)."""
        import torch
        B = self.B
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        n_out = _per_stream(B, n_out, np.int32, "n_out"); n0 = _per_stream(B, n0, np.int64, "n0")
        if out is None:
            out = torch.zeros((B, max(int(n_out.max()), 1), 2), dtype=torch.complex64, device=self.device)
        assert out.is_cuda and out.dtype == torch.complex64 and out.dim() == 3 and out.shape[0] == B and out.shape[2] == 2 and out.stride(2) == 1 \
            and (out.stride(1) == 2 or out.shape[1] <= 1) and out.stride(0) % 2 == 0
        if self.lib.rade_batch_multipath_piece(self.h, taps.ctypes.data, taps.size, int(low_ratio), float(hf_gain), int(seed), n0.ctypes.data, n_out.ctypes.data,
                                               out.data_ptr(), _row_stride(out, 2 * out.shape[1]) // 2, _stream_ptr()):
            raise RuntimeError("rade_batch_multipath_piece failed (1..256 finite taps, low_ratio >= 1, hf_gain >= 0, n0 >= 0, n_out <= the row of out)")
        return out, n_out

    def channel_piece(self, tx, sigma=0.0, freq_offset=0.0, df_dt=0.0, gain=1.0, n0=0, in_base=None, n_in=None, n_out=None, G=None, g_base=None, n_g=None, noise=None,
                      seed: int = 0, real_noise: bool = False, sine_amp: float = 0.0, sine_freq: float = 0.0, rx_gain: float = 1.0, out=None):
        """The rate-Fs channel on a piece of every stream (rade_batch_channel_piece): tx cuda complex64 [B, N], whose sample g has the absolute index in_base + g (default
        in_base = n0) -> (rx complex64 [B, max n_out], n_out int32 [B]), output i the received sample of absolute index n0 + i (default n_out = in_base + n_in - n0).
        G: cuda complex64 [B, Ng, 2] Doppler pairs whose pair g has the absolute index g_base + g (default max(n0 - 16, 0)), n_g pairs per row (default Ng): the two-path
        model tx[n] G1[n] + tx[n - 16] G2[n - 16]; None: none.  gain multiplies the two-path sample (no power is measured).  noise: cuda complex64 [B, >= max n_out] unit
        noise, or generated from `seed` (complex, or real-valued with real_noise: the lead and tail of inference.py).  sigma, freq_offset, df_dt, gain, n0, in_base,
        g_base, n_in, n_out, n_g: scalars or B per-stream values.  Pieces equal the whole, bit for bit."""
        import torch
        from .abi import CHANP_NOISE_COMPLEX, CHANP_NOISE_REAL, ChannelPieceParams
        B = self.B
        assert _is_rows(tx, B, torch.complex64)
        N = tx.shape[1]
        n_in = _counts(B, n_in, N, "n_in")
        n0 = _per_stream(B, n0, np.int64, "n0")
        in_base = n0.copy() if in_base is None else _per_stream(B, in_base, np.int64, "in_base")
        n_out = np.maximum(in_base + n_in - n0, 0).astype(np.int32) if n_out is None else _per_stream(B, n_out, np.int32, "n_out")
        out = _out_rows(out, B, n_out, n_out.max(), tx.device)
        vals = [_per_stream(B, v, np.float32, w) for v, w in ((sigma, "sigma"), (freq_offset, "freq_offset"), (df_dt, "df_dt"), (gain, "gain"))]
        p = ChannelPieceParams()
        p.sigma_host, p.freq_offset_host, p.df_dt_host, p.gain_host = (v.ctypes.data for v in vals)
        p.n0_host, p.in_base_host = n0.ctypes.data, in_base.ctypes.data
        if G is not None:
            assert G.is_cuda and G.dtype == torch.complex64 and G.dim() == 3 and G.shape[0] == B and G.shape[2] == 2 and G.stride(2) == 1 \
                and (G.stride(1) == 2 or G.shape[1] <= 1) and G.stride(0) % 2 == 0
            g_base = np.maximum(n0 - 16, 0) if g_base is None else _per_stream(B, g_base, np.int64, "g_base")
            n_g = _counts(B, n_g, G.shape[1], "n_g")
            p.G_dev, p.g_stride, p.n_g_host, p.g_base_host = G.data_ptr(), _row_stride(G, 2 * G.shape[1]) // 2, n_g.ctypes.data, g_base.ctypes.data
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.complex64 and noise.dim() == 2 and noise.shape[0] == B and noise.shape[1] >= n_out.max()
            noise = noise[:, :int(n_out.max())].contiguous()          # dense [B][max n_out]
            p.noise_dev = noise.data_ptr()
        p.seed, p.noise_mode = int(seed), CHANP_NOISE_REAL if real_noise else CHANP_NOISE_COMPLEX
        p.sine_amp, p.sine_freq, p.rx_gain = float(sine_amp), float(sine_freq), float(rx_gain)
        if self.lib.rade_batch_channel_piece(self.h, tx.data_ptr(), _row_stride(tx, N), n_in.ctypes.data, out.data_ptr(), _row_stride(out, out.shape[1]), n_out.ctypes.data,
                                             C.byref(p), _stream_ptr()):
            raise RuntimeError("rade_batch_channel_piece failed (finite values, sigma >= 0, |freq_offset| <= 2000, n0, in_base, g_base >= 0, a G row that covers "
                               "[max(n0 - 16, 0), n0 + n_out), n_out <= the row of out)")
        return out, n_out

    # ---- the sound-card wire ------------------------------------------------------------------
    def wire_in(self, i16, n=None, iq: bool = False, gain: float = 1.0):
        """int16 samples to complex64 on the device (rade_batch_wire_in; `int16tof32.py --zeropad` when real).  i16: cuda int16 [B, N], one real channel, or with iq
        [B, N, 2] (or [B, 2 N]) ..IQIQ..; n: samples of each stream (a scalar or B values; default N).  Returns complex64 [B, max(n)] = gain * sample, Q = +0 for a real
        channel; samples past a stream's n are zeros.  gain = 1 gives the reference script's bytes."""
        import torch
        assert _is_i16_rows(i16, self.B) and (iq or i16.dim() == 2)
        row = i16.shape[1] if i16.dim() == 3 or not iq else i16.shape[1] // 2
        n = _counts(self.B, n, row, "n")
        out = torch.zeros((self.B, max(int(n.max()), 1)), dtype=torch.complex64, device=i16.device)
        if self.lib.rade_batch_wire_in(self.h, i16.data_ptr(), _row_stride(i16, row << int(iq)), n.ctypes.data, WIRE_IQ if iq else WIRE_REAL, gain, out.data_ptr(), out.shape[1], _stream_ptr()):
            raise RuntimeError("rade_batch_wire_in failed (a finite gain, rows of at least n samples)")
        return out

    def wire_out(self, x, n=None, real: bool = True, scale: float = 32767.0, meters: bool = False):
        """complex64 samples to int16 on the device (rade_batch_wire_out; `f32toint16.py [--real] --scale S`): x cuda complex64 [B, N] -> int16 [B, N] of the I component
        (real) or [B, N, 2] of I and Q, int16(x * scale) truncated toward zero, saturated to -32768 / 32767 where that does not fit, 0 for NaN.  n: samples of each stream
        (default N); the rest of a row is zeros.  meters: also returns WireMeters (the call then synchronises)."""
        import torch
        assert _is_rows(x, self.B, torch.complex64)
        B, N = self.B, x.shape[1]
        n = _counts(B, n, N, "n")
        out = torch.zeros((B, N) if real else (B, N, 2), dtype=torch.int16, device=x.device)
        m = np.zeros((B, 4), np.float64) if meters else None
        if self.lib.rade_batch_wire_out(self.h, x.data_ptr(), _row_stride(x, N), n.ctypes.data, WIRE_REAL if real else WIRE_IQ, scale, out.data_ptr(), N if real else 2 * N,
                                        m.ctypes.data if meters else None, _stream_ptr()):
            raise RuntimeError("rade_batch_wire_out failed (a finite scale, rows of at least n samples)")
        if not meters:
            return out
        comps = np.maximum((n.astype(np.float64) * (1 if real else 2)) - m[:, 3], 1.0)
        return out, WireMeters(m[:, 0].copy(), np.sqrt(m[:, 1] / comps), m[:, 2].astype(np.int64), m[:, 3].astype(np.int64))



class _TailCarry:
    """What a stateless stage needs to be applied to streams that arrive in pieces (every stream gets pieces of the same length): per stream the last `hist` input samples
    stay on the device, in the format they arrive in.  self.tail = input samples [n_fed - hist, n_fed), zeros ahead of the stream (made from the first piece unless the
    stage made it); self.n_fed = input samples taken so far.  A piece is joined to the tail and handed to the stage's _emit(buf, in_end) with in_end = n_fed - lag, the
    "complete up to" rule: an output is emitted once the input sample `lag` past its position has arrived."""

    def _carry(self, hist: int, lag: int, tail=None):
        self.hist, self.lag, self.tail, self.n_fed = hist, lag, tail, 0

    def _feed(self, x, **kw):
        import torch
        if self.tail is None:
            self.tail = torch.zeros((x.shape[0], self.hist) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
        assert x.is_cuda and x.dtype == self.tail.dtype and x.shape[0] == self.eng.B and x.shape[2:] == self.tail.shape[2:]
        buf = torch.cat([self.tail, x], dim=1)
        out = self._emit(buf, self.n_fed + x.shape[1] - self.lag, **kw)
        self.tail = buf[:, -self.hist:].contiguous()
        self.n_fed += x.shape[1]
        return out


class ClockOffset(_TailCarry):
    """A sample-clock offset applied to streams that arrive in pieces (BatchEngine.resample is stateless: this keeps what the next piece needs).  Per stream the last 32
    input samples stay on the device; feed() emits the outputs whose whole 32-tap window has arrived, flush() the rest (their windows run into zeros, as at the end of a
    whole-stream call).  The concatenated outputs of a stream are bit-identical to one resample() call over the whole stream."""
    HIST = 32

    def __init__(self, engine: BatchStages, ppm, t0=0.0, mode: str = "sinc32"):
        import torch
        self.eng, self.mode = engine, mode
        self.ppm = _per_stream(engine.B, ppm, np.float64, "ppm"); self.t0 = _per_stream(engine.B, t0, np.float64, "t0")
        self._carry(self.HIST, 16, torch.zeros((engine.B, self.HIST), dtype=torch.complex64, device=engine.device))      # output n is complete once sample i(n) + 16 has arrived
        self.n_done = np.zeros(engine.B, np.int64)                    # outputs emitted so far

    def _emit(self, buf, in_end: int):
        """the outputs of positions below in_end that have not been emitted, from buf = input samples [n_fed - 32, ..)"""
        upto = np.array([resample_count(in_end, self.t0[b], self.ppm[b]) for b in range(self.eng.B)], np.int64)
        n_out = np.maximum(upto - self.n_done, 0).astype(np.int32)
        y, _ = self.eng.resample(buf, self.ppm, self.t0, self.mode, n_out=n_out, n0=self.n_done, in_base=self.n_fed - self.HIST)
        self.n_done += n_out
        return y, n_out

    def feed(self, x):
        """x cuda complex64 [B, n]: the next n input samples of every stream -> (y [B, max n_out], n_out int32 [B])"""
        return self._feed(x)

    def flush(self):
        """the outputs whose position lies inside the input fed so far and whose window runs past it"""
        return self._emit(self.tail, self.n_fed)


class RateConverter(_TailCarry):
    """A sample-rate conversion by L / M applied to streams that arrive in pieces (BatchEngine.rate_convert is stateless: this keeps what the next piece needs).  Per stream
    the last T input samples stay on the device, in the format they arrive in; feed() emits the outputs whose whole T-tap window has arrived, flush() the rest (their
    windows run into zeros, as at the end of a whole-stream call).  The concatenated outputs of a stream are bit-identical to one rate_convert() call over the whole stream."""

    def __init__(self, engine: BatchStages, L: int, M: int, gain: float = 1.0):
        self.eng, self.L, self.M, self.gain = engine, int(L), int(M), gain
        self.T = rate_taps(L, M).shape[1]
        self._carry(self.T, self.T // 2)                              # output n is complete once sample i(n) + T / 2 has arrived
        self.n_done = 0                                               # outputs emitted so far (the same for every stream: one ratio, equal pieces)

    def _emit(self, buf, in_end: int):
        """the outputs of positions below in_end that have not been emitted, from buf = input samples [n_fed - T, ..)"""
        n_out = max(rate_count(in_end, self.L, self.M) - self.n_done, 0)
        y, n = self.eng.rate_convert(buf, self.L, self.M, n_out=n_out, n0=self.n_done, in_base=self.n_fed - self.T, gain=self.gain)
        self.n_done += n_out
        return y, n

    def feed(self, x):
        """x cuda complex64 [B, n], int16 [B, n] or int16 [B, n, 2]: the next n input samples of every stream -> (y [B, max n_out], n_out int32 [B])"""
        return self._feed(x)

    def flush(self):
        """the outputs whose position lies inside the input fed so far and whose window runs past it"""
        if self.tail is None:
            return None, np.zeros(self.eng.B, np.int32)
        return self._emit(self.tail, self.n_fed)


class FmModulator:
    """The FM modulator applied to streams that arrive in pieces: carries each stream's NCO phase and absolute sample index (the noise counter) from piece to piece.
    The concatenated outputs are bit-identical to one fm_mod() call over the whole stream, noise included."""

    def __init__(self, engine: BatchStages, Fs: float, fc: float, fd: float, real: bool = False, sigma: float = 0.0, seed: int = 0):
        self.eng, self.Fs, self.fc, self.fd, self.real, self.sigma, self.seed = engine, Fs, fc, fd, real, sigma, seed
        self.phase = np.zeros(engine.B, np.uint32)
        self.n0 = 0                                                   # samples taken so far (every stream gets pieces of the same length)

    def feed(self, m, noise=None):
        """m cuda float32 or complex64 [B, n]: the next n modulating samples of every stream -> tx complex64 [B, n]"""
        tx, self.phase = self.eng.fm_mod(m, self.Fs, self.fc, self.fd, real=self.real, sigma=self.sigma, seed=self.seed, noise=noise, phase0=self.phase, n0=self.n0)
        self.n0 += m.shape[1]
        return tx


class FmDemodulator(_TailCarry):
    """The FM demodulator applied to streams that arrive in pieces (BatchEngine.fm_demod is stateless: this keeps what the next piece needs): the last N1 + N2 - 1 input
    samples of every stream stay on the device.  The concatenated outputs are bit-identical to one fm_demod() call over the whole stream."""

    def __init__(self, engine: BatchStages, Fs: float, fc: float, fd: float, b1, b2, complex_out: bool = False, ph_dont_limit: bool = False):
        self.eng, self.Fs, self.fc, self.fd, self.complex_out, self.ph_dont_limit = engine, Fs, fc, fd, complex_out, ph_dont_limit
        self.b1, self.b2 = np.ascontiguousarray(b1, dtype=np.float32), np.ascontiguousarray(b2, dtype=np.float32)
        self.H = self.b1.size + self.b2.size - 1                      # output n depends on inputs n - H .. n
        self._carry(self.H, 0)                                        # and so is complete with input n: one output per input

    def _emit(self, buf, in_end: int, want_bb: bool = False):
        y, bb, _ = self.eng.fm_demod(buf, self.Fs, self.fc, self.fd, self.b1, self.b2, in_base=self.n_fed - self.H, n0=self.n_fed, n_out=in_end - self.n_fed,
                                     complex_out=self.complex_out, ph_dont_limit=self.ph_dont_limit, want_bb=want_bb)
        return y, bb

    def feed(self, x, want_bb: bool = False):
        """x cuda complex64 [B, n]: the next n samples of every stream -> (y [B, n], bb [B, n] or None)"""
        return self._feed(x, want_bb=want_bb)


class ChannelStream(_TailCarry):
    """The rate-Fs channel applied to transmit streams that arrive in pieces, for as long as they last (BatchEngine.channel_piece and .multipath_piece are stateless: this
    keeps what the next piece needs): each stream's absolute sample index and its last 16 transmit samples, the delay of the second path.  channel: a preset of
    channel_tools.PRESETS (the two-path Watterson model, its Doppler samples generated again for every piece over [n0 - 16, n0 + n): nothing of them is carried) or
    None (AWGN).  EbNodB, freq_offset, df_dt, gain, n0 (the absolute index a stream starts at, for a stream that resumes): scalars or B per-stream values.  push()
    returns the received piece, contiguous complex64 [B, n]: what BatchEngine.rx takes.  The concatenated pieces of a stream are bit-identical to one push of the whole
    stream.  Silence, an end-of-over frame or lead-in noise are transmit samples the caller pushes."""
    DELAY = 16

    def __init__(self, engine: BatchStages, channel, EbNodB, freq_offset=0.0, df_dt=0.0, seed: int = 1, n0=0, gain=1.0, fs: int = 8000):
        from .channel_tools import PRESETS, doppler_plan
        B = engine.B
        lib = load_library()
        self.eng, self.seed = engine, int(seed)
        self.sigma = np.array([lib.rade_sigma_from_EbNodB(float(e)) for e in _per_stream(B, EbNodB, np.float64, "EbNodB")], np.float32)
        self.freq_offset, self.df_dt, self.gain = (_per_stream(B, v, np.float32, w) for v, w in ((freq_offset, "freq_offset"), (df_dt, "df_dt"), (gain, "gain")))
        self.start = _per_stream(B, n0, np.int64, "n0").copy()
        assert self.start.min() >= 0
        self.taps = None
        if channel is not None:
            taps, self.ratio, _ = doppler_plan(PRESETS[channel][0], fs, 2)
            self.taps = np.ascontiguousarray(taps, dtype=np.float32)
            self.hf_gain = multipath_gain(self.taps)
        self._carry(self.DELAY, 0)

    @property
    def n0(self) -> np.ndarray:
        """the absolute index of the next sample of every stream, int64 [B]"""
        return self.start + self.n_fed

    def _emit(self, buf, in_end: int):
        """buf = transmit samples [n_fed - 16, in_end): the piece [n_fed, in_end) through the channel"""
        hist = min(self.DELAY, self.n_fed)                            # samples of the tail that have been pushed: in front of them a stream reads zeros by itself
        n0, n = self.n0, in_end - self.n_fed
        kw = {}
        if self.taps is not None:
            g0 = np.maximum(n0 - self.DELAY, 0)
            G, n_g = self.eng.multipath_piece(self.taps, self.ratio, (n0 + n - g0).astype(np.int32), n0=g0, seed=self.seed, hf_gain=self.hf_gain)
            kw = dict(G=G, g_base=g0, n_g=n_g)
        rx, _ = self.eng.channel_piece(buf[:, self.DELAY - hist:], self.sigma, self.freq_offset, self.df_dt, self.gain, n0=n0, in_base=n0 - hist, n_out=n, seed=self.seed, **kw)
        return rx[:, :n]

    def push(self, tx):
        """tx cuda complex64 [B, n]: the next n transmit samples of every stream -> rx complex64 [B, n]"""
        return self._feed(tx)
