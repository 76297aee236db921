"""Python binding of the batched HIP engine (include/rade_batch.h) over ctypes.

PyTorch is used only as plumbing: device tensors own the HBM buffers whose raw pointers are handed
to the C ABI, and `torch.cuda.current_stream()` supplies the hipStream_t.  All compute happens in
radae_amd/libradehip.so (radae_amd/csrc); there is no CPU or PyTorch fallback -- if the shared
library or a GPU is missing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RADE_LIBRADEHIP") or os.path.join(_HERE, "libradehip.so")      # the override is a developer aid (A/B builds, tools/ab_build.sh)
DEFAULT_BLOB = os.path.join(os.path.dirname(_HERE), "weights", "model19_check3.bin")

NMF, NEOO, NIN_MAX, FEAT_MF, NEOO_BITS, ZMF = 960, 1152, 1120, 432, 180, 240
BOTTLENECK1, TX_BPF, BYPASS_DEC, TX_LINEAR = 0x100, 0x400, 0x800, 0x1000          # include/rade_batch.h flags
EQ_MODES = {"ls": 0, "mean6": 1, "all": 2, "none": 3}                              # rade_ideal_rx_params.eq


class BatchConfig(C.Structure):
    _fields_ = [("n_streams", C.c_int), ("max_tx_mf", C.c_int), ("device", C.c_int), ("flags", C.c_int), ("rx_trace_calls", C.c_int), ("disable_unsync", C.c_float)]


class ChannelParams(C.Structure):
    _fields_ = [("n_sig", C.c_int), ("n_pre", C.c_int), ("n_post", C.c_int), ("with_eoo", C.c_int), ("sigma", C.c_float), ("freq_offset", C.c_float),
                ("df_dt", C.c_float), ("G_dev", C.c_void_p), ("noise_dev", C.c_void_p), ("seed", C.c_ulonglong),
                ("sine_amp", C.c_float), ("sine_freq", C.c_float), ("rx_gain", C.c_float)]


class ChannelStreams(C.Structure):
    _fields_ = [("sigma", C.c_void_p), ("freq_offset", C.c_void_p), ("df_dt", C.c_void_p)]


class IdealRxParams(C.Structure):
    _fields_ = [("time_offset", C.c_int), ("eq", C.c_int), ("coarse_mag", C.c_int), ("freq_offset_host", C.c_void_p), ("df_dt_host", C.c_void_p),
                ("z_ref_dev", C.c_void_p), ("n_errors_host", C.c_void_p)]


class ResampleParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("ppm", C.c_double), ("ppm_host", C.c_void_p), ("t0_host", C.c_void_p), ("n0_host", C.c_void_p), ("in_base_host", C.c_void_p)]


class RateParams(C.Structure):
    _fields_ = [("L", C.c_int), ("M", C.c_int), ("n0_host", C.c_void_p), ("in_base_host", C.c_void_p)]


class FmModParams(C.Structure):
    _fields_ = [("Fs", C.c_double), ("fc", C.c_double), ("fd", C.c_double), ("in_format", C.c_int), ("out_mode", C.c_int), ("sigma", C.c_double),
                ("seed", C.c_ulonglong), ("noise_dev", C.c_void_p), ("phase0_host", C.c_void_p), ("phase_end_host", C.c_void_p), ("n0_host", C.c_void_p)]


class FmDemodParams(C.Structure):
    _fields_ = [("Fs", C.c_double), ("fc", C.c_double), ("fd", C.c_double), ("out_format", C.c_int), ("ph_dont_limit", C.c_int), ("b1", C.c_void_p), ("N1", C.c_int),
                ("b2", C.c_void_p), ("N2", C.c_int), ("in_base_host", C.c_void_p), ("n0_host", C.c_void_p), ("bb_out_dev", C.c_void_p), ("bb_stride", C.c_long)]


class CnoParams(C.Structure):
    _fields_ = [("window_time", C.c_double), ("flow", C.c_double), ("fhigh", C.c_double)]


class CnoPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("N", "J", "n_bins", "flow_bin", "fhigh_bin", "noise_st", "noise_en")]


class CnoResult(C.Structure):
    _fields_ = [("n_windows", C.c_int), ("n_positive", C.c_int), ("max_st", C.c_longlong), ("max_CNodB", C.c_double), ("max_SNRdB", C.c_double)]


class SpecgramParams(C.Structure):
    _fields_ = [("fmin", C.c_double), ("fmax", C.c_double), ("lo", C.c_double), ("hi", C.c_double), ("peak_in_host", C.c_void_p)]


class SpecgramPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_bins", "k0", "k1", "win", "step", "nfft")]


class RxStatus(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("consumed", "n_calls", "n_valid", "has_eoo", "nin", "sync", "snr_dB", "state")]


class RxTrace(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("state_before", "state_after", "nin_before", "nin_after", "ret", "tmax", "f_ind_max", "valid_count",
                                        "uw_errors", "synced_count", "snr_int", "pad")] + \
               [(n, C.c_double) for n in ("fmax", "Dthresh", "Dtmax12", "Dtmax12_eoo")] + [("snrdB_3k_est", C.c_float), ("pad2", C.c_float)]


_lib = None


def load_library() -> C.CDLL:
    """dlopen radae_amd/libradehip.so and declare the C ABI.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"or `make -C radae_amd/csrc` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.rade_batch_open.restype = vp; L.rade_batch_open.argtypes = [C.c_char_p, C.POINTER(BatchConfig)]
    L.rade_batch_open_mem.restype = vp; L.rade_batch_open_mem.argtypes = [vp, C.c_size_t, C.POINTER(BatchConfig)]
    L.rade_batch_close.argtypes = [vp]
    L.rade_batch_n_streams.argtypes = [vp]
    L.rade_batch_tx.argtypes = [vp, vp, C.c_int, vp, C.c_long, vp, vp]
    L.rade_batch_tx_latents.argtypes = [vp, vp, C.c_int, vp, C.c_long, vp]
    L.rade_batch_tx_channel.argtypes = [vp, vp, C.c_int, vp, C.c_long, vp, C.c_long, vp, vp]
    L.rade_batch_tx_set_eoo_bits.argtypes = [vp, vp]
    L.rade_batch_tx_eoo.argtypes = [vp, vp, C.c_long, vp]
    L.rade_batch_tx_reset.argtypes = [vp]
    L.rade_batch_channel.argtypes = [vp, vp, C.c_long, vp, C.c_long, C.POINTER(ChannelParams), vp]
    L.rade_batch_multipath_gen.argtypes = [vp, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, vp, C.c_ulonglong, vp, vp]
    L.rade_batch_multipath_h.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp]
    L.rade_sigma_from_EbNodB.restype = C.c_float; L.rade_sigma_from_EbNodB.argtypes = [C.c_float]
    if hasattr(L, "rade_batch_rx_ideal"):         # (absent from older A/B builds loaded through $RADE_LIBRADEHIP)
        L.rade_sigma_from_EbNodB_bn1.restype = C.c_float; L.rade_sigma_from_EbNodB_bn1.argtypes = [C.c_float]
        L.rade_batch_rx_ideal.argtypes = [vp, vp, C.c_long, C.c_int, C.POINTER(IdealRxParams), vp, vp, vp]
    L.rade_batch_rx.argtypes = [vp, vp, C.c_long, C.POINTER(C.c_int), C.c_int, vp, C.c_long, vp, C.POINTER(RxStatus), vp]
    L.rade_batch_rx_reset.argtypes = [vp]
    L.rade_batch_encode.argtypes = [vp, vp, C.c_int, vp, vp]
    L.rade_batch_decode.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
    L.rade_batch_channel_symbol.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_ulonglong, vp]
    L.rade_batch_reset.argtypes = [vp, vp]
    L.rade_batch_profile.argtypes = [vp, C.c_int]
    L.rade_batch_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long)]
    L.rade_batch_rx_set_lcg.argtypes = [vp, C.POINTER(C.c_uint)]
    L.rade_batch_rx_get_trace.argtypes = [vp, C.c_int, C.POINTER(RxTrace), vp, C.c_int]
    L.rade_batch_rx_stream_cycles.argtypes = [vp, vp]
    if hasattr(L, "rade_sync_policy"):
        L.rade_host_cpu_quota.restype = C.c_double; L.rade_host_cpu_quota.argtypes = []
        L.rade_sync_policy.argtypes = [C.c_int, C.c_double]
        L.rade_batch_sync_counts.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]; L.rade_batch_sync_counts.restype = None
    if hasattr(L, "rade_batch_rx_filtered"):      # (absent from older A/B builds loaded through $RADE_LIBRADEHIP)
        L.rade_batch_rx_filtered.argtypes = [vp, C.c_int, vp, C.c_int]
    if hasattr(L, "rade_batch_loss"):             # (absent from older A/B builds loaded through $RADE_LIBRADEHIP)
        L.rade_batch_channel_streams.argtypes = [vp, vp, C.c_long, vp, C.c_long, C.POINTER(ChannelParams), C.POINTER(ChannelStreams), vp]
        L.rade_batch_tx_channel_streams.argtypes = [vp, vp, C.c_int, vp, C.c_long, vp, C.c_long, C.POINTER(ChannelParams), C.POINTER(ChannelStreams), vp]
        L.rade_batch_loss.argtypes = [vp, vp, C.c_long, C.c_int, vp, vp, C.c_long, C.c_int, vp, vp, vp, vp, C.c_long, vp]
    if hasattr(L, "rade_batch_channel_rs_pa"):    # (absent from older A/B builds loaded through $RADE_LIBRADEHIP)
        L.rade_sigma_from_EbNodB_rs3.restype = C.c_float; L.rade_sigma_from_EbNodB_rs3.argtypes = [C.c_float]
        L.rade_batch_channel_rs_pa.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_float, vp, C.c_float, C.c_ulonglong, vp, vp]
    if hasattr(L, "rade_batch_resample"):         # (absent from older A/B builds loaded through $RADE_LIBRADEHIP)
        L.rade_batch_resample.argtypes = [vp, vp, C.c_long, vp, vp, C.c_long, vp, C.POINTER(ResampleParams), vp]
        L.rade_resample_count.restype = C.c_longlong; L.rade_resample_count.argtypes = [C.c_longlong, C.c_double, C.c_double]
        L.rade_resample_taps.restype = None; L.rade_resample_taps.argtypes = [vp]
    if hasattr(L, "rade_batch_wire_in"):
        L.rade_batch_wire_in.argtypes = [vp, vp, C.c_long, vp, C.c_int, C.c_float, vp, C.c_long, vp]
        L.rade_batch_wire_out.argtypes = [vp, vp, C.c_long, vp, C.c_int, C.c_float, vp, C.c_long, vp, vp]
    if hasattr(L, "rade_batch_rate_convert"):     # (absent from older A/B builds loaded through $RADE_LIBRADEHIP)
        L.rade_batch_rate_convert.argtypes = [vp, vp, C.c_long, vp, C.c_int, C.c_float, vp, C.c_long, vp, C.POINTER(RateParams), vp]
        L.rade_rate_count.restype = C.c_longlong; L.rade_rate_count.argtypes = [C.c_longlong, C.c_int, C.c_int]
        L.rade_rate_taps.argtypes = [C.c_int, C.c_int, vp]
    if hasattr(L, "rade_batch_fm_mod"):
        L.rade_batch_fm_mod.argtypes = [vp, vp, C.c_long, vp, vp, C.c_long, C.POINTER(FmModParams), vp]
        L.rade_batch_fm_demod.argtypes = [vp, vp, C.c_long, vp, vp, C.c_long, vp, C.POINTER(FmDemodParams), vp]
        L.rade_fm_sigma.restype = C.c_double; L.rade_fm_sigma.argtypes = [C.c_double] * 4
        L.rade_fm_deemph_len.argtypes = [C.c_double, C.c_double]
        L.rade_fm_taps.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, vp, vp]
    if hasattr(L, "rade_batch_cno_est"):
        L.rade_batch_cno_est.argtypes = [vp, vp, C.c_long, vp, C.POINTER(CnoParams), vp, C.c_int, vp, vp]
        L.rade_cno_plan.argtypes = [C.POINTER(CnoParams), C.POINTER(CnoPlan)]
        L.rade_chirp.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double]
    if hasattr(L, "rade_batch_specgram"):         # (absent from older A/B builds loaded through $RADE_LIBRADEHIP)
        L.rade_batch_specgram.argtypes = [vp, vp, C.c_long, vp, C.c_int, C.c_float, C.POINTER(SpecgramParams), vp, C.c_long, vp, C.c_long, vp, vp, vp]
        L.rade_specgram_plan.argtypes = [C.POINTER(SpecgramParams), C.POINTER(SpecgramPlan)]
        L.rade_specgram_slices.restype = C.c_longlong; L.rade_specgram_slices.argtypes = [C.c_longlong]
        L.rade_specgram_window.restype = None; L.rade_specgram_window.argtypes = [vp]
        L.rade_specgram_levels.argtypes = [C.c_double, C.c_double, vp]
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    # include/rade_api.h
    "rade_initialize", "rade_finalize", "rade_open", "rade_close", "rade_version", "rade_n_tx_out", "rade_n_tx_eoo_out", "rade_nin_max",
    "rade_n_features_in_out", "rade_n_eoo_bits", "rade_tx", "rade_tx_set_eoo_bits", "rade_tx_eoo", "rade_nin", "rade_rx", "rade_sync",
    "rade_freq_offset", "rade_snrdB_3k_est",
    # include/rade_batch.h
    "rade_batch_open", "rade_batch_open_mem", "rade_batch_close", "rade_batch_n_streams", "rade_batch_tx", "rade_batch_tx_latents", "rade_batch_tx_set_eoo_bits",
    "rade_batch_tx_eoo", "rade_batch_tx_reset", "rade_batch_channel", "rade_batch_tx_channel", "rade_batch_multipath_gen", "rade_batch_multipath_h", "rade_sigma_from_EbNodB", "rade_batch_rx", "rade_batch_rx_reset",
    "rade_batch_rx_set_lcg", "rade_batch_rx_get_trace", "rade_batch_reset", "rade_batch_profile", "rade_batch_profile_get", "rade_batch_profile_ref", "rade_batch_profile_intervals",
    "rade_batch_encode", "rade_batch_decode", "rade_batch_channel_symbol",
    "rade_batch_rx_stream_cycles", "rade_batch_rx_filtered", "rade_host_cpu_quota", "rade_sync_policy", "rade_batch_sync_counts",
    "rade_multi_open", "rade_multi_close", "rade_multi_n_devices", "rade_multi_transport", "rade_multi_engine", "rade_multi_shard", "rade_multi_foreach",
    "rade_multi_allreduce_sum",
    "rade_batch_rx_ideal", "rade_sigma_from_EbNodB_bn1",
    "rade_batch_loss", "rade_batch_channel_streams", "rade_batch_tx_channel_streams",
    "rade_batch_channel_rs_pa", "rade_sigma_from_EbNodB_rs3",
    "rade_batch_resample", "rade_resample_count", "rade_resample_taps",
    "rade_batch_wire_in", "rade_batch_wire_out",
    "rade_batch_rate_convert", "rade_rate_count", "rade_rate_taps",
    "rade_batch_fm_mod", "rade_batch_fm_demod", "rade_fm_sigma", "rade_fm_deemph_len", "rade_fm_taps",
    "rade_batch_cno_est", "rade_cno_plan", "rade_chirp",
    "rade_batch_specgram", "rade_specgram_plan", "rade_specgram_slices", "rade_specgram_window", "rade_specgram_levels",
]
WIRE_REAL, WIRE_IQ = 0, 1                                                          # rade_batch_wire_in / _out mode


class WireMeters(NamedTuple):
    """Level of what wire_out wrote, one value per stream: the largest |x scale| (before saturation), the RMS of x scale over the written components (NaN components
    excluded), and how many components saturated / were NaN."""
    peak: np.ndarray
    rms: np.ndarray
    clipped: np.ndarray
    nan: np.ndarray

RESAMPLE_MODES = {"sinc32": 0, "linear": 1}                                        # rade_resample_params.mode
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


RATE_C64, RATE_S16_REAL, RATE_S16_IQ = 0, 1, 2                                     # rade_batch_rate_convert format


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


FM_F32, FM_C64 = 0, 1                                                              # rade_batch_fm_mod input / rade_batch_fm_demod output format
FM_OUT_COMPLEX, FM_OUT_REAL = 0, 1                                                 # rade_batch_fm_mod output mode
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


CNO_FS, CNO_HOP = 8000, 2000                                                       # est_CNo.py:23, :31 (Fs // 4)


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


SPEC_C64, SPEC_S16_REAL = 0, 1                                                     # rade_batch_specgram format
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


def _per_stream(B: int, v, dtype, what: str) -> np.ndarray:
    """a scalar (every stream) or B per-stream values -> a contiguous [B] array"""
    a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=dtype)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
        raise ValueError(f"{what}: a scalar or {B} per-stream values, got shape {a.shape}")
    return np.ascontiguousarray(np.broadcast_to(a, (B,)))


def _is_rows(t, B: int, dtype) -> bool:
    """2-D device rows [B, N] of `dtype` with unit inner stride (a row of at most one sample may carry any)"""
    return t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[0] == B and (t.stride(1) == 1 or t.shape[1] <= 1)


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


def sigma_from_EbNodB(EbNodB, bottleneck: int = 3, rate_Fs: bool = True):
    """AWGN standard deviation of the rate-Fs channel: bottleneck 3 (radae.py:567-573) or bottleneck 1 (:574-576, the waveform of TX_LINEAR); with rate_Fs=False
    of the rate-Rs channel of bottleneck 3 (radae.py:627-630, channel_rs_pa: 12.66 at 3 dB, for symbols of magnitude M / sqrt(Nc)).
    A scalar gives a float; an array of Eb/No points gives a float32 array of the same shape, each value what the scalar form gives (per-stream channels)."""
    L = load_library()
    if not rate_Fs:
        if bottleneck != 3:
            raise ValueError("rate-Rs noise is offered for bottleneck 3 (bottleneck 1: sigma = 10 ** (-EbNodB / 20), radae.py:632)")
        f = L.rade_sigma_from_EbNodB_rs3
    elif bottleneck == 1:
        f = L.rade_sigma_from_EbNodB_bn1
    elif bottleneck == 3:
        f = L.rade_sigma_from_EbNodB
    else:
        raise ValueError("rate-Fs noise is defined for bottleneck 1 or 3")
    if np.ndim(EbNodB) == 0:
        return float(f(EbNodB))
    e = np.asarray(EbNodB, dtype=np.float32)
    return np.array([f(float(x)) for x in e.ravel()], dtype=np.float32).reshape(e.shape)


def channel_stream_values(B: int, sigma, freq_offset, df_dt):
    """sigma / freq_offset / df_dt of a channel call, each a scalar (every stream) or a length-B sequence (one value per stream, rade_channel_streams).
    Returns the three scalars for rade_channel_params (0.0 where a sequence was given) and {name: float32[B]} of the sequences, or None when all are scalars."""
    scal, per = [], {}
    for name, v in (("sigma", sigma), ("freq_offset", freq_offset), ("df_dt", df_dt)):
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        if np.ndim(v) == 0:
            scal.append(float(v))
            continue
        a = np.ascontiguousarray(v, dtype=np.float32)
        if a.ndim != 1 or a.shape[0] != B:
            raise ValueError(f"{name}: a scalar or {B} per-stream values, got shape {a.shape}")
        scal.append(0.0)
        per[name] = a
    return tuple(scal), (per or None)


def _channel_streams(per):
    return ChannelStreams(*(per[k].ctypes.data if k in per else None for k in ("sigma", "freq_offset", "df_dt")))


def loss_lengths(B: int, n_in, n_hat, rows_in: int, rows_hat: int, clip_start: int = 0, clip_end: int = 0):
    """Per-stream row counts of a rade_batch_loss call: n_in / n_hat each None (every row of the buffer), a scalar or B values; n_hat may also be rx()'s
    status list (12 x n_valid).  clip_start / clip_end (loss.py's flags) drop decoded rows at either end: the returned n_hat counts the rows after
    clip_start (0 when none are left).  Counts beyond the buffers' rows are refused: the kernel would read past them."""
    def per_stream(v, rows, what):
        if v is None:
            v = rows
        elif isinstance(v, (list, tuple, C.Array)) and len(v) and hasattr(v[0], "n_valid"):
            v = [12 * s.n_valid for s in v]
        a = np.asarray(v, dtype=np.int64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != B):
            raise ValueError(f"{what}: a scalar or {B} per-stream values, got shape {a.shape}")
        a = np.broadcast_to(a, (B,))
        if a.max(initial=0) > rows:
            raise ValueError(f"{what}: {int(a.max())} rows asked for, the buffer holds {rows}")
        return a
    if clip_start < 0 or clip_end < 0:
        raise ValueError("clip_start / clip_end must be >= 0")
    ni = per_stream(n_in, rows_in, "n_in")
    nh = per_stream(n_hat, rows_hat, "n_hat")
    return ni.astype(np.int32), np.maximum(nh - clip_start - clip_end, 0).astype(np.int32)


def _stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class BatchEngine:
    """B independent RADE streams on one GPU (one engine per process/GPU)."""

    def __init__(self, n_streams: int, max_tx_mf: int = 1, device: int = 0, flags: int = 0, blob: Optional[str] = None,
                 blob_bytes: Optional[bytes] = None, rx_trace_calls: int = 0, disable_unsync: float = 0.0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("radae_amd.BatchEngine needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.lib = load_library()
        self.B = n_streams
        self.device = torch.device("cuda", device)
        self.trace_calls = rx_trace_calls
        self.rx_row_floats = ZMF if flags & BYPASS_DEC else FEAT_MF      # RADE_BATCH_BYPASS_DEC: 240 latents per valid modem frame instead of 432 feature floats
        cfg = BatchConfig(n_streams, max_tx_mf, device, flags, rx_trace_calls, disable_unsync)
        if blob_bytes is not None:
            buf = C.create_string_buffer(blob_bytes, len(blob_bytes))
            self.h = self.lib.rade_batch_open_mem(C.cast(buf, C.c_void_p), len(blob_bytes), C.byref(cfg))
        else:
            self.h = self.lib.rade_batch_open((blob or DEFAULT_BLOB).encode(), C.byref(cfg))
        if not self.h:
            raise RuntimeError("rade_batch_open failed (see stderr)")
        self.max_tx_mf = max_tx_mf

    def close(self):
        if getattr(self, "h", None):
            self.lib.rade_batch_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Stream-ordered reset of encoder and receiver state (a new batch of utterances)."""
        self.lib.rade_batch_reset(self.h, _stream_ptr())

    PROF_CLASSES = ("gemm", "gru_scan", "ofdm_mod", "channel", "rx_sync", "rx_bpf")

    def profile(self, enable: bool):
        self.lib.rade_batch_profile(self.h, int(enable))

    def profile_ref(self, event_handle: int):
        """absolute launch intervals (profile_intervals) are measured from this hipEvent_t (e.g. torch.cuda.Event(enable_timing=True).cuda_event after record())"""
        self.lib.rade_batch_profile_ref.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.rade_batch_profile_ref(self.h, C.c_void_p(event_handle))

    def profile_intervals(self, cls_name: str, max_n: int = 4096):
        self.lib.rade_batch_profile_intervals.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        t0 = np.zeros(max_n, np.float32); t1 = np.zeros(max_n, np.float32)
        n = self.lib.rade_batch_profile_intervals(self.h, self.PROF_CLASSES.index(cls_name), t0.ctypes.data_as(C.c_void_p), t1.ctypes.data_as(C.c_void_p), max_n)
        return t0[:n].astype(np.float64), t1[:n].astype(np.float64)

    def profile_get(self):
        out = {}
        for i, name in enumerate(self.PROF_CLASSES):
            ms, wk, n = C.c_double(), C.c_double(), C.c_long()
            self.lib.rade_batch_profile_get(self.h, i, C.byref(ms), C.byref(wk), C.byref(n))
            out[name] = {"ms": ms.value, "flops": wk.value, "launches": n.value}
        return out

    # ---- transmit ---------------------------------------------------------------------------
    def tx(self, features, want_z: bool = False):
        """features: cuda float32 [B, n_mf*12, 36] -> iq complex64 [B, n_mf*960] (+ z [B, n_mf*3, 80])."""
        import torch
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        B, nfr, w = features.shape
        assert B == self.B and w == 36 and nfr % 12 == 0
        n_mf = nfr // 12
        iq = torch.empty((B, n_mf * NMF), dtype=torch.complex64, device=features.device)
        z = torch.empty((B, n_mf * 3, 80), dtype=torch.float32, device=features.device) if want_z else None
        done = 0
        while done < n_mf:                       # chunk by the engine's capacity; state carries across chunks
            k = min(self.max_tx_mf, n_mf - done)
            f = features[:, done * 12:(done + k) * 12, :].contiguous()
            zc = torch.empty((B, k * 3, 80), dtype=torch.float32, device=features.device) if want_z else None
            r = self.lib.rade_batch_tx(self.h, f.data_ptr(), k, iq.data_ptr() + done * NMF * 8, n_mf * NMF, zc.data_ptr() if want_z else None, _stream_ptr())
            if r != k * NMF:
                raise RuntimeError("rade_batch_tx failed")
            if want_z:
                z[:, done * 3:(done + k) * 3] = zc
            done += k
        return (iq, z) if want_z else iq

    def tx_latents(self, z):
        """`radae_txe.py --bypass_enc` (radae_txe.py:124-126): z cuda float32 [B, n_mf*3, 80] from an external core encoder -> iq complex64 [B, n_mf*960]."""
        import torch
        assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.shape[0] == self.B and z.shape[2] == 80 and z.shape[1] % 3 == 0
        n_mf = z.shape[1] // 3
        iq = torch.empty((self.B, n_mf * NMF), dtype=torch.complex64, device=z.device)
        done = 0
        while done < n_mf:
            k = min(self.max_tx_mf, n_mf - done)
            zc = z[:, done * 3:(done + k) * 3, :].contiguous()
            if self.lib.rade_batch_tx_latents(self.h, zc.data_ptr(), k, iq.data_ptr() + done * NMF * 8, n_mf * NMF, _stream_ptr()) != k * NMF:
                raise RuntimeError("rade_batch_tx_latents failed")
            done += k
        return iq

    def tx_reset(self):
        self.lib.rade_batch_tx_reset(self.h)

    def set_eoo_bits(self, bits: Optional[np.ndarray]):
        if bits is None:
            r = self.lib.rade_batch_tx_set_eoo_bits(self.h, None)
        else:
            b = np.ascontiguousarray(bits, dtype=np.float32).reshape(self.B, NEOO_BITS)
            r = self.lib.rade_batch_tx_set_eoo_bits(self.h, b.ctypes.data_as(C.c_void_p))
        if r:
            raise RuntimeError("rade_batch_tx_set_eoo_bits failed")

    def tx_eoo(self):
        import torch
        out = torch.empty((self.B, NEOO), dtype=torch.complex64, device=self.device)
        if self.lib.rade_batch_tx_eoo(self.h, out.data_ptr(), NEOO, _stream_ptr()) != NEOO:
            raise RuntimeError("rade_batch_tx_eoo failed")
        return out

    # ---- core encoder / decoder alone, symbol-domain channels (configs 1, 2, 5) -----------------
    def encode(self, features):
        """features cuda float32 [B, n_steps, 4*feat_dim] -> z [B, n_steps, 80] (state carried; tx_reset() clears)."""
        import torch
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous() and features.shape[0] == self.B
        n = features.shape[1]
        z = torch.empty((self.B, n, 80), dtype=torch.float32, device=features.device)
        if self.lib.rade_batch_encode(self.h, features.data_ptr(), n, z.data_ptr(), _stream_ptr()) != n:
            raise RuntimeError("rade_batch_encode failed (n_steps > 3*max_tx_mf?)")
        return z

    def decode(self, z, feat_width: int, reset: bool = True):
        """z cuda float32 [B, n_steps, 80] -> features [B, n_steps, feat_width] (feat_width = 4*feat_dim of the blob)."""
        import torch
        assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and tuple(z.shape[::2]) == (self.B, 80)
        n = z.shape[1]
        out = torch.empty((self.B, n, feat_width), dtype=torch.float32, device=z.device)
        if self.lib.rade_batch_decode(self.h, z.data_ptr(), n, out.data_ptr(), int(reset), _stream_ptr()) != n:
            raise RuntimeError("rade_batch_decode failed")
        return out

    def channel_symbol(self, z, mode: str, p0: float, p1: float = 0.0, H=None, noise=None, seed: int = 0):
        """mode 'rs': z*H + sigma*noise (p0 = sigma, H per QPSK symbol [B, n*40]); mode 'bbfm': FM-demod SNR model
        (p0 = CNRdB, p1 = Gfm dB, H per real symbol [B, n*80]).  noise float32 [B, n*80] or None -> Philox(seed)."""
        import torch
        n = z.shape[1]
        out = torch.empty_like(z)
        r = self.lib.rade_batch_channel_symbol(self.h, z.data_ptr(), H.data_ptr() if H is not None else None, noise.data_ptr() if noise is not None else None,
                                               out.data_ptr(), n, 0 if mode == "rs" else 1, p0, p1, seed, _stream_ptr())
        if r != n:
            raise RuntimeError("rade_batch_channel_symbol failed")
        return out

    def channel_rs_pa(self, z, sigma, H=None, noise=None, phase_offset: float = 0.0, seed: int = 0, want_stats: bool = False):
        """The rate-Rs channel of the bottleneck-3 model (rade_batch_channel_rs_pa; radae.py:603-634): z cuda float32 [B, n_steps, 80] -> z_hat of the same shape.
        Every OFDM symbol (40 floats of z: 20 carriers) through IDFT, PA limiter and DFT, then e^{j phase_offset}, H (float32 [B, 2 n_steps, 20] magnitudes or
        None = 1) and sigma times noise (complex64 [B, 2 n_steps, 20], unit variance; None -> Philox(seed), seed 0 = no noise).  sigma: a scalar for every
        stream or B per-stream values (sigma_from_EbNodB(.., rate_Fs=False)).  want_stats: also returns float64 [B, 3] = sum |tx'|^2, max |tx'|, sum |Y|^2 per
        stream (inference.py:215-227's Eq and PAPR; the call then synchronises)."""
        import torch
        assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.dim() == 3 and z.shape[0] == self.B and z.shape[2] == 80 and z.shape[1] >= 1
        n = z.shape[1]
        (sigma, _, _), per = channel_stream_values(self.B, sigma, 0.0, 0.0)
        if H is not None:
            assert H.is_cuda and H.dtype == torch.float32 and H.is_contiguous() and tuple(H.shape) == (self.B, 2 * n, 20)
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.complex64 and noise.is_contiguous() and tuple(noise.shape) == (self.B, 2 * n, 20)
        out = torch.empty_like(z)
        stats = np.zeros((self.B, 3), np.float64) if want_stats else None
        r = self.lib.rade_batch_channel_rs_pa(self.h, z.data_ptr(), H.data_ptr() if H is not None else None, noise.data_ptr() if noise is not None else None,
                                              out.data_ptr(), n, sigma, per["sigma"].ctypes.data if per else None, phase_offset, seed,
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
            assert x.dtype == torch.int16 and (x.dim() == 2 or (x.dim() == 3 and x.shape[2] == 2)) and x.stride(-1) == 1
            assert x.dim() == 2 or x.stride(1) == 2 or x.shape[1] <= 1
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

    # ---- the sound-card wire ------------------------------------------------------------------
    def wire_in(self, i16, n=None, iq: bool = False, gain: float = 1.0):
        """int16 samples to complex64 on the device (rade_batch_wire_in; `int16tof32.py --zeropad` when real).  i16: cuda int16 [B, N], one real channel, or with iq
        [B, N, 2] (or [B, 2 N]) ..IQIQ..; n: samples of each stream (a scalar or B values; default N).  Returns complex64 [B, max(n)] = gain * sample, Q = +0 for a real
        channel; samples past a stream's n are zeros.  gain = 1 gives the reference script's bytes."""
        import torch
        assert i16.is_cuda and i16.dtype == torch.int16 and i16.shape[0] == self.B and (i16.dim() == 2 or (iq and i16.dim() == 3 and i16.shape[2] == 2))
        assert i16.stride(-1) == 1 and (i16.dim() == 2 or i16.stride(1) == 2 or i16.shape[1] <= 1)
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

    # ---- channel ----------------------------------------------------------------------------
    def channel(self, tx, sigma, freq_offset=0.0, n_pre: int = 0, n_post: int = 0, with_eoo: bool = False,
                G=None, noise=None, seed: int = 0, df_dt=0.0, sine_amp: float = 0.0, sine_freq: float = 0.0, rx_gain: float = 1.0):
        """tx complex64 [B, n_sig]; G complex64 [B, n_sig, 2] or None; noise complex64 [B, n_total] or None;
        sine_amp/sine_freq: complex tone over the whole output, rx_gain: final scale (inference.py:285-289).
        sigma / freq_offset / df_dt: a scalar for every stream, or B per-stream values (rade_batch_channel_streams)."""
        import torch
        assert tx.is_cuda and tx.dtype == torch.complex64 and tx.is_contiguous() and tx.shape[0] == self.B
        n_sig = tx.shape[1]
        n_total = n_pre + n_sig + (NEOO if with_eoo else 0) + n_post
        (sigma, freq_offset, df_dt), per = channel_stream_values(self.B, sigma, freq_offset, df_dt)
        rx = torch.empty((self.B, n_total), dtype=torch.complex64, device=tx.device)
        p = ChannelParams(n_sig, n_pre, n_post, int(with_eoo), sigma, freq_offset, df_dt, None, None, seed, sine_amp, sine_freq, rx_gain)
        if G is not None:
            assert G.is_cuda and G.dtype == torch.complex64 and G.is_contiguous() and tuple(G.shape) == (self.B, n_sig, 2)
            p.G_dev = G.data_ptr()
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.complex64 and noise.is_contiguous() and tuple(noise.shape) == (self.B, n_total)
            p.noise_dev = noise.data_ptr()
        if per is None:
            r = self.lib.rade_batch_channel(self.h, tx.data_ptr(), n_sig, rx.data_ptr(), n_total, C.byref(p), _stream_ptr())
        else:
            r = self.lib.rade_batch_channel_streams(self.h, tx.data_ptr(), n_sig, rx.data_ptr(), n_total, C.byref(p), C.byref(_channel_streams(per)), _stream_ptr())
        if r != n_total:
            raise RuntimeError("rade_batch_channel failed")
        return rx

    def tx_channel(self, features, sigma, freq_offset=0.0, n_pre: int = 0, n_post: int = 0, with_eoo: bool = False,
                   G=None, noise=None, seed: int = 0, df_dt=0.0, want_iq: bool = False):
        """Transmit and channel in one pass (RADAE.forward): features [B, n_mf*12, 36] -> rx complex64 [B, n_total] (and iq if wanted).
        With G the modulator applies the two-path model itself (rade_batch_tx_channel); the whole utterance must fit max_tx_mf.
        sigma / freq_offset / df_dt: a scalar for every stream, or B per-stream values (rade_batch_tx_channel_streams)."""
        import torch
        assert features.is_cuda and features.dtype == torch.float32 and features.is_contiguous()
        B, nfr, w = features.shape
        assert B == self.B and w == 36 and nfr % 12 == 0 and nfr // 12 <= self.max_tx_mf
        n_mf = nfr // 12; n_sig = n_mf * NMF
        n_total = n_pre + n_sig + (NEOO if with_eoo else 0) + n_post
        (sigma, freq_offset, df_dt), per = channel_stream_values(B, sigma, freq_offset, df_dt)
        rx = torch.empty((B, n_total), dtype=torch.complex64, device=features.device)
        iq = torch.empty((B, n_sig), dtype=torch.complex64, device=features.device) if (want_iq or G is None) else None
        p = ChannelParams(n_sig, n_pre, n_post, int(with_eoo), sigma, freq_offset, df_dt, None, None, seed, 0.0, 0.0, 1.0)
        if G is not None:
            assert G.is_cuda and G.dtype == torch.complex64 and G.is_contiguous() and tuple(G.shape) == (B, n_sig, 2)
            p.G_dev = G.data_ptr()
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.complex64 and noise.is_contiguous() and tuple(noise.shape) == (B, n_total)
            p.noise_dev = noise.data_ptr()
        iq_ptr = iq.data_ptr() if iq is not None else None
        if per is None:
            r = self.lib.rade_batch_tx_channel(self.h, features.data_ptr(), n_mf, iq_ptr, n_sig, rx.data_ptr(), n_total, C.byref(p), _stream_ptr())
        else:
            r = self.lib.rade_batch_tx_channel_streams(self.h, features.data_ptr(), n_mf, iq_ptr, n_sig, rx.data_ptr(), n_total, C.byref(p),
                                                       C.byref(_channel_streams(per)), _stream_ptr())
        if r != n_total:
            raise RuntimeError("rade_batch_tx_channel failed")
        return (rx, iq) if want_iq else rx

    def multipath_gen(self, channel: str, n_out: int, seed: int = 1, noise_low=None, fs: int = 8000):
        """Doppler-spread samples G [B, n_out, 2] complex64 generated on the device (multipath_samples.m presets
        mpg / mpp / mpd).  noise_low: optional complex64 [B, 2, n_low + 100] unit-variance-per-component low-rate
        input noise (parity with channel_tools.multipath_g); otherwise Philox from `seed`."""
        import torch
        from .channel_tools import PRESETS, doppler_plan
        taps, ratio, n_low = doppler_plan(PRESETS[channel][0], fs, n_out)
        G = torch.empty((self.B, n_out, 2), dtype=torch.complex64, device=self.device)
        tp = np.ascontiguousarray(taps, dtype=np.float32)
        nz = None
        if noise_low is not None:
            assert noise_low.is_cuda and noise_low.dtype == torch.complex64 and noise_low.is_contiguous() and tuple(noise_low.shape) == (self.B, 2, n_low + len(tp))
            nz = noise_low.data_ptr()
        r = self.lib.rade_batch_multipath_gen(self.h, tp.ctypes.data_as(C.POINTER(C.c_float)), len(tp), ratio, n_out, nz, seed, G.data_ptr(), _stream_ptr())
        if r != n_out:
            raise RuntimeError("rade_batch_multipath_gen failed")
        return G

    def multipath_h_gen(self, channel: str, n_sym: int, rs: int = 2000, nc: int = 1, fs: int = 8000, seed: int = 1, noise_low=None, complex_: bool = False):
        """multipath_samples.m's H output generated on the device: |H| float32 [B, n_sym, nc] (complex64 with complex_) at symbol rate rs from the preset's
        Doppler process at fs (BBFM.md:37: multipath_h_gen("lmr60", 20000) is `multipath_samples("lmr60", 8000, 2000, 1, 10, ...)` per stream)."""
        import torch
        from .channel_tools import PRESETS
        m = fs // rs
        assert m * rs == fs
        n_g = (n_sym - 1) * m + 1
        G = self.multipath_gen(channel, n_g, seed=seed, noise_low=noise_low, fs=fs)
        H = torch.empty((self.B, n_sym, nc, 2) if complex_ else (self.B, n_sym, nc), dtype=torch.float32, device=self.device)
        if self.lib.rade_batch_multipath_h(self.h, G.data_ptr(), n_g, m, n_sym, nc, PRESETS[channel][1], float(rs), int(complex_), H.data_ptr(), _stream_ptr()) != n_sym:
            raise RuntimeError("rade_batch_multipath_h failed")
        return torch.view_as_complex(H) if complex_ else H

    # ---- receive ----------------------------------------------------------------------------
    def rx_reset(self, lcg_seeds: Optional[Sequence[int]] = None):
        if lcg_seeds is None:
            self.lib.rade_batch_rx_reset(self.h)
        else:
            arr = (C.c_uint * self.B)(*[int(s) for s in lcg_seeds])
            self.lib.rade_batch_rx_set_lcg(self.h, arr)

    def rx(self, rx, n_avail=None, max_calls: int = 1 << 20, features_out=None, eoo_out=None):
        """rx complex64 [B, N] holding each stream's not-yet-consumed samples.  Returns
        (features [B, cap, 432] -- [B, cap, 240] latents for an engine opened with BYPASS_DEC --, status list[RxStatus], eoo [B, 180]).  features_out / eoo_out: caller-owned device buffers (as a C host passes
        them: rows beyond status.n_valid, and the EOO bits of a stream without status.has_eoo, keep whatever they held); without them fresh zeroed
        ones are allocated per call."""
        import torch
        assert rx.is_cuda and rx.dtype == torch.complex64 and rx.is_contiguous() and rx.shape[0] == self.B
        N = rx.shape[1]
        avail = np.full(self.B, N, np.int32) if n_avail is None else np.ascontiguousarray(n_avail, dtype=np.int32)
        cap = min(max_calls, int(avail.max()) // 800 + 1)
        if features_out is None:
            features_out = torch.zeros((self.B, cap, self.rx_row_floats), dtype=torch.float32, device=rx.device)
        # features_out.shape[1] is the per-stream frame capacity handed to the C ABI: a stream pauses (status.consumed < avail)
        # once it has filled its rows, so a short buffer never makes the kernel write into the next stream's region
        assert features_out.is_cuda and features_out.dtype == torch.float32 and features_out.is_contiguous() and features_out.dim() == 3 \
            and features_out.shape[0] == self.B and features_out.shape[1] >= 1 and features_out.shape[2] == self.rx_row_floats
        eoo = eoo_out if eoo_out is not None else torch.zeros((self.B, NEOO_BITS), dtype=torch.float32, device=rx.device)
        assert eoo.is_cuda and eoo.dtype == torch.float32 and eoo.is_contiguous() and tuple(eoo.shape) == (self.B, NEOO_BITS)
        status = (RxStatus * self.B)()
        r = self.lib.rade_batch_rx(self.h, rx.data_ptr(), N, avail.ctypes.data_as(C.POINTER(C.c_int)), max_calls, features_out.data_ptr(),
                                   features_out.shape[1] * self.rx_row_floats, eoo.data_ptr(), status, _stream_ptr())
        if r:
            raise RuntimeError("rade_batch_rx failed")
        self._rx_last = (features_out.data_ptr(), list(status)) if self.rx_row_floats == FEAT_MF else None    # loss()'s default n_hat
        return features_out, list(status), eoo

    # ---- scoring ----------------------------------------------------------------------------
    def loss(self, features, features_hat, n_in=None, n_hat=None, clip_start: int = 0, clip_end: int = 0, frame_loss: bool = False):
        """loss.py:find_loss (:64-91) of every stream in one launch (rade_batch_loss): features / features_hat cuda float32 [B, rows, width >= 20]
        (the first 20 columns of each row are used) or rx()'s [B, n_valid_cap, 432], read as rows of 36.  n_in / n_hat: per-stream row counts (see
        loss_lengths); n_hat defaults to 12 x n_valid of the rx() call that returned features_hat, else every row.  clip_start / clip_end: loss.py's flags.
        Returns (loss float64 [B], start int32 [B], frame_loss or None): NaN and -1 for a stream with no decoded rows or more than were sent;
        acq_time = 0.01 s x start; frame_loss cuda float32 [B, max n_hat] holds loss.py's per-frame curve in [0, n_hat - start) of each row, NaN after."""
        import torch

        def rows(x, what):
            assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == self.B and x.stride(2) == 1, what
            if x.shape[2] == FEAT_MF and x.stride(1) == FEAT_MF:
                x = x.as_strided((self.B, x.shape[1] * 12, 36), (x.stride(0), 36, 1))
            assert x.shape[2] >= 20 and x.stride(1) >= 20, what
            return x, (x.stride(0) if self.B > 1 else 0), x.stride(1)
        last = getattr(self, "_rx_last", None)
        if n_hat is None and last is not None and last[0] == features_hat.data_ptr():
            n_hat = last[1]
        f, f_sb, f_row = rows(features, "features")
        h, h_sb, h_row = rows(features_hat, "features_hat")
        ni, nh = loss_lengths(self.B, n_in, n_hat, f.shape[1], h.shape[1], clip_start, clip_end)
        fl = None
        if frame_loss:
            fl = torch.full((self.B, max(int(nh.max(initial=0)), 1)), float("nan"), dtype=torch.float32, device=f.device)
        loss = np.zeros(self.B, np.float64)
        start = np.zeros(self.B, np.int32)
        r = self.lib.rade_batch_loss(self.h, f.data_ptr(), f_sb, f_row, ni.ctypes.data, h.data_ptr() + 4 * clip_start * h_row, h_sb, h_row, nh.ctypes.data,
                                     loss.ctypes.data, start.ctypes.data, fl.data_ptr() if fl is not None else None, fl.shape[1] if fl is not None else 0,
                                     _stream_ptr())
        if r < 0:
            raise RuntimeError("rade_batch_loss failed")
        return loss, start, fl

    def rx_ideal(self, rx, n_mf: int, time_offset: int = -16, eq: str = "ls", coarse_mag: bool = True, freq_offset=None, df_dt=None, z_ref=None,
                 feat_width: int = 84):
        """The ideal-timing receiver of RADAE.forward / RADAE.receiver (rade_batch_rx_ideal): rx complex64 [B, >= n_mf*960], every stream's first modem frame at
        sample 0.  eq: "ls" (--eq_ls), "mean6", "all" (per_carrier_eq off) or "none" (no --pilot_eq).  freq_offset / df_dt: per-stream known offsets (a scalar
        is taken for every stream) removed before the DFT (--correct_freq_offset).  z_ref [B, n_mf*3, 80]: count bit errors (ber_test).  feat_width: the blob's
        decoder output per step (84 model19_check3, 80 model05), 0 = no decoder.
        Returns (features [B, n_mf*3, feat_width] or None, z_hat [B, n_mf*3, 80], n_errors np.int64 [B] or None)."""
        import torch
        assert rx.is_cuda and rx.dtype == torch.complex64 and rx.dim() == 2 and rx.shape[0] == self.B and rx.stride(1) == 1 and rx.shape[1] >= n_mf * NMF
        z_hat = torch.empty((self.B, n_mf * 3, 80), dtype=torch.float32, device=rx.device)
        feats = None
        if feat_width:
            feats = torch.empty((self.B, n_mf * 3, feat_width), dtype=torch.float32, device=rx.device)
        keep = []

        def per_stream(v):
            if v is None:
                return None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (self.B,)))
            keep.append(a)
            return a.ctypes.data
        p = IdealRxParams(int(time_offset), EQ_MODES[eq], int(coarse_mag), per_stream(freq_offset), per_stream(df_dt), None, None)
        n_err = None
        if z_ref is not None:
            assert z_ref.is_cuda and z_ref.dtype == torch.float32 and z_ref.is_contiguous() and tuple(z_ref.shape) == (self.B, n_mf * 3, 80)
            n_err = np.zeros(self.B, np.int64)     # C long
            p.z_ref_dev = z_ref.data_ptr(); p.n_errors_host = n_err.ctypes.data
        r = self.lib.rade_batch_rx_ideal(self.h, rx.data_ptr(), _row_stride(rx, rx.shape[1]), n_mf, C.byref(p), z_hat.data_ptr(), feats.data_ptr() if feats is not None else None,
                                         _stream_ptr())
        if r != n_mf:
            raise RuntimeError("rade_batch_rx_ideal failed (n_mf >= 2, time_offset in [-32, 0], 3 n_mf <= 3 max_tx_mf with decode)")
        return feats, z_hat, n_err

    def rx_filtered(self, b: int, n: int) -> np.ndarray:
        """The first n band-pass filtered samples stream b's receiver read in the most recent rx() invocation (complex_bpf.bpf output)."""
        out = np.zeros(n, np.complex64)
        got = self.lib.rade_batch_rx_filtered(self.h, b, out.ctypes.data_as(C.c_void_p), n)
        if got < 0:
            raise RuntimeError("rade_batch_rx_filtered failed")
        return out[:got]

    def sync_counts(self):
        """(waits that slept on the blocking event, waits that spun) of this engine's rx() calls so far"""
        a, b = C.c_long(0), C.c_long(0)
        if not hasattr(self.lib, "rade_batch_sync_counts"):      # (older A/B builds loaded through $RADE_LIBRADEHIP)
            return 0, 0
        self.lib.rade_batch_sync_counts(self.h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def rx_stream_cycles(self) -> np.ndarray:
        """Shader-clock cycles each stream's workgroup spent in the most recent receiver launch."""
        out = np.zeros(self.B, np.int64)
        if self.lib.rade_batch_rx_stream_cycles(self.h, out.ctypes.data_as(C.c_void_p)) != self.B:
            raise RuntimeError("rade_batch_rx_stream_cycles failed")
        return out

    def rx_trace(self, b: int = 0):
        """Per-call trace of stream b in the layout of tests/golden/rxtrace_*.npz."""
        n = self.trace_calls
        tr = (RxTrace * n)()
        z = np.zeros((n, ZMF), np.float32)
        got = self.lib.rade_batch_rx_get_trace(self.h, b, tr, z.ctypes.data_as(C.c_void_p), n)
        if got < 0:
            raise RuntimeError("trace not enabled")
        ints = ["state_before", "state_after", "nin_before", "nin_after", "ret", "tmax", "f_ind_max", "valid_count", "uw_errors", "synced_count", "snr_int"]
        flts = ["fmax", "Dthresh", "Dtmax12", "Dtmax12_eoo", "snrdB_3k_est"]
        d = {k: np.array([getattr(tr[i], k) for i in range(got)], np.int32) for k in ints}
        d.update({k: np.array([getattr(tr[i], k) for i in range(got)], np.float64) for k in flts})
        d["z_all"] = z[:got]
        d["z_hat"] = z[:got][(d["ret"] & 1) == 1]
        d["eoo_out"] = z[:got][(d["ret"] & 2) == 2][:, :NEOO_BITS]
        return d


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

    def __init__(self, engine: BatchEngine, ppm, t0=0.0, mode: str = "sinc32"):
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

    def __init__(self, engine: BatchEngine, L: int, M: int, gain: float = 1.0):
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

    def __init__(self, engine: BatchEngine, Fs: float, fc: float, fd: float, real: bool = False, sigma: float = 0.0, seed: int = 0):
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

    def __init__(self, engine: BatchEngine, Fs: float, fc: float, fd: float, b1, b2, complex_out: bool = False, ph_dont_limit: bool = False):
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
