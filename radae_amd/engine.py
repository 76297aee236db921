"""Python binding of the batched HIP engine (include/rade_batch.h) over ctypes: the engine proper -- open / close, transmit, channel, receive, loss, the ideal-timing
receiver, profiling and multipath.  The C ABI itself (structures, constants, prototypes, load_library) is radae_amd/abi.py; the front-end stages, which BatchEngine
inherits as methods, are radae_amd/stages.py.  Every name either of them defines that was reachable as radae_amd.engine.X is imported here by name and stays so.

PyTorch is used only as plumbing: device tensors own the HBM buffers whose raw pointers are handed
to the C ABI, and `torch.cuda.current_stream()` supplies the hipStream_t.  All compute happens in
radae_amd/libradehip.so (radae_amd/csrc); there is no CPU or PyTorch fallback -- if the shared
library or a GPU is missing this module raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from .abi import (BOTTLENECK1, BYPASS_DEC, DEFAULT_BLOB, EQ_MODES, EXPORTED_SYMBOLS, FEAT_MF, FM_C64, FM_F32, FM_OUT_COMPLEX, FM_OUT_REAL, LIB_PATH, NEOO, NEOO_BITS,  # noqa: F401
                  NIN_MAX, NMF, RATE_C64, RATE_S16_IQ, RATE_S16_REAL, RESAMPLE_MODES, SPEC_C64, SPEC_S16_REAL, TX_BPF, TX_LINEAR, WIRE_IQ, WIRE_REAL, ZMF, BatchConfig,
                  ChannelParams, ChannelStreams, CnoParams, CnoPlan, CnoResult, FmDemodParams, FmModParams, IdealRxParams, RateParams, ResampleParams, RxStatus, RxTrace,
                  PsdPlan, SigstatResult, SpecgramParams, SpecgramPlan, _lib, load_library)
from .stages import (CNO_FS, CNO_HOP, FM_DE_EMP_TC, RESAMPLE_PPM_MAX, SPEC_HI, SPEC_LO, SPEC_NFFT, SPEC_STEP, SPEC_WIN, BatchStages, ClockOffset, FmDemodulator,  # noqa: F401
                     FmModulator, RateConverter, WireMeters, ber_best, file_plan, _per_stream, _row_stride, _scalar_or_streams, _stream_ptr, chirp, cno_plan, cno_windows, fm_deemph_len,
                     fm_pre_emphasis, fm_sigma, fm_taps, ppm_from_rates, rate_count, rate_taps, resample_count, resample_taps, specgram_levels, specgram_plan,
                     specgram_slices, specgram_window)
from .stages import PSD_FS, PSD_HEAD, PSD_NFFT, SigStat, psd_bandwidth, psd_octave_default, psd_plan, psd_segments, psd_window  # noqa: F401
from .stages import ChannelStream, multipath_gain  # noqa: F401
from .abi import SNR_SYMBOLS, SnrParams, SnrPoint, SnrSums  # noqa: F401
from .stages import SNR_C, SNR_M, SNR_NC, SNR_NS, SnrSweep, snr_finish, snr_fit, snr_sigma, snr_sweep, snr_track, snr_windows_rows  # noqa: F401


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
    both = {name: _scalar_or_streams(B, v, name) for name, v in (("sigma", sigma), ("freq_offset", freq_offset), ("df_dt", df_dt))}
    per = {name: a for name, (_, a) in both.items() if a is not None}
    return tuple(s for s, _ in both.values()), (per or None)


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
        a = _per_stream(B, v, np.int64, what)
        if a.max(initial=0) > rows:
            raise ValueError(f"{what}: {int(a.max())} rows asked for, the buffer holds {rows}")
        return a
    if clip_start < 0 or clip_end < 0:
        raise ValueError("clip_start / clip_end must be >= 0")
    ni = per_stream(n_in, rows_in, "n_in")
    nh = per_stream(n_hat, rows_hat, "n_hat")
    return ni.astype(np.int32), np.maximum(nh - clip_start - clip_end, 0).astype(np.int32)


class BatchEngine(BatchStages):
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
        self.lib.rade_batch_profile_ref(self.h, C.c_void_p(event_handle))

    def profile_intervals(self, cls_name: str, max_n: int = 4096):
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

    # ---- channel ----------------------------------------------------------------------------
    def _channel_call(self, name: str, head, device, n_sig: int, n_pre: int, n_post: int, with_eoo, sigma, freq_offset, df_dt, G, noise, seed: int,
                      sine_amp: float = 0.0, sine_freq: float = 0.0, rx_gain: float = 1.0):
        """What channel and tx_channel share: rade_channel_params with G and noise checked, and the call of rade_batch_<name> -- of its _streams form when a value is per
        stream -- with `head` as the arguments ahead of rx_out_dev.  Returns rx complex64 [B, n_total]."""
        import torch
        n_total = n_pre + n_sig + (NEOO if with_eoo else 0) + n_post
        (sigma, freq_offset, df_dt), per = channel_stream_values(self.B, sigma, freq_offset, df_dt)
        rx = torch.empty((self.B, n_total), dtype=torch.complex64, device=device)
        p = ChannelParams(n_sig, n_pre, n_post, int(with_eoo), sigma, freq_offset, df_dt, None, None, seed, sine_amp, sine_freq, rx_gain)
        if G is not None:
            assert G.is_cuda and G.dtype == torch.complex64 and G.is_contiguous() and tuple(G.shape) == (self.B, n_sig, 2)
            p.G_dev = G.data_ptr()
        if noise is not None:
            assert noise.is_cuda and noise.dtype == torch.complex64 and noise.is_contiguous() and tuple(noise.shape) == (self.B, n_total)
            p.noise_dev = noise.data_ptr()
        if per is None:
            r = getattr(self.lib, name)(self.h, *head, rx.data_ptr(), n_total, C.byref(p), _stream_ptr())
        else:
            r = getattr(self.lib, name + "_streams")(self.h, *head, rx.data_ptr(), n_total, C.byref(p), C.byref(_channel_streams(per)), _stream_ptr())
        if r != n_total:
            raise RuntimeError(f"{name} failed")
        return rx

    def channel(self, tx, sigma, freq_offset=0.0, n_pre: int = 0, n_post: int = 0, with_eoo: bool = False,
                G=None, noise=None, seed: int = 0, df_dt=0.0, sine_amp: float = 0.0, sine_freq: float = 0.0, rx_gain: float = 1.0):
        """tx complex64 [B, n_sig]; G complex64 [B, n_sig, 2] or None; noise complex64 [B, n_total] or None;
        sine_amp/sine_freq: complex tone over the whole output, rx_gain: final scale (inference.py:285-289).
        sigma / freq_offset / df_dt: a scalar for every stream, or B per-stream values (rade_batch_channel_streams)."""
        import torch
        assert tx.is_cuda and tx.dtype == torch.complex64 and tx.is_contiguous() and tx.shape[0] == self.B
        n_sig = tx.shape[1]
        return self._channel_call("rade_batch_channel", (tx.data_ptr(), n_sig), tx.device, n_sig, n_pre, n_post, with_eoo, sigma, freq_offset, df_dt, G, noise, seed,
                                  sine_amp, sine_freq, rx_gain)

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
        iq = torch.empty((B, n_sig), dtype=torch.complex64, device=features.device) if (want_iq or G is None) else None
        rx = self._channel_call("rade_batch_tx_channel", (features.data_ptr(), n_mf, iq.data_ptr() if iq is not None else None, n_sig), features.device, n_sig, n_pre,
                                n_post, with_eoo, sigma, freq_offset, df_dt, G, noise, seed)
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
        fo, dd = (None if v is None else _per_stream(self.B, v, np.float32, what) for v, what in ((freq_offset, "freq_offset"), (df_dt, "df_dt")))
        p = IdealRxParams(int(time_offset), EQ_MODES[eq], int(coarse_mag), None if fo is None else fo.ctypes.data, None if dd is None else dd.ctypes.data, None, None)
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
        d = {k: np.array([getattr(tr[i], k) for i in range(got)], np.int32 if t is C.c_int else np.float64) for k, t in RxTrace._fields_ if not k.startswith("pad")}
        d["z_all"] = z[:got]
        d["z_hat"] = z[:got][(d["ret"] & 1) == 1]
        d["eoo_out"] = z[:got][(d["ret"] & 2) == 2][:, :NEOO_BITS]
        return d
