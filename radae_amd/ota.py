"""The receive side of the reference's stored-file off-air test on the device: what ota_test.sh:136-163 (process_rx) does to a recording between the `sox -r 8k` stage
(BatchEngine.rate_convert) and the report, for a batch of recordings at once.

    chirp header (4.5 s sent, >= 4 s received) - 1 s silence - x s SSB - 1 s silence - x s RADAE            ota_test.sh:151, :322-379

process_rx optionally draws the spectrogram of the whole recording (ota_test.sh:130-134: plot_specgram(s, 8000, 200, 3000); BatchEngine.specgram, write_png), estimates
the C/No of the chirp header and the time it starts at (est_CNo.py over the first 10 s: BatchEngine.cno_est), trims the recording there, splits what follows by the
layout above and hands the last part to the receiver.  The SSB part is only located (its bounds are returned): analog_compressor and the speech path of the script are
outside this project."""
from __future__ import annotations

import math
import struct
import zlib
from dataclasses import dataclass

import numpy as np

from . import engine as _engine

FS = 8000
CHIRP_WINDOW_S = 10                   # ota_test.sh:138: `trim 0 10`
HEADER_S = 4.5                        # ota_test.sh:336
SPEC_BAND = (200.0, 3000.0)           # ota_test.sh:133: plot_specgram(s, 8000, 200, 3000)


def ota_header(amp: float = 0.25) -> np.ndarray:
    """the 4.5 s, 400-2000 Hz chirp header as ota_test.sh:336 makes it (`chirp.py .. 4.5 --amp AMP`): complex64; the transmitter sends its real part"""
    return _engine.chirp(HEADER_S, amp=amp)


def nearest_sample(seconds: float) -> int:
    """seconds -> samples at 8 kHz, to the nearest sample, halves upward.  This is the one rounding of process_rx that is NOT pinned against the reference: the script hands
    `sox trim` a time printed with six decimals, and how sox rounds it to samples could not be checked (no sox where this was written)."""
    return int(math.floor(seconds * FS + 0.5))


def layout(total: int):
    """ota_test.sh:151-158 for a trimmed recording of `total` samples: x = (duration - 6) / 2 seconds, the SSB part at 5 s for x s, RADAE from 5 + x s.  Returns
    (ssb_start, ssb_len, radae_start) in samples from the trim point."""
    x = (total / FS - 6) / 2
    if x < 0:
        raise ValueError(f"{total} samples behind the chirp's start: shorter than the 6 s of header and silences")
    return 5 * FS, nearest_sample(x), nearest_sample(5 + x)


@dataclass
class OtaResult:
    max_time: np.ndarray              # [B] seconds: the `Measured:` line's Time
    CNodB: np.ndarray                 # [B] C/No
    SNR3kdB: np.ndarray               # [B] SNR3k
    start: np.ndarray                 # [B] sample at which the recording is trimmed (the best window's start)
    ssb: np.ndarray                   # [B, 2] first and one-past-last sample of the SSB part, in samples of the untrimmed recording
    radae_start: np.ndarray           # [B] first sample handed to the receiver, in samples of the untrimmed recording
    n_radae: np.ndarray               # [B] samples handed to the receiver
    features: object                  # BatchEngine.rx's three results
    status: list
    eoo: object
    spec: object = None               # with spectrogram=True: uint8 [B, W, 717] on the device, the levels of the whole untrimmed recording, 200-3000 Hz (BatchEngine.specgram)
    spec_slices: object = None        # [B] slices (rows of spec) of each recording


def write_png(path, img, n_slices=None) -> None:
    """One stream's spectrogram as an 8-bit grey-scale PNG, written with zlib and struct alone.  img: [W, n_bins] levels (a host array or a device tensor), rows = slices;
    n_slices: the rows that count (default all).  The picture has time to the right and frequency upward, as plot_specgram.m:16-17 shows it (imagesc(t, f, ..) with
    set(gca, "ydir", "normal")): pixel (row r, column c) = img[c, n_bins - 1 - r].  DEVIATION: no axes, no colour map, no JPEG."""
    a = np.asarray(img.detach().cpu().numpy() if hasattr(img, "detach") else img, dtype=np.uint8)
    assert a.ndim == 2
    a = a[:a.shape[0] if n_slices is None else int(n_slices)]
    pix = np.ascontiguousarray(a.T[::-1])                                  # [n_bins, W]: the highest bin on top
    h, w = pix.shape
    raw = np.zeros((h, w + 1), np.uint8)                                   # filter type 0 in front of every row
    raw[:, 1:] = pix

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


def process_rx(engine, x, n=None, window_time: float = 4.0, flow: float = 400.0, fhigh: float = 2000.0, spectrogram: bool = False) -> OtaResult:
    """x: cuda complex64 [B, S], a batch of 8 kHz recordings (a real recording as (x, +0), what wire_in and rate_convert deliver); n: samples of each (default S).
    cno_est over the first min(n, 80000) samples; start = max_st; the layout of ota_test.sh:151-158 behind it (seconds to samples: nearest_sample, not pinned against
    sox); the trim as rate_convert with L = M = 1 and n0 = start + radae_start (a bit-exact copy); then the receiver.  spectrogram: first, as in the script, the
    spectrogram of the whole untrimmed recording, 200-3000 Hz (result.spec, result.spec_slices; every n above 1280).  Synchronises the current stream."""
    B = engine.B
    S = x.shape[1]
    n = _engine._per_stream(B, S if n is None else n, np.int32, "n")
    spec, spec_slices = (engine.specgram(x, n=n, fmin=SPEC_BAND[0], fmax=SPEC_BAND[1])[:2]) if spectrogram else (None, None)
    res = engine.cno_est(x, n=np.minimum(n, CHIRP_WINDOW_S * FS), window_time=window_time, flow=flow, fhigh=fhigh)
    start = np.array([r.max_st for r in res], np.int64)
    lay = [layout(int(n[b] - start[b])) for b in range(B)]
    ssb = np.array([[start[b] + s0, start[b] + s0 + sl] for b, (s0, sl, _) in enumerate(lay)], np.int64)
    radae_start = np.array([start[b] + r0 for b, (_, _, r0) in enumerate(lay)], np.int64)
    n_radae = (n - radae_start).astype(np.int32)
    y, n_y = engine.rate_convert(x, 1, 1, n_out=n_radae, n_in=n, n0=radae_start)
    features, status, eoo = engine.rx(y.contiguous(), n_avail=n_y)
    return OtaResult(start / FS, np.array([r.max_CNodB for r in res]), np.array([r.max_SNRdB for r in res]), start, ssb, radae_start, n_radae, features, status, eoo,
                     spec, spec_slices)
