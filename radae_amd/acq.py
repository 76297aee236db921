"""Whole-file pilot acquisition: the stored-file receiver's front half (rx.py:96-195) for a batch of recordings.

rx.py band-pass filters the whole file, then walks it one modem frame at a time: detect_pilots over 2112 samples, a small state machine, refine where it acquires; with
--acq_test it starts searching again after every acquisition and reports passes, fails, P(fail) and the mean acquisition time.  Here every hop of every stream is one
device call (BatchEngine.acq_detect), the state machine and the statistics are the library's host functions, and refine is one launch for all events
(BatchEngine.acq_refine).  include/rade_batch.h states the arithmetic and the deviations.

Out of scope: decoding the acquired file (rx.py:223-253) -- that is rate_convert(1, 1, n0 = t - Ncp) + rx_ideal(correct_freq_offset = f) + decode on the offsets this
stage returns, a follow-up with its own golden --, and --rx_one, --ber_test, --plots.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .stages import acq_fmax, acq_stats, acq_track

FS, M, NCP, NMF, NC, NTAP = 8000, 160, 32, 960, 30, 101


class StreamAcq(NamedTuple):
    """One stream's acquisition: hops (record array of abi.AcqHop), fmax float64 [n_hops], log (abi.AcqLog per hop: what the script prints), events (abi.AcqEvent),
    refined (abi.AcqRefined: absolute t, f, Dmax per event) and stats (abi.AcqResult; None without acq_test)."""
    hops: np.ndarray
    fmax: np.ndarray
    log: np.ndarray
    events: np.ndarray
    refined: np.ndarray
    stats: object


def bpf_design(ntap: int = NTAP):
    """rx.py:110-113 and dsp.py:42-49: (h float32 [ntap], alpha) of the whole-file input band-pass: bandwidth 1.2 (w[Nc-1] - w[0]) Fs / 2 pi around the carriers'
    mid-point, w = 2 pi (15 + k) / 160 in float32 as the model holds it.  The script's w is a float32 array, so every step of its arithmetic is a float32 operation;
    written out so here (the receiver's own filter, tests/golden/consts.npz: bpf_h, bpf_alpha, bit for bit)."""
    f = np.float32
    w = (f(2 * np.pi) * (15 + np.arange(NC, dtype=f)) / f(M)).astype(f)
    bandwidth = f(1.2) * (w[NC - 1] - w[0]) * f(FS) / f(2 * np.pi)
    centre = (w[NC - 1] + w[0]) * f(FS) / f(2 * np.pi) / f(2)
    Bn = bandwidth / f(FS)
    h = (Bn * np.sinc((np.arange(ntap) - (ntap - 1) / 2).astype(f) * Bn)).astype(f)
    return h, float(f(2 * np.pi) * centre / f(FS))


def complex_bpf(x, ntap: int = NTAP):
    """complex_bpf(ntap, Fs, bandwidth, centre, len).bpf(x) over every row of x (torch complex64 [B, S], any device): mix down by e^{-j alpha (i + 1)}, the real
    low-pass with zero initial memory as ONE conv1d over the batch, mix back up.  The mixer phases are formed in double and rounded once.  DEVIATION: the script builds
    phase_vec_exp from a float32 argument (np.exp(.., dtype=complex64)), which jitters the phase by up to an ulp of alpha i per sample on long files; not reproduced.
    Plumbing, not a hot path: a fused band-pass kernel is out of scope."""
    import torch
    h, alpha = bpf_design(ntap)
    B, S = x.shape
    ang = -alpha * torch.arange(1, S + 1, dtype=torch.float64, device=x.device)
    pv = torch.complex(torch.cos(ang), torch.sin(ang)).to(torch.complex64)
    bb = torch.view_as_real(x * pv)                                                     # [B, S, 2]
    rows = torch.nn.functional.pad(bb.permute(0, 2, 1).reshape(2 * B, 1, S), (ntap - 1, 0))
    y = torch.nn.functional.conv1d(rows, torch.tensor(h, device=x.device).view(1, 1, ntap))      # y[i] = sum_k mem[i + k] h[k] (h is symmetric)
    y = torch.view_as_complex(y.reshape(B, 2, S).permute(0, 2, 1).contiguous())
    return y * pv.conj()


def acquire(engine, x, n=None, bpf: bool = True, acq_test: bool = False, fmax_target: float = 0.0, acq_time_target: float = 1.0, pacq_error1: float = 1e-5, dt_rows=None):
    """rx.py's acquisition over every stream of x (cuda complex64 [B, S]; n: samples of each stream, default S).  bpf: the whole-file input band-pass first (torch, on
    the device).  acq_test False: stop at each stream's first acquisition (the script's normal run) and refine it; True: keep searching, refine and judge every
    acquisition against fmax_target (a scalar or B values, as acq_time_target) and Ncp + Ntap / 2, and fill stats.  Returns a list of B StreamAcq; with dt_rows=(t0, n_rows) also the complex surface D[t0 .. t0 + n_rows) of the (filtered) streams, cuda
    [B, n_rows, 40], from the same detect call (rx.py --write_Dt)."""
    B = engine.B
    fmax_target, acq_time_target = (np.broadcast_to(np.asarray(v, np.float64), (B,)) for v in (fmax_target, acq_time_target))      # a scalar or B per-stream values
    n = np.broadcast_to(np.asarray(x.shape[1] if n is None else n, np.int32), (B,)).copy()
    if bpf:
        x = complex_bpf(x).contiguous()
    hops, n_hops, *dt = engine.acq_detect(x, n, pacq_error1, dt_rows)
    tracked, todo = [], []
    for b in range(B):
        hb = hops[b, :n_hops[b]]
        fm = acq_fmax(hb)
        ev, log = acq_track(hb, acq_test)
        tracked.append((hb, fm, ev, log))
        todo += [(b, NMF * int(e["hop"]) + int(e["tmax"]), float(fm[e["hop"]])) for e in ev]
    refined = engine.acq_refine(x, todo, n)
    out, at = [], 0
    for b, (hb, fm, ev, log) in enumerate(tracked):
        rf = refined[at:at + len(ev)]; at += len(ev)
        st = acq_stats(ev, rf, len(hb), NTAP if bpf else 0, fmax_target[b], acq_time_target[b]) if acq_test else None
        out.append(StreamAcq(hb, fm, log, ev, rf, st))
    return (out, dt[0]) if dt else out
