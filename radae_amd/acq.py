"""The stored-file receiver (rx.py) for a batch of recordings: whole-file pilot acquisition (rx.py:96-195) and, behind it, the decode of the acquired file (rx.py:197-276).

rx.py band-pass filters the whole file, then walks it one modem frame at a time: detect_pilots over 2112 samples, a small state machine, refine where it acquires; with
--acq_test it starts searching again after every acquisition and reports passes, fails, P(fail) and the mean acquisition time.  Here every hop of every stream is one
device call (BatchEngine.acq_detect), the state machine and the statistics are the library's host functions, and refine is one launch for all events
(BatchEngine.acq_refine): acquire().  In its normal run the script then advances one more frame, refines there, trims to the refined timing, mixes the refined frequency
out, demodulates with that one fixed estimate, decodes and (--ber_test) aligns the latents with the transmitted ones: receive(), on BatchEngine.bpf_file, .rx_file and
.ber_align -- samples to features without leaving the device.  include/rade_batch.h states the arithmetic and the deviations.

Out of scope: --rx_one, --stateful, --plots.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .stages import acq_fmax, acq_stats, acq_track, file_plan

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
    The torch form of the filter: acquire() keeps it (its results are pinned); receive() runs the kernel, BatchEngine.bpf_file, whose mixers are these."""
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


class FileRx(NamedTuple):
    """One stream of receive(): acq (StreamAcq of the script's normal run: at most one event, refined one frame after it), plan (abi.FilePlan: start, n_mf, freq, status),
    z_hat cuda float32 [3 n_mf, 80], features cuda float32 [3 n_mf, feat_width] (None without a decoder) and n_errors (np.int64 [20], the BER alignment's counts; None
    without z_ref)."""
    acq: StreamAcq
    plan: object
    z_hat: object
    features: object
    n_errors: object


def receive(engine, x, n=None, bpf: bool = True, freq_offset=None, time_offset: int = -16, eq: str = "ls", coarse_mag: bool = True, feat_width: int = 84, z_ref=None,
            pacq_error1: float = 1e-5):
    """rx.py's normal run over every stream of x (cuda complex64 [B, S]; n: samples of each stream, default S): the whole-file band-pass (bpf_file), the frame loop up to
    the first acquisition (acq_detect + the host's state machine), the script's refine one frame AFTER the acquiring hop (rx = rx[Nmf:-1]; mf += 1 comes first:
    t_abs = 960 (hop + 1) + tmax in a stream of n - (hop + 1) samples), the plan (file_plan: start = t - Ncp, n_mf, freq; freq_offset replaces freq as --freq_offset
    does), the fixed-timing demodulator and decoder (rx_file) and, with z_ref (cuda float32 [B, N], or (that, n_ref) with the floats of each stream), the BER alignment
    (ber_align).  Returns a list of B FileRx; a stream that does not acquire or cannot be decoded has plan.status != 0 and no rows.  The engine's max_tx_mf bounds the
    frames that can be decoded.  Cost: acq_detect forms the surface of EVERY hop of every file, although the script's loop stops at the first acquisition -- the hops
    behind it are computed and dropped (on long files they are most of the call's time: a detect bounded by a hop count would save them); and refine runs in full even
    when freq_offset replaces its frequency, since its timing is still needed."""
    B = engine.B
    n = np.broadcast_to(np.asarray(x.shape[1] if n is None else n, np.int32), (B,)).copy()
    xf = engine.bpf_file(x, n) if bpf else x
    hops, n_hops = engine.acq_detect(xf, n, pacq_error1)
    tracked, todo, n_ref = [], [], n.copy()
    for b in range(B):
        hb = hops[b, :n_hops[b]]
        fm = acq_fmax(hb)
        ev, log = acq_track(hb, False)
        tracked.append((hb, fm, ev, log))
        for e in ev:
            todo.append((b, NMF * (int(e["hop"]) + 1) + int(e["tmax"]), float(fm[e["hop"]])))
            n_ref[b] = n[b] - (int(e["hop"]) + 1)
    refined = engine.acq_refine(xf, todo, n_ref)
    acqs, plans, at = [], [], 0
    for b, (hb, fm, ev, log) in enumerate(tracked):
        rf = refined[at:at + len(ev)]; at += len(ev)
        acqs.append(StreamAcq(hb, fm, log, ev, rf, None))
        plans.append(file_plan(n[b], int(ev[0]["hop"]), int(rf[0]["t"]), float(rf[0]["f"]), freq_offset) if len(ev) else file_plan(n[b], -1, 0, 0.0, freq_offset))
    feats, z_hat = engine.rx_file(xf, plans, None, time_offset, eq, coarse_mag, feat_width)
    err = None
    if z_ref is not None:
        z_ref, n_zref = z_ref if isinstance(z_ref, tuple) else (z_ref, None)
        err = engine.ber_align(z_ref, z_hat, n_zref, np.array([240 * p.n_mf for p in plans], np.int64))
    return [FileRx(acqs[b], p, z_hat[b, :3 * p.n_mf], None if feats is None else feats[b, :3 * p.n_mf], None if err is None else err[b]) for b, p in enumerate(plans)]
