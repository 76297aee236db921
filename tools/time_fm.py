#!/usr/bin/env python3
"""Time of the analog FM stage on the device (rade_batch_fm_mod: k_fm_sums, k_fm_tile_scan, k_fm_mod; rade_batch_fm_demod: k_fm_demod) by HIP events, in alternating
rounds in one process: the modulator without and with generated noise (float32 in, complex64 out), and the demodulator with the 201-tap filters of fm.m (complex64 in,
float32 out), each next to the device's own complex64 copy of the same number of bytes, and next to the path the call replaces: the float64 restatement of
tests/fm_ref.py on one host core plus the copy of the result across the host link, timed by the host clock on --host_streams streams and scaled to the batch.  Bytes
are what the algorithm has to move (every input sample read once, every output sample written once); FLOP counts two per multiply-add of the two FIRs (4 N1 + 2 N2 per
output sample) for the demodulator and are not stated for the modulator (integer sums and a sincos).  Every call waits once on the host, ahead of its launches, for the
copy of its per-stream records: the figure is per CALL, back to back, and includes the launch gap behind that wait (for the modulator's three short kernels a visible share),
not the kernels alone.  DESIGN.md quotes the medians.

    python3 tools/time_fm.py [--streams 256] [--seconds 10] [--rounds 5] [--reps 3] [--host_streams 2] [--out FILE.json]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

FS, FC, FD, FM_MAX = 48000.0, 12000.0, 5000.0, 3000.0


def main():
    import torch
    import fm_ref as fr
    import stage_timing as stg
    from radae_amd.engine import BatchEngine, FmDemodParams, FmModParams, fm_sigma, fm_taps
    ap = stg.parser(rounds=5, reps=3)
    ap.add_argument("--seconds", type=int, default=10); ap.add_argument("--host_streams", type=int, default=2)
    a = ap.parse_args()
    B, n = a.streams, int(FS) * a.seconds
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    lib, h = eng.lib, eng.h
    t = torch.arange(n, device=dev, dtype=torch.float32)[None, :] + torch.arange(B, device=dev, dtype=torch.float32)[:, None]
    m = (0.5 * torch.sin(2 * np.pi * 1000.0 / FS * t) + 0.5 * torch.sin(2 * np.pi * 3000.0 / FS * t)).contiguous()
    del t
    tx = torch.empty((B, n), dtype=torch.complex64, device=dev)
    y = torch.empty((B, n), dtype=torch.float32, device=dev)
    b1, b2 = (v.astype(np.float32) for v in fm_taps(FS, FM_MAX, FD))
    counts = np.full(B, n, np.int32)
    sp = lambda: torch.cuda.current_stream().cuda_stream
    p_off = FmModParams(FS, FC, FD, 0, 0, 0.0, 0, None, None, None, None)
    p_on = FmModParams(FS, FC, FD, 0, 0, fm_sigma(20.0, FS, FM_MAX, FD), 1, None, None, None, None)
    p_dem = FmDemodParams(FS, FC, FD, 0, 0, b1.ctypes.data, b1.size, b2.ctypes.data, b2.size, None, None, None, 0)
    mod = lambda p: (lambda: lib.rade_batch_fm_mod(h, m.data_ptr(), n, counts.ctypes.data, tx.data_ptr(), n, C.byref(p), sp()))
    dem = lambda: lib.rade_batch_fm_demod(h, tx.data_ptr(), n, counts.ctypes.data, y.data_ptr(), n, counts.ctypes.data, C.byref(p_dem), sp())
    cases = {"mod_noise_off": (mod(p_off), 4 * n + 8 * n), "mod_noise_on": (mod(p_on), 4 * n + 8 * n), "demod": (dem, 8 * n + 4 * n)}
    calls, by = {}, {}
    src = torch.empty((B, n), dtype=torch.complex64, device=dev).view(-1)
    dst = torch.empty((B, n), dtype=torch.complex64, device=dev).view(-1)
    for k, (fn, nbytes) in cases.items():
        def checked(fn=fn):
            assert fn() == 0
        calls[k], by[k] = checked, float(nbytes)
        n_copy = B * nbytes // 16                                  # the device's copy of as many bytes: 8 read + 8 written per complex64 sample
        calls["copy_" + k], by["copy_" + k] = (lambda c=n_copy: dst[:c].copy_(src[:c])), 16.0 * n_copy / B

    calls["mod_noise_on"]()                                        # the demodulator's timed input: a modulated carrier with noise at 20 dB
    stg.warm(calls)
    calls["mod_noise_on"]()
    ts = stg.rounds(calls, a.rounds, a.reps)

    # the host path: the float64 restatement on one core, and the copy of its result across the host link
    th = {}
    Bh = min(a.host_streams, B)
    if Bh > 0:
        mh, xh = m[:Bh].cpu().numpy(), tx[:Bh].cpu().numpy()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = np.stack([fr.mod(mh[b], FS, FC, FD)[0] for b in range(Bh)]).astype(np.complex64)
        tx[:Bh].copy_(torch.from_numpy(out)); torch.cuda.synchronize()
        th["mod_noise_off"] = 1e3 * (time.perf_counter() - t0) * B / Bh
        tx[:Bh].copy_(torch.from_numpy(xh))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = np.stack([fr.demod(xh[b], FS, FC, FD, b1, b2)[0] for b in range(Bh)]).astype(np.float32)
        y[:Bh].copy_(torch.from_numpy(out)); torch.cuda.synchronize()
        th["demod"] = 1e3 * (time.perf_counter() - t0) * B / Bh
    res = {"streams": B, "seconds": a.seconds, "Fs": FS, "N1": int(b1.size), "N2": int(b2.size), "rounds": a.rounds, "reps": a.reps, "host_streams": Bh,
           "ms_per_call": stg.stats(ts), "host_ms_per_call_scaled_to_the_batch": th, "algorithmic_bytes_per_stream": by}
    med = lambda k: res["ms_per_call"][k]["median"] * 1e-3
    res["TB_per_s"] = {k: by[k] * B / med(k) / 1e12 for k in by}
    flop = (4.0 * b1.size + 2.0 * b2.size) * n * B
    res["demod_algorithmic_TFLOP_per_call"] = flop / 1e12
    res["demod_algorithmic_TFLOP_per_s"] = flop / med("demod") / 1e12
    res["call_over_copy"] = {k: med(k) / med("copy_" + k) for k in cases}
    res["host_over_device"] = {k: th[k] / (1e3 * med(k)) for k in th}
    res["x_real_time"] = {k: B * a.seconds / med(k) for k in cases}
    stg.emit(res, a.out)
    eng.close()


if __name__ == "__main__":
    main()
