#!/usr/bin/env python3
"""Time of the chirp C/No estimator on the device (rade_batch_cno_est: k_cno_blocks + k_cno_sum, the read-back and the host arithmetic) in alternating rounds in one
process: 256 streams x 80000 samples (24 windows of 32000) at the defaults, next to
    (a) the device's own complex64 copy of the same input bytes (HIP events),
    (b) the reference's algorithm, float64 numpy.fft.fft per window as est_CNo.py runs it, on one host core (--host_streams streams timed, scaled to the batch) plus the copy
        of the input across the host link,
    (c) the share of the call spent behind the kernels: the read-back of the band sums and the host arithmetic (the call's host-clock time minus the kernels' event time).
The call synchronises its stream, so it is timed by the host clock around the call; the kernels alone by HIP events through the engine's profiler.  DESIGN.md quotes the
medians.

    python3 tools/time_cno.py [--streams 256] [--samples 80000] [--rounds 5] [--reps 3] [--host_streams 4] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from radae_amd.engine import BatchEngine, CnoParams, CnoResult, cno_plan, cno_windows
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256); ap.add_argument("--samples", type=int, default=80000); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--host_streams", type=int, default=4); ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    B, S = a.streams, a.samples
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    lib, h = eng.lib, eng.h
    g = torch.Generator(device=dev); g.manual_seed(1)
    x = torch.view_as_complex(torch.randn((B, S, 2), generator=g, device=dev, dtype=torch.float32) * 3000.0)
    y = torch.empty_like(x)
    q = cno_plan()
    n_win = cno_windows(S, q.N)
    n = np.full(B, S, np.int32)
    res = (CnoResult * B)()
    p = CnoParams(4.0, 400.0, 2000.0)
    sp = lambda: torch.cuda.current_stream().cuda_stream

    def call():
        assert lib.rade_batch_cno_est(h, x.data_ptr(), S, n.ctypes.data, p, None, 0, res, sp()) == 0

    def wall(fn, reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def kernels(reps):
        """the two launches alone, by the engine's HIP-event profiler (class `channel`)"""
        eng.profile(True)
        for _ in range(reps):
            call()
        eng.profile(False)
        got = eng.profile_get()["channel"]
        return got["ms"] / max(got["launches"], 1)

    copy = lambda: y.copy_(x)
    for _ in range(2):
        call(); copy()
    torch.cuda.synchronize()
    t = {"call": [], "kernels": [], "copy": []}
    for _ in range(a.rounds):
        t["call"].append(wall(call, a.reps))
        t["kernels"].append(kernels(a.reps))
        t["copy"].append(events(copy, a.reps))

    # (b) the reference's algorithm on one host core: np.fft.fft of every window in float64 (est_CNo.py:31-45), plus the input across the host link
    Bh = max(min(a.host_streams, B), 1)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    xh = x[:Bh].cpu().numpy()
    for b in range(Bh):
        for st in np.arange(0, S - q.N, 2000):
            Rx = np.abs(np.fft.fft(xh[b, st:st + q.N])) ** 2
            np.sum(Rx[q.flow_bin:q.fhigh_bin]); np.sum(Rx[q.noise_st:q.noise_en])
    host_ms = 1e3 * (time.perf_counter() - t0) * B / Bh
    stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    out = {"streams": B, "samples": S, "windows_per_stream": n_win, "N": q.N, "J": q.J, "rounds": a.rounds, "reps": a.reps, "host_streams": Bh,
           "ms_per_call": {k: stat(v) for k, v in t.items()}, "host_numpy_fft_ms_scaled_to_the_batch": host_ms, "input_bytes": 8 * B * S}
    call_ms, k_ms, c_ms = (out["ms_per_call"][k]["median"] for k in ("call", "kernels", "copy"))
    out["call_over_copy"] = call_ms / c_ms
    out["host_over_call"] = host_ms / call_ms
    out["share_behind_the_kernels"] = max(call_ms - k_ms, 0.0) / call_ms
    out["first_result"] = {"max_st": int(res[0].max_st), "max_CNodB": float(res[0].max_CNodB)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
