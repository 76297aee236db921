#!/usr/bin/env python3
"""Time of the SNR estimator trials on the device (rade_batch_snr_trials: k_snr_trials, the read-back of the six sums per window) in alternating rounds in one process,
at two shapes with generated noise and a complex H per stream:
    curves   75 streams x 60 windows x 8 rows: est_snr_curves.sh (three channels x 25 set points, --Nt 60, -T 1.0)
    large    256 streams x 4096 windows x 8 rows
each next to
    (a) the device's own copy of the H bytes the call reads (HIP events),
    (b) the float64 model of tests/snr_ref.py (est_pilots as array operations, far cheaper than the reference's loop of Nw x Nc small torch products) on one host core,
        --host_windows windows timed, scaled to the shape,
    (c) the kernel alone, by HIP events through the engine's profiler: the rest of the call is the read-back of 48 bytes per window and the copy into the caller's array.
The call synchronises its stream, so it is timed by the host clock around the call.  DESIGN.md quotes the medians.

    python3 tools/time_snr_est.py [--rounds 5] [--reps 3] [--host_windows 240] [--out profiles/time_snr_est.json]
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
SHAPES = {"curves": (75, 60, 8), "large": (256, 4096, 8)}


def main():
    import stage_timing as stg
    import torch
    import snr_ref as sr
    from radae_amd.engine import BatchEngine, SnrParams, SnrSums, snr_sigma
    ap = stg.parser(rounds=5, reps=3)
    ap.add_argument("--host_windows", type=int, default=240)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sp = lambda: torch.cuda.current_stream().cuda_stream
    out = {"rounds": a.rounds, "reps": a.reps, "shapes": {}}
    for name, (B, Nt, Nw) in SHAPES.items():
        eng = BatchEngine(B, max_tx_mf=1)
        lib, h = eng.lib, eng.h
        g = torch.Generator(device=dev); g.manual_seed(1)
        H = torch.view_as_complex(torch.randn((B, Nt * Nw, 30, 2), generator=g, device=dev, dtype=torch.float32) * 0.70710678)
        Hc = torch.empty_like(H)
        nw = np.full(B, Nt, np.int32)
        sg = np.array([snr_sigma(-5 + b % 25) for b in range(B)], np.float32)
        res = np.zeros((B, Nt), np.dtype(SnrSums))
        p = SnrParams(Nw, 1, H.data_ptr(), Nt * Nw * 30, sg.ctypes.data, None, None, None, 0, 1)

        def call():
            assert lib.rade_batch_snr_trials(h, nw.ctypes.data, p, res.ctypes.data, Nt, sp()) == 0

        def kernels(fn, reps):
            eng.profile(True)
            for _ in range(reps):
                fn()
            eng.profile(False)
            got = eng.profile_get()["channel"]
            return got["ms"] / max(got["launches"], 1)

        calls = {"call": call, "kernel": call, "copy": lambda: Hc.copy_(H)}
        stg.warm(calls)
        t = stg.rounds(calls, a.rounds, a.reps, clocks={"call": stg.wall, "kernel": kernels})
        # (b) the float64 model on one host core, a stream of the script's size (60 windows) at a time, after one untimed pass; the same measurement scales to either shape
        hh = H[0, :60 * Nw].cpu().numpy()
        reps_h = max(-(-a.host_windows // 60), 1)
        for r in range(reps_h + 1):
            if r == 1:
                t0 = time.perf_counter()
            sr.trial_sums(hh, sr.gen_noise(1, r, 0, len(hh)), float(sg[0]), Nw)
        host_ms = 1e3 * (time.perf_counter() - t0) * (B * Nt) / (reps_h * 60)
        s = stg.stats(t)
        call_ms, k_ms, c_ms = (s[k]["median"] for k in ("call", "kernel", "copy"))
        out["shapes"][name] = {"streams": B, "windows": Nt, "rows": Nw, "ms_per_call": s, "h_bytes": 8 * B * Nt * Nw * 30, "sums_bytes": 48 * B * Nt,
                               "host_model_ms_scaled_to_the_shape": host_ms, "host_windows_timed": reps_h * 60, "call_over_copy": call_ms / c_ms,
                               "host_over_call": host_ms / call_ms, "share_behind_the_kernel": max(call_ms - k_ms, 0.0) / call_ms,
                               "windows_per_second": B * Nt / (call_ms * 1e-3), "first_S2_est": float(res[0, 0]["S2_est"])}
        eng.close()
    stg.emit(out, a.out)


if __name__ == "__main__":
    main()
