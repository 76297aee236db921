#!/usr/bin/env python3
"""Time of the Welch periodogram and of the power / peak sums on the device (rade_batch_psd: k_psd and k_psd_fold; rade_batch_sigstat: k_sigstat, its fold and the
read-back) in alternating rounds in one process, at 256 streams x 80,000 complex64 samples and 256 x 806,400 (the benchmark's recording), win = 1024, step = 512,
next to
    (a) the device's own complex64 copy of the same input bytes (HIP events),
    (b) the host path there was before: scipy.signal.welch plus numpy's mean and maximum of |x|^2 on one host core (--host_streams streams timed, scaled to the
        batch) plus the copy of the input across the host link.
Both calls synchronise their stream, so they are timed by the host clock around the call.  Per shape: the 1024-point transforms per second.  DESIGN.md quotes the medians.

    python3 tools/time_psd.py [--streams 256] [--rounds 5] [--reps 3] [--host_streams 2] [--shapes 80000,806400] [--win 1024] [--step 512] [--out FILE.json]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import stage_timing as stg
    import torch
    from radae_amd.engine import BatchEngine, psd_segments
    ap = stg.parser(rounds=5, reps=3)
    ap.add_argument("--shapes", type=str, default="80000,806400"); ap.add_argument("--host_streams", type=int, default=2)
    ap.add_argument("--win", type=int, default=1024); ap.add_argument("--step", type=int, default=512)
    a = ap.parse_args()
    B = a.streams
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    out = {"streams": B, "rounds": a.rounds, "reps": a.reps, "win": a.win, "step": a.step, "shapes": {}}
    for S in (int(v) for v in a.shapes.split(",")):
        g = torch.Generator(device=dev); g.manual_seed(1)
        x = torch.view_as_complex(torch.randn((B, S, 2), generator=g, device=dev, dtype=torch.float32))
        y = torch.empty_like(x)
        ns = psd_segments(S, a.win, a.step)
        last = {}

        def psd():
            last["psd"] = eng.psd(x, win=a.win, step=a.step)[0]

        def sigstat():
            last["stat"] = eng.sigstat(x)

        calls = {"psd": psd, "sigstat": sigstat, "copy": lambda: y.copy_(x)}
        stg.warm(calls)
        t = stg.rounds(calls, a.rounds, a.reps, clocks={"psd": stg.wall, "sigstat": stg.wall})

        # (b) the host path: the input across the host link, scipy.signal.welch and numpy's power and peak on one core, in float64 as the script computes
        from scipy import signal
        Bh = max(min(a.host_streams, B), 1)
        w = signal.windows.hamming(a.win, sym=True)
        signal.welch(np.ones(2 * a.win, np.complex128), fs=8000, window=w, nperseg=a.win, noverlap=a.win - a.step, nfft=1024, detrend=False, return_onesided=False)   # scipy's first call loads its transforms: not timed
        np.abs(x[:1, :a.win].cpu().numpy().astype(np.complex128)) ** 2                 # ... nor the process's first copy across the host link
        host_runs = []
        for _ in range(2):                                                             # the faster of two runs: the first still pays what a process pays once
            torch.cuda.synchronize(); t0 = time.perf_counter()
            xh = x[:Bh].cpu().numpy()
            for b in range(Bh):
                xd = xh[b].astype(np.complex128)
                signal.welch(xd, fs=8000, window=w, nperseg=a.win, noverlap=a.win - a.step, nfft=1024, detrend=False, return_onesided=False, scaling="density")
                p = np.abs(xd) ** 2
                p.mean(), p.max(), p[:160].mean(), p[:160].max()
            host_runs.append(1e3 * (time.perf_counter() - t0) * B / Bh)
        host_ms = min(host_runs)
        r = {"samples": S, "segments_per_stream": ns, "transforms": B * ns, "ms_per_call": stg.stats(t), "host_scipy_welch_and_numpy_ms_scaled_to_the_batch": host_ms,
             "host_runs_ms_scaled_to_the_batch": host_runs, "host_streams": Bh, "input_bytes": 8 * B * S}
        med = {k: r["ms_per_call"][k]["median"] for k in calls}
        r["derived"] = {"transforms_per_s": B * ns / (med["psd"] * 1e-3), "psd_over_copy": med["psd"] / med["copy"], "sigstat_over_copy": med["sigstat"] / med["copy"],
                        "host_over_psd_plus_sigstat": host_ms / (med["psd"] + med["sigstat"])}
        r["spread"] = {k: (v["max"] - v["min"]) / v["median"] for k, v in r["ms_per_call"].items()}
        r["first_bin"] = float(last["psd"][0, 0]); r["first_Pav"] = float(last["stat"].Pav[0])
        out["shapes"][str(S)] = r
        del x, y
        torch.cuda.empty_cache()
    stg.emit(out, a.out)
    eng.close()


if __name__ == "__main__":
    main()
