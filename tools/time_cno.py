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
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import stage_timing as stg
    import torch
    from radae_amd.engine import BatchEngine, CnoParams, CnoResult, cno_plan, cno_windows
    ap = stg.parser(rounds=5, reps=3)
    ap.add_argument("--samples", type=int, default=80000); ap.add_argument("--host_streams", type=int, default=4)
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

    def kernels(fn, reps):
        """the two launches alone, by the engine's HIP-event profiler (class `channel`)"""
        eng.profile(True)
        for _ in range(reps):
            fn()
        eng.profile(False)
        got = eng.profile_get()["channel"]
        return got["ms"] / max(got["launches"], 1)

    calls = {"call": call, "kernels": call, "copy": lambda: y.copy_(x)}
    stg.warm(calls)
    t = stg.rounds(calls, a.rounds, a.reps, clocks={"call": stg.wall, "kernels": kernels})      # the call synchronises its stream: the host clock

    # (b) the reference's algorithm on one host core: np.fft.fft of every window in float64 (est_CNo.py:31-45), plus the input across the host link
    Bh = max(min(a.host_streams, B), 1)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    xh = x[:Bh].cpu().numpy()
    for b in range(Bh):
        for st in np.arange(0, S - q.N, 2000):
            Rx = np.abs(np.fft.fft(xh[b, st:st + q.N])) ** 2
            np.sum(Rx[q.flow_bin:q.fhigh_bin]); np.sum(Rx[q.noise_st:q.noise_en])
    host_ms = 1e3 * (time.perf_counter() - t0) * B / Bh
    out = {"streams": B, "samples": S, "windows_per_stream": n_win, "N": q.N, "J": q.J, "rounds": a.rounds, "reps": a.reps, "host_streams": Bh,
           "ms_per_call": stg.stats(t), "host_numpy_fft_ms_scaled_to_the_batch": host_ms, "input_bytes": 8 * B * S}
    call_ms, k_ms, c_ms = (out["ms_per_call"][k]["median"] for k in ("call", "kernels", "copy"))
    out["call_over_copy"] = call_ms / c_ms
    out["host_over_call"] = host_ms / call_ms
    out["share_behind_the_kernels"] = max(call_ms - k_ms, 0.0) / call_ms
    out["first_result"] = {"max_st": int(res[0].max_st), "max_CNodB": float(res[0].max_CNodB)}
    stg.emit(out, a.out)
    eng.close()


if __name__ == "__main__":
    main()
