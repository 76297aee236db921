"""What the tools/time_*.py scripts share: the common arguments, the warm-up of every timed shape, alternating rounds in one process, the two clocks, the statistics and
the JSON line.  A script keeps its cases and byte counts, its host-path comparison and its derived ratios."""
import argparse
import json
import os
import time

import numpy as np

HBM_TB_S = 6.3          # what a float4 copy achieves on an MI355X (8.0 is the data sheet's figure)


def parser(rounds: int, reps=None, streams: int = 256):
    """--streams, --rounds, --reps (not offered when the script fixes the repetitions of its cases) and --out; the script adds its own"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=streams); ap.add_argument("--rounds", type=int, default=rounds)
    if reps is not None:
        ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--out", type=str, default="")
    return ap


def timed(fn, reps: int) -> float:
    """ms per call by HIP events around `reps` calls back to back"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(fn, reps: int) -> float:
    """ms per call by the host clock, for a call that synchronises its stream"""
    import torch
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def warm(calls, n: int = 2):
    """every shape of the timed windows, code objects loaded"""
    for fn in calls.values():
        for _ in range(n):
            fn()


def rounds(calls, n_rounds: int, reps, clocks=None):
    """Alternating rounds: every case once per round, in the order of `calls`.  reps: one number or {case: reps}; clocks: {case: clock(fn, reps)} for the cases not
    timed by HIP events.  Returns {case: [ms per call of each round]}."""
    import torch
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(n_rounds):
        for k, fn in calls.items():
            t[k].append((clocks or {}).get(k, timed)(fn, reps[k] if isinstance(reps, dict) else reps))
    return t


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def stats(t):
    return {k: stat(v) for k, v in t.items()}


def emit(res, out: str):
    """the one JSON line, printed and (--out) written"""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(line + "\n")
