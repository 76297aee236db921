#!/usr/bin/env python3
"""Time of the spectrogram on the device (rade_batch_specgram: k_specgram once or twice, the read-back of the peaks) in alternating rounds in one process, at
256 streams x 80,000 samples (what process_rx looks at) and 256 x 806,400 (the benchmark's recording), with the image only (two passes: the transforms are computed
twice), the magnitudes only (one pass) and both (two passes), next to
    (a) the device's own complex64 copy of the same input bytes (HIP events),
    (b) the reference's algorithm, float64 numpy.fft.rfft per slice with the magnitudes, the maximum and the clips of plot_specgram.m, on one host core (--host_streams
        streams timed, scaled to the batch) plus the copy of the input across the host link.
The call synchronises its stream, so it is timed by the host clock around the call.  Per case: the slice pairs transformed per second and the float32 vector
instructions executed per second (OPS_PER_PAIR of them per 2048-point pair transform, counted from rade_spec.hip: five radix-4 stages of 512 butterflies with 16
additions and three 4-instruction products, the window, the radix-2 stage, the separation and the two magnitudes of 1023 bins).  DESIGN.md quotes the medians.

    python3 tools/time_specgram.py [--streams 256] [--rounds 5] [--reps 3] [--host_streams 2] [--shapes 80000,806400] [--out FILE.json]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS_PER_PAIR = 5 * 512 * (16 + 12) + 2 * 1280 + 1023 * 22


def main():
    import stage_timing as stg
    import torch
    from radae_amd.engine import BatchEngine, specgram_slices
    ap = stg.parser(rounds=5, reps=3)
    ap.add_argument("--shapes", type=str, default="80000,806400"); ap.add_argument("--host_streams", type=int, default=2)
    a = ap.parse_args()
    B = a.streams
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    out = {"streams": B, "rounds": a.rounds, "reps": a.reps, "ops_per_pair": OPS_PER_PAIR, "shapes": {}}
    for S in (int(v) for v in a.shapes.split(",")):
        g = torch.Generator(device=dev); g.manual_seed(1)
        x = torch.view_as_complex(torch.randn((B, S, 2), generator=g, device=dev, dtype=torch.float32) * 3000.0)
        y = torch.empty_like(x)
        ns = specgram_slices(S)
        pairs = B * ((ns + 1) // 2)
        last = {}

        def call(img, mag):
            def f():
                last[(img, mag)] = eng.specgram(x, img=img, mag=mag)[2]
            return f

        # the output tensors are allocated and cleared inside BatchEngine.specgram; that memset is part of what a Python caller pays, and is timed on its own
        calls = {"image": call(True, False), "magnitudes": call(False, True), "both": call(True, True), "peak_only": call(False, False), "copy": lambda: y.copy_(x),
                 "clear_image": lambda: torch.zeros((B, ns, 768), dtype=torch.uint8, device=dev), "clear_magnitudes": lambda: torch.zeros((B, ns, 1023), dtype=torch.float32, device=dev)}
        stg.warm(calls)
        clocks = {k: stg.wall for k in ("image", "magnitudes", "both", "peak_only")}
        t = stg.rounds(calls, a.rounds, a.reps, clocks=clocks)

        # (b) plot_specgram.m's arithmetic on one host core in float64, plus the input across the host link
        Bh = max(min(a.host_streams, B), 1)
        w = 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(1280) + 1) / 1281)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        xh = x[:Bh].cpu().numpy()
        for b in range(Bh):
            xr = xh[b].real.astype(np.float64)
            Sm = np.empty((ns, 1023))
            for s in range(ns):
                Sm[s] = np.abs(np.fft.rfft(xr[160 * s:160 * s + 1280] * w, 2048)[1:1024])
            Sm /= Sm.max()
            np.log(np.minimum(np.maximum(Sm, 10 ** -2.0), 10 ** -0.3))
        host_ms = 1e3 * (time.perf_counter() - t0) * B / Bh
        r = {"samples": S, "slices_per_stream": ns, "pairs_per_pass": pairs, "ms_per_call": stg.stats(t), "host_numpy_rfft_ms_scaled_to_the_batch": host_ms, "host_streams": Bh,
             "input_bytes": 8 * B * S, "image_bytes": B * ns * 768, "magnitude_bytes": 4 * B * ns * 1023}
        med = {k: r["ms_per_call"][k]["median"] for k in calls}
        passes = {"image": 2, "magnitudes": 1, "both": 2, "peak_only": 1}
        clear = {"image": med["clear_image"], "magnitudes": med["clear_magnitudes"], "both": med["clear_image"] + med["clear_magnitudes"], "peak_only": 0.0}
        r["derived"] = {k: {"passes": p, "ms_without_the_clearing_of_the_outputs": med[k] - clear[k], "pairs_per_s": p * pairs / ((med[k] - clear[k]) * 1e-3),
                            "vector_ops_per_s": p * pairs * OPS_PER_PAIR / ((med[k] - clear[k]) * 1e-3), "call_over_copy": med[k] / med["copy"], "host_over_call": host_ms / med[k]}
                        for k, p in passes.items()}
        r["spread"] = {k: (v["max"] - v["min"]) / v["median"] for k, v in r["ms_per_call"].items()}
        r["first_peak"] = float(last[(True, True)][0])
        out["shapes"][str(S)] = r
        del x, y
        torch.cuda.empty_cache()
    stg.emit(out, a.out)
    eng.close()


if __name__ == "__main__":
    main()
