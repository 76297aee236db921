#!/usr/bin/env python3
"""Time of the whole-file pilot search on the device (rade_batch_acq_detect: k_acq_detect, k_acq_combine, the read-back of the hop records) in alternating rounds in one
process, at 256 streams x 80,000 and 256 x 806,400 noise-only samples, next to
    (a) the device's own complex64 copy of the same input bytes (HIP events),
    (b) float32 detect_pilots as the reference computes it (a matmul per timing; oracle/golden/acquisition.py's loop) on one host core (--host_hops hops timed, scaled to the
        batch) plus the copy of the input across the host link,
    (c) rade_batch_rx over the same noise-only streams: the streaming receiver stays in search and runs the same correlation once per modem frame, serially per stream
        inside its 256-thread workgroup (its input band-pass included: it cannot be switched off).
The calls synchronise their stream, so they are timed by the host clock around the call.  Per shape: the matrix instructions per second and their share of the
v_mfma_f32_16x16x32_f16 rate (MFMA_PER_TILE = 85 per tile of 16 timings and block, the two-stage form; 16 x 16 x 32 x 2 flop each), and acq_detect against rade_batch_rx: the medians, their
ratio, and whether the difference exceeds the 3 % by which rounds and boxes differ (tools/ab_bench.py's rule).  DESIGN.md quotes the medians.

    python3 tools/time_acq.py [--streams 256] [--rounds 10] [--host_hops 2] [--shapes 80000,806400] [--out profiles/time_acq.json]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_PER_TILE = 85
MFMA_PEAK_PER_S = 2.5e15 / (16 * 16 * 32 * 2)          # the data sheet's dense binary16 rate in instructions


def main():
    import stage_timing as stg
    import torch
    from radae_amd.engine import BatchEngine
    from radae_amd.stages import acq_hops, acq_track
    ap = stg.parser(rounds=10)
    ap.add_argument("--shapes", type=str, default="80000,806400"); ap.add_argument("--host_hops", type=int, default=2)
    a = ap.parse_args()
    B = a.streams
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    p_w = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "consts.npz"))["acq_p_w"]
    out = {"streams": B, "rounds": a.rounds, "mfma_per_tile": MFMA_PER_TILE, "shapes": {}}
    for S in (int(v) for v in a.shapes.split(",")):
        g = torch.Generator(device=dev); g.manual_seed(1)
        x = torch.view_as_complex(torch.randn((B, S, 2), generator=g, device=dev, dtype=torch.float32) * 0.3)
        y = torch.empty_like(x)
        H = acq_hops(S)
        last = {}

        def detect():
            last["hops"] = eng.acq_detect(x)

        def receive():
            eng.rx_reset()
            last["rx"] = eng.rx(x)[1]

        calls = {"acq_detect": detect, "rade_batch_rx": receive, "copy": lambda: y.copy_(x)}
        stg.warm(calls, 1)
        t = stg.rounds(calls, a.rounds, 1, clocks={"acq_detect": stg.wall, "rade_batch_rx": stg.wall})
        # noise only: single candidate hops are expected at this many hops (Pacq_error1 = 1e-5 per hop), acquisitions (four in a row at one timing) are not
        hops, nh = last["hops"]
        noise = {"candidate_hops": int(hops["candidate"].sum()), "acq_events": sum(len(acq_track(hops[b, :nh[b]], True)[0]) for b in range(B)),
                 "rx_valid_frames": sum(s.n_valid for s in last["rx"])}

        # (b) float32 detect_pilots on one host core, plus the input across the host link
        torch.cuda.synchronize(); t0 = time.perf_counter()
        xh = x[:1].cpu().numpy()[0]
        link_ms = 1e3 * (time.perf_counter() - t0) * B
        t0 = time.perf_counter()
        for k in range(a.host_hops):
            rx = np.conj(xh[960 * k:960 * k + 2112])
            Dt1, Dt2 = np.zeros((960, 40), np.csingle), np.zeros((960, 40), np.csingle)
            best = 0.0
            for tt in range(960):
                Dt1[tt], Dt2[tt] = np.matmul(rx[tt:tt + 160], p_w), np.matmul(rx[tt + 960:tt + 1120], p_w)
                best = max(best, np.max(np.abs(Dt1[tt]) + np.abs(Dt2[tt])))
            np.mean(np.abs(Dt1)) + np.mean(np.abs(Dt2))
        host_ms = 1e3 * (time.perf_counter() - t0) / a.host_hops * H * B
        r = {"samples": S, "hops_per_stream": H, "ms_per_call": stg.stats(t), "host_detect_pilots_ms_scaled_to_the_batch": host_ms, "host_link_ms_scaled_to_the_batch": link_ms,
             "input_bytes": 8 * B * S, "noise_only": noise}
        med = {k: r["ms_per_call"][k]["median"] for k in calls}
        mfma = B * (H + 1) * 60 * MFMA_PER_TILE
        r["derived"] = {"mfma_per_s": mfma / (med["acq_detect"] * 1e-3), "share_of_the_f16_matrix_rate": mfma / (med["acq_detect"] * 1e-3) / MFMA_PEAK_PER_S,
                        "call_over_copy": med["acq_detect"] / med["copy"], "host_over_call": (host_ms + link_ms) / med["acq_detect"],
                        "rx_over_acq_detect": med["rade_batch_rx"] / med["acq_detect"],
                        "faster_than_rade_batch_rx_by_more_than_3_percent": bool(med["acq_detect"] < 0.97 * med["rade_batch_rx"])}
        r["spread"] = {k: (v["max"] - v["min"]) / v["median"] for k, v in r["ms_per_call"].items()}
        out["shapes"][str(S)] = r
        del x, y
        torch.cuda.empty_cache()
    stg.emit(out, a.out)
    eng.close()


if __name__ == "__main__":
    main()
