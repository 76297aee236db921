#!/usr/bin/env python3
"""Time of the stored-file receiver past the acquisition on the device (rade_file.hip, rade_irx.hip), in alternating rounds in one process, at 256 streams x 80,000 and 256 x 806,400
samples:
    bpf_file    rade_batch_bpf_file (k_file_phase + k_file_bpf; the call synchronises: host clock) next to
                (a) the device's own complex64 copy of the same input bytes (HIP events; 16 bytes per sample, the filter's floor), and
                (b) radae_amd.acq.complex_bpf, the torch filter acquire() runs, on the same input (HIP events);
    rx_file     rade_batch_rx_file at S // 960 frames per stream, every stream mixed down by its own frequency: the demodulator alone and with the decoder, next to
                rade_batch_rx_ideal at the same frame count (freq_offset given, so that both correct a frequency);
    receive     radae_amd.acq.receive end to end (filter, detect, track, refine, plan, demodulate, decode) on a committed recording repeated to the length.
Per shape the medians, the filter's share of the copy's rate, and whether bpf_file's median beats the torch filter's by more than the 3 % by which rounds and boxes differ
(tools/ab_bench.py's rule).  DESIGN.md quotes the medians.

    python3 tools/time_rx_file.py [--streams 256] [--rounds 7] [--shapes 80000,806400] [--out profiles/time_rx_file.json]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import stage_timing as stg
    import torch
    from radae_amd import acq
    from radae_amd.engine import BatchEngine
    ap = stg.parser(rounds=7)
    ap.add_argument("--shapes", type=str, default="80000,806400")
    a = ap.parse_args()
    B = a.streams
    dev = torch.device("cuda", 0)
    shapes = [int(v) for v in a.shapes.split(",")]
    eng = BatchEngine(B, max_tx_mf=max(shapes) // 960)
    rec = np.load(os.path.join(REPO, "tests", "golden", "rxtrace_mpp.npz"))["rx_in"].astype(np.complex64)
    out = {"streams": B, "rounds": a.rounds, "shapes": {}}
    for S in shapes:
        g = torch.Generator(device=dev); g.manual_seed(1)
        x = torch.view_as_complex(torch.randn((B, S, 2), generator=g, device=dev, dtype=torch.float32) * 0.3)
        y, c = torch.empty_like(x), torch.empty_like(x)
        xr = torch.tensor(np.tile(rec, S // len(rec) + 1)[:S], device=dev).repeat(B, 1)
        n_mf = S // 960
        plans = [(0, n_mf, 1.0 + 0.01 * b) for b in range(B)]
        fo = np.array([p[2] for p in plans], np.float32)
        last = {}

        def receive():
            last["rx"] = acq.receive(eng, xr)

        calls = {"bpf_file": lambda: eng.bpf_file(x, out=y), "copy": lambda: c.copy_(x), "torch_bpf": lambda: acq.complex_bpf(x),
                 "rx_file_demod": lambda: eng.rx_file(x, plans, feat_width=0), "rx_ideal_demod": lambda: eng.rx_ideal(x, n_mf, freq_offset=fo, feat_width=0),
                 "rx_file": lambda: eng.rx_file(x, plans), "rx_ideal": lambda: eng.rx_ideal(x, n_mf, freq_offset=fo), "receive": receive}
        wall = {k: stg.wall for k in ("bpf_file", "rx_file_demod", "rx_file", "receive")}
        stg.warm(calls, 1)
        t = stg.rounds(calls, a.rounds, 1, clocks=wall)
        r = {"samples": S, "frames_per_stream": n_mf, "ms_per_call": stg.stats(t), "input_bytes": 8 * B * S,
             "receive_frames_decoded": int(sum(v.plan.n_mf for v in last["rx"])), "receive_acquired": int(sum(v.plan.status == 0 for v in last["rx"]))}
        med = {k: r["ms_per_call"][k]["median"] for k in calls}
        r["derived"] = {"bpf_file_over_copy": med["bpf_file"] / med["copy"], "torch_bpf_over_bpf_file": med["torch_bpf"] / med["bpf_file"],
                        "bpf_file_GB_per_s": 16e-9 * B * S / (med["bpf_file"] * 1e-3),
                        "bpf_file_faster_than_torch_bpf_by_more_than_3_percent": bool(med["bpf_file"] < 0.97 * med["torch_bpf"]),
                        "rx_file_demod_over_rx_ideal_demod": med["rx_file_demod"] / med["rx_ideal_demod"], "rx_file_over_rx_ideal": med["rx_file"] / med["rx_ideal"]}
        r["spread"] = {k: (v["max"] - v["min"]) / v["median"] for k, v in r["ms_per_call"].items()}
        out["shapes"][str(S)] = r
        del x, y, c, xr
        torch.cuda.empty_cache()
    stg.emit(out, a.out)
    eng.close()


if __name__ == "__main__":
    main()
