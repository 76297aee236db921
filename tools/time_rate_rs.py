#!/usr/bin/env python3
"""Time of the rate-Rs channel call (rade_batch_channel_rs_pa) next to the rate-Fs path it spares (rade_batch_tx_channel + rade_batch_rx_ideal) at the same
size, by HIP events, both in one process and in alternating rounds (DESIGN.md quotes the medians).  The rate-Fs pair includes the core encoder, so the encoder
alone is timed as well: rate Rs per utterance batch = encode + channel_rs_pa.

    python3 tools/time_rate_rs.py [--streams 256] [--n_mf 84] [--rounds 7] [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import BatchEngine, sigma_from_EbNodB
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256); ap.add_argument("--n_mf", type=int, default=84); ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    B, n_mf = a.streams, a.n_mf
    rows = 3 * n_mf
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=n_mf)
    feats = torch.tensor(np.stack([synth_features(100 + b % 8, 12 * n_mf) for b in range(B)]), device=dev)
    f84 = feats[:, :, :21].clone(); f84[:, :, 20] = -1.0
    f84 = f84.reshape(B, rows, 84).contiguous()
    rng = np.random.default_rng(1)
    H = torch.tensor(np.abs(rng.standard_normal((B, 2 * rows, 20)) + 1j * rng.standard_normal((B, 2 * rows, 20))).astype(np.float32) / np.float32(np.sqrt(2)), device=dev)
    G = eng.multipath_gen("mpp", n_mf * 960, seed=3)
    s_rs, s_fs = sigma_from_EbNodB(3.0, rate_Fs=False), sigma_from_EbNodB(3.0)
    z = eng.encode(f84)

    def rs():
        eng.channel_rs_pa(z, s_rs, H=H, seed=7)

    def enc():
        eng.encode(f84)

    def fs():
        rx = eng.tx_channel(feats, s_fs, 0.0, G=G, seed=7)
        eng.rx_ideal(rx, n_mf, feat_width=0)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / n

    for fn in (rs, enc, fs):                                  # every shape of the timed windows, code objects loaded
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"rs": [], "enc": [], "fs": []}
    for _ in range(a.rounds):
        t["rs"].append(timed(rs, 200)); t["enc"].append(timed(enc, 10)); t["fs"].append(timed(fs, 10))
    res = {"streams": B, "latent_rows": rows, "rounds": a.rounds,
           "ms_per_call": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in t.items()},
           "calls": {"rs": "rade_batch_channel_rs_pa, H given, Philox noise", "enc": "rade_batch_encode", "fs": "rade_batch_tx_channel (two-path G, Philox noise) + rade_batch_rx_ideal (no decoder)"},
           "algorithmic_flops_rs": 8.0 * B * 2 * rows * 2 * 20 * 160}
    res["rs_gflops_per_s"] = res["algorithmic_flops_rs"] / (res["ms_per_call"]["rs"]["median"] * 1e-3) / 1e9
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
