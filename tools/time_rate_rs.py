#!/usr/bin/env python3
"""Time of the rate-Rs channel call (rade_batch_channel_rs_pa) next to the rate-Fs path it spares (rade_batch_tx_channel + rade_batch_rx_ideal) at the same
size, by HIP events, both in one process and in alternating rounds (DESIGN.md quotes the medians).  The rate-Fs pair includes the core encoder, so the encoder
alone is timed as well: rate Rs per utterance batch = encode + channel_rs_pa.

    python3 tools/time_rate_rs.py [--streams 256] [--n_mf 84] [--rounds 7] [--out FILE.json]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import stage_timing as stg
    import torch
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import BatchEngine, sigma_from_EbNodB
    ap = stg.parser(rounds=7)
    ap.add_argument("--n_mf", type=int, default=84)
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

    calls = {"rs": rs, "enc": enc, "fs": fs}
    stg.warm(calls, 3)
    t = stg.rounds(calls, a.rounds, {"rs": 200, "enc": 10, "fs": 10})
    res = {"streams": B, "latent_rows": rows, "rounds": a.rounds,
           "ms_per_call": stg.stats(t),
           "calls": {"rs": "rade_batch_channel_rs_pa, H given, Philox noise", "enc": "rade_batch_encode", "fs": "rade_batch_tx_channel (two-path G, Philox noise) + rade_batch_rx_ideal (no decoder)"},
           "algorithmic_flops_rs": 8.0 * B * 2 * rows * 2 * 20 * 160}
    res["rs_gflops_per_s"] = res["algorithmic_flops_rs"] / (res["ms_per_call"]["rs"]["median"] * 1e-3) / 1e9
    stg.emit(res, a.out)
    eng.close()


if __name__ == "__main__":
    main()
