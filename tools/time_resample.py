#!/usr/bin/env python3
"""Time of the fractional resampler (rade_batch_resample) in both modes next to the rate-Fs channel call (rade_batch_channel: k_chan_power + k_chan_gain +
k_chan_apply, no multipath, no noise: its bandwidth-bound form) at the same size, by HIP events, all in one process and in alternating rounds (DESIGN.md quotes the
medians).  Bytes are what the algorithm has to move: 8 read + 8 written per output sample for the resampler; 8 read by the power pass, 8 read + 8 written by the
apply pass for the channel.  Operations of the sinc32 mode: 64 fused multiply-adds for the coefficients + 64 for the products per output.

    python3 tools/time_resample.py [--streams 256] [--samples 806400] [--ppm -2493.77] [--rounds 7] [--out FILE.json]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import stage_timing as stg
    import torch
    from radae_amd.engine import BatchEngine, resample_count
    ap = stg.parser(rounds=7, reps=10)
    ap.add_argument("--samples", type=int, default=806400); ap.add_argument("--ppm", type=float, default=-2493.77)
    a = ap.parse_args()
    B, N = a.streams, a.samples
    assert N % 960 == 0, "the channel call takes whole modem frames"
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    g = torch.Generator(device=dev); g.manual_seed(1)
    x = torch.view_as_complex(torch.randn((B, N, 2), generator=g, device=dev, dtype=torch.float32))
    n_out = resample_count(N, 0.0, a.ppm)
    y = torch.empty((B, n_out), dtype=torch.complex64, device=dev)

    def sinc():
        eng.resample(x, a.ppm, 0.0, "sinc32", n_out=n_out, out=y)

    def lin():
        eng.resample(x, a.ppm, 0.0, "linear", n_out=n_out, out=y)

    def chan():
        eng.channel(x, 0.0, 0.0, seed=0)

    calls = {"sinc32": sinc, "linear": lin, "channel": chan}
    stg.warm(calls)
    t = stg.rounds(calls, a.rounds, a.reps)
    by = {"sinc32": 16.0 * B * n_out, "linear": 16.0 * B * n_out, "channel": 24.0 * B * N}
    res = {"streams": B, "samples_in": N, "samples_out": n_out, "ppm": a.ppm, "rounds": a.rounds, "reps": a.reps,
           "ms_per_call": stg.stats(t),
           "algorithmic_bytes": by, "algorithmic_flops_sinc32": 2.0 * 128 * B * n_out,
           "calls": {"sinc32": "rade_batch_resample, RADE_RESAMPLE_SINC32", "linear": "rade_batch_resample, RADE_RESAMPLE_LINEAR",
                     "channel": "rade_batch_channel without G, sigma 0, seed 0 (k_chan_power + k_chan_gain + k_chan_apply)"}}
    res["TB_per_s"] = {k: by[k] / (res["ms_per_call"][k]["median"] * 1e-3) / 1e12 for k in by}
    res["sinc32_TFLOP_per_s"] = res["algorithmic_flops_sinc32"] / (res["ms_per_call"]["sinc32"]["median"] * 1e-3) / 1e12
    stg.emit(res, a.out)
    eng.close()


if __name__ == "__main__":
    main()
