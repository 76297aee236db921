#!/usr/bin/env python3
"""Time of the rational rate converter on the device (rade_batch_rate_convert: k_rate_convert) by HIP events, in alternating rounds in one process: 48 kHz int16 real
-> 8 kHz, 48 kHz complex64 -> 8 kHz, 8 kHz -> 48 kHz and 44.1 kHz -> 8 kHz (complex64), each next to the device's own complex64 copy of the same number of bytes, and
next to the path the call replaces: scipy.signal.resample_poly with the same prototype (the library's table laid out at the rate L Fin) on one host core plus the copy
of the result (or of the input, when up-sampling) across the host link, timed by the host clock on --host_streams streams and scaled to the batch.  Bytes are what the
algorithm has to move: every input sample read once, every output sample written once.  DESIGN.md quotes the medians.

    python3 tools/time_rate.py [--streams 256] [--seconds 10] [--rounds 5] [--reps 3] [--host_streams 8] [--out FILE.json]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def prototype(C):
    """the [L][T] table as one filter at the rate L Fin, in the order scipy's upfirdn applies it (include/rade_batch.h: t_j = j - (T / 2 - 1) - ph / L)"""
    L, T = C.shape
    p = np.zeros(L * T)
    for ph in range(L):
        p[np.arange(T) * L - ph + (L - 1)] = C[ph]
    return p[::-1].copy()


def main():
    import stage_timing as stg
    import torch
    from radae_amd.engine import BatchEngine, RateParams, rate_count, rate_taps
    ap = stg.parser(rounds=5, reps=3)
    ap.add_argument("--seconds", type=int, default=10); ap.add_argument("--host_streams", type=int, default=8)
    a = ap.parse_args()
    B, S = a.streams, a.seconds
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    lib, h = eng.lib, eng.h
    g = torch.Generator(device=dev); g.manual_seed(1)
    n48, n44, n8 = 48000 * S, 44100 * S, 8000 * S
    i16 = torch.randint(-32768, 32768, (B, n48), generator=g, device=dev, dtype=torch.int32).to(torch.int16)
    big = torch.view_as_complex(torch.randn((B, n48, 2), generator=g, device=dev, dtype=torch.float32))           # 48 kHz (and, its first samples, 44.1 kHz) input; 48 kHz output
    small = torch.view_as_complex(torch.randn((B, n8, 2), generator=g, device=dev, dtype=torch.float32))          # 8 kHz input
    y8 = torch.empty((B, n8), dtype=torch.complex64, device=dev)
    y48 = torch.empty((B, n48), dtype=torch.complex64, device=dev)
    sp = lambda: torch.cuda.current_stream().cuda_stream
    keep = []

    def conv(x, x_stride, n_in, fmt, y, y_stride, L, M):
        n_i = np.full(B, n_in, np.int32); n_o = np.full(B, rate_count(n_in, L, M), np.int32); p = RateParams(L, M, None, None)
        keep.extend([n_i, n_o, p])
        return lambda: lib.rade_batch_rate_convert(h, x.data_ptr(), x_stride, n_i.ctypes.data, fmt, 1.0 / 8192, y.data_ptr(), y_stride, n_o.ctypes.data, p, sp())

    # name: (call, bytes per stream, (L, M), input samples per stream)
    cases = {"s16_48k_to_8k": (conv(i16, n48, n48, 1, y8, n8, 1, 6), 2 * n48 + 8 * n8, (1, 6), n48),
             "c64_48k_to_8k": (conv(big, n48, n48, 0, y8, n8, 1, 6), 8 * n48 + 8 * n8, (1, 6), n48),
             "c64_8k_to_48k": (conv(small, n8, n8, 0, y48, n48, 6, 1), 8 * n8 + 8 * n48, (6, 1), n8),
             "c64_44k1_to_8k": (conv(big, n48, n44, 0, y8, n8, 80, 441), 8 * n44 + 8 * n8, (80, 441), n44)}
    calls, by = {}, {}
    flat_src, flat_dst = big.view(-1), y48.view(-1)
    for k, (fn, nbytes, _, _) in cases.items():
        def checked(fn=fn):
            assert fn() == 0
        calls[k], by[k] = checked, float(nbytes)
        n_copy = B * nbytes // 16                                  # the device's copy of as many bytes: 8 read + 8 written per complex64 sample
        calls["copy_" + k], by["copy_" + k] = (lambda n=n_copy: flat_dst[:n].copy_(flat_src[:n])), 16.0 * n_copy / B

    stg.warm(calls)
    t = stg.rounds(calls, a.rounds, a.reps)

    # the host path: scipy's polyphase filter on one core with the same prototype, and the copy across the host link (the smaller side of the conversion stays on the
    # host side of the link: the 8 kHz result of a down-conversion goes up, the 48 kHz result of an up-conversion goes up)
    th = {}
    try:
        from scipy import signal
    except ImportError:
        signal = None
    Bh = min(a.host_streams, B)
    if signal is not None and Bh > 0:
        srcs = {"s16_48k_to_8k": i16[:Bh].cpu().numpy(), "c64_48k_to_8k": big[:Bh].cpu().numpy(), "c64_8k_to_48k": small[:Bh].cpu().numpy(),
                "c64_44k1_to_8k": big[:Bh, :n44].cpu().numpy()}
        for k, (_, _, (L, M), n_in) in cases.items():
            hproto = prototype(rate_taps(L, M).astype(np.float64))
            x = srcs[k]
            dst = y8 if M > L else y48
            torch.cuda.synchronize(); t0 = time.perf_counter()
            xin = (x.astype(np.float32) * np.float32(1.0 / 8192)) if x.dtype == np.int16 else x
            out = signal.upfirdn(hproto, xin, up=L, down=M, axis=1).astype(np.complex64)
            n_o = min(out.shape[1], dst.shape[1])
            dst[:Bh, :n_o].copy_(torch.from_numpy(np.ascontiguousarray(out[:, :n_o]))); torch.cuda.synchronize()
            th[k] = 1e3 * (time.perf_counter() - t0) * B / Bh
    res = {"streams": B, "seconds": S, "rounds": a.rounds, "reps": a.reps, "host_streams": Bh,
           "ms_per_call": stg.stats(t), "host_ms_per_call_scaled_to_the_batch": th,
           "algorithmic_bytes_per_stream": by}
    res["TB_per_s"] = {k: by[k] * B / (res["ms_per_call"][k]["median"] * 1e-3) / 1e12 for k in by}
    res["share_of_measured_hbm_copy_rate"] = {k: v / stg.HBM_TB_S for k, v in res["TB_per_s"].items()}
    res["copy_over_call"] = {k: res["ms_per_call"]["copy_" + k]["median"] / res["ms_per_call"][k]["median"] for k in cases}
    res["host_over_device"] = {k: th[k] / res["ms_per_call"][k]["median"] for k in th}
    res["x_real_time"] = {k: 1e3 * B * S / res["ms_per_call"][k]["median"] for k in cases}
    stg.emit(res, a.out)
    eng.close()


if __name__ == "__main__":
    main()
