#!/usr/bin/env python3
"""Time of the sound-card wire on the device (rade_batch_wire_in / rade_batch_wire_out: k_wire_in, k_wire_out, k_wire_meters) by HIP events, every mode, with and
without meters, in alternating rounds in one process -- next to the path the calls replace at the same commit: radae_amd/wire.py on a host core plus the copy of the
complex64 samples across the host link (receive side: convert, then copy to the device; transmit side: copy to the host, then convert), timed by the host clock around
work that ends in a synchronise.  Bytes are what the algorithm has to move per sample: real in 2 read + 8 written, IQ in 4 + 8, real out 8 read (the lines that hold
I also hold Q) + 2 written, IQ out 8 + 4.  DESIGN.md quotes the medians.

    python3 tools/time_wire.py [--streams 256] [--samples 806400] [--rounds 10] [--reps 5] [--host_reps 2] [--out FILE.json]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import stage_timing as stg
    import torch
    from radae_amd import wire
    from radae_amd.engine import BatchEngine
    ap = stg.parser(rounds=10, reps=5)
    ap.add_argument("--samples", type=int, default=806400); ap.add_argument("--host_reps", type=int, default=2)
    a = ap.parse_args()
    B, N = a.streams, a.samples
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    L, h = eng.lib, eng.h
    g = torch.Generator(device=dev); g.manual_seed(1)
    i16 = torch.randint(-32768, 32768, (B, N, 2), generator=g, device=dev, dtype=torch.int32).to(torch.int16)      # real mode reads the first N of each row
    x = torch.view_as_complex(torch.randn((B, N, 2), generator=g, device=dev, dtype=torch.float32) * 1.2)          # at scale 8192 a few samples in a thousand clip
    c64 = torch.empty((B, N), dtype=torch.complex64, device=dev)
    o16 = torch.empty((B, N, 2), dtype=torch.int16, device=dev)
    n = np.full(B, N, np.int32)
    meters = np.zeros((B, 4), np.float64)
    sp = lambda: torch.cuda.current_stream().cuda_stream

    def w_in(mode):
        assert L.rade_batch_wire_in(h, i16.data_ptr(), 2 * N, n.ctypes.data, mode, 1.0, c64.data_ptr(), N, sp()) == 0

    def w_out(mode, m):
        assert L.rade_batch_wire_out(h, x.data_ptr(), N, n.ctypes.data, mode, 8192.0, o16.data_ptr(), 2 * N, meters.ctypes.data if m else None, sp()) == 0

    def copy():                                                # the device's own copy of the complex64 rows: 8 read + 8 written per sample
        c64.copy_(x)
    calls = {"in_real": lambda: w_in(0), "in_iq": lambda: w_in(1), "out_real": lambda: w_out(0, False), "out_iq": lambda: w_out(1, False),
             "out_real_meters": lambda: w_out(0, True), "out_iq_meters": lambda: w_out(1, True), "copy_c64": copy}
    by = {"in_real": 10.0, "in_iq": 12.0, "out_real": 10.0, "out_iq": 12.0, "out_real_meters": 10.0, "out_iq_meters": 12.0, "copy_c64": 16.0}

    stg.warm(calls)
    t = stg.rounds(calls, a.rounds, a.reps)

    # the host path at the same commit (one core, as a service's feeding thread has it)
    s_host = i16.cpu().numpy()
    th = {"host_in_real": [], "host_in_iq": [], "host_out_real": [], "host_out_iq": []}
    for _ in range(a.host_reps):
        for mode, key in ((0, "host_in_real"), (1, "host_in_iq")):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            raw = np.ascontiguousarray(s_host[:, :, 0] if mode == 0 else s_host).tobytes()
            f = np.frombuffer(wire.int16_to_f32(raw, zeropad=mode == 0), np.complex64).reshape(B, N)
            c64.copy_(torch.from_numpy(f)); torch.cuda.synchronize()
            th[key].append(1e3 * (time.perf_counter() - t0))
        for mode, key in ((0, "host_out_real"), (1, "host_out_iq")):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            wire.f32_to_int16(x.cpu().numpy().tobytes(), 8192.0, real=mode == 0)
            th[key].append(1e3 * (time.perf_counter() - t0))
    del s_host
    res = {"streams": B, "samples": N, "rounds": a.rounds, "reps": a.reps, "host_reps": a.host_reps,
           "ms_per_call": stg.stats(t), "host_ms_per_call": stg.stats(th),
           "algorithmic_bytes_per_sample": by}
    res["TB_per_s"] = {k: by[k] * B * N / (res["ms_per_call"][k]["median"] * 1e-3) / 1e12 for k in by}
    res["share_of_measured_hbm_copy_rate"] = {k: v / stg.HBM_TB_S for k, v in res["TB_per_s"].items()}
    res["host_over_device"] = {k: res["host_ms_per_call"]["host_" + k]["median"] / res["ms_per_call"][k]["median"] for k in ("in_real", "in_iq", "out_real", "out_iq")}
    stg.emit(res, a.out)
    eng.close()


if __name__ == "__main__":
    main()
