#!/usr/bin/env python3
"""Time of the channel in pieces (rade_batch_channel_piece: k_chan_piece; rade_batch_multipath_piece: k_dopp_piece) next to the whole-utterance calls it stands beside
(rade_batch_channel: k_chan_power, k_chan_gain, k_chan_apply; rade_batch_multipath_gen), on the same total: --streams streams x --samples samples, pushed as pieces of
--piece.  Cases, each the whole total once:
    whole_awgn        rade_batch_channel, generated noise, 3 dB, +8 Hz          piece_awgn        the same through rade_batch_channel_piece
    whole_mpp         rade_batch_channel with G (mpp) resident                   piece_mpp         rade_batch_channel_piece with the piece's G resident
    whole_mpp_gen     rade_batch_multipath_gen of the whole G                    piece_mpp_gen     rade_batch_multipath_piece of every piece's G (16 samples of overlap)
    copy              the device's own copy of the output bytes (8 read + 8 written per sample): the floor
Clock: the host's, around the calls and a device synchronise (the piece calls wait once ahead of their launches for the copy of their per-stream records, and
rade_batch_multipath_gen waits for its kernel), in alternating rounds in one process.  g_share = 1 - piece_awgn / piece_mpp: the share of the two-path piece call's time
that the Doppler pairs cost (16 bytes read per sample on top of 8 read and 8 written, and two complex products) -- what generating G inside k_chan_piece could save.
DESIGN.md quotes the medians.

    python3 tools/time_chan_piece.py [--streams 256] [--samples 806400] [--piece 96000] [--rounds 5] [--out profiles/time_chan_piece.json]
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    import torch
    import stage_timing as stg
    from radae_amd.abi import ChannelParams, ChannelPieceParams
    from radae_amd.channel_tools import PRESETS, doppler_plan
    from radae_amd.engine import BatchEngine, multipath_gain, sigma_from_EbNodB
    ap = stg.parser(rounds=5)
    ap.add_argument("--samples", type=int, default=806400); ap.add_argument("--piece", type=int, default=96000)
    a = ap.parse_args()
    B, n, pc = a.streams, a.samples, a.piece
    dev = torch.device("cuda", 0)
    eng = BatchEngine(B, max_tx_mf=1)
    lib, h = eng.lib, eng.h
    sp = lambda: torch.cuda.current_stream().cuda_stream
    sigma, f0, seed = float(sigma_from_EbNodB(3.0)), 8.0, 12345
    taps, ratio, _ = doppler_plan(PRESETS["mpp"][0], 8000, n)
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    hf = multipath_gain(taps)
    g = torch.Generator(device=dev); g.manual_seed(1)
    tx = torch.view_as_complex(torch.randn((B, n, 2), generator=g, device=dev) * 0.5)
    rx = torch.empty((B, n), dtype=torch.complex64, device=dev)
    G = torch.empty((B, n, 2), dtype=torch.complex64, device=dev)
    rxp = torch.empty((B, pc), dtype=torch.complex64, device=dev)
    Gp = torch.empty((B, pc + 16, 2), dtype=torch.complex64, device=dev)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))

    def whole(with_G):
        p = ChannelParams(n, 0, 0, 0, sigma, f0, 0.0, G.data_ptr() if with_G else None, None, seed, 0.0, 0.0, 1.0)
        assert lib.rade_batch_channel(h, tx.data_ptr(), n, rx.data_ptr(), n, C.byref(p), sp()) == n

    def whole_gen():
        assert lib.rade_batch_multipath_gen(h, tp, len(taps), ratio, n, None, seed, G.data_ptr(), sp()) == n

    def pieces(chan, gen, with_G):
        for s in range(0, n, pc):
            m, lo = min(pc, n - s), max(s - 16, 0)
            cnt, cnt_g = np.full(B, m, np.int32), np.full(B, s + m - lo, np.int32)
            if gen:
                assert lib.rade_batch_multipath_piece(h, taps.ctypes.data, len(taps), ratio, hf, seed, np.full(B, lo, np.int64).ctypes.data, cnt_g.ctypes.data,
                                                      Gp.data_ptr(), pc + 16, sp()) == 0
            if chan:
                p = ChannelPieceParams()
                p.sigma, p.freq_offset, p.gain, p.n0, p.in_base, p.g_base, p.seed, p.rx_gain = sigma, f0, 1.0, s, lo, lo, seed, 1.0
                if with_G:
                    p.G_dev, p.g_stride, p.n_g_host = Gp.data_ptr(), pc + 16, cnt_g.ctypes.data
                assert lib.rade_batch_channel_piece(h, tx.data_ptr() + 8 * lo, n, cnt_g.ctypes.data, rxp.data_ptr(), pc, cnt.ctypes.data, C.byref(p), sp()) == 0

    calls = {"whole_awgn": lambda: whole(False), "piece_awgn": lambda: pieces(True, False, False), "whole_mpp": lambda: whole(True),
             "piece_mpp": lambda: pieces(True, False, True), "whole_mpp_gen": whole_gen, "piece_mpp_gen": lambda: pieces(False, True, False),
             "copy": lambda: rx.copy_(tx)}
    whole_gen()
    stg.warm(calls, 1)
    ts = stg.rounds(calls, a.rounds, 1, clocks={k: stg.wall for k in calls})
    res = {"streams": B, "samples": n, "piece": pc, "pieces": -(-n // pc), "low_ratio": ratio, "n_taps": int(len(taps)), "rounds": a.rounds, "clock": "host, synchronised",
           "ms_per_total": stg.stats(ts)}
    med = lambda k: res["ms_per_total"][k]["median"]
    res["ns_per_sample"] = {k: 1e6 * med(k) / (B * n) for k in calls}
    res["piece_over_whole"] = {"awgn": med("piece_awgn") / med("whole_awgn"), "mpp_channel": med("piece_mpp") / med("whole_mpp"),
                               "mpp_generator": med("piece_mpp_gen") / med("whole_mpp_gen"),
                               "mpp_generator_and_channel": (med("piece_mpp") + med("piece_mpp_gen")) / (med("whole_mpp") + med("whole_mpp_gen"))}
    res["over_copy"] = {k: med(k) / med("copy") for k in calls if k != "copy"}
    res["g_share_of_piece_mpp"] = 1.0 - med("piece_awgn") / med("piece_mpp")
    res["x_real_time"] = {k: B * n / 8000.0 / (1e-3 * med(k)) for k in calls if k != "copy"}
    stg.emit(res, a.out)
    eng.close()


if __name__ == "__main__":
    main()
