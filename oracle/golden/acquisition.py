"""Writes tests/golden/acq.npz: what the reference's stored-file receiver (rx.py --pilots [--bpf] --acq_test) computes on eight inputs, frame by frame.

It imports the reference's radae.dsp.acquisition and complex_bpf (without the n() and randint patches) and drives them with its own restatement of rx.py:146-195: rx.py itself cannot be imported (it runs at import, and needs a checkpoint).

Inputs: the rx_in of the committed rxtrace_mpp / _awgn / _foff / _dfdt recordings (read from those files, not stored again), and two seeded must-not-acquire streams of 12
modem frames, which are stored (awgn320 / dfdt320 are views of the recordings): complex noise, and a real 1 kHz sine in real noise (the reference's acq_noise and acq_sine ctests in small).
Recorded per input, without and with the input band-pass: per hop candidate, tmax, f_ind_max, fmax, Dthresh, Dtmax12 and the state log (state, tmax_candidate as the
script prints them); the acquisition events with refine's results; the --acq_test statistics.  Also Dt1 of one hop of rxtrace_mpp for 64 timings.
"""
import os

import numpy as np

from . import reference as R
from .reference import golden

FS, M, NCP, NMF, NC = 8000, 160, 32, 960, 30
RECORDINGS = ("mpp", "awgn", "foff", "dfdt")
NAMES = RECORDINGS + ("noise", "sine", "awgn320", "dfdt320")
# --fmax_target and --acq_time_target of an input's run (default 0.0, 1.0).  awgn320 / dfdt320 are the recordings less their first 320 samples, which puts the pilots
# at the timing --acq_test expects without a band-pass (Ncp): the first passes, the second has one of five acquisitions off in frequency (P(fail) = 0.2: no PASS)
TARGETS = {"awgn320": (11.0, 2.0), "dfdt320": (13.25, 2.0)}


def inputs(src):
    x = {k: np.load(golden(src, f"rxtrace_{k}.npz"))["rx_in"].astype(np.complex64) for k in RECORDINGS}
    rng = np.random.default_rng(20261)
    n = 12 * NMF
    x["noise"] = (0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x["sine"] = (0.3 * np.cos(2 * np.pi * 1000.0 * np.arange(n) / FS) + 0.1 * rng.standard_normal(n)).astype(np.complex64)
    x["awgn320"], x["dfdt320"] = x["awgn"][320:], x["dfdt"][320:]
    return x


def run(acq, rx, ntap, fmax_target=0.0, acq_time_target=1.0):
    """rx.py:134-195 with --acq_test"""
    target = NCP + ntap / 2
    rec = {k: [] for k in ("candidate", "tmax", "f_ind", "fmax", "Dthresh", "Dtmax12", "state", "tmax_candidate")}
    events, refined = [], []
    acq_pass = acq_fail = 0
    tmax_candidate, state, valid_count, mf = 0, "search", 0, 1
    while len(rx) >= 2 * NMF + M + NCP:                # DEVIATION from rx.py:146 (>= 2 Nmf + M): the hop its assert would trip on is not run
        candidate, tmax, fmax = acq.detect_pilots(rx[:2 * NMF + M + NCP])
        for k, v in (("candidate", int(candidate)), ("tmax", tmax), ("f_ind", acq.f_ind_max), ("fmax", float(fmax)), ("Dthresh", float(acq.Dthresh)),
                     ("Dtmax12", float(acq.Dtmax12)), ("state", int(state == "candidate")), ("tmax_candidate", tmax_candidate)):
            rec[k].append(v)
        next_state = state
        if state == "search":
            if candidate:
                next_state, tmax_candidate, valid_count = "candidate", tmax, 1
        elif candidate and np.abs(tmax - tmax_candidate) < 0.02 * M:
            valid_count += 1
            if valid_count > 3:
                next_state = "search"
                events.append((mf - 1, tmax, acq.f_ind_max))
                t2, f2 = acq.refine(rx, tmax, fmax, np.arange(tmax - 1, tmax + 2), np.arange(fmax - 10, fmax + 10, 0.25))
                refined.append((t2, f2))
                if np.abs(t2 - target) < 0.0025 * FS and np.abs(f2 - fmax_target) <= 5.0:
                    acq_pass += 1
                else:
                    acq_fail += 1
        else:
            next_state = "search"
        state = next_state
        rx = rx[NMF:-1]
        mf += 1
    mean_acq_time = (NMF * mf / FS) / acq_pass if acq_pass else np.inf
    pfail = acq_fail / (acq_pass + acq_fail) if acq_pass + acq_fail else 0.0
    out = {k: np.array(v, np.float64 if k in ("fmax", "Dthresh", "Dtmax12") else np.int32) for k, v in rec.items()}
    out["events"] = np.array(events, np.int32).reshape(-1, 3)
    out["refined"] = np.array(refined, np.float64).reshape(-1, 2)
    out["stats"] = np.array([acq_pass, acq_fail, pfail, mean_acq_time, float(pfail < 0.2 and mean_acq_time < acq_time_target)], np.float64)
    return out


def main(src, dst):
    R.enter(patched=False)
    from radae.dsp import acquisition, complex_bpf
    c = np.load(golden(src, "consts.npz"))
    acq = acquisition(FS, 50, M, NCP, NMF, c["p"], c["pend"])
    assert np.array_equal(acq.p_w, c["acq_p_w"])
    w = c["w"]
    bandwidth = 1.2 * (w[NC - 1] - w[0]) * FS / (2 * np.pi)
    centre = (w[NC - 1] + w[0]) * FS / (2 * np.pi) / 2
    out = {}
    x = inputs(src)
    out["x_noise"], out["x_sine"] = x["noise"], x["sine"]
    for name in NAMES:
        for tag, ntap in (("raw", 0), ("bpf", 101)):
            rx = x[name] if not ntap else complex_bpf(ntap, FS, bandwidth, centre, len(x[name])).bpf(x[name])
            r = run(acq, rx, ntap, *TARGETS.get(name, (0.0, 1.0)))
            print(f"{name:6s} {tag}: {len(r['tmax'])} hops, {int(r['candidate'].sum())} candidates, events {r['events'].tolist()}, stats {r['stats'].tolist()}")
            out.update({f"{name}_{tag}_{k}": v for k, v in r.items()})
    acq.detect_pilots(x["mpp"][2 * NMF:2 * NMF + 2 * NMF + M + NCP])
    out["mpp_raw_hop2_Dt1"] = acq.Dt1[:64].astype(np.complex64)
    np.savez_compressed(golden(dst, "acq.npz"), **out)
    print(os.path.getsize(golden(dst, "acq.npz")), "bytes")
