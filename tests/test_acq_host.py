"""The host side of the whole-file acquisition stage, on the CPU: rade_acq_hops, rade_acq_track and rade_acq_stats against tests/golden/acq.npz (what the reference's
rx.py --acq_test computes frame by frame on eight inputs, oracle/golden/acquisition.py), the float64 restatement tests/acq_ref.py pinned to the same fixture, each comparison
shown to reject the mistake it is there for, and the torch band-pass of radae_amd/acq.py against a float64 FIR."""
import numpy as np
import pytest

import acq_ref as R
from radae_amd import abi, acq, stages

FX = R.fixture()


def fixture_hops(name, tag):
    h = np.zeros(len(FX[f"{name}_{tag}_tmax"]), np.dtype(abi.AcqHop))
    for k in ("tmax", "f_ind", "candidate", "Dthresh", "Dtmax12"):
        h[k] = FX[f"{name}_{tag}_{k}"]
    return h


def test_the_engines_tables_are_the_references():
    """acq_ref reads p and p_w as the engine holds them; they are the reference's within an ulp of the largest entry (p) and two (p_w: a rounded product of rounded
    factors, formed by another libm)"""
    c = np.load(R.GOLDEN + "/consts.npz")
    p, p_w = R.consts()
    assert np.abs(p - c["p"]).max() <= 2.0 ** -23 * np.abs(c["p"]).max() and np.abs(p_w - c["acq_p_w"]).max() <= 2.0 ** -22 * np.abs(c["p"]).max()


# ---- rade_acq_hops ---------------------------------------------------------------------------------------------------------------------------------------------
def test_hops_at_the_edges_and_against_the_loop():
    assert [stages.acq_hops(n) for n in (0, 2111, 2112, 3072, 3073)] == [0, 0, 1, 1, 2]
    assert all(stages.acq_hops(n) == R.hops(n) for n in range(6001))
    assert [stages.acq_hops(len(R.fixture_input(k))) for k in R.RECORDINGS] == [30, 24, 26, 30]


# ---- rade_acq_track, rade_acq_stats ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["raw", "bpf"])
@pytest.mark.parametrize("name", R.ALL)
def test_track_and_stats_reproduce_the_fixture(name, tag):
    h = fixture_hops(name, tag)
    ev, log = stages.acq_track(h, acq_test=True)
    want = FX[f"{name}_{tag}_events"]
    assert np.array_equal(np.stack([ev["hop"], ev["tmax"], ev["f_ind"]], 1).reshape(-1, 3), want)
    assert np.array_equal(log["state"], FX[f"{name}_{tag}_state"]) and np.array_equal(log["tmax_candidate"], FX[f"{name}_{tag}_tmax_candidate"])
    assert np.array_equal(stages.acq_fmax(h), FX[f"{name}_{tag}_fmax"])
    first, _ = stages.acq_track(h, acq_test=False)                       # rx.py's normal run stops at the first acquisition
    assert len(first) == min(len(want), 1) and (not len(want) or tuple(first[0]) == tuple(want[0]))
    rf = np.zeros(len(ev), np.dtype(abi.AcqRefined))
    rf["t"] = FX[f"{name}_{tag}_refined"][:, 0] + 960 * want[:, 0]       # the fixture holds refine's timing inside the hop
    rf["f"] = FX[f"{name}_{tag}_refined"][:, 1]
    st = stages.acq_stats(ev, rf, len(h), 101 if tag == "bpf" else 0, *R.TARGETS.get(name, (0.0, 1.0)))
    passes, fails, pfail, mean, passed = FX[f"{name}_{tag}_stats"]
    assert (st.passes, st.fails, st.pfail, st.mean_acq_time, st.passed) == (passes, fails, pfail, mean, passed)
    assert R.stats(want.tolist(), list(zip(rf["t"], rf["f"])), len(h), 101 if tag == "bpf" else 0, *R.TARGETS.get(name, (0.0, 1.0))) == (passes, fails, pfail, mean, bool(passed))
    ev2, log2 = R.track(h["candidate"], h["tmax"], h["f_ind"], True)
    assert ev2 == [tuple(e) for e in want.tolist()] and [tuple(v) for v in log2] == [tuple(v) for v in log.tolist()]


@pytest.mark.parametrize("name", ["noise", "sine"])
def test_the_must_not_acquire_inputs_do_not_pass(name):
    for tag in ("raw", "bpf"):
        h = fixture_hops(name, tag)
        ev, _ = stages.acq_track(h, acq_test=True)
        st = stages.acq_stats(ev, np.zeros(len(ev), np.dtype(abi.AcqRefined)), len(h), 0, 0.0, 1e9)
        assert len(ev) == 0 and not st.passed and st.passes == 0 and np.isinf(st.mean_acq_time) and st.pfail == 0.0


def test_the_fixture_has_a_passing_and_a_just_failing_run():
    assert FX["awgn320_raw_stats"][4] == 1 and FX["awgn320_bpf_stats"][4] == 1
    assert FX["dfdt320_raw_stats"][2] == 0.2 and FX["dfdt320_raw_stats"][4] == 0           # P(fail) = 0.2 is not < 0.2


def test_track_and_stats_refuse():
    lib = abi.load_library()
    h = fixture_hops("awgn", "raw")
    ev = np.zeros(4, np.dtype(abi.AcqEvent))
    assert lib.rade_acq_track(None, 3, 1, ev.ctypes.data, 4, None) == -1 and lib.rade_acq_track(h.ctypes.data, -1, 1, ev.ctypes.data, 4, None) == -1
    assert lib.rade_acq_track(h.ctypes.data, len(h), 1, None, 4, None) == -1
    assert lib.rade_acq_track(h.ctypes.data, len(h), 1, ev.ctypes.data, 2, None) == 4 and ev["hop"].tolist() == [10, 14, 0, 0]      # counted, not stored
    assert lib.rade_acq_stats(None, None, 1, 3, 0, 0.0, 1.0, abi.AcqResult()) == -1 and lib.rade_acq_stats(None, None, 0, 3, 0, 0.0, 1.0, None) == -1


# ---- acq_ref against the fixture, and what the comparison rejects -------------------------------------------------------------------------------------------------
def hop_mismatches(got, name):
    """acq_ref.detect's hops against the fixture's unfiltered run: discrete values equal, Dtmax12 and Dthresh to 1e-6 relative (the reference's float32 surface is
    within 8e-7 max |x| of float64)"""
    bad = []
    if len(got) != len(FX[f"{name}_raw_tmax"]):
        return [f"{len(got)} hops"]
    for k, h in enumerate(got):
        for f in ("tmax", "f_ind", "candidate", "fmax"):
            if h[f] != FX[f"{name}_raw_{f}"][k]:
                bad.append(f"hop {k}: {f} {h[f]} != {FX[f'{name}_raw_{f}'][k]}")
        for f in ("Dtmax12", "Dthresh"):
            if abs(h[f] - FX[f"{name}_raw_{f}"][k]) > 1e-6 * FX[f"{name}_raw_{f}"][k]:
                bad.append(f"hop {k}: {f} {h[f]} != {FX[f'{name}_raw_{f}'][k]}")
    return bad


@pytest.mark.parametrize("name", R.ALL)
def test_acq_ref_matches_the_fixture(name):
    assert not hop_mismatches(R.fixture_detect(name), name)
    x = R.fixture_input(name)
    for (hop, tmax, f_ind), (t, f) in zip(FX[f"{name}_raw_events"], FX[f"{name}_raw_refined"]):
        got = R.refine(x, 960 * hop + tmax, -50 + 2.5 * f_ind)
        assert (got[0] - 960 * hop, got[1]) == (t, f)
    assert np.abs(R.surface(R.fixture_input("mpp"), 1920, 64) - FX["mpp_raw_hop2_Dt1"]).max() < 8e-7 * np.abs(R.fixture_input("mpp")).max() * 160 * 0.124


@pytest.mark.parametrize("bug", ["hop961", "dt2_own", "s1_only"])
def test_the_fixture_comparison_rejects(bug):
    bad = hop_mismatches(R.detect(R.fixture_input("awgn"), bug=bug), "awgn")
    print(bug, len(bad), bad[:2])
    assert bad
    if bug == "hop961":
        assert not any(b.startswith("hop 0:") for b in bad) and any(b.startswith("hop 1: tmax") for b in bad)      # the first hop is where it should be
    if bug == "s1_only":
        assert all("Dthresh" in b or "candidate" in b for b in bad)


def test_ties_go_to_the_first_cell_and_the_comparison_rejects_the_last():
    """a stream of period 480: D[t] = D[t + 480] exactly, so every hop's best cell has an equal 480 timings later"""
    rng = np.random.default_rng(5)
    x = np.tile((rng.standard_normal(480) + 1j * rng.standard_normal(480)).astype(np.complex64), 7)[:3073]
    first, last = R.detect(x), R.detect(x, bug="ties_last")
    assert len(first) == 2
    for a, b in zip(first, last):
        assert a["tmax"] < 480 and b["tmax"] == a["tmax"] + 480 and a["f_ind"] == b["f_ind"] and a["Dtmax12"] == b["Dtmax12"] == a["second"]


def test_the_refine_comparison_rejects_a_missing_phase_term():
    x = R.fixture_input("foff")
    hop, tmax, f_ind = FX["foff_raw_events"][0]
    t, f = FX["foff_raw_refined"][0]
    assert (R.refine(x, 960 * hop + tmax, -50 + 2.5 * f_ind)[1], R.refine(x, 960 * hop + tmax, -50 + 2.5 * f_ind, bug="no_phase")[1] != f) == (f, True)


def test_refine_skips_the_timings_outside_the_stream():
    x = R.fixture_input("awgn320")
    assert R.refine(x[32:], 0, 10.0)[0] in (0, 1)                         # t = -1 is not read
    assert R.refine(x[:1000], 0, 10.0)[:3] == (0, 10.0, 0.0)              # no window fits


# ---- the band-pass of radae_amd/acq.py ----------------------------------------------------------------------------------------------------------------------------
def test_the_design_is_the_receivers_filter():
    c = np.load(R.GOLDEN + "/consts.npz")
    h, alpha = acq.bpf_design()
    assert np.array_equal(h, c["bpf_h"].real.astype(np.float32)) and alpha == float(c["bpf_alpha"])


def test_the_torch_band_pass_against_float64_on_the_cpu():
    import torch
    xs = [R.fixture_input("awgn")[:5000], R.fixture_input("sine")[:5000]]
    y = acq.complex_bpf(torch.tensor(np.stack(xs))).numpy()
    h, _ = acq.bpf_design()
    for x, got in zip(xs, y):
        want = R.bpf(x)
        # float32: the phasor (2^-24), two complex products (2 x 2 x 2^-24) and a 101-term sum in an unknown order (101 x 2^-24), relative to sum |h| max |x|
        tol = (101 + 5) * 2.0 ** -24 * np.abs(h).sum() * np.abs(x).max()
        err = np.abs(got - want).max()
        print(f"band-pass: max error {err:.3g}, bound {tol:.3g}")
        assert err < tol
    # a stream's filtered samples do not depend on what lies behind its length (the FIR is causal)
    assert np.array_equal(acq.complex_bpf(torch.tensor(xs[0][None, :3000])).numpy()[0], y[0][:3000])
