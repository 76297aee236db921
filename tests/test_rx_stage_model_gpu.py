"""k_rx_sync2's signal processing against tests/rx_ref.py, the float64 statement of one receiver call, call by call: the two-stage pilot search (rx2_detect_q), both forms
of refine(), check_pilots (check2_rows_q), the four correlations at (tmax, fmax), the frequency-corrected window, the matrix-core demodulator DFT, the 3-pilot LS equaliser,
mag, the SNR estimate and the end-of-over branch.  Everything compared is visible through existing entry points: rx_filtered (the samples the receiver consumed), rx_trace
(the scalars and the 240-float row of every call), rx_reset (the row draws' seeds).

Every test runs the device once, replays every stream's trace through the model (teacher-forced: the model is run at the device's decisions and the decisions are held to
the model's own surfaces) and asserts for every call of every stream what rx_ref.check states: the cell rule, fmax and the slip rule bit for bit, every value inside the
bound rx_ref's docstring derives.  The bounds are counts of the kernel's roundings, not measurements; WORST_MEASURED records the largest error / bound the MI355X has shown
per quantity and case and is printed beside each run's figures, never asserted: only the counted bounds decide.  A device that exceeds a bound is a finding: a term the count missed, or a mistake of the kernel."""
import numpy as np
import pytest

import rx_ref as X
from gpu_kit import Engine, dev, engine, pack, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# largest error / bound seen on the MI355X, per case (a) peak placement, (b) levels, (c) committed inputs
WORST_MEASURED = {
    "a": {"Dthresh": 0.0022, "Dtmax12 search": 0.0241, "Dtmax12 sync": 0.0406, "Dtmax12_eoo": 0.0403, "snrdB_3k_est": 0.0017, "z_hat": 0.0119},
    "b": {"Dthresh": 0.0017, "Dtmax12 search": 0.0238, "Dtmax12 sync": 0.0406, "Dtmax12_eoo": 0.0224, "snrdB_3k_est": 0.0009, "z_hat": 0.0535},
    "c": {"Dthresh": 0.0018, "Dtmax12 search": 0.0171, "Dtmax12 sync": 0.0307, "Dtmax12_eoo": 0.0231, "eoo symbols": 0.0109, "snrdB_3k_est": 0.0005, "z_hat": 0.0092},
}
N_CALLS = X.N_CALLS


def run_and_check(eng, rows, seeds=None, foff_err=0.0, what=""):
    """one invocation on `rows` (a list of complex64 streams), every stream replayed and checked: (traces, per-stream check results, rx()'s outputs)"""
    import torch
    x, n = pack(rows)
    eng.rx_reset(seeds if seeds is not None else [1] * len(rows))
    out, st, eoo = eng.rx(torch.tensor(x, device=eng.device), n_avail=n)
    torch.cuda.synchronize()
    traces, results = [], []
    for b in range(len(rows)):
        tr = eng.rx_trace(b)
        assert st[b].n_calls == len(tr["ret"]) <= eng.trace_calls and st[b].consumed == int(tr["nin_before"].sum()), (what, b)
        f = eng.rx_filtered(b, st[b].consumed)
        assert len(f) == st[b].consumed
        recs = X.replay(f, tr, (seeds[b] if seeds is not None else 1), foff_err)
        c = X.check(recs, tr)
        c["recs"] = [{k: v for k, v in r.items() if k not in ("S", "b12", "V", "bV")} for r in recs]       # (the surfaces are 600 KB per call)
        traces.append(tr); results.append(c)
    return traces, results, (out, st, eoo)


def report(case, results):
    """print each figure before anything is asserted, then: no value outside its bound in any call of any stream"""
    worst, calls, undecided, reseeded = {}, 0, 0, 0
    for c in results:
        calls += c["calls"]; undecided += c["undecided"]; reseeded += c["snr_reseeded"]
        for k, v in c["worst"].items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"case {case}: {len(results)} streams, {calls} calls, undecided {undecided}, snr reseeded {reseeded}; error / bound:", {k: round(v, 4) for k, v in sorted(worst.items())})
    print(f"case {case}: recorded so far:", WORST_MEASURED[case])
    fails = [(b,) + q for b, c in enumerate(results) for q in c["fail"]]
    assert not fails, (len(fails), fails[:6])
    assert reseeded == 0                                     # no call's snrdB_3k_est was left out: the SNR bound stayed finite in every call, the model's state never restarted from the trace
    return worst, calls, undecided


def test_peak_placement(engine):
    """(a) 32 crafted streams through an engine without the decoder: every timing and frequency edge of the correlator's tiles is some stream's peak.  The streams go search,
    candidate, entry, sync on their own; covered besides: the entry grid at t0 = max(0, tm - 1) with tm = 0, 800- and 1120-sample calls off the band-pass grid, the first
    synchronised call (nobody prepared refine()'s constants).  The 240-float output rows are the trace's z_hat rows bit for bit."""
    from radae_amd.engine import BYPASS_DEC
    B = 32
    tg, rows = X.crafted_batch(B)
    eng = engine(B, max_tx_mf=1, rx_trace_calls=N_CALLS + 4, flags=BYPASS_DEC)
    traces, results, (out, st, _) = run_and_check(eng, rows, what="a")
    worst, calls, undecided = report("a", results)
    assert undecided == 0                                                           # a condition on the inputs: tests/test_rx_ref_host.py shows the model alone meets it
    out = out.cpu().numpy()
    nins, found, first_sync = set(), set(), 0
    for b, (tr, c) in enumerate(zip(traces, results)):
        sb, sa = tr["state_before"], tr["state_after"]
        assert len(sb) >= N_CALLS - 1 and sb[0] == 0 and (sb == 1).any() and (sb == 2).sum() >= 3, (b, sb)
        # from the fourth call on rx_buf holds no sample of the first call: the target is the model's arg-max of every search call (the cell rule ties the device's cell
        # to it), and the cell the trace names wherever the call does not enter sync (an entry call's trace row holds the refined timing)
        steady = [r for r in c["recs"] if r["kind"] == "search" and r["call"] >= 3]
        assert steady and all(r["argmax"] == tg[b] for r in steady), (b, tg[b], [r["argmax"] for r in steady])
        assert all((int(tr["tmax"][r["call"]]), int(tr["f_ind_max"][r["call"]])) == tg[b] for r in steady if "entry" not in r), (b, tg[b])
        assert all(int(tr["f_ind_max"][r["call"]]) == tg[b][1] and abs(int(tr["tmax"][r["call"]]) - tg[b][0]) <= 1 for r in steady if "entry" in r), (b, tg[b])
        found.add(tg[b])
        # the uncached first call (Dt1 and Dt2 computed) and cached ones (the previous call's |Dt2| read back) both occur
        cached = [r["cached"] for r in c["recs"] if r["kind"] == "search"]
        assert cached[0] is False and sum(cached) >= 2, (b, cached)
        nins |= set(tr["nin_before"].tolist())
        e = int(np.argmax(sa == 2))
        first_sync += int(sb[e] == 1 and sb[e + 1] == 2)
        assert np.array_equal(out[b, :st[b].n_valid].view(np.uint32), tr["z_hat"].view(np.uint32)) and st[b].n_valid == len(tr["z_hat"]) > 0, b
        assert not tr["uw_errors"].any()                                            # no decoder stage in this engine: nothing ever sums unique-word errors
    assert found == set(tg) and {t for t, _ in found} == set(X.TIMINGS) and {f for _, f in found} == set(X.FREQS)
    assert nins == {800, 960, 1120} and first_sync == B
    entries = [r["entry"]["tgrid"] for c in results for r in c["recs"] if "entry" in r]
    assert any(len(g) == 2 and g[0] == 0 for g in entries) and any(len(g) == 3 for g in entries)      # t0 = max(0, tm - 1) with tm = 0


def test_levels(engine):
    """(b) the same recipe at 2^-14, 1, 2^10 and 32767 (int16-scaled input), one stream whose level drops by 2^8 between two synchronised calls (the operand scale of the
    next two calls then comes from a call one and two back) and one with a single 60 dB click inside the synchronised part.  The bounds scale with the weights, so the assertions are the same; the click's
    stream is held to its bound with the click in the weights and in X: there the 22-bit planes lose 10 bits (rx_ref: FLOOR)."""
    from radae_amd.engine import BYPASS_DEC
    tg, rows = X.level_batch()
    B, at = len(rows), X.LEVEL_AT
    eng = engine(B, max_tx_mf=1, rx_trace_calls=N_CALLS + 4, flags=BYPASS_DEC)
    traces, results, _ = run_and_check(eng, rows, what="b")
    worst, calls, undecided = report("b", results)
    assert undecided == 0                                                           # crafted streams: tests/test_rx_ref_host.py shows the model alone decides every arg-max of these eight
    for b, (tr, c) in enumerate(zip(traces, results)):                              # and the peak sits on its target once rx_buf holds no sample of the first call
        steady = [r for r in c["recs"] if r["kind"] == "search" and r["call"] >= 3]
        assert steady and all(r["argmax"] == tg[b] for r in steady), (b, tg[b], [r["argmax"] for r in steady])
        assert all((int(tr["tmax"][r["call"]]), int(tr["f_ind_max"][r["call"]])) == tg[b] for r in steady if "entry" not in r), (b, tg[b])
        assert not tr["uw_errors"].any()
    for b, tr in enumerate(traces):
        assert (tr["state_before"] == 2).sum() >= 3, (b, tr["state_before"])
    for b in (4, 5):                                                                # the step and the click fall into synchronised calls, and synchronised calls follow them
        sb, first = traces[b]["state_before"], np.cumsum(traces[b]["nin_before"]) - traces[b]["nin_before"]
        k = int(np.searchsorted(first, at, side="right")) - 1
        assert sb[k] == 2 and k + 2 < len(sb) and sb[k + 1] == 2 and sb[k + 2] == 2, (b, k, sb)
    r4 = results[4]["recs"]
    last = eng.rx_filtered(4, int(traces[4]["nin_before"].sum()))[-int(traces[4]["nin_before"][-1]):]
    assert r4[-1]["X"] > 100 * float(max(np.abs(last.real).max(), np.abs(last.imag).max()))          # the last call's operand scale is two calls old
    X5 = [r["X"] for r in results[5]["recs"]]
    assert max(X5) > 20 * min(x for x in X5 if x > 0)                              # the click really sets the operand scale of three calls


@pytest.fixture(scope="module")
def committed(golden):
    names = ("mpp", "foff", "slip_plus", "slip_minus", "dfdt", "eoo_mpp")
    return names, [golden("rxtrace_" + n)["rx_in"].astype(np.complex64) for n in names], [golden("rxtrace_" + n) for n in names]


def test_committed_inputs(engine, committed):
    """(c) six committed recordings as the streams of one default engine (ragged n_avail, LCG seed 1): fading, frequency drift, real slips, five end-of-over frames with data
    bits; the decoder stage runs between calls, so rx_buf is parked and reloaded, the pilot replicas are reloaded and refine()'s constants rebuilt.  The foff recording runs
    once more through an engine of its own with the 10 Hz entry error (flag 4: it applies to every stream of an engine)."""
    names, rows, gold = committed
    eng = engine(len(rows), max_tx_mf=1, rx_trace_calls=64)
    traces, results, (_, st, eoo) = run_and_check(eng, rows, what="c")
    one = engine(1, max_tx_mf=1, rx_trace_calls=64, flags=4)
    t1, r1, _ = run_and_check(one, [rows[1]], foff_err=10.0, what="c foff")
    worst, calls, undecided = report("c", results + r1)
    assert undecided <= 0.02 * calls
    for b, (name, tr, g) in enumerate(zip(names + ("foff",), traces + t1, list(gold) + [gold[1]])):
        if name != "foff" or b == len(names):
            for k in ("state_before", "state_after", "nin_before", "nin_after", "ret", "tmax", "f_ind_max", "uw_errors", "synced_count"):
                assert np.array_equal(tr[k], g[k]), (name, k)
    # a decoder stage ran between two synchronised calls: unique-word errors are summed behind the decoder only (an engine without it never counts one: cases (a), (b)),
    # so a count that rises from one synchronised call to the next, with sync held, shows the stage ran in between -- rx_buf parked and reloaded around it
    ran = [(b, i) for b, tr in enumerate(traces) for i in range(1, len(tr["ret"]) - 1)
           if tr["state_before"][i - 1] == 2 and tr["state_before"][i] == 2 and tr["state_after"][i] == 2 and tr["uw_errors"][i] > tr["uw_errors"][i - 1]]
    assert ran, [tr["uw_errors"].tolist() for tr in traces]
    k = names.index("eoo_mpp")
    ends = [r for r in results[k]["recs"] if r["kind"] == "sync" and r["eoo"]]
    assert len(ends) == 5 and st[k].has_eoo
    assert np.array_equal(eoo.cpu().numpy()[k].view(np.uint32), traces[k]["eoo_out"][-1].view(np.uint32))          # eoo_out is the trace's row
    assert any(r["kind"] == "sync" and r["nin_after"] == 1120 for r in results[names.index("slip_plus")]["recs"])
    assert any(r["kind"] == "sync" and r["nin_after"] == 800 for r in results[names.index("slip_minus")]["recs"])


def test_cutting_invariance(Engine, monkeypatch):
    """(d) on (a)'s batch, one call per launch (RADE_ROUND_CALLS=1) and the default give the same trace and the same rows per call, bit for bit.  Only the default run is
    compared with the model (test_peak_placement): rx_filtered shows one invocation."""
    import torch
    from radae_amd.engine import BYPASS_DEC
    B = 32
    _, rows = X.crafted_batch(B)
    x, n = pack(rows)
    got = {}
    for mode in ("1", None):
        monkeypatch.delenv("RADE_ROUND_CALLS", raising=False)
        if mode:
            monkeypatch.setenv("RADE_ROUND_CALLS", mode)
        eng = Engine(B, max_tx_mf=1, rx_trace_calls=N_CALLS + 4, flags=BYPASS_DEC)
        try:
            out, st, _ = eng.rx(torch.tensor(x, device=eng.device), n_avail=n)
            torch.cuda.synchronize()
            got[mode] = ([eng.rx_trace(b) for b in range(B)], out.cpu().numpy(), [(s.consumed, s.n_calls, s.n_valid, s.nin, s.state) for s in st])
        finally:
            eng.close()
    assert got["1"][2] == got[None][2]
    assert np.array_equal(got["1"][1].view(np.uint32), got[None][1].view(np.uint32))
    for b in range(B):
        a, d = got["1"][0][b], got[None][0][b]
        for k in a:
            assert a[k].shape == d[k].shape and np.array_equal(a[k].view(np.uint8), d[k].view(np.uint8)), (b, k)
