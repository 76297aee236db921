"""tests/rx_ref.py -- the float64 statement of one call of the live receiver -- held to what the reference recorded (tests/golden/rxtrace_*.npz, bpf.npz), and its bounds
shown to be sharp: every `bug=` variant of the model breaks one against the unperturbed model.  The comparison is always with the reference's recorded output, never with a
device.  CPU only.

What the reference's float32 arithmetic (and its band-pass's float32 mixer phases, 5e-5 of the peak) differs by is measured in units of the model's own per-value bound
-- the bound the MI355X is held to in tests/test_rx_stage_model_gpu.py -- so that the figure means the same on a unit-scale recording and on an int16-scaled one.  REF_WORST
holds the largest error / bound over the ten recordings as measured, the assertions stand at the next power of two above it."""
import os
import re

import numpy as np
import pytest

import acq_ref
import rx_ref as X
from trace_ref import edge_case_input

FULL = ("awgn", "mpp", "foff", "slip_plus", "slip_minus", "dfdt", "nounsync", "eoo_mpp")
THIN = ("slipdrops", "dfs8001")                                # every fourth row kept: per-call scalars only
# largest error / bound against the reference's recorded traces, and the bar: the next power of two
REF_WORST = {"Dthresh": (0.0313, 2.0 ** -4), "Dtmax12 search": (0.838, 1.0), "Dtmax12 sync": (13.3, 16.0), "Dtmax12_eoo": (18.6, 32.0), "z_hat": (1.39, 2.0),
             "snrdB_3k_est": (0.0487, 2.0 ** -4), "eoo symbols": (1.60, 2.0)}
BPF_WORST = (4.57e-5, 2.0 ** -14)                              # bpf_calls against bpf.npz, of the peak


def _stored(golden, name):
    g = golden("rxtrace_" + name)
    d = {k: g[k] for k in g.files}
    d["z_all"] = X.z_all_of(d)
    return d, edge_case_input(g)


@pytest.fixture(scope="module")
def replayed(golden):
    """replay() of a recording, computed once and shared (read-only)"""
    made = {}

    def get(name):
        if name not in made:
            g, x = _stored(golden, name)
            f = X.bpf_calls(x, g["nin_before"]).astype(np.complex64)
            made[name] = (g, f, X.replay(f, g, 1, 10.0 if name == "foff" else 0.0))
        return made[name]
    return get


def test_bpf_calls_honours_the_filter_memory_quirk(golden):
    """complex_bpf keeps 102 samples of memory where it allocated 100 (dsp.py:55, :96): against the reference's own output for 960 / 800 / 1120-sample calls"""
    g = golden("bpf")
    y = X.bpf_calls(g["x"], g["sizes"])
    err = float(np.abs(y - g["y"]).max() / np.abs(g["y"]).max())
    print(f"bpf_calls against bpf.npz: {err:.3e} of the peak")
    assert err < BPF_WORST[1]
    n0 = int(g["sizes"][0])
    plain = acq_ref.bpf(g["x"])                                # the filter without the quirk: equal over the first call, two samples early afterwards
    assert np.abs(plain[:n0] - g["y"][:n0]).max() < BPF_WORST[1] * np.abs(g["y"]).max()
    assert np.abs(plain[n0:len(y)] - g["y"][n0:]).max() > 0.05 * np.abs(g["y"]).max()


def test_rx_buf_is_the_references_shift_and_append():
    """rx_bufs() against radae_rxe.py:196-197 as written, bit for bit, over 960 / 800 / 1120-sample calls"""
    rng = np.random.default_rng(5)
    sizes = [960, 960, 800, 1120, 960, 1120, 800]
    x = (rng.standard_normal(sum(sizes)) + 1j * rng.standard_normal(sum(sizes))).astype(np.complex64)
    rx_buf, pos = np.zeros(2 * 960 + 160 + 32, np.csingle), 0
    got = X.rx_bufs(x, sizes)
    for k, nin in enumerate(sizes):
        rx_buf[:-nin] = rx_buf[nin:]
        rx_buf[-nin:] = x[pos:pos + nin]
        pos += nin
        assert np.array_equal(got[k].view(np.uint32), rx_buf.view(np.uint32)), k


def test_lcg_rows_are_the_kernels_jump_table():
    """check_pilots' row draws: the model's sequential generator against the 48 jump-ahead pairs k_rx_sync2 uses (x_k = A[k] x + C[k]), for several seeds.  (The C oracle
    draws the same rows but shows neither them nor its rx_buf: an accessor there is a follow-up)"""
    with open(os.path.join(os.path.dirname(X.__file__), "..", "radae_amd", "csrc", "rade_rx.hip")) as f:
        src = f.read()
    tab = {n: [int(v) for v in re.search(r"LCG_%s\[48\] = \{([^}]*)\}" % n, src).group(1).replace("u", "").split(",")] for n in "AC"}
    assert len(tab["A"]) == 48 and len(tab["C"]) == 48 and tab["A"][0] == 1664525 and tab["C"][0] == 1013904223
    for seed in (1, 2, 12345, 0xFFFFFFFF):
        rows, nxt = X.lcg_rows(seed)
        xs = [(a * seed + c) & 0xFFFFFFFF for a, c in zip(tab["A"], tab["C"])]
        assert rows == [(v >> 8) % 960 for v in xs] and nxt == xs[-1]


@pytest.mark.parametrize("name", FULL + THIN)
def test_replay_against_the_recorded_traces(replayed, name):
    """every call of a recording: the reference's cell is the model's arg-max wherever the float64 lead decides, fmax bit for bit, the slip rule and the end-of-over
    decision equal; Dtmax12, Dtmax12_eoo, Dthresh, snrdB_3k_est and z_hat / the end-of-over symbols within the reference's float32 rounding"""
    g, f, recs = replayed(name)
    assert len(recs) == len(g["ret"]) and int(np.sum(g["nin_before"])) <= len(f)
    c = X.check(recs, g, z=name in FULL)
    print(name, len(recs), "calls;", "undecided", c["undecided"], {k: f"{v:.3g}" for k, v in c["worst"].items()}, {k: f"{v:.2e}" for k, v in c["largest"].items()})
    discrete = [q for q in c["fail"] if q[3] == 0.0 or "cell" in q[1] or "decision" in q[1]]
    assert not discrete, discrete[:4]
    assert c["undecided"] <= 0.02 * len(recs) and c["snr_reseeded"] == 0
    for k, v in c["worst"].items():
        assert v <= REF_WORST[k][1], (k, v)
    kinds = {r["kind"] for r in recs}
    assert kinds == {"search", "sync"} and any("entry" in r for r in recs)
    if name.startswith("slip") or name == "dfs8001":
        assert any(r["kind"] == "sync" and r["nin_after"] != 960 for r in recs)
    if name == "eoo_mpp":
        assert sum(1 for r in recs if r["kind"] == "sync" and r["eoo"]) == 5


def test_ref_worst_is_what_the_recordings_give(replayed):
    """REF_WORST's measured column, so that the table of DESIGN.md cannot drift from the code: within 2 % of the largest error / bound over the recordings"""
    tot = {}
    for name in FULL + THIN:
        g, _, recs = replayed(name)
        for k, v in X.check(recs, g, z=name in FULL)["worst"].items():
            tot[k] = max(tot.get(k, 0.0), v)
    for k, (measured, bar) in REF_WORST.items():
        assert abs(tot[k] - measured) <= 0.02 * measured and measured < bar <= 2 * measured + 1e-12, (k, tot[k], measured, bar)


@pytest.mark.parametrize("bug", X.BUGS)
def test_every_planted_mistake_breaks_a_bound(replayed, bug):
    """the sharpness rule: a trace made of the perturbed model's values, held to the unperturbed model, on the recordings the GPU test feeds the device.  phase_960 is the
    one that no output can show -- a constant rotation of a call's window, which the pilot equaliser removes and the correlations never see (the reference's own comment at
    radae_rxe.py:226 suspects as much): for it the symbols before the equaliser move and every output stays inside its bound."""
    want = {"win_late": "z_hat", "dft_11bit": "z_hat", "eq_edge_noclamp": "z_hat", "row_off": "Dthresh", "pend_p": "Dtmax12_eoo", "peak_cell_off": "search", "mag_nogain": "z_hat"}
    for name in ("mpp", "eoo_mpp"):
        g, f, clean = replayed(name)
        assert not X.check(clean, X.synth_trace(clean, g))["fail"]                 # the unperturbed model passes its own check exactly
        bad = X.replay(f, g, 1, 0.0, bug=bug)
        c = X.check(clean, X.synth_trace(bad, g))
        if bug == "phase_960":
            moved = max(float(np.abs(a["sym"] - b["sym"]).max() / a["e_sym"].max()) for a, b in zip(clean, bad) if a["kind"] == "sync")
            assert moved > 1e3 and not c["fail"]
            continue
        hit = [q for q in c["fail"] if q[1].startswith(want[bug])]
        assert hit, (bug, name, c["worst"])
        if bug == "eq_edge_noclamp":                                               # the edge carriers c = 0 and c = 29 move (the others only through mag)
            idx = {int(re.search(r"\[(\d+)\]", q[1]).group(1)) // 2 % 30 for q in hit}
            assert idx & {0, 29}, idx


@pytest.mark.parametrize("case", ["peak_placement", "levels"])
def test_crafted_streams_meet_their_conditions(oracle, oracle_model, case):
    """the GPU test's crafted streams as the device gets them (12 calls; the level streams with their step and click), on the CPU: the float64 band-pass for the device's
    filter, the C oracle's trace for the decisions.  Every arg-max of every call -- search surface, entry grid, in-sync grid -- leads its runner-up by more than the two
    cells' bounds, so no call can come out undecided (what `undecided == 0` on the GPU relies on).  In the first search call whose rx_buf holds only samples from the second
    call on (the fourth: until then the band-pass's two-sample quirk splits a pilot pair) every stream's targeted (timing, frequency) cell is the arg-max, with a lead of at
    least ten times the sum of the two cells' bounds, and the batch's arg-max cells contain every target of the list."""
    tg, rows = X.crafted_batch(32) if case == "peak_placement" else X.level_batch()
    if case == "peak_placement":
        assert {t for t, _ in tg} == set(X.TIMINGS) and {f for _, f in tg} == set(X.FREQS)
    found, smallest = set(), np.inf
    for b, x in enumerate(rows):
        tr = oracle.run_rx_stream(oracle_model, x)
        tr["z_all"] = X.z_all_of(tr)
        recs = X.replay(X.bpf_calls(x, tr["nin_before"]).astype(np.complex64), tr)
        assert len(recs) >= X.N_CALLS - 1 and sum(r["kind"] == "sync" for r in recs) >= 3, (b, len(recs))
        for i, what, lead, two in X.decidable(recs):
            assert lead > two, (b, i, what, lead, two)
            smallest = min(smallest, lead / two)
        r3 = recs[3]
        assert r3["kind"] == "search" and r3["argmax"] == tg[b], (b, tg[b], r3["argmax"])
        order = np.argsort(r3["S"].ravel())
        assert r3["lead"] >= 10 * (r3["b12"].ravel()[order[-1]] + r3["b12"].ravel()[order[-2]]), (b, r3["lead"])
        found.add(r3["argmax"])
    print(f"{case}: smallest lead / bounds over every arg-max {smallest:.2f}")
    assert found == set(tg)
