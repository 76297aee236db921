"""rade_batch_acq_detect and rade_batch_acq_refine on the device against the float64 restatement tests/acq_ref.py (pinned to tests/golden/acq.npz by
tests/test_acq_host.py): the surface within the header's derived bound, the hop records of the fixture inputs under that bound's decidability rule, the smallest shapes at
which the kernel takes another path (planted pilots), refine, radae_amd.acq.acquire end to end, the buffer contract on sentinel buffers (tests/bands.py) and the refusals.

The bound (include/rade_batch.h): | |D|^ - |D| | <= RADE_ACQ_EPS A[t][f], A[t][f] = sum_m |x[t + m]| (|p[m]| G[f][m] + RADE_ACQ_TAB / RADE_ACQ_EPS), RADE_ACQ_EPS = 4.5 x
2^-20, G the moment form's gain (acq_ref.moment_gain), for the complex value too; a hop's Dtmax12 cell RADE_ACQ_EPS (A1[t][f] + A2[t][f]) + 2^-24 Dtmax12; S1 within
RADE_ACQ_EPS sum A1 over the block's cells.  It is a worst-case bound under the header's assumption about the matrix
instruction's rounding; WORST_MEASURED records how far below it the device stays."""
import ctypes as C

import numpy as np
import pytest

import acq_ref as R
from bands import Band
from gpu_kit import dev, engines, pack, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

WORST_MEASURED = 0.0177                # largest |dD| / bound over test_surface on the MI355X
NMF, M = 960, 160
KK = 2 * np.sqrt(-np.log(1e-5 / 5)) / (NMF * 40) / np.sqrt(np.pi / 2) / 2          # Dthresh = KK (S1 + S2)


def raw_detect(eng, x_ptr, x_stride, n, pacq=1e-5, hops=None, max_hops=None, nh=None, dt_ptr=None, t0=0, n_rows=0, null_n=False, null_hops=False, null_nh=False):
    from radae_amd.abi import AcqHop
    from radae_amd.engine import _stream_ptr
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (eng.B,)))
    max_hops = max(max(R.hops(int(v)) for v in n), 1) if max_hops is None else max_hops
    hops = np.zeros((eng.B, max(max_hops, 1)), np.dtype(AcqHop)) if hops is None else hops
    nh = np.zeros(eng.B, np.int32) if nh is None else nh
    rc = eng.lib.rade_batch_acq_detect(eng.h, C.c_void_p(x_ptr), x_stride, None if null_n else n.ctypes.data, pacq, None if null_hops else hops.ctypes.data, max_hops,
                                       None if null_nh else nh.ctypes.data, C.c_void_p(dt_ptr), t0, n_rows, _stream_ptr())
    return rc, hops, nh


def planted(rng, n, plants, noise=1e-3):
    """weak noise with p_w[:, f] added at sample 960 k + t and one frame later, for every (k, t, f): |Dt1| + |Dt2| of hop k peaks at (t, f)"""
    _, p_w = R.consts()
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for k, t, f in plants:
        for off in (NMF * k + t, NMF * (k + 1) + t):
            x[off:off + M] += p_w[:, f]
    return x.astype(np.complex64)


def check_hops(x, got, n_hops, what, ref=None):
    """one stream's records against float64 under the bound's decidability rule; returns the number of hops whose argmax or candidate flag is undecidable"""
    ref = R.detect(x) if ref is None else ref
    assert n_hops == len(ref), what
    undecidable = 0
    for k, (h, g) in enumerate(zip(ref, got[:n_hops])):
        w = f"{what}, hop {k}"
        t, f = int(g["tmax"]), int(g["f_ind"])
        assert 0 <= t < NMF and 0 <= f < 40, w
        assert abs(g["Dtmax12"] - h["cells"][t, f]) <= h["b12"][t, f], (w, g["Dtmax12"], h["cells"][t, f], h["b12"][t, f])      # the value of the cell it names
        assert abs(g["S1"] - h["S1"]) <= R.EPS * h["A1"] and abs(g["S2"] - h["S2"]) <= R.EPS * h["A2"], w
        assert g["Dthresh"] == KK * (g["S1"] + g["S2"]) or abs(g["Dthresh"] / (KK * (g["S1"] + g["S2"])) - 1) < 1e-14, w
        assert g["candidate"] == (np.float64(g["Dtmax12"]) > g["Dthresh"]), w
        lead = h["Dtmax12"] - h["second"]
        if h["Dtmax12"] == 0:
            assert (t, f, g["Dtmax12"], g["candidate"]) == (0, 0, 0.0, 0), w                    # an all-zero hop
            continue
        elif lead > h["b12"][h["tmax"], h["f_ind"]] + h["b12"].ravel()[h["second_at"]]:
            assert (t, f) == (h["tmax"], h["f_ind"]), (w, (t, f), (h["tmax"], h["f_ind"]))
        else:
            undecidable += 1
            continue
        if abs(h["Dtmax12"] - h["Dthresh"]) > h["b12"][h["tmax"], h["f_ind"]] + KK * R.EPS * (h["A1"] + h["A2"]):
            assert bool(g["candidate"]) == h["candidate"], w
        else:
            undecidable += 1
    return undecidable


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------------------------------
def test_surface(engines, torch_dev):
    """dt_dev against float64, every cell within RADE_ACQ_EPS A[t]: one 2112-sample stream (rows 0..1919 exist, nothing behind them is written) and the first three hops
    of rxtrace_mpp (rows 0..3839); then a row range that starts inside a block gives the same bits"""
    rng = np.random.default_rng(11)
    rows = [planted(rng, 2112, [(0, 700, 3)], noise=0.2), R.fixture_input("mpp")[:2112 + 2 * 961]]
    x, n = pack(rows)
    xd = dev(x, torch_dev)
    hops, nh, dt = engines(2).acq_detect(xd, n, dt_rows=(0, 4 * NMF))
    dt = dt.cpu().numpy()
    assert nh.tolist() == [1, 3]
    worst = 0.0
    for b, nr in ((0, 2 * NMF), (1, 4 * NMF)):
        want, A = R.surface(rows[b], 0, nr), R.weight(rows[b], 0, nr)
        frac = np.abs(dt[b, :nr] - want) / (R.EPS * A)
        worst = max(worst, float(frac.max()))
        assert np.all(dt[b, nr:] == 0), "rows behind the last block were written"
    print(f"surface: largest |dD| / bound {worst:.3g} (measured so far: {WORST_MEASURED})")
    assert worst <= 1.0
    _, _, part = engines(2).acq_detect(xd, n, dt_rows=(950, 100))
    assert np.array_equal(part.cpu().numpy().view(np.int32), dt[:, 950:1050].view(np.int32))
    assert np.abs(dt[1, 1920:1984] - R.fixture()["mpp_raw_hop2_Dt1"]).max() < 1e-5          # the script's own Dt1 of hop 2, in its convention


# ---- 2. the hop records of the fixture inputs -----------------------------------------------------------------------------------------------------------------------
def test_hop_records_of_the_fixture_inputs(engines, torch_dev):
    """all six inputs as one batch of unequal lengths, and each alone: equal bit for bit; against float64 at most one hop per recording may be undecidable"""
    rows = [R.fixture_input(k) for k in R.SIX]
    x, n = pack(rows)
    hops, nh = engines(6).acq_detect(dev(x, torch_dev), n)
    assert nh.tolist() == [30, 24, 26, 30, 10, 10]
    for b, name in enumerate(R.SIX):
        und = check_hops(rows[b], hops[b], nh[b], name, R.fixture_detect(name))
        print(f"{name}: {und} undecidable of {nh[b]} hops")
        assert und <= 1
        h1, n1 = engines(1).acq_detect(dev(rows[b][None], torch_dev))
        assert n1[0] == nh[b] and h1[0, :nh[b]].tobytes() == hops[b, :nh[b]].tobytes(), f"{name} alone differs from {name} in the batch"
        fx = R.fixture()
        assert np.array_equal(hops[b, :nh[b]]["tmax"], fx[f"{name}_raw_tmax"]) and np.array_equal(hops[b, :nh[b]]["f_ind"], fx[f"{name}_raw_f_ind"])      # the script's own
        assert np.array_equal(hops[b, :nh[b]]["candidate"], fx[f"{name}_raw_candidate"])
    again, _ = engines(6).acq_detect(dev(x, torch_dev), n)
    assert again.tobytes() == hops.tobytes()


# ---- 3. the smallest shapes ----------------------------------------------------------------------------------------------------------------------------------------
def test_planted_pilots_at_the_edges(engines, torch_dev):
    """timings 0, 15, 16, 63, 64, 959 (tile, wavefront and workgroup edges), frequencies 0 and 39, the last hop of a stream, exactly one hop and exactly two, an all-zero
    stream and one without a hop inside a batch; B = 1, 3 and 6 -- the issue's "one value above the number of workgroups a stream is split into" is the 6: a stream is 20
    wavefronts, 2.5 workgroups of eight -- (20 B wavefronts dealt eight to a workgroup: workgroups that span streams of different length, and a last
    one with idle wavefronts) give a stream the same bits"""
    rng = np.random.default_rng(12)
    plants = [[(0, 0, 0)], [(1, 959, 39)], [], [], [(0, 15, 39), (2, 16, 0)], [(1, 63, 39), (3, 64, 0)]]
    lens = [2112, 3073, 3000, 2000, 2112 + 3 * 961, 2112 + 3 * 961]
    rows = [planted(rng, L, pl) for L, pl in zip(lens, plants)]
    rows[2] = np.zeros(3000, np.complex64)
    x, n = pack(rows)
    hops, nh = engines(6).acq_detect(dev(x, torch_dev), n)
    assert nh.tolist() == [1, 2, 1, 0, 4, 4]
    for b in range(6):
        assert check_hops(rows[b], hops[b], nh[b], f"stream {b}") == 0
        for k, t, f in plants[b]:
            assert (hops[b, k]["tmax"], hops[b, k]["f_ind"], hops[b, k]["candidate"]) == (t, f, 1), (b, k)
    assert hops[2, 0].tolist() == (0.0, 0.0, 0, 0, 0, 0.0, 0.0)
    for B, pick in ((3, [4, 3, 1]), (1, [5])):
        xs, ns = pack([rows[b] for b in pick])
        h2, n2 = engines(B).acq_detect(dev(xs, torch_dev), ns)
        for j, b in enumerate(pick):
            assert n2[j] == nh[b] and h2[j, :nh[b]].tobytes() == hops[b, :nh[b]].tobytes(), (B, b)


def test_equal_cells_go_to_the_first(engines, torch_dev):
    """a stream of period 480: the samples under timing t and under t + 480 are the same, so are the wavefront's scale and every bit of the two cells, which lie in
    different wavefronts and (with eight wavefronts to a workgroup) in different workgroups.  The first in the script's order wins at every stage: inside a lane, across
    the lanes of a wavefront, across the twenty wavefronts of a hop.  Frequency ties inside one timing are pinned by the all-zero stream above (f_ind 0)"""
    rng = np.random.default_rng(5)
    x = np.tile((rng.standard_normal(480) + 1j * rng.standard_normal(480)).astype(np.complex64), 7)[:3073]
    hops, nh, dt = engines(1).acq_detect(dev(x[None], torch_dev), dt_rows=(0, 3 * NMF))
    dt = dt.cpu().numpy()[0]
    assert nh[0] == 2 and np.array_equal(dt[:480].view(np.int32), dt[480:960].view(np.int32)) and np.array_equal(dt[:960].view(np.int32), dt[960:1920].view(np.int32))
    ref = R.detect(x)
    for k in range(2):
        assert hops[0, k]["tmax"] < 480                                                         # the earlier of the two equal cells
        assert ref[k]["Dtmax12"] == ref[k]["second"] and ref[k]["tmax"] < 480                   # the reference has the tie too, and resolves it the same way
        if ref[k]["Dtmax12"] - np.sort(ref[k]["cells"].ravel())[-3] > 2 * ref[k]["b12"].max():  # the pair leads every other cell by more than the bound
            assert (hops[0, k]["tmax"], hops[0, k]["f_ind"]) == (ref[k]["tmax"], ref[k]["f_ind"])


# ---- 4. refine -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refine(engines, torch_dev):
    """the fixture's events, planted offsets of +3.25 Hz one sample either side of the coarse timing, and an event at t_abs = 0 (timing -1 is skipped)"""
    p, _ = R.consts()
    rng = np.random.default_rng(13)
    w = 2 * np.pi * 3.25 / 8000
    tone = 0.01 * (rng.standard_normal(4000) + 1j * rng.standard_normal(4000))
    for off in (0, 1500):
        for fr in (0, NMF):
            tone[off + fr:off + fr + M] += p * np.exp(1j * w * (fr + np.arange(M)))
    rows = [R.fixture_input(k) for k in R.RECORDINGS] + [tone.astype(np.complex64)]
    fx = R.fixture()
    events = [(b, NMF * int(h) + int(t), -50 + 2.5 * int(f)) for b, k in enumerate(R.RECORDINGS) for h, t, f in fx[f"{k}_raw_events"]]
    events += [(4, 1499, 2.5), (4, 1501, 5.0), (4, 0, 2.5), (4, 1, 5.0), (4, 3000, 0.0)]
    x, n = pack(rows)
    out, dfine = engines(5).acq_refine(dev(x, torch_dev), events, n, want_dfine=True)
    for (b, t_abs, fmax), g, d in zip(events, out, dfine):
        t, f, Dmax, d1, second = R.refine(rows[b], t_abs, fmax)
        assert abs(g["Dmax"] - Dmax) <= 1e-11 * max(Dmax, 1e-30) and np.abs(d - d1).max() <= 1e-11 * max(d1.max(), 1e-30), (b, t_abs)
        if Dmax - second > 1e-10 * Dmax or Dmax == 0:
            assert (g["t"], g["f"]) == (t, f), (b, t_abs, fmax)
    assert [(int(g["t"]), float(g["f"])) for g in out[-5:-1]] == [(1500, 3.25), (1500, 3.25), (0, 3.25), (0, 3.25)]
    assert (out[-1]["t"], out[-1]["f"], out[-1]["Dmax"]) == (3000, 0.0, 0.0)                    # no window fits behind sample 3000 of 4000
    k = len(fx["mpp_raw_events"])
    got = [(int(g["t"]) - NMF * int(e[0]), float(g["f"])) for g, e in zip(out[k:], fx["awgn_raw_events"])]
    assert got == [tuple(v) for v in fx["awgn_raw_refined"].tolist()]                        # the script's own refine


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpf", [False, True])
def test_acquire_end_to_end(engines, torch_dev, bpf):
    from radae_amd import acq
    tag = "bpf" if bpf else "raw"
    x, n = pack([R.fixture_input(k) for k in R.ALL])
    tg = np.array([R.TARGETS.get(k, (0.0, 1.0)) for k in R.ALL])
    res = acq.acquire(engines(8), dev(x, torch_dev), n, bpf=bpf, acq_test=True, fmax_target=tg[:, 0], acq_time_target=tg[:, 1])
    fx = R.fixture()
    for name, r in zip(R.ALL, res):
        ev = np.stack([r.events["hop"], r.events["tmax"], r.events["f_ind"]], 1).reshape(-1, 3)
        assert np.array_equal(ev, fx[f"{name}_{tag}_events"]), name
        passes, fails, pfail, mean, passed = fx[f"{name}_{tag}_stats"]
        assert (r.stats.passes, r.stats.fails, r.stats.passed) == (passes, fails, passed) and r.stats.mean_acq_time == mean, name
        assert np.array_equal(r.log["state"], fx[f"{name}_{tag}_state"]), name
    assert not res[4].stats.passed and not res[5].stats.passed and len(res[4].events) == len(res[5].events) == 0       # noise and the carrier do not acquire
    first = acq.acquire(engines(8), dev(x, torch_dev), n, bpf=bpf)                            # the script's normal run: the first acquisition only
    assert [len(r.events) for r in first] == [min(len(r.events), 1) for r in res] and first[0].stats is None


# ---- 6. the buffer contract ----------------------------------------------------------------------------------------------------------------------------------------
def test_buffer_contract(engines, torch_dev):
    """input rows in a sentinel buffer (NaN guards and gaps, odd stride, row 0 eight bytes off a 16-byte boundary): the input is untouched and no NaN reaches a result
    (nothing outside a stream's n samples is read); dt_dev in a sentinel buffer: only the rows that exist are written; records past a stream's hops keep their bytes"""
    from radae_amd.abi import AcqHop
    B, row = 3, 2112 + 961 + 40
    rng = np.random.default_rng(14)
    n = np.array([row, 2112, 2111], np.int32)
    vals = np.stack([planted(rng, row, [(0, 100 + b, 7)], noise=0.02) for b in range(B)])
    band = Band(B, row, row + 3, 8, torch_dev, base_offset_bytes=8).fill(vals)
    t0, nr = 900, 1100                                                                       # rows 900..1999: stream 0 has all (2 hops: 2880), stream 1 up to 1919, stream 2 none
    dtb = Band(B, nr * 40, nr * 40, 8, torch_dev, base_offset_bytes=8)                     # [B][n_rows][40] is dense: the guards stand in front and behind
    hops = np.zeros((B, 3), np.dtype(AcqHop))
    hops.view(np.uint8)[:] = 0xA5
    before = hops.tobytes()
    rc, hops, nh = raw_detect(engines(B), band.ptr, row + 3, n, hops=hops, max_hops=3, dt_ptr=dtb.ptr, t0=t0, n_rows=nr)
    assert rc == 0 and nh.tolist() == [2, 1, 0]
    band.check(what="x")
    assert np.array_equal(band.rows(np.complex64).view(np.int32), vals.view(np.int32))
    dtb.check(written=[nr * 40, (1920 - t0) * 40, 0], what="dt_dev")
    sz = hops.dtype.itemsize
    for b in range(B):
        assert hops[b].tobytes()[nh[b] * sz:] == before[(3 * b + nh[b]) * sz:3 * (b + 1) * sz], f"stream {b}: a record past its hops was written"
        assert check_hops(vals[b, :n[b]], hops[b], nh[b], f"stream {b}") == 0
    got = dtb.rows(np.complex64)[0].reshape(nr, 40)
    assert np.all(np.abs(got - R.surface(vals[0], t0, nr)) <= R.EPS * R.weight(vals[0], t0, nr))
    # refine reads its two windows only
    from radae_amd.abi import AcqRefined, AcqRefineIn
    from radae_amd.engine import _stream_ptr
    ev = np.zeros(2, np.dtype(AcqRefineIn)); ev[0] = (0, 100, 7 * 2.5 - 50); ev[1] = (1, 2112 - 1120, 0.0)
    out = np.zeros(2, np.dtype(AcqRefined))
    assert engines(B).lib.rade_batch_acq_refine(engines(B).h, C.c_void_p(band.ptr), row + 3, n.ctypes.data, ev.ctypes.data, 2, out.ctypes.data, None, _stream_ptr()) == 0
    band.check(what="x after refine")
    assert np.isfinite(out["Dmax"]).all() and out[0]["t"] == 100 and out[1]["t"] in (2112 - 1121, 2112 - 1120)      # t + 1 would read sample 2112 of stream 1


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engines, torch_dev):
    """argument checking on the host: each of these returns -1 before any launch, and hops_host, n_hops_host and dt_dev keep their bytes"""
    from radae_amd.abi import AcqHop, AcqRefined, AcqRefineIn
    from radae_amd.engine import _stream_ptr
    B, row = 3, 3100
    eng = engines(B)
    xin = Band(B, row, row + 1, 8, torch_dev).fill(planted(np.random.default_rng(15), B * row, []).reshape(B, row))
    dtb = Band(B, 64 * 40, 64 * 40, 8, torch_dev)
    hops = np.zeros((B, 2), np.dtype(AcqHop))
    hops.view(np.uint8)[:] = 0xA5
    nh = np.full(B, -7, np.int32)
    before = hops.tobytes()
    ok = dict(x_ptr=xin.ptr, x_stride=row + 1, n=row, hops=hops, max_hops=2, nh=nh, dt_ptr=dtb.ptr, t0=0, n_rows=64)
    nan = float("nan")
    bad = [dict(x_ptr=0), dict(x_ptr=xin.ptr + 4), dict(dt_ptr=dtb.ptr + 4), dict(null_n=True), dict(null_hops=True), dict(null_nh=True), dict(n=(row, -1, row)),
           dict(x_stride=row - 1), dict(max_hops=1), dict(max_hops=0), dict(t0=-1), dict(n_rows=0), dict(t0=row + 1 - 63), dict(pacq=0.0), dict(pacq=5.0), dict(pacq=-1e-5),
           dict(pacq=nan)]
    for kw in bad:
        rc, _, _ = raw_detect(eng, **{**ok, **kw})
        assert rc == -1, kw
        assert hops.tobytes() == before and np.all(nh == -7), kw
        dtb.untouched(what=f"dt_dev after {kw}")
    for kw in (dict(dt_ptr=None), dict(n=(row, 2111, 0)), dict(pacq=4.9), dict(x_ptr=xin.ptr + 8, x_stride=row, n=row - 1), dict()):
        rc, _, _ = raw_detect(eng, **{**ok, **kw})
        assert rc == 0, kw                                                         # ... and the same arguments without the fault are accepted
    assert nh.tolist() == [2, 2, 2]
    xin.check(what="x")
    ev = np.zeros(1, np.dtype(AcqRefineIn)); ev[0] = (0, 100, 0.0)
    out = np.zeros(1, np.dtype(AcqRefined)); out.view(np.uint8)[:] = 0xA5
    n = np.full(B, row, np.int32)
    call = lambda x=xin.ptr, nn=n.ctypes.data, e=ev.ctypes.data, k=1, o=out.ctypes.data: eng.lib.rade_batch_acq_refine(eng.h, C.c_void_p(x), row + 1, nn, e, k, o, None, _stream_ptr())
    for kw, val in (("x", 0), ("x", xin.ptr + 4), ("nn", None), ("e", None), ("o", None), ("k", -1)):
        assert call(**{kw: val}) == -1, kw
    for bad_ev in ((3, 100, 0.0), (-1, 100, 0.0), (0, 1 << 41, 0.0), (0, 100, nan)):
        ev[0] = bad_ev
        assert call() == -1, bad_ev
    assert np.all(out.view(np.uint8) == 0xA5)
    ev[0] = (0, 100, 0.0)
    assert call() == 0 and call(k=0) == 0
    with pytest.raises(RuntimeError):
        eng.acq_detect(dev(np.zeros((B, row), np.complex64), torch_dev), pacq_error1=7.0)


# ---- 8. the command line --------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_rx_prints_the_scripts_lines(torch_dev, tmp_path, capsys):
    """cli rx --acq_test --no_bpf on the recording that passes: the script's per-frame lines, its `Acquired!` lines, the summary and PASS; and --write_Dt writes Dt1"""
    from radae_amd import cli
    path, dt = str(tmp_path / "rx.f32"), str(tmp_path / "dt.c64")
    R.fixture_input("awgn320").tofile(path)
    assert cli.main(["rx", path, "--pilots", "--no_bpf", "--acq_test", "--fmax_target", "11", "--acq_time_target", "2", "--write_Dt", dt]) == 0
    out = capsys.readouterr().out.splitlines()
    fx = R.fixture()
    assert sum(ln.startswith("Acquired! Timing: 1 Freq: 1") for ln in out) == 3 and out[-2:] == ["PASS", "Acquisition failed...."]      # the script's own last line under --acq_test
    out = out[:-1]
    assert out[-2] == "Acq Test Passes: 3 Fails: 0 Pfail:  0.00 Mean Acq time:  1.00 s"
    frames = [ln for ln in out if " state: " in ln]
    assert len(frames) == 24 and frames[11].startswith("12 state: candidate ") and f"tmax: {fx['awgn320_raw_tmax'][11]:4d} tmax_candidate:   32 fmax:  10.00" in frames[11]
    d = np.fromfile(dt, np.complex64).reshape(24, 960, 40)
    assert np.abs(d[2, :8] - R.surface(R.fixture_input("awgn320"), 1920, 8)).max() <= R.EPS * R.weight(R.fixture_input("awgn320"), 1920, 8).max()
