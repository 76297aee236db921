"""CPU tests of the chirp C/No stage's definition (include/rade_batch.h: rade_batch_cno_est, rade_cno_plan, rade_chirp): the float64 restatement of tests/cno_ref.py
against what the reference's est_CNo.py and chirp.py printed and wrote (tests/golden/cno.npz, oracle/golden/cno.py), the library's host functions against the
restatement, and the block identity the kernel rests on.  The kernel itself is held to the same restatement in tests/test_cno_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import cno_ref as cr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "cno.npz")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def have_device():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_cno_symbols_are_declared_and_exported(lib):
    from radae_amd import engine, ota
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    for s in ("rade_batch_cno_est", "rade_cno_plan", "rade_chirp"):
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert "int rade_batch_cno_est(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, const rade_cno_params *p," in hdr
    assert "int rade_cno_plan(const rade_cno_params *p, rade_cno_plan_t *out);" in hdr and "int rade_chirp(float *iq_out /* [nsam][2] */, int nsam, double flow, double fhigh, double amp);" in hdr
    assert "DEVIATION" in hdr[hdr.index("C/No of the chirp header"):]
    assert hasattr(engine.BatchEngine, "cno_est") and hasattr(engine, "cno_plan") and hasattr(engine, "chirp")
    assert hasattr(ota, "process_rx") and hasattr(ota, "ota_header")
    assert C.sizeof(engine.CnoParams) == 24 and C.sizeof(engine.CnoPlan) == 28 and C.sizeof(engine.CnoResult) == 32


@pytest.mark.parametrize("k", [0, 1, 2])
def test_restatement_against_the_scripts_output(golden, k):
    """cno_ref on the golden recordings: the lines it would print equal the lines est_CNo.py printed (window list, %5.2f / %6.2f values), apart from the listed window of
    the noise-only recording whose C is too close to 0 to pin its sign"""
    rx = cr.int16_zeropad(golden[f"rec{k}"])
    r = cr.est(rx, float(golden["window_time"][k]))
    mine, theirs = cr.lines(r), [str(l) for l in golden[f"text{k}"]]
    skip = [f"time: {int(st):8d}" for st in (golden["skip2"] if k == 2 else [])]
    drop = lambda ls: [l for l in ls if not any(l.startswith(s) for s in skip)]
    assert drop(mine) == drop(theirs)
    assert np.array_equal(r["st"], golden[f"st{k}"]) or k == 2
    m = golden["measured"][k]
    assert f"{r['max_st'] / cr.FS:5.2f}" == f"{m[0]:5.2f}" and f"{r['max_CNodB']:6.2f}" == f"{m[1]:6.2f}" and f"{r['max_SNRdB']:6.2f}" == f"{m[2]:6.2f}"


def test_chirp_against_the_script(lib, golden):
    """rade_chirp and the restatement against chirp.py's 2.5 s file: at most 1 float32 ulp per component (libm's and NumPy's cos / sin may differ in the last place of the
    double); the number of differing samples is reported, 0 expected"""
    from radae_amd import engine
    want = golden["chirp"]
    assert np.array_equal(cr.chirp(2.5), want)
    got = engine.chirp(2.5)
    assert got.dtype == np.complex64 and got.shape == want.shape
    differing = int((got != want).sum())
    print(f"rade_chirp: {differing} of {len(want)} samples differ from chirp.py's")
    for part in ("real", "imag"):
        g, w = getattr(got, part), getattr(want, part)
        assert np.all(np.abs(g.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)))
    # the sweep turns twice in 2.5 s at the defaults: 1 s up, 1 s down, 0.5 s up
    other = engine.chirp(0.3, 500.0, 900.0, 0.5)
    assert np.array_equal(other, cr.chirp(0.3, 500.0, 900.0, 0.5)) and abs(np.abs(other).max() - 0.5) < 1e-7
    buf = np.zeros(8, np.float32)
    assert lib.rade_chirp(None, 4, 400.0, 2000.0, 0.25) == -1 and lib.rade_chirp(buf.ctypes.data, -1, 400.0, 2000.0, 0.25) == -1
    for bad in ((float("nan"), 2000.0, 0.25), (400.0, float("inf"), 0.25), (400.0, 2000.0, float("nan"))):
        assert lib.rade_chirp(buf.ctypes.data, 4, *bad) == -1
    assert not buf.any() and lib.rade_chirp(buf.ctypes.data, 0, 400.0, 2000.0, 0.25) == 0


@pytest.mark.parametrize("window_time,flow,fhigh", [(4.0, 400.0, 2000.0), (0.25, 400.0, 2000.0), (1.0, 400.0, 2000.0), (8.0, 400.0, 2000.0), (2.0, 700.3, 1333.7), (0.5, 0.0, 100.0)])
def test_plan_against_python_int(lib, window_time, flow, fhigh):
    from radae_amd import engine
    q = engine.cno_plan(window_time, flow, fhigh)
    N, flow_bin, fhigh_bin, noise_st, noise_en = cr.plan(window_time, flow, fhigh)
    assert (q.N, q.J, q.flow_bin, q.fhigh_bin, q.noise_st, q.noise_en) == (N, N // 2000, flow_bin, fhigh_bin, noise_st, noise_en)
    assert q.n_bins == (fhigh_bin - flow_bin) + (noise_en - noise_st)
    if (window_time, flow, fhigh) == (4.0, 400.0, 2000.0):
        assert (q.N, q.J, q.n_bins, q.flow_bin, q.fhigh_bin, q.noise_st, q.noise_en) == (32000, 16, 7200, 1600, 8000, 8800, 9600)


def test_plan_refusals(lib):
    """every refusal of the header: values that are not finite; N not a positive multiple of 2000 or J > 32 (the one deviation from the script); flow_bin >= fhigh_bin;
    (int)(0.1 fhigh_bin) < 1; noise_en > N; a negative flow; bands wider than the kernel's ring; NULL"""
    from radae_amd import engine
    q = engine.CnoPlan()
    call = lambda wt=4.0, fl=400.0, fh=2000.0: lib.rade_cno_plan(C.byref(engine.CnoParams(wt, fl, fh)), C.byref(q))
    assert call() == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(wt=nan), dict(wt=inf), dict(fl=nan), dict(fh=inf), dict(fl=-inf),
               dict(wt=0.0), dict(wt=-4.0), dict(wt=0.1), dict(wt=0.3), dict(wt=8.25), dict(wt=1e12),
               dict(fl=2000.0), dict(fl=2500.0), dict(fh=400.0),
               dict(wt=0.25, fl=0.0, fh=36.0),                     # fhigh_bin 9: (int)(0.9) = 0 bins of noise
               dict(fl=-400.0), dict(fh=1e300)):
        assert call(**kw) == -1, kw
    # noise_en > N exactly at the edge: N = 2000, fhigh_bin = 1667 -> noise_en = 1667 + 166 + 166 = 1999 <= 2000 passes; 1675 -> 1675 + 167 + 167 = 2009 refused
    assert call(wt=0.25, fl=1500.0, fh=6668.0) == 0 and (q.fhigh_bin, q.noise_en) == (1667, 1999)
    assert call(wt=0.25, fl=1500.0, fh=6700.0) == -1
    # the ring: J (ceil(wc / J) + ceil(wn / J)) <= 16000
    assert call(wt=8.0, fl=400.0, fh=2100.0) == 0 and call(wt=8.0, fl=100.0, fh=2200.0) == -1
    assert lib.rade_cno_plan(None, C.byref(q)) == -1 and lib.rade_cno_plan(C.byref(engine.CnoParams(4.0, 400.0, 2000.0)), None) == -1
    with pytest.raises(ValueError):
        engine.cno_plan(0.3)


@pytest.mark.parametrize("J", [1, 2, 16])
def test_block_identity(J):
    """B_b[k] = DFT_H(x[b H + n] e^{-2 pi i r n / N})[q], X_w[k] = sum_j e^{-2 pi i r j / J} B_{w+j}[k] against np.fft.fft of the window, in float64, on the second
    window of a random signal: relative difference below 1e-9 (3e-8 would be single precision)"""
    N = 2000 * J
    rng = np.random.default_rng(J)
    x = rng.standard_normal(N + 4000) + 1j * rng.standard_normal(N + 4000)
    X = cr.window_by_blocks(x, 2000, N)
    ref = np.fft.fft(x[2000:2000 + N])
    d = float(np.abs(X - ref).max() / np.abs(ref).max())
    print(f"J {J}: largest difference to np.fft.fft, relative to the largest bin: {d:.3g}")
    assert d < 1e-9


def test_window_counts():
    """np.arange(0, n - N, 2000): n = N none, N + 1 .. N + 2000 one, N + 2001 two -- the restatement, the engine's count and the band sums' shape"""
    from radae_amd import engine
    N = 2000
    for n, want in ((N, 0), (N + 1, 1), (N + 2000, 1), (N + 2001, 2), (N - 5, 0), (N + 4001, 3)):
        assert len(cr.starts(n, N)) == want == engine.cno_windows(n, N), n
    assert cr.band_sums(np.ones(N + 2001, np.complex64), 0.25).shape == (2, 2) and cr.band_sums(np.ones(N, np.complex64), 0.25).shape == (0, 2)
    r = cr.finish(np.zeros((0, 2)), 0.25)
    assert (r["n_windows"], r["max_st"], r["max_CNodB"]) == (0, 0, 0.0) and abs(r["max_SNRdB"] + 10 * np.log10(3000)) < 1e-12


def test_layout_of_a_trimmed_recording():
    """ota_test.sh:151-158: x = (duration - 6) / 2, SSB at 5 s for x s, RADAE from 5 + x s, to the nearest sample"""
    from radae_amd import ota
    assert ota.layout(6 * 8000 + 2 * 24000) == (40000, 24000, 64000)
    assert ota.layout(6 * 8000 + 2 * 24000 + 1) == (40000, 24001, 64001)        # half a sample: upward
    assert ota.layout(6 * 8000) == (40000, 0, 40000)
    with pytest.raises(ValueError):
        ota.layout(6 * 8000 - 1)
    h = ota.ota_header(0.1)
    assert h.shape == (36000,) and h.dtype == np.complex64 and np.array_equal(h, cr.chirp(4.5, amp=0.1))


def test_cli_chirp(lib, golden, tmp_path):
    from radae_amd import cli
    out = tmp_path / "c.f32"
    assert cli.main(["chirp", str(out), "2.5"]) == 0
    got = np.fromfile(out, np.complex64)
    assert got.shape == golden["chirp"].shape and np.abs(got - golden["chirp"]).max() <= 2.0 ** -25
    assert cli.main(["chirp", str(out), "0.01", "--flow", "500", "--fhigh", "900", "--amp", "0.5"]) == 0
    assert np.array_equal(np.fromfile(out, np.complex64), cr.chirp(0.01, 500.0, 900.0, 0.5))


@pytest.mark.skipif(not have_device(), reason="est_cno runs its periodograms on the device")
@pytest.mark.parametrize("k", [0, 1, 2])
def test_cli_est_cno(lib, golden, tmp_path, capsys, k):
    """`cli est_cno` on the golden recordings prints what est_CNo.py printed (apart from the listed window)"""
    from radae_amd import cli
    path = tmp_path / "rx.f32"
    cr.int16_zeropad(golden[f"rec{k}"]).tofile(path)
    capsys.readouterr()
    assert cli.main(["est_cno", str(path), "--window_time", str(float(golden["window_time"][k]))]) == 0
    mine = [l for l in capsys.readouterr().out.split("\n") if l.strip()]
    skip = [f"time: {int(st):8d}" for st in (golden["skip2"] if k == 2 else [])]
    drop = lambda ls: [l for l in ls if not any(l.startswith(s) for s in skip)]
    assert drop(mine) == drop([str(l) for l in golden[f"text{k}"]])
