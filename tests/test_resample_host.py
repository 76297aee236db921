"""CPU tests of the fractional resampler's definition (include/rade_batch.h: rade_batch_resample): the library's table and output count against the restatement
of tests/resample_ref.py, the design condition of the 32-tap / 256-phase / beta = 10 choice on a float64 model, and the restatement's linear mode against what the
reference's dsp.py:sample_clock_offset recorded in tests/golden/clock_offset.npz (oracle/golden/clock_offset.py).  The kernel itself is checked against the
same restatement and the same recording in tests/test_resample_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


def test_table(lib):
    """rade_resample_taps against the numpy restatement (np.i0) to one float32 ulp per entry; rows 0 and 256 exact impulses; every row sums to 1 within 32 x 2^-24"""
    from radae_amd import engine
    T = engine.resample_taps()
    assert T.dtype == np.float32 and T.shape == (257, 32)
    ref = rr.taps64().astype(np.float32)
    ulp = np.spacing(np.abs(ref))
    worst = float((np.abs(T.astype(np.float64) - ref.astype(np.float64)) / ulp).max())
    print(f"largest difference to the restatement: {worst:.3g} ulp")
    assert worst <= 1.0
    imp = np.zeros(32, np.float32); imp[15] = 1.0
    assert np.array_equal(T[0], imp) and np.array_equal(T[256], np.roll(imp, 1))
    sums = T.astype(np.float64).sum(1)
    print(f"row sums: 1 {sums.min() - 1:+.3g} .. 1 {sums.max() - 1:+.3g}")
    assert np.abs(sums - 1.0).max() <= 32 * 2.0 ** -24
    # g is even, so row 256 - p is row p read backwards (a property of the definition, not of how the sines are formed)
    assert np.abs(T[::-1, ::-1].astype(np.float64) - T.astype(np.float64)).max() <= 2.0 ** -23


def test_design_condition():
    """the float64 model of the definition on unit tones at 55 frequencies in +-2700 Hz, the step of an 8020 Hz receiver, t0 = 40.37, 4000 outputs well inside the input:
    worst error below 3e-5 (1.97e-5 measured).  Guards the parameters (32 taps, 256 phases, beta 10), not the kernel."""
    n_out, t0 = 4000, 40.37
    T = rr.taps64()
    i, mu = rr.positions(0, n_out, t0, rr.PPM_8020)
    pos = i + mu / 4294967296.0
    n = np.arange(int(pos.max()) + 40)
    worst = 0.0
    for f in np.linspace(-2700.0, 2700.0, 55):
        x = np.exp(2j * np.pi * f / 8000.0 * n)
        y, _ = rr.resample(x, n_out, rr.PPM_8020, t0, rr.SINC32, T=T)
        worst = max(worst, float(np.abs(y - np.exp(2j * np.pi * f / 8000.0 * pos)).max()))
    print(f"worst error on unit tones: {worst:.3g}")
    assert worst < 3e-5


@pytest.mark.parametrize("ppm", [0.0, 100.0, -100.0, -2493.77, 50000.0])
def test_count_against_a_brute_force_loop(lib, ppm):
    """rade_resample_count = the number of n >= 0 with t0_q + n step_q < in_end 2^32, counted one by one in Python integers"""
    for t0 in (0.0, 0.37, -3.0, -2.625, 1999.5, 2500.0):
        step_q, t0_q = rr.q32(t0, ppm)
        for in_end in (0, 1, 2000):
            n = 0
            while t0_q + n * step_q < in_end << 32:
                n += 1
            got = lib.rade_resample_count(in_end, t0, ppm)
            assert got == n == rr.count(in_end, t0, ppm), (ppm, t0, in_end, got, n)


def test_count_refusals(lib):
    """|ppm| > 50 000, a start that is not a number, and more outputs than 2^62 / step_q: -1.  The last one that fits is still counted."""
    from radae_amd import engine
    assert lib.rade_resample_count(2000, 0.0, 60000.0) == -1 and lib.rade_resample_count(2000, 0.0, -50000.5) == -1
    assert lib.rade_resample_count(2000, float("nan"), 0.0) == -1 and lib.rade_resample_count(2000, 0.0, float("nan")) == -1
    assert lib.rade_resample_count(1 << 30, 0.0, 0.0) == 1 << 30                 # n step_q = 2^62 exactly: not past it
    assert lib.rade_resample_count((1 << 30) + 1, 0.0, 0.0) == -1
    assert lib.rade_resample_count(1 << 30, 0.0, -100.0) == -1                   # a slower step needs more than 2^62 / step_q outputs for the same input
    assert lib.rade_resample_count((1 << 30) - 2, 0.0, 100.0) == rr.count((1 << 30) - 2, 0.0, 100.0) > 0
    with pytest.raises(ValueError):
        engine.resample_count(2000, 0.0, 60000.0)
    assert engine.resample_count(2000, -3.0, 0.0) == 2003


def test_restatement_linear_mode_reproduces_the_reference(golden):
    """the outputs dsp.py:sample_clock_offset produced (those with tin + 1 < len) within (N 2^-33 + N^2 2^-52) max |dx| + 4 x 2^-24 max |x|; what it did not produce it left 0"""
    g = golden("clock_offset")
    x = g["x"]
    assert x.dtype == np.complex64 and x.shape == (2000,) and os.path.getsize(os.path.join(REPO, "tests", "golden", "clock_offset.npz")) < 100 << 10
    assert g["ppm"][0] == 100.0 and g["ppm"][1] == -625.0 and g["ppm"][2] == rr.PPM_8020
    for k, ppm in enumerate(g["ppm"]):
        n = int(g["n"][k])
        assert n in (1999, 2000) and np.all(g["y"][k, n:] == 0)
        y, _ = rr.resample(x, n, float(ppm), 0.0, rr.LINEAR)
        err = float(np.abs(y - g["y"][k, :n]).max())
        tol = rr.reference_bound(n, x)
        print(f"ppm {ppm:+.2f}: {n} outputs, max |dy| {err:.3g}, bound {tol:.3g}")
        assert err <= tol
        assert n == min(2000, rr.count(1999, 0.0, float(ppm)))      # an output is produced while tin + 1 < len and the output array has room


def test_ppm_from_rates():
    from radae_amd import engine
    assert engine.ppm_from_rates(8000, 8020) == (8000 / 8020 - 1) * 1e6 == rr.PPM_8020
    assert engine.ppm_from_rates(8000, 8000) == 0.0 and engine.ppm_from_rates(8000, 7995) > 0


def test_resample_symbols_are_declared_and_exported(lib):
    from radae_amd import engine
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    for s in ("rade_batch_resample", "rade_resample_count", "rade_resample_taps"):
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert "int rade_batch_resample(rade_batch *h," in hdr and "enum { RADE_RESAMPLE_SINC32 = 0, RADE_RESAMPLE_LINEAR = 1 };" in hdr
    assert hasattr(engine.BatchEngine, "resample") and hasattr(engine, "ClockOffset")
    assert C.sizeof(engine.ResampleParams) == 48
