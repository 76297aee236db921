"""CPU tests of the rational rate converter's definition (include/rade_batch.h: rade_batch_rate_convert): the library's table and output count against the restatement
of tests/rate_ref.py, the quality of the definition on the library's float32 table (tones of the modem's band at every phase, the prototype's stop band), and the
restatement against scipy.signal.upfirdn where scipy is installed.  The kernel itself is checked against the same restatement in tests/test_rate_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import rate_ref as rf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(1, 6), (6, 1), (80, 441), (441, 80), (2, 3), (1, 1)]
TONE_RATIOS = [(1, 6), (6, 1), (80, 441), (441, 80), (1, 2), (2, 3)]


def rates(L, M):
    """(Fin, Fout) in Hz: the modem's 8 kHz is the output of a down-conversion and the input of an up-conversion"""
    return (8000.0 * M / L, 8000.0) if M > L else (8000.0, 8000.0 * L / M)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


def test_rate_symbols_are_declared_and_exported(lib):
    from radae_amd import engine
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    for s in ("rade_batch_rate_convert", "rade_rate_count", "rade_rate_taps"):
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert "int rade_batch_rate_convert(rade_batch *h," in hdr and "enum { RADE_RATE_C64 = 0, RADE_RATE_S16_REAL = 1, RADE_RATE_S16_IQ = 2 };" in hdr
    assert "long long rade_rate_count(long long in_end, int L, int M);" in hdr and "int rade_rate_taps(int L, int M, float *out);" in hdr
    assert hasattr(engine.BatchEngine, "rate_convert") and hasattr(engine, "RateConverter") and hasattr(engine, "rate_count") and hasattr(engine, "rate_taps")
    assert C.sizeof(engine.RateParams) == 24
    assert (engine.RATE_C64, engine.RATE_S16_REAL, engine.RATE_S16_IQ) == (rf.C64, rf.S16_REAL, rf.S16_IQ) == (0, 1, 2)


@pytest.mark.parametrize("L,M", RATIOS)
def test_table(lib, L, M):
    """rade_rate_taps against the numpy restatement (np.i0) to one float32 ulp per entry; for M <= L row 0 is the exact unit impulse at j = 15; every row sums to 1
    within T x 2^-24; a common factor of L and M changes nothing; out == NULL only queries T"""
    from radae_amd import engine
    Lr, Mr, K, T = rf.reduce(L, M)
    assert lib.rade_rate_taps(L, M, None) == T == 32 * K
    Ct = engine.rate_taps(L, M)
    assert Ct.dtype == np.float32 and Ct.shape == (Lr, T)
    ref = rf.taps64(L, M).astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(ref), np.float32(2.0 ** -126)))
    worst = float((np.abs(Ct.astype(np.float64) - ref.astype(np.float64)) / ulp).max())
    print(f"{L}/{M}: T {T}, {Lr * T} floats, largest difference to the restatement: {worst:.3g} ulp")
    assert worst <= 1.0
    if M <= L:
        imp = np.zeros(32, np.float32); imp[15] = 1.0
        assert T == 32 and np.array_equal(Ct[0], imp)               # (zeros of either sign: a product with them adds nothing to the sum)
    sums = Ct.astype(np.float64).sum(1)
    print(f"row sums: 1 {sums.min() - 1:+.3g} .. 1 {sums.max() - 1:+.3g}")
    assert np.abs(sums - 1.0).max() <= T * 2.0 ** -24
    assert np.array_equal(engine.rate_taps(3 * L, 3 * M), Ct)


def test_table_of_the_unit_ratio_is_row_0_of_the_resampler(lib):
    from radae_amd import engine
    assert np.array_equal(engine.rate_taps(1, 1)[0], engine.resample_taps()[0])
    assert np.array_equal(engine.rate_taps(7, 7), engine.rate_taps(1, 1))


def test_sizes_the_header_admits_and_refuses(lib):
    """T and table size of the ratios the header lists; K > 8, L T > 16384 floats, L or M < 1 are refused by the table function as by the call"""
    from radae_amd import engine
    for (L, M), (T, floats) in {(1, 6): (192, 192), (6, 1): (32, 192), (80, 441): (192, 15360), (441, 80): (32, 14112), (1, 2): (64, 64), (2, 3): (64, 128),
                                (3, 2): (32, 96), (1, 8): (256, 256), (512, 1): (32, 16384), (160, 882): (192, 15360)}.items():
        assert lib.rade_rate_taps(L, M, None) == T and engine.rate_taps(L, M).size == floats, (L, M)
    for L, M in [(1, 9), (2, 17), (513, 1), (0, 1), (1, 0), (-1, 6), (1, -6), (200, 441)]:
        assert lib.rade_rate_taps(L, M, None) == -1, (L, M)
    with pytest.raises(ValueError):
        engine.rate_taps(1, 9)


@pytest.mark.parametrize("L,M", [(1, 6), (6, 1), (80, 441), (441, 80), (2, 3), (1, 1), (4, 12)])
def test_count_against_a_brute_force_loop(lib, L, M):
    """rade_rate_count = the number of n >= 0 with n M < in_end L, counted one by one in Python integers"""
    for in_end in (-3, 0, 1, 2, 5, 6, 7, 441, 442, 2000):
        n = 0
        while n * M < in_end * L:
            n += 1
        got = lib.rade_rate_count(in_end, L, M)
        assert got == n == rf.count(in_end, L, M), (L, M, in_end, got, n)


def test_count_refusals(lib):
    from radae_amd import engine
    assert lib.rade_rate_count(100, 0, 1) == -1 and lib.rade_rate_count(100, 1, 0) == -1 and lib.rade_rate_count(100, -1, 1) == -1
    assert lib.rade_rate_count(1 << 62, 1, 1) == 1 << 62                           # n M = 2^62 exactly: not past it
    assert lib.rade_rate_count((1 << 62) + 1, 1, 1) == -1
    assert lib.rade_rate_count(1 << 61, 6, 1) == -1 and lib.rade_rate_count((1 << 62) - 4, 1, 6) == rf.count((1 << 62) - 4, 1, 6) > 0
    with pytest.raises(ValueError):
        engine.rate_count(100, 0, 1)
    assert engine.rate_count(480000, 1, 6) == 80000 and engine.rate_count(441000, 80, 441) == 80000 and engine.rate_count(80000, 6, 1) == 480000


@pytest.mark.parametrize("L,M", TONE_RATIOS)
def test_tones_of_the_modem_band_at_every_phase(lib, L, M):
    """the library's float32 table in float64 arithmetic on unit tones at 55 frequencies in +-2700 Hz, outputs well inside the input and through every phase of the
    table: worst error below 2e-5 (1.43e-5 for the worst ratio in float64).  Guards the parameters of the definition (32 K taps, beta 10, cut-off), not the kernel."""
    from radae_amd import engine
    Ct = engine.rate_taps(L, M)
    Lr, Mr, K, T = rf.reduce(L, M)
    Fin, _ = rates(L, M)
    n_out = Lr + 60
    n0 = -(-(T * Lr) // Mr)                                        # the first window starts at or behind sample T / 2
    i, ph = rf.positions(n0, n_out, L, M)
    assert set(ph.tolist()) == set(range(Lr)) and i[0] >= T // 2
    k = np.arange(int(i[-1]) + T)
    pos = i + ph / Lr
    worst = 0.0
    for f in np.linspace(-2700.0, 2700.0, 55):
        y, _ = rf.convert(np.exp(2j * np.pi * f / Fin * k), n_out, L, M, n0=n0, C=Ct)
        worst = max(worst, float(np.abs(y - np.exp(2j * np.pi * f / Fin * pos)).max()))
    print(f"{L}/{M}: worst error on unit tones {worst:.3g}")
    assert worst < 2e-5


@pytest.mark.parametrize("L,M", TONE_RATIOS)
def test_prototype_stop_band(lib, L, M):
    """the float32 table laid out as one filter at the rate L Fin: its response, relative to DC, is at most -95 dB from 0.6 x min(Fin, Fout) up to L Fin / 2
    (-99.1 dB for the worst ratio) -- what aliases into, or images of, the 8 kHz band"""
    from radae_amd import engine
    Ct = engine.rate_taps(L, M)
    Lr = Ct.shape[0]
    Fin, Fout = rates(L, M)
    p = rf.prototype(Ct, Lr)
    nfft = 1 << 19
    Hf = np.abs(np.fft.rfft(p, nfft)) / p.sum()
    f = np.arange(len(Hf)) * (Lr * Fin / nfft)
    stop = f >= 0.6 * min(Fin, Fout)
    worst = 20.0 * np.log10(Hf[stop].max())
    print(f"{L}/{M}: stop band from {0.6 * min(Fin, Fout):.0f} Hz: {worst:.1f} dB")
    assert stop.any() and worst <= -95.0


@pytest.mark.parametrize("L,M", [(1, 6), (6, 1), (80, 441), (441, 80), (2, 3), (3, 2)])
def test_restatement_equals_upfirdn(L, M):
    """the restatement (float64 table) against scipy.signal.upfirdn with the prototype laid out at the rate L Fin: y[n] = sum_k h[n M + d - k L] x[k] with h the
    time-reversed prototype and d = (T / 2) L; upfirdn starts its outputs at n M, so h gets z = q M - d leading zeros, q = ceil(d / M), and y[n] is upfirdn's n + q"""
    signal = pytest.importorskip("scipy.signal")
    Lr, Mr, K, T = rf.reduce(L, M)
    rng = np.random.default_rng(3)
    n_in = 900 if M > L else 150
    x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
    C64 = rf.taps64(L, M)
    n_out = rf.count(n_in, L, M)
    y, _ = rf.convert(x, n_out, L, M, C=C64)
    d = (T // 2) * Lr
    q = -(-d // Mr)
    h = np.concatenate([np.zeros(q * Mr - d), rf.prototype(C64, Lr)[::-1]])
    yu = signal.upfirdn(h, x, up=Lr, down=Mr)
    assert len(yu) >= n_out + q
    err = float(np.abs(yu[q:q + n_out] - y).max())
    print(f"{L}/{M}: {n_out} outputs, max difference to upfirdn {err:.3g}")
    assert err <= 1e-12
