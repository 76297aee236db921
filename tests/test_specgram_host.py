"""CPU tests of the spectrogram stage's definition (include/rade_batch.h: rade_batch_specgram, rade_specgram_plan, _slices, _window, _levels): the library's host
functions against the formulas, the float64 restatement of tests/specgram_ref.py against scipy.signal.spectrogram on what does not rest on the recalled Octave facts, the
float32 factorisation the header states against the restatement, and the PNG writer.  The kernel itself is held to the same restatement in tests/test_specgram_gpu.py."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import specgram_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


def test_specgram_symbols_are_declared_and_exported(lib):
    from radae_amd import cli, engine, ota
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    for s in ("rade_batch_specgram", "rade_specgram_plan", "rade_specgram_slices", "rade_specgram_window", "rade_specgram_levels"):
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert "int rade_batch_specgram(rade_batch *h, const void *x_dev, long x_stride, const int *n_host, int format, float gain," in hdr
    assert "int rade_specgram_plan(const rade_specgram_params *p, rade_specgram_plan_t *out);" in hdr and "long long rade_specgram_slices(long long n);" in hdr
    assert "void rade_specgram_window(float *out /* [1280] */);" in hdr and "int rade_specgram_levels(double lo, double hi, float *out /* [255] */);" in hdr
    block = hdr[hdr.index("the spectrogram of a recording"):]
    assert "DEVIATION" in block and "RECALLED, NOT VERIFIED" in block
    assert hasattr(engine.BatchEngine, "specgram") and all(hasattr(engine, f) for f in ("specgram_plan", "specgram_slices", "specgram_window", "specgram_levels"))
    assert hasattr(ota, "write_png") and "spectrogram" in ota.process_rx.__code__.co_varnames and hasattr(cli, "_specgram")
    assert C.sizeof(engine.SpecgramParams) == 40 and C.sizeof(engine.SpecgramPlan) == 24


@pytest.mark.parametrize("n", [0, 1280, 1281, 1440, 1441, 1600, 1601, 80000, 806400])
def test_slices(lib, n):
    from radae_amd import engine
    assert engine.specgram_slices(n) == len(np.arange(0, n - 1280, 160)) == len(sr.starts(n))


@pytest.mark.parametrize("fmin,fmax,k0,k1", [(0.0, 3000.0, 1, 768), (200.0, 3000.0, 52, 768), (0.0, 4000.0, 1, 1023), (3.9, 3.91, 1, 1)])
def test_plan(lib, fmin, fmax, k0, k1):
    from radae_amd import engine
    q = engine.specgram_plan(fmin, fmax)
    assert (q.k0, q.k1) == (k0, k1) == sr.band(fmin, fmax) and q.n_bins == k1 - k0 + 1
    assert (q.k0, q.k1) == (max(1, int(np.ceil(fmin * 2048 / 8000))), min(1023, int(np.floor(fmax * 2048 / 8000))))
    assert (q.win, q.step, q.nfft) == (1280, 160, 2048)


def test_plan_refusals(lib):
    from radae_amd import engine
    nan, inf = float("nan"), float("inf")
    for kw in (dict(fmin=nan), dict(fmax=inf), dict(lo=nan), dict(hi=inf), dict(fmin=3000.0, fmax=200.0), dict(fmin=3.91, fmax=7.8), dict(fmin=4000.0, fmax=4000.0),
               dict(fmin=-10.0, fmax=0.0), dict(lo=0.0), dict(lo=-0.1), dict(lo=0.6, hi=0.5), dict(lo=0.5, hi=0.5), dict(hi=1.5)):
        with pytest.raises(ValueError):
            engine.specgram_plan(**kw)
    assert lib.rade_specgram_plan(None, C.byref(engine.SpecgramPlan())) == -1
    assert lib.rade_specgram_plan(C.byref(engine.SpecgramParams(0.0, 3000.0, sr.LO, sr.HI, None)), None) == -1
    assert engine.specgram_plan(hi=1.0).n_bins == 768 and engine.specgram_plan(-500.0, 3000.0).k0 == 1
    for lo, hi in ((0.0, 0.5), (0.5, 0.5), (0.1, 1.5), (nan, 0.5)):
        with pytest.raises(ValueError):
            engine.specgram_levels(lo, hi)
    assert lib.rade_specgram_levels(0.01, 0.5, None) == -1


def test_window(lib):
    from radae_amd import engine
    w = engine.specgram_window()
    want = (0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(1280) + 1) / 1281)).astype(np.float32)
    assert w.dtype == np.float32 and np.array_equal(w.view(np.int32), want.view(np.int32))
    assert w.min() > 0 and abs(float(w[639]) - 1.0) < 2e-6                       # no zero end points


def test_levels(lib):
    from radae_amd import engine
    for lo, hi in ((sr.LO, sr.HI), (1e-3, 1.0)):
        T = engine.specgram_levels(lo, hi)
        want = (lo * (hi / lo) ** ((np.arange(1, 256) - 0.5) / 255)).astype(np.float32)
        assert np.array_equal(T.view(np.int32), want.view(np.int32))
        assert (np.diff(T) > 0).all() and T[0] > lo and T[254] < hi


def test_restatement_against_scipy():
    """scipy.signal.spectrogram with the same window, hop and transform length makes the same slices plus the one at s = n - 1280 exactly when 160 divides n - 1280 (Octave's
    range ends below it): mags / peak agree within 1e-10 on the slices both have"""
    from scipy import signal
    rng = np.random.default_rng(7)
    w = sr.window()
    for n in (1441, 1600, 2401, 8000, 8037):
        x = np.rint(9000 * rng.standard_normal(n))
        m = sr.mags(x)
        f, t, S = signal.spectrogram(x, 8000, window=w, nperseg=1280, noverlap=1120, nfft=2048, detrend=False, mode="magnitude")
        S = S[1:1024].T                                                            # [slices, bins 1..1023]
        extra = 1 if (n - 1280) % 160 == 0 else 0
        assert len(S) == len(m) + extra == (n - 1280) // 160 + 1
        both = len(m)
        assert np.abs(m / m.max() - S[:both] / S[:both].max()).max() < 1e-10
        assert np.allclose(t[:both] * 8000 - 640, sr.starts(n))


def test_stated_factorisation_is_the_transform(lib):
    """the float32 arithmetic the header states (pairs, five radix-4 stages, the radix-2 stage, the separation), written out in NumPy, stays under the header's bound"""
    from radae_amd import engine
    t = np.exp(-2j * np.pi * np.arange(2048) / 2048)
    t32 = (t.real.astype(np.float32) + 1j * t.imag.astype(np.float32)).astype(np.complex64)
    rng = np.random.default_rng(8)
    x = np.rint(9000 * rng.standard_normal(2081)).astype(np.float32)              # 6 slices
    for sig in (x, x[:1761], x[:1601]):                                            # 6 slices, 4, and 3 (the last one without a partner)
        got, ref, S = sr.stated_mags(sig, engine.specgram_window(), t32), sr.mags(sig), sr.pair_sums(sig)
        assert got.shape == ref.shape and (np.abs(got - ref) <= sr.GAMMA * S[:, None]).all()


def test_levels_rule():
    T = sr.levels_table().astype(np.float32)
    pk = np.float32(1234.5)
    m = np.array([0.0, T[0] * pk, np.nextafter(T[0] * pk, np.float32(0)), T[254] * pk, pk, np.float32(np.nan)], np.float32)
    assert sr.levels(m, pk, T).tolist() == [0, 1, 0, 255, 255, 0]
    assert not sr.levels(m, 0.0, T).any()


def test_write_png_round_trip(tmp_path):
    from radae_amd import ota
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (11, 7)).astype(np.uint8)                            # 11 slices of 7 bins; only 9 count
    path = str(tmp_path / "a.png")
    ota.write_png(path, img, 9)
    d = open(path, "rb").read()
    assert d[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(d):
        ln, tag = struct.unpack(">I", d[pos:pos + 4])[0], d[pos + 4:pos + 8]
        body = d[pos + 8:pos + 8 + ln]
        assert struct.unpack(">I", d[pos + 8 + ln:pos + 12 + ln])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + ln
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (9, 7, 8, 0, 0, 0, 0)          # width = slices, height = bins, 8-bit grey
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(7, 10)
    assert not raw[:, 0].any()                                                       # filter 0 on every row
    pix = raw[:, 1:]
    assert pix[0, 0] == img[0, 6] and pix[6, 0] == img[0, 0] and pix[0, 8] == img[8, 6]     # frequency upward, time to the right
    assert np.array_equal(pix, img[:9].T[::-1])
