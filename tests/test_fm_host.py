"""CPU tests of the analog FM stage's definition (include/rade_batch.h: rade_batch_fm_mod, rade_batch_fm_demod): the numpy least-squares design of tests/fm_ref.py against
scipy.signal.firls where scipy is installed, the library's rade_fm_taps / rade_fm_sigma / rade_fm_deemph_len against the restatement, the 32-bit NCO against fm.m's
float64 accumulate-and-wrap, and the restated modulator -> noise -> demodulator chain against the theory line of fm.m:196 on run_fm_curves's case.  The kernels are
held to the same restatement in tests/test_fm_gpu.py.

Measured on the CPU (the bound of test_library_taps_against_the_restatement is four times the first figure):
    rade_fm_taps against fm_ref.design, 48 and 96 kHz, with and without the folded de-emphasis: at most 2.3e-15 per tap (bin at 48 kHz)
    NCO phasor against fm.m's float64 accumulate after 1 s of a 1 kHz tone: 3.4e-9 at 48 kHz, 6.8e-9 at 96 kHz"""
import ctypes as C
import os

import numpy as np
import pytest

import fm_ref as fr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM_MAX, FD = 3000.0, 5000.0
TAPS_MEASURED = 2.3e-15                # largest |rade_fm_taps - fm_ref.design| over the four designs below
TAPS_BOUND = 4 * TAPS_MEASURED


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


@pytest.fixture(scope="module")
def tone():
    """per rate: the 1 s, 1 kHz test tone of analog_fm_test (fm.m:150,166) in float32 and its restated modulation at fc = Fs / 4; made once, never written"""
    made = {}

    def get(Fs, fc):
        if (Fs, fc) not in made:
            m = np.sin(2 * np.pi * 1000.0 / Fs * np.arange(int(Fs))).astype(np.float32)
            made[(Fs, fc)] = (m, fr.mod(m, Fs, fc, FD)[0])
        return made[(Fs, fc)]
    return get


def test_fm_symbols_are_declared_and_exported(lib):
    from radae_amd import engine
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    for s in ("rade_batch_fm_mod", "rade_batch_fm_demod", "rade_fm_sigma", "rade_fm_deemph_len", "rade_fm_taps"):
        assert s in engine.EXPORTED_SYMBOLS and hasattr(lib, s)
    assert "int rade_batch_fm_mod(rade_batch *h," in hdr and "int rade_batch_fm_demod(rade_batch *h," in hdr
    assert "enum { RADE_FM_F32 = 0, RADE_FM_C64 = 1 };" in hdr and "enum { RADE_FM_OUT_COMPLEX = 0, RADE_FM_OUT_REAL = 1 };" in hdr
    for name in ("fm_mod", "fm_demod"):
        assert hasattr(engine.BatchEngine, name)
    for name in ("FmModulator", "FmDemodulator", "fm_taps", "fm_sigma", "fm_deemph_len", "fm_pre_emphasis"):
        assert hasattr(engine, name)
    assert (engine.FM_F32, engine.FM_C64, engine.FM_OUT_COMPLEX, engine.FM_OUT_REAL) == (fr.F32, fr.C64, fr.OUT_COMPLEX, fr.OUT_REAL) == (0, 1, 0, 1)
    assert C.sizeof(engine.FmModParams) == 80 and C.sizeof(engine.FmDemodParams) == 96


@pytest.mark.parametrize("Fs", [48000.0, 96000.0])
def test_numpy_firls_against_scipy(Fs):
    """the closed form of fm_ref.firls equals scipy.signal.firls(201, ..) on both designs of fm.m:41-47 within 1e-12"""
    signal = pytest.importorskip("scipy.signal")
    b_in, b_out, amp = fr.design_bands(Fs, FM_MAX, FD)
    for bands in (b_in, b_out):
        d = float(np.abs(fr.firls(201, bands, amp) - signal.firls(201, bands, amp)).max())
        print(f"Fs {Fs:.0f}, bands {bands}: largest difference to scipy {d:.3g}")
        assert d <= 1e-12


@pytest.mark.parametrize("Fs", [48000.0, 96000.0])
@pytest.mark.parametrize("tc", [0.0, fr.TC])
def test_library_taps_against_the_restatement(lib, Fs, tc):
    """rade_fm_taps against fm_ref.design, per tap within TAPS_BOUND = 4 x 2.3e-15 (measured, see the module's docstring; below 1e-9); lengths 201 and 201 + K - 1; the
    filters are symmetric without the de-emphasis; out == NULL only queries"""
    from radae_amd import engine
    K = fr.deemph_len(Fs, tc) if tc else 0
    N2 = 201 + K - 1 if tc else 201
    assert lib.rade_fm_taps(Fs, FM_MAX, FD, 201, tc, None, None) == N2
    b1, b2 = engine.fm_taps(Fs, FM_MAX, FD, 201, tc)
    r1, r2 = fr.design(Fs, FM_MAX, FD, 201, tc)
    assert b1.shape == (201,) and b2.shape == (N2,)
    d1, d2 = float(np.abs(b1 - r1).max()), float(np.abs(b2 - r2).max())
    print(f"Fs {Fs:.0f} tc {tc}: bin {d1:.3g}, bout {d2:.3g}; sum |bin| {np.abs(b1).sum():.4f}, sum |bout| {np.abs(b2).sum():.4f}")
    assert TAPS_BOUND < 1e-9 and max(d1, d2) <= TAPS_BOUND
    assert np.array_equal(b1, b1[::-1])
    if not tc:
        assert np.array_equal(b2, b2[::-1])


def test_deemphasis_length_and_tail():
    """K = 39 at 48 kHz and 90 at 96 kHz (the first power of a below 2^-30), so 201 + K - 1 <= 512; the folded filter equals the recurrence filter(1, prede, .) of
    fm.m:123-125 applied to bout within the cut tail: below 1e-9 per tap, and summed at most a^K / (1 - a) sum |bout|"""
    from radae_amd import engine
    for Fs, K in ((48000.0, 39), (96000.0, 90)):
        assert engine.fm_deemph_len(Fs) == fr.deemph_len(Fs) == K and 201 + K - 1 <= 512
        a = 1.0 - 1.0 / (fr.TC * Fs)
        assert a ** K < 2.0 ** -30 <= a ** (K - 1)
        _, bout = fr.design(Fs, FM_MAX, FD)
        _, folded = fr.design(Fs, FM_MAX, FD, 201, fr.TC)
        x = np.concatenate([bout, np.zeros(400)])                     # the impulse response of bout followed by the recurrence
        y = np.zeros(len(x))
        for i in range(len(x)):
            y[i] = x[i] + (a * y[i - 1] if i else 0.0)
        d = np.abs(y - np.concatenate([folded, np.zeros(len(x) - len(folded))]))
        print(f"Fs {Fs:.0f}: K {K}, largest difference to the recurrence {d.max():.3g}, summed {d.sum():.3g}")
        assert d.max() < 1e-9 and d.sum() <= a ** K / (1.0 - a) * np.abs(bout).sum()      # every cut term a^k, k >= K, meets every tap of bout once
    assert engine.fm_deemph_len(48000.0, 0.0) == 0


def test_sigma_and_refusals(lib):
    """rade_fm_sigma = sqrt(Fs / (CN Bfm)) (fm.m:16,162); the refusals of the three host helpers"""
    from radae_amd import engine
    for CN, Fs in ((20.0, 48000.0), (4.0, 96000.0), (-4.0, 48000.0)):
        assert abs(engine.fm_sigma(CN, Fs, FM_MAX, FD) - fr.sigma(CN, Fs, FM_MAX, FD)) <= 1e-15 * fr.sigma(CN, Fs, FM_MAX, FD) * 4
    assert abs(engine.fm_sigma(20.0, 48000.0, FM_MAX, FD) ** 2 - 48000.0 / (100.0 * 16000.0)) < 1e-15
    for bad in ((float("nan"), 48000.0, FM_MAX, FD), (20.0, 0.0, FM_MAX, FD), (20.0, 48000.0, -1.0, FD), (20.0, 48000.0, FM_MAX, 0.0), (20.0, float("inf"), FM_MAX, FD)):
        assert lib.rade_fm_sigma(*bad) == -1.0
        with pytest.raises(ValueError):
            engine.fm_sigma(*bad)
    buf = np.zeros(1024)
    ok = dict(Fs=48000.0, fm_max=FM_MAX, fd=FD, ntaps=201, tc=0.0)
    call = lambda **kw: lib.rade_fm_taps(*[{**ok, **kw}[k] for k in ("Fs", "fm_max", "fd", "ntaps", "tc")], buf.ctypes.data, buf[512:].ctypes.data)
    assert call() == 201
    for kw in (dict(ntaps=200), dict(ntaps=1), dict(ntaps=513), dict(ntaps=-3), dict(Fs=0.0), dict(Fs=float("nan")), dict(fm_max=0.0), dict(fd=-5.0), dict(tc=-1.0),
               dict(tc=float("nan")), dict(Fs=16000.0), dict(ntaps=511, tc=fr.TC), dict(tc=1e-9)):      # 16 kHz: the pass band of bin ends past the Nyquist rate
        assert call(**kw) == -1, kw
    assert call(ntaps=511) == 511 and call(ntaps=3) == 3 and call(tc=fr.TC) == 239
    with pytest.raises(ValueError):
        engine.fm_taps(48000.0, FM_MAX, FD, 200)
    assert lib.rade_fm_deemph_len(48000.0, -1.0) == -1 and lib.rade_fm_deemph_len(0.0, fr.TC) == -1 and lib.rade_fm_deemph_len(48000.0, 1e-9) == -1


@pytest.mark.parametrize("Fs", [48000.0, 96000.0])
def test_nco_against_the_float64_accumulator(tone, Fs):
    """the 32-bit NCO against analog_fm_mod's float64 accumulate-and-wrap (fm.m:85-93) on the same float32 input, 1 s of a 1 kHz tone at fc = Fs / 4: the phasors
    differ by less than 1e-8 (measured: 3.4e-9 at 48 kHz, 6.8e-9 at 96 kHz)"""
    m, tx = tone(Fs, Fs / 4)
    d = float(np.abs(tx - fr.mod_fm_m(m, Fs, Fs / 4, FD)).max())
    print(f"Fs {Fs:.0f}: largest |NCO phasor - float64 accumulator phasor| over {len(m)} samples: {d:.3g}")
    assert d < 1e-8


def test_nco_increments_follow_the_rule():
    """the increment rule on chosen samples: m = 0 gives rint(kc); Fs / 4 gives exactly 2^30; samples that are not finite or outside +-2^16 count as 0; a negative sum
    wraps mod 2^32; a case whose fused sum lies next to a half-integer is decided by the single rounding"""
    Fs, fc = 48000.0, 12000.0
    inc = fr.nco_inc(np.array([0.0, np.nan, np.inf, -np.inf, 65537.0, 65536.0, -65536.0, 1.0, -1.0], np.float32), Fs, fc, FD)
    kd = FD / Fs * fr.TWO32
    assert list(inc[:5]) == [1 << 30] * 5
    assert inc[5] == (int(np.rint(65536.0 * kd)) + (1 << 30)) % (1 << 32) and inc[6] == (-int(np.rint(65536.0 * kd)) + (1 << 30)) % (1 << 32)
    assert inc[7] == (1 << 30) + int(np.rint(kd)) and inc[8] == (1 << 30) - int(np.rint(kd))
    assert fr.nco_inc(np.array([-1.0], np.float32), Fs, 0.0, FD)[0] == (1 << 32) - int(np.rint(kd))
    tx, ph = fr.mod(np.zeros(8, np.float32), Fs, fc, FD)
    assert np.array_equal(tx, np.array([1j, -1, -1j, 1] * 2)) and ph[3] == 0


@pytest.mark.parametrize("Fs,fc", [(96000.0, 24000.0), (48000.0, 12000.0), (48000.0, 0.0)])
def test_restatement_against_the_theory_line(tone, Fs, fc):
    """run_fm_curves's case (fm.m:134-137, :240-246: fm_max 3 kHz, fd 5 kHz, 1 s of a 1 kHz tone, complex noise, no pre / de-emphasis, the notch of :180-191), also at
    48 kHz and at fc = 0: at C/N 20 and 30 dB the tone SNR of the restated chain lies within 1 dB below C/N + 10 log10(3 m^2 (m + 1)) (fm.m:196) and not above it
    (measured: 0.4 to 0.8 dB below); at C/N 4 dB it is more than 5 dB below: the threshold exists"""
    m, tx = tone(Fs, fc)
    b1, b2 = (b.astype(np.float32) for b in fr.design(Fs, FM_MAX, FD))
    for CN in (4.0, 20.0, 30.0):
        g0, g1 = fr.mod_noise(77 + int(CN), 1, len(m))
        rx = fr.add_noise(tx, g0[0], g1[0], fr.sigma(CN, Fs, FM_MAX, FD), fr.OUT_COMPLEX)
        y, _, _ = fr.demod(rx, Fs, fc, FD, b1, b2)
        snr, theory = fr.tone_snr_dB(y, Fs), fr.snr_theory_dB(CN, FM_MAX, FD)
        print(f"Fs {Fs:.0f} fc {fc:.0f} C/N {CN:.0f} dB: tone SNR {snr:.2f} dB, theory {theory:.2f} dB")
        if CN >= 20.0:
            assert theory - 1.0 <= snr <= theory
        else:
            assert snr < theory - 5.0
