"""CPU tests of the Welch / PAPR / bandwidth stage (include/rade_batch.h: rade_batch_psd, rade_batch_sigstat, rade_psd_*): the float64 restatement tests/psd_ref.py
against scipy.signal.welch (an independent implementation: it pins the window, the segment starts and the density scaling), the host helpers, the header and the
exported symbols, the header's float32 factorisation inside the counted bound, and the margin of the end-to-end signals from the step of the bandwidth."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import psd_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(1024, 512), (512, 256), (400, 173), (16, 1)]


def signals(n):
    rng = np.random.default_rng(5)
    noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    real = np.cos(2 * np.pi * 1234.5 / 8000 * np.arange(n)) + 0.1 * rng.standard_normal(n)
    return {"complex_noise": noise, "real": real}


# ---- 1. the restatement against scipy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["complex_noise", "real"])
@pytest.mark.parametrize("win, step", GEOMETRIES)
def test_restatement_against_scipy(win, step, kind):
    from scipy import signal
    x = signals(3000)[kind]
    f, want = signal.welch(x, fs=8000, window=signal.windows.hamming(win, sym=True), nperseg=win, noverlap=win - step, nfft=1024, detrend=False, return_onesided=False,
                           scaling="density")
    got = pr.welch(x, win, step)
    assert np.array_equal(f[:512], np.arange(512) * 8000 / 1024)                       # natural order, 0 .. Fs 1023 / 1024 (scipy names the upper half negative)
    assert np.allclose(f[512:] + 8000, np.arange(512, 1024) * 8000 / 1024)
    assert np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.allclose(signal.get_window("hamming", win, fftbins=False), pr.window(win), rtol=0, atol=1e-15)


# ---- 2. the host helpers ---------------------------------------------------------------------------------------------------------------------------------------
def test_segments_window_plan_and_defaults():
    from radae_amd import engine as E
    for win, step in GEOMETRIES:
        for n in (win - 1, win, win + step - 1, win + step, 80000, 806400):
            assert E.psd_segments(n, win, step) == len(range(0, n - win + 1, step)) == pr.segments(n, win, step), (win, step, n)
        assert np.array_equal(E.psd_window(win).view(np.int32), pr.window(win).astype(np.float32).view(np.int32))          # one rounding of the double formula
        q = E.psd_plan(win, step)
        assert (q.nfft, q.win, q.step) == (1024, win, step) and q.run >= 1
    assert E.psd_segments(0, 16, 1) == 0 and E.psd_segments(15, 16, 1) == 0
    for win, step in ((15, 1), (1025, 1), (16, 0), (16, 17), (1024, 1025)):
        with pytest.raises(ValueError):
            E.psd_plan(win, step)
    for win in (15, 1025, 0):
        with pytest.raises(ValueError):
            E.psd_window(win)
    for n in (1, 2, 3, 127, 128, 129, 20000, 80000, 806400):                           # the recalled rule, as stated
        win = 2 ** int(np.ceil(np.log2(np.sqrt(n / 0.5))))
        assert E.psd_octave_default(n) == (win, win - win // 2), n
    with pytest.raises(ValueError):
        E.psd_octave_default(0)


def test_bandwidth_on_hand_built_spectra():
    from radae_amd import engine as E
    P = np.zeros(1024)
    P[191] = 3.0                                                                       # all power in the centre bin: one-based 192 = round(1024 1500 / 8000)
    assert E.psd_bandwidth(P) == (2 * 8000 / 1024, 1.0) == pr.bandwidth(P)
    # a flat band of 101 bins, one-based 142..242 = 192 +- 50.  bw = 2 m takes 192 - m .. 192 + m (2 m + 1 bins); bw = 2 m + 1 takes round(191.5 - m) .. round(192.5 + m)
    # = 192 - m .. 193 + m under Octave's rounding (2 m + 2 bins).  More than 99.99 of 101 needs 100 bins inside the band: bw = 98 has 99 (143..241), bw = 99 has
    # 143..242 = 100.  Rounding half to even would take 142..242 at bw = 99: the same bw, but a ratio of 1.
    P = np.zeros(1024)
    P[141:242] = 1.0
    assert E.psd_bandwidth(P) == (99 * 8000 / 1024, 100 / 101) == pr.bandwidth(P)
    # two bins, one-based 191 and 195: bw = 2 (191..193), bw = 3 (191..194) and bw = 4 (190..194) hold half; bw = 5 takes round(189.5) .. round(194.5) = 190 .. 195
    # under Octave's rounding and holds all; rounding half to even would end at 194 and go on to bw = 6
    P = np.zeros(1024)
    P[[190, 194]] = 1.0
    assert E.psd_bandwidth(P) == (5 * 8000 / 1024, 1.0) == pr.bandwidth(P)
    assert E.psd_bandwidth(P, frac=0.4) == (2 * 8000 / 1024, 0.5)
    # never reached inside the array: centre 6250 Hz is bin 800; en passes 1024 at bw = 449 while st is still 576, and the power lies below
    P = np.zeros(1024)
    P[:100] = 1.0
    assert E.psd_bandwidth(P, centre_hz=6250.0) is None and pr.bandwidth(P, centre_hz=6250.0) is None
    assert E.psd_bandwidth(np.zeros(1024)) is None                                     # silence: 0 > 0 never holds
    # float32 input is summed in double
    rng = np.random.default_rng(1)
    P = rng.uniform(0.5, 1.5, 1024).astype(np.float32)
    got, want = E.psd_bandwidth(P), pr.bandwidth(P)
    assert got[0] == want[0] and abs(got[1] - want[1]) < 1e-13


def test_octave_rounding():
    assert [pr.octave_round(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 190.5, 2.4999)] == [1, 2, 3, -1, -2, 191, 2]


# ---- 3. the header and the symbols --------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_structures():
    from radae_amd import abi, engine as E
    lib = abi.load_library()
    text = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    names = ["rade_psd_plan", "rade_psd_segments", "rade_psd_window", "rade_psd_octave_default", "rade_psd_bandwidth", "rade_batch_psd", "rade_batch_sigstat"]
    for n in names:
        assert n in E.EXPORTED_SYMBOLS and hasattr(lib, n), n
        assert re.search(r"^(int|long long) %s\(" % n, text, re.M), n
    assert C.sizeof(abi.PsdPlan) == 16 and C.sizeof(abi.SigstatResult) == 40
    block = text[text.index("Welch power spectrum, 99 % bandwidth"):text.index("int rade_batch_sigstat(")]
    assert "DEVIATION" in block and "RECALLED, NOT VERIFIED" in block and "(80 + R) u" in block
    for n in ("psd_plan", "psd_segments", "psd_window", "psd_bandwidth", "psd_octave_default"):
        assert callable(getattr(E, n))
    assert callable(E.BatchEngine.psd) and callable(E.BatchEngine.sigstat)


# ---- 4. the header's factorisation stays inside the counted bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win, step, n", [(1024, 512, 1024), (1024, 512, 1024 + 512 * 64), (400, 173, 2000), (16, 1, 300), (1024, 1024, 3000)])
def test_stated_factorisation_within_the_bound(win, step, n):
    from radae_amd import engine as E
    R = E.psd_plan(win, step).run
    rng = np.random.default_rng(win + n)
    x = (3000 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    m = np.arange(1024)
    t32 = (np.cos(2 * np.pi * m / 1024).astype(np.float32) - 1j * np.sin(2 * np.pi * m / 1024).astype(np.float32)).astype(np.complex64)
    got = pr.stated_psd(x, win, step, R, E.psd_window(win), t32).astype(np.float64)
    ref, bound = pr.welch(x, win, step), pr.bound(x, win, step, R)
    ratio = np.abs(got - ref).max() / bound
    print(f"win {win} step {step} n {n}: largest |P^ - P| / bound {ratio:.3e}; relative to the largest bin {np.abs(got - ref).max() / ref.max():.3e}")
    assert ratio <= 1
    assert np.abs(got - ref).max() <= 1e-5 * ref.max()                                 # ... and it is a DFT at all: the bound alone would admit far more


# ---- 5. the end-to-end signals are far from the step of the bandwidth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pr.E2E_SEEDS))
def test_margin_of_the_end_to_end_signals(name):
    x = pr.e2e_signal(name)
    P = pr.welch(x, pr.E2E_WIN, pr.E2E_STEP)
    m = pr.margin(P)
    print(f"{name}: bandwidth {pr.bandwidth(P)}, margin {m:.3e}; bound / total {pr.bound(x, pr.E2E_WIN, pr.E2E_STEP, 32) * 1024 / P.sum():.3e}")
    assert m > 1e-4
    # the lines `cli do_plots` prints do not sit on a rounding edge of their last digit either: the header's float32 arithmetic prints what float64 prints
    from radae_amd import engine as E
    k = np.arange(1024)
    t32 = (np.cos(2 * np.pi * k / 1024).astype(np.float32) - 1j * np.sin(2 * np.pi * k / 1024).astype(np.float32)).astype(np.complex64)
    P32 = pr.stated_psd(x, pr.E2E_WIN, pr.E2E_STEP, E.psd_plan(pr.E2E_WIN, pr.E2E_STEP).run, E.psd_window(pr.E2E_WIN), t32).astype(np.float64)
    t = pr.sigstat_f32(x).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        first = "Pav: %f PAPRdB: %5.2f PilotPAPRdB: %5.2f" % (t.sum() / len(x), 10 * np.log10(t.max() / (t.sum() / len(x))), 10 * np.log10(t[:160].max() / (t[:160].sum() / 160)))
    assert (first, "bandwidth (Hz): %f power/total_power: %f" % pr.bandwidth(P32)) == pr.papr_lines(x, P)
