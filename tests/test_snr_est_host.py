"""Host tests (no GPU) of the SNR estimator trials (include/rade_batch.h: rade_batch_snr_trials and the host functions behind it): tests/snr_ref.py against the
reference live, the C rade_snr_sigma / _finish / _fit / _track against snr_ref, the counter mapping of the generated noise, the planted mistakes against the bound,
and the binding's symbols."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import noise_ref as nr
import snr_ref as sr

SET_POINTS, NWS = (-5.0, 5.0, 19.0), (1, 8, 66)
REL = 1e-12


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))                                  # the infinities and NaN of S2 = 0 equal themselves
    with np.errstate(invalid="ignore"):
        return bool(np.all(same | (np.abs(a - b) <= REL * np.abs(b))))


def records(sums):
    from radae_amd.engine import SnrSums
    a = np.zeros(len(sums), np.dtype(SnrSums))
    for i, f in enumerate(sr.FIELDS):
        a[f] = np.asarray(sums)[:, i]
    return a


@pytest.fixture(scope="module")
def inputs():
    """complex Gaussian h and unit noise at the three set points x the three window lengths, two windows each; the model's sums, computed once"""
    rng = np.random.default_rng(2024)
    out = {}
    for sp in SET_POINTS:
        for Nw in NWS:
            h = (rng.standard_normal((2 * Nw, sr.NC)) + 1j * rng.standard_normal((2 * Nw, sr.NC))) / np.sqrt(2)
            n = rng.standard_normal((2 * Nw, sr.NC)) + 1j * rng.standard_normal((2 * Nw, sr.NC))
            sg = float(np.float32(sr.sigma(sp)))
            out[sp, Nw] = (h, n, sg, sr.trial_sums(h, n, sg, Nw), sr.bounds(h, n, sg, Nw))
    return out


def test_restatement_against_the_reference_live():
    """receiver_one.est_pilots and Pmat of the reference itself (a child process: its modules want their own directory)"""
    ref = os.environ.get("RADAE_REFERENCE") or "/root/reference"
    if not os.path.isfile(os.path.join(ref, "radae", "dsp.py")):
        pytest.skip("the reference is not on this machine")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "snr_ref.py"), ref], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": here})
    assert r.returncode == 0 and r.stdout.strip().endswith("live ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_the_model_is_consistent(inputs):
    """S1 = S1_sig + Re-cross-with-conjugate + S1_noise is NOT what the script sums (its cross term has no conjugate); what does hold: S2_genie = sum Im(n)^2, every
    sum but the cross term is positive, and est_pilots returns h pg exactly for a noiseless channel that is linear in e^{-j w a} across three carriers"""
    for (sp, Nw), (h, n, sg, S, B) in inputs.items():
        assert np.all(S[:, [0, 1, 3, 4, 5]] > 0) and np.all(B > 0) and np.all(B[:, 5] < 1e-3 * S[:, 5])
        assert close(S[:, 4], ((sg * n.imag) ** 2).reshape(2, -1).sum(axis=1))
    a, b = 0.7 - 0.2j, -0.3 + 0.5j
    x = (a + b * sr.ROT)[None, :] * sr.P                                          # q = a + b e^{-j w a}: the model the least squares fits
    assert np.abs(sr.est_pilots(x) - (a + b * sr.ROT)).max() < 1e-6              # (the entries of A are float32 values, e^{-j w a} here is not)


def test_sigma_finish_fit_track_against_the_restatement(inputs):
    from radae_amd import engine
    for sp in (-5.0, 0.0, 3.3, 19.0):
        assert close(engine.snr_sigma(sp), sr.sigma(sp))
    Es = np.sum(sr.PGP ** 2) / sr.NC
    assert close(engine.snr_sigma(0.0), np.sqrt(Es / 2))
    rows = [S[k] for (_, _, _, S, _) in inputs.values() for k in range(2)]
    rows += [np.array([10.0, 9.0, 0.1, 1.0, 6.0, 7.0]),                           # S1 / (2 S2) - 1 < 0 either way: the clamp at 0.1
             np.array([12.0, 9.0, 0.1, 1.0, 6.0, 3.0]),                           # exactly 0 with the genie (clamped: <= 0), 1 with the estimate
             np.array([10.0, 9.0, 0.1, 1.0, 0.0, 0.0]),                           # S2 = 0: IEEE, +inf and -inf
             np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])]                            # 0 / 0: NaN passes the clamp, as in the script
    rec = records(rows)
    for eq_ls in (False, True):
        for c, m in ((0.0, 1.0), (2.513, 0.8070)):
            got = engine.snr_finish(rec, eq_ls, c, m)
            for i, row in enumerate(rows):
                want = sr.finish(row, eq_ls, c, m)
                assert close([got[i][f] for f in ("snrdB_genie", "snrdB_est", "NdB_genie", "NdB_est")], want), (i, eq_ls, c, m, got[i], want)
    clamp = engine.snr_finish(rec[-4:], False)
    assert close(clamp["snrdB_est"][:2], [-10.0, -10.0]) and clamp["snrdB_est"][2] == np.inf and clamp["NdB_genie"][2] == -np.inf and np.isnan(clamp["snrdB_est"][3])
    assert close(engine.snr_finish(rec[-3:-2], True)["snrdB_est"], [0.0])
    rng = np.random.default_rng(5)
    x = rng.uniform(-5, 20, 1500)
    y = 0.91 * x + 2.4 + rng.standard_normal(1500)
    m, c = engine.snr_fit(x, y)
    z = np.polyfit(x, y, 1)
    assert close([m, c], z) and close([m, c], sr.fit(x, y))
    assert close(engine.snr_fit([1.0, 3.0], [2.0, -2.0]), [-2.0, 4.0])
    ones = [(k, v) for k, v in inputs.items() if k[1] == 1]
    S1 = np.array([v[3][k, 0] for _, v in ones for k in range(2)] + [10.0, 0.0]); S2 = np.array([v[3][k, 5] for _, v in ones for k in range(2)] + [7.0, 0.0])
    seq = records(np.stack([S1, S1, S1, S1, S2, S2], axis=1))
    assert close(engine.snr_track(seq), sr.track(S1, S2))
    assert close(engine.snr_track(seq, c=0.0, m=1.0, state=3.5), sr.track(S1, S2, 0.0, 1.0, 3.5))
    assert close(engine.snr_track(seq[-1:], state=0.0), [0.1 * ((10 * np.log10(0.1) - 2.513) / 0.8070 + 10 * np.log10(50 * 30 / 3000) + 10 * np.log10(192 / 160))])


def test_host_refusals():
    from radae_amd import engine
    from radae_amd.engine import SnrPoint, SnrSums
    lib = engine.load_library()
    s, out = SnrSums(1, 1, 0, 1, 1, 1), SnrPoint(7.0, 7.0, 7.0, 7.0)
    nan = float("nan")
    for args in ((None, 0, 0.0, 1.0, C.byref(out)), (C.byref(s), 0, 0.0, 1.0, None), (C.byref(s), 0, 0.0, 0.0, C.byref(out)), (C.byref(s), 0, nan, 1.0, C.byref(out)),
                 (C.byref(s), 1, 0.0, float("inf"), C.byref(out))):
        assert lib.rade_snr_finish(*args) == -1 and bytes(out) == bytes(SnrPoint(7.0, 7.0, 7.0, 7.0))
    x, y = np.array([1.0, 1.0, 1.0]), np.array([1.0, 2.0, 3.0])
    m, c = C.c_double(7.0), C.c_double(7.0)
    for args in ((x.ctypes.data, y.ctypes.data, 1), (x.ctypes.data, y.ctypes.data, 3), (None, y.ctypes.data, 3), (x.ctypes.data, None, 3), (x.ctypes.data, y.ctypes.data, 0)):
        assert lib.rade_snr_fit(*args, C.byref(m), C.byref(c)) == -1 and (m.value, c.value) == (7.0, 7.0)
    assert lib.rade_snr_fit(y.ctypes.data, x.ctypes.data, 3, None, C.byref(c)) == -1
    st = C.c_double(1.5)
    seq = (SnrSums * 2)(s, s)
    for args in ((None, 2, 0.0, 1.0, C.byref(st), None), (seq, 2, 0.0, 1.0, None, None), (seq, -1, 0.0, 1.0, C.byref(st), None), (seq, 2, 0.0, 0.0, C.byref(st), None),
                 (seq, 2, nan, 1.0, C.byref(st), None)):
        assert lib.rade_snr_track(*args) == -1 and st.value == 1.5
    assert lib.rade_snr_track(seq, 0, 0.0, 1.0, C.byref(st), None) == 0 and st.value == 1.5
    with pytest.raises(ValueError):
        engine.snr_fit([1.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError):
        engine.snr_finish(records([np.ones(6)]), m=0.0)


def test_generated_noise_mapping():
    """counters of adjacent carriers (pairs), rows and streams are distinct; row0 shifts by whole rows; the third word keeps the draws apart from the four earlier
    consumers of the generator (third words 0..3)"""
    ctr = np.concatenate([sr.counters(b, row0, 70).reshape(-1, 4) for b in (0, 1, 2) for row0 in (0, 1 << 32, 1 << 40)])
    keys = {tuple(int(v) for v in r) for r in ctr}
    assert len(keys) == len(ctr) == 3 * 3 * 70 * 15
    assert set(ctr[:, 2].tolist()) == {4} and ctr[:, 0].max() < 1 << 32 and ctr[:, 3].max() < 1 << 32
    a = sr.counters(1, 0, 10)
    assert np.array_equal(a[3:], sr.counters(1, 3, 7)) and np.array_equal(a[0, 1], a[0, 0] + [1, 0, 0, 0]) and np.array_equal(a[1, 0], a[0, 0] + [15, 0, 0, 0])
    big = sr.counters(0, (1 << 32) // 15 + 1, 1)
    assert big[0, -1, 3] == 1 and sr.counters(0, 1 << 40, 1)[0, 0, 3] == (15 << 40) >> 32      # the fourth word carries q >> 32
    g = sr.gen_noise(12345, 1, 0, 10)
    assert np.array_equal(g[3:], sr.gen_noise(12345, 1, 3, 7)) and not np.array_equal(g, sr.gen_noise(12345, 2, 0, 10))
    w = nr.philox4x32_10(a[0, 0, 0], 1, 4, 0, 12345, 0)
    x0, y0 = nr.gauss_pair(w[0], w[1]); x1, y1 = nr.gauss_pair(w[2], w[3])
    assert g[0, 0] == x0 + 1j * y0 and g[0, 1] == x1 + 1j * y1
    big_n = sr.gen_noise(99, 0, 0, 4000)
    v = np.concatenate([big_n.real.ravel(), big_n.imag.ravel()])
    assert abs(v.mean()) < 0.01 and abs(v.var() - 1.0) < 0.01                    # unit variance per component


@pytest.mark.parametrize("mistake", list(sr.MISTAKES) + ["words"])
def test_planted_mistakes_move_S2_est_past_the_bound(inputs, mistake):
    """Each mistake, applied to the float64 model, moves S2_est of every window by more than the bound.  The smallest relative change over these inputs (printed;
    measured on the CPU) and how many times the bound that is: conjugate transpose 5.4e-2 (1190 x), wrap instead of c_mid 2.3e-4 (10 x: a window of one row whose
    edge carriers happen to carry little), phase sign 5.0e-2 (1490 x), e^{-j w a} left out 2.2e-2 (597 x), words 2-3 to the even carrier 2.5e-3 (44 x)."""
    least, ratio = np.inf, np.inf
    for (sp, Nw), (h, n, sg, S, B) in inputs.items():
        if mistake == "words":
            n = sr.gen_noise(77, 1, 5, 2 * Nw)
            S, B = sr.trial_sums(h, n, sg, Nw), sr.bounds(h, n, sg, Nw, dg=nr.EPS)
            bad = sr.trial_sums(h, sr.gen_noise(77, 1, 5, 2 * Nw, "words"), sg, Nw)
        else:
            bad = sr.trial_sums(h, n, sg, Nw, mistake)
        d = np.abs(bad[:, 5] - S[:, 5])
        assert np.all(d > B[:, 5]), (mistake, sp, Nw, d, B[:, 5])
        least, ratio = min(least, float((d / S[:, 5]).min())), min(ratio, float((d / B[:, 5]).min()))
    print(f"{mistake}: smallest relative change of S2_est {least:.3g}, {ratio:.3g} times the bound")


def test_symbols_are_bound_and_in_the_library():
    from radae_amd import abi, engine
    lib = engine.load_library()
    names = ["rade_batch_snr_trials", "rade_snr_sigma", "rade_snr_finish", "rade_snr_fit", "rade_snr_track"]
    assert engine.SNR_SYMBOLS == names                                             # a list of its own: abi.py says why they are not in EXPORTED_SYMBOLS
    for n in names:
        assert n in abi.PROTOTYPES["rade_batch.h"] and hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    assert C.sizeof(engine.SnrSums) == 48 and C.sizeof(engine.SnrPoint) == 32
