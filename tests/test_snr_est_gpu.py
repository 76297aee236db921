"""GPU tests (-m gpu) of the SNR estimator trials (rade_batch_snr_trials, rade_snr.hip; include/rade_batch.h states the arithmetic): the six sums of every window against
the float64 restatement of tests/snr_ref.py under the bound counted from the kernel's roundings (snr_ref.bounds restates the header's derivation: u = 2^-24 per rounding
of s, n and x, 10 / 14 u along the two rows of Pmat plus the errors of x through the same weights for r, (pi / 2) e_r / |r| for its angle, 10 u |x| for the unit phasor
and the last products), the generated noise against the Philox / Box-Muller reference, a stream in pieces, independence of the batch, the buffer contract on sentinel
buffers (tests/bands.py), the refusals, snr_sweep and the command line.  It is a worst-case bound: WORST_MEASURED records how far below it the device stays."""
import contextlib
import ctypes as C
import io
import re

import numpy as np
import pytest

import noise_ref as nr
import snr_ref as sr
from bands import Band
from gpu_kit import dev, engines, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
# largest |d| / bound per sum over the 18 cases of test_given_noise_against_the_model on the MI355X (the test prints the running figures)
WORST_MEASURED = {"S1": 0.129, "S1_sig": 0.094, "S1_cross": 0.0405, "S1_noise": 0.0735, "S2_genie": 0.157, "S2_est": 0.00693}
SIG = [0.0, float(np.float32(sr.sigma(-5.0))), float(np.float32(sr.sigma(19.0)))]
NWS, STEPS, KINDS = (1, 8, 66), (1, 5), ("awgn", "fading", "zeros")
WORST = dict.fromkeys(sr.FIELDS, 0.0)


def raw_call(eng, nw, Nw, sigma, out, max_windows, H=0, h_stride=0, h_step=1, noise=0, noise_out=0, noise_stride=0, seed=0, row0=None, null=()):
    from radae_amd.engine import SnrParams, _stream_ptr
    nw = np.ascontiguousarray(np.broadcast_to(np.asarray(nw, np.int32), (eng.B,)))
    sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, np.float32), (eng.B,)))
    r0 = None if row0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(row0, np.int64), (eng.B,)))
    p = SnrParams(Nw, h_step, H or None, h_stride, None if "sigma" in null else sg.ctypes.data, None if r0 is None else r0.ctypes.data, noise or None, noise_out or None,
                  noise_stride, seed)
    return eng.lib.rade_batch_snr_trials(eng.h, None if "nw" in null else nw.ctypes.data, None if "p" in null else C.byref(p), None if "out" in null else out.ctypes.data,
                                         max_windows, _stream_ptr())


def f64(rec):
    """a record array of abi.SnrSums [..] as float64 [.., 6]"""
    return np.ascontiguousarray(rec).view(np.float64).reshape(rec.shape + (6,))


def c64(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def check(got, h, n, sigma, Nw, what, dg=0.0):
    """one stream's windows against the model: every one of the six sums of every window within its bound; the ratios go into WORST"""
    ref, bnd = sr.trial_sums(h, n, sigma, Nw), sr.bounds(h, n, sigma, Nw, dg)
    d = np.abs(got[:len(ref)] - ref)
    assert np.all(d <= bnd), (what, np.argwhere(d > bnd).tolist(), d[d > bnd], bnd[d > bnd])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bnd > 0, d / bnd, 0.0)
    for i, f in enumerate(sr.FIELDS):
        WORST[f] = max(WORST[f], float(ratio[:, i].max(initial=0.0)))
    return ref, bnd


def case_inputs(Nw, h_step, kind, seed):
    """B = 3 streams with (3, 1, 0) windows: H [3, rows, 30] or None, noise [3, 3 Nw, 30], sigma per stream"""
    rng = np.random.default_rng(seed)
    nwin = np.array([3, 1, 0], np.int32)
    H = None if kind == "awgn" else c64(rng, 3, (3 * Nw - 1) * h_step + 1, sr.NC) / np.float32(np.sqrt(2))
    n = c64(rng, 3, 3 * Nw, sr.NC)
    if kind == "zeros":
        H[0, 0] = 0; H[0, Nw * h_step] = 0                                         # the first row of windows 0 and 1 of stream 0
        H[1] = 0; n[1, :Nw] = 0                                                    # stream 1's only window: h = 0 and no noise, so r = 0
    k = NWS.index(Nw) + STEPS.index(h_step) + KINDS.index(kind)
    return nwin, H, n, np.roll(np.array(SIG, np.float32), k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h_step", STEPS)
@pytest.mark.parametrize("Nw", NWS)
def test_given_noise_against_the_model(engines, torch_dev, Nw, h_step, kind):
    eng = engines(3)
    nwin, H, n, sg = case_inputs(Nw, h_step, kind, 100 * Nw + 10 * h_step + KINDS.index(kind))
    got = f64(eng.snr_trials(nwin, Nw, sg, H=dev(H, torch_dev), h_step=h_step, noise=dev(n, torch_dev)))
    assert got.shape == (3, 3, 6) and not got[1, 1:].any() and not got[2].any()    # windows past a stream's own stay zero
    for b in range(2):
        rows = int(nwin[b]) * Nw
        ref, _ = check(got[b], None if H is None else H[b, :(rows - 1) * h_step + 1:h_step], n[b, :rows], float(sg[b]), Nw, (Nw, h_step, kind, b))
        if kind == "zeros" and b == 1:
            assert not ref.any() and not got[b].any()                              # r = 0: angle 0, every sum exactly 0
    print(f"Nw {Nw} h_step {h_step} {kind}: largest |d| / bound so far " + ", ".join(f"{f} {v:.3g}" for f, v in WORST.items()) + f" (recorded: {WORST_MEASURED})")


def test_edge_carriers(engines, torch_dev):
    """a window whose only non-zero noise sits on carriers 0, 1, 28, 29: the estimates of the edge carriers take c_mid = 1 and 28"""
    Nw, rng = 8, np.random.default_rng(3)
    n = np.zeros((1, Nw, sr.NC), np.complex64)
    n[0][:, [0, 1, 28, 29]] = c64(rng, Nw, 4)
    for H in (None, c64(rng, 1, Nw, sr.NC)):
        got = f64(engines(1).snr_trials(1, Nw, SIG[1], H=dev(H, torch_dev), noise=dev(n, torch_dev)))
        ref, bnd = check(got[0], None if H is None else H[0], n[0], SIG[1], Nw, "edge")
        wrong = sr.trial_sums(None if H is None else H[0], n[0], SIG[1], Nw, "wrap")
        assert abs(wrong[0, 5] - ref[0, 5]) > 10 * bnd[0, 5]                       # ... and the test can tell


def test_generated_noise(engines, torch_dev):
    """noise_out sample by sample against snr_ref.gen_noise within noise_ref.EPS; the sums within the bound widened by that EPS; and bit-equal to a given-noise run fed
    with noise_out.  Streams 0..2 differ: the stream index is in the counter"""
    Nw, seed, eng = 8, 0x1234567887654321, engines(3)
    nwin = np.array([2, 3, 1], np.int32)
    rng = np.random.default_rng(4)
    H = c64(rng, 3, 3 * Nw, sr.NC)
    Ht = dev(H, torch_dev)
    sums, nout = eng.snr_trials(nwin, Nw, SIG[1:] + SIG[1:2], H=Ht, seed=seed, want_noise=True)
    again = eng.snr_trials(nwin, Nw, SIG[1:] + SIG[1:2], H=Ht, noise=nout)
    assert np.array_equal(f64(sums).view(np.int64), f64(again).view(np.int64))
    g = nout.cpu().numpy()
    for b in range(3):
        rows = int(nwin[b]) * Nw
        ref = sr.gen_noise(seed, b, 0, rows)
        assert np.abs(g[b, :rows].real - ref.real).max() <= nr.EPS and np.abs(g[b, :rows].imag - ref.imag).max() <= nr.EPS, b
        assert not g[b, rows:].any()
        check(f64(sums)[b], H[b, :rows], ref, (SIG[1:] + SIG[1:2])[b], Nw, ("generated", b), dg=nr.EPS)
        check(f64(sums)[b], H[b, :rows], g[b, :rows], (SIG[1:] + SIG[1:2])[b], Nw, ("generated, its own draws", b))


@pytest.mark.parametrize("row0", [0, (1 << 32) // 15 - 10, (1 << 40) - 21])
def test_a_stream_in_pieces(engines, torch_dev, row0):
    """7 windows in one call against the same stream as calls of 3 + 4 windows with row0 and the H pointer advanced: the same bits; with row0 near 2^32 / 15 the fourth
    counter word turns non-zero inside the stream, and the draws still are snr_ref's"""
    Nw, h_step, seed, eng = 3, 5, 77, engines(2)
    rng = np.random.default_rng(5)
    H = dev(c64(rng, 2, (7 * Nw - 1) * h_step + 1, sr.NC), torch_dev)
    r0 = np.array([row0, row0 + 1], np.int64)
    whole, g = eng.snr_trials(7, Nw, SIG[2], H=H, h_step=h_step, seed=seed, row0=r0, want_noise=True)
    a = eng.snr_trials(3, Nw, SIG[2], H=H, h_step=h_step, seed=seed, row0=r0)
    b = eng.snr_trials(4, Nw, SIG[2], H=H[:, 3 * Nw * h_step:], h_step=h_step, seed=seed, row0=r0 + 3 * Nw)
    assert np.array_equal(f64(whole).view(np.int64), np.concatenate([f64(a), f64(b)], axis=1).view(np.int64))
    g = g.cpu().numpy()
    for s in range(2):
        ref = sr.gen_noise(seed, s, int(r0[s]), 7 * Nw)
        assert np.abs(g[s].real - ref.real).max() <= nr.EPS and np.abs(g[s].imag - ref.imag).max() <= nr.EPS
    assert not np.array_equal(g[0, 1:], g[1, :-1])                                 # stream 1 holds the same absolute rows one row earlier: the stream is in the counter


def test_independence_of_the_batch(engines, torch_dev):
    """a stream's windows give the same bits alone (B = 1) and as stream 2 of B = 3, with given noise"""
    Nw, rng = 8, np.random.default_rng(6)
    H, n = c64(rng, 3, 4 * Nw, sr.NC), c64(rng, 3, 4 * Nw, sr.NC)
    three = f64(engines(3).snr_trials([1, 4, 3], Nw, SIG[1], H=dev(H, torch_dev), noise=dev(n, torch_dev)))
    one = f64(engines(1).snr_trials(3, Nw, SIG[1], H=dev(H[2:], torch_dev), noise=dev(n[2:], torch_dev)))
    assert np.array_equal(one[0].view(np.int64), three[2, :3].view(np.int64))
    part = f64(engines(1).snr_trials(1, Nw, SIG[1], H=dev(H[2:, Nw:], torch_dev), noise=dev(n[2:, Nw:], torch_dev)))
    assert np.array_equal(part[0, 0].view(np.int64), three[2, 1].view(np.int64))  # ... nor on which other windows are in the call


def test_buffer_contract(engines, torch_dev):
    """H, noise and noise_out in sentinel buffers (NaN guards and gaps, strides above the minimum, row 0 eight bytes off a 16-byte boundary): inputs untouched, nothing
    written outside a stream's rows of noise_out, no NaN in a result (nothing outside a stream's rows is read), entries of out at or beyond a stream's count untouched"""
    B, Nw, h_step, W = 3, 8, 5, 4
    eng, rng = engines(B), np.random.default_rng(8)
    nwin = np.array([3, 1, 0], np.int32)
    h_row, n_row = ((3 * Nw - 1) * h_step + 1) * sr.NC, 3 * Nw * sr.NC
    Hv, nv = c64(rng, B, h_row), c64(rng, B, n_row)
    Hb = Band(B, h_row, h_row + 7, 8, torch_dev, base_offset_bytes=8).fill(Hv)
    nb = Band(B, n_row, n_row + 31, 8, torch_dev, base_offset_bytes=8).fill(nv)
    out = np.full((B, W, 6), -1.0)
    assert raw_call(eng, nwin, Nw, SIG[1], out, W, H=Hb.ptr, h_stride=h_row + 7, h_step=h_step, noise=nb.ptr, noise_stride=n_row + 31) == 0
    Hb.check(what="H"); nb.check(what="noise")
    assert np.array_equal(Hb.rows(np.complex64).view(np.int32), Hv.view(np.int32)) and np.array_equal(nb.rows(np.complex64).view(np.int32), nv.view(np.int32))
    for b in range(B):
        k = int(nwin[b])
        assert np.isfinite(out[b, :k]).all() and np.all(out[b, k:] == -1.0)
        if k:
            check(out[b, :k], Hv[b].reshape(-1, sr.NC)[:(k * Nw - 1) * h_step + 1:h_step], nv[b].reshape(-1, sr.NC)[:k * Nw], SIG[1], Nw, ("banded", b))
    ob = Band(B, n_row, n_row + 31, 8, torch_dev, base_offset_bytes=8)
    out2 = np.full((B, W, 6), -1.0)
    assert raw_call(eng, nwin, Nw, SIG[1], out2, W, H=Hb.ptr, h_stride=h_row + 7, h_step=h_step, noise_out=ob.ptr, noise_stride=n_row + 31, seed=9) == 0
    ob.check(written=nwin.astype(np.int64) * Nw * sr.NC, what="noise_out")
    Hb.check(what="H")
    assert np.all(out2[0, 3:] == -1.0) and np.all(out2[1, 1:] == -1.0) and np.all(out2[2] == -1.0) and np.isfinite(out2[0, :3]).all()
    g = ob.rows(np.complex64)
    out3 = np.full((B, W, 6), -1.0)
    gb = Band(B, n_row, n_row + 1, 8, torch_dev).fill(np.where(np.isnan(g.real), 0, g).astype(np.complex64))
    assert raw_call(eng, nwin, Nw, SIG[1], out3, W, H=Hb.ptr, h_stride=h_row + 7, h_step=h_step, noise=gb.ptr, noise_stride=n_row + 1) == 0
    assert np.array_equal(out3.view(np.int64), out2.view(np.int64))


def test_refusals_write_nothing(engines, torch_dev):
    """argument checking on the host: each of these returns -1 before any launch; out_host and noise_out keep their bytes"""
    B, Nw, h_step, W = 3, 8, 5, 3
    eng, rng = engines(B), np.random.default_rng(10)
    h_row, n_row = ((3 * Nw - 1) * h_step + 1) * sr.NC, 3 * Nw * sr.NC
    Hb = Band(B, h_row, h_row, 8, torch_dev).fill(c64(rng, B, h_row))
    nb = Band(B, n_row, n_row, 8, torch_dev).fill(c64(rng, B, n_row))
    ob = Band(B, n_row, n_row, 8, torch_dev)
    out = np.full((B, W, 6), -7.0)
    given = dict(nw=(3, 1, 0), Nw=Nw, sigma=SIG[1], out=out, max_windows=W, H=Hb.ptr, h_stride=h_row, h_step=h_step, noise=nb.ptr, noise_stride=n_row)
    made = {**given, "noise": 0, "noise_out": ob.ptr, "seed": 5}
    nan, inf = float("nan"), float("inf")
    bad = [(given, kw) for kw in (dict(null=("nw",)), dict(null=("p",)), dict(null=("sigma",)), dict(null=("out",)), dict(Nw=0), dict(Nw=67), dict(Nw=-1), dict(h_step=0),
                                  dict(h_step=6), dict(seed=5), dict(noise=0), dict(noise_out=ob.ptr), dict(max_windows=2), dict(nw=(3, 1, -1)), dict(nw=(3, 4, 0)),
                                  dict(h_stride=h_row - 1), dict(noise_stride=n_row - 1), dict(H=Hb.ptr + 4), dict(noise=nb.ptr + 4), dict(sigma=-1.0), dict(sigma=nan),
                                  dict(sigma=(1.0, inf, 1.0)), dict(row0=-1), dict(row0=(0, 0, (1 << 40) + 1)))]
    bad += [(made, kw) for kw in (dict(noise_stride=n_row - 1), dict(noise_out=ob.ptr + 4), dict(noise=nb.ptr), dict(seed=0), dict(h_stride=h_row - 1))]
    for base, kw in bad:
        assert raw_call(eng, **{**base, **kw}) == -1, kw
        assert np.all(out == -7.0), kw
    ob.untouched(what="noise_out")
    for base, kw in ((given, dict()), (given, dict(H=0, h_stride=0)), (given, dict(row0=1 << 40)), (given, dict(nw=(1, 1, 0), h_stride=h_row - 1)),
                     (given, dict(H=Hb.ptr + 8, h_stride=h_row - 1, nw=(2, 1, 0))), (made, dict()), (made, dict(noise_out=0, noise_stride=0)), (given, dict(nw=0, max_windows=0))):
        assert raw_call(eng, **{**base, **kw}) == 0, kw                            # ... and the same arguments without the fault are accepted
    assert np.all(out[0] != -7.0) and np.all(out[1, 1:] == -7.0) and np.all(out[2] == -7.0)
    Hb.check(what="H"); nb.check(what="noise")
    with pytest.raises(RuntimeError):
        eng.snr_trials(1, 67, 1.0, seed=1)
    with pytest.raises(ValueError):
        eng.snr_trials(1, 8, 1.0, noise=dev(c64(rng, B, 8, sr.NC), torch_dev), want_noise=True)


def model_points(channels, Nt, Nw, set_points, seed, eq_ls, c, m, h_step=5):
    """snr_sweep's points from the float64 model with snr_ref's own draws: x, y and their bounds [n_channels, n_set_points Nt]"""
    x, y, bx, by = [], [], [], []
    for j, ch in enumerate(channels):
        h = None if ch is None else np.asarray(ch)[:(Nt * Nw - 1) * h_step + 1:h_step]
        for i, sp in enumerate(set_points):
            sg = float(np.float32(sr.sigma(sp)))
            n = sr.gen_noise(seed, j * len(set_points) + i, 0, Nt * Nw)
            S, Bd = sr.trial_sums(h, n, sg, Nw), sr.bounds(h, n, sg, Nw, dg=nr.EPS)
            for k in range(Nt):
                f, fb = sr.finish(S[k], eq_ls, c, m), sr.finish_bounds(S[k], Bd[k], eq_ls, m)
                x.append(f[0]); y.append(f[1]); bx.append(fb[0]); by.append(fb[1])
    return (np.array(v).reshape(len(channels), -1) for v in (x, y, bx, by))


def test_snr_sweep(engines, torch_dev):
    """two channels (AWGN, and an MPP H from multipath_h_gen at the rate-Rs file's shape) x 25 set points x 4 windows in one device call: the points equal snr_finish of
    the model's sums within the bound propagated through finish, the fit is within the same propagated tolerance of snr_ref.fit over the model's points"""
    from radae_amd import engine
    Nt, Nw = 4, 8
    Hm = engines(1).multipath_h_gen("mpp", (Nt * Nw - 1) * 5 + 1, rs=50, nc=sr.NC, seed=3, complex_=True)[0]
    assert tuple(Hm.shape) == ((Nt * Nw - 1) * 5 + 1, sr.NC)
    r = engine.snr_sweep([None, Hm], Nt, 1.0, eq_ls=True, c=2.513, m=0.8070, seed=11, engine=engines(50))
    x, y, bx, by = model_points([None, Hm.cpu().numpy()], Nt, Nw, range(-5, 20), 11, True, 2.513, 0.8070)
    assert np.isfinite(bx).all() and np.isfinite(by).all() and by.max() < 1e-2
    assert r.snrdB_genie.shape == x.shape == (2, 100) and np.all(np.abs(r.snrdB_genie - x) <= bx) and np.all(np.abs(r.snrdB_est - y) <= by)
    for j in range(2):
        m, c = sr.fit(x[j], y[j])
        dm, dc = sr.fit_bounds(x[j], y[j], bx[j], by[j])
        assert abs(r.fit[j, 0] - m) <= dm + 1e-12 * abs(m) and abs(r.fit[j, 1] - c) <= dc + 1e-12 * abs(c), (j, r.fit[j], m, c, dm, dc)
    print(f"fits (m, c): AWGN {r.fit[0].round(4).tolist()}, MPP {r.fit[1].round(4).tolist()}; largest propagated bound {max(bx.max(), by.max()):.3g} dB")
    with pytest.raises(ValueError):
        engine.snr_sweep([None], Nt, engine=engines(3))


def run_cli(argv):
    from radae_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(argv) == 0
    return buf.getvalue().splitlines()


def test_command_line(torch_dev):
    """est_snr --single and --sequence print the script's lines; the numbers are snr_ref's for the same seed within the propagated bound and half a unit of %5.2f"""
    num = r"\s*(-?\d+\.\d\d)"
    (single,) = run_cli(["est_snr", "--single", "--snrdB", "10", "--seed", "1"])
    got = [float(v) for v in re.fullmatch(rf"setpoint snrdB:{num} snrdB_genie:{num} snrdB_est:{num}", single).groups()]
    x, y, bx, by = model_points([None], 1, 8, [10.0], 1, False, 0.0, 1.0)
    assert got[0] == 10.0 and abs(got[1] - x[0, 0]) <= 0.005 + bx[0, 0] and abs(got[2] - y[0, 0]) <= 0.005 + by[0, 0], (single, x, y)
    lines = run_cli(["est_snr", "--sequence", "--Nt", "3", "--eq_ls", "-c", "2.513", "-m", "0.8070"])
    assert len(lines) == 3
    sg = float(np.float32(sr.sigma(10.0)))
    n = sr.gen_noise(1, 0, 0, 24)
    S, Bd = sr.trial_sums(None, n, sg, 8), sr.bounds(None, n, sg, 8, dg=nr.EPS)
    for k, line in enumerate(lines):
        got = [float(v) for v in re.fullmatch(rf"setpoint snrdB:{num} snrdB_genie:{num} snrdB_est:{num} NdB:{num}{num}", line).groups()]
        want, tol = sr.finish(S[k], True, 2.513, 0.8070), sr.finish_bounds(S[k], Bd[k], True, 0.8070)
        assert got[0] == 10.0 and all(abs(g - w) <= 0.005 + t for g, w, t in zip(got[1:], want, tol)), (line, want, tol)
    s1 = run_cli(["est_snr", "--single", "--test_S1", "--seed", "1"])
    assert len(s1) == 3 and s1[0].startswith("S1_first:") and s1[2] == single                      # the same seed and set point: the same trial
    a, b = (float(v) for v in re.fullmatch(rf"S1:{num} S1_sum:{num}", s1[1]).groups())
    assert abs(a - b) <= 0.02 and abs(a - S[0, 0]) <= 0.005 + Bd[0, 0]                               # est_snr.py:90-93: the three terms add up to S1
