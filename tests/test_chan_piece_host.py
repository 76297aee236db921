"""The channel and the Doppler generator in pieces, on the CPU: what tests/chanp_ref.py and the host side of the feature rest on.

1. rade_multipath_gain equals its closed form for the taps of the four presets, and lies inside the spread of the gain realised by channel_tools' sequences of 1200 s.
2. chanp_ref's wrapping uint64 phase equals Python-integer arithmetic, far beyond 2^32 samples.
3. chanp_ref's checkers accept the restatement rounded to float32 and reject four planted bugs (as tests/test_tx_units_host.py does for its checkers).
4. ChannelStream's bookkeeping -- absolute indices, the 16-sample tail, the window of Doppler samples it asks for -- with the device calls stubbed.
(The refusals of the two calls need an engine: tests/test_chan_piece_gpu.py.)"""
import numpy as np
import pytest

import chanp_ref as cp
from radae_amd import channel_tools as ct
from radae_amd import stages


def preset_taps(name):
    taps, ratio, _ = ct.doppler_plan(ct.PRESETS[name][0], 8000, 2)
    return np.asarray(taps, np.float32), ratio


# ================================================================================================================================================================
# 1. the expected-value gain
# ================================================================================================================================================================
@pytest.mark.parametrize("name", list(ct.PRESETS))
def test_multipath_gain_is_its_closed_form(name):
    taps, ratio = preset_taps(name)
    t = taps.astype(np.float64)
    R0, R1 = 2 * sum(v * v for v in t), 2 * sum(a * b for a, b in zip(t[:-1], t[1:]))
    want = 1.0 / np.sqrt(2 * ((2 / 3) * R0 + (1 / 3) * R1))
    got = stages.multipath_gain(taps)
    print(f"{name}: ratio {ratio}, hf_gain {got:.6f}")
    assert abs(got - want) <= 1e-12 * want and abs(cp.multipath_gain(taps) - want) <= 1e-12 * want


def test_multipath_gain_refuses():
    from radae_amd.abi import load_library
    lib = load_library()
    t = np.ones(4, np.float32)
    assert lib.rade_multipath_gain(None, 4) == -1.0 and lib.rade_multipath_gain(t.ctypes.data, 0) == -1.0 and lib.rade_multipath_gain(t.ctypes.data, 257) == -1.0
    t[2] = np.inf
    assert lib.rade_multipath_gain(t.ctypes.data, 4) == -1.0
    assert lib.rade_multipath_gain(np.zeros(4, np.float32).ctypes.data, 4) == -1.0


def realised_gain(name, seconds, seed, full_rate):
    """1 / sqrt(var G1 + var G2) of the sequence channel_tools.multipath_g normalises (the same generator, the same draws).  full_rate: from doppler_spread's samples;
    else from the low-rate points, the sums over each interpolated block in closed form (sum f = (M - 1) / 2, sum f^2 = (M - 1)(2 M - 1) / (6 M) for f = j / M; the last
    block is extrapolated, f = 1 + j / M): 1200 s are 9.6 M samples per path at the full rate and 12,000 points at the low one."""
    spread = ct.PRESETS[name][0]
    nsam = seconds * 8000
    rng = np.random.default_rng(seed)
    if full_rate:
        return 1.0 / np.sqrt(sum(np.var(ct.doppler_spread(spread, 8000, nsam, rng)) for _ in range(2)))
    taps, M, nl = ct.doppler_plan(spread, 8000, nsam)
    assert nl * M == nsam
    var = 0.0
    for _ in range(2):
        x = rng.standard_normal(nl + 100) + 1j * rng.standard_normal(nl + 100)
        y = np.convolve(x, taps)[:nl + 100][100:]
        a, d = y[:-1], y[1:] - y[:-1]
        s1, s2 = (M - 1) / 2, (M - 1) * (2 * M - 1) / (6 * M)
        sg = (M * a + d * s1).sum() + M * a[-1] + d[-1] * (M + s1)
        sq = (M * np.abs(a) ** 2 + 2 * (a * d.conj()).real * s1 + np.abs(d) ** 2 * s2).sum() \
            + M * abs(a[-1]) ** 2 + 2 * (a[-1] * d[-1].conjugate()).real * (M + s1) + abs(d[-1]) ** 2 * (M + 2 * s1 + s2)
        var += sq / nsam - abs(sg / nsam) ** 2
    return 1.0 / np.sqrt(var)


@pytest.mark.parametrize("name", ["mpp", "mpd"])
def test_multipath_gain_lies_inside_the_realised_spread(name):
    """over 8 seeds x 1200 s the realised gain brackets the expected one (the block sums are held to the full-rate samples on 20 s first)"""
    assert abs(realised_gain(name, 20, 5, False) / realised_gain(name, 20, 5, True) - 1) < 1e-9
    got = stages.multipath_gain(preset_taps(name)[0])
    real = [realised_gain(name, 1200, seed, False) for seed in range(1, 9)]
    print(f"{name}: expected {got:.4f}, realised {min(real):.4f} .. {max(real):.4f}, mean ratio {np.mean(real) / got:.4f}")
    assert min(real) <= got <= max(real)


# ================================================================================================================================================================
# 2. the phase
# ================================================================================================================================================================
@pytest.mark.parametrize("f0, df_dt", [(10.0, 0.0), (-1999.5, 0.3), (0.0, -2.5), (1e-3, 1e-4)])
def test_phase_equals_python_integers(f0, df_dt):
    f0q, dq = cp.phase_q(f0, df_dt)
    assert 0 <= f0q < 1 << 64 and 0 <= dq < 1 << 64
    hz = ((f0q + (1 << 63)) % (1 << 64) - (1 << 63)) / 2.0 ** 64 * 8000        # exact where there is a drift, the float32 omega's (2e-7 relative at most) where not
    assert abs(hz - np.float32(f0)) <= (1e-12 if df_dt else 2e-7 * abs(f0))
    if not df_dt:                          # the whole call's omega, as tests/tx_ref.py restates chan_phase_acc: its phase at sample 0
        import tx_ref as tx
        assert f0q == int(np.rint(float(tx.chan_phase(0, f0, 0.0)) / (2 * np.pi) * 2.0 ** 64)) % (1 << 64)
    for n in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 62 - 1):
        want = ((n + 1) * f0q + (n * (n + 1) // 2) * dq) % (1 << 64)
        assert int(cp.phase(n, f0q, dq)[0]) == want, n
        want_ex = (n * f0q + (n * (n - 1) // 2) * dq) % (1 << 64)
        assert int(cp.phase(n, f0q, dq, inclusive=False)[0]) == want_ex, n
    n = np.array([0, 1, 2 ** 33 + 5, 2 ** 33 + 6], np.uint64)
    assert [int(v) for v in cp.phase(n, f0q, dq)] == [((int(k) + 1) * f0q + (int(k) * (int(k) + 1) // 2) * dq) % (1 << 64) for k in n]


# ================================================================================================================================================================
# 3. the checkers reject what they are for
# ================================================================================================================================================================
def _chan_case(rng, **kw):
    n_in, n0, n_out = 300, 21, 260
    txs = ((rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)) * 0.5).astype(np.complex64)
    G = ((rng.standard_normal((n_in, 2)) + 1j * rng.standard_normal((n_in, 2))) * 0.7).astype(np.complex64)
    return dict(txs=txs, in_base=n0 - 16, n0=n0, n_out=n_out, b=1, G=G, g_base=n0 - 16, gain=1.25, sigma=0.4, rx_gain=0.5, **kw)


@pytest.mark.parametrize("bug, kw", [
    ("delay", dict(seed=7, freq_offset=3.0)),
    ("exclusive", dict(seed=7, freq_offset=10.0, df_dt=0.5)),
    ("imag", dict(seed=7, noise_mode=cp.NOISE_REAL)),
])
def test_the_channel_checker_rejects(bug, kw):
    c = _chan_case(np.random.default_rng(11), **kw)
    ref = cp.chan_ref(**c)
    r = cp.check_chan(ref[0].astype(np.complex64), ref, "the restatement rounded to float32")
    assert r < 1.0
    with pytest.raises(AssertionError, match="outside the bound"):
        cp.check_chan(cp.chan_ref(bug=bug, **c)[0].astype(np.complex64), ref, bug)


def test_the_generator_checker_rejects_an_off_by_one_in_i0():
    taps, _ = preset_taps("mpp")
    for ratio in (1, 16):
        ref = cp.dopp_ref(taps, ratio, 2.0, 9, 1, 2 ** 33 + 5, 200)
        assert cp.check_dopp(ref[0].astype(np.complex64), ref, "the restatement rounded to float32") < 1.0
        with pytest.raises(AssertionError, match="outside the bound"):
            cp.check_dopp(cp.dopp_ref(taps, ratio, 2.0, 9, 1, 2 ** 33 + 5, 200, i0_bug=1)[0].astype(np.complex64), ref, "i0 + 1")


def test_generator_restatement_is_the_whole_generators_on_its_interior():
    """dopp_ref with the gain of a realised sequence equals tests/tx_ref.py's mpgen_ref (the whole generator's float64 model) where that does not extrapolate"""
    import noise_ref as nr
    import tx_ref as tx
    taps, _ = preset_taps("mpd")
    ratio, n_out, seed = 16, 1000, 5
    n_low = tx.n_low_of(ratio, n_out)
    want, _ = tx.mpgen_ref(nr.multipath_low(seed, 2, n_low, len(taps)).astype(np.complex128), taps, ratio, n_out)
    keep = (n_low - 1) * ratio
    for b in range(2):
        g, _ = cp.dopp_ref(taps, ratio, 1.0, seed, b, 0, keep)
        hf = (want[b, :keep] * g.conj()).real.sum() / (np.abs(g) ** 2).sum()
        assert np.abs(hf * g - want[b, :keep]).max() < 1e-6 * np.abs(want[b]).max()      # (multipath_low hands the draws over as complex64)


# ================================================================================================================================================================
# 4. ChannelStream's bookkeeping
# ================================================================================================================================================================
def test_channel_stream_bookkeeping():
    import torch

    class Cuda(torch.Tensor):            # a host tensor that says it is on the device: all _TailCarry asks of a piece
        is_cuda = property(lambda self: True)

    class Stub:
        B, device = 2, torch.device("cpu")

        def __init__(self):
            self.gen, self.chan = [], []

        def multipath_piece(self, taps, ratio, n_out, n0=0, seed=1, hf_gain=0.0, out=None):
            self.gen.append(dict(ratio=ratio, n_out=np.array(n_out), n0=np.array(n0), seed=seed, hf_gain=hf_gain, n_taps=len(taps)))
            return torch.zeros((self.B, int(np.max(n_out)), 2), dtype=torch.complex64), np.asarray(n_out, np.int32)

        def channel_piece(self, tx, sigma, freq_offset, df_dt, gain, n0=0, in_base=None, n_out=None, seed=0, G=None, g_base=None, n_g=None):
            self.chan.append(dict(tx=tx.clone(), sigma=sigma, freq_offset=freq_offset, n0=np.array(n0), in_base=np.array(in_base), n_out=n_out, seed=seed,
                                  g_base=None if g_base is None else np.array(g_base), n_g=n_g, G=G))
            return tx[:, tx.shape[1] - n_out:].clone(), np.full(self.B, n_out, np.int32)

    start = np.array([0, 1000], np.int64)
    whole = torch.randn(2, 126, dtype=torch.complex64)
    for channel in ("mpp", None):
        eng = Stub()
        cs = stages.ChannelStream(eng, channel, [6.0, 3.0], freq_offset=8.0, seed=5, n0=start)
        assert cs.sigma.dtype == np.float32 and cs.sigma[0] < cs.sigma[1]
        pos, out = 0, []
        for n in (5, 20, 1, 100):
            out.append(cs.push(whole[:, pos:pos + n].as_subclass(Cuda)))
            call = eng.chan[-1]
            hist = min(16, pos)
            assert np.array_equal(call["n0"], start + pos) and np.array_equal(call["in_base"], start + pos - hist) and call["n_out"] == n and call["seed"] == 5
            assert torch.equal(call["tx"].as_subclass(torch.Tensor), whole[:, pos - hist:pos + n]), "the piece behind its last 16 transmit samples"
            if channel:
                g = eng.gen[-1]
                g0 = np.maximum(start + pos - 16, 0)
                assert np.array_equal(g["n0"], g0) and np.array_equal(g["n_out"], start + pos + n - g0) and np.array_equal(call["g_base"], g0)
                assert g["ratio"] == 800 and g["n_taps"] == 100 and g["seed"] == 5 and abs(g["hf_gain"] - stages.multipath_gain(preset_taps("mpp")[0])) < 1e-15
            else:
                assert call["G"] is None and not eng.gen
            pos += n
            assert np.array_equal(cs.n0, start + pos)
        assert torch.equal(torch.cat(out, dim=1).as_subclass(torch.Tensor), whole)
