"""GPU tests (-m gpu) of the noise generated on the device (seed != 0) against tests/noise_ref.py, sample by sample: the two primitives philox4x32 and
gauss_pair (rade_devutil.h) through the probe shim rd_launch_noise_probe, then the four kernels that consume them, each with its own counter mapping
(k_chan_apply, k_chan_symbol, k_rs_pa, k_multipath_gen; noise_ref.py's docstring states the mappings).  The signal is zero (or subtracted) in every case, so what
is left is sigma x noise; a word taken from the wrong place moves a sample by about 1, the bar is EPS.

EPS.  The Philox words must be equal bit for bit.  gauss_pair runs on the hardware log2 / sqrt / sin / cos units, so it is held to the float64 Box-Muller of the
same float32 uniforms within EPS = four times the largest deviation measured on the MI355X over the inputs of test_probe_gauss_pair (2^20 reference word pairs
and the 64 crossed extremes), rounded up to one digit; the margin is for other inputs and for the float32 scaling by sigma / sqrt(2) in the consumers.  The
consumers' errors scale with sigma (the sigmas used here are powers of two: exactly), so their bar is sigma x EPS."""
import numpy as np
import pytest

import dev_abi
import noise_ref as nr
from gpu_kit import torch_dev  # noqa: F401
from noise_ref import EPS

pytestmark = pytest.mark.gpu

NEOO = 1152
B = 3
EXTREMES = np.array([0, 1, 1 << 24, (1 << 24) + 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], np.uint32)


@pytest.fixture(scope="module")
def L(torch_dev):
    return dev_abi.load()


@pytest.fixture(scope="module")
def eng(torch_dev):
    from radae_amd.engine import BatchEngine
    e = BatchEngine(B, max_tx_mf=2)
    yield e
    e.close()


def probe(L, dev, ctr, key, u=None, m=None):
    """-> (words uint32 [n, 4], g float32 [m, 2]) of one rd_launch_noise_probe call; u None with m: the pairs come from the call's own words"""
    import torch
    from radae_amd.engine import _stream_ptr

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)
    n = 0 if ctr is None else len(ctr)
    m = len(u) if u is not None else (m or 0)
    ctr_d = up(ctr) if n else None
    u_d = up(u) if u is not None else None
    words = torch.full((max(n, 1), 4), -1, dtype=torch.int32, device=dev)
    g = torch.full((max(m, 1), 2), float("nan"), dtype=torch.float32, device=dev)
    rc = L.rd_launch_noise_probe(ctr_d.data_ptr() if n else None, key[0], key[1], u_d.data_ptr() if u_d is not None else None, words.data_ptr(), g.data_ptr(),
                                 n, m, _stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return words.cpu().numpy().view(np.uint32)[:n], g.cpu().numpy()[:m]


def dev_err(got, ref):
    """largest |device - reference| over a real array (float64), after the finiteness check"""
    assert np.isfinite(got).all()
    return float(np.abs(got.astype(np.float64) - ref).max())


def max_part(d):
    """largest component (not modulus) of a complex difference: the bar is per real sample"""
    assert np.isfinite(d.real).all() and np.isfinite(d.imag).all()
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))


def hold(err, bar, what=""):
    """print the figure, then hold it to its bar"""
    print(f"  max |device - reference| {err:.3e} (bar {bar:.3e}) {what}")
    assert err <= bar, (err, bar, what)


# ================================================================================================================================================================
# the probe: philox4x32 and gauss_pair alone
# ================================================================================================================================================================
def test_probe_known_answers(L, torch_dev):
    for ctr, key, want in nr.KNOWN_ANSWERS:
        words, _ = probe(L, torch_dev, np.array([ctr], np.uint32), key)
        assert [int(w) for w in words[0]] == list(want), [hex(int(w)) for w in words[0]]


def test_probe_philox_random_counters_and_keys(L, torch_dev):
    """2^20 counters with all four words random, under four keys (both words, the low one alone, the high one alone, all ones): equal to the reference bit for bit"""
    rng = np.random.default_rng(20)
    keys = [tuple(int(k) for k in rng.integers(0, 1 << 32, 2)), (int(rng.integers(1, 1 << 32)), 0), (0, int(rng.integers(1, 1 << 32))), (0xffffffff, 0xffffffff)]
    for key in keys:
        ctr = rng.integers(0, 1 << 32, (1 << 18, 4), dtype=np.uint64).astype(np.uint32)
        ctr[:4] = np.diag([0xffffffff] * 4)                      # one word alone
        words, _ = probe(L, torch_dev, ctr, key)
        ref = np.stack(nr.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key), axis=1)
        bad = np.nonzero((words != ref).any(axis=1))[0]
        assert bad.size == 0, (key, bad[:4], words[bad[:1]], ref[bad[:1]])


def test_probe_gauss_pair(L, torch_dev):
    """THE measurement behind EPS: 2^20 reference word pairs (key (1234, 0), counters 0 .. 2^19 - 1, both pairs) and the extremes crossed"""
    r = nr.philox4x32_10(np.arange(1 << 19), 0, 0, 0, 1234, 0)
    u = np.concatenate([np.stack([r[0], r[1]], axis=1), np.stack([r[2], r[3]], axis=1),
                        np.stack(np.meshgrid(EXTREMES, EXTREMES, indexing="ij"), axis=-1).reshape(-1, 2)])
    assert u.shape == ((1 << 20) + 64, 2)
    _, g = probe(L, torch_dev, None, (0, 0), u=u)
    x, y = nr.gauss_pair(u[:, 0], u[:, 1])
    ref = np.stack([x, y], axis=1)
    assert np.isfinite(g).all()
    d = np.abs(g.astype(np.float64) - ref)
    k = np.unravel_index(np.argmax(d), d.shape)
    print(f"gauss_pair: max |device - float64| = {d.max():.3e} at u = ({int(u[k[0], 0]):#x}, {int(u[k[0], 1]):#x}) component {k[1]} (reference {ref[k]:.6f}); "
          f"random pairs {d[:1 << 20].max():.3e}, extremes {d[1 << 20:].max():.3e}; EPS {EPS:.1e}")
    assert EPS <= 1e-4
    assert d.max() <= EPS
    # a = 1 gives exactly zero; the largest radius is finite
    assert np.all(g[-8:] == 0.0) and abs(np.hypot(*g[1 << 20].astype(np.float64)) - np.sqrt(66 * np.log(2))) <= EPS
    # without u the pairs are the call's own words: words 0-1 then 2-3 of each counter
    n = 1000
    ctr = np.zeros((n, 4), np.uint32); ctr[:, 0] = np.arange(n)
    words, g2 = probe(L, torch_dev, ctr, (1234, 0), m=2 * n)
    _, g3 = probe(L, torch_dev, None, (0, 0), u=words.reshape(2 * n, 2))
    assert np.array_equal(g2.view(np.uint32), g3.view(np.uint32))
    assert np.array_equal(words[:, 0], r[0][:n]) and np.array_equal(words[:, 3], r[3][:n])


# ================================================================================================================================================================
# the rate-Fs channel (k_chan_apply): counter (p, b, 0, 0), words 0-1 -> sample 2p, 2-3 -> sample 2p + 1
# ================================================================================================================================================================
def fs_noise(eng, dev, n_sig, seed, sigma=1.0, **kw):
    import torch
    tx = torch.zeros((B, n_sig), dtype=torch.complex64, device=dev)
    return eng.channel(tx, sigma, seed=seed, **kw).cpu().numpy()


def test_fs_odd_total_and_real_noise_outside_the_signal(eng, torch_dev):
    """n_total = 1461 is odd: the last counter feeds one sample.  In n_pre and n_post the noise is real with the full sigma, inside complex with 1 / sqrt(2) each"""
    n_pre, n_sig, n_post = 301, 960, 200
    rx = fs_noise(eng, torch_dev, n_sig, 5, n_pre=n_pre, n_post=n_post)
    ref = nr.chan_fs(5, B, n_pre, n_sig, 0, n_post)
    assert rx.shape == ref.shape == (B, 1461)
    out = np.r_[0:n_pre, n_pre + n_sig:1461]
    assert np.all(rx[:, out].imag == 0.0)
    gx = ref[:, out].real                                        # the full g.x outside
    hold(max_part(rx[:, out] - gx), EPS, "n_pre and n_post")
    hold(max_part(rx - ref), EPS, "whole output")
    for b in range(B):                                           # every stream is its own b, and no other
        for c in range(B):
            assert (max_part(rx[b] - ref[c]) <= EPS) == (b == c)


def test_fs_grid_wraps(eng, torch_dev):
    """more than 16384 samples per stream: the 32 workgroups of a stream go round"""
    n_pre, n_sig = 301, 18 * 960
    rx = fs_noise(eng, torch_dev, n_sig, 5, n_pre=n_pre)
    assert rx.shape[1] > 16384
    hold(max_part(rx - nr.chan_fs(5, B, n_pre, n_sig, 0, 0)), EPS)


def test_fs_seed_words(eng, torch_dev):
    """both words of the seed are the key"""
    seeds = [5, (1 << 32) + 5, 5 << 32]
    rx = [fs_noise(eng, torch_dev, 960, s, n_pre=301, n_post=200) for s in seeds]
    for s, r in zip(seeds, rx):
        hold(max_part(r - nr.chan_fs(s, B, 301, 960, 0, 200)), EPS, hex(s))
    for i in range(3):
        for j in range(i):
            assert max_part(rx[i] - rx[j]) > 1.0


def test_fs_per_stream_sigma(eng, torch_dev):
    sig = np.float32([0.5, 2.0, 0.0])
    rx = fs_noise(eng, torch_dev, 960, 5, sigma=sig, n_pre=301, n_post=200)
    ref = nr.chan_fs(5, B, 301, 960, 0, 200)
    for b in range(2):
        hold(max_part(rx[b] - float(sig[b]) * ref[b]), float(sig[b]) * EPS, f"stream {b}")
    assert np.all(rx[2].view(np.float32) == 0.0)


def test_fs_end_of_over_frame(eng, torch_dev):
    """with_eoo: the end-of-over frame carries complex noise like the signal; rx(seed) - rx(seed = 0) is the noise, within EPS and one float32 ulp of the largest sample"""
    kw = dict(n_pre=301, n_post=200, with_eoo=True)
    rx0 = fs_noise(eng, torch_dev, 960, 0, **kw)
    rx = fs_noise(eng, torch_dev, 960, 5, **kw)
    assert np.abs(rx0[:, 301 + 960:301 + 960 + NEOO]).max() > 0.1 and np.all(rx0[:, :301 + 960] == 0)
    ulp = float(np.spacing(np.float32(np.abs(rx0).max())))
    d = rx.astype(np.complex128) - rx0.astype(np.complex128)
    hold(max_part(d - nr.chan_fs(5, B, 301, 960, NEOO, 200)), EPS + ulp)


def test_fs_fused_transmit_with_multipath(eng, torch_dev):
    """tx_channel with a device G: the modulator's own multipath output (rd_chan_args.mp) goes through the same noise"""
    import torch
    from radae_amd.channel_tools import synth_features
    feats = torch.tensor(np.stack([synth_features(31 + b, 24) for b in range(B)]), device=torch_dev)
    G = eng.multipath_gen("mpp", 2 * 960, seed=3)
    kw = dict(n_pre=301, n_post=200, with_eoo=True, G=G)
    eng.tx_reset()
    rx0 = eng.tx_channel(feats, 1.0, seed=0, **kw).cpu().numpy()
    eng.tx_reset()
    rx = eng.tx_channel(feats, 1.0, seed=5, **kw).cpu().numpy()
    assert np.abs(rx0[:, 301:301 + 1920]).max() > 0.1
    ulp = float(np.spacing(np.float32(np.abs(rx0).max())))
    d = rx.astype(np.complex128) - rx0.astype(np.complex128)
    hold(max_part(d - nr.chan_fs(5, B, 301, 2 * 960, NEOO, 200)), EPS + ulp)


def test_fs_seed_zero_is_noiseless(eng, torch_dev):
    """seed 0 and no noise tensor: the signal bit for bit (no G, no offset: the samples themselves), zeros around it"""
    import torch
    rng = np.random.default_rng(8)
    tx = (rng.standard_normal((B, 960)) + 1j * rng.standard_normal((B, 960))).astype(np.complex64)
    rx = eng.channel(torch.tensor(tx, device=torch_dev), 1.0, n_pre=301, n_post=200, seed=0).cpu().numpy()
    assert np.array_equal(rx[:, 301:301 + 960].view(np.uint32), tx.view(np.uint32))
    assert np.all(rx[:, :301].view(np.uint32) == 0) and np.all(rx[:, 301 + 960:].view(np.uint32) == 0)


# ================================================================================================================================================================
# the symbol channel (k_chan_symbol): counter (i >> 1, 0, 0, 0) over the flat index of the whole call, words 0-1
# ================================================================================================================================================================
@pytest.mark.parametrize("n", [5, 8800])
def test_symbol_rs(eng, torch_dev, n):
    """mode rs, sigma 2.  n = 8800: B n 80 = 2,112,000 > 8192 x 256, the grid goes round.  The draw is not keyed by stream: stream b continues where b - 1 ended"""
    import torch
    z = torch.zeros((B, n, 80), device=torch_dev)
    out = eng.channel_symbol(z, "rs", 2.0, seed=(3 << 32) + 5).cpu().numpy()
    assert B * n * 80 > 2097152 or n == 5
    ref = 2.0 * nr.chan_symbol((3 << 32) + 5, B * n * 80, "rs").reshape(B, n, 80)
    hold(dev_err(out, ref), 2.0 * EPS)
    assert np.abs(out[1] - out[0]).max() > 1.0


def test_symbol_bbfm(eng, torch_dev):
    """mode bbfm, CNR 20 dB, Gfm 0, no H: SNR 20 dB, sigma 0.1 (computed here in float64; the kernel's float32 powf is inside the 1e-6), unit-variance real noise"""
    import torch
    n = 5
    z = torch.zeros((B, n, 80), device=torch_dev)
    out = eng.channel_symbol(z, "bbfm", 20.0, 0.0, seed=5).cpu().numpy()
    snr_dB = max(20.0 - 12.0, 0.0) + 12.0 + 0.0 - max(12.0 - 20.0, 0.0) * (1.0 + 0.0 / 3.0)
    sigma = 1.0 / np.sqrt(10.0 ** (snr_dB / 10.0))
    ref = sigma * nr.chan_symbol(5, B * n * 80, "bbfm").reshape(B, n, 80)
    assert abs(sigma - 0.1) < 1e-15 and np.abs(ref).max() < 1.0          # the clamp is never reached
    hold(dev_err(out, ref), 0.1 * EPS + 1e-6)


# ================================================================================================================================================================
# the rate-Rs channel (k_rs_pa): counter (i >> 1, b, 2, 0), words 0-1 -> even carrier, 2-3 -> odd carrier
# ================================================================================================================================================================
@pytest.mark.parametrize("n,seed", [(1, 5), (7, 5), (37, 5), (7, (9 << 32) + 5)])
def test_rate_rs(eng, torch_dev, n, seed):
    """z = 0 leaves sigma x noise.  n = 37: 74 symbols are ten tiles of eight, so the eight chunks go round and the last tile is partial"""
    import torch
    z = torch.zeros((B, n, 80), device=torch_dev)
    out = eng.channel_rs_pa(z, 2.0, seed=seed).cpu().numpy()
    hold(dev_err(out, 2.0 * nr.chan_rs(seed, B, n)), 2.0 * EPS)
    if seed != 5:
        assert np.abs(out - 2.0 * nr.chan_rs(5, B, n)).max() > 1.0


# ================================================================================================================================================================
# the Doppler generator (k_multipath_gen): counter (xi, 2 b + p, 1, 0), words 0-1
# ================================================================================================================================================================
@pytest.mark.parametrize("channel,n_out,seed", [("mpp", 4 * 960, 4), ("lmr60", 2049 * 15 - 4, 4), ("mpp", 960, (6 << 32) + 4)])
def test_doppler_generator(eng, torch_dev, channel, n_out, seed):
    """the generator fed from the seed against the same generator fed the reference's low-rate noise.  lmr60: 2049 low-rate points, past what the kernel keeps in LDS.
    Bar: an input sample off by EPS moves a filtered point by at most EPS sum |taps|, scaled by hf_gain; plus the 2e-5 of the explicit-noise parity test (the
    reference input is rounded to complex64)."""
    import torch
    from radae_amd.channel_tools import PRESETS, doppler_plan
    taps, ratio, n_low = doppler_plan(PRESETS[channel][0], 8000, n_out)
    taps = taps.astype(np.float32).astype(np.float64)
    assert (n_low > 2048) == (channel == "lmr60")
    low = nr.multipath_low(seed, B, n_low, len(taps))
    G_seed = eng.multipath_gen(channel, n_out, seed=seed).cpu().numpy()
    G_ref = eng.multipath_gen(channel, n_out, seed=99, noise_low=torch.tensor(low, device=torch_dev)).cpu().numpy()
    pos = np.arange(n_out) / ratio
    i0 = np.minimum(np.floor(pos).astype(np.int64), n_low - 2)
    for b in range(B):
        var = 0.0
        for p in range(2):                                       # hf_gain of the explicit-noise run: 1 / sqrt(var G1 + var G2) ahead of the scaling
            y = np.convolve(low[b, p].astype(np.complex128), taps)[len(taps):len(taps) + n_low]
            var += np.var(y[i0] + (y[i0 + 1] - y[i0]) * (pos - i0))
        bar = EPS * np.abs(taps).sum() / np.sqrt(var) + 2e-5
        hold(max_part(G_seed[b].astype(np.complex128) - G_ref[b]), bar, f"stream {b}")
    flat = [G_seed[b, :, p] for b in range(B) for p in range(2)]
    for i in range(len(flat)):
        for j in range(i):
            assert np.abs(flat[i] - flat[j]).max() > 1e-2
