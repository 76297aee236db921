"""rade_batch_channel_piece and rade_batch_multipath_piece (radae_amd/csrc/rade_chanp.hip) on the device, B = 3, every output in a padded, offset buffer with an odd
stride between sentinels: nothing outside a written extent changes, no input changes.

1. pieces equal one piece, bit for bit, for both kernels: 4,099 samples cut at 1, 15, 16, 17, 255, 257, 959, 961 and the rest, in another order for every stream, from
   odd start indices and from 2^33 + 5 (the fourth counter word is non-zero there and the phase has wrapped), the generator also at 2^32 + 3 with low_ratio 1;
2. every sample of those runs against the float64 restatement tests/chanp_ref.py, within the bounds derived there;
3. anchors to the whole-utterance calls: (a) rade_batch_channel with generated noise equals three piece calls bit for bit, (b) the two-path model with the reference's
   gain, (c) a 10 Hz offset against the float32 phase of the whole call, (d) k_dopp_piece against rade_batch_multipath_gen where that does not extrapolate;
4. ChannelStream("mpp", 6 dB, +8 Hz) in pieces of 1,000, 7,777 and the rest, through rade_batch_rx in three invocations, against one piece fed once;
and the refusals (each -1, nothing written) and per-stream arrays against scalars.

Largest observed error / bound on the MI355X (test 2; each must stay below 1): see the docstrings of test_generator and test_channel."""
import ctypes as C

import numpy as np
import pytest

import chanp_ref as cp
import kernel_ref as kr
import noise_ref as nr
import tx_ref as tx
from gpu_kit import engine, engines, stream, sync, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

B, N, SEED = 3, 4099, 0x1234567887654321
CUTS = [1, 15, 16, 17, 255, 257, 959, 961]
BIG = 2 ** 33 + 5


def cut_plan():
    """(starts, lens) int64 [B][9]: the eight lengths in another order for every stream, the rest last"""
    lens = np.array([CUTS[3 * b:] + CUTS[:3 * b] + [N - sum(CUTS)] for b in range(B)], np.int64)
    return np.cumsum(lens, axis=1) - lens, lens


@pytest.fixture(scope="module")
def eng(engines):
    return engines(B)


def crand(rng, shape, scale=1.0):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * (scale / np.sqrt(2))).astype(np.complex64)


# ---- sentinel buffers -----------------------------------------------------------------------------------------------------------------------------------------------
class Out:
    """complex64 rows [B, width] (inner = 1) or pairs [B, width, 2] (inner = 2) at element off + b stride inner of a flat tensor filled with sentinels"""

    def __init__(self, dev, width, stride, off, inner=1):
        import torch
        self.width, self.stride, self.off, self.inner = width, stride * inner, off, inner
        n = off + (B - 1) * self.stride + width * inner + 64
        self.flat = torch.from_numpy(np.full(2 * n, kr.SENT32, np.uint32).view(np.complex64)).to(dev)
        self.rows = torch.as_strided(self.flat, (B, width) if inner == 1 else (B, width, 2), (self.stride, 1) if inner == 1 else (self.stride, 2, 1), off)

    def take(self, n_out, what):
        """the n_out[b] written elements of every row; everything else must still be the sentinel"""
        w = self.flat.cpu().numpy().view(np.uint32).reshape(-1, 2)
        outside = np.ones(len(w), bool)
        got = []
        for b in range(B):
            lo = self.off + b * self.stride
            outside[lo:lo + int(n_out[b]) * self.inner] = False
            v = np.ascontiguousarray(w[lo:lo + int(n_out[b]) * self.inner]).view(np.complex64).ravel()
            assert not (v.view(np.uint32) == kr.SENT32).any(), f"{what}: stream {b} has unwritten samples inside its extent"
            got.append(v.reshape(-1, 2) if self.inner == 2 else v)
        bad = np.flatnonzero(outside & (w != kr.SENT32).any(axis=1))
        assert not bad.size, f"{what}: {bad.size} samples written outside the documented extents, the first at element {bad[0]}"
        return got


class In:
    """host arrays uploaded as they are; unchanged() compares every word"""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def put(self, a):
        import torch
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.copy()).to(self.dev)
        self.items.append((t, a))
        return t

    def unchanged(self):
        for i, (t, a) in enumerate(self.items):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32)), f"input buffer {i} was written"


def odd(n):
    return n | 1


# ================================================================================================================================================================
# the generator
# ================================================================================================================================================================
def preset_taps(n_taps):
    from radae_amd import channel_tools as ct
    t = np.asarray(ct.doppler_plan(ct.PRESETS["mpp"][0], 8000, 2)[0], np.float32)
    return t[50 - n_taps // 2:50 - n_taps // 2 + n_taps].copy() if n_taps < 100 else t


def run_gen(eng, dev, taps, ratio, n0, n_out, hf_gain, off):
    o = Out(dev, int(max(n_out)), odd(int(max(n_out)) + 4), off, inner=2)
    eng.multipath_piece(taps, ratio, n_out, n0=n0, seed=SEED, hf_gain=hf_gain, out=o.rows)
    sync()
    return o.take(n_out, f"k_dopp_piece ratio {ratio} taps {len(taps)} n0 {list(n0)}")


@pytest.mark.parametrize("n_taps", [1, 100])
@pytest.mark.parametrize("ratio", [1, 16, 800])
def test_generator(eng, torch_dev, ratio, n_taps):
    """pieces (8-byte stores: a base at an odd element) equal one piece (16-byte stores), bit for bit, and every sample of the one piece lies within dopp_ref's bound.
    n_taps = 100 runs with the default gain (rade_multipath_gain), n_taps = 1 with a given one.
    Largest error / bound observed on the MI355X (ratio, taps): (1, 1) 0.189, (1, 100) 0.036, (16, 1) 0.131, (16, 100) 0.031, (800, 1) 0.108, (800, 100) 0.033."""
    taps = preset_taps(n_taps)
    hf = 0.0 if n_taps == 100 else 1.7
    hf_ref = cp.multipath_gain(taps) if n_taps == 100 else 1.7
    starts, lens = cut_plan()
    bases = [np.array([1, 12345, 7], np.int64), BIG + np.array([0, 2, 7], np.int64)] + ([2 ** 32 + 3 + np.array([0, 1, 4], np.int64)] if ratio == 1 else [])
    worst = 0.0
    for base in bases:
        whole = run_gen(eng, torch_dev, taps, ratio, base, np.full(B, N, np.int32), hf, off=2)
        parts = [run_gen(eng, torch_dev, taps, ratio, base + starts[:, k], lens[:, k].astype(np.int32), hf, off=1) for k in range(lens.shape[1])]
        for b in range(B):
            what = f"k_dopp_piece ratio {ratio} taps {n_taps} n0 {base[b]} stream {b}"
            tx.check_bits(np.concatenate([p[b] for p in parts]), whole[b], what + ": pieces against one piece", ("sample", "component of path"))
            worst = max(worst, cp.check_dopp(whole[b], cp.dopp_ref(taps, ratio, hf_ref, SEED, b, int(base[b]), N), what))
    print(f"k_dopp_piece ratio {ratio} taps {n_taps}: largest error / bound {worst:.3f}")
    assert worst < 1.0


# ================================================================================================================================================================
# the channel
# ================================================================================================================================================================
F0 = np.array([10.0, -3.5, 1999.0], np.float32)
DF = np.array([0.5, 0.0, -0.25], np.float32)
SIGMA = np.array([0.5, 0.3, 0.7], np.float32)
GAIN = np.array([1.0, 1.5, 0.75], np.float32)
CHAN_CASES = {
    "awgn_complex_rot_tone": dict(G=False, noise="complex", f0=F0, df=DF, tone=True),
    "awgn_real": dict(G=False, noise="real", f0=0.0, df=0.0, tone=False),
    "mp_complex_rot_tone": dict(G=True, noise="complex", f0=F0, df=DF, tone=True),
    "mp_explicit_rot": dict(G=True, noise="explicit", f0=10.0, df=0.0, tone=False),
    "mp_real_drift": dict(G=True, noise="real", f0=0.0, df=DF, tone=True),
    "mp_quiet": dict(G=True, noise=None, f0=0.0, df=0.0, tone=False),
}
TONE = dict(sine_amp=0.3, sine_freq=1234.5, rx_gain=0.5)


class Stream:
    """one stream's transmit, Doppler and noise samples over absolute indices: tx and G from max(base - 16, 0), noise from base"""

    def __init__(self, rng, base):
        self.base, self.lo = int(base), max(int(base) - 16, 0)
        n = self.base + N - self.lo
        self.tx, self.G, self.noise = crand(rng, n, 0.8), crand(rng, (n, 2)), crand(rng, N)

    def window(self, n0, n_out):
        """(lo, tx, G, noise) a piece [n0, n0 + n_out) needs: the transmit and Doppler samples from 16 in front of it, its own noise"""
        lo = max(n0 - 16, 0)
        return lo, self.tx[lo - self.lo:n0 + n_out - self.lo], self.G[lo - self.lo:n0 + n_out - self.lo], self.noise[n0 - self.base:n0 - self.base + n_out]


def run_chan(eng, dev, c, streams, n0, n_out, off):
    """one call: every stream's window uploaded in rows padded with huge values (a read outside a row would show), the output between sentinels"""
    wins = [s.window(int(n0[b]), int(n_out[b])) for b, s in enumerate(streams)]
    L = max(len(w[1]) for w in wins) + 3
    txh, Gh, nzh = np.full((B, L), 1e30 + 1e30j, np.complex64), np.full((B, L, 2), 1e30 - 1e30j, np.complex64), np.full((B, max(int(max(n_out)), 1)), 1e30, np.complex64)
    for b, (lo, t, g, nz) in enumerate(wins):
        txh[b, :len(t)] = t; Gh[b, :len(g)] = g; nzh[b, :len(nz)] = nz
    i = In(dev)
    o = Out(dev, int(max(n_out)), odd(int(max(n_out)) + 4), off)
    kw = dict(TONE) if c["tone"] else {}
    if c["G"]:
        kw.update(G=i.put(Gh), g_base=[w[0] for w in wins], n_g=[len(w[2]) for w in wins])
    if c["noise"] == "explicit":
        kw.update(noise=i.put(nzh))
    elif c["noise"]:
        kw.update(seed=SEED, real_noise=c["noise"] == "real")
    eng.channel_piece(i.put(txh), SIGMA, c["f0"], c["df"], GAIN, n0=n0, in_base=[w[0] for w in wins], n_in=[len(w[1]) for w in wins], n_out=n_out, out=o.rows, **kw)
    sync()
    i.unchanged()
    return o.take(n_out, f"k_chan_piece n0 {list(n0)}")


def chan_ref_of(c, s, b, **over):
    f0, df = (np.broadcast_to(np.asarray(v, np.float32), (B,))[b] for v in (c["f0"], c["df"]))
    kw = dict(TONE) if c["tone"] else {}
    if c["noise"] == "explicit":
        kw.update(noise=s.noise)
    elif c["noise"]:
        kw.update(seed=SEED, noise_mode=cp.NOISE_REAL if c["noise"] == "real" else cp.NOISE_COMPLEX)
    return cp.chan_ref(s.tx, s.lo, s.base, N, b=b, G=s.G if c["G"] else None, g_base=s.lo, gain=GAIN[b], sigma=SIGMA[b], freq_offset=f0, df_dt=df, **{**kw, **over})


@pytest.mark.parametrize("name", list(CHAN_CASES))
def test_channel(eng, torch_dev, name):
    """pieces (each handed only its own window of tx, G and noise) equal one piece, bit for bit, across the two store paths (row offsets 3 and 2), and every sample of the
    one piece lies within chan_ref's bound.  Largest error / bound observed on the MI355X: awgn_complex_rot_tone 0.116, awgn_real 0.133, mp_complex_rot_tone 0.113,
    mp_explicit_rot 0.200, mp_real_drift 0.130, mp_quiet 0.330."""
    c = CHAN_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    starts, lens = cut_plan()
    worst = 0.0
    for base in (np.array([1, 33, 1001], np.int64), BIG + np.array([0, 1, 2], np.int64)):
        streams = [Stream(rng, base[b]) for b in range(B)]
        whole = run_chan(eng, torch_dev, c, streams, base, np.full(B, N, np.int32), off=2)
        parts = [run_chan(eng, torch_dev, c, streams, base + starts[:, k], lens[:, k].astype(np.int32), off=3) for k in range(lens.shape[1])]
        for b in range(B):
            what = f"k_chan_piece {name} n0 {base[b]} stream {b}"
            tx.check_bits(np.concatenate([p[b] for p in parts]), whole[b], what + ": pieces against one piece", ("sample",))
            worst = max(worst, cp.check_chan(whole[b], chan_ref_of(c, streams[b], b), what))
    print(f"k_chan_piece {name}: largest error / bound {worst:.3f}")
    assert worst < 1.0


def test_per_stream_arrays_equal_scalars(eng, torch_dev):
    """stream b of a call with [B] arrays equals stream b of the call with its values as the scalars, bit for bit"""
    c = CHAN_CASES["mp_complex_rot_tone"]
    rng = np.random.default_rng(5)
    base = np.array([7, 16, 901], np.int64)
    streams = [Stream(rng, base[b]) for b in range(B)]
    n_out = np.array([300, 257, 31], np.int32)
    got = run_chan(eng, torch_dev, c, streams, base, n_out, off=1)
    import torch
    for b in range(B):
        lo, t, g, _ = streams[b].window(int(base[b]), int(n_out[b]))
        t_d = torch.tensor(np.broadcast_to(t, (B, len(t))).copy(), device=torch_dev); g_d = torch.tensor(np.broadcast_to(g, (B,) + g.shape).copy(), device=torch_dev)
        rx, _ = eng.channel_piece(t_d, float(SIGMA[b]), float(F0[b]), float(DF[b]), float(GAIN[b]), n0=int(base[b]), in_base=lo, n_out=int(n_out[b]), G=g_d, g_base=lo,
                                  seed=SEED, **TONE)
        tx.check_bits(rx[b, :n_out[b]].cpu().numpy(), got[b], f"stream {b}: arrays against scalars", ("sample",))


# ================================================================================================================================================================
# refusals
# ================================================================================================================================================================
def test_refusals_write_nothing(eng, torch_dev):
    from radae_amd.abi import ChannelPieceParams
    import torch
    n, L = 100, 131
    txd = torch.zeros((B, L), dtype=torch.complex64, device=torch_dev); Gd = torch.zeros((B, L, 2), dtype=torch.complex64, device=torch_dev)
    nzd = torch.zeros((B, n), dtype=torch.complex64, device=torch_dev)
    o = Out(torch_dev, L, odd(L + 4), 1); og = Out(torch_dev, L, odd(L + 4), 1, inner=2)
    keep = []

    def arr(v, dt):
        keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (B,))))
        return keep[-1].ctypes.data

    def chan(tx_ptr=txd.data_ptr(), tx_stride=L, n_in=n + 16, rx_ptr=o.rows.data_ptr(), rx_stride=o.stride, n_out=n, p_null=False, **f):
        p = ChannelPieceParams()
        base = dict(n0=16, in_base=0, g_base=0, sigma=0.5, freq_offset=10.0, gain=1.0, seed=3, G_dev=Gd.data_ptr(), g_stride=L, n_g_host=n + 16)
        for k, v in {**base, **f}.items():
            if k.endswith("_host") and v is not None:                     # a value (every stream) or B values -> a [B] host array
                v = arr(v, np.int32 if k == "n_g_host" else np.int64 if k in ("n0_host", "in_base_host", "g_base_host") else np.float32)
            setattr(p, k, v)
        return eng.lib.rade_batch_channel_piece(eng.h, tx_ptr, tx_stride, None if n_in is None else arr(n_in, np.int32), rx_ptr, rx_stride,
                                                None if n_out is None else arr(n_out, np.int32), None if p_null else C.byref(p), stream())

    bad = [dict(tx_ptr=None), dict(rx_ptr=None), dict(n_in=None), dict(n_out=None), dict(p_null=True), dict(n_g_host=None),
           dict(tx_ptr=txd.data_ptr() + 4), dict(rx_ptr=o.rows.data_ptr() + 4), dict(G_dev=Gd.data_ptr() + 4), dict(noise_dev=nzd.data_ptr() + 4),
           dict(n_in=-1), dict(n_out=-1), dict(n_in=[5, 5, -1]), dict(n_g_host=[116, -1, 116]),
           dict(n0=-1), dict(in_base=-1), dict(g_base=-1), dict(n0_host=[16, 16, -1]), dict(in_base_host=[0, -1, 0]), dict(g_base_host=[-1, 0, 0]),
           dict(n0=2 ** 62 + 1, G_dev=None), dict(in_base=2 ** 62 + 1), dict(g_base=2 ** 62 + 1), dict(n0=2 ** 62 - 50, in_base=2 ** 62 - 50, G_dev=None),
           dict(tx_stride=n + 15), dict(rx_stride=n - 1), dict(g_stride=n + 15),
           dict(g_base=1), dict(n_g_host=n + 15), dict(n0=17), dict(n0_host=[16, 16, 18]),
           dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=-0.5), dict(sigma_host=[0.1, -0.1, 0.1]),
           dict(freq_offset=float("nan")), dict(freq_offset=2000.5), dict(freq_offset=-2000.5), dict(freq_offset_host=[0.0, 0.0, 2001.0]),
           dict(df_dt=float("inf")), dict(df_dt=1.7e7), dict(gain=float("nan")), dict(gain_host=[1.0, float("inf"), 1.0]),
           dict(sine_amp=float("nan")), dict(sine_freq=float("inf")), dict(rx_gain=float("nan")), dict(noise_mode=2), dict(noise_mode=-1)]
    for f in bad:
        assert chan(**f) == -1, f"rade_batch_channel_piece accepted {f}"

    taps = preset_taps(100)

    def gen(taps_ptr=taps.ctypes.data, n_taps=100, ratio=800, hf=0.0, n0=5, n_out=n, G_ptr=og.rows.data_ptr(), g_stride=og.stride // 2):
        return eng.lib.rade_batch_multipath_piece(eng.h, taps_ptr, n_taps, ratio, hf, SEED, None if n0 is None else arr(n0, np.int64), None if n_out is None else arr(n_out, np.int32),
                                                  G_ptr, g_stride, stream())

    nan_taps = taps.copy(); nan_taps[7] = np.nan
    badg = [dict(taps_ptr=None), dict(n_out=None), dict(G_ptr=None), dict(G_ptr=og.rows.data_ptr() + 4), dict(n_taps=0), dict(n_taps=257), dict(ratio=0), dict(ratio=-3),
            dict(hf=float("nan")), dict(hf=float("inf")), dict(hf=-1.0), dict(taps_ptr=nan_taps.ctypes.data), dict(taps_ptr=nan_taps.ctypes.data, hf=1.0),
            dict(n_out=-1), dict(n_out=[n, -1, n]), dict(n0=-1), dict(n0=[5, 5, -1]), dict(n0=2 ** 62 + 1), dict(n0=2 ** 62 - 50), dict(g_stride=n - 1)]
    for f in badg:
        assert gen(**f) == -1, f"rade_batch_multipath_piece accepted {f}"
    sync()
    o.take(np.zeros(B, np.int32), "refused channel calls"); og.take(np.zeros(B, np.int32), "refused generator calls")
    assert chan() == 0 and gen() == 0 and gen(n0=None) == 0 and chan(n_out=0) == 0          # what the refused calls were variations of
    sync()
    o.take(np.full(B, n, np.int32), "the accepted channel call"); og.take(np.full(B, n, np.int32), "the accepted generator call")


# ================================================================================================================================================================
# 3. anchors to the whole-utterance calls
# ================================================================================================================================================================
def test_anchor_awgn_equals_three_pieces(eng, torch_dev):
    """(a) rade_batch_channel, generated noise, no frequency offset, n_pre = 7, n_sig = 960, n_post = 5 and a tone: real noise over [0, 7), complex over [7, 967) with
    in_base = 7, real over [967, 972) -- three piece calls, bit for bit"""
    import torch
    rng = np.random.default_rng(21)
    txd = torch.tensor(crand(rng, (B, 960), 0.8), device=torch_dev)
    kw = dict(sine_amp=0.3, sine_freq=1234.5, rx_gain=0.5)
    whole = eng.channel(txd, 0.6, 0.0, n_pre=7, n_post=5, seed=SEED, **kw).cpu().numpy()
    pieces = [eng.channel_piece(txd, 0.6, n0=0, in_base=0, n_in=0, n_out=7, seed=SEED, real_noise=True, **kw)[0],
              eng.channel_piece(txd, 0.6, n0=7, in_base=7, n_out=960, seed=SEED, **kw)[0],
              eng.channel_piece(txd, 0.6, n0=967, in_base=0, n_in=0, n_out=5, seed=SEED, real_noise=True, **kw)[0]]
    tx.check_bits(np.concatenate([p.cpu().numpy() for p in pieces], axis=1), whole, "three pieces against rade_batch_channel", ("stream", "sample"))


def test_anchor_two_path_with_the_reference_gain(eng, torch_dev):
    """(b) with G and gain_b = the float64 reference's sqrt(tx power / two-path power), rounded to float32, the piece matches the whole call: both lie within their
    bounds of the same float64 value, so |piece - whole| <= check_chan's bound (tests/tx_ref.py, the whole call) + chan_ref's bound (the piece, which takes the gain as
    a float32 operand) + u |v| (that operand's rounding)"""
    import torch
    rng = np.random.default_rng(22)
    n = 1920
    txs, G, noise = crand(rng, (B, n), 0.8), crand(rng, (B, n, 2)), crand(rng, (B, n))
    mp = tx.mp_ref(txs, G)[0]
    gain = np.sqrt((np.abs(tx.c128(txs)) ** 2).sum(1) / (np.abs(mp) ** 2).sum(1)).astype(np.float32)
    td, Gd, nd = (torch.tensor(v, device=torch_dev) for v in (txs, G, noise))
    whole = eng.channel(td, 0.6, 0.0, G=Gd, noise=nd).cpu().numpy()
    piece = eng.channel_piece(td, 0.6, gain=gain, G=Gd, g_base=0, noise=nd)[0].cpu().numpy()
    wref = tx.chan_ref(txs, noise, G=G, sigma=0.6)
    tx.check_chan(whole, wref, "rade_batch_channel against its own reference")
    worst = 0.0
    for b in range(B):
        pref = cp.chan_ref(txs[b], 0, 0, n, b=b, G=G[b], g_base=0, gain=gain[b], sigma=0.6, noise=noise[b])
        cp.check_chan(piece[b], pref, f"the piece against its own reference, stream {b}")
        worst = max(worst, tx.check_close(piece[b], whole[b].astype(np.complex128), wref[1][b] + pref[1] + kr.U * np.abs(wref[0][b]), f"(b) piece against whole, stream {b}", ("sample",)))
    print(f"(b) piece against whole: largest difference / bound {worst:.3f}")


def test_anchor_frequency_offset(eng, torch_dev):
    """(c) freq_offset = 10 Hz over 1,920 samples, no noise: |piece - whole| <= |v| (half an ulp of the float32 phase at its largest value + EPS_CIS).
    The bound is 7.87e-07 = 4.77e-07 (half an ulp of the phase 15.08) + 3.10e-07 (EPS_CIS).  It holds because the piece turns at the whole call's rate: without a
    drift f0q is made from the float32 omega ((f0 * 2) * pi) / 8000 that chan_phase_acc adds up (rade_stages.c: piece_turns).  With f0q made from f0 / 8000 in double
    the two rates are 5.2e-08 apart, 7.77e-07 rad at the last sample, and the largest |piece - whole| / |v| observed on the MI355X was 1.334e-06 (795 of 5,760 samples
    outside the bound).  Observed now: 5.64e-07 (sample 1863)."""
    import torch
    rng = np.random.default_rng(23)
    n = 1920
    txs = crand(rng, (B, n), 0.8)
    td = torch.tensor(txs, device=torch_dev)
    whole = eng.channel(td, 0.0, 10.0).cpu().numpy()
    piece = eng.channel_piece(td, 0.0, 10.0)[0].cpu().numpy()
    ph_max = np.float32(tx.chan_phase(n - 1, 10.0, 0.0))
    rel = 0.5 * float(np.spacing(ph_max)) + cp.EPS_CIS
    err = np.abs(piece.astype(np.complex128) - whole) / np.abs(txs)
    print(f"(c) largest |piece - whole| / |v| {err.max():.4g} at sample {int(err.argmax()) % n}; bound {rel:.4g} (half an ulp of {ph_max} + EPS_CIS)")
    tx.check_close(piece, whole.astype(np.complex128), rel * np.abs(txs), "(c) piece against whole", ("stream", "sample"))


def test_anchor_generator(eng, torch_dev):
    """(d) k_dopp_piece with the gain the whole sequence realised (tests/tx_ref.py's mpgen_ref) against rade_batch_multipath_gen, n_out = 4,000 at low_ratio 16: within
    2 float32 ulps per component on every sample the whole generator interpolates, n < (n_low - 1) low_ratio; the last block, which it extrapolates, is left out"""
    import torch
    taps, ratio, n_out = preset_taps(100), 16, 4000
    n_low = tx.n_low_of(ratio, n_out)
    keep = (n_low - 1) * ratio
    assert 0 <= n_out - keep <= ratio
    Gw = torch.zeros((B, n_out, 2), dtype=torch.complex64, device=torch_dev)
    assert eng.lib.rade_batch_multipath_gen(eng.h, taps.ctypes.data_as(C.POINTER(C.c_float)), len(taps), ratio, n_out, None, SEED, Gw.data_ptr(), stream()) == n_out
    whole = Gw.cpu().numpy()
    want, _ = tx.mpgen_ref(nr.multipath_low(SEED, B, n_low, len(taps)).astype(np.complex128), taps, ratio, n_out)
    for b in range(B):
        g, _ = cp.dopp_ref(taps, ratio, 1.0, SEED, b, 0, keep)
        hf = float((want[b, :keep] * g.conj()).real.sum() / (np.abs(g) ** 2).sum())            # the reference's hf_gain of this stream
        got = eng.multipath_piece(taps, ratio, n_out, seed=SEED, hf_gain=hf)[0][b].cpu().numpy()
        a, w = (np.ascontiguousarray(v[:keep]).view(np.float32).astype(np.float64) for v in (got, whole[b]))
        ulps = np.abs(a - w) / np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
        print(f"(d) stream {b}: hf_gain {hf:.6f}, largest difference {ulps.max():.2f} ulps over {keep} of {n_out} samples")
        assert ulps.max() <= 2.0


# ================================================================================================================================================================
# 4. end to end
# ================================================================================================================================================================
def rx_in_turns(e, pieces):
    """feed rade_batch_rx one invocation per piece, every stream's unconsumed samples carried in front of the next piece -> (features per stream, last status, totals)"""
    import torch
    left = [np.zeros(0, np.complex64) for _ in range(e.B)]
    feats = [[] for _ in range(e.B)]
    consumed, st = np.zeros(e.B, np.int64), None
    for p in pieces:
        p = p.cpu().numpy()
        rows = [np.concatenate([left[b], p[b]]) for b in range(e.B)]
        n = np.array([len(r) for r in rows], np.int32)
        buf = np.zeros((e.B, int(n.max())), np.complex64)
        for b, r in enumerate(rows):
            buf[b, :len(r)] = r
        fo, st, _ = e.rx(torch.tensor(buf, device=e.device), n_avail=n)
        fo = fo.cpu().numpy()
        for b in range(e.B):
            feats[b].append(fo[b, :st[b].n_valid]); left[b] = rows[b][st[b].consumed:]; consumed[b] += st[b].consumed
    return [np.concatenate(f) for f in feats], st, consumed


def test_end_to_end_stream_in_pieces(engine, torch_dev):
    """ChannelStream("mpp", 6 dB, +8 Hz) on 2 streams x 40 modem frames, pushed as 1,000 + 7,777 + the rest and received in three invocations, against one 38,400-sample
    piece received in one: the same received samples, status records and feature bits; both streams reach sync"""
    import torch
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import ChannelStream
    n_mf = 40
    e = engine(2, max_tx_mf=n_mf)
    feats = np.stack([synth_features(31 + b, n_mf * 12) for b in range(2)])
    iq = e.tx(torch.tensor(feats, device=torch_dev))
    assert iq.shape == (2, 960 * n_mf)
    one = ChannelStream(e, "mpp", 6.0, 8.0, seed=77).push(iq)
    cs = ChannelStream(e, "mpp", 6.0, 8.0, seed=77)
    pieces = [cs.push(iq[:, a:b].contiguous()) for a, b in ((0, 1000), (1000, 8777), (8777, 960 * n_mf))]
    tx.check_bits(torch.cat(pieces, dim=1).cpu().numpy(), one.cpu().numpy(), "the received stream in pieces against one piece", ("stream", "sample"))
    f1, s1, c1 = rx_in_turns(e, [one])
    e.rx_reset()
    f3, s3, c3 = rx_in_turns(e, pieces)
    for b in range(2):
        assert s1[b].sync == 1 and s3[b].sync == 1, f"stream {b} did not reach sync"
        assert len(f1[b]) > 20 and f1[b].shape == f3[b].shape and np.array_equal(f1[b].view(np.uint32), f3[b].view(np.uint32)), f"stream {b}: features"
        assert c1[b] == c3[b] and all(getattr(s1[b], k) == getattr(s3[b], k) for k in ("nin", "sync", "snr_dB", "state", "has_eoo")), f"stream {b}: status"
    print(f"end to end: {[len(f) for f in f1]} decoded frames per stream, snr {[s.snr_dB for s in s1]} dB")
