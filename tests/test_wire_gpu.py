"""GPU tests (-m gpu) of the sound-card wire (rade_batch_wire_in / rade_batch_wire_out, rade_wire.hip; include/rade_batch.h states the rule): every int16 value in,
saturation / NaN / truncation and the meters out against tests/wire_ref.py, heads and tails of the 16-byte path in sentinel buffers (tests/bands.py), the host-side
refusals, the receiver fed through wire_in against the receiver fed through radae_amd/wire.py, the transmitter through wire_out, and the command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

import wire_ref as wr
from bands import SENTINEL, Band
from gpu_kit import REPO, dev, engines, stream as stream_ptr, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
REAL, IQ = 0, 1
COUNTS = np.array([0, 1, 7, 8, 1031], np.int32)                  # no word, a head alone, head + tail without a word, one word, 128 words + head + tail: more than one chunk has work
SENT16 = np.array([SENTINEL], np.int32).view(np.int16)           # the sentinel word as the two int16 it is made of


def u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


class Band16:
    """B rows of int16 at `stride` int16 elements, row 0 `off` elements behind a 16-byte boundary, inside ONE guarded row of a Band (the band counts 32-bit words; an
    odd stride or offset puts rows on half words).  expect() is the whole allocation as int16 with the sentinel everywhere but where the caller says."""

    def __init__(self, B, stride, off, device):
        words = (off + B * stride + 1) // 2 + 8
        self.band, self.B, self.stride, self.off = Band(1, words, words, 4, device=device), B, stride, off
        self.ptr = self.band.ptr + 2 * off
        self.base = 2 * self.band.front + off                   # int16 index of row 0 in host()

    def host(self):
        return np.array(self.band.host()).view(np.int16)

    def put(self, rows):
        """rows: B arrays of int16, written at the start of each row (the rest keeps the sentinel)"""
        import torch
        h = self.host()
        for b, r in enumerate(rows):
            h[self.base + b * self.stride:self.base + b * self.stride + len(r)] = r
        self.band.words.copy_(torch.from_numpy(h.view(np.int32)))
        return h

    def expect(self, rows):
        e = np.tile(SENT16, self.band.n_words)
        for b, r in enumerate(rows):
            e[self.base + b * self.stride:self.base + b * self.stride + len(r)] = r
        return e


# ---- 1. every int16 value in ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_int16_value_in_both_modes(engines, torch_dev):
    eng = engines(1)
    s = np.arange(-32768, 32768, dtype=np.int16)
    z = eng.wire_in(dev(s[None], torch_dev))
    assert np.array_equal(u32(z)[0], wr.int16_to_c64(s).view(np.uint32))                 # as bit patterns: a -0.0 anywhere, Q of real mode included, would show
    assert not u32(z)[0][1::2].any()
    pairs = np.stack([s, s[::-1]], axis=1)                                               # every value as I and as Q
    z = eng.wire_in(dev(pairs[None], torch_dev), iq=True)
    assert np.array_equal(u32(z)[0], wr.int16_to_c64(pairs, iq=True).view(np.uint32))
    z = eng.wire_in(dev(pairs[None], torch_dev), iq=True, gain=1.0 / 8192)
    assert np.array_equal(u32(z)[0], wr.int16_to_c64(pairs, iq=True, gain=1.0 / 8192).view(np.uint32))


# ---- 2. conversion out and the meters ---------------------------------------------------------------------------------------------------------------------------------
def check_out(eng, x, scale, real, torch_dev):
    import torch
    ref, m = wr.c64_to_int16(x, scale, real)
    xd = dev(x[None], torch_dev)
    n = np.array([len(x)], np.int32)
    raws, outs = [], []
    for _ in range(2):                                           # the C ABI itself, twice: the raw meters [B][4] = peak, sum of squares, clipped, NaN
        o = torch.zeros(ref.shape, dtype=torch.int16, device=torch_dev)
        raw = np.zeros((1, 4), np.float64)
        assert eng.lib.rade_batch_wire_out(eng.h, xd.data_ptr(), len(x), n.ctypes.data, REAL if real else IQ, scale, o.data_ptr(), ref.size, raw.ctypes.data, stream_ptr()) == 0
        raws.append(raw); outs.append(o.cpu().numpy())
    assert np.array_equal(outs[0], ref) and np.array_equal(outs[1], ref)
    assert raws[0].tobytes() == raws[1].tobytes()                # two identical calls: identical bits
    peak, sum2, clipped, nan = raws[0][0]
    assert clipped == m["clipped"] and nan == m["nan"] and peak == m["peak"]
    # sum of squares: every square is exact in float64 (24 x 24 bits), so the device's error is that of its additions.  N non-negative terms take N - 1 additions in any
    # order (adding the 0.0 a thread or a chunk starts from is exact), each off by at most u = 2^-53 of a partial sum that is at most the total:
    # |error| <= (N - 1) u S / (1 - (N - 1) u).  The reference (math.fsum) is the exact sum rounded once: u S more.
    N, u = m["components"] - m["nan"], 2.0 ** -53
    if np.isfinite(m["sum2"]):
        print(f"scale {scale} real {real}: sum2 {sum2!r} reference {m['sum2']!r} |difference| {abs(sum2 - m['sum2'])!r} bound {N * u * m['sum2'] / (1 - N * u)!r}")
        assert abs(sum2 - m["sum2"]) <= N * u * m["sum2"] / (1 - N * u)
    else:
        assert sum2 == m["sum2"]
    # the Python record says the same, and the call without meters writes the same samples
    out, got = eng.wire_out(xd, scale=scale, real=real, meters=True)
    assert np.array_equal(out.cpu().numpy()[0], ref) and np.array_equal(eng.wire_out(xd, scale=scale, real=real).cpu().numpy()[0], ref)
    assert got.peak[0] == peak and got.clipped[0] == clipped and got.nan[0] == nan and got.rms[0] == np.sqrt(sum2 / max(N, 1))


@pytest.mark.parametrize("real", [True, False])
def test_conversion_out_hand_made_vector(engines, torch_dev, real):
    x = (wr.HAND.astype(np.complex64) + 1j * np.float32(7.0)).astype(np.complex64)
    ref, _ = wr.c64_to_int16(x, 1.0, real)
    assert np.array_equal(ref if real else ref[:, 0], wr.HAND_I16)
    check_out(engines(1), x, 1.0, real, torch_dev)
    check_out(engines(1), np.array([1e-40, -1e-40, 2e-38, -2e-38], np.float32).astype(np.complex64), 32767.0, real, torch_dev)     # subnormal inputs
    check_out(engines(1), np.array([1e-36, -1e-36, 0.0, -0.0], np.float32).astype(np.complex64), 1e-3, real, torch_dev)           # a subnormal product


@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("scale", [32767.0, 8192.0, 1.0])
def test_conversion_out_random(engines, torch_dev, scale, real):
    rng = np.random.default_rng(int(scale) + real)
    v = rng.uniform(0.0, 40000.0, (1 << 16, 2)) * rng.choice([-1.0, 1.0], (1 << 16, 2))
    x = (v / scale).astype(np.float32).view(np.complex64).ravel()
    ref, m = wr.c64_to_int16(x, scale, real)
    assert m["clipped"] > 1000 and np.abs(ref.astype(np.int32)).max() == 32768 and (np.abs(ref.astype(np.int32)) < 100).any()      # both sides of the limit are in the draw
    check_out(engines(1), x, scale, real, torch_dev)


# ---- 3. heads and tails -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_off", [0, 1])
@pytest.mark.parametrize("i_off", range(8))
@pytest.mark.parametrize("mode", [REAL, IQ])
def test_heads_and_tails_in_sentinel_buffers(engines, torch_dev, mode, i_off, c_off):
    """B = 5 streams of 0, 1, 7, 8 and 1031 samples, odd strides, the int16 base 0..7 elements and the complex64 base 0..1 elements behind a 16-byte boundary: with the
    strides odd every stream meets another pair of alignments, so each call runs rows with and without a head, with 16-, 8- and (IQ) 4-byte words on the float side.
    In both directions nothing but [b stride, b stride + n[b]) of the output changes and the inputs keep every bit."""
    eng = engines(5)
    B, k = 5, 1 + mode
    i_stride, c_stride = k * 1031 + 3 + (k * 1031) % 2, 1033                              # both odd
    rng = np.random.default_rng(100 * mode + 10 * i_off + c_off)
    s = [rng.integers(-32768, 32768, k * n).astype(np.int16) for n in COUNTS]
    # in
    src = Band16(B, i_stride, i_off, torch_dev)
    before = src.put(s)
    dst = Band(B, 1031, c_stride, 8, device=torch_dev, base_offset_bytes=8 * c_off)
    r = eng.lib.rade_batch_wire_in(eng.h, src.ptr, i_stride, COUNTS.ctypes.data, mode, 1.0, dst.ptr, c_stride, stream_ptr())
    assert r == 0
    dst.check(written=COUNTS, what="wire_in out")
    rows = dst.rows(np.uint32)
    for b, n in enumerate(COUNTS):
        ref = wr.int16_to_c64(s[b].reshape(-1, 2) if mode else s[b], iq=bool(mode))
        assert np.array_equal(rows[b, :2 * n], ref.view(np.uint32)), (b, n)
    assert np.array_equal(src.host(), before)
    # out: a signal around the limit, so that the words carry saturated and plain values
    x = [((rng.uniform(-36000, 36000, (n, 2))).astype(np.float32) / np.float32(8192.0)).view(np.complex64).ravel() for n in COUNTS]
    xin = Band(B, 1031, c_stride, 8, device=torch_dev, base_offset_bytes=8 * c_off)
    full = np.zeros((B, 1031), np.complex64)
    for b, n in enumerate(COUNTS):
        full[b, :n] = x[b]
        full[b, n:] = 9e9                                                                 # readable, and never to be read: it would clip
    xin.fill(full)
    x_before = np.array(xin.host())
    out = Band16(B, i_stride, i_off, torch_dev)
    meters = np.zeros((B, 4), np.float64)
    r = eng.lib.rade_batch_wire_out(eng.h, xin.ptr, c_stride, COUNTS.ctypes.data, mode, 8192.0, out.ptr, i_stride, meters.ctypes.data, stream_ptr())
    assert r == 0
    refs = [wr.c64_to_int16(x[b], 8192.0, real=not mode) for b in range(B)]
    assert np.array_equal(out.host(), out.expect([ref.ravel() for ref, _ in refs]))
    assert np.array_equal(xin.host(), x_before)
    for b, (_, m) in enumerate(refs):
        assert meters[b, 0] == m["peak"] and meters[b, 2] == m["clipped"] and meters[b, 3] == 0, (b, meters[b], m)
        assert abs(meters[b, 1] - m["sum2"]) <= m["components"] * 2.0 ** -53 * m["sum2"] * 1.001
    out2 = Band16(B, i_stride, i_off, torch_dev)                                          # without meters: the other kernel instance
    assert eng.lib.rade_batch_wire_out(eng.h, xin.ptr, c_stride, COUNTS.ctypes.data, mode, 8192.0, out2.ptr, i_stride, None, stream_ptr()) == 0
    assert np.array_equal(out2.host(), out.host())


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(engines, torch_dev):
    eng = engines(5)
    B, L = 5, eng.lib
    n = np.full(B, 64, np.int32)
    i16 = Band(B, 64, 65, 4, device=torch_dev)                   # rows of 128 int16: enough for IQ
    c64 = Band(B, 64, 65, 8, device=torch_dev)
    meters = np.full((B, 4), -1.0)
    neg = n.copy(); neg[3] = -1
    nan, inf = float("nan"), float("inf")

    def w_in(i=None, istr=130, cnt=n, mode=REAL, gain=1.0, o=None, ostr=65):
        return L.rade_batch_wire_in(eng.h, i16.ptr if i is None else i, istr, cnt.ctypes.data if cnt is not None else None, mode, gain, c64.ptr if o is None else o, ostr, stream_ptr())

    def w_out(x=None, xstr=65, cnt=n, mode=REAL, scale=1.0, o=None, ostr=130, m=meters):
        return L.rade_batch_wire_out(eng.h, c64.ptr if x is None else x, xstr, cnt.ctypes.data if cnt is not None else None, mode, scale, i16.ptr if o is None else o, ostr,
                                     m.ctypes.data if m is not None else None, stream_ptr())
    for call, i_name, c_name, i_short, c_short in ((w_in, "i", "o", "istr", "ostr"), (w_out, "o", "x", "ostr", "xstr")):
        k_name = "gain" if call is w_in else "scale"
        bad = [{i_name: 0}, {c_name: 0}, {i_name: i16.ptr + 1}, {c_name: c64.ptr + 4}, {c_name: c64.ptr + 2}, {"cnt": None}, {"cnt": neg},
               {i_short: 63}, {i_short: 127, "mode": IQ}, {c_short: 63}, {c_short: 63, "mode": IQ}, {"mode": 2}, {"mode": -1},
               {k_name: nan}, {k_name: inf}, {k_name: -inf}]
        for kw in bad:
            assert call(**kw) == -1, (call.__name__, kw)
        assert L.rade_batch_wire_in(None, i16.ptr, 130, n.ctypes.data, REAL, 1.0, c64.ptr, 65, stream_ptr()) == -1
    import torch
    torch.cuda.synchronize()
    i16.untouched("int16 buffer of refused calls")
    c64.untouched("complex64 buffer of refused calls")
    assert np.all(meters == -1.0)
    assert w_in(mode=IQ) == 0 and w_out(mode=IQ, m=None) == 0    # the same buffers, strides and counts are accepted when nothing is wrong


# ---- 5. through the receiver ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["slipdrops", "dfs8001"])
def test_receiver_fed_through_wire_in_equals_receiver_fed_by_the_host_converter(engines, torch_dev, golden, name):
    """The first 40 000 samples of the two streaming fixtures that carry int16 (one real channel; I and Q): stream 0 converted by wire_in on the device, stream 1 by
    radae_amd/wire.py on the host, both through one rade_batch_rx call.  Device against host at the same commit: the new path is a drop-in.  (That the receiver is
    right is what the trace tests of test_hip_parity.py show.)"""
    import torch
    from radae_amd import wire
    s = np.ascontiguousarray(golden("rxtrace_" + name)["rx_i16"][:40000])
    iq = s.ndim == 2
    assert iq == (name == "dfs8001")
    eng = engines(2, rx_trace_calls=64)
    eng.reset()
    host = np.frombuffer(wire.int16_to_f32(s.tobytes(), zeropad=not iq), np.complex64)
    assert host.size == 40000
    z = eng.wire_in(dev(np.stack([s, s]), torch_dev), iq=iq)
    assert np.array_equal(u32(z)[0], host.view(np.uint32))
    x = torch.stack([z[0], dev(host, torch_dev)])
    feats, st, eoo = eng.rx(x)
    t0, t1 = eng.rx_trace(0), eng.rx_trace(1)
    assert st[0].n_calls == st[1].n_calls >= 35 and st[0].n_valid == st[1].n_valid
    for f in ("consumed", "n_calls", "n_valid", "has_eoo", "nin", "sync", "snr_dB", "state"):
        assert getattr(st[0], f) == getattr(st[1], f), f
    assert set(t0) == set(t1)
    for k in t0:
        a, b = np.ascontiguousarray(t0[k]), np.ascontiguousarray(t1[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert np.array_equal(u32(feats)[0], u32(feats)[1])


# ---- 6. the transmitter -----------------------------------------------------------------------------------------------------------------------------------------------
def test_transmitter_through_wire_out_equals_the_host_converter(engines, torch_dev, golden):
    from radae_amd import wire
    from radae_amd.engine import BatchEngine
    feats = golden("enc_tx")["features"].astype(np.float32)
    eng = BatchEngine(2, max_tx_mf=10)
    iq = eng.tx(dev(feats, torch_dev))
    out, m = eng.wire_out(iq, scale=8192.0, real=True, meters=True)
    h = iq.cpu().numpy()
    for b in range(2):
        assert out[b].cpu().numpy().tobytes() == wire.f32_to_int16(np.ascontiguousarray(h[b]).tobytes(), 8192.0, real=True)
        assert m.clipped[b] == 0 and m.nan[b] == 0
        v = h[b].real.astype(np.float32) * np.float32(8192.0)
        assert m.peak[b] == np.abs(v).max() and abs(m.rms[b] - np.sqrt(np.mean(v.astype(np.float64) ** 2))) < 1e-9 * m.rms[b]
    eng.close()


# ---- 7. the command lines ---------------------------------------------------------------------------------------------------------------------------------------------
def test_command_lines_speak_int16(golden, tmp_path):
    """`rxe --int16` takes the bytes of the ctest radae_rx_slip_plus_drops file as they are (no `int16tof32.py --zeropad` in front) and ends in sync like the pipe
    of test_hip_parity.py; `txe --int16_real 8192` writes what `txe | f32toint16.py --real --scale 8192` writes and reports the level on stderr."""
    from radae_amd import wire
    env = dict(os.environ); env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")

    def run(args, data):
        r = subprocess.run([sys.executable, "-m", "radae_amd.cli"] + args, input=data, capture_output=True, cwd=str(tmp_path), env=env, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        return r.stdout, r.stderr.decode()
    _, err = run(["rxe", "--int16", "-v", "1", "--no_stdout"], golden("rxtrace_slipdrops")["rx_i16"].tobytes())
    assert err.strip().splitlines()[-1] == "state: sync"
    feats = golden("enc_tx")["features"][0].astype(np.float32)
    i16, err = run(["txe", "--int16_real", "8192"], feats.tobytes())
    iq, _ = run(["txe"], feats.tobytes())
    assert len(i16) == 2 * (10 * 960 + 1152) and i16 == wire.f32_to_int16(iq, 8192.0, real=True)
    last = err.strip().splitlines()[-1].split()
    assert last[0::2] == ["peak:", "rms:", "clipped:"] and last[5] == "0"
    v = np.frombuffer(iq, np.complex64).real * np.float32(8192.0)
    assert abs(float(last[1]) - np.abs(v).max()) <= 0.051 and abs(float(last[3]) - np.sqrt(np.mean(v.astype(np.float64) ** 2))) <= 0.051       # printed to one decimal
