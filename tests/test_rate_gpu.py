"""GPU tests (-m gpu) of the rational rate converter (rade_batch_rate_convert, rade_rate.hip; include/rade_batch.h states the arithmetic): bit-exact identities, the
float32 kernel against the float64 restatement of tests/rate_ref.py on the library's own table under the bound counted from the roundings, tile and input edges in
sentinel buffers (tests/bands.py), pieces against the whole, the fused int16 formats against wire_in + the complex64 call, host-side refusals, a change of ratio
between calls, and the receiver end to end on samples that went up to 48 kHz int16 and back on the device."""
import ctypes as C

import numpy as np
import pytest

import rate_ref as rf
from bands import Band
from gpu_kit import INT_KEYS, bits, crandn, define, dev, engines, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
WIN, TILE_MAX = define("RD_RATE_WIN"), define("RD_RATE_TILE_MAX")


def tile_of(L, M):
    """rd_rate_tile of rade_dev.h: the outputs of a tile, from the window's fixed capacity"""
    L, M, K, T = rf.reduce(L, M)
    return min((WIN - T - K) * L // M + 1, TILE_MAX) // 64 * 64


@pytest.fixture(scope="module")
def taps():
    from radae_amd.engine import rate_taps
    made = {}

    def get(L, M):
        if (L, M) not in made:
            made[(L, M)] = rate_taps(L, M)
        return made[(L, M)]
    return get


def irand(rng, *shape):
    """int16 samples over the whole range, the three extreme values among them"""
    v = rng.integers(-32768, 32768, shape).astype(np.int16)
    flat = v.reshape(-1)
    flat[:3] = (32767, -32767, -32768)
    flat[-3:] = (-32768, 32767, -32767)
    return v


def raw_call(eng, x_ptr, x_stride, n_in, y_ptr, y_stride, n_out, L, M, fmt=rf.C64, gain=1.0, n0=None, in_base=None):
    """rade_batch_rate_convert through the C ABI with caller-owned pointers; returns its return value"""
    from radae_amd.engine import RateParams, _stream_ptr
    B = eng.B
    keep = [np.ascontiguousarray(np.broadcast_to(np.asarray(n_in, np.int32), (B,))), np.ascontiguousarray(np.broadcast_to(np.asarray(n_out, np.int32), (B,)))]
    ptr = lambda v, dt: (keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (B,)))) or keep[-1].ctypes.data) if v is not None else None
    p = RateParams(L, M, ptr(n0, np.int64), ptr(in_base, np.int64))
    return eng.lib.rade_batch_rate_convert(eng.h, C.c_void_p(x_ptr), x_stride, keep[0].ctypes.data, fmt, gain, C.c_void_p(y_ptr), y_stride, keep[1].ctypes.data,
                                           C.byref(p), _stream_ptr())


def check_against_restatement(y, x, n_out, L, M, Ct, what, n0=0, in_base=0, fmt=rf.C64, gain=1.0):
    """per real component |y - y64| <= (T + 1) 2^-24 x (the sum of |coefficient| |operand| of the output) (tests/rate_ref.py)"""
    y64, mag = rf.convert(x, n_out, L, M, n0, in_base, Ct, fmt, gain)
    err = np.stack([np.abs(y.real - y64.real), np.abs(y.imag - y64.imag)], axis=-1)
    tol = rf.kernel_bound(L, M, mag)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if n_out else 0.0
    print(f"{what}: {n_out} outputs, max |dy| {err.max() if n_out else 0.0:.3g}, largest error / bound {worst:.3g}")
    assert np.all(err <= tol), what


# ---- 1. bit-exact identities ---------------------------------------------------------------------------------------------------------------------------------
def test_unit_ratio_copies_and_upsampling_keeps_the_samples(engines, torch_dev):
    """L = M = 1: y == x bit for bit; 6 / 1: y[6 k] == x[k] bit for bit (random non-zero input, B = 3, 300 samples); outputs in NaN-sentinel buffers at odd
    strides and offset bases, guards untouched, the input unchanged"""
    import torch
    B, N = 3, 300
    eng = engines(B)
    x = crandn(np.random.default_rng(21), B, N)
    assert np.all(x.real != 0) and np.all(x.imag != 0)
    xin = Band(B, N, N + 7, 8, torch_dev, base_offset_bytes=8).fill(x)
    snap = xin.host().copy()
    out = Band(B, N, N + 3, 8, torch_dev, base_offset_bytes=8)
    assert raw_call(eng, xin.ptr, N + 7, N, out.ptr, N + 3, N, 1, 1) == 0
    torch.cuda.synchronize()
    out.check(what="y, 1/1")
    assert np.array_equal(out.rows(), bits(x))
    out = Band(B, 6 * N, 6 * N + 1, 8, torch_dev, base_offset_bytes=8)
    assert raw_call(eng, xin.ptr, N + 7, N, out.ptr, 6 * N + 1, 6 * N, 6, 1) == 0
    torch.cuda.synchronize()
    out.check(what="y, 6/1")
    assert np.array_equal(bits(out.rows(np.complex64)[:, ::6]), bits(x))
    assert np.array_equal(xin.host(), snap), "the input was written"


# ---- 2. random operands against the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M", [(1, 6), (6, 1), (80, 441), (441, 80), (2, 3)])
def test_random_operands_against_the_restatement(engines, torch_dev, taps, L, M):
    B, N = 3, 3000 if (L, M) in ((1, 6), (80, 441)) else 1500
    x = crandn(np.random.default_rng(22), B, N)
    y, n_out = engines(B).rate_convert(dev(x, torch_dev), L, M)
    y = y.cpu().numpy()
    for b in range(B):
        assert n_out[b] == rf.count(N, L, M) > 0
        check_against_restatement(y[b, :n_out[b]], x[b], int(n_out[b]), L, M, taps(L, M), f"{L}/{M} stream {b}")


@pytest.mark.parametrize("fmt", ["c64", "s16_real", "s16_iq"])
def test_input_formats_against_the_restatement(engines, torch_dev, taps, fmt):
    """1 / 6 in all three input formats; the int16 inputs hold +-32767 and -32768, gain 1 / 8192"""
    B, N, L, M = 3, 3000, 1, 6
    rng = np.random.default_rng(23)
    x, f, gain = {"c64": (crandn(rng, B, N), rf.C64, 1.0), "s16_real": (irand(rng, B, N), rf.S16_REAL, 1.0 / 8192), "s16_iq": (irand(rng, B, N, 2), rf.S16_IQ, 1.0 / 8192)}[fmt]
    y, n_out = engines(B).rate_convert(dev(x, torch_dev), L, M, gain=gain)
    y = y.cpu().numpy()
    for b in range(B):
        assert n_out[b] == 500
        check_against_restatement(y[b, :500], x[b], 500, L, M, taps(L, M), f"{fmt} stream {b}", fmt=f, gain=gain)


# ---- 3. tile and input edges ---------------------------------------------------------------------------------------------------------------------------------
EDGES = [(L, M, n) for L, M in ((1, 6), (6, 1)) for n in sorted({1, 2, tile_of(L, M) - 1, tile_of(L, M), tile_of(L, M) + 1})]


@pytest.mark.parametrize("L,M,n_out", EDGES)
def test_tile_and_input_edges(engines, torch_dev, taps, L, M, n_out):
    """n_out around the kernel's tile (and 1, 2); stream 0 with all the input its windows need, stream 1 with an input that ends inside its last windows, stream 2 with
    n_in = 1.  The rows hold samples behind n_in: they must read as zeros.  Each stream against the restatement with zero extension, from n0 = 5 and in_base = -3;
    no byte written outside [b stride, b stride + n_out)."""
    import torch
    B, n0, in_base = 3, 5, -3
    eng = engines(B)
    T = rf.reduce(L, M)[3]
    i, _ = rf.positions(n0, n_out, L, M)
    row = int(i[-1]) - in_base + T                                   # past the last window
    x = crandn(np.random.default_rng(300 + n_out), B, row)
    n_in = np.array([row, max(int(i[-1]) - in_base - 5, 1), 1], np.int32)
    xin = Band(B, row, row + 1 + (row % 2), 8, torch_dev, base_offset_bytes=8).fill(x)      # odd strides
    out = Band(B, n_out, n_out + 1 + (n_out % 2), 8, torch_dev, base_offset_bytes=8)
    assert raw_call(eng, xin.ptr, xin.stride, n_in, out.ptr, out.stride, n_out, L, M, n0=n0, in_base=in_base) == 0
    torch.cuda.synchronize()
    out.check(what=f"y, {L}/{M}, n_out {n_out}")
    y = out.rows(np.complex64)
    for b in range(B):
        check_against_restatement(y[b], x[b, :n_in[b]], n_out, L, M, taps(L, M), f"{L}/{M} n_out {n_out} stream {b} n_in {n_in[b]}", n0=n0, in_base=in_base)


def test_a_workgroup_walks_several_tiles(engines, torch_dev, taps):
    """B = 64 gives 32 workgroups per stream, so a stream of more than 32 tiles makes each workgroup take a second tile (the window buffer is refilled): one long
    stream beside 63 short ones at 1 / 6 from int16, against the restatement, and the short ones written for their n_out only"""
    B, L, M = 64, 1, 6
    n_long = 33 * tile_of(L, M) + 5
    n_in = 6 * n_long + 40
    x = irand(np.random.default_rng(24), n_in)
    xt = dev(np.broadcast_to(x, (B, n_in)), torch_dev)
    n_out = np.full(B, 10, np.int32); n_out[5] = n_long
    y, _ = engines(B).rate_convert(xt, L, M, n_out=n_out, gain=1.0 / 32768)
    y = y.cpu().numpy()
    check_against_restatement(y[5], x, n_long, L, M, taps(L, M), "the long stream", fmt=rf.S16_REAL, gain=1.0 / 32768)
    assert np.array_equal(bits(y[:, :10]), bits(np.broadcast_to(y[5, :10], (B, 10)))) and np.all(np.delete(y, 5, axis=0)[:, 10:] == 0)


# ---- 4. pieces equal the whole ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,M", [(1, 6), (80, 441)])
def test_pieces_equal_the_whole(engines, torch_dev, L, M):
    """2048 outputs as calls of 700, 1 and 1347 outputs through n0 / in_base, each handed only the input samples its windows cover"""
    eng = engines(1)
    T = rf.reduce(L, M)[3]
    N = int(rf.positions(2047, 1, L, M)[0][0]) + 40
    x = crandn(np.random.default_rng(25), 1, N)
    whole, _ = eng.rate_convert(dev(x, torch_dev), L, M, n_out=2048)
    whole = whole.cpu().numpy()[0]
    parts, n0 = [], 0
    for k in (700, 1, 1347):
        i, _ = rf.positions(n0, k, L, M)
        lo, hi = max(int(i[0]) - (T // 2 - 1), 0), min(int(i[-1]) + T // 2, N - 1)
        y, _ = eng.rate_convert(dev(x[:, lo:hi + 1], torch_dev), L, M, n_out=k, n0=n0, in_base=lo)
        parts.append(y.cpu().numpy()[0, :k])
        n0 += k
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))


@pytest.mark.parametrize("L,M,mul", [(1, 6, 6), (80, 441, 1)])
def test_rate_converter_helper_equals_the_whole(engines, torch_dev, L, M, mul):
    """RateConverter fed 960-, 800- and 1120-sample pieces (x 6 for 1 / 6), then flush(): the concatenated outputs are the whole-stream call's, bit for bit, two streams"""
    from radae_amd.engine import RateConverter
    eng = engines(2)
    pieces = [960 * mul, 800 * mul, 1120 * mul]
    N = sum(pieces)
    x = crandn(np.random.default_rng(26), 2, N)
    whole, n_whole = eng.rate_convert(dev(x, torch_dev), L, M)
    whole = whole.cpu().numpy()
    rc = RateConverter(eng, L, M)
    got, pos = [[], []], 0
    for k in pieces:
        y, n = rc.feed(dev(x[:, pos:pos + k], torch_dev))
        pos += k
        y = y.cpu().numpy()
        for b in range(2):
            got[b].append(y[b, :n[b]])
            assert n[b] > 0
    y, n = rc.flush()
    y = y.cpu().numpy()
    for b in range(2):
        assert n[b] > 0
        full = np.concatenate(got[b] + [y[b, :n[b]]])
        assert len(full) == n_whole[b] == rf.count(N, L, M)
        assert np.array_equal(bits(full), bits(whole[b, :n_whole[b]])), b


# ---- 5. fused equals composed ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iq", [False, True])
def test_fused_int16_equals_wire_in_then_c64(engines, torch_dev, iq):
    """the int16 formats against rade_batch_wire_in followed by the complex64 call, bit for bit; the real format's imaginary parts all have the bit pattern of +0.0f"""
    B, N, gain = 3, 3000, 1.0 / 8192
    eng = engines(B)
    x = irand(np.random.default_rng(27), B, N, 2) if iq else irand(np.random.default_rng(27), B, N)
    xt = dev(x, torch_dev)
    for L, M in ((1, 6), (80, 441)):
        fused, n1 = eng.rate_convert(xt, L, M, gain=gain)
        comp, n2 = eng.rate_convert(eng.wire_in(xt, iq=iq, gain=gain), L, M)
        assert np.array_equal(n1, n2) and n1[0] == rf.count(N, L, M)
        fused, comp = fused.cpu().numpy(), comp.cpu().numpy()
        assert np.array_equal(bits(fused), bits(comp)), (L, M)
        if not iq:
            assert np.all(bits(fused)[:, 1::2] == 0) and np.any(fused.real != 0)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engines, torch_dev):
    """argument checking on the host: each of these returns -1 before any launch, and the output buffer still holds its sentinel"""
    import torch
    B, N, NO = 3, 600, 100
    eng = engines(B)
    xin = Band(B, N, N + 1, 8, torch_dev).fill(crandn(np.random.default_rng(28), B, N))
    out = Band(B, NO, NO + 1, 8, torch_dev)
    ok = dict(x_ptr=xin.ptr, x_stride=N + 1, n_in=N, y_ptr=out.ptr, y_stride=NO + 1, n_out=NO, L=1, M=6)
    s16 = dict(fmt=rf.S16_REAL, x_stride=2 * (N + 1))                   # the same bytes read as int16 rows
    bad = [dict(x_ptr=xin.ptr + 4), dict(y_ptr=out.ptr + 4), dict(x_ptr=0), dict(y_ptr=0), dict(x_stride=N - 1), dict(y_stride=NO - 1), dict(fmt=3), dict(fmt=-1),
           dict(s16, x_ptr=xin.ptr + 1), dict(s16, gain=float("inf")), dict(s16, gain=float("nan")), dict(fmt=rf.S16_IQ, x_stride=2 * N - 1),
           dict(fmt=rf.S16_REAL, x_stride=N - 1), dict(L=0), dict(M=0), dict(L=-1), dict(M=-6), dict(L=1, M=9), dict(L=2, M=17), dict(L=513, M=1), dict(L=200, M=441),
           dict(n_out=(NO, -1, NO)), dict(n_in=(N, N, -1)), dict(n0=(0, -1, 0)), dict(n0=(1 << 62) // 6), dict(n0=1 << 62, L=1, M=1)]
    for kw in bad:
        assert raw_call(eng, **{**ok, **kw}) == -1, kw
    torch.cuda.synchronize()
    out.untouched("y of the refused calls")
    for kw in (dict(), s16, dict(s16, x_ptr=xin.ptr + 2), dict(fmt=rf.S16_IQ, x_stride=2 * N), dict(L=1, M=8), dict(L=512, M=1, n_out=NO), dict(n0=(1 << 62) // 6 - NO)):
        assert raw_call(eng, **{**ok, **kw}) == 0, kw                    # ... and the same arguments without the fault are accepted
    torch.cuda.synchronize()
    out.check(what="y")
    with pytest.raises(ValueError):                                      # the binding: the default n_out comes from rade_rate_count, which refuses the same L
        eng.rate_convert(dev(np.zeros((B, 8), np.complex64), torch_dev), 0, 1)
    with pytest.raises(RuntimeError):
        eng.rate_convert(dev(np.zeros((B, 8), np.complex64), torch_dev), 1, 9, n_out=1)


# ---- 7. another ratio between calls ----------------------------------------------------------------------------------------------------------------------------
def test_changing_the_ratio_between_calls(engines, torch_dev, taps):
    """1 / 6, then 80 / 441, then 1 / 6 again on one engine: the table on the device follows the ratio, and the third call gives the first one's bits"""
    B, N = 3, 3000
    eng = engines(B)
    x = crandn(np.random.default_rng(29), B, N)
    xt = dev(x, torch_dev)
    a, na = eng.rate_convert(xt, 1, 6)
    b, nb = eng.rate_convert(xt, 80, 441)
    c, nc = eng.rate_convert(xt, 1, 6)
    a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(na, nc) and np.array_equal(bits(a), bits(c))
    check_against_restatement(a[1, :na[1]], x[1], int(na[1]), 1, 6, taps(1, 6), "1/6 first")
    check_against_restatement(b[1, :nb[1]], x[1], int(nb[1]), 80, 441, taps(80, 441), "80/441 between")


# ---- 8. end to end: 8 kHz -> 48 kHz int16 -> 8 kHz on the device, then the receiver ---------------------------------------------------------------------------
def test_receiver_on_samples_through_a_48_kHz_sound_card(torch_dev, oracle, oracle_model):
    """Oracle transmitter and channel (30 modem frames, 10 dB AWGN, about 1 s of leading noise, 1152 trailing samples); on the device 6 / 1 up, wire_out real at scale
    8192 (what feeds a 48 kHz card), the fused int16 1 / 6 down with gain 1 / 8192, copied back; the device receiver and the oracle receiver on those same samples: the
    eleven discrete outputs equal per call, fmax bit-equal, features < 1e-4 RMS.  Asserted on the oracle's own trace: it ends in sync with at least 20 decoded frames."""
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import BatchEngine, sigma_from_EbNodB
    n_mf, n_pre = 30, 8150
    feats = synth_features(31, n_mf * 12)
    tx = oracle.Tx(oracle_model)
    sig = np.concatenate([tx.frame(feats[12 * k:12 * k + 12].ravel())[0] for k in range(n_mf)])
    n_tot = n_pre + len(sig) + 1152
    noise = crandn(np.random.default_rng(5), n_tot)
    sigma = sigma_from_EbNodB(10.0)
    r, _ = oracle.channel(sig, None, noise[n_pre:n_pre + len(sig)], sigma, 0.0)
    full = np.concatenate([sigma * noise[:n_pre], r, sigma * noise[-1152:]]).astype(np.complex64)
    eng = BatchEngine(1, max_tx_mf=1, rx_trace_calls=64)
    up, n_up = eng.rate_convert(dev(full[None], torch_dev), 6, 1)
    assert n_up[0] == 6 * n_tot
    card, meters = eng.wire_out(up, real=True, scale=8192.0, meters=True)
    assert meters.clipped[0] == 0 and meters.nan[0] == 0
    y, n_out = eng.rate_convert(card, 1, 6, gain=1.0 / 8192)
    assert n_out[0] == n_tot
    rx = y[:, :n_tot].contiguous()
    samples = rx.cpu().numpy()[0]
    assert np.all(bits(samples)[1::2] == 0)
    d = oracle.run_rx_stream(oracle_model, samples)
    print(f"oracle: {len(d['nin_after'])} calls, {len(d['features_out'])} decoded frames, final state {d['state_after'][-1]}")
    assert d["state_after"][-1] == 2 and len(d["features_out"]) >= 20
    fo, st, _ = eng.rx(rx)
    t = eng.rx_trace(0)
    for k in INT_KEYS:
        assert np.array_equal(t[k], d[k]), k
    assert np.array_equal(t["fmax"], d["fmax"])
    nv = st[0].n_valid
    assert nv == len(d["features_out"])
    rms = float(np.sqrt(np.mean((fo.cpu().numpy()[0, :nv] - d["features_out"]) ** 2)))
    print(f"features rms {rms:.3g} over {nv} frames")
    assert rms < 1e-4
    eng.close()
