"""GPU tests (-m gpu) of the fractional resampler (rade_batch_resample, rade_clk.hip; include/rade_batch.h states the arithmetic): bit-exact delays, the float32 kernel
against the float64 restatement of tests/resample_ref.py on the library's own table under a bound counted from the roundings, tile and input edges in sentinel
buffers (tests/bands.py), pieces against the whole, per-stream values against the scalar call, the linear mode against the reference's recording
(tests/golden/clock_offset.npz), host-side refusals, and the receiver's slip path end to end on samples resampled on the device."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as rr
from bands import Band
from gpu_kit import INT_KEYS, bits, crandn, define, dev, engines, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
MODES = {"sinc32": rr.SINC32, "linear": rr.LINEAR}
TILE = define("RD_CLK_TILE")


@pytest.fixture(scope="module")
def taps():
    from radae_amd.engine import resample_taps
    return resample_taps()


def raw_call(eng, x_ptr, x_stride, n_in, y_ptr, y_stride, n_out, mode, ppm=0.0, ppm_b=None, t0=None, n0=None, in_base=None):
    """rade_batch_resample through the C ABI with caller-owned pointers; returns its return value"""
    from radae_amd.engine import ResampleParams, _stream_ptr
    B = eng.B
    keep = [np.ascontiguousarray(np.broadcast_to(np.asarray(n_in, np.int32), (B,))), np.ascontiguousarray(np.broadcast_to(np.asarray(n_out, np.int32), (B,)))]
    ptr = lambda v, dt: (keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (B,)))) or keep[-1].ctypes.data) if v is not None else None
    p = ResampleParams(mode, ppm, ptr(ppm_b, np.float64), ptr(t0, np.float64), ptr(n0, np.int64), ptr(in_base, np.int64))
    return eng.lib.rade_batch_resample(eng.h, C.c_void_p(x_ptr), x_stride, keep[0].ctypes.data, C.c_void_p(y_ptr), y_stride, keep[1].ctypes.data, C.byref(p), _stream_ptr())


def check_against_restatement(y, x, n_out, ppm, t0, mode, T, what, n0=0, in_base=0):
    """per real component |y - y64| <= K 2^-24 x (the sum of |coefficient| |operand| of the output), K from the roundings (tests/resample_ref.py)"""
    y64, mag = rr.resample(x, n_out, ppm, t0, mode, n0, in_base, T)
    err = np.stack([np.abs(y.real - y64.real), np.abs(y.imag - y64.imag)], axis=-1)
    tol = rr.KERNEL_ROUNDINGS[mode] * rr.EPS * mag
    worst = float((err / np.maximum(tol, 1e-300)).max()) if n_out else 0.0
    print(f"{what}: {n_out} outputs, max |dy| {err.max() if n_out else 0.0:.3g}, largest error / bound {worst:.3g}")
    assert np.all(err <= tol), what


# ---- 1. bit-exact delays ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sinc32", "linear"])
def test_integer_delays_are_bit_exact(engines, torch_dev, mode):
    """ppm = 0: t0 = 0 gives y == x, t0 = 7 an advance and t0 = -3 a delay with zeros where the input ends; outputs in NaN-sentinel buffers at odd strides, guards
    untouched, the input unchanged"""
    import torch
    B, N = 3, 1500
    eng = engines(B)
    x = crandn(np.random.default_rng(11), B, N)
    xin = Band(B, N, N + 7, 8, torch_dev, base_offset_bytes=8).fill(x)
    snap = xin.host().copy()
    for t0 in (0, 7, -3):
        out = Band(B, N, N + 3, 8, torch_dev, base_offset_bytes=8)
        assert raw_call(eng, xin.ptr, N + 7, N, out.ptr, N + 3, N, MODES[mode], t0=float(t0)) == 0
        torch.cuda.synchronize()
        out.check(what=f"y, t0 {t0}")
        want = np.zeros_like(x)
        if t0 >= 0:
            want[:, :N - t0] = x[:, t0:]
        else:
            want[:, -t0:] = x[:, :N + t0]
        assert np.array_equal(out.rows(), bits(want)), t0
    assert np.array_equal(xin.host(), snap), "the input was written"


# ---- 2. / 5. random operands against the restatement; per-stream values against the scalar calls ------------------------------------------------------------
MIX_PPM, MIX_T0 = (-2493.77, 625.0, 0.0), (0.37, -2.625, 11.5)


@pytest.fixture(scope="module")
def mixed(engines, torch_dev):
    """B = 3 with three clock offsets and three fractional starts in ONE call per mode, n_in = 1500: {mode: (y, n_out)} and the input"""
    x = crandn(np.random.default_rng(12), 3, 1500)
    xt = dev(x, torch_dev)
    res = {}
    for mode in MODES:
        y, n_out = engines(3).resample(xt, MIX_PPM, MIX_T0, mode)
        res[mode] = (y.cpu().numpy(), n_out)
    return x, xt, res


@pytest.mark.parametrize("mode", ["sinc32", "linear"])
def test_random_operands_against_the_restatement(mixed, taps, mode):
    x, _, res = mixed
    y, n_out = res[mode]
    for b in range(3):
        assert n_out[b] == rr.count(1500, MIX_T0[b], MIX_PPM[b]) and n_out[b] > 1400
        check_against_restatement(y[b, :n_out[b]], x[b], int(n_out[b]), MIX_PPM[b], MIX_T0[b], MODES[mode], taps, f"{mode} stream {b} ppm {MIX_PPM[b]}")
        assert np.all(y[b, n_out[b]:] == 0)


@pytest.mark.parametrize("mode", ["sinc32", "linear"])
def test_per_stream_values_equal_the_scalar_call(engines, mixed, mode):
    """the rule of rade_channel_streams: stream b of the mixed call is what the call with its ppm and t0 as scalars gives for it, bit for bit"""
    _, xt, res = mixed
    y, n_out = res[mode]
    for b in range(3):
        ys, ns = engines(3).resample(xt, MIX_PPM[b], MIX_T0[b], mode)
        assert ns[b] == n_out[b]
        assert np.array_equal(bits(ys.cpu().numpy()[b, :ns[b]]), bits(y[b, :n_out[b]])), b


# ---- 3. tile and input edges ---------------------------------------------------------------------------------------------------------------------------------
EDGE_N = sorted({1, 2, 255, 256, 257, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1})


@pytest.mark.parametrize("n_out", EDGE_N)
def test_tile_and_input_edges(engines, torch_dev, taps, n_out):
    """n_out around the kernel's tile (and 1, 2, 255..257); stream 0 with all the input its windows need, stream 1 at the largest step (+50 000 ppm: the widest window a
    tile can have) with an input that ends inside its last windows, stream 2 with n_in = 1.  The rows hold samples behind n_in: they must read as zeros.  Each stream
    against the restatement with zero extension, both modes; no byte written outside [b stride, b stride + n_out)."""
    import torch
    B = 3
    eng = engines(B)
    ppm, t0 = (-2493.77, 50000.0, 625.0), (3.25, -4.5, -6.75)
    row = int(n_out * 1.05) + 40
    x = crandn(np.random.default_rng(100 + n_out), B, row)
    last1 = rr.positions(n_out - 1, 1, t0[1], ppm[1])[0][0]               # centre sample of stream 1's last output
    n_in = np.array([row, max(int(last1) - 5, 1), 1], np.int32)
    xin = Band(B, row, row + 1 + (row % 2), 8, torch_dev, base_offset_bytes=8).fill(x)      # odd strides
    for mode in MODES:
        out = Band(B, n_out, n_out + 1 + (n_out % 2), 8, torch_dev, base_offset_bytes=8)
        assert raw_call(eng, xin.ptr, xin.stride, n_in, out.ptr, out.stride, n_out, MODES[mode], ppm_b=ppm, t0=t0) == 0
        torch.cuda.synchronize()
        out.check(what=f"y, n_out {n_out}, {mode}")
        y = out.rows(np.complex64)
        for b in range(B):
            check_against_restatement(y[b], x[b, :n_in[b]], n_out, ppm[b], t0[b], MODES[mode], taps, f"{mode} n_out {n_out} stream {b} n_in {n_in[b]}")


def test_a_workgroup_walks_several_tiles(engines, torch_dev, taps):
    """B = 64 gives 32 workgroups per stream, so a stream of more than 32 tiles makes each workgroup take a second tile (the window buffer is refilled): one long
    stream beside 63 short ones, against the restatement, and the short ones written for their n_out only"""
    B = 64
    n_long = 33 * TILE + 5
    ppm, t0 = 1234.5, 0.625
    n_in = int(n_long * 1.002) + 40
    x = crandn(np.random.default_rng(13), n_in)
    xt = dev(np.broadcast_to(x, (B, n_in)), torch_dev)
    n_out = np.full(B, 10, np.int32); n_out[5] = n_long
    y, _ = engines(B).resample(xt, ppm, t0, "sinc32", n_out=n_out)
    y = y.cpu().numpy()
    check_against_restatement(y[5], x, n_long, ppm, t0, rr.SINC32, taps, "the long stream")
    assert np.array_equal(bits(y[:, :10]), bits(np.broadcast_to(y[5, :10], (B, 10)))) and np.all(np.delete(y, 5, axis=0)[:, 10:] == 0)


# ---- 4. pieces equal the whole ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sinc32", "linear"])
def test_pieces_equal_the_whole(engines, torch_dev, mode):
    """2048 outputs at -2493.77 ppm as calls of 700, 1 and 1347 outputs through n0 / in_base, each handed only the input samples its windows cover"""
    eng = engines(1)
    ppm, t0, N = -2493.77, 0.37, 2100
    x = crandn(np.random.default_rng(14), 1, N)
    whole, _ = eng.resample(dev(x, torch_dev), ppm, t0, mode, n_out=2048)
    whole = whole.cpu().numpy()[0]
    parts, n0 = [], 0
    for k in (700, 1, 1347):
        i, _ = rr.positions(n0, k, t0, ppm)
        lo, hi = max(int(i[0]) - 15, 0), min(int(i[-1]) + 16, N - 1)
        y, _ = eng.resample(dev(x[:, lo:hi + 1], torch_dev), ppm, t0, mode, n_out=k, n0=n0, in_base=lo)
        parts.append(y.cpu().numpy()[0, :k])
        n0 += k
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))


@pytest.mark.parametrize("mode", ["sinc32", "linear"])
def test_clock_offset_helper_equals_the_whole(engines, torch_dev, mode):
    """ClockOffset fed 960, 800 and 1120 input samples, then flush(): the concatenated outputs are the whole-stream call's, bit for bit, for two streams with their own ppm"""
    from radae_amd.engine import ClockOffset
    eng = engines(2)
    ppm, t0 = (-2493.77, 1800.0), (0.37, -1.5)
    x = crandn(np.random.default_rng(15), 2, 2880)
    whole, n_whole = eng.resample(dev(x, torch_dev), ppm, t0, mode)
    whole = whole.cpu().numpy()
    co = ClockOffset(eng, ppm, t0, mode)
    got, pos = [[], []], 0
    for k in (960, 800, 1120):
        y, n = co.feed(dev(x[:, pos:pos + k], torch_dev))
        pos += k
        y = y.cpu().numpy()
        for b in range(2):
            got[b].append(y[b, :n[b]])
            assert n[b] > 0
    y, n = co.flush()
    y = y.cpu().numpy()
    for b in range(2):
        assert 0 < n[b] <= 17
        full = np.concatenate(got[b] + [y[b, :n[b]]])
        assert len(full) == n_whole[b] == rr.count(2880, t0[b], ppm[b])
        assert np.array_equal(bits(full), bits(whole[b, :n_whole[b]])), b


# ---- 6. the linear mode against the reference's recording -----------------------------------------------------------------------------------------------------
def test_linear_mode_against_the_reference_recording(engines, torch_dev, golden):
    """dsp.py:sample_clock_offset's outputs for ppm = +100, -625 and the 8020 Hz receiver's, three streams of one call, under the bound of the host test"""
    g = golden("clock_offset")
    x = g["x"]
    y, n = engines(3).resample(dev(np.broadcast_to(x, (3, len(x))), torch_dev), g["ppm"], 0.0, "linear", n_out=g["n"].astype(np.int32))
    y = y.cpu().numpy()
    for k in range(3):
        nk = int(g["n"][k])
        err = float(np.abs(y[k, :nk] - g["y"][k, :nk]).max())
        tol = rr.reference_bound(nk, x)
        print(f"ppm {g['ppm'][k]:+.2f}: {nk} outputs, max |dy| {err:.3g}, bound {tol:.3g}")
        assert err <= tol


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engines, torch_dev):
    """argument checking on the host: each of these returns -1 before any launch, and the output buffer still holds its sentinel"""
    import torch
    B, N = 3, 300
    eng = engines(B)
    xin = Band(B, N, N + 1, 8, torch_dev).fill(crandn(np.random.default_rng(16), B, N))
    out = Band(B, N, N + 1, 8, torch_dev)
    ok = dict(x_ptr=xin.ptr, x_stride=N + 1, n_in=N, y_ptr=out.ptr, y_stride=N + 1, n_out=N, mode=rr.SINC32)
    bad = [dict(x_ptr=xin.ptr + 4), dict(y_ptr=out.ptr + 4), dict(x_ptr=0), dict(y_ptr=0), dict(x_stride=N - 1), dict(y_stride=N - 1), dict(mode=2), dict(mode=-1),
           dict(ppm=60000.0), dict(ppm=-60000.0), dict(ppm_b=(0.0, 0.0, 60000.0)), dict(ppm=float("nan")), dict(n_out=(N, -1, N)), dict(n_in=(N, N, -1)),
           dict(n0=(0, -1, 0)), dict(n0=1 << 30, ppm=100.0), dict(t0=float("inf"))]
    for kw in bad:
        assert raw_call(eng, **{**ok, **kw}) == -1, kw
    torch.cuda.synchronize()
    out.untouched("y of the refused calls")
    assert raw_call(eng, **ok) == 0                                   # ... and the same arguments without the fault are accepted
    torch.cuda.synchronize()
    out.check(what="y")
    with pytest.raises(ValueError):                                   # the binding: the default n_out comes from rade_resample_count, which refuses the same ppm
        eng.resample(dev(np.zeros((B, 8), np.complex64), torch_dev), 60000.0)
    with pytest.raises(RuntimeError):
        eng.resample(dev(np.zeros((B, 8), np.complex64), torch_dev), 60000.0, n_out=4)


# ---- 8. end to end: the receiver's slip path from a generated input -------------------------------------------------------------------------------------------
def test_receiver_slip_path_on_device_resampled_samples(torch_dev, oracle, oracle_model):
    """Oracle transmitter and channel (30 modem frames, 10 dB AWGN, about 1 s of leading noise), resampled on the device as an 8020 Hz sound card hears it, copied back;
    the device receiver and the oracle receiver on those same samples: the eleven discrete outputs equal per call, fmax bit-equal, features < 1e-4 RMS.  The stretched
    frames push tmax up by 2.4 samples per modem frame; the leading noise (8150 samples) puts it about 35 samples below 800 at sync, so the oracle must make a
    1120-sample call while in sync about 14 frames later -- asserted on the oracle's own trace, as is that it ends in sync."""
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import BatchEngine, ppm_from_rates, sigma_from_EbNodB
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
    ppm = ppm_from_rates(8000, 8020)
    y, n_out = eng.resample(dev(full[None], torch_dev), ppm)
    assert n_out[0] == rr.count(n_tot, 0.0, ppm) > n_tot
    rx = y[:, :n_out[0]].contiguous()
    samples = rx.cpu().numpy()[0]
    d = oracle.run_rx_stream(oracle_model, samples)
    slips = [i for i in range(len(d["nin_after"])) if d["nin_after"][i] == 1120 and d["state_before"][i] == 2]
    print(f"oracle: {len(d['nin_after'])} calls, 1120-sample calls asked for in sync at {slips}, tmax {d['tmax'].tolist()}")
    assert slips and d["state_after"][-1] == 2 and len(d["features_out"]) >= 20
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
