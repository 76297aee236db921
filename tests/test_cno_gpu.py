"""GPU tests (-m gpu) of the chirp C/No stage (rade_batch_cno_est, rade_cno.hip; include/rade_batch.h states the arithmetic): the golden recordings of the reference's
est_CNo.py, the kernel's band sums against the float64 restatement of tests/cno_ref.py under the bound counted from the roundings, the shapes at which the kernel takes
another path, the buffer contract on sentinel buffers (tests/bands.py), the refusals, and radae_amd.ota.process_rx end to end.

The bound (derived in include/rade_batch.h, restated here).  u = 2^-24.  Every coefficient of the kernel's four stages has modulus 1, so an error made in one stage
reaches the bin unamplified.  A table entry is off by at most u.  A lone product (one rounded multiply, one fused multiply-add per component) is off by at most 4 u of
its operand's modulus.  A sum of m terms is per component a 2 m-term real dot product of fused multiply-adds: off by at most 2 m u sqrt 2 sum |y_i| per component,
4 m u sum |y_i| in modulus.  Along the path of a bin: pre-twiddle (1 + 4), 40-term stage (1 + 160), inter-stage twiddle (1 + 4), 50-term stage (1 + 200), J-term sum
(1 + 4 J): (372 + 4 J) u, times 1.01 for the terms of second order.  So |X^[k] - X[k]| <= 1.01 (372 + 4 J) u sum_n |x_n| <= gamma ||x_w||_2 with
gamma = 1.01 (372 + 4 J) 2^-24 sqrt N (Cauchy-Schwarz), and for a band of nb bins with exact sum S: |dS| <= 2 e sqrt(nb S) + nb e^2, e = gamma ||x_w||_2.  The sums behind
|X|^2 are double and add nothing that counts.  It is a worst-case bound: random rounding errors stay far below it, which WORST_MEASURED records."""
import ctypes as C
import os

import numpy as np
import pytest

import cno_ref as cr
from bands import Band
from gpu_kit import INT_KEYS, REPO, dev, engines, pack, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(REPO, "tests", "golden", "cno.npz")
WORST_MEASURED = 6.45e-4               # largest |dS| / bound over test_band_sums_against_the_restatement on the MI355X (8 s window, 1000-1000.9 Hz; 2.3e-5 at the defaults)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def raw_call(eng, x_ptr, x_stride, n, wt=4.0, fl=400.0, fh=2000.0, bands=None, max_windows=0, res=None, null_n=False, null_p=False, null_res=False):
    from radae_amd.engine import CnoParams, CnoResult, _stream_ptr
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (eng.B,)))
    res = (CnoResult * eng.B)() if res is None else res
    p = CnoParams(wt, fl, fh)
    rc = eng.lib.rade_batch_cno_est(eng.h, C.c_void_p(x_ptr), x_stride, None if null_n else n.ctypes.data, None if null_p else C.byref(p),
                                    None if bands is None else bands.ctypes.data, max_windows, None if null_res else C.byref(res), _stream_ptr())
    return rc, res


def check_stream(x, got_bands, got_res, wt, fl, fh, what, skip_st=()):
    """one stream's band sums and result against the float64 restatement: counts, the bound on both sums of every window, the window list and the best window equal,
    every C/No within the bound propagated through est_CNo.py:44-52 (cno_ref.cnodb_bound).  Returns the largest |dS| / bound and the windows' C/No bounds in dB."""
    N, flow_bin, fhigh_bin, noise_st, noise_en = cr.plan(wt, fl, fh)
    ref = cr.band_sums(x, wt, fl, fh)
    r = cr.finish(ref, wt, fl, fh)
    assert got_res.n_windows == r["n_windows"] == len(ref), what
    worst, bdB = 0.0, {}
    Nbw = (noise_en - noise_st) / (N / cr.FS)
    keep = [w for w in range(len(ref)) if w * cr.HOP not in skip_st]
    pos_ref = [w for w in keep if r["C"][w] > 0]
    pos_got = []
    for w in range(len(ref)):
        xw = x[w * cr.HOP:w * cr.HOP + N]
        bc, bn = cr.band_bound(xw, ref[w, 0], fhigh_bin - flow_bin), cr.band_bound(xw, ref[w, 1], noise_en - noise_st)
        dc, dn = abs(got_bands[w, 0] - ref[w, 0]), abs(got_bands[w, 1] - ref[w, 1])
        worst = max(worst, dc / bc, dn / bn)
        assert dc <= bc and dn <= bn, (what, w, dc, bc, dn, bn)
        No = got_bands[w, 1] / Nbw
        Cg = got_bands[w, 0] - No * (fh - fl)
        if Cg > 0 and w in keep:
            pos_got.append(w)
        bdB[w] = cr.cnodb_bound(xw, ref[w, 0], ref[w, 1], wt, fl, fh)
        if Cg > 0 and r["C"][w] > 0 and np.isfinite(bdB[w]):
            got_dB, ref_dB = 10 * np.log10(Cg) - 10 * np.log10(No), 10 * np.log10(r["C"][w]) - 10 * np.log10(ref[w, 1] / Nbw)
            assert abs(got_dB - ref_dB) <= bdB[w], (what, w, got_dB, ref_dB, bdB[w])
    assert pos_got == pos_ref, what
    if not skip_st:
        assert got_res.n_positive == len(pos_ref) and got_res.max_st == r["max_st"], (what, got_res.max_st, r["max_st"])
        if r["max_CNodB"] > 0:
            assert abs(got_res.max_CNodB - r["max_CNodB"]) <= bdB[r["max_st"] // cr.HOP]
        assert got_res.max_SNRdB == got_res.max_CNodB - 10 * np.log10(3000)
    return worst, bdB


def shaped(rng, n, wt, fl, fh):
    """random complex64 at int16 scale (integers up to 32767 in both parts) plus a tone on each band edge bin (8000) and on the bin just outside it (5000)"""
    N, flow_bin, fhigh_bin, noise_st, noise_en = cr.plan(wt, fl, fh)
    x = rng.integers(-32767, 32768, n) + 1j * rng.integers(-32767, 32768, n)
    t = np.arange(n)
    for k_in, k_out in ((flow_bin, flow_bin - 1), (fhigh_bin - 1, fhigh_bin), (noise_st, noise_st - 1), (noise_en - 1, noise_en)):
        x = x + 8000.0 * np.exp(2j * np.pi * ((k_in * t) % N) / N) + 5000.0 * np.exp(2j * np.pi * ((k_out * t) % N) / N)
    return x.astype(np.complex64)


# ---- 1. the golden recordings ------------------------------------------------------------------------------------------------------------------------------------
def test_golden_recordings(engines, torch_dev, golden):
    """rec1 and rec2 (window 1 s) in one batch with rec0 and a fourth stream of another length, then rec0 (window 4 s) with three streams of other lengths: the window lists,
    max_st, n_windows and n_positive the script printed (apart from the listed window of the noise-only recording), its C/No values within the propagated bound (and
    within half a unit of its %5.2f print plus that bound)"""
    eng = engines(4)
    recs = [cr.int16_zeropad(golden[f"rec{k}"]) for k in range(3)]
    rng = np.random.default_rng(41)
    other = (300.0 * (rng.standard_normal(9001) + 1j * rng.standard_normal(9001))).astype(np.complex64)
    for wt, rows, which in ((1.0, [recs[0], recs[1], recs[2], other], {1: 1, 2: 2}), (4.0, [recs[0][:40000], recs[0], other.repeat(4)[:33000], recs[0][:32001]], {1: 0})):
        x, n = pack(rows)
        res, bands = eng.cno_est(dev(x, torch_dev), n=n, window_time=wt, bands=True)
        for b, row in enumerate(rows):
            k = which.get(b)
            skip = tuple(int(s) for s in golden["skip2"]) if k == 2 else ()
            _, bdB = check_stream(row, bands[b], res[b], wt, 400.0, 2000.0, f"window {wt} stream {b}", skip)
            if k is None:
                continue
            st, cno, m = golden[f"st{k}"], golden[f"cno{k}"], golden["measured"][k]
            N = int(8000 * wt)
            Nbw = (cr.plan(wt)[4] - cr.plan(wt)[3]) / (N / 8000)
            No = bands[b, :res[b].n_windows, 1] / Nbw
            Cg = bands[b, :res[b].n_windows, 0] - No * 1600.0
            mine = [(w * 2000, 10 * np.log10(Cg[w]) - 10 * np.log10(No[w])) for w in range(res[b].n_windows) if Cg[w] > 0 and w * 2000 not in skip]
            theirs = [(int(s), c) for s, c in zip(st, cno) if int(s) not in skip]
            assert [s for s, _ in mine] == [s for s, _ in theirs]
            assert all(abs(a - c) <= 0.005 + bdB[s // 2000] for (s, a), (_, c) in zip(mine, theirs))          # half a unit of the script's %5.2f, and the bound
            assert res[b].n_windows == len(cr.starts(len(row), N))
            if not skip:
                assert res[b].n_positive == len(st)
            assert f"{res[b].max_st / 8000:5.2f}" == f"{m[0]:5.2f}" and abs(res[b].max_CNodB - m[1]) <= 0.005 + bdB[res[b].max_st // 2000] and abs(res[b].max_SNRdB - m[2]) <= 0.005 + bdB[res[b].max_st // 2000]


# ---- 2. band sums under the counted bound, at the shapes where the kernel can go wrong -----------------------------------------------------------------------------
@pytest.mark.parametrize("wt,fl,fh", [(0.25, 400.0, 2000.0), (0.5, 400.0, 2000.0), (4.0, 400.0, 2000.0), (8.0, 400.0, 2000.0), (4.0, 433.0, 1999.0), (4.0, 1000.0, 1001.5),
                                      (8.0, 1000.0, 1000.9), (0.25, 1500.0, 6668.0)])
def test_band_sums_against_the_restatement(engines, torch_dev, wt, fl, fh):
    """J = 1, 2, 16, 32; bands whose edges fall on every kind of residue, bands narrower than J (most residues own no bin of the C + N band), a noise band that ends on the
    last bin but one; n = N (no window), N + 1, N + 2000 (one), N + 2001 (two) and N + 4500 (three): a batch whose streams differ in window count.  Tones sit on the
    edge bins and just outside them."""
    N = cr.plan(wt, fl, fh)[0]
    eng = engines(5)
    rng = np.random.default_rng(int(N + fl))
    rows = [shaped(rng, n, wt, fl, fh) for n in (N, N + 1, N + 2000, N + 2001, N + 4500)]
    x, n = pack(rows)
    res, bands = eng.cno_est(dev(x, torch_dev), n=n, window_time=wt, flow=fl, fhigh=fh, bands=True)
    assert [r.n_windows for r in res] == [0, 1, 1, 2, 3] and bands.shape == (5, 3, 2)
    assert (res[0].n_positive, res[0].max_st, res[0].max_CNodB) == (0, 0, 0.0) and res[0].max_SNRdB == -10 * np.log10(3000)
    worst = max(check_stream(rows[b], bands[b], res[b], wt, fl, fh, f"stream {b}")[0] for b in range(1, 5))
    print(f"window {wt} s, {fl}-{fh} Hz: largest |dS| / bound {worst:.3g} (measured so far: {WORST_MEASURED})")
    for b in range(5):
        assert not bands[b, res[b].n_windows:].any()                               # windows past a stream's own are not written


# ---- 3. the buffer contract ---------------------------------------------------------------------------------------------------------------------------------------
def test_buffer_contract(engines, torch_dev):
    """input rows in a sentinel buffer (NaN guards and gaps, odd stride, row 0 eight bytes off a 16-byte boundary): the input is untouched, no NaN reaches a result (nothing
    outside a stream's n samples is read), identical calls give identical bits, and a stream alone in a batch of 1 gives the bits it gives in a batch of 5"""
    wt, N = 0.5, 4000
    B, row = 5, N + 4500
    rng = np.random.default_rng(43)
    n = np.array([N + 4500, N + 1, N + 2001, N, N + 2000], np.int32)
    vals = np.stack([shaped(rng, row, wt, 400.0, 2000.0) for _ in range(B)])
    band = Band(B, row, row + 3, 8, torch_dev, base_offset_bytes=8).fill(vals)
    W = 3
    outs = []
    for _ in range(2):
        bh = np.full((B, W, 2), -1.0)
        rc, res = raw_call(engines(B), band.ptr, row + 3, n, wt=wt, bands=bh, max_windows=W)
        assert rc == 0
        outs.append((bh.copy(), bytes(res)))
    band.check(what="x")                                                           # rows still filled, gaps and guards still the sentinel
    assert np.array_equal(band.rows(np.complex64).view(np.int32), vals.view(np.int32))
    assert outs[0][1] == outs[1][1] and np.array_equal(outs[0][0].view(np.int64), outs[1][0].view(np.int64))
    bh, res = outs[0][0], (type(res)).from_buffer_copy(outs[0][1])
    for b in range(B):
        nw = res[b].n_windows
        assert np.isfinite(bh[b, :nw]).all() and np.all(bh[b, nw:] == -1.0)
        check_stream(vals[b, :n[b]], bh[b], res[b], wt, 400.0, 2000.0, f"stream {b}")
    one = Band(1, row, row + 5, 8, torch_dev).fill(vals[2:3])
    b1 = np.full((1, W, 2), -1.0)
    rc, r1 = raw_call(engines(1), one.ptr, row + 5, n[2:3], wt=wt, bands=b1, max_windows=W)
    assert rc == 0 and np.array_equal(b1[0].view(np.int64), bh[2].view(np.int64)) and bytes(r1) == bytes(res)[2 * C.sizeof(r1[0]):3 * C.sizeof(r1[0])]


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engines, torch_dev):
    """argument checking on the host: each of these returns -1 before any launch, and result_host and bands_host keep their bytes"""
    from radae_amd.engine import CnoResult
    B, N = 3, 2000
    row = N + 2001
    eng = engines(B)
    xin = Band(B, row, row + 1, 8, torch_dev).fill(shaped(np.random.default_rng(44), B * row, 0.25, 400.0, 2000.0).reshape(B, row))
    res = (CnoResult * B)()
    C.memset(res, 0xA5, C.sizeof(res))
    before = bytes(res)
    bh = np.full((B, 2, 2), -7.0)
    ok = dict(x_ptr=xin.ptr, x_stride=row + 1, n=row, wt=0.25, bands=bh, max_windows=2, res=res)
    nan, inf = float("nan"), float("inf")
    bad = [dict(x_ptr=0), dict(x_ptr=xin.ptr + 4), dict(null_n=True), dict(null_p=True), dict(null_res=True), dict(n=(row, -1, row)), dict(x_stride=row - 1),
           dict(n=(row, N - 1, row)), dict(n=(row, row, 0)), dict(wt=0.3), dict(wt=0.1), dict(wt=8.25), dict(wt=0.0), dict(wt=-1.0), dict(wt=nan), dict(wt=inf),
           dict(fl=nan), dict(fh=inf), dict(fl=2000.0), dict(fl=0.0, fh=36.0), dict(fl=1500.0, fh=6700.0), dict(fl=-400.0), dict(max_windows=1), dict(max_windows=0),
           dict(wt=8.0, fl=100.0, fh=2200.0, n=70000, x_stride=70000)]
    for kw in bad:
        rc, _ = raw_call(eng, **{**ok, **kw})
        assert rc == -1, kw
        assert bytes(res) == before and np.all(bh == -7.0), kw
    for kw in (dict(bands=None, max_windows=0), dict(n=(row, N, row - 1)), dict(fl=1500.0, fh=6668.0), dict(x_ptr=xin.ptr + 8, x_stride=row, n=row - 1), dict()):
        rc, _ = raw_call(eng, **{**ok, **kw})
        assert rc == 0, kw                                                         # ... and the same arguments without the fault are accepted
    assert bytes(res) != before and res[0].n_windows == 2
    xin.check(what="x")
    with pytest.raises(ValueError):
        eng.cno_est(dev(np.zeros((B, row), np.complex64), torch_dev), window_time=0.3)
    with pytest.raises(RuntimeError):
        eng.cno_est(dev(np.zeros((B, 100), np.complex64), torch_dev), window_time=0.25)


def test_changing_the_window_between_calls(engines, torch_dev):
    """0.5 s, then 0.25 s, then 0.5 s again on one engine: the table on the device follows N, and the third call gives the first one's bits"""
    eng = engines(3)
    x = np.stack([shaped(np.random.default_rng(45 + b), 9000, 0.5, 400.0, 2000.0) for b in range(3)])
    xt = dev(x, torch_dev)
    ra, a = eng.cno_est(xt, window_time=0.5, bands=True)
    rb, b = eng.cno_est(xt, window_time=0.25, bands=True)
    rc, c = eng.cno_est(xt, window_time=0.5, bands=True)
    assert np.array_equal(a.view(np.int64), c.view(np.int64)) and [bytes(r) for r in ra] == [bytes(r) for r in rc]
    check_stream(x[1], b[1], rb[1], 0.25, 400.0, 2000.0, "0.25 s between")


# ---- 5. end to end: ota.process_rx ----------------------------------------------------------------------------------------------------------------------------------
def test_process_rx_end_to_end(torch_dev):
    """Three recordings laid out as ota_test.sh:322-379 makes them, with the engine's own transmitter: a lead-in (0.75 s, 0.5 s, 1.1 s), the real part of the 4.5 s chirp,
    1 s of silence, x s of band-limited filler, 1 s of silence, x s of RADAE with end-of-over (20 modem frames); through wire_out / wire_in as real int16, plus real
    noise at two levels.  process_rx returns the start cno_ref picks on the same samples, which lies inside the 0.5 s of slack the 4.5 s chirp allows, and a receiver
    trace and features bit-equal to BatchEngine.rx on the slice cut here in numpy at the same offset; every stream reaches sync."""
    import torch
    from radae_amd import ota
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import BatchEngine
    B, n_mf = 3, 20
    lead = [6000, 4000, 8800]
    sigma = [150.0, 600.0, 150.0]
    eng = BatchEngine(B, max_tx_mf=n_mf, rx_trace_calls=64)
    feats = np.stack([synth_features(50 + b, n_mf * 12) for b in range(B)])
    iq = eng.tx(dev(feats, torch_dev))
    n_sig = iq.shape[1]
    quiet = torch.zeros((B, 8000 + n_sig + 1152), dtype=torch.complex64, device=torch_dev)
    radae = eng.channel(iq, 0.0, 0.0, n_pre=8000, n_post=0, with_eoo=True, noise=quiet)          # 1 s of silence, the frames, the end-of-over frame
    radae16 = eng.wire_out(radae, real=True, scale=8192.0).cpu().numpy()
    header = dev(np.tile(ota.ota_header(0.25), (B, 1)), torch_dev)
    chirp16 = eng.wire_out(header, real=True, scale=16384.0).cpu().numpy()
    x_len = n_sig + 1152
    rng = np.random.default_rng(46)
    rows = []
    for b in range(B):
        f = np.fft.rfft(rng.standard_normal(x_len))
        hz = np.fft.rfftfreq(x_len, 1 / 8000)
        f[(hz < 300) | (hz > 2700)] = 0
        filler = np.fft.irfft(f, x_len)
        filler = np.concatenate([np.zeros(8000), 3000.0 * filler / np.abs(filler).max()])
        clean = np.concatenate([np.zeros(lead[b]), chirp16[b].astype(np.float64), filler, radae16[b].astype(np.float64)])
        rows.append(np.clip(np.rint(clean + sigma[b] * rng.standard_normal(len(clean))), -32767, 32767).astype(np.int16))
    n = np.array([len(r) for r in rows], np.int32)
    s16 = np.zeros((B, int(n.max())), np.int16)
    for b in range(B):
        s16[b, :n[b]] = rows[b]
    x = eng.wire_in(dev(s16, torch_dev), n=n)
    eng.reset()
    r = ota.process_rx(eng, x, n)
    traces = [eng.rx_trace(b) for b in range(B)]
    feats_a = r.features.cpu().numpy()
    xs = x.cpu().numpy()
    cut = []
    for b in range(B):
        rb = cr.band_sums(xs[b, :min(int(n[b]), 80000)])
        ref = cr.finish(rb)
        assert r.start[b] == ref["max_st"] and lead[b] <= r.start[b] <= lead[b] + 4000, (b, r.start[b], ref["max_st"])
        wb = xs[b, ref["max_st"]:ref["max_st"] + 32000]
        sc, sn = rb[ref["max_st"] // 2000]
        assert r.max_time[b] == ref["max_st"] / 8000 and abs(r.CNodB[b] - ref["max_CNodB"]) <= cr.cnodb_bound(wb, sc, sn) and r.SNR3kdB[b] == r.CNodB[b] - 10 * np.log10(3000)
        total = int(n[b]) - int(r.start[b])
        off = int(r.start[b]) + int(np.floor((5 + (total / 8000 - 6) / 2) * 8000 + 0.5))
        assert r.radae_start[b] == off and r.n_radae[b] == n[b] - off
        silence = lead[b] + 36000 + 8000 + x_len                                   # the silence in front of the RADAE part starts here; the script's layout counts 4 s of
        assert silence - 2000 <= off <= silence, (b, off, silence)                 # chirp where 4.5 s were sent, so the receiver is fed from up to 0.25 s ahead of it
        assert tuple(r.ssb[b]) == (r.start[b] + 40000, r.start[b] + 40000 + int(np.floor((total / 8000 - 6) / 2 * 8000 + 0.5)))
        cut.append(xs[b, off:n[b]])
    print(f"start {r.start.tolist()}, C/No {np.round(r.CNodB, 2).tolist()} dB, receiver fed from {r.radae_start.tolist()}")
    y, ny = pack(cut)
    eng.reset()
    fo, st, _ = eng.rx(dev(y, torch_dev), n_avail=ny)
    fo = fo.cpu().numpy()
    for b in range(B):
        t = eng.rx_trace(b)
        for k in INT_KEYS + ["fmax"]:
            assert np.array_equal(t[k], traces[b][k]), (b, k)
        assert np.any(t["state_after"] == 2), f"stream {b} never reached sync"
        assert st[b].n_valid == r.status[b].n_valid > 0 and np.array_equal(fo[b, :st[b].n_valid].view(np.int32), feats_a[b, :st[b].n_valid].view(np.int32))
    eng.close()

