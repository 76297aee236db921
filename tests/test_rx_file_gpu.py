"""The stored-file receiver past the acquisition on the device (rade_file.hip: rade_batch_bpf_file; rade_irx.hip: rade_batch_rx_file, rade_batch_ber_align; radae_amd.acq.receive)
against the float64 restatements tests/file_ref.py and tests/acq_ref.py: the whole-file band-pass within the header's derived bound at every size at which the kernel takes
another path, its power-of-two covariance, the acquisition on kernel-filtered recordings, the ragged demodulator bit for bit against rade_batch_rx_ideal and against
single-stream runs, receive end to end on the committed recordings, the BER alignment, the buffer contract on sentinel buffers (tests/bands.py) and the refusals.

The filter's bound (include/rade_batch.h): |y^[i] - y[i]| <= RADE_FILE_BPF_EPS S[i] + RADE_FILE_BPF_TINY X, S[i] = sum_t |h[t]| |x[i - 100 + t]|, X the stream's largest
|component|.  A worst-case bound under the header's assumption about the matrix instruction's rounding; WORST_MEASURED records how far below it the device stays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import acq_ref as R
import file_ref as F
from bands import Band
from gpu_kit import REPO, bits, crandn, define, dev, engine, engines, pack, stream, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

WORST_MEASURED = 0.0748                # largest |dy| / bound over test_filter_sizes_bound_and_contract on the MI355X


def header_value(name):
    """the value of `#define name (a / b)` in include/rade_batch.h"""
    with open(os.path.join(REPO, "include", "rade_batch.h")) as f:
        m = re.search(r"^#define %s \((\d+\.\d+) / (\d+\.\d+)\)" % re.escape(name), f.read(), re.M)
    return float(m.group(1)) / float(m.group(2))


EPS, TINY = header_value("RADE_FILE_BPF_EPS"), header_value("RADE_FILE_BPF_TINY")
SPAN = define("RD_FILE_CHUNK") * define("RD_FILE_NCHUNK")             # outputs per workgroup of k_file_bpf (rade_dev.h: RD_FILE_SPAN)
assert (EPS, TINY) == (2.0 / 2 ** 20, 2.0 ** -27) and SPAN % 256 == 0
NMF, M, ZMF = 960, 160, 240
KK = 2 * np.sqrt(-np.log(1e-5 / 5)) / (NMF * 40) / np.sqrt(np.pi / 2) / 2


def filter_bound(x):
    from radae_amd.acq import bpf_design
    h, _ = bpf_design()
    x = np.asarray(x, np.complex128)
    S = np.convolve(np.concatenate([np.zeros(R.NTAP - 1), np.abs(x)]), np.abs(h.astype(np.float64)), "valid")
    return EPS * S + TINY * max(np.abs(x.real).max(), np.abs(x.imag).max())


def raw_bpf(eng, x_ptr, x_stride, n, y_ptr, y_stride, null_n=False):
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (eng.B,)))
    return eng.lib.rade_batch_bpf_file(eng.h, C.c_void_p(x_ptr), x_stride, None if null_n else n.ctypes.data, C.c_void_p(y_ptr), y_stride, stream())


# ---- 1. the filter ------------------------------------------------------------------------------------------------------------------------------------------------
def test_filter_sizes_bound_and_contract(engines, torch_dev):
    """one call, nine streams: n = 1, 100, 101 (the taps), 256, 257 (a tile), one below / at / one above the workgroup's span of 8192, and 3 spans + 7, each with its own
    level (2^-6 .. 2^2) and a quiet stretch across a chunk boundary; rows in sentinel buffers at an odd stride, 8 bytes off a 16-byte boundary, NaN behind a stream's n
    samples.  Every output within the bound, exactly n[b] samples written, x untouched, no NaN read"""
    lens = [1, 100, 101, 256, 257, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 7]
    B, row = len(lens), 3 * SPAN + 7
    rng = np.random.default_rng(21)
    vals = np.full((B, row), np.nan + 1j * np.nan, np.complex64)
    for b, L in enumerate(lens):
        v = crandn(rng, L) * np.float32(2.0 ** (b - 6))
        v[900:1100] *= np.float32(1e-4)                                # (where the stream is that long) a quiet stretch over the first chunk boundary
        vals[b, :L] = v
    xin = Band(B, row, row + 5, 8, torch_dev, base_offset_bytes=8).fill(vals)
    out = Band(B, row, row + 3, 8, torch_dev, base_offset_bytes=8)
    assert raw_bpf(engines(B), xin.ptr, row + 5, lens, out.ptr, row + 3) == 0
    xin.check(what="x")
    assert np.array_equal(xin.rows(np.int32), vals.view(np.int32)), "x was written"
    out.check(written=lens, what="y")
    y = out.rows(np.complex64)
    worst = 0.0
    for b, L in enumerate(lens):
        d = np.abs(y[b, :L] - R.bpf(vals[b, :L]))
        frac = float((d / filter_bound(vals[b, :L])).max())
        print(f"n = {L}: largest |dy| / bound {frac:.3g}")
        worst = max(worst, frac)
    print(f"filter: largest |dy| / bound {worst:.3g} (measured so far: {WORST_MEASURED})")
    assert worst <= 1.0
    again = Band(B, row, row + 3, 8, torch_dev, base_offset_bytes=8)
    assert raw_bpf(engines(B), xin.ptr, row + 5, lens, again.ptr, row + 3) == 0
    assert np.array_equal(again.host(), out.host()), "identical calls, different bits"


def test_filter_zero_stream_and_powers_of_two(engines, torch_dev):
    """an all-zero stream gives zeros; 2^-100 x and 2^100 x give 2^-100 y and 2^100 y bit for bit (the block scales and the pre-scale are powers of two); and a stream's
    bits do not depend on the batch"""
    rng = np.random.default_rng(22)
    L = SPAN + 300
    v = (rng.integers(-512, 513, L) + 1j * rng.integers(-512, 513, L)).astype(np.complex64) / np.float32(1024)      # exact under either scale
    rows = [v, v * np.float32(2.0 ** -100), v * np.float32(2.0 ** 100), np.zeros(L, np.complex64)]
    y = engines(4).bpf_file(dev(np.stack(rows), torch_dev)).cpu().numpy()
    assert np.all(np.abs(y[0] - R.bpf(v)) <= filter_bound(v))
    assert np.array_equal((y[0] * np.float32(2.0 ** -100)).view(np.int32), y[1].view(np.int32))
    assert np.array_equal((y[0] * np.float32(2.0 ** 100)).view(np.int32), y[2].view(np.int32))
    assert np.all(y[3] == 0)
    y1 = engines(1).bpf_file(dev(v[None], torch_dev)).cpu().numpy()
    assert np.array_equal(y1[0].view(np.int32), y[0].view(np.int32))


def check_hops(ref, got, n_hops, what):
    """every hop of one stream against float64, none left out: the record within the header's bound (RADE_ACQ_EPS, section 3.17) of the cell it names, and the arg-max and
    the candidate flag equal to the reference's in EVERY hop -- not only, as the hop rule of tests/test_acq_gpu.py has it, where that bound decides them.  Returns the
    number of hops that rule would have let pass unchecked (reported, not used)"""
    assert n_hops == len(ref), what
    undecided = 0
    for k, (h, g) in enumerate(zip(ref, got[:n_hops])):
        w = f"{what}, hop {k}"
        t, f = int(g["tmax"]), int(g["f_ind"])
        assert abs(g["Dtmax12"] - h["cells"][t, f]) <= h["b12"][t, f], (w, g["Dtmax12"], h["cells"][t, f], h["b12"][t, f])
        assert abs(g["S1"] - h["S1"]) <= R.EPS * h["A1"] and abs(g["S2"] - h["S2"]) <= R.EPS * h["A2"], w
        assert g["Dthresh"] == KK * (g["S1"] + g["S2"]) or abs(g["Dthresh"] / (KK * (g["S1"] + g["S2"])) - 1) < 1e-14, w
        assert (t, f) == (h["tmax"], h["f_ind"]), (w, (t, f), (h["tmax"], h["f_ind"]))
        assert bool(g["candidate"]) == h["candidate"], w
        undecided += (h["Dtmax12"] - h["second"] <= h["b12"][h["tmax"], h["f_ind"]] + h["b12"].ravel()[h["second_at"]] or
                      abs(h["Dtmax12"] - h["Dthresh"]) <= h["b12"][h["tmax"], h["f_ind"]] + KK * R.EPS * (h["A1"] + h["A2"]))
    return undecided


def test_acquisition_over_the_kernel_filtered_recordings(engines, torch_dev):
    """acq_detect over bpf_file's output of the mpp and awgn recordings against acq_ref.detect(acq_ref.bpf(x)) under the acquisition's own bound (the filter's error, a
    few 1e-7 of the samples, is a small part of it): in all 30 + 24 hops the record is within the bound and names the reference's cell and candidate flag; no hop is
    left out.  (Measured: one of the 54, hop 28 of mpp, leads its runner-up by 1.08e-4 where the two cells' bounds add up to 1.36e-4; it is held to equality like the rest.)"""
    rows = [R.fixture_input(k) for k in ("mpp", "awgn")]
    x, n = pack(rows)
    eng = engines(2)
    y = eng.bpf_file(dev(x, torch_dev), n)
    hops, nh = eng.acq_detect(y, n)
    assert nh.tolist() == [30, 24]
    for b, name in enumerate(("mpp", "awgn")):
        und = check_hops(R.detect(R.bpf(rows[b])), hops[b], nh[b], name)
        print(f"{name}: all {nh[b]} hops equal the reference's; {und} of them closer than the bound decides")


# ---- 2. the demodulator ---------------------------------------------------------------------------------------------------------------------------------------------
def test_demodulator_equals_rx_ideal_bit_for_bit(engine, torch_dev, golden):
    """start 0, freq 0, equal n_mf: z_hat and features are rade_batch_rx_ideal's bits in every EQ mode, with coarse_mag on and off, time_offset 0 and -16; at the
    recording's whole length and at the smallest frame counts: 2 (every frame is the first or the last) and 3 (one frame that is neither)"""
    import torch
    rx_np = golden("chan_mpp")["rx"]
    full = len(rx_np) // NMF
    eng = engine(2, max_tx_mf=full)
    rx = torch.tensor(np.stack([rx_np, np.roll(rx_np, 960 * 3)]), device=torch_dev)
    for n_mf in (full, 2, 3):
        for eq in ("ls", "mean6", "all", "none"):
            for cm in (True, False):
                for to in (0, -16):
                    f0, z0, _ = eng.rx_ideal(rx, n_mf, time_offset=to, eq=eq, coarse_mag=cm)
                    f1, z1 = eng.rx_file(rx, [(0, n_mf, 0.0)] * 2, time_offset=to, eq=eq, coarse_mag=cm)
                    assert torch.equal(z0, z1) and torch.equal(f0, f1), (n_mf, eq, cm, to)


def test_demodulator_takes_its_own_start_and_frequency(engine, torch_dev, golden):
    """chan_mpp's rx behind 37 zeros (an odd offset), mixed up on the host by +7.25 Hz counted from its own first sample: with start and freq given the result is the
    reference's a_ls_t16_bn3, under the rule of tests/test_ideal_rx_gpu.py"""
    import torch
    g, rx = golden("ideal_rx"), golden("chan_mpp")["rx"]
    start, freq, n_mf = 37, 7.25, len(rx) // NMF
    xs = np.concatenate([np.zeros(start, np.complex64), (rx * np.exp(2j * np.pi * freq / 8000 * np.arange(len(rx)))).astype(np.complex64)])
    _, z = engine(1, max_tx_mf=2).rx_file(torch.tensor(xs[None], device=torch_dev), [(start, n_mf, freq)], feat_width=0)
    F.check_z(z.cpu().numpy()[0], g["a_ls_t16_bn3"], "start 37, +7.25 Hz")
    F.check_z(z.cpu().numpy()[0], F.demod(F.mix(xs, start, freq)), "float64 restatement")


def test_ragged_batch(engine, torch_dev, golden):
    """n_mf = 2, 3, 20, 0 in one call, each stream at its own start and frequency, z_hat and the features in sentinel buffers: a stream's valid rows are the bits of the
    stream run alone (the decoder is causal: its zero tail cannot reach them), z_hat rows past 3 n_mf are zeros, nothing behind 3 max_mf rows is written"""
    import torch
    from radae_amd.abi import FileRxIn
    rx = golden("chan_mpp")["rx"]
    plans = [(5, 2, 3.0), (961, 3, 0.0), (0, 20, -2.5), (100, 0, 1.0)]
    B, max_mf, fw = 4, 20, 84
    eng = engine(B, max_tx_mf=max_mf)
    x = torch.tensor(np.stack([np.roll(rx, 7 * b) for b in range(B)]), device=torch_dev)
    fb = Band(B, 3 * max_mf * fw, 3 * max_mf * fw, 4, torch_dev)
    rec = np.zeros(B, np.dtype(FileRxIn))
    for b, p in enumerate(plans):
        rec[b] = p
    # (a stride of z_hat other than 240 max_mf is not part of the call: the rows are dense, the guards of the band stand in front and behind)
    zb = Band(B, 3 * max_mf * 80, 3 * max_mf * 80, 4, torch_dev)
    assert eng.lib.rade_batch_rx_file(eng.h, C.c_void_p(x.data_ptr()), x.stride(0), rec.ctypes.data, max_mf, -16, 0, 1, C.c_void_p(zb.ptr), C.c_void_p(fb.ptr), stream()) == max_mf
    zb.check(what="z_hat"); fb.check(what="features")
    z, f = zb.rows(np.float32).reshape(B, 3 * max_mf, 80), fb.rows(np.float32).reshape(B, 3 * max_mf, fw)
    one = engine(1, max_tx_mf=max_mf)
    for b, (start, n_mf, freq) in enumerate(plans):
        assert np.all(z[b, 3 * n_mf:] == 0), b
        if n_mf:
            f1, z1 = one.rx_file(x[b:b + 1], [(start, n_mf, freq)])
            assert np.array_equal(bits(z1.cpu().numpy()[0]), bits(z[b, :3 * n_mf])), f"stream {b}: z_hat differs from the stream alone"
            assert np.array_equal(bits(f1.cpu().numpy()[0]), bits(f[b, :3 * n_mf])), f"stream {b}: features differ from the stream alone"
            F.check_z(z[b, :3 * n_mf], F.demod(F.mix(x[b].cpu().numpy(), start, freq), n_mf=n_mf), f"stream {b}")


# ---- 3. receive end to end ------------------------------------------------------------------------------------------------------------------------------------------
def check_receive(eng, res, inputs, refs, margins, torch_dev):
    """event, refined (t, f), start and n_mf of every stream equal file_ref.plan where the float64 refine leads its runner-up by more than the stream's margin; z_hat and
    features"""
    import torch
    undecidable = 0
    for b, (r, x, p) in enumerate(zip(res, inputs, refs)):
        assert len(r.acq.events) == 1 and (int(r.acq.events[0]["hop"]), int(r.acq.events[0]["tmax"])) == (p["hop"], p["tmax"]), b
        if p["Dmax"] - p["second"] <= margins[b]:
            undecidable += 1
            continue
        assert (int(r.acq.refined[0]["t"]), float(r.acq.refined[0]["f"])) == (p["t"], p["f"]), (b, r.acq.refined[0], p["t"], p["f"])
        assert (r.plan.status, r.plan.start, r.plan.n_mf, r.plan.freq) == (F.OK, p["start"], p["n_mf"], p["f"]), b
        zr = F.demod(F.mix(x, p["start"], p["f"]), n_mf=p["n_mf"])
        F.check_z(r.z_hat.cpu().numpy(), zr, f"stream {b}")
        fr = eng.decode(torch.tensor(np.broadcast_to(zr.astype(np.float32), (eng.B,) + zr.shape).copy(), device=torch_dev), 84).cpu().numpy()[0]
        assert np.sqrt(np.mean((r.features.cpu().numpy() - fr) ** 2)) <= 1e-4, b
    print(f"receive: {undecidable} undecidable refines of {len(res)}")
    assert undecidable == 0
    return undecidable


def refine_margin(name, p):
    """how far the kernel's filter can move refine's |Dt1 + Dt2| on a recording, twice (the winner and its runner-up): Dt = sum_m y[t + m] q[m] with |q[m]| = |p[m]| over
    the two windows, so |dD| <= sum_m (e[t + m] + e[t + 960 + m]) |p[m]|, e[i] the header's bound on the filter's output (RADE_FILE_BPF_EPS S[i] + RADE_FILE_BPF_TINY X) plus
    2^-24 |y[i]| for the complex64 the float64 filter is rounded to before the reference refines it; the largest of the three timings; plus refine's own 1e-10 Dmax"""
    pil, _ = R.consts()
    x = R.fixture_input(name)
    e = filter_bound(x) + 2.0 ** -24 * np.abs(R.bpf(x))
    d = max(float((e[t:t + M] + e[t + NMF:t + NMF + M]) @ np.abs(pil)) for t in (p["t"] - 1, p["t"], p["t"] + 1))
    return 2 * d + 1e-10 * p["Dmax"]


def test_receive_on_the_recordings(engine, torch_dev):
    """B = 8 with per-stream n.  Call 1 (no filter): the four recordings raw and band-passed on the host; every figure equals file_ref.plan (the refine kernel's double
    rounding, 1e-10 of Dmax, decides).  Call 2 (the kernel's filter): the four recordings, noise, the carrier and two shifted recordings; against the plan over the
    float64 filter, decided where the lead exceeds what the filter's bound can move (refine_margin: a few 1e-5 of Dmax on these recordings, the leads are above 2e-3);
    noise and the carrier end as not acquired with zero rows"""
    from radae_amd import acq
    eng = engine(8, max_tx_mf=20)
    inputs = [F.recording(k, bpf) for bpf in (False, True) for k in R.RECORDINGS]
    x, n = pack(inputs)
    res = acq.receive(eng, dev(x, torch_dev), n, bpf=False)
    refs = [F.recording_plan(k, bpf) for bpf in (False, True) for k in R.RECORDINGS]
    check_receive(eng, res, inputs, refs, [1e-10 * p["Dmax"] for p in refs], torch_dev)
    x2, n2 = pack([R.fixture_input(k) for k in R.ALL])
    res2 = acq.receive(eng, dev(x2, torch_dev), n2, bpf=True)
    margins = [refine_margin(k, p) for k, p in zip(R.RECORDINGS, refs[4:])]
    print("refine margins / Dmax:", [f"{m / p['Dmax']:.2g}" for m, p in zip(margins, refs[4:])])
    check_receive(eng, res2[:4], inputs[4:], refs[4:], margins, torch_dev)
    for b in (4, 5):
        r = res2[b]
        assert r.plan.status == F.NOT_ACQUIRED and len(r.acq.events) == 0 and r.z_hat.shape[0] == 0 and r.features.shape[0] == 0, R.ALL[b]
    for b in (6, 7):
        assert res2[b].plan.status == F.OK and res2[b].plan.n_mf >= 2


# ---- 4. the BER alignment -------------------------------------------------------------------------------------------------------------------------------------------
def test_ber_align_counts(engines, torch_dev):
    """random sign latents, z_hat cut out of them at a shift with planted flips, lengths that make the last shifts run out and a length that is no multiple of a frame"""
    rng = np.random.default_rng(23)
    n_ref, n_hat, shift = [12 * ZMF, 25 * ZMF + 17, 5 * ZMF, 0], [6 * ZMF, 20 * ZMF, 3 * ZMF + 5, ZMF], [3, 2, 1, 0]
    zr, zh = np.zeros((4, max(n_ref) + 3), np.float32), np.zeros((4, max(n_hat) + 1), np.float32)
    for b in range(4):
        zr[b, :n_ref[b]] = np.sign(rng.standard_normal(n_ref[b]))
        src = np.concatenate([zr[b, shift[b] * ZMF:n_ref[b]], np.sign(rng.standard_normal(n_hat[b]))])[:n_hat[b]].copy()
        src[rng.integers(0, n_hat[b], 7)] *= -1
        zh[b, :n_hat[b]] = src * rng.uniform(0.1, 2.0, n_hat[b])
    zr[:, -3:] = np.nan; zh[:, -1:] = np.nan                            # behind the longest stream: never read
    err = engines(4).ber_align(dev(zr, torch_dev), dev(zh, torch_dev), n_ref, n_hat)
    for b in range(4):
        want, best, ber = F.ber_align(zr[b, :n_ref[b]], zh[b, :n_hat[b]])
        assert np.array_equal(err[b], want), (b, err[b], want)
        assert engines(4).ber_best(err[b], n_ref[b]) == (best, ber)
    assert np.all(err[3] == -1) and err[2, 5] == -1 and err[2, 4] >= 0 and engines(4).ber_best(err[0], n_ref[0])[0] == 3


def test_ber_of_a_clean_loop(engine, torch_dev):
    """sign latents through rade_batch_tx_latents (TX_LINEAR), no channel noise, the signal 3.4 frames into weak noise, through receive with the filter: the best shift
    is the number of whole frames the receiver starts behind the signal's first, with no error there"""
    import torch
    from radae_amd import acq
    from radae_amd.engine import TX_LINEAR
    n_mf, lead = 24, 3264
    eng = engine(1, max_tx_mf=n_mf, flags=TX_LINEAR)
    rng = np.random.default_rng(24)
    z = torch.tensor(np.sign(rng.standard_normal((1, 3 * n_mf, 80))).astype(np.float32), device=torch_dev)
    iq = eng.tx_latents(z).cpu().numpy()[0]
    x = 1e-3 * crandn(rng, lead + len(iq) + 700)
    x[lead:lead + len(iq)] += iq
    r = acq.receive(eng, dev(x[None], torch_dev), z_ref=z.reshape(1, -1))[0]
    assert r.plan.status == F.OK
    off = r.plan.start - lead - 50                                      # the filter delays the signal by (Ntap - 1) / 2 samples
    j = int(round(off / NMF))
    assert abs(off - NMF * j) <= 2 and j == int(r.acq.events[0]["hop"]) + 1 - 3, (r.plan.start, j, r.acq.events)
    best, ber = eng.ber_best(r.n_errors, ZMF * n_mf)
    assert (best, ber) == (j, 0.0) and r.n_errors[j] == 0, (best, ber, r.n_errors)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine, torch_dev):
    """argument checking on the host: each of these returns -1 before any launch and the outputs keep their sentinels; the same arguments without the fault are accepted"""
    from radae_amd.abi import FileRxIn
    B, row = 2, 2500
    eng = engine(B, max_tx_mf=2)
    rng = np.random.default_rng(25)
    xin = Band(B, row, row + 1, 8, torch_dev).fill(crandn(rng, B, row))
    out = Band(B, row, row + 1, 8, torch_dev)
    ok = dict(x_ptr=xin.ptr, x_stride=row + 1, n=row, y_ptr=out.ptr, y_stride=row + 1)
    for kw in (dict(x_ptr=0), dict(y_ptr=0), dict(x_ptr=xin.ptr + 4), dict(y_ptr=out.ptr + 4), dict(null_n=True), dict(n=(row, -1)), dict(n=(row, row + 2)), dict(y_stride=row - 1),
               dict(x_stride=row - 1), dict(y_ptr=xin.ptr), dict(y_ptr=xin.ptr + 8 * 100), dict(y_ptr=xin.ptr + 8 * (2 * row))):
        assert raw_bpf(eng, **{**ok, **kw}) == -1, kw
        out.untouched(what=f"y after {kw}"); xin.check(what="x")
    assert raw_bpf(eng, **ok) == 0 and raw_bpf(eng, **{**ok, "n": (0, 0)}) == 0
    # rade_batch_rx_file
    zb, fb = Band(B, 6 * 80, 6 * 80, 4, torch_dev), Band(B, 6 * 84, 6 * 84, 4, torch_dev)
    rec = np.zeros(B, np.dtype(FileRxIn))

    def rx_file(x=xin.ptr, stride=row + 1, r=None, max_mf=2, to=-16, eq=0, z=zb.ptr, f=fb.ptr, plans=((0, 2, 0.0), (500, 2, 1.0))):
        for b, p in enumerate(plans):
            rec[b] = p
        return eng.lib.rade_batch_rx_file(eng.h, C.c_void_p(x), stride, rec.ctypes.data if r is None else r, max_mf, to, eq, 1, C.c_void_p(z), C.c_void_p(f), stream())
    nan = float("nan")
    for kw in (dict(x=0), dict(x=xin.ptr + 4), dict(r=0), dict(z=0), dict(z=zb.ptr + 4), dict(max_mf=0), dict(max_mf=3), dict(to=-33), dict(to=1), dict(eq=4), dict(eq=-1),
               dict(plans=((0, 1, 0.0), (0, 2, 0.0))), dict(plans=((0, -1, 0.0), (0, 2, 0.0))), dict(plans=((0, 3, 0.0), (0, 2, 0.0))), dict(plans=((-1, 2, 0.0), (0, 2, 0.0))),
               dict(plans=((0, 2, 0.0), (row + 1 - 1919, 2, 0.0))), dict(plans=((0, 2, nan), (0, 2, 0.0)))):
        assert rx_file(**kw) == -1, kw
        zb.untouched(what=f"z_hat after {kw}"); fb.untouched(what=f"features after {kw}")
    assert rx_file(plans=((0, 2, 0.0), (row + 1 - 1920, 2, 0.0)), f=0) == 2 and rx_file() == 2
    # rade_batch_ber_align
    zr = Band(B, 960, 961, 4, torch_dev).fill(np.ones((B, 960), np.float32))
    err = np.full((B, 20), -7, np.int64)
    n_ok = np.array([960, 480], np.int64)

    def ber(r=zr.ptr, h=zb.ptr, nr=n_ok, nh=np.array([480, 480], np.int64), e=err.ctypes.data, rs=961, hs=480):
        return eng.lib.rade_batch_ber_align(eng.h, C.c_void_p(r), rs, None if nr is None else nr.ctypes.data, C.c_void_p(h), hs, None if nh is None else nh.ctypes.data, e, stream())
    for kw in (dict(r=0), dict(h=0), dict(r=zr.ptr + 2), dict(nr=None), dict(nh=None), dict(e=None), dict(nr=np.array([962, 0], np.int64)), dict(nr=np.array([-1, 0], np.int64)),
               dict(nh=np.array([0, 481], np.int64))):
        assert ber(**kw) == -1, kw
        assert np.all(err == -7), kw
    assert ber() == 0 and np.all(err[:, 4:] == -1) and np.all(err[0, :4] >= 0)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------------------------------------------
SCRIPT_FLAGS = ["--pilots", "--pilot_eq", "--bottleneck", "3", "--cp", "0.004", "--coarse_mag", "--time_offset", "-16"]      # rx.sh and the rx_* ctests


def test_cli_rx_decode(torch_dev, tmp_path, capsys):
    """cli rx --decode with the script's flags on the awgn recording: --pilot_eq alone is the least-squares equaliser (rx.py builds its model with eq_mean6 = False), so the
    feature file (20 of the 21 decoded features in 36 columns, the rest zeros) and the latents are receive(eq = "ls", coarse_mag = True)'s bytes; the script's lines up to
    the acquiring frame, "Acquired!", "refined fmax", the BER lines; a recording that does not acquire writes nothing.  Without --decode: the acquisition's output, every
    frame's line, and no file"""
    from radae_amd import acq, cli
    from radae_amd.engine import BatchEngine
    x = R.fixture_input("awgn")
    path, feat, lat, zf = (str(tmp_path / k) for k in ("rx.f32", "feat.f32", "z_hat.f32", "z.f32"))
    x.tofile(path)
    assert cli.main(["rx", path, "model", feat] + SCRIPT_FLAGS) == 0
    out = capsys.readouterr().out.splitlines()
    assert not os.path.exists(feat)
    assert len([ln for ln in out if " state: " in ln]) == 24 and out.count("Acquired!") == 1 and out[-1] == "refined fmax: 11.000000" and out[0].startswith("samples: 24992 Nmf: 960")
    eng = BatchEngine(1, max_tx_mf=len(x) // NMF)
    r = acq.receive(eng, dev(x[None], torch_dev), eq="ls", coarse_mag=True)[0]
    z_hat, fh = r.z_hat.cpu().numpy(), r.features.cpu().numpy().reshape(-1, 21)
    r6 = acq.receive(eng, dev(x[None], torch_dev), eq="mean6", coarse_mag=True)[0]
    assert not np.array_equal(r6.z_hat.cpu().numpy(), z_hat)           # the equaliser the command must NOT pick gives other latents
    eng.close()
    p = F.recording_plan("awgn", True)
    assert (r.plan.start, r.plan.n_mf) == (p["start"], p["n_mf"]) and z_hat.shape == (3 * 14, 80)
    rng = np.random.default_rng(26)
    np.concatenate([np.sign(rng.standard_normal(2 * ZMF)), np.sign(z_hat.ravel())]).astype(np.float32).tofile(zf)      # the latents' own signs behind two other frames
    assert cli.main(["rx", path, "model", feat] + SCRIPT_FLAGS + ["--decode", "--write_latent", lat, "--ber_test", zf]) == 0
    out = capsys.readouterr().out.splitlines()
    assert len([ln for ln in out if " state: " in ln]) == p["hop"] + 1 and "Acquired!" in out and f"refined fmax: {p['f']:f}" in out
    ber = [ln for ln in out if ln.startswith("f: ")]
    assert ber[0].startswith(f"f:  0 n_bits: {16 * ZMF:d} ") and ber[-1] == f"f:  2 n_bits: {14 * ZMF:d} n_errors: 0 BER: 0.000"
    assert np.array_equal(np.fromfile(lat, np.float32).view(np.int32), z_hat.ravel().view(np.int32))
    got = np.fromfile(feat, np.float32).reshape(-1, 36)
    assert got.shape[0] == len(fh) and np.array_equal(got[:, :20].view(np.int32), fh[:, :20].view(np.int32)) and np.all(got[:, 20:] == 0)
    nf = str(tmp_path / "none.f32")
    R.fixture_input("noise").tofile(path)
    assert cli.main(["rx", path, "model", nf] + SCRIPT_FLAGS + ["--decode"]) == 0
    assert capsys.readouterr().out.splitlines()[-1] == "Acquisition failed...." and not os.path.exists(nf)
