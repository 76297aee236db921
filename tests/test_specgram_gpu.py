"""GPU tests (-m gpu) of the spectrogram stage (rade_batch_specgram, rade_spec.hip; include/rade_batch.h states the arithmetic): the magnitudes against the float64
restatement of tests/specgram_ref.py under the bound counted from the roundings, the image as an exact function of the device's own magnitudes, the image against the
float64 reference, the display band as a crop, the int16 format, the buffer contract on sentinel buffers (tests/bands.py), the refusals, silence, and
radae_amd.ota.process_rx and `cli specgram` end to end.

The bound (derived in include/rade_batch.h, restated here).  u = 2^-24.  Slices (2 m, 2 m + 1) of a stream are the two parts of one complex 2048-point transform of
z[i] = (v_a[i], v_b[i]); every factor has modulus 1 and a butterfly's outputs are bounded by the sum of its inputs' moduli, so the stages' errors add, each relative to
S = sum_i |z[i]|.  The window entry u and the operand's multiply u; per radix-4 stage two levels of additions 2 u, a table entry u, a lone product 4 u: five stages 35 u;
the radix-2 stage u; the separating addition u; the magnitude 3 u: 42 u, times 1.01 and rounded up: | mag^ - |X[k]| | <= 44 u S (specgram_ref.GAMMA, pair_sums).
A worst-case bound: random rounding errors stay far below it, which WORST_MEASURED records.  For the image test: S <= sqrt(2) sqrt(1280) ||v||_2 for slices of like energy,
so the count corresponds to 62 u where the issue's estimate of the undecided share asks for at most 187 u."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import specgram_ref as sr
from bands import Band
from gpu_kit import REPO, dev, engines, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
WORST_MEASURED = 4.79e-2               # largest |mag^ - mag| / bound over test_magnitudes_under_the_counted_bound on the MI355X (the one-sample stream, whose S is one |v|; 5e-3 on the noise streams)
N5 = [1281, 1440, 1441, 2401, 8037]    # one slice, one, two, eight, 43 (an odd count: the last slice has no partner)


def tone(n, k, amp):
    return amp * np.cos(2 * np.pi * ((k * np.arange(n)) % sr.NFFT) / sr.NFFT + 0.3 * k)


def make_streams():
    """int16 [5, 8037] and the counts N5: a stream that is zero except for one sample; tones exactly on bins 1, 52 and 768 (the band edges) and on 51 and 769 just outside;
    noise; a 400-2000 Hz chirp over a noise floor 46 dB below it; noise at int16 scale"""
    rng = np.random.default_rng(2024)
    s = np.zeros((5, max(N5)), np.float64)
    s[0, 700] = 12345
    s[1, :N5[1]] = tone(N5[1], 1, 3000) + tone(N5[1], 52, 5000) + tone(N5[1], 51, 2500) + tone(N5[1], 768, 4000) + tone(N5[1], 769, 2000) + 20 * rng.standard_normal(N5[1])
    s[2, :N5[2]] = 9000 * rng.standard_normal(N5[2])
    t = np.arange(N5[3]) / sr.FS
    T = N5[3] / sr.FS
    s[3, :N5[3]] = 20000 * np.cos(2 * np.pi * (400 * t + 0.5 * (1600 / T) * t * t)) + 100 * rng.standard_normal(N5[3])
    s[4, :N5[4]] = 9000 * rng.standard_normal(N5[4])
    return np.clip(np.rint(s), -32767, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def case(engines, torch_dev):
    """The batch of five, its float64 reference (computed once, shared, left unchanged) and the device's results for the 0-3000 Hz band with magnitudes"""
    s16 = make_streams()
    x = s16.astype(np.float32).astype(np.complex64)
    ref = [sr.mags(s16[b, :N5[b]]) for b in range(5)]
    S = [sr.pair_sums(s16[b, :N5[b]]) for b in range(5)]
    eng = engines(5)
    img, ns, pk, mag = eng.specgram(dev(x, torch_dev), n=np.array(N5, np.int32), mag=True)
    return dict(s16=s16, x=x, ref=ref, S=S, img=img.cpu().numpy(), ns=ns, pk=pk, mag=mag.cpu().numpy(), table=sr.levels_table())


def raw_call(eng, x_ptr, x_stride, n, fmt=0, gain=1.0, fmin=0.0, fmax=3000.0, lo=sr.LO, hi=sr.HI, peak_in=None, img_ptr=0, img_stride=0, mag_ptr=0, mag_stride=0, pk=None, ns=None,
             null_n=False, null_p=False, null_pk=False, null_ns=False, null_h=False):
    from radae_amd.engine import SpecgramParams, _stream_ptr
    n = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (eng.B,)))
    pk = np.zeros(eng.B, np.float32) if pk is None else pk
    ns = np.zeros(eng.B, np.int32) if ns is None else ns
    pin = None if peak_in is None else np.ascontiguousarray(np.broadcast_to(np.asarray(peak_in, np.float32), (eng.B,)))
    p = SpecgramParams(fmin, fmax, lo, hi, None if pin is None else pin.ctypes.data)
    rc = eng.lib.rade_batch_specgram(None if null_h else eng.h, C.c_void_p(x_ptr), x_stride, None if null_n else n.ctypes.data, fmt, gain, None if null_p else C.byref(p),
                                     C.c_void_p(img_ptr), img_stride, C.c_void_p(mag_ptr), mag_stride, None if null_pk else pk.ctypes.data, None if null_ns else ns.ctypes.data,
                                     _stream_ptr())
    return rc, pk, ns


class ByteBand:
    """B byte rows `stride` bytes apart inside one allocation whose every byte starts as a position-dependent pattern; row 0 at `offset` bytes from a 16-byte boundary"""
    def __init__(self, B, stride, offset, torch_dev):
        import torch
        self.B, self.stride, self.guard = B, stride, 4096 + offset
        total = 2 * 4096 + 16 + B * stride
        self.before = ((np.arange(total, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)
        self.t = torch.tensor(self.before, device=torch_dev)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.guard

    def check(self, rows):
        """rows[b]: the bytes stream b must hold from the start of its row; everything else keeps the pattern"""
        want = self.before.copy()
        for b, r in enumerate(rows):
            r = np.asarray(r, np.uint8).ravel()
            assert r.size <= self.stride
            want[self.guard + b * self.stride:self.guard + b * self.stride + r.size] = r
        got = self.t.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} bytes differ, the first at {int(bad[0]) - self.guard} from row 0"


# ---- 1. magnitudes under the counted bound ---------------------------------------------------------------------------------------------------------------------
def test_magnitudes_under_the_counted_bound(case):
    worst = 0.0
    for b in range(5):
        ns = len(sr.starts(N5[b]))
        assert case["ns"][b] == ns
        got, ref, bound = case["mag"][b, :ns].astype(np.float64), case["ref"][b], sr.GAMMA * case["S"][b][:, None]
        assert np.isfinite(got).all()
        ratio = np.abs(got - ref) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), (b, float(ratio.max()))
        assert not case["mag"][b, ns:].any()                                       # rows past a stream's slices are not written
        s_pk = int(np.argmax(ref.max(axis=1)))                                     # the peak within the bound of its slice
        assert abs(float(case["pk"][b]) - sr.peak(ref)) <= sr.GAMMA * case["S"][b][s_pk], b
        assert case["pk"][b] == case["mag"][b, :ns].max()
    print(f"largest |mag^ - mag| / bound: {worst:.3e} (WORST_MEASURED {WORST_MEASURED})")
    assert WORST_MEASURED is None or worst <= 2 * WORST_MEASURED                   # the record is kept honest: a device that doubles it has changed its arithmetic


# ---- 2. the image is an exact function of the device's own numbers -------------------------------------------------------------------------------------------------
def test_image_exact_from_the_devices_own_numbers(case, engines, torch_dev):
    from radae_amd.engine import specgram_levels
    table = specgram_levels()
    eng = engines(5)
    xt = dev(case["x"], torch_dev)
    n = np.array(N5, np.int32)
    for fmin, fmax in ((0.0, 3000.0), (200.0, 3000.0)):
        k0, k1 = sr.band(fmin, fmax)
        for scale in (None, 0.5, 2.0):
            pin = None if scale is None else (case["pk"] * np.float32(scale)).astype(np.float32)
            img, ns, pk = eng.specgram(xt, n=n, fmin=fmin, fmax=fmax, peak=pin)
            img = img.cpu().numpy()
            assert np.array_equal(pk, case["pk"] if pin is None else pin) and np.array_equal(ns, case["ns"])
            for b in range(5):
                want = sr.levels(case["mag"][b, :ns[b], k0 - 1:k1], pk[b], table)
                assert np.array_equal(img[b, :ns[b]], want), (fmin, scale, b)
                assert not img[b, ns[b]:].any()
    assert len(np.unique(case["img"][4, :case["ns"][4]])) > 200                    # the noise stream uses the grey scale


# ---- 3. the image against the float64 reference ----------------------------------------------------------------------------------------------------------------------
def test_image_against_the_float64_reference(case):
    """A cell is decided when the reference magnitude is farther from every threshold T peak64 than the cell's bound plus T times the peak's bound (plus the two float32
    roundings of T peak).  Decided cells are equal, the others differ by at most one level, and they are at most 10 % of the noise stream's image, 1 % of the chirp's."""
    T = case["table"]
    share = {}
    for b in range(5):
        ns = case["ns"][b]
        m = case["ref"][b][:, :768]
        p64 = sr.peak(case["ref"][b])
        cell = (sr.GAMMA * case["S"][b])[:, None]
        pkb = sr.GAMMA * case["S"][b].max() + 2 * sr.U * p64
        dist = np.abs(m[:, :, None] - T[None, None, :] * p64) - T[None, None, :] * pkb
        decided = (dist > cell[:, :, None]).all(axis=2)
        want, got = sr.levels64(m, p64), case["img"][b, :ns].astype(np.int64)
        assert np.array_equal(got[decided], want[decided]), b
        assert np.abs(got - want).max() <= 1, b
        share[b] = 1 - decided.mean()
    print("undecided share per stream:", {b: round(float(v), 5) for b, v in share.items()})
    assert share[4] <= 0.10 and share[3] <= 0.01


# ---- 4. the display band is a crop -------------------------------------------------------------------------------------------------------------------------------------
def test_crop(case, engines, torch_dev):
    eng = engines(5)
    xt, n = dev(case["x"], torch_dev), np.array(N5, np.int32)
    a, _, pa = eng.specgram(xt, n=n, fmin=200.0, fmax=3000.0)
    f, _, pf = eng.specgram(xt, n=n, fmin=0.0, fmax=4000.0)
    assert a.shape[2] == 717 and f.shape[2] == 1023 and case["img"].shape[2] == 768
    assert np.array_equal(a.cpu().numpy(), case["img"][:, :, 51:768]) and np.array_equal(f.cpu().numpy()[:, :, :768], case["img"])
    assert np.array_equal(pa, case["pk"]) and np.array_equal(pf, case["pk"])


# ---- 5. the int16 format ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 0.37])
def test_int16_equals_wire_in_then_complex(case, engines, torch_dev, gain):
    eng = engines(5)
    n = np.array(N5, np.int32)
    st = dev(case["s16"], torch_dev)
    a = eng.specgram(st, n=n, mag=True, gain=gain)
    b = eng.specgram(eng.wire_in(st, n=n, gain=gain), n=n, mag=True)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) and np.array_equal(a[3].cpu().numpy().view(np.int32), b[3].cpu().numpy().view(np.int32))
    assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32)) and np.array_equal(a[1], b[1])
    if gain == 1.0:
        assert np.array_equal(a[3].cpu().numpy().view(np.int32), case["mag"].view(np.int32))


# ---- 6. the buffer contract ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("img_off", [1, 7])
def test_buffer_contract(case, engines, torch_dev, img_off):
    """input, img and mag in sentinel bands with odd strides, img 1 or 7 bytes and mag 4 bytes off a 16-byte boundary"""
    B, row, W = 5, max(N5), 43
    n = np.array(N5, np.int32)
    ns = case["ns"]
    xin = Band(B, row, row + 4, 8, torch_dev, base_offset_bytes=8)
    vals = case["x"].copy()
    for b in range(B):
        vals[b, N5[b]:] = np.array([np.nan + 1j * np.nan], np.complex64)          # behind a stream's samples: what must not be read
    xin.fill(vals)
    mag_stride, img_stride = W * 1023 + 4, W * 768 + 3
    outs = []
    for _ in range(2):
        mg = Band(B, W * 1023, mag_stride, 4, torch_dev, base_offset_bytes=4)
        im = ByteBand(B, img_stride, img_off, torch_dev)
        rc, pk, nsl = raw_call(engines(B), xin.ptr, row + 4, n, img_ptr=im.ptr, img_stride=img_stride, mag_ptr=mg.ptr, mag_stride=mag_stride)
        assert rc == 0 and np.array_equal(nsl, ns) and np.array_equal(pk.view(np.int32), case["pk"].view(np.int32))
        mg.check(written=ns.astype(np.int64) * 1023, what="mag")                   # rows past a stream's slices, gaps and guards keep the sentinel
        im.check([case["img"][b, :ns[b]] for b in range(B)])
        outs.append((mg.rows(np.int32), im.t.cpu().numpy()))
    xin.check(what="x")
    assert np.array_equal(xin.rows(np.complex64).view(np.int32), vals.view(np.int32))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])           # two calls give identical bytes
    m = outs[0][0].view(np.float32).reshape(B, W, 1023)
    for b in range(B):
        assert np.isfinite(m[b, :ns[b]]).all() and np.array_equal(m[b, :ns[b]].view(np.int32), case["mag"][b, :ns[b]].view(np.int32))
    # either output alone
    im = ByteBand(B, img_stride, img_off, torch_dev)
    rc, pk, _ = raw_call(engines(B), xin.ptr, row + 4, n, img_ptr=im.ptr, img_stride=img_stride)
    assert rc == 0 and np.array_equal(pk, case["pk"])
    im.check([case["img"][b, :ns[b]] for b in range(B)])
    mg = Band(B, W * 1023, mag_stride, 4, torch_dev, base_offset_bytes=4)
    rc, pk, _ = raw_call(engines(B), xin.ptr, row + 4, n, mag_ptr=mg.ptr, mag_stride=mag_stride)
    assert rc == 0 and np.array_equal(pk, case["pk"]) and np.array_equal(mg.rows(np.int32), outs[0][0])
    # a stream alone in a batch of 1
    for b in (3, 4):
        one = Band(1, row, row + 5, 8, torch_dev).fill(vals[b:b + 1])
        mg1 = Band(1, W * 1023, mag_stride + 2, 4, torch_dev)
        im1 = ByteBand(1, img_stride + 4, img_off, torch_dev)
        rc, pk, nsl = raw_call(engines(1), one.ptr, row + 5, n[b:b + 1], img_ptr=im1.ptr, img_stride=img_stride + 4, mag_ptr=mg1.ptr, mag_stride=mag_stride + 2)
        assert rc == 0 and nsl[0] == ns[b] and pk[0] == case["pk"][b]
        im1.check([case["img"][b, :ns[b]]])
        mg1.check(written=int(ns[b]) * 1023, what="mag of one")
        assert np.array_equal(mg1.rows(np.int32)[0], outs[0][0][b])


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(case, engines, torch_dev):
    """argument checking on the host: each of these returns -1 before any launch; peak_host, n_slices_host, img and mag keep their bytes"""
    B, row, W = 5, max(N5), 43
    eng = engines(B)
    n = np.array(N5, np.int32)
    xin = Band(B, row, row + 1, 8, torch_dev).fill(case["x"])
    mg = Band(B, W * 1023, W * 1023 + 1, 4, torch_dev)
    im = ByteBand(B, W * 768 + 1, 0, torch_dev)
    pk, ns = np.full(B, -5.0, np.float32), np.full(B, -9, np.int32)
    ok = dict(x_ptr=xin.ptr, x_stride=row + 1, n=n, img_ptr=im.ptr, img_stride=W * 768 + 1, mag_ptr=mg.ptr, mag_stride=W * 1023 + 1, pk=pk, ns=ns)
    nan, inf = float("nan"), float("inf")
    short = n.copy(); short[2] = 1280
    neg = n.copy(); neg[1] = -1
    bad = [dict(null_h=True), dict(x_ptr=0), dict(null_n=True), dict(null_p=True), dict(null_pk=True), dict(null_ns=True),
           dict(img_ptr=0, mag_ptr=0, peak_in=1.0), dict(x_ptr=xin.ptr + 4), dict(mag_ptr=mg.ptr + 2), dict(fmt=1, x_ptr=xin.ptr + 1),
           dict(n=neg), dict(x_stride=row - 1), dict(n=short), dict(n=0), dict(img_stride=W * 768 - 1), dict(mag_stride=W * 1023 - 1), dict(fmt=2), dict(fmt=-1),
           dict(gain=nan), dict(gain=inf), dict(fmin=nan), dict(fmax=inf), dict(lo=nan), dict(hi=inf), dict(fmin=3000.0, fmax=200.0), dict(fmin=3.91, fmax=7.8),
           dict(fmin=4000.0, fmax=4000.0), dict(lo=0.0), dict(lo=-0.1), dict(lo=0.6, hi=0.5), dict(lo=0.5, hi=0.5), dict(hi=1.5), dict(peak_in=-1.0), dict(peak_in=nan)]
    for kw in bad:
        rc, _, _ = raw_call(eng, **{**ok, **kw})
        assert rc == -1, kw
        assert np.all(pk == -5.0) and np.all(ns == -9), kw
    mg.untouched(what="mag")
    im.check([])
    for kw in (dict(img_ptr=0), dict(mag_ptr=0), dict(img_ptr=0, mag_ptr=0), dict(mag_ptr=0, peak_in=1.0), dict(fmin=3.9, fmax=3.91), dict(hi=1.0), dict(x_stride=row), dict()):
        rc, _, _ = raw_call(eng, **{**ok, **kw})
        assert rc == 0, kw                                                         # ... and the same arguments without the fault are accepted
    assert np.array_equal(ns, case["ns"]) and np.array_equal(pk, case["pk"])
    xin.check(what="x")
    with pytest.raises(ValueError):
        eng.specgram(dev(case["x"], torch_dev), fmin=3000.0, fmax=200.0)
    with pytest.raises(RuntimeError):
        eng.specgram(dev(case["x"][:, :1280].copy(), torch_dev))


# ---- 8. silence ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_silence_next_to_a_live_stream(case, engines, torch_dev):
    eng = engines(5)
    x = case["x"].copy()
    x[2] = 0
    img, ns, pk, mag = eng.specgram(dev(x, torch_dev), n=np.array(N5, np.int32), mag=True)
    img, mag = img.cpu().numpy(), mag.cpu().numpy()
    assert pk[2] == 0 and not img[2].any() and not mag[2].any() and ns[2] == 2
    for b in (0, 1, 3, 4):
        assert pk[b] == case["pk"][b] and np.array_equal(img[b], case["img"][b]) and np.array_equal(mag[b].view(np.int32), case["mag"][b].view(np.int32))


# ---- 9. end to end: ota.process_rx and the command line ------------------------------------------------------------------------------------------------------------------
def chirp_hz(i):
    """the frequency chirp.py:50-65 has at sample i of the header: 400 Hz, rising 0.2 Hz per sample to 2000 Hz, falling again, and so on (a triangle of 16000 samples)"""
    ph = np.asarray(i, np.float64) % 16000
    return 400 + 0.2 * np.where(ph < 8000, ph, 16000 - ph)


def test_process_rx_with_spectrogram_and_cli(torch_dev, tmp_path):
    """Three recordings laid out as ota_test.sh:322-379 makes them (as tests/test_cno_gpu.py builds them): process_rx(.., spectrogram=True) returns BatchEngine.specgram
    of the same samples at 200-3000 Hz and leaves every other field as a run without the flag gives it; in the chirp's first 4 s the brightest bin of every slice lies
    inside the frequencies the chirp passes through under that slice's window, within two bins (chirp.py sweeps (fhigh - flow) / 8000 = 0.2 Hz per sample, 400 -> 2000 Hz
    in one second and back, so a 160 ms window sees up to 256 Hz of sweep; the issue's `400 + 400 t Hz` is not what the header does); `cli specgram` on the int16 file
    writes a PNG whose pixels are that image."""
    import torch
    from radae_amd import ota
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import BatchEngine
    B, n_mf = 3, 20
    lead = [6000, 4000, 8800]
    sigma = [150.0, 600.0, 150.0]
    eng = BatchEngine(B, max_tx_mf=n_mf)
    feats = np.stack([synth_features(50 + b, n_mf * 12) for b in range(B)])
    iq = eng.tx(dev(feats, torch_dev))
    n_sig = iq.shape[1]
    quiet = torch.zeros((B, 8000 + n_sig + 1152), dtype=torch.complex64, device=torch_dev)
    radae = eng.channel(iq, 0.0, 0.0, n_pre=8000, n_post=0, with_eoo=True, noise=quiet)
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
    plain = ota.process_rx(eng, x, n)
    eng.reset()
    r = ota.process_rx(eng, x, n, spectrogram=True)
    assert plain.spec is None and plain.spec_slices is None
    for k in ("max_time", "CNodB", "SNR3kdB", "start", "ssb", "radae_start", "n_radae"):
        assert np.array_equal(getattr(r, k), getattr(plain, k)), k
    assert np.array_equal(r.features.cpu().numpy().view(np.int32), plain.features.cpu().numpy().view(np.int32))
    assert [bytes(s) for s in r.status] == [bytes(s) for s in plain.status] and (r.eoo is plain.eoo or torch.equal(r.eoo, plain.eoo))
    img, ns, pk, mag = eng.specgram(x, n=n, fmin=200.0, fmax=3000.0, mag=True)
    assert torch.equal(r.spec, img) and np.array_equal(r.spec_slices, ns) and r.spec.shape[2] == 717
    mag = mag.cpu().numpy()
    for b in range(B):
        for s in range(ns[b]):
            i0 = s * sr.STEP - lead[b]                                             # the window's first sample, counted from the chirp's first
            if i0 < 0 or i0 + sr.WIN > 32000:
                continue
            hz = chirp_hz(np.arange(i0, i0 + sr.WIN))
            k = 1 + int(np.argmax(mag[b, s]))
            assert hz.min() * sr.NFFT / sr.FS - 2 <= k <= hz.max() * sr.NFFT / sr.FS + 2, (b, s, k, hz.min(), hz.max())
    eng.close()
    path, png = str(tmp_path / "rec.s16"), str(tmp_path / "rec.png")
    rows[0].tofile(path)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "radae_amd.cli", "specgram", path, png, "--fmin", "200"], check=True, cwd=REPO, env=env, timeout=120)
    pix = read_png(png)
    want = r.spec[0, :ns[0]].cpu().numpy()
    assert pix.shape == (717, ns[0]) and np.array_equal(pix, want.T[::-1])


def read_png(path):
    """the pixels of an 8-bit grey-scale PNG whose rows all use filter 0"""
    import struct
    d = open(path, "rb").read()
    assert d[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(d):
        ln, tag = struct.unpack(">I", d[pos:pos + 4])[0], d[pos + 4:pos + 8]
        body = d[pos + 8:pos + 8 + ln]
        assert struct.unpack(">I", d[pos + 8 + ln:pos + 12 + ln])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            w, h, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", body)
            assert (depth, colour, comp, filt, inter) == (8, 0, 0, 0, 0)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + ln
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)
    assert not raw[:, 0].any()
    return raw[:, 1:]
