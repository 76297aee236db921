"""GPU tests (-m gpu) of the analog FM modulator and demodulator (rade_batch_fm_mod, rade_batch_fm_demod, rade_fm.hip; include/rade_batch.h states the arithmetic):
bit-exact identities, the phasor and the discriminator's atan2 against float64, the modulator's integer phases bit for bit and its samples within EPS_CIS, the
demodulator stage by stage and end to end against the float64 restatement of tests/fm_ref.py under bounds counted from the roundings, generated noise against
tests/noise_ref.py, pieces against the whole, the buffer contract on sentinel buffers (tests/bands.py), host-side refusals, a change of taps between calls, and
`cli analog_fm` against the same chain on the float64 references.

EPS_CIS and EPS_ATAN follow the convention of tests/test_device_noise_gpu.py: four times the largest deviation measured on the MI355X by test_probe_phasor_and_atan2
(2^16 spread phases / angles and the edges of every quadrant and octant), and each must stay below 1e-6.
    EPS_CIS_MEASURED   7.753e-08: largest |device phasor - float64 phasor| (complex modulus), at phase 0x1ca0d4c7; EPS_CIS = 3.1e-07
    EPS_ATAN_MEASURED  1.192e-07 rad: largest |device atan2 - float64 atan2| over the whole circle, at (re, im) = (-0.05075179, 0.11006417): half a float32 ulp of an angle
                       above 2 rad (the double result is rounded once); EPS_ATAN = 4.8e-07
Other figures of the same run, each far inside its bound: modulator samples 5.6e-08 from the float64 phasor; stage 1 7.1e-07 (bound 2.7e-05); stage 2 6.6e-07 with the clamp and
9.9e-07 with ph_dont_limit (bound 2.7e-05); end to end 6.3e-07 at 96 kHz, C/N 20 dB (bound 9.8e-04); generated noise 1.35e-07 from sigma x the reference noise at sigma 0.25."""
import ctypes as C

import numpy as np
import pytest

import dev_abi
import fm_ref as fr
from bands import Band
from gpu_kit import bits, crandn, define, dev, engines, torch_dev  # noqa: F401
from noise_ref import EPS as NOISE_EPS          # the bar of gauss_pair against the float64 Box-Muller

pytestmark = pytest.mark.gpu
TILE, NMAX = define("RD_FM_TILE"), define("RD_FM_NMAX")

EPS_CIS_MEASURED = 7.753e-08     # largest |device phasor - float64 phasor| over test_probe_phasor_and_atan2's phases on the MI355X: at phase 0x1ca0d4c7
EPS_CIS = 4 * EPS_CIS_MEASURED
EPS_ATAN_MEASURED = 1.192e-07    # largest |device atan2 - float64 atan2| over its pairs on the MI355X: at (re, im) = (-0.05075179, 0.11006417), half a float32 ulp of 2.0 rad
EPS_ATAN = 4 * EPS_ATAN_MEASURED

FS, FC, FD, FM_MAX = 48000.0, 12000.0, 5000.0, 3000.0
B = 3
N = np.array([2 * TILE + 37, 2 * TILE + 1, TILE + 513], np.int32)          # about two tiles plus an odd remainder, unequal
NMAXS = int(N.max())


@pytest.fixture(scope="module")
def ref():
    """made once and never written: the two-tone input (0.5 sin 1 kHz + 0.5 sin 3 kHz, a start phase of its own per stream) in float32, the restated phases and
    phasors per rate, and the float32 filter tables"""
    made = {}

    def get(Fs=FS, fc=FC):
        if (Fs, fc) not in made:
            t = np.arange(NMAXS)[None, :] + np.array([0, 7, 19])[:, None]
            m = (0.5 * np.sin(2 * np.pi * 1000.0 / Fs * t) + 0.5 * np.sin(2 * np.pi * 3000.0 / Fs * t)).astype(np.float32)
            ph = np.stack([fr.nco_phase(m[b], Fs, fc, FD) for b in range(B)])
            b1, b2 = (v.astype(np.float32) for v in fr.design(Fs, FM_MAX, FD))
            b2d = fr.design(Fs, FM_MAX, FD, 201, fr.TC)[1].astype(np.float32)
            made[(Fs, fc)] = dict(m=m, ph=ph, tx=fr.cis(ph), b1=b1, b2=b2, b2d=b2d)
            for v in made[(Fs, fc)].values():
                v.setflags(write=False)
        return made[(Fs, fc)]
    return get


def cmax(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


def _arr(keep, v, dt, nb):
    if v is None:
        return None
    keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (nb,))))
    return keep[-1].ctypes.data


def raw_mod(eng, m_ptr, m_stride, n, y_ptr, y_stride, Fs=FS, fc=FC, fd=FD, fmt=fr.F32, mode=fr.OUT_COMPLEX, sigma=0.0, seed=0, noise_ptr=None, phase0=None, n0=None,
            want_end=False):
    """rade_batch_fm_mod through the C ABI with caller-owned pointers; returns its return value (and the final phases with want_end)"""
    from radae_amd.engine import FmModParams, _stream_ptr
    keep = []
    end = np.zeros(eng.B, np.uint32)
    p = FmModParams(Fs, fc, fd, fmt, mode, sigma, seed, noise_ptr, _arr(keep, phase0, np.uint32, eng.B), end.ctypes.data if want_end else None, _arr(keep, n0, np.int64, eng.B))
    r = eng.lib.rade_batch_fm_mod(eng.h, C.c_void_p(m_ptr), m_stride, _arr(keep, n, np.int32, eng.B), C.c_void_p(y_ptr), y_stride, C.byref(p), _stream_ptr())
    return (r, end) if want_end else r


def raw_demod(eng, x_ptr, x_stride, n_in, y_ptr, y_stride, n_out, b1, b2, Fs=FS, fc=FC, fd=FD, fmt=fr.F32, dont_limit=0, in_base=None, n0=None, bb_ptr=None, bb_stride=0,
              N1=None, N2=None):
    from radae_amd.engine import FmDemodParams, _stream_ptr
    keep = []
    b1 = None if b1 is None else np.ascontiguousarray(b1, np.float32)
    b2 = None if b2 is None else np.ascontiguousarray(b2, np.float32)
    p = FmDemodParams(Fs, fc, fd, fmt, dont_limit, None if b1 is None else b1.ctypes.data, (0 if b1 is None else b1.size) if N1 is None else N1,
                      None if b2 is None else b2.ctypes.data, (0 if b2 is None else b2.size) if N2 is None else N2,
                      _arr(keep, in_base, np.int64, eng.B), _arr(keep, n0, np.int64, eng.B), bb_ptr, bb_stride)
    return eng.lib.rade_batch_fm_demod(eng.h, C.c_void_p(x_ptr), x_stride, _arr(keep, n_in, np.int32, eng.B), C.c_void_p(y_ptr), y_stride, _arr(keep, n_out, np.int32, eng.B),
                                       C.byref(p), _stream_ptr())


# ---- 1. the two measurements -------------------------------------------------------------------------------------------------------------------------------------
def test_probe_phasor_and_atan2(torch_dev):
    """THE measurements behind EPS_CIS and EPS_ATAN: the device phasor on 2^16 phases spread over the circle by a golden-ratio stride plus the edges of every quadrant and
    octant, against float64; the discriminator's atan2 on 2^16 float32 pairs of spread angle and radius plus the axes, against float64 atan2 of the same float32 pairs"""
    import torch
    from radae_amd.engine import _stream_ptr
    lib = dev_abi.load()
    k = np.arange(1 << 16, dtype=np.uint64)
    edges = np.array([(q << 29) + d for q in range(8) for d in (-2, -1, 0, 1, 2)], np.int64) & 0xFFFFFFFF
    ph = np.concatenate([(k * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF), edges.astype(np.uint64)]).astype(np.uint32)
    rng = np.random.default_rng(40)
    th = np.concatenate([(k.astype(np.float64) + 0.5) * (2 * np.pi / (1 << 16)) - np.pi, np.arange(-4, 5) * (np.pi / 4)])
    rad = np.exp(rng.uniform(-6, 2, len(th)))
    d = np.stack([rad * np.cos(th), rad * np.sin(th)], axis=-1).astype(np.float32)
    d[-9:] = np.round(d[-9:] / rad[-9:, None]) * rad[-9:, None].astype(np.float32)      # the axes and diagonals exactly (zeros of either sign among them)
    n = max(len(ph), len(d))
    ph_t, d_t = dev(np.resize(ph, n).view(np.int32), torch_dev), dev(np.resize(d, (n, 2)), torch_dev)
    cis_t, at_t = torch.zeros((n, 2), dtype=torch.float32, device=torch_dev), torch.zeros(n, dtype=torch.float32, device=torch_dev)
    assert lib.rd_launch_fm_probe(ph_t.data_ptr(), cis_t.data_ptr(), d_t.data_ptr(), at_t.data_ptr(), n, _stream_ptr()) == 0
    torch.cuda.synchronize()
    c = cis_t.cpu().numpy().astype(np.float64)[:len(ph)]
    e_cis = np.abs((c[:, 0] + 1j * c[:, 1]) - fr.cis(ph))
    a = at_t.cpu().numpy().astype(np.float64)[:len(d)]
    d64 = d.astype(np.float64)
    e_atan = np.abs(a - np.arctan2(d64[:, 1], d64[:, 0]))
    print(f"largest |phasor - float64|: {e_cis.max():.4g} at phase {int(ph[e_cis.argmax()]):#x}; EPS_CIS {EPS_CIS:.2g}; "
          f"largest |atan2 - float64|: {e_atan.max():.4g} rad at {d[e_atan.argmax()]}; EPS_ATAN {EPS_ATAN:.2g}")
    assert EPS_CIS < 1e-6 and EPS_ATAN < 1e-6
    assert e_cis.max() <= EPS_CIS and e_atan.max() <= EPS_ATAN
    assert np.array_equal(c[-len(edges):][2::10], np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], np.float64))        # the four quadrant edges, exactly


# ---- 2. exact identities -------------------------------------------------------------------------------------------------------------------------------------
def test_exact_phasors_and_final_phase(engines, torch_dev):
    """m = 0 at fc = Fs / 4: exactly (0, 1), (-1, 0), (0, -1), (1, 0), ..; m = 0 at fc = 0: all (1, 0); phase_end = phase0 + the integer sum of the increments computed
    in numpy, on random input from a non-zero phase0; a stream of no samples keeps its phase"""
    eng = engines(B)
    z = dev(np.zeros((B, NMAXS), np.float32), torch_dev)
    tx, end = eng.fm_mod(z, FS, FS / 4, FD, n=N)
    tx = tx.cpu().numpy()
    four = np.array([1j, -1, -1j, 1], np.complex64)
    for b in range(B):
        assert np.array_equal(tx[b, :N[b]], np.resize(four, N[b])) and np.all(tx[b, N[b]:] == 0)
        assert end[b] == (int(N[b]) << 30) & 0xFFFFFFFF
    tx, end = eng.fm_mod(z, FS, 0.0, FD, n=N)
    assert np.all(tx.cpu().numpy()[:, :N.min()] == 1.0 + 0j) and np.all(end == 0)
    m = np.random.default_rng(41).uniform(-1.5, 1.5, (B, NMAXS)).astype(np.float32)
    ph0 = np.array([0xFFFFFFF0, 12345, 1 << 31], np.uint32)
    n = np.array([N[0], 0, N[2]], np.int32)
    _, end = eng.fm_mod(dev(m, torch_dev), FS, FC, FD, n=n, phase0=ph0)
    for b in range(B):
        want = (int(ph0[b]) + int(fr.nco_inc(m[b, :n[b]], FS, FC, FD).astype(np.uint64).sum())) & 0xFFFFFFFF
        assert end[b] == want, b
    _, end = eng.fm_mod(dev(m, torch_dev), FS, FC, FD, n=0, phase0=ph0)
    assert np.array_equal(end, ph0)


def test_one_tap_filters_pass_the_input_through(engines, torch_dev):
    """fc = 0 and the one-tap tables {1.0f}: bb_out is the input bit for bit (random finite non-zero samples), and the output is the clamped angle of
    x[n] conj(x[n - 1]) over wd, within the atan2 bound"""
    eng = engines(B)
    x = crandn(np.random.default_rng(42), B, NMAXS)
    y, bb, n_out = eng.fm_demod(dev(x, torch_dev), FS, 0.0, FD, [1.0], [1.0], n_in=N, want_bb=True)
    bb, y = bb.cpu().numpy(), y.cpu().numpy()
    for b in range(B):
        assert n_out[b] == N[b] and np.array_equal(bits(bb[b, :N[b]]), bits(x[b, :N[b]])), b
        want, _ = fr.discriminate(x[b, :N[b]].astype(np.complex128), FS, FD)
        assert cmax(y[b, :N[b]] - want) <= (EPS_ATAN + 3 * fr.U) / fr.wd_of(FS, FD)[0] + 2 * fr.U
        assert y[b, 0] == 0.0


# ---- 3. the modulator against the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "c64"])
def test_modulator_against_the_restatement(engines, torch_dev, ref, fmt):
    """two-tone input, float32 and complex64 (random imaginary parts: not used): the integer phases bit-equal to the restatement's, read back through phase_end on
    prefixes that end around every tile edge; the samples within EPS_CIS of the float64 phasor of those phases"""
    eng = engines(B)
    R = ref()
    m = R["m"] if fmt == "f32" else (R["m"] + 1j * np.random.default_rng(43).standard_normal(R["m"].shape)).astype(np.complex64)
    mt = dev(m, torch_dev)
    tx, end = eng.fm_mod(mt, FS, FC, FD, n=N)
    tx = tx.cpu().numpy()
    for b in range(B):
        assert end[b] == R["ph"][b, N[b] - 1], b
        e = cmax(tx[b, :N[b]] - R["tx"][b, :N[b]])
        print(f"{fmt} stream {b}: {N[b]} samples, largest |tx - float64| {e:.3g} (EPS_CIS {EPS_CIS:.2g})")
        assert e <= EPS_CIS
    for k in (1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1):
        n = np.minimum(N, [k, k + 1, max(k - 1, 1)]).astype(np.int32)
        _, end = eng.fm_mod(mt, FS, FC, FD, n=n)
        assert np.array_equal(end, [R["ph"][b, n[b] - 1] for b in range(B)]), k


# ---- 4. the demodulator, stage by stage and end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def demod_run(engines, torch_dev, ref):
    """per (rate, carrier, C/N, clamp): the float32 input (restated modulator plus restated noise, rounded to complex64), the device's outputs and the restatement's;
    computed once and shared"""
    made = {}

    def get(Fs=FS, fc=FC, CN=None, dont_limit=False):
        key = (Fs, fc, CN, dont_limit)
        if key not in made:
            R = ref(Fs, fc)
            x = R["tx"].copy()
            if CN is not None:
                g0, g1 = fr.mod_noise(1000 + int(CN), B, NMAXS)
                x = fr.add_noise(x, g0, g1, fr.sigma(CN, Fs, FM_MAX, FD), fr.OUT_COMPLEX)
            x = x.astype(np.complex64)
            y, bb, n_out = engines(B).fm_demod(dev(x, torch_dev), Fs, fc, FD, R["b1"], R["b2"], n_in=N, ph_dont_limit=dont_limit, want_bb=True)
            assert np.array_equal(n_out, N)
            made[key] = dict(x=x, y=y.cpu().numpy(), bb=bb.cpu().numpy(), ref=[fr.demod(x[b, :N[b]], Fs, fc, FD, R["b1"], R["b2"], dont_limit) for b in range(B)])
        return made[key]
    return get


def test_stage_1_baseband_against_the_restatement(demod_run, ref):
    """bb_out against the float64 mix and input FIR, every sample (the 200-sample start-up included), per component within ((N1 + 2) u + EPS_CIS) sum |b1| max |x|"""
    D, R = demod_run(), ref()
    for b in range(B):
        tol = fr.stage1_bound(R["b1"], cmax(D["x"][b, :N[b]]), EPS_CIS)
        d = D["bb"][b, :N[b]] - D["ref"][b][1]
        e = max(cmax(d.real), cmax(d.imag))
        print(f"stream {b}: largest |bb - bb64| per component {e:.3g}, bound {tol:.3g}")
        assert e <= tol


@pytest.mark.parametrize("dont_limit", [False, True])
def test_stage_2_output_against_the_restatement_on_the_device_baseband(demod_run, ref, dont_limit):
    """the device output against the float64 discriminator and output FIR applied to the device's OWN bb_out: well conditioned for every sample, the start-up included;
    bound (EPS_ATAN + 3 u) / wd sum |b2| + (N2 + 1) u sum |b2|; with the clamp and with ph_dont_limit"""
    D, R = demod_run(dont_limit=dont_limit), ref()
    tol = fr.stage2_bound(R["b2"], FS, FD, EPS_ATAN)
    for b in range(B):
        a, _ = fr.discriminate(D["bb"][b, :N[b]].astype(np.complex128), FS, FD, dont_limit)
        e = cmax(D["y"][b, :N[b]] - fr.causal_fir(R["b2"], a))
        print(f"dont_limit {dont_limit} stream {b}: largest |y - y64(device bb)| {e:.3g}, bound {tol:.3g}; largest |a / wd| {cmax(a):.3g}")
        assert e <= tol
        assert np.all(D["y"][b, N[b]:] == 0)


@pytest.mark.parametrize("Fs,fc,CN", [(48000.0, 12000.0, None), (48000.0, 12000.0, 20.0), (48000.0, 0.0, 30.0), (96000.0, 24000.0, 20.0)])
def test_end_to_end_against_the_restatement(demod_run, ref, Fs, fc, CN):
    """against the full float64 restatement on the same float32 input, on the samples whose whole output window lies where the restatement has |bb| >= 0.5 and
    Re d >= 0.5 |d| (there an error e of bb moves the angle by at most 2 e / 0.5): asserted that at most the first N1 + N2 samples of a stream fall outside.  Bound: the
    stage-1 bound times 2 sum |b2| / (0.5 wd), plus the stage-2 bound."""
    D, R = demod_run(Fs, fc, CN), ref(Fs, fc)
    N1, N2 = len(R["b1"]), len(R["b2"])
    s2 = fr.stage2_bound(R["b2"], Fs, FD, EPS_ATAN)
    for b in range(B):
        y64, bb64, d64 = D["ref"][b]
        tol = fr.stage1_bound(R["b1"], cmax(D["x"][b, :N[b]]), EPS_CIS) * 2 * np.abs(R["b2"]).sum() / (0.5 * fr.wd_of(Fs, FD)[0]) + s2
        good = (np.abs(bb64) >= 0.5) & (np.abs(np.concatenate([[0.0], bb64[:-1]])) >= 0.5) & (d64.real >= 0.5 * np.abs(d64))
        bad = np.flatnonzero(~good)
        last_bad = int(bad[-1]) if bad.size else -1
        use = np.arange(N[b]) >= last_bad + N2                         # the N2 angles of an output's window all lie behind the last bad one
        print(f"Fs {Fs:.0f} fc {fc:.0f} C/N {CN} stream {b}: last sample outside the conditions {last_bad}; behind it min |bb| {np.abs(bb64[last_bad + 1:]).min():.2f}, "
              f"min Re d / |d| {(d64.real / np.abs(d64))[last_bad + 1:].min():.2f}; largest |y - y64| {cmax((D['y'][b, :N[b]] - y64)[use]):.3g}, bound {tol:.3g}")
        assert last_bad + N2 <= N1 + N2 and use.sum() >= N[b] - (N1 + N2)
        assert cmax((D["y"][b, :N[b]] - y64)[use]) <= tol


def test_complex_output_and_folded_deemphasis(engines, torch_dev, ref, demod_run):
    """RADE_FM_C64: the real parts are the float32 output's bits and every imaginary part is +0.0f; the 239-tap table with the de-emphasis folded in (fm_demod_file's
    configuration) against the restatement on the device's own baseband, under the stage-2 bound of that table"""
    eng, R, D = engines(B), ref(), demod_run()
    y, _, _ = eng.fm_demod(dev(D["x"], torch_dev), FS, FC, FD, R["b1"], R["b2"], n_in=N, complex_out=True)
    y = y.cpu().numpy()
    assert np.array_equal(bits(y)[:, 0::2], bits(D["y"])) and np.all(bits(y)[:, 1::2] == 0)
    assert len(R["b2d"]) == 239
    y, bb, _ = eng.fm_demod(dev(D["x"], torch_dev), FS, FC, FD, R["b1"], R["b2d"], n_in=N, want_bb=True)
    y, bb = y.cpu().numpy(), bb.cpu().numpy()
    for b in range(B):
        a, _ = fr.discriminate(bb[b, :N[b]].astype(np.complex128), FS, FD)
        assert cmax(y[b, :N[b]] - fr.causal_fir(R["b2d"], a)) <= fr.stage2_bound(R["b2d"], FS, FD, EPS_ATAN)


# ---- 5. noise ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [fr.OUT_COMPLEX, fr.OUT_REAL])
def test_generated_noise_against_the_reference(engines, torch_dev, ref, mode):
    """counter (p, b, 3, 0), p = (n0 + i) >> 1, words 0-1 for the even sample of a pair and 2-3 for the odd one: the noisy output minus the device's own noise-free
    output against sigma x the reference noise, sample by sample within sigma EPS (tests/test_device_noise_gpu.py) plus the two float32 roundings of tx + s g; from an even and an odd n0.
    Real mode: (Re tx + sigma g0, +0)"""
    eng, R = engines(B), ref()
    mt = dev(R["m"], torch_dev)
    sig, seed = 0.25, 0x1234567890
    clean, _ = eng.fm_mod(mt, FS, FC, FD, n=N, real=mode == fr.OUT_REAL)
    clean = clean.cpu().numpy()
    for n0 in (0, 1001):
        y, _ = eng.fm_mod(mt, FS, FC, FD, n=N, real=mode == fr.OUT_REAL, sigma=sig, seed=seed, n0=n0)
        y = y.cpu().numpy()
        g0, g1 = fr.mod_noise(seed, B, NMAXS, n0)
        want = fr.add_noise(np.zeros((B, NMAXS), np.complex128), g0, g1, sig, mode)
        for b in range(B):
            d = (y[b, :N[b]].astype(np.complex128) - clean[b, :N[b]]) - want[b, :N[b]]
            e = max(cmax(d.real), cmax(d.imag))
            print(f"mode {mode} n0 {n0} stream {b}: largest deviation from sigma x reference noise {e:.3g}")
            w, yy = want[b, :N[b]], y[b, :N[b]]                         # y = fl(tx + fl(s g)): the product's rounding u |s g|, the sum's u |y|, per component
            tol = sig * NOISE_EPS + fr.U * (np.maximum(np.abs(w.real), np.abs(w.imag)) + np.maximum(np.abs(yy.real), np.abs(yy.imag)))
            assert np.all(np.maximum(np.abs(d.real), np.abs(d.imag)) <= tol)
            if mode == fr.OUT_REAL:
                assert np.all(bits(y[b])[1::2] == 0)
        assert abs(np.std(y[0, :N[0]].real - clean[0, :N[0]].real) / (sig * (1.0 if mode == fr.OUT_REAL else np.sqrt(0.5))) - 1) < 0.05


def test_explicit_noise_and_streams_alone(engines, torch_dev, ref):
    """an explicit noise tensor: bit-equal to tx + float32(sigma) x noise added by hand in float32 (the real part only in real mode); every stream of the batch equals
    the same stream modulated alone; with generated noise stream 0 equals itself alone (the counter carries the stream's index)"""
    eng, one, R = engines(B), engines(1), ref()
    mt = dev(R["m"], torch_dev)
    nz = crandn(np.random.default_rng(44), B, NMAXS)
    sig = np.float32(0.3)
    clean = eng.fm_mod(mt, FS, FC, FD, n=N)[0].cpu().numpy()
    y = eng.fm_mod(mt, FS, FC, FD, n=N, sigma=float(sig), noise=dev(nz, torch_dev))[0].cpu().numpy()
    yr = eng.fm_mod(mt, FS, FC, FD, n=N, sigma=float(sig), noise=dev(nz, torch_dev), real=True)[0].cpu().numpy()
    for b in range(B):
        k = N[b]
        hand, hand_r = np.zeros(k, np.complex64), np.zeros(k, np.complex64)
        hand.real = clean[b, :k].real + sig * nz[b, :k].real
        hand.imag = clean[b, :k].imag + sig * nz[b, :k].imag
        hand_r.real = hand.real
        assert (sig * nz[b, :k].real).dtype == np.float32 and np.array_equal(bits(y[b, :k]), bits(hand)), b
        assert np.array_equal(bits(yr[b, :k]), bits(hand_r)), b
        alone = one.fm_mod(mt[b:b + 1], FS, FC, FD, n=int(k), sigma=float(sig), noise=dev(nz[b:b + 1], torch_dev))[0].cpu().numpy()
        assert np.array_equal(bits(alone[0, :k]), bits(y[b, :k])), b
    g = eng.fm_mod(mt, FS, FC, FD, n=N, sigma=0.3, seed=9)[0].cpu().numpy()
    alone = one.fm_mod(mt[:1], FS, FC, FD, n=int(N[0]), sigma=0.3, seed=9)[0].cpu().numpy()
    assert np.array_equal(bits(alone[0, :N[0]]), bits(g[0, :N[0]]))


# ---- 6. pieces equal the whole -------------------------------------------------------------------------------------------------------------------------------
CUTS = [1, 17, TILE, TILE + 1]


def test_modulator_in_pieces(engines, torch_dev, ref):
    """the modulator with generated noise, cut at 1, 17, a tile edge and a tile edge + 1 (pieces of 1, 16, TILE - 17, 1 and the rest), each piece given the phase the
    previous one ended on and its absolute index: bit-equal to the whole; also through FmModulator"""
    from radae_amd.engine import FmModulator
    eng, R = engines(B), ref()
    n = int(N.min())
    mt = dev(R["m"][:, :n], torch_dev)
    whole, end = eng.fm_mod(mt, FS, FC, FD, sigma=0.2, seed=77)
    whole = whole.cpu().numpy()
    edges = [0] + CUTS + [n]
    parts, ph = [], np.zeros(B, np.uint32)
    fm = FmModulator(eng, FS, FC, FD, sigma=0.2, seed=77)
    helper = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        y, ph = eng.fm_mod(mt[:, lo:hi].contiguous(), FS, FC, FD, sigma=0.2, seed=77, phase0=ph, n0=lo)
        parts.append(y.cpu().numpy())
        helper.append(fm.feed(mt[:, lo:hi].contiguous()).cpu().numpy())
    assert np.array_equal(ph, end) and np.array_equal(fm.phase, end)
    assert np.array_equal(bits(np.concatenate(parts, axis=1)), bits(whole))
    assert np.array_equal(bits(np.concatenate(helper, axis=1)), bits(whole))


def test_demodulator_in_pieces(engines, torch_dev, ref, demod_run):
    """the demodulator cut at 1, 17, a tile edge and a tile edge + 1: each piece handed the N1 + N2 - 1 samples in front of it (through in_base / n0) is bit-equal to
    the whole, output and baseband; through FmDemodulator as well; and a piece handed ONE sample less history differs (the test can fail)"""
    from radae_amd.engine import FmDemodulator
    eng, R, D = engines(B), ref(), demod_run(CN=20.0)
    n = int(N.min())
    H = len(R["b1"]) + len(R["b2"]) - 1
    x = D["x"][:, :n]
    whole_y, whole_bb = D["y"][:, :n], D["bb"][:, :n]
    edges = [0] + CUTS + [n]
    ys, bbs, hy = [], [], []
    fmd = FmDemodulator(eng, FS, FC, FD, R["b1"], R["b2"])
    for lo, hi in zip(edges[:-1], edges[1:]):
        base = max(lo - H, 0)
        y, bb, n_out = eng.fm_demod(dev(x[:, base:hi], torch_dev), FS, FC, FD, R["b1"], R["b2"], in_base=base, n0=lo, n_out=hi - lo, want_bb=True)
        assert np.all(n_out == hi - lo)
        ys.append(y.cpu().numpy()); bbs.append(bb.cpu().numpy())
        hy.append(fmd.feed(dev(x[:, lo:hi], torch_dev))[0].cpu().numpy())
    assert np.array_equal(bits(np.concatenate(ys, axis=1)), bits(whole_y))
    assert np.array_equal(bits(np.concatenate(bbs, axis=1)), bits(whole_bb))
    assert np.array_equal(bits(np.concatenate(hy, axis=1)), bits(whole_y))
    lo, hi = TILE + 1, n
    y, _, _ = eng.fm_demod(dev(x[:, lo - H + 1:hi], torch_dev), FS, FC, FD, R["b1"], R["b2"], in_base=lo - H + 1, n0=lo, n_out=hi - lo)
    y = y.cpu().numpy()
    assert not np.array_equal(bits(y[:, 0]), bits(whole_y[:, lo])) and np.array_equal(bits(y[:, 1:]), bits(whole_y[:, lo + 1:]))


# ---- 7. the buffer contract ------------------------------------------------------------------------------------------------------------------------------------
def test_buffer_contract_of_the_modulator(engines, torch_dev, ref):
    """sentinel buffers at odd strides and odd element offsets, unequal counts with a zero among them, both input formats and explicit noise: the inputs untouched,
    exactly n[b] samples of each row written and nothing else; equal to the plain call's bits"""
    import torch
    eng, R = engines(B), ref()
    n = np.array([N[0], 0, TILE + 3], np.int32)
    row = int(n.max())
    want = eng.fm_mod(dev(R["m"][:, :row], torch_dev), FS, FC, FD, n=n, sigma=0.1, seed=5)[0].cpu().numpy()
    for fmt, data, eb, off in ((fr.F32, R["m"][:, :row], 4, 4), (fr.C64, (R["m"][:, :row] + 2j).astype(np.complex64), 8, 8)):
        min_ = Band(B, row, row + 3, eb, torch_dev, base_offset_bytes=off).fill(data)
        snap = min_.host().copy()
        out = Band(B, row, row + 1 + (row % 2), 8, torch_dev, base_offset_bytes=8)
        assert raw_mod(eng, min_.ptr, min_.stride, n, out.ptr, out.stride, fmt=fmt, sigma=0.1, seed=5) == 0
        torch.cuda.synchronize()
        out.check(written=n, what=f"tx, input format {fmt}")
        got = out.rows(np.complex64)
        for b in range(B):
            assert np.array_equal(bits(got[b, :n[b]]), bits(want[b, :n[b]])), (fmt, b)
        assert np.array_equal(min_.host(), snap), "the input was written"


def test_buffer_contract_of_the_demodulator(engines, torch_dev, ref, demod_run):
    """the same for the demodulator, float32 and complex64 outputs and bb_out: odd strides, odd element offsets, unequal counts, a zero count, n0 behind in_base"""
    import torch
    eng, R, D = engines(B), ref(), demod_run()
    n_in = np.array([N[0], 0, TILE + 3], np.int32)
    n_out = np.array([N[0] - 5, 0, TILE + 3 - 5], np.int32)
    row = int(n_in.max())
    xin = Band(B, row, row + 1 + (row % 2), 8, torch_dev, base_offset_bytes=8).fill(D["x"][:, :row])
    snap = xin.host().copy()
    for fmt, eb in ((fr.F32, 4), (fr.C64, 8)):
        out = Band(B, row, row + 3, eb, torch_dev, base_offset_bytes=eb)
        bb = Band(B, row, row + 5, 8, torch_dev, base_offset_bytes=8)
        assert raw_demod(eng, xin.ptr, xin.stride, n_in, out.ptr, out.stride, n_out, R["b1"], R["b2"], fmt=fmt, in_base=10, n0=15, bb_ptr=bb.ptr, bb_stride=bb.stride) == 0
        torch.cuda.synchronize()
        out.check(written=n_out, what=f"y, output format {fmt}")
        bb.check(written=n_out, what="bb_out")
        assert np.array_equal(xin.host(), snap), "the input was written"
    y = out.rows(np.complex64)
    want, _, _ = eng.fm_demod(dev(D["x"][:, :row], torch_dev), FS, FC, FD, R["b1"], R["b2"], n_in=n_in, in_base=10, n0=15, n_out=n_out)
    want = want.cpu().numpy()
    for b in (0, 2):
        assert np.array_equal(bits(y[b, :n_out[b]].real.copy()), bits(want[b, :n_out[b]])) and np.all(bits(y[b, :n_out[b]])[1::2] == 0)


# ---- 8. refusals, and other taps between calls --------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engines, torch_dev, ref):
    """argument checking on the host: each of these returns -1 before any launch, and the output buffers still hold their sentinel"""
    import torch
    eng, R = engines(B), ref()
    n = 600
    nan, inf = float("nan"), float("inf")
    min_ = Band(B, n, n + 1, 8, torch_dev).fill(crandn(np.random.default_rng(45), B, n))
    out = Band(B, n, n + 1, 8, torch_dev)
    bb = Band(B, n, n + 1, 8, torch_dev)
    ok = dict(m_ptr=min_.ptr, m_stride=n + 1, n=n, y_ptr=out.ptr, y_stride=n + 1, fmt=fr.C64)
    f32 = dict(fmt=fr.F32, m_stride=2 * (n + 1))                          # the same bytes read as float32 rows
    bad = [dict(m_ptr=0), dict(y_ptr=0), dict(m_ptr=min_.ptr + 4), dict(y_ptr=out.ptr + 4), dict(f32, m_ptr=min_.ptr + 2), dict(n=(n, -1, n)), dict(m_stride=n - 1),
           dict(y_stride=n - 1), dict(fmt=2), dict(fmt=-1), dict(mode=2), dict(mode=-1), dict(Fs=0.0), dict(Fs=-48000.0), dict(Fs=nan), dict(fc=FS / 2 + 1), dict(fc=-FS / 2 - 1),
           dict(fc=nan), dict(fd=0.0), dict(fd=-1.0), dict(fd=FS / 2 + 1), dict(fd=nan), dict(sigma=-0.1, seed=1), dict(sigma=nan, seed=1), dict(sigma=inf, seed=1),
           dict(sigma=0.1), dict(sigma=0.1, noise_ptr=min_.ptr + 4), dict(sigma=0.1, seed=1, n0=(0, -1, 0)), dict(n0=-1)]
    for kw in bad:
        assert raw_mod(eng, **{**ok, **kw}) == -1, kw
    x = dict(x_ptr=min_.ptr, x_stride=n + 1, n_in=n, y_ptr=out.ptr, y_stride=n + 1, n_out=n, b1=R["b1"], b2=R["b2"], fmt=fr.C64, bb_ptr=bb.ptr, bb_stride=n + 1)
    t_nan = R["b1"].copy(); t_nan[100] = nan
    t_inf = R["b2"].copy(); t_inf[0] = inf
    badd = [dict(x_ptr=0), dict(y_ptr=0), dict(x_ptr=min_.ptr + 4), dict(y_ptr=out.ptr + 4), dict(fmt=fr.F32, y_ptr=out.ptr + 2), dict(bb_ptr=bb.ptr + 4), dict(n_in=(n, -1, n)),
            dict(n_out=(n, n, -1)), dict(x_stride=n - 1), dict(y_stride=n - 1), dict(bb_stride=n - 1), dict(fmt=2), dict(fmt=-1), dict(Fs=0.0), dict(Fs=nan), dict(fc=FS),
            dict(fc=-FS), dict(fd=0.0), dict(fd=FS), dict(b1=None), dict(b2=None), dict(N1=0), dict(N2=0), dict(N1=NMAX + 1), dict(N2=NMAX + 1), dict(N1=-1), dict(b1=t_nan),
            dict(b2=t_inf), dict(in_base=(1 << 62) + 1), dict(in_base=-(1 << 62) - 1), dict(n0=(1 << 62) + 1)]
    for kw in badd:
        assert raw_demod(eng, **{**x, **kw}) == -1, kw
    torch.cuda.synchronize()
    out.untouched("the outputs of the refused calls")
    bb.untouched("bb_out of the refused calls")
    for kw in (dict(), f32, dict(f32, m_ptr=min_.ptr + 4), dict(mode=fr.OUT_REAL, fc=0.0), dict(fc=FS / 2), dict(fc=-FS / 2), dict(fd=FS / 2), dict(sigma=0.1, seed=1),
               dict(sigma=0.1, noise_ptr=bb.ptr), dict(sigma=0.0, n0=1 << 62)):
        assert raw_mod(eng, **{**ok, **kw}) == 0, kw                      # ... and the same arguments without the fault are accepted
    big = np.resize(R["b2"], NMAX).astype(np.float32)
    for kw in (dict(), dict(fmt=fr.F32), dict(fmt=fr.F32, y_ptr=out.ptr + 4), dict(b1=big, b2=big), dict(b1=[1.0], b2=[1.0]), dict(in_base=1 << 62), dict(in_base=-(1 << 62)),
               dict(bb_ptr=None)):
        assert raw_demod(eng, **{**x, **kw}) == 0, kw
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        eng.fm_mod(dev(np.zeros((B, 8), np.float32), torch_dev), FS, FS, FD)
    with pytest.raises(RuntimeError):
        eng.fm_demod(dev(np.zeros((B, 8), np.complex64), torch_dev), FS, FC, FD, np.zeros(NMAX + 1), [1.0])


def test_changing_the_taps_between_calls(engines, torch_dev, ref, demod_run):
    """the shipped tables, then other bytes of the same lengths, then other lengths, then the shipped tables again: every call uses the tables it was given (the copy in
    engine memory follows the bytes), and the last call gives the first one's bits"""
    eng, R, D = engines(B), ref(), demod_run()
    xt = dev(D["x"], torch_dev)
    run = lambda b1, b2: eng.fm_demod(xt, FS, FC, FD, b1, b2, n_in=N, want_bb=True)
    first = [v.cpu().numpy() for v in run(R["b1"], R["b2"])[:2]]
    assert np.array_equal(bits(first[0]), bits(D["y"]))
    other = [v.cpu().numpy() for v in run(R["b1"] * np.float32(0.5), R["b2"])[:2]]
    assert np.array_equal(bits(other[1]), bits(first[1] * np.float32(0.5)))               # halved taps: every product and sum halves exactly
    y1, bb1, _ = run([1.0], [1.0])
    a, _ = fr.discriminate(bb1.cpu().numpy()[0, :N[0]].astype(np.complex128), FS, FD)
    assert cmax(y1.cpu().numpy()[0, :N[0]] - a) <= (EPS_ATAN + 3 * fr.U) / fr.wd_of(FS, FD)[0] + 2 * fr.U
    again = [v.cpu().numpy() for v in run(R["b1"], R["b2"])[:2]]
    assert np.array_equal(bits(again[0]), bits(first[0])) and np.array_equal(bits(again[1]), bits(first[1]))


# ---- 9. the command line: analog_bbfm.sh:37-43 on the device ---------------------------------------------------------------------------------------------------
def test_cli_analog_fm_against_the_float64_chain(tmp_path):
    """0.5 s of a 1 kHz tone (8 kHz int16) through `cli analog_fm` at C/N 30 dB: the tone SNR of the 8 kHz int16 output (the notch measurement of fm.m:180-192 at 8 kHz)
    lies within 1 dB of the same chain on the float64 restatements: tests/rate_ref.py up, fm_ref.mod with the reference's real noise, int16 x 16384 (tests/wire_ref.py),
    fm_ref.demod with the folded de-emphasis, rate_ref down, int16 x 20000"""
    import rate_ref as rf
    import wire_ref as wr
    from radae_amd import cli
    from radae_amd.engine import fm_sigma, fm_taps, rate_taps
    n, CN, seed = 4000, 30.0, 1
    x16 = np.round(16000.0 * np.sin(2 * np.pi * 1000.0 / 8000.0 * np.arange(n))).astype(np.int16)
    src, dst = tmp_path / "in.s16", tmp_path / "out.s16"
    x16.tofile(src)
    assert cli.main(["analog_fm", str(src), str(dst), str(CN), "--seed", str(seed)]) == 0
    got = np.fromfile(dst, np.int16)
    assert got.shape == (n,)
    up, _ = rf.convert(x16, 6 * n, 6, 1, C=rate_taps(6, 1), fmt=rf.S16_REAL, gain=1.0 / 32767.0)
    tx, _ = fr.mod(up.real.astype(np.float32), 48000.0, 12000.0, FD)
    g0, g1 = fr.mod_noise(seed, 1, 6 * n)
    air = fr.add_noise(tx, g0[0], g1[0], fm_sigma(CN, 48000.0, FM_MAX, FD), fr.OUT_REAL)
    card, _ = wr.c64_to_int16(air.astype(np.complex64), scale=16384.0, real=True)
    b1, b2 = (v.astype(np.float32) for v in fm_taps(48000.0, FM_MAX, FD, 201, fr.TC))
    y, _, _ = fr.demod(card.astype(np.float64) + 0j, 48000.0, 12000.0, FD, b1, b2)
    down, _ = rf.convert(y.astype(np.complex64), n, 1, 6, C=rate_taps(1, 6))
    want, _ = wr.c64_to_int16(down.astype(np.complex64), scale=20000.0, real=True)
    snr_dev, snr_ref = fr.tone_snr_dB(got.astype(np.float64), 8000.0), fr.tone_snr_dB(want.astype(np.float64), 8000.0)
    print(f"tone SNR at 8 kHz: device chain {snr_dev:.2f} dB, float64 chain {snr_ref:.2f} dB; largest difference of the int16 outputs {np.abs(got.astype(int) - want).max()}")
    assert snr_ref > 20.0 and abs(snr_dev - snr_ref) <= 1.0
