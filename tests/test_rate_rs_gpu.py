"""GPU tests (-m gpu) of the rate-Rs channel of the bottleneck-3 model (rade_batch_channel_rs_pa, rade_rs.hip; radae.py:603-634): against the reference's
recordings (tests/golden/rate_rs_bn3.npz) and against the float64 restatement of tests/rate_rs_ref.py on fresh inputs.  The bar on z_hat is the project's for
latents: max |delta| <= 2e-5 of the full scale max |z_hat| of the compared streams.  Explicit noise throughout; the generated noise is only checked for its
statistics and for being keyed by (seed, stream)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rate_rs_ref as rs
from bands import Band
from gpu_kit import REPO, Engine, dev, engines, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def random_inputs(B, n, seed):
    """latents that fill the amplifier (N(0, 25^2): |tx| ~ 1 before the limiter), Rayleigh magnitudes, unit-variance complex noise"""
    rng = np.random.default_rng(seed)
    z = (25.0 * rng.standard_normal((B, n, 80))).astype(np.float32)
    H = np.abs((rng.standard_normal((B, 2 * n, 20)) + 1j * rng.standard_normal((B, 2 * n, 20))) / np.sqrt(2)).astype(np.float32)
    noise = ((rng.standard_normal((B, 2 * n, 20)) + 1j * rng.standard_normal((B, 2 * n, 20))) / np.sqrt(2)).astype(np.complex64)
    return z, H, noise


@pytest.mark.parametrize("case", rs.CASES)
def test_fixture_cases(engines, torch_dev, golden, case):
    """the reference's recordings: z_hat within the bar; the zero symbol of the edge case comes out as sigma x noise exactly and the 1e4 symbol finite"""
    g = golden("rate_rs_bn3")
    z, H, noise, sigma, ph = rs.fixture_case(g, case)
    zh = engines(1).channel_rs_pa(dev(z[None], torch_dev), sigma, H=dev(None if H is None else H[None], torch_dev), noise=dev(noise[None], torch_dev),
                                  phase_offset=ph).cpu().numpy()[0]
    ref = g[case + "_z_hat"]
    full = np.abs(ref).max()
    err = np.abs(zh - ref).max()
    print(f"{case}: max |dz_hat| {err:.3g} = {err / full:.3g} of full scale {full:.3g}")
    assert np.isfinite(zh).all()
    assert err <= rs.BAR * full
    if case == "edge":
        s5 = zh.reshape(24, 20, 2)[5]
        assert np.array_equal(s5[:, 0], np.float32(sigma) * noise[5].real) and np.array_equal(s5[:, 1], np.float32(sigma) * noise[5].imag)


@pytest.mark.parametrize("B,n", [(3, 1), (3, 3), (3, 7), (3, 12), (1, 12), (1, 5)])
def test_fresh_inputs_against_the_restatement(engines, torch_dev, B, n):
    """2 n symbols per stream against tiles of 8: 2, 6, 14, 24 (and 10) leave a tile partly filled or fill it exactly; per-stream sigma, H and a phase offset"""
    z, H, noise = random_inputs(B, n, 1000 + 16 * B + n)
    sigma = rs.sigma_rs3(np.float32([3.0, -6.0, 10.0])[:B]).astype(np.float32)
    zh, st = engines(B).channel_rs_pa(dev(z, torch_dev), sigma if B > 1 else float(sigma[0]), H=dev(H, torch_dev), noise=dev(noise, torch_dev), phase_offset=-0.7,
                                      want_stats=True)
    zh = zh.cpu().numpy()
    r = rs.channel(z, H, noise, sigma.astype(np.float64), -0.7)
    for b in range(B):
        full = np.abs(r["z_hat"][b]).max()
        err = np.abs(zh[b] - r["z_hat"][b]).max()
        print(f"B {B} n {n} stream {b}: max |dz_hat| {err:.3g} = {err / full:.3g} of full scale {full:.3g}")
        assert err <= rs.BAR * full
    # without H, noise or phase offset the call is the bare IDFT - limiter - DFT
    bare = engines(B).channel_rs_pa(dev(z, torch_dev), 0.0).cpu().numpy()
    rb = rs.channel(z, None, None, 0.0)["z_hat"]
    assert np.abs(bare - rb).max() <= rs.BAR * np.abs(rb).max()
    # inference.py's measurements: two decimals are printed; 0.005 dB is far above the float32 rounding of the terms
    want = rs.measured_dB(r["stats"], sigma.astype(np.float64), n)
    got = rs.measured_dB(st, sigma.astype(np.float64), n)
    print("Eq/No dB", got[0], want[0], "PAPR dB", got[1], want[1])
    assert np.abs(got[0] - want[0]).max() <= 0.005 and np.abs(got[1] - want[1]).max() <= 0.005


def test_two_calls_are_bit_identical(engines, torch_dev):
    z, H, noise = random_inputs(3, 12, 77)
    zt, Ht, nt = dev(z, torch_dev), dev(H, torch_dev), dev(noise, torch_dev)
    a, sa = engines(3).channel_rs_pa(zt, 12.66, H=Ht, noise=nt, phase_offset=0.3, want_stats=True)
    b, sb = engines(3).channel_rs_pa(zt, 12.66, H=Ht, noise=nt, phase_offset=0.3, want_stats=True)
    assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    assert np.array_equal(sa.view(np.int64), sb.view(np.int64)) and np.all(sa > 0)
    # generated noise too: the same seed gives the same bits, another seed other bits
    g1 = engines(3).channel_rs_pa(zt, 12.66, seed=5).cpu().numpy()
    g2 = engines(3).channel_rs_pa(zt, 12.66, seed=5).cpu().numpy()
    g3 = engines(3).channel_rs_pa(zt, 12.66, seed=6).cpu().numpy()
    assert np.array_equal(g1.view(np.int32), g2.view(np.int32)) and not np.array_equal(g1, g3)


def test_per_stream_sigma_equals_the_scalar_calls(engines, torch_dev):
    """the rule of rade_channel_streams: stream b of a per-stream call is what the scalar call with its value gives, bit for bit; no array = the scalar call"""
    z, H, noise = random_inputs(3, 7, 78)
    zt, Ht, nt = dev(z, torch_dev), dev(H, torch_dev), dev(noise, torch_dev)
    eng = engines(3)
    sig = np.float32([12.66, 35.7, 0.25])
    per = eng.channel_rs_pa(zt, sig, H=Ht, noise=nt).cpu().numpy().view(np.int32)
    for b in range(3):
        one = eng.channel_rs_pa(zt, float(sig[b]), H=Ht, noise=nt).cpu().numpy().view(np.int32)
        assert np.array_equal(per[b], one[b]), b
    same = eng.channel_rs_pa(zt, np.float32([0.25, 0.25, 0.25]), H=Ht, noise=nt).cpu().numpy().view(np.int32)
    assert np.array_equal(same, eng.channel_rs_pa(zt, 0.25, H=Ht, noise=nt).cpu().numpy().view(np.int32))
    # generated noise: keyed by (seed, stream), scaled per stream
    gp = eng.channel_rs_pa(zt, sig, seed=9).cpu().numpy().view(np.int32)
    for b in range(3):
        assert np.array_equal(gp[b], eng.channel_rs_pa(zt, float(sig[b]), seed=9).cpu().numpy().view(np.int32)[b]), b


def test_generated_noise(engines, torch_dev):
    """z = 0 leaves sigma x noise: finite, zero mean, 1/2 per component (unit variance in total) over 3 x 80,000 complex samples, streams differ, and stream 0 of a
    batch of three is stream 0 of a batch of one.  Bounds: five standard deviations of the sample mean (s / sqrt N) and of the sample variance (s^2 sqrt(2 / N))."""
    import torch
    n = 2000                                                     # 80,000 complex samples per stream
    sigma = 2.0
    z3 = torch.zeros((3, n, 80), device=torch_dev)
    a = engines(3).channel_rs_pa(z3, sigma, seed=1234).cpu().numpy()
    assert np.isfinite(a).all()
    x = a.reshape(3, -1, 2).astype(np.float64) / sigma
    N = x.shape[0] * x.shape[1]
    assert N >= 100000
    for comp in range(2):
        v = x[..., comp].ravel()
        assert abs(v.mean()) <= 5 * np.sqrt(0.5 / N), v.mean()
        assert abs(v.var() - 0.5) <= 5 * 0.5 * np.sqrt(2.0 / N), v.var()
    assert abs(np.mean(x[..., 0] * x[..., 1])) <= 5 * 0.5 / np.sqrt(N)              # the two components are uncorrelated
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    one = engines(1).channel_rs_pa(z3[:1].contiguous(), sigma, seed=1234).cpu().numpy()
    assert np.array_equal(one[0].view(np.int32), a[0].view(np.int32))
    assert np.all(engines(1).channel_rs_pa(z3[:1].contiguous(), sigma, seed=0).cpu().numpy() == 0.0)       # seed 0: no noise


def test_buffer_contract(engines, torch_dev):
    """the dense buffers of the call at the smallest offsets the header allows (one element past a 16-byte boundary): guards around z_hat untouched, every float of it
    written, inputs untouched, the same bits as the aligned call; a pointer that is not element-aligned is refused on the host with nothing written"""
    from radae_amd.engine import _stream_ptr
    B, n = 3, 7
    eng = engines(B)
    z, H, noise = random_inputs(B, n, 79)
    sig = np.float32([12.66, 3.0, 0.5])
    want = eng.channel_rs_pa(dev(z, torch_dev), sig, H=dev(H, torch_dev), noise=dev(noise, torch_dev), phase_offset=0.3).cpu().numpy().view(np.int32)
    ins = [Band(1, z.size, z.size, 4, torch_dev, base_offset_bytes=4).fill(z.reshape(1, -1)), Band(1, H.size, H.size, 4, torch_dev, base_offset_bytes=12).fill(H.reshape(1, -1)),
           Band(1, noise.size, noise.size, 8, torch_dev, base_offset_bytes=8).fill(noise.reshape(1, -1))]
    snaps = [bd.host().copy() for bd in ins]
    out = Band(1, z.size, z.size, 4, torch_dev, base_offset_bytes=4)
    stats = np.zeros((B, 3), np.float64)
    L, vp = eng.lib, C.c_void_p
    r = L.rade_batch_channel_rs_pa(eng.h, vp(ins[0].ptr), vp(ins[1].ptr), vp(ins[2].ptr), vp(out.ptr), n, 0.0, sig.ctypes.data, 0.3, 0, stats.ctypes.data, _stream_ptr())
    assert r == n
    out.check(what="z_hat")
    assert np.array_equal(out.rows().reshape(want.shape), want)
    for bd, snap in zip(ins, snaps):
        assert np.array_equal(bd.host(), snap), "an input buffer was written"
    assert np.all(stats[:, 0] > 0) and np.all(stats[:, 1] <= 1.0)
    fresh = Band(1, z.size, z.size, 4, torch_dev, base_offset_bytes=4)
    for bad in ((ins[0].ptr + 2, ins[2].ptr, fresh.ptr), (ins[0].ptr, ins[2].ptr + 4, fresh.ptr), (ins[0].ptr, ins[2].ptr, fresh.ptr + 1)):
        assert L.rade_batch_channel_rs_pa(eng.h, vp(bad[0]), vp(ins[1].ptr), vp(bad[1]), vp(bad[2]), n, 0.0, sig.ctypes.data, 0.3, 0, None, _stream_ptr()) < 0
    assert L.rade_batch_channel_rs_pa(eng.h, vp(ins[0].ptr), None, None, vp(fresh.ptr), 0, 1.0, None, 0.0, 0, None, _stream_ptr()) < 0       # n_steps >= 1
    import torch
    torch.cuda.synchronize()
    fresh.untouched("z_hat of the refused calls")


def test_model19_rate_rs_composition(Engine, torch_dev, oracle, oracle_model):
    """Modelled on test_model05_rate_rs_config1, on model19_check3.  Chain against chain: oracle encoder -> restatement -> oracle decoder versus encode ->
    rade_batch_channel_rs_pa -> decode, features within that test's 2e-5 RMS (measured 7e-7).  And, as that test does, each stage against its reference on the
    reference's input: latents and z_hat within 2e-5 of full scale, the decoder on the restatement's z_hat within the same 2e-5 RMS."""
    import torch
    from radae_amd.channel_tools import synth_features
    rms = lambda a, b: float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
    n_mf = 4
    T = 3 * n_mf
    f = synth_features(99, 12 * n_mf)[:, :21].copy(); f[:, 20] = -1.0
    x = np.ascontiguousarray(f.reshape(T, 84))
    enc, dec = oracle.Encoder(oracle_model), oracle.Decoder(oracle_model)
    z_ref = np.stack([enc.step(r) for r in x])
    rng = np.random.default_rng(5)
    H = np.abs((rng.standard_normal((2 * T, 20)) + 1j * rng.standard_normal((2 * T, 20))) / np.sqrt(2)).astype(np.float32)
    noise = ((rng.standard_normal((2 * T, 20)) + 1j * rng.standard_normal((2 * T, 20))) / np.sqrt(2)).astype(np.complex64)
    sigma = float(rs.sigma_rs3(3.0))
    zh_ref = rs.channel(z_ref, H, noise, sigma)["z_hat"].astype(np.float32)
    fh_ref = np.stack([dec.step(r) for r in zh_ref])
    eng = Engine(1, max_tx_mf=n_mf)
    z = eng.encode(dev(x[None], torch_dev))
    chain = eng.decode(eng.channel_rs_pa(z, sigma, H=dev(H[None], torch_dev), noise=dev(noise[None], torch_dev)), 84).cpu().numpy()[0]
    print(f"encode -> channel -> decode against oracle -> restatement -> oracle: rms {rms(chain, fh_ref):.3g}, |tx_sym| rms {np.sqrt(np.mean(z_ref ** 2) * 2):.3g}")
    assert np.isfinite(chain).all() and rms(chain, fh_ref) < 2e-5
    assert np.abs(z.cpu().numpy()[0] - z_ref).max() <= rs.BAR * np.abs(z_ref).max()
    zh = eng.channel_rs_pa(dev(z_ref[None], torch_dev), sigma, H=dev(H[None], torch_dev), noise=dev(noise[None], torch_dev))
    assert np.abs(zh.cpu().numpy()[0] - zh_ref).max() <= rs.BAR * np.abs(zh_ref).max()
    fh = eng.decode(dev(zh_ref[None], torch_dev), 84).cpu().numpy()[0]
    print(f"decoder on the restatement's z_hat: rms {rms(fh, fh_ref):.3g}")
    assert rms(fh, fh_ref) < 2e-5
    eng.close()


def test_limiter_at_any_finite_size(engines, torch_dev):
    """latents of 1e25 (|tx| up to 1e24: its square is past float32) and of 1e-12 beside ordinary ones: every output finite; the huge symbols come out of the amplifier at
    magnitude 1 on every sample (sum |tx'|^2 = 160 per symbol, max 1), so their |Y| <= 160; the tiny ones pass in the linear region (the restatement's z_hat, which is z)"""
    z, _, _ = random_inputs(3, 4, 80)
    z[0] = np.float32(1e25) * np.sign(z[0])
    z[1] = np.float32(1e-12) * z[1] / 25
    zh, st = engines(3).channel_rs_pa(dev(z, torch_dev), 0.0, want_stats=True)
    zh = zh.cpu().numpy()
    assert np.isfinite(zh).all() and np.isfinite(st).all()
    assert abs(st[0, 0] - 8 * 160) <= 1e-4 * 8 * 160 and abs(st[0, 1] - 1.0) <= 1e-6 and np.abs(zh[0]).max() <= 160.0 * (1 + 1e-6)
    for b in (1, 2):
        r = rs.channel(z[b], None, None, 0.0)["z_hat"]
        assert np.abs(zh[b] - r).max() <= rs.BAR * np.abs(r).max(), b
    assert np.abs(zh[1] - z[1]).max() <= 1e-3 * np.abs(z[1]).max()      # linear region: the two transforms undo each other (to the reference's twiddle errors)


def _cli(tmp_path, n_frames):
    from radae_amd.channel_tools import synth_features
    env = dict(os.environ); env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    synth_features(4242, n_frames).tofile(str(tmp_path / "features_in.f32"))
    blob = os.path.join(REPO, "weights", "model19_check3.bin")

    def run(args, ok=True):
        r = subprocess.run([sys.executable, "-m", "radae_amd.cli", "inference", blob, "features_in.f32"] + args + ["--bottleneck", "3", "--auxdata"], capture_output=True,
                           cwd=str(tmp_path), env=env, timeout=300)
        assert (r.returncode == 0) == ok, r.stderr.decode()[-1500:]
        print(r.stdout.decode())
        return r.stdout.decode() + r.stderr.decode()
    return run


def _loss(o):
    return float([l for l in o.splitlines() if l.startswith("loss:")][0].split()[1])


def _measured(o):
    """Eq/No - 3 dB, SNR3k, Eq, PAPR of the Measured: line"""
    m = [l for l in o.splitlines() if l.startswith("Measured:")][0].split()
    assert len(m) == 5
    return [float(v) for v in m[1:]]


def test_cli_inference_rate_rs(tmp_path):
    """`cli inference MODEL features /dev/null --bottleneck 3 --auxdata` without --rate_Fs is the rate-Rs run: Target and Measured lines in the reference's format,
    a finite loss at 100 dB and at -6 dB, the first the smaller; --loss_test prints PASS / FAIL; --write_latent and features_hat are written; a third run adds
    --mp_test and a phase offset to the -6 dB one (H between 0 and 2, mean H^2 = 2: Eq about doubles)"""
    run = _cli(tmp_path, 120)
    hi = run(["features_hat.f32", "--EbNodB", "100", "--write_latent", "z_hat.f32", "--loss_test", "5.0"])
    lo = run(["/dev/null", "--EbNodB", "-6", "--loss_test", "0.001"])
    mp = run(["/dev/null", "--EbNodB", "-6", "--mp_test", "--phase_offset", "0.3"])
    assert "Target..: 100.00  133.01   98.24  2000" in hi and "Target..:  -6.00" in lo
    assert all(np.isfinite(v) for o in (hi, lo, mp) for v in _measured(o)) and 0.0 < _measured(hi)[3] < 10.0
    assert np.isfinite(_loss(hi)) and np.isfinite(_loss(lo)) and np.isfinite(_loss(mp)) and _loss(hi) < _loss(lo)
    assert "\nPASS" in hi and "\nFAIL" in lo and "PASS" not in mp and "FAIL" not in mp
    assert _measured(lo)[2] == _measured(hi)[2]                # Eq is measured ahead of the noise
    assert 1.5 < _measured(mp)[2] / _measured(lo)[2] < 2.5     # the mean of H^2 over the carriers is 2; the carriers' powers are equal only on average
    assert np.fromfile(str(tmp_path / "z_hat.f32"), np.float32).size == 30 * 80 and np.fromfile(str(tmp_path / "features_hat.f32"), np.float32).size == 120 * 36


def test_cli_inference_rate_rs_h_file(tmp_path):
    """--h_file: float32 [.][20] magnitudes, the first 6 n_mf rows used (a longer file is cut, as the reference does); magnitudes of 0.5 quarter the measured Eq
    and leave the PAPR of tx alone; a file with fewer rows is refused with the reference's message"""
    run = _cli(tmp_path, 24)                                   # 2 modem frames: 12 OFDM symbols
    np.full((15, 20), 0.5, np.float32).tofile(str(tmp_path / "h_half.f32"))
    np.ones((10, 20), np.float32).tofile(str(tmp_path / "h_short.f32"))
    plain = _measured(run(["/dev/null", "--EbNodB", "10"]))
    half = _measured(run(["/dev/null", "--EbNodB", "10", "--h_file", "h_half.f32"]))
    assert abs(half[2] / plain[2] - 0.25) < 1e-3 and half[3] == plain[3] and abs((plain[0] - half[0]) - 10 * np.log10(4.0)) < 0.011
    assert "Multipath H file too short" in run(["/dev/null", "--h_file", "h_short.f32"], ok=False)
