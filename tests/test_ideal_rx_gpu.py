"""GPU tests (-m gpu) of the ideal-timing ("genie") receiver (rade_batch_rx_ideal: k_irx_demod + k_irx_scale, radae.py:312-420, :590-657) and of the
bottleneck-1 rate-Fs transmitter (RADE_BATCH_TX_LINEAR): parity with the reference's recorded z_hat (tests/golden/chan_*.npz z_fwd, ideal_rx.npz),
batch independence, the reference's BER checks (CMakeLists.txt:112-130) at their bars, and the command line of inference.py --ber_test."""
import os
import subprocess
import sys

import numpy as np
import pytest

from file_ref import check_z
from gpu_kit import REPO, engine, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
M05 = os.path.join(REPO, "weights", "model05.bin")


@pytest.mark.parametrize("case", ["awgn", "mpp"])
def test_z_fwd_parity(engine, torch_dev, golden, case):
    """RADAE.forward's own receiver (eq_ls, coarse_mag, time_offset -16, correct_freq_offset) on the fixture's samples: z_hat and the decoded features"""
    import torch
    g = golden("chan_" + case)
    n_mf = len(g["rx"]) // 960
    eng = engine(1, max_tx_mf=n_mf)
    rx = torch.tensor(g["rx"][None], device=torch_dev)
    feats, z_hat, n_err = eng.rx_ideal(rx, n_mf, time_offset=-16, eq="ls", coarse_mag=True, freq_offset=float(g["freq_offset"]))
    assert n_err is None
    check_z(z_hat.cpu().numpy()[0], g["z_fwd"], case)
    f_ref = eng.decode(torch.tensor(g["z_fwd"][None], device=torch_dev), 84).cpu().numpy()
    assert np.sqrt(np.mean((feats.cpu().numpy() - f_ref) ** 2)) <= 1e-4


def test_every_eq_mode_matches_the_reference(engine, torch_dev, golden):
    import torch
    from radae_amd.engine import TX_LINEAR
    g = golden("ideal_rx")
    rx_np = golden("chan_mpp")["rx"]
    n_mf = len(rx_np) // 960
    engs = {3: engine(1, max_tx_mf=2), 1: engine(1, max_tx_mf=2, flags=TX_LINEAR)}     # the coarse_mag scaling follows the waveform
    rx = torch.tensor(rx_np[None], device=torch_dev)
    n = 0
    for key in g.files:
        if not key.startswith("a_"):
            continue
        _, eq, t, sc = key.split("_")
        for bn in ((1, 3) if sc == "nomag" else (int(sc[2]),)):
            _, z_hat, _ = engs[bn].rx_ideal(rx, n_mf, time_offset=-int(t[1:]), eq=eq, coarse_mag=sc != "nomag", feat_width=0)
            check_z(z_hat.cpu().numpy()[0], g[key], f"{key} bn{bn}")
            n += 1
    assert n == 28


def test_bottleneck1_ber_forward_run(engine, torch_dev, golden):
    """fixture (b): TX_LINEAR modulation of the sign latents, the channel with the recorded noise, the genie receiver's BER count"""
    import torch
    from radae_amd.engine import BOTTLENECK1, TX_LINEAR, sigma_from_EbNodB
    g = golden("ideal_rx")
    z = torch.tensor(g["b_z"][None], device=torch_dev)
    n_mf = z.shape[1] // 3
    eng = engine(1, max_tx_mf=n_mf, blob=M05, flags=BOTTLENECK1 | TX_LINEAR)
    iq = eng.tx_latents(z)
    assert np.abs(iq.cpu().numpy()[0] - g["b_tx"]).max() < 2e-5
    assert abs(sigma_from_EbNodB(float(g["b_EbNodB"]), bottleneck=1) - float(g["b_sigma"])) < 1e-6 * float(g["b_sigma"])
    rx = eng.channel(iq, float(g["b_sigma"]), float(g["b_freq_offset"]), G=torch.tensor(g["b_G"][None], device=torch_dev),
                     noise=torch.tensor(g["b_noise"][None], device=torch_dev))
    assert np.abs(rx.cpu().numpy()[0] - g["b_rx"]).max() < 1e-5
    _, z_hat, n_err = eng.rx_ideal(torch.tensor(g["b_rx"][None], device=torch_dev), n_mf, time_offset=0, eq="ls", coarse_mag=False, z_ref=z, feat_width=0)
    check_z(z_hat.cpu().numpy()[0], g["b_z_hat"], "ber run")
    ties = int(np.sum(np.abs(g["b_z_hat"]) < 1e-5))
    assert abs(int(n_err[0]) - int(g["b_n_errors"])) <= ties
    # the flag is refused where it cannot be honoured
    with pytest.raises(RuntimeError):
        eng.tx_eoo()
    with pytest.raises(RuntimeError):
        eng.channel(iq, 0.1, with_eoo=True)


def test_batch_streams_are_independent(engine, torch_dev, golden):
    """64 streams with different samples and frequency offsets: per-stream z_hat bit-equal to one-stream runs"""
    import torch
    rx_np = golden("chan_mpp")["rx"]
    n_mf = len(rx_np) // 960
    B = 64
    rxs = np.stack([np.roll(rx_np, 960 * (b % n_mf) + 7 * b) for b in range(B)]).astype(np.complex64)
    fo = -11.0 + 0.37 * np.arange(B, dtype=np.float32)
    dfdt = np.where(np.arange(B) % 3 == 0, 0.5, 0.0).astype(np.float32)
    eng = engine(B, max_tx_mf=n_mf)
    z_ref = torch.tensor(np.sign(np.random.default_rng(3).standard_normal((B, 3 * n_mf, 80))).astype(np.float32), device=torch_dev)
    feats, z_hat, n_err = eng.rx_ideal(torch.tensor(rxs, device=torch_dev), n_mf, time_offset=-16, eq="ls", coarse_mag=True, freq_offset=fo, df_dt=dfdt, z_ref=z_ref)
    one = engine(1, max_tx_mf=n_mf)
    for b in range(B):
        f1, z1, e1 = one.rx_ideal(torch.tensor(rxs[b:b + 1], device=torch_dev), n_mf, time_offset=-16, eq="ls", coarse_mag=True, freq_offset=fo[b], df_dt=dfdt[b], feat_width=0,
                                  z_ref=z_ref[b:b + 1].contiguous())
        assert torch.equal(z1[0], z_hat[b]), b
        assert int(e1[0]) == int(n_err[b])
        assert int(n_err[b]) == int((-z_ref[b] * z_hat[b] > 0).sum())


def test_rx_ideal_error_count_equals_ber_align_shift_0(engine, torch_dev, golden):
    """B = 2, two modem frames, random sign latents as the reference: the count rade_batch_rx_ideal reads back is rade_batch_ber_align's at shift 0 on the same z_hat
    (one workgroup count behind both), and both are NumPy's.  Integers: no tolerance"""
    import torch
    rx_np = golden("chan_mpp")["rx"]
    B, n_mf = 2, 2
    rx = torch.tensor(np.stack([rx_np[:n_mf * 960], np.roll(rx_np, 960 * 3)[:n_mf * 960]]), device=torch_dev)
    z_ref = torch.tensor(np.sign(np.random.default_rng(31).standard_normal((B, 3 * n_mf, 80))).astype(np.float32), device=torch_dev)
    eng = engine(B, max_tx_mf=n_mf)
    _, z_hat, n_err = eng.rx_ideal(rx, n_mf, z_ref=z_ref, feat_width=0)
    shifts = eng.ber_align(z_ref, z_hat)
    want = np.sum(-z_ref.cpu().numpy() * z_hat.cpu().numpy() > 0, axis=(1, 2))
    print("n_errors", n_err.tolist(), "ber_align shift 0", shifts[:, 0].tolist(), "numpy", want.tolist())
    assert 0 < want.min() and want.max() < 3 * n_mf * 80            # (a count that could not tell the two sides apart would be 0 or all)
    for b in range(B):
        assert int(n_err[b]) == int(shifts[b, 0]) == int(want[b]), b


def ber_run(torch_dev, EbNodB, freq_offset, mpp, B=64, n_mf=72, seed=9):
    import torch
    from radae_amd.engine import BOTTLENECK1, TX_LINEAR, BatchEngine, sigma_from_EbNodB
    eng = BatchEngine(B, max_tx_mf=n_mf, blob=M05, flags=BOTTLENECK1 | TX_LINEAR)
    gen = torch.Generator(device=torch_dev).manual_seed(seed)
    z = torch.sign(torch.rand((B, 3 * n_mf, 80), device=torch_dev, generator=gen) - 0.5)
    iq = eng.tx_latents(z)
    G = eng.multipath_gen("mpp", n_mf * 960, seed=seed) if mpp else None       # one Doppler realisation per stream
    rx = eng.channel(iq, sigma_from_EbNodB(EbNodB, bottleneck=1), freq_offset, G=G, seed=seed)
    _, _, n_err = eng.rx_ideal(rx, n_mf, time_offset=0, eq="ls", coarse_mag=False, z_ref=z, feat_width=0)    # --pilot_eq --eq_ls, no correction
    eng.close()
    return int(n_err.sum()), z.numel()


def test_ber_awgn_high_snr_is_error_free(torch_dev):
    e, n = ber_run(torch_dev, 100.0, 0.0, False, B=8, n_mf=50)
    assert e == 0, e / n


def test_ber_awgn_operating_point(torch_dev):
    """inference_ber_awgn: Eb/No 0 dB, +1 Hz uncorrected: BER < 0.5 erfc(sqrt(10^((0 - 2) / 10))) = 0.131, and above the no-loss theory at the nominal Eb/No,
    0.5 erfc(1) = 0.0786: the waveform spends 1.76 dB on cyclic prefix and pilots, so a BER below the floor means the generator delivers too little noise"""
    from math import erfc, sqrt
    e, n = ber_run(torch_dev, 0.0, 1.0, False)
    assert n >= 10 ** 6
    bar = 0.5 * erfc(sqrt(10 ** ((0 - 2) / 10)))
    floor = 0.5 * erfc(1.0)
    print(f"AWGN 0 dB: BER {e / n:.4f} over {n} bits (floor {floor:.4f}, bar {bar:.4f})")
    assert floor < e / n < bar


def test_ber_mpp_operating_point(torch_dev):
    """inference_ber_mpp: Eb/No 0 dB, MPP (64 device-generated Doppler realisations), +1 Hz: BER < 0.5 (1 - sqrt(EbNo / (EbNo + 1))) with 2 dB loss = 0.189,
    and above the same curve without loss at the nominal Eb/No, 0.5 (1 - sqrt(1 / 2)) = 0.1464"""
    e, n = ber_run(torch_dev, 0.0, 1.0, True)
    assert n >= 10 ** 6
    ebno = 10 ** ((0 - 2) / 10)
    bar = 0.5 * (1 - np.sqrt(ebno / (ebno + 1)))
    floor = 0.5 * (1 - np.sqrt(0.5))
    print(f"MPP 0 dB: BER {e / n:.4f} over {n} bits (floor {floor:.4f}, bar {bar:.4f})")
    assert floor < e / n < bar


def test_cli_inference_ber_test(tmp_path):
    """ctest inference_ber: model05, --rate_Fs --pilots --cp 0.004 --pilot_eq --eq_ls --ber_test at Eb/No 100 dB prints BER: 0.000"""
    feats = np.zeros((12 * 20, 36), np.float32)
    fpath = tmp_path / "features.f32"
    feats.tofile(fpath)
    zpath = tmp_path / "z_hat.f32"
    r = subprocess.run([sys.executable, "-m", "radae_amd.cli", "inference", M05, str(fpath), "/dev/null", "--rate_Fs", "--pilots", "--EbNodB", "100", "--cp", "0.004",
                        "--pilot_eq", "--eq_ls", "--ber_test", "--bottleneck", "1", "--write_latent", str(zpath)],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "n_bits: 4800 BER: 0.000" in r.stdout, r.stdout
    z = np.fromfile(zpath, np.float32)
    assert z.size == 4800 and np.all(np.abs(np.abs(z) - 1.0) < 0.05)
