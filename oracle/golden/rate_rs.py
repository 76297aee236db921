"""Write tests/golden/rate_rs_bn3.npz: the rate-Rs channel of the bottleneck-3 model (radae.py:603-634, the "hybrid time & frequency domain model": IDFT, PA limiter,
DFT, phase offset, |H|, AWGN) as the reference's RADAE.forward computes it.

The encoder is stubbed to return given latents and the decoder to return z_hat, so a case is (z, H, noise, sigma, phase_offset) -> (z_hat, tx, tx_sym); the noise is the
forward's own draw, re-seeded and drawn again (as oracle/golden/ideal_rx.py does), and the script asserts that it reproduces the forward's z_hat bit for bit.
Numerology: RADAE(21, 80, EbNodB, bottleneck=3) without pilots, cyclic prefix or rate_Fs: Nc = 20, Ns = 6, M = 160 (pilots=True does not run in this branch).
Cases (keys <case>_<array>):
  sat   12 latent rows of N(0, 25^2) latents (the PA saturates, as under the trained encoder), Rayleigh magnitudes H, phase offset 0.3 rad, Eb/No 3 dB
  lin   latents scaled so that |tx| < 0.05 (the limiter's linear region), H = 1, phase 0, 100 dB
  edge  as sat, with one all-zero OFDM symbol and one symbol whose latents are all 1e4
"""
import os

import numpy as np

from . import reference as R
from .reference import golden

ROWS, NC, M = 12, 20, 160


def forward_case(z, H, EbNodB, phase_offset, seed):
    import torch
    from radae import RADAE
    model = RADAE(21, 80, EbNodB, bottleneck=3, phase_offset=phase_offset)
    assert (model.Nc, model.Ns, model.M, model.Ncp) == (NC, 6, M, 0) and abs(float(model.w[0]) - 2 * np.pi * 20 / 160) < 1e-6
    model.eval()
    del model._modules["core_encoder"], model._modules["core_decoder"]
    zt = torch.tensor(z[None])
    model.core_encoder = lambda f: zt
    model.core_decoder = lambda zh: zh
    n_sym = 2 * len(z)
    assert model.num_timesteps_at_rate_Rs(4 * len(z)) == n_sym
    torch.manual_seed(seed)
    with torch.inference_mode():
        o = model(torch.zeros(1, 4 * len(z), 21), torch.tensor(H[None]))
    torch.manual_seed(seed)                                   # the forward's only draw: randn_like(tx_sym)
    noise = torch.randn(1, n_sym, NC, dtype=torch.complex64)
    sigma = float(np.asarray(o["sigma"]).item())
    rx_sym = (o["tx_sym"] + torch.tensor(np.asarray(o["sigma"])) * noise).reshape(1, len(z), 40)
    z_hat = torch.zeros_like(zt)
    z_hat[:, :, ::2] = rx_sym.real
    z_hat[:, :, 1::2] = rx_sym.imag
    assert torch.equal(z_hat, o["z_hat"]), "the re-drawn noise does not reproduce the forward's z_hat"
    want = M / np.sqrt(2 * NC * 10 ** (EbNodB / 10)) / np.sqrt(2)
    assert abs(sigma - want) < 2e-6 * want
    return dict(z=z.astype(np.float32), H=H.astype(np.float32), noise=noise.numpy()[0].astype(np.complex64), sigma=np.float64(sigma), EbNodB=np.float64(EbNodB),
                phase_offset=np.float64(phase_offset), z_hat=o["z_hat"].numpy()[0].astype(np.float32), tx=o["tx"].numpy()[0].astype(np.complex64),
                tx_sym=o["tx_sym"].numpy()[0].astype(np.complex64))


def main(src, dst):
    R.enter()
    OUT = golden(dst, "rate_rs_bn3.npz")
    rng = np.random.default_rng(20241017)
    z_sat = (25.0 * rng.standard_normal((ROWS, 80))).astype(np.float32)
    H_ray = np.abs((rng.standard_normal((2 * ROWS, NC)) + 1j * rng.standard_normal((2 * ROWS, NC))) / np.sqrt(2)).astype(np.float32)
    cases = {"sat": forward_case(z_sat, H_ray, 3.0, 0.3, 11)}
    assert np.abs(cases["sat"]["tx"]).max() > 0.95                 # rms |tx| before the limiter is about 1: its peaks are flattened

    z_lin = rng.standard_normal((ROWS, 80)).astype(np.float32)
    sym = (z_lin[:, ::2] + 1j * z_lin[:, 1::2]).reshape(2 * ROWS, NC)
    w = 2 * np.pi * (20 + np.arange(NC)) / M
    peak = np.abs(sym @ (np.exp(1j * np.outer(w, np.arange(M))) / M)).max()
    z_lin = (z_lin * np.float32(0.04 / peak)).astype(np.float32)
    cases["lin"] = forward_case(z_lin, np.ones((2 * ROWS, NC), np.float32), 100.0, 0.0, 12)
    assert np.abs(cases["lin"]["tx"]).max() < 0.05

    z_edge = z_sat.copy().reshape(2 * ROWS, 40)
    z_edge[5] = 0.0
    z_edge[9] = 1e4
    cases["edge"] = forward_case(z_edge.reshape(ROWS, 80), H_ray, 3.0, 0.3, 13)
    e = cases["edge"]
    assert np.isfinite(e["z_hat"]).all() and np.all(e["tx"][5] == 0) and np.array_equal(e["tx_sym"][5], np.zeros(NC, np.complex64))

    out = {f"{k}_{name}": v for k, c in cases.items() for name, v in c.items()}
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes; full scale " + ", ".join(f"{k} {np.abs(c['z_hat']).max():.3g}" for k, c in cases.items()))
