"""Write tests/golden/ideal_rx.npz: the ideal-timing receiver of RADAE.forward / RADAE.receiver (radae.py:312-420, :590-657) as the reference computes it.

(a) `RADAE.receiver` (its decoder stubbed out: z_hat is what the test compares) on the received samples of tests/golden/chan_mpp.npz for every pilot-EQ mode
    (eq_ls, the 3-pilot mean of the default, the mean over all pilots, no pilot EQ) x coarse_mag x time_offset 0 / -16, with the coarse_mag scaling of
    bottleneck 1 and of bottleneck 3.  Results that cannot differ are stored once: coarse_mag off is the same at both bottlenecks, and without pilot EQ
    coarse_mag does nothing (it lives in do_pilot_eq).  Keys: a_<eq>_t<-time_offset>_<bn1|bn3|nomag>.
(b) one bottleneck-1 `ber_test` forward run (inference.py --rate_Fs --pilots --pilot_eq --eq_ls --cp 0.004 --ber_test --freq_offset 1, MPP Doppler samples):
    the sign latents z, G, the channel noise (re-seeded and drawn again, as oracle/golden/reference.py:channel_case does), tx, rx, z_hat, n_errors.
"""
import os

import numpy as np

from . import reference as R
from .reference import golden

EQS = {"ls": dict(pilot_eq=True, eq_mean6=False), "mean6": dict(pilot_eq=True, eq_mean6=True),
       "all": dict(pilot_eq=True, eq_mean6=True, per_carrier_eq=False), "none": dict(pilot_eq=False)}


def genie_z_hat(rx, eq, coarse_mag, time_offset, bottleneck):
    import torch
    from radae import RADAE
    kw = dict(EQS[eq])
    per_carrier = kw.pop("per_carrier_eq", True)
    feat = 21 if bottleneck == 3 else 20
    model = RADAE(feat, 80, 100.0, rate_Fs=True, pilots=True, cyclic_prefix=0.004, time_offset=time_offset, coarse_mag=coarse_mag, bottleneck=bottleneck, **kw)
    model.per_carrier_eq = per_carrier
    del model._modules["core_decoder"]
    model.core_decoder = lambda z: z
    with torch.inference_mode():
        _, z_hat = model.receiver(torch.tensor(rx))
    return z_hat.numpy()[0].astype(np.float32)


def main(src, dst):
    R.enter()
    import torch
    from radae import RADAE
    from radae_amd.channel_tools import multipath_g
    OUT = golden(dst, "ideal_rx.npz")
    out = {}
    rx = np.load(golden(src, "chan_mpp.npz"))["rx"]
    for eq in EQS:
        for t in (0, -16):
            if eq == "none":
                out[f"a_{eq}_t{-t}_nomag"] = genie_z_hat(rx, eq, False, t, 3)
                continue
            out[f"a_{eq}_t{-t}_nomag"] = genie_z_hat(rx, eq, False, t, 3)
            assert np.array_equal(out[f"a_{eq}_t{-t}_nomag"], genie_z_hat(rx, eq, False, t, 1))
            for bn in (1, 3):
                out[f"a_{eq}_t{-t}_bn{bn}"] = genie_z_hat(rx, eq, True, t, bn)
    assert np.array_equal(out["a_none_t16_nomag"], genie_z_hat(rx, "none", True, -16, 3))

    # (b) bottleneck-1 ber_test, model05 numerology
    n_mf, EbNodB, seed = 8, 3.0, 11
    torch.manual_seed(1)
    model = RADAE(20, 80, EbNodB, ber_test=True, rate_Fs=True, freq_offset=1.0, pilots=True, pilot_eq=True, eq_mean6=False, cyclic_prefix=0.004,
                  time_offset=0, coarse_mag=False, bottleneck=1)
    model.eval()
    T = 12 * n_mf
    features = torch.zeros(1, T, 20)
    nRs = model.num_timesteps_at_rate_Rs(T)
    nFs = model.num_timesteps_at_rate_Fs(nRs)
    G = multipath_g("mpp", 8000, nFs, seed + 7)
    torch.manual_seed(seed)
    with torch.inference_mode():
        o = model(features, torch.ones((1, nRs, model.Nc)), torch.tensor(G[None]))
    torch.manual_seed(seed)                                   # the forward's draws again: the sign latents, then the channel noise
    z = torch.sign(torch.rand(1, 3 * n_mf, 80) - 0.5)
    noise = torch.randn(1, nFs, dtype=torch.complex64)
    z_hat = o["z_hat"]
    sigma = float(o["sigma"].item())
    # the draws are the forward's: its tx is the OFDM modulation of z, its rx the channel of tx with this noise
    tx_sym = (z[0, :, ::2] + 1j * z[0, :, 1::2]).reshape(n_mf, 4, 30).numpy()
    sym = np.concatenate([np.broadcast_to(model.P.numpy(), (n_mf, 1, 30)), tx_sym], axis=1).reshape(-1, 30)
    t = sym @ model.Winv.numpy()
    t = np.concatenate([t[:, -32:], t], axis=1).reshape(-1)
    tx = o["tx"].numpy()[0]
    assert np.abs(t - tx).max() < 1e-5
    mp = tx * G[:, 0]; mp[16:] += tx[:-16] * G[:-16, 1]
    mp = mp * np.sqrt(np.mean(np.abs(tx) ** 2) / np.mean(np.abs(mp) ** 2))
    ph = np.exp(1j * np.cumsum(np.full(nFs, np.float32(1.0 * 2 * np.pi / 8000), np.float32), dtype=np.float64))
    assert np.abs(mp * ph + sigma * noise.numpy()[0] - o["rx"].numpy()[0]).max() < 1e-4
    n_errors = int(torch.sum(-z * z_hat > 0))
    out.update(b_z=z.numpy()[0].astype(np.float32), b_G=G.astype(np.complex64), b_noise=noise.numpy()[0].astype(np.complex64), b_sigma=np.float64(sigma),
               b_EbNodB=np.float64(EbNodB), b_freq_offset=np.float64(1.0), b_tx=tx.astype(np.complex64), b_rx=o["rx"].numpy()[0].astype(np.complex64),
               b_z_hat=z_hat.numpy()[0].astype(np.float32), b_n_errors=np.int64(n_errors))
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes; ber_test n_errors {n_errors} of {z.numel()}")
