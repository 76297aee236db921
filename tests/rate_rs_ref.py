"""float64 restatement of the rate-Rs channel of the bottleneck-3 model (radae.py:603-634, include/rade_batch.h: rade_batch_channel_rs_pa), shared by
tests/test_rate_rs_host.py and tests/test_rate_rs_gpu.py: every sum and product in float64 / complex128.

The transform matrices are the reference's own by default: its Winv / Wfwd are complex64 exponentials of float32 arguments n w[c] up to 245 rad, up to 2e-5 rad
from the exact ones.  On ordinary latents that moves z_hat by 3e-6 of full scale; on a symbol whose carriers cancel in the time domain (all latents 1e4: terms of
88 that sum to 0 at every eighth sample) the residue the reference's matrices leave, 1e-2, IS the sample, and the exact matrices give another signal there.  The
20 carriers at DFT bins 20..39 are columns 5..24 of the recorded 30-carrier matrices of tests/golden/consts.npz (same M, same w).  exact=True: the ideal ones."""
import os

import numpy as np

NC, M, C0 = 20, 160, 20                     # carriers, samples per symbol, DFT bin of the first carrier
BAR = 2e-5                                  # the project's bar for latents: max |delta| over the full scale max |z_hat| (rade_batch.h, tests/test_hip_parity.py)
_W_EXACT = np.exp(1j * np.outer(2 * np.pi * (C0 + np.arange(NC)) / M, np.arange(M)))      # e^{+j m w_c}, [c][m]
_REF = []


def matrices(exact=False):
    """(Winv [20][160], Wfwd [160][20]) complex128"""
    if exact:
        return _W_EXACT / M, _W_EXACT.conj().T
    if not _REF:
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consts.npz"))
        assert abs(float(g["w"][5]) - 2 * np.pi * C0 / M) < 1e-6
        _REF.extend([g["Winv"][5:5 + NC].astype(np.complex128), g["Wfwd"][:, 5:5 + NC].astype(np.complex128)])
    return _REF[0], _REF[1]


def sigma_rs3(EbNodB):
    return M / np.sqrt(2 * NC * 10 ** (np.asarray(EbNodB, np.float64) / 10)) / np.sqrt(2)


def channel(z, H, noise, sigma, phase_offset=0.0, exact=False):
    """z [..., n_steps, 80]; H [..., 2 n_steps, 20] or None; noise complex [..., 2 n_steps, 20] or None; sigma a scalar or [...] per stream.
    Returns dict(z_hat, tx, tx_sym, stats = [..., 3]: sum |tx'|^2, max |tx'|, sum |tx_sym|^2 per stream)."""
    z = np.asarray(z, np.float64)
    Winv, Wfwd = matrices(exact)
    lead, n = z.shape[:-2], z.shape[-2]
    sym = (z[..., 0::2] + 1j * z[..., 1::2]).reshape(lead + (2 * n, NC))
    tx = sym @ Winv
    mag = np.abs(tx)
    tx = np.where(mag > 0, np.tanh(mag) / np.where(mag > 0, mag, 1.0), 0.0) * tx
    y = tx @ Wfwd * np.exp(1j * phase_offset)
    if H is not None:
        y = y * np.asarray(H, np.float64)
    r = y
    if noise is not None:
        r = y + np.asarray(sigma, np.float64).reshape(np.shape(sigma) + (1, 1)) * np.asarray(noise, np.complex128)
    r = r.reshape(lead + (n, 40))
    z_hat = np.zeros_like(z)
    z_hat[..., 0::2], z_hat[..., 1::2] = r.real, r.imag
    stats = np.stack([(np.abs(tx) ** 2).sum((-2, -1)), np.abs(tx).max((-2, -1)), (np.abs(y) ** 2).sum((-2, -1))], -1)
    return dict(z_hat=z_hat, tx=tx, tx_sym=y, stats=stats)


def measured_dB(stats, sigma, n_steps):
    """inference.py:215-227 from the per-stream measurements: (10 log10(Eq / No), PAPR in dB)"""
    stats = np.asarray(stats, np.float64)
    Eq = stats[..., 2] / (2 * n_steps * NC)
    S = stats[..., 0] / (2 * n_steps * M)
    return 10 * np.log10(Eq / np.asarray(sigma, np.float64) ** 2), 20 * np.log10(stats[..., 1] / np.sqrt(S))


def fixture_case(g, case):
    """(z, H or None, noise, sigma, phase_offset) of one case of tests/golden/rate_rs_bn3.npz; H = 1 everywhere is given as None (the call's NULL)"""
    H = g[case + "_H"]
    return g[case + "_z"], (None if np.all(H == 1.0) else H), g[case + "_noise"], float(g[case + "_sigma"]), float(g[case + "_phase_offset"])


CASES = ("sat", "lin", "edge")
