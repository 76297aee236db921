"""CPU tests of the ideal-timing ("genie") receiver (RADAE.forward / RADAE.receiver, radae.py:312-420, :590-657): the C ABI exports it and the
bottleneck-1 noise scale, and a NumPy restatement of the receiver -- cyclic prefix removal, DFT, do_pilot_eq in all four EQ modes, the last-frame
slope of the reference, coarse_mag at both bottleneck scalings, the demapper -- reproduces what the reference recorded in tests/golden/ideal_rx.npz
(oracle/golden/ideal_rx.py).  The GPU kernels are checked against the same recordings in tests/test_ideal_rx_gpu.py."""
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, NC, M, NCP = 4, 30, 160, 32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


def test_ideal_rx_symbols_are_exported(lib):
    from radae_amd import engine
    for s in ("rade_batch_rx_ideal", "rade_sigma_from_EbNodB_bn1"):
        assert s in engine.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    assert engine.TX_LINEAR == 0x1000
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    assert "#define RADE_BATCH_TX_LINEAR 0x1000" in hdr and "int rade_batch_rx_ideal(" in hdr


def test_bottleneck1_sigma(lib):
    from radae_amd import engine
    for e in (-3.0, 0.0, 2.5, 10.0, 100.0):
        want = (10 ** (e / 10) * 160) ** -0.5                       # radae.py:574-576
        assert abs(engine.sigma_from_EbNodB(e, bottleneck=1) - want) <= 2e-6 * want
        assert abs(engine.sigma_from_EbNodB(e) - (8000 / (10 ** (e / 10) * 2000)) ** 0.5) <= 2e-6 * engine.sigma_from_EbNodB(e)
    with pytest.raises(ValueError):
        engine.sigma_from_EbNodB(0.0, bottleneck=2)


def genie_receiver(rx, consts, eq, coarse_mag, time_offset, bottleneck, quirk=True):
    """RADAE.receiver up to z_hat, restated in NumPy (complex128)."""
    P, Wfwd, w = consts["P"].real.astype(np.float64), consts["Wfwd"].astype(np.complex128), consts["w"].astype(np.float64)
    n_mf = len(rx) // ((NS + 1) * (M + NCP))
    r = rx[:n_mf * (NS + 1) * (M + NCP)].reshape(n_mf * (NS + 1), M + NCP)[:, NCP + time_offset:NCP + time_offset + M]
    sym = (r.astype(np.complex128) @ Wfwd).reshape(n_mf, NS + 1, NC)
    if eq != "none":
        h = sym[:, 0, :] / P
        rp = np.zeros((n_mf, NC), np.complex128)
        for c in range(NC):
            cm = min(max(c, 1), NC - 2)
            if eq == "all":
                rp[:, c] = h.mean(axis=1)
            elif eq == "mean6":
                rp[:, c] = h[:, cm - 1:cm + 2].mean(axis=1)
            else:                                                       # 3-pilot least squares, a = 0.0025 Fs
                a = 0.0025 * 8000
                A = np.stack([np.ones(3), np.exp(-1j * w[cm - 1:cm + 2] * a)], axis=1)
                Pm = np.linalg.inv(A.T @ A) @ A.T
                g = h[:, cm - 1:cm + 2] @ Pm.T
                rp[:, c] = g[:, 0] + g[:, 1] * np.exp(-1j * w[c] * a)
        s = np.arange(1, NS + 1)
        for i in range(n_mf):
            # every frame but the last: towards the next frame's pilot; the last one reuses the loop's final slope (carrier Nc-1, frame n_mf-2)
            if i < n_mf - 1:
                slope = (rp[i + 1] - rp[i]) / (NS + 1)
            elif quirk:
                slope = np.full(NC, (rp[i, NC - 1] - rp[i - 1, NC - 1]) / (NS + 1))
            else:                                                       # (what a per-carrier last slope would give)
                slope = (rp[i] - rp[i - 1]) / (NS + 1)
            ch = slope[None, :] * s[:, None] + rp[i][None, :]
            sym[i, 1:] *= np.exp(-1j * np.angle(ch))
        if coarse_mag:
            mag = np.sqrt(np.mean(np.abs(rp) ** 2))
            if bottleneck == 3:
                mag *= abs(P[0]) / (10 ** (-2 / 20) * M / NC ** 0.5)
            sym = sym / mag
    d = sym[:, 1:, :].reshape(n_mf * 3, 40)
    z = np.zeros((n_mf * 3, 80))
    z[:, ::2], z[:, 1::2] = d.real, d.imag
    return z


def test_numpy_genie_receiver_matches_reference_recordings(golden):
    g, consts = golden("ideal_rx"), golden("consts")
    rx = golden("chan_mpp")["rx"]
    n = 0
    for key in g.files:
        if not key.startswith("a_"):
            continue
        _, eq, t, sc = key.split("_")
        z = genie_receiver(rx, consts, eq, sc != "nomag", -int(t[1:]), 1 if sc == "bn1" else 3)
        ref = g[key]
        assert z.shape == ref.shape
        err = np.sqrt(np.mean((z - ref) ** 2)) / np.sqrt(np.mean(ref ** 2))
        assert err < 1e-5, (key, err)
        n += 1
    assert n == 20
    # the last-frame quirk is pinned: per-carrier slopes in the last frame miss the recording by far more than the bar
    z = genie_receiver(rx, consts, "ls", False, -16, 3, quirk=False)
    ref = g["a_ls_t16_nomag"]
    assert np.sqrt(np.mean((z[-3:] - ref[-3:]) ** 2)) > 1e-3 * np.sqrt(np.mean(ref ** 2))
    assert np.array_equal(z[:-3], genie_receiver(rx, consts, "ls", False, -16, 3)[:-3])


def test_ber_fixture_is_consistent(golden):
    """fixture (b): the recorded error count is the reference's rule (-z z_hat > 0) on the recorded sign latents"""
    g = golden("ideal_rx")
    z, zh = g["b_z"], g["b_z_hat"]
    assert set(np.unique(z)) <= {-1.0, 1.0}
    assert int(np.sum(-z * zh > 0)) == int(g["b_n_errors"])
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "ideal_rx.npz")) < 1 << 20
