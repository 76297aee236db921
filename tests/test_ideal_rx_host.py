"""CPU tests of the ideal-timing ("genie") receiver (RADAE.forward / RADAE.receiver, radae.py:312-420, :590-657): the C ABI exports it and the
bottleneck-1 noise scale, and the NumPy restatement of the receiver (file_ref.demod) -- cyclic prefix removal, DFT, do_pilot_eq in all four EQ modes, the last-frame
slope of the reference, coarse_mag at both bottleneck scalings, the demapper -- reproduces what the reference recorded in tests/golden/ideal_rx.npz
(oracle/golden/ideal_rx.py).  The GPU kernels are checked against the same recordings in tests/test_ideal_rx_gpu.py."""
import os

import numpy as np
import pytest

import file_ref as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_numpy_genie_receiver_matches_reference_recordings(golden):
    g, rx = golden("ideal_rx"), golden("chan_mpp")["rx"]
    n = 0
    for key in g.files:
        if not key.startswith("a_"):
            continue
        _, eq, t, sc = key.split("_")
        z = F.demod(rx, eq, sc != "nomag", -int(t[1:]), 1 if sc == "bn1" else 3)
        ref = g[key]
        assert z.shape == ref.shape
        err = np.sqrt(np.mean((z - ref) ** 2)) / np.sqrt(np.mean(ref ** 2))
        assert err < 1e-5, (key, err)
        n += 1
    assert n == 20
    # the last-frame quirk is pinned: per-carrier slopes in the last frame miss the recording by far more than the bar
    z = F.demod(rx, "ls", False, -16, 3, quirk=False)
    ref = g["a_ls_t16_nomag"]
    assert np.sqrt(np.mean((z[-3:] - ref[-3:]) ** 2)) > 1e-3 * np.sqrt(np.mean(ref ** 2))
    assert np.array_equal(z[:-3], F.demod(rx, "ls", False, -16, 3)[:-3])


def test_ber_fixture_is_consistent(golden):
    """fixture (b): the recorded error count is the reference's rule (-z z_hat > 0) on the recorded sign latents"""
    g = golden("ideal_rx")
    z, zh = g["b_z"], g["b_z_hat"]
    assert set(np.unique(z)) <= {-1.0, 1.0}
    assert int(np.sum(-z * zh > 0)) == int(g["b_n_errors"])
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "ideal_rx.npz")) < 1 << 20
