"""CPU tests of the rate-Rs channel of the bottleneck-3 model (RADAE.forward without rate_Fs, radae.py:603-634; rade_batch_channel_rs_pa): the float64
restatement of tests/rate_rs_ref.py reproduces what the reference recorded in tests/golden/rate_rs_bn3.npz (oracle/golden/rate_rs.py), the C ABI exports
the call and its noise scale, and the command line refuses the combination the reference cannot run.  The kernel itself is checked against the same
recordings and the same restatement in tests/test_rate_rs_gpu.py."""
import os

import numpy as np
import pytest

import rate_rs_ref as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


@pytest.mark.parametrize("case", rs.CASES)
def test_restatement_reproduces_the_reference_recordings(golden, case):
    """z_hat and tx_sym inside the project's bar for latents, 2e-5 of the case's full scale; tx at the bound of a float32 sum of 20 terms.  With the ideal transform matrices in
    place of the reference's the ordinary cases still hold the bar (the reference's matrices are 2e-5 rad off at worst: 3e-6 of full scale on z_hat); the symbol of
    latents 1e4 does not, which is why the restatement takes the recorded matrices (tests/rate_rs_ref.py)."""
    g = golden("rate_rs_bn3")
    z, H, noise, sigma, ph = rs.fixture_case(g, case)
    r = rs.channel(z, H, noise, sigma, ph)
    full = np.abs(g[case + "_z_hat"]).max()
    err = np.abs(r["z_hat"] - g[case + "_z_hat"]).max()
    print(f"{case}: max |dz_hat| {err:.3g} = {err / full:.3g} of full scale {full:.3g}; max |dtx| {np.abs(r['tx'] - g[case + '_tx']).max():.3g}")
    assert err <= rs.BAR * full
    assert np.abs(r["tx_sym"] - g[case + "_tx_sym"]).max() <= rs.BAR * full
    # tx: the reference sums 20 float32 terms sym[c] Winv[c][m] per sample: at most 20 x 2^-24 of the sum of their magnitudes (|Winv| = 1/160), plus a few
    # roundings of the limiter on a value <= 1 -- 5e-6 on ordinary symbols, 2e-3 on the symbol of latents 1e4 (terms of 88 each)
    sym = np.abs(z[:, 0::2] + 1j * z[:, 1::2]).reshape(24, 20)
    tol = 20 * 2.0 ** -24 * sym.sum(1) / 160 + 8 * 2.0 ** -24
    assert np.all(np.abs(r["tx"] - g[case + "_tx"]).max(1) <= tol), (np.abs(r["tx"] - g[case + "_tx"]).max(1) / tol).max()
    x = rs.channel(z, H, noise, sigma, ph, exact=True)
    ex = np.abs(x["z_hat"] - g[case + "_z_hat"]).max()
    print(f"{case}: ideal matrices: max |dz_hat| {ex:.3g} = {ex / full:.3g} of full scale")
    if case != "edge":                       # (measured on the edge case: 1.8e-4 of full scale, all of it in the symbol of latents 1e4)
        assert ex <= rs.BAR * full
    assert r["z_hat"].shape == (12, 80) and r["tx"].shape == (24, 160) and r["tx_sym"].shape == (24, 20)


def test_fixture_is_what_the_issue_describes(golden):
    g = golden("rate_rs_bn3")
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "rate_rs_bn3.npz")) < 1 << 20
    for case in rs.CASES:
        assert abs(float(g[case + "_sigma"]) - rs.sigma_rs3(float(g[case + "_EbNodB"]))) <= 2e-6 * float(g[case + "_sigma"])
        assert g[case + "_noise"].dtype == np.complex64 and g[case + "_z"].shape == (12, 80) and g[case + "_H"].shape == (24, 20)
    assert np.abs(g["sat_tx"]).max() > 0.95 and np.abs(g["lin_tx"]).max() < 0.05 and np.all(g["lin_H"] == 1.0)
    assert float(g["sat_phase_offset"]) == 0.3 and float(g["lin_phase_offset"]) == 0.0 and float(g["lin_EbNodB"]) == 100.0
    ze = g["edge_z"].reshape(24, 40)
    assert np.all(ze[5] == 0.0) and np.all(ze[9] == 1e4) and np.isfinite(g["edge_z_hat"]).all()
    # the zero symbol comes out as sigma times its noise, exactly (float32 product, as torch forms it)
    zh = g["edge_z_hat"].reshape(24, 20, 2)
    n5 = g["edge_noise"][5]
    assert np.array_equal(zh[5, :, 0], np.float32(g["edge_sigma"]) * n5.real) and np.array_equal(zh[5, :, 1], np.float32(g["edge_sigma"]) * n5.imag)


def test_rate_rs_sigma(lib):
    from radae_amd import engine
    for e in (-6.0, 0.0, 3.0, 100.0):
        want = 160 / (2 * 20 * 10 ** (e / 10)) ** 0.5 / 2 ** 0.5          # radae.py:627-630
        assert abs(engine.sigma_from_EbNodB(e, rate_Fs=False) - want) <= 2e-6 * want
        assert abs(float(lib.rade_sigma_from_EbNodB_rs3(e)) - want) <= 2e-6 * want
    assert abs(engine.sigma_from_EbNodB(3.0, rate_Fs=False) - 12.66) < 5e-3
    v = engine.sigma_from_EbNodB(np.float32([-6.0, 3.0]), rate_Fs=False)
    assert v.dtype == np.float32 and v[1] == np.float32(engine.sigma_from_EbNodB(3.0, rate_Fs=False))
    with pytest.raises(ValueError):
        engine.sigma_from_EbNodB(0.0, bottleneck=1, rate_Fs=False)
    assert engine.sigma_from_EbNodB(3.0) == engine.sigma_from_EbNodB(3.0, bottleneck=3, rate_Fs=True)      # the rate-Fs forms are what they were


def test_rate_rs_symbols_are_declared_and_exported(lib):
    from radae_amd import engine
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    for s in ("rade_batch_channel_rs_pa", "rade_sigma_from_EbNodB_rs3"):
        assert s in engine.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    assert "int rade_batch_channel_rs_pa(rade_batch *h," in hdr and "float rade_sigma_from_EbNodB_rs3(float EbNodB);" in hdr
    assert hasattr(engine.BatchEngine, "channel_rs_pa")


def test_cli_refuses_pilots_without_rate_Fs(capsys):
    """pilots=True without rate_Fs does not run in the reference (tx_sym * H: 5 n_mf against 4 n_mf symbols); refused before any file or GPU is touched"""
    from radae_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["inference", "no_such_model.bin", "no_such_features.f32", "/dev/null", "--pilots", "--bottleneck", "3", "--auxdata"])
    assert "--pilots needs --rate_Fs" in str(e.value) and "reference does not run" in str(e.value)


@pytest.mark.parametrize("extra,word", [(["--g_file", "g.f32"], "--g_file"), (["--write_rx", "rx.f32"], "--write_rx"), (["--freq_offset", "-11"], "--freq_offset"),
                                        (["--end_of_over", "--prepend_noise", "1"], "--prepend_noise, --end_of_over"), (["--ideal_rx"], "--ideal_rx"), (["--rx_gain", "2"], "--rx_gain")])
def test_cli_rate_rs_refuses_what_only_rate_Fs_has(extra, word):
    """without --rate_Fs the run is the rate-Rs one: an option of the sample-rate channel is refused (before any file or GPU is touched), not ignored"""
    from radae_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["inference", "no_such_model.bin", "no_such_features.f32", "/dev/null", "--bottleneck", "3", "--auxdata"] + extra)
    assert word in str(e.value) and "--rate_Fs" in str(e.value)


def test_cli_rate_rs_needs_auxdata():
    from radae_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["inference", "no_such_model.bin", "no_such_features.f32", "/dev/null", "--bottleneck", "3"])
    assert "--auxdata" in str(e.value)
