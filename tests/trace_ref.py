"""The receiver's edge-case recordings (tests/golden/rxtrace_slipdrops, _dfs8001, _eoo_mpp): the samples a recording feeds the receiver and the check of a
trace against it.  The bars are the same for the CPU oracle (tests/test_oracle_golden.py) and for the device (tests/test_hip_parity.py), so both take them
from here.  numpy only; holds no fixtures."""
import numpy as np

from gpu_kit import INT_KEYS, rms


def edge_case_input(g):
    """The round-6 streaming fixtures carry what the reference's ctests pipe into the receiver: int16 samples, converted as the ctest converts them
    (`int16tof32.py --zeropad` for the mono slip + drops file, `int16tof32.py` for the two-channel 8001 Hz file), or complex64 samples."""
    from radae_amd import wire
    if "rx_in" in g.files:
        return g["rx_in"]
    i16 = g["rx_i16"]
    return np.frombuffer(wire.int16_to_f32(np.ascontiguousarray(i16).tobytes(), zeropad=(i16.ndim == 1)), np.complex64)


def check_edge_trace(d, g, zhat_tol=1e-4):
    for k in INT_KEYS:
        assert np.array_equal(d[k], g[k]), (k, int(np.argmax(d[k][:len(g[k])] != g[k][:len(d[k])])) if len(d[k]) == len(g[k]) else (len(d[k]), len(g[k])))
    assert np.abs(d["fmax"] - g["fmax"]).max() < 1e-9
    for k in ["Dthresh", "Dtmax12", "Dtmax12_eoo", "snrdB_3k_est"]:
        assert np.abs(d[k] - g[k]).max() < 3e-5 * max(1.0, np.abs(g[k]).max()), k
    rows = g["rows_kept"] if "rows_kept" in g.files else np.arange(len(g["features_out"]))
    assert len(d["features_out"]) == (int(g["n_valid_total"]) if "n_valid_total" in g.files else len(g["features_out"]))
    zs = np.abs(g["z_hat"]).max()
    assert rms(d["z_hat"][rows], g["z_hat"]) < zhat_tol * max(1.0, zs)
    fo = d["features_out"][rows]
    assert rms(fo, g["features_out"]) < 1e-5 and np.abs(fo - g["features_out"]).max() < 1e-4
    if g["eoo_out"].size:
        assert d["eoo_out"].shape == g["eoo_out"].shape and np.array_equal(d["eoo_out"] > 0, g["eoo_out"] > 0)
