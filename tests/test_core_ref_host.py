"""tests/core_ref.py -- the float64 statement of the core encoder and decoder -- held to what the repository already has, at the tolerances it already states
(test_dnnw_export.py::test_oracle_core_on_the_exported_blob_vs_reference_modules: rms < 2e-6, max < 2e-5 against float32 references): the reference's own traces,
the reference's modules on the exporter's checkpoint, and the C oracle on blobs made at run time.  CPU only."""
import glob
import os

import numpy as np
import pytest

import core_ref
from oracle import dnnw_synth
from radae_amd import dnnw

HERE = os.path.dirname(os.path.abspath(__file__))
BLOB_A = os.path.join(HERE, "golden", "dnnw_export_A.bin")
DEFAULT_BLOB = os.path.join(os.path.dirname(HERE), "weights", "model19_check3.bin")


def _replayable(path):
    """a trace that stores z_hat and features_out of EVERY valid call (rxtrace_slipdrops and rxtrace_dfs8001 keep every fourth: the decoder's state at a kept row
    depends on the latents of the rows that were dropped)"""
    with np.load(path) as g:
        return "z_hat" in g.files and "features_out" in g.files and "rows_kept" not in g.files


TRACES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "golden", "rxtrace_*.npz")) if _replayable(p))


def close32(got, want):
    """the bar of a float64 model against a float32 evaluation of the same model"""
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    rms, mx = float(np.sqrt(np.mean(d ** 2))), float(np.abs(d).max())
    assert rms < 2e-6 and mx < 2e-5, (rms, mx)
    return rms, mx


@pytest.fixture(scope="module")
def default_model():
    return dnnw.load_model(DEFAULT_BLOB)


def test_there_are_golden_traces():
    assert len(TRACES) >= 8 and "rxtrace_awgn" in TRACES


@pytest.mark.parametrize("name", TRACES)
def test_decoder_reproduces_the_golden_traces(golden, default_model, name):
    """z_hat -> features_out of every receiver trace of the reference that stores both (the reference resets its decoder at every sync entry)"""
    g = golden(name)
    flags = core_ref.row_resets(core_ref.resets_from_trace(g["ret"], g["state_before"], g["state_after"]))
    assert len(flags) == 3 * len(g["z_hat"]) and flags[0]
    out, _ = core_ref.Decoder(default_model).run(g["z_hat"].reshape(-1, 80), flags)
    feats = core_ref.rows_to_features(out)
    rms, mx = close32(feats, g["features_out"])
    print(f"{name}: rms {rms:.2e} max {mx:.2e}")
    assert not feats.reshape(-1, 12, 36)[:, :, 20:].any()
    idx, want = core_ref.uw_errors_from_rows(g, out)                                # the unique-word sums the reference recorded, from the model's column 20
    assert len(idx) and np.array_equal(g["uw_errors"][idx], want)


def test_encoder_and_decoder_on_the_exporters_checkpoint(golden):
    """the reference's float modules holding checkpoint A (tests/golden/dnnw_export.npz, A/run/*) against the restatement on blob A: both directions, and the
    encoder under bottleneck 1.  This fixture is what pins the encoder restatement: dilations, concat order, gate order."""
    fx = golden("dnnw_export")
    m = dnnw.load_model(BLOB_A)
    close32(core_ref.Encoder(m).run(fx["A/run/features"]), fx["A/run/z"])
    close32(core_ref.Encoder(m).run(fx["A/run/features"], bottleneck=1), fx["A/run/z_bottleneck1"])
    close32(core_ref.Decoder(m).run(fx["A/run/z_hat"])[0], fx["A/run/features_out"])
    e = core_ref.Encoder(m)
    first = e.run(fx["A/run/features"][:5])
    e.reset()
    assert np.array_equal(e.run(fx["A/run/features"][:5]), first)                   # reset() returns to the start-of-utterance state


@pytest.mark.parametrize("seed,lossless", [(4101, True), (4102, False)])
def test_against_the_c_oracle_on_run_time_blobs(oracle, tmp_path, seed, lossless):
    """oracle.Encoder / oracle.Decoder (float32 C) on a synthetic blob written here; the lossless=False model is what the blob holds after quantisation"""
    path = core_ref.write_probe(dnnw_synth.synth_model(seed, lossless=lossless), tmp_path / "m.bin")
    m = dnnw.load_model(path)
    if lossless:
        want = dnnw_synth.tensors(dnnw_synth.synth_model(seed, lossless=True))
        assert all(np.array_equal(v, want[k]) for k, v in dnnw_synth.tensors(m).items())
    om = oracle.Model(path)
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((24, 84)).astype(np.float32)
    z_hat = rng.standard_normal((24, 80)).astype(np.float32)
    oe, oe1, od = oracle.Encoder(om), oracle.Encoder(om), oracle.Decoder(om)
    close32(core_ref.Encoder(m).run(feats), np.stack([oe.step(f) for f in feats]))
    close32(core_ref.Encoder(m).run(feats, bottleneck=1), np.stack([oe1.step(f, bottleneck=1) for f in feats]))
    out, x = core_ref.Decoder(m).run(z_hat)
    close32(out, np.stack([od.step(v) for v in z_hat]))
    assert np.abs(x).max() <= 1.0                                                  # (the reference's clamps are the identity on these values)


def test_probe_blobs_survive_the_round_trip(tmp_path):
    """after write_blob / load_model the output layer is the selector (or the aux row) exactly, and the rest of the model is untouched"""
    base = dnnw_synth.synth_model(4103, lossless=True)
    cols = set()
    for w in range(core_ref.N_WINDOWS):
        m = dnnw.load_model(core_ref.write_probe(core_ref.window(base, w), tmp_path / f"w{w}.bin"))
        c0 = core_ref.window_base(w)
        W = np.zeros((84, core_ref.DEC_W), np.float32); W[np.arange(84), c0 + np.arange(84)] = 1
        b = np.zeros(84, np.float32); b[20] = -4
        assert np.array_equal(m.dec_output.w, W) and np.array_equal(m.dec_output.b, b)
        want, got = dnnw_synth.tensors(base), dnnw_synth.tensors(m)
        assert all(np.array_equal(got[k], want[k]) for k in want if not k.startswith("dec_output"))
        cols |= set(range(c0, c0 + 84))
    assert cols == set(range(core_ref.DEC_W))                                      # every column of x falls in at least one window
    # ... but a valid call keeps 80 of a row's 84 columns: the holes probe shows the in-kernel decoder the 35 columns no window does
    hid = core_ref.hidden_columns()
    assert len(hid) == 35 and hid[0] == 20 and hid[-1] == 735 and 671 not in hid
    shown = set(hid.tolist())
    for w in range(core_ref.N_WINDOWS):
        shown |= set((core_ref.window_base(w) + core_ref.VISIBLE).tolist())
    assert shown == set(range(core_ref.DEC_W))                                     # windows + holes: all 736 columns reach features_out
    m = dnnw.load_model(core_ref.write_probe(core_ref.holes(base), tmp_path / "h.bin"))
    rows, xc = np.nonzero(m.dec_output.w)
    assert np.array_equal(xc, hid) and np.array_equal(rows, core_ref.VISIBLE[:35]) and np.all(m.dec_output.w[rows, xc] == 1) and m.dec_output.b[20] == -4
    for bias in (-4.0, 4.0):
        m = dnnw.load_model(core_ref.write_probe(core_ref.aux(base, bias), tmp_path / "a.bin"))
        assert m.dec_output.b[20] == bias and np.abs(m.dec_output.w[20]).sum() < 1.0
        keep = np.arange(84) != 20
        assert np.array_equal(m.dec_output.w[keep], base.dec_output.w[keep]) and np.array_equal(m.dec_output.b[keep], base.dec_output.b[keep])
    assert base.dec_output.b[20] != 4.0                                            # (aux copies: the model it was given is unchanged)
    assert [core_ref.column_name(c) for c in (0, 95, 96, 191, 192, 223, 224, 735)] == \
        ["dense1[0]", "dense1[95]", "GLU 1[0]", "GLU 1[95]", "conv 1[0]", "conv 1[31]", "GLU 2[0]", "conv 5[31]"]


def test_a_planted_single_column_error_passes_the_rms_bar_and_fails_per_element():
    """Why this file exists.  1e-5 on ONE conv-3 column of every row, seen through the window that covers it: the aggregate bar every decoder has been held to
    (rms < 1e-5, max < 1e-4 over the 432-column features) passes; the per-element comparison at 2^-20 (the in-kernel decoder's limit is below that) names
    the column."""
    base = dnnw_synth.synth_model(4104, lossless=True)
    z_hat = np.random.default_rng(5).standard_normal((24, 80)).astype(np.float32)
    col = 96 + 2 * 128 + 96 + 7                                                     # conv 3, column 7
    w = next(w for w in range(core_ref.N_WINDOWS) if core_ref.window_base(w) <= col < core_ref.window_base(w) + 84)
    dec = core_ref.Decoder(core_ref.window(base, w))
    want, x = dec.run(z_hat)
    c0 = core_ref.window_base(w)
    assert np.array_equal(want[:, np.arange(84) != 20], x[:, c0:c0 + 84][:, np.arange(84) != 20])
    bad = want.copy(); bad[:, col - c0] += 1e-5
    assert core_ref.passes_rms_criterion(core_ref.rows_to_features(bad), core_ref.rows_to_features(want))
    assert core_ref.check_elements("planted", "synthetic", want, want, 2.0 ** -20, x_cols=c0 + np.arange(84)) == 0.0
    with pytest.raises(AssertionError, match=r"x\[%d\], conv 3\[7\].*stream 1, row \d+, row 2 of a chunk of 12" % col):
        core_ref.check_elements("planted", "synthetic", bad, want, 2.0 ** -20, x_cols=c0 + np.arange(84), stream=1, chunk_pos=[(2, 12)] * len(want))


def test_trace_bookkeeping():
    """resets, segments and the unique-word sum on a hand-made trace: search, candidate x3, sync entry, 9 sync calls (window boundary at synced_count 8)"""
    sb = np.array([0, 1, 1, 1] + [2] * 9); sa = np.array([1, 1, 1, 2] + [2] * 9)
    ret = np.array([0, 0, 0, 0] + [1] * 9); sc = np.array([0, 0, 0, 0] + list(range(1, 10)))
    calls = core_ref.resets_from_trace(ret, sb, sa)
    assert calls.tolist() == [True] + [False] * 8
    rows = core_ref.row_resets(calls)
    assert core_ref.segments(rows) == [(0, 27)] and core_ref.segments(np.array([0, 0, 0, 1, 0, 0], bool)) == [(0, 3), (3, 6)]
    out = np.full((27, 84), -1.0); out[[0, 4, 5, 21, 26], 20] = 1.0                 # calls 0, 1, 1, 7 (synced_count 8: new window), 8
    idx, want = core_ref.uw_errors_from_rows({"ret": ret, "state_before": sb, "state_after": sa, "synced_count": sc}, out)
    assert idx.tolist() == list(range(4, 13)) and want.tolist() == [1, 3, 3, 3, 3, 3, 3, 1, 2]
    # the decoder stage's queue: 21 rows ahead of the call with synced_count 8, the last 6 at the end of the launch; 12 + 9 and 6
    pos, queues = core_ref.chunk_plan({"ret": ret, "state_before": sb, "state_after": sa, "synced_count": sc})
    assert queues == [21, 6] and pos[:13].tolist() == [[i, 12] for i in range(12)] + [[0, 9]] and pos[21:].tolist() == [[i, 6] for i in range(6)]
    assert core_ref.chunk_plan({"ret": ret, "state_before": sb, "state_after": sa, "synced_count": sc}, dec_rows=15)[1] == [15, 6, 6]
    assert core_ref.chunk_plan({"ret": ret, "state_before": sb, "state_after": sa, "synced_count": sc}, per_call=True)[1] == [3] * 9
    f = core_ref.rows_to_features(np.arange(3 * 84, dtype=np.float32).reshape(1, 3, 84))
    assert f.shape == (1, 432) and f[0, 19] == 19 and f[0, 20] == 0 and f[0, 36] == 21 and f[0, 4 * 36] == 84 and f[0, 36 * 11 + 19] == 2 * 84 + 63 + 19
