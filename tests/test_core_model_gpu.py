"""Every device decoder and encoder against the float64 model of tests/core_ref.py, PER ELEMENT.

The decoder has three doors on the device and the suite has judged them by one blob and an aggregate (rms over the 432-column features):
    K   the decoder stage inside the receiver kernel (dq2_layers, rade_rx_dec.h): the receiver's features_out
    L   the layer-wise decoder (rade_batch_decode, BatchEngine.decode)
    S   the single-stream step kernel (k_core_dec_step, CoreDecoder.step)
Here all three run on IDENTICAL rows: the receiver's trace records the float32 latents its decoder stage reads (trace_z is written from the same registers as
the stage's input rows), and the reset flags follow from the trace's states.  F is core_ref.Decoder on the same rows and flags.

What is visible.  The decoder's concat buffer x[736] holds every layer's output, and the output layer is a float dense layer, so a blob whose output layer
copies 84 columns of x (core_ref.window, nine of them) shows every internal column in the rows the doors return.  A valid receiver call keeps 80 of a row's 84
columns; core_ref.holes shows K the 35 columns that no window does.  core_ref.aux fixes the unique-word decisions: -4 never fails a window, +4 fails every
window, which loses sync with three rows pending and puts the next reset flag on row 3 of a chunk.

Limits.  dense1 (x[0..95]) is tanh(W z + b) with K = 80 and nothing compounds, so K is held to a derived bound there (dense1_bound).  Everything else has
passed through recurrent state; a forward bound is not practical, and the limit is measured against F with L -- the decoder built from kernels whose bounds ARE
derived (tests/test_kernel_units_gpu.py) -- as the anchor: per case, with e_D = max |D - F| over streams, rows and the columns K shows,
    e_K <= C_K max(e_L, 2^-24)
for every element (the dense1 columns included: they get the smaller of the two limits).
L and S are held to their own measured maxima over all cases, rounded up to a power of two (LIM_L, LIM_S); the encoder doors likewise (LIM_ENC).  Every
figure measured on the MI355X stands in DESIGN.md section 3.5 beside these constants.  On top, every door keeps the bar the suite has held it to (rms < 1e-5,
max < 1e-4 over the 432-column features)."""
import numpy as np
import pytest

import core_ref
from gpu_kit import INT_KEYS, dev, engine, pack, torch_dev  # noqa: F401
from kernel_ref import EPS_TANH_HW, SENT32, U, gemm_bound
from oracle import dnnw_synth
from radae_amd import dnnw

pytestmark = pytest.mark.gpu

# ---- the assertion constants (measured figures: DESIGN.md section 3.5, "Per-element parity of the core network") --------------------------------------------------
C_K = 8.0                         # e_K <= C_K max(e_L, 2^-24): largest ratio measured 7.04 (synthA/window3)
LIM_L = 2.0 ** -16                # max |L - F| over all 84 columns of a row: measured 1.131e-05 (synthA/window0, the stream with |z_hat| in the thousands)
LIM_S = 2.0 ** -16                # max |S - F|: measured 8.691e-06 (the same rows)
LIM_ENC = {"encode B=1": 2.0 ** -14, "encode B=3": 2.0 ** -14, "step": 2.0 ** -14, "step bottleneck 1": 2.0 ** -15, "tx_frame3": 2.0 ** -14}

B, N_MF, N_PRE = 4, 40, 3000
LEAD_CUT = (0, 517, 1203, 0)      # samples of the common noise lead-in a stream does not get
TAIL_CUT = (0, 5000, 12345, 0)    # samples a stream ends early by (streams 1 and 2 never see their end-of-over frame)
EBNO = (20.0, 20.0, 20.0, 60.0)
FOFF = (3.0, -5.0, 7.0, 7.0)
FADED = range(6, 10)              # stream 3: the pilot symbols of these frames x 1e-4 (test_unbounded_operands_do_not_overflow (c)): |z_hat| leaves +-256.  Inside the
                                  # first synchronised period, so that the rows are decoded whether the first unique-word window then fails (+4) or not
TRACE_CALLS = 64
CAP = N_MF + 4                    # valid calls a stream can have, and max_tx_mf of the engine: L's longest segment is 3 CAP rows

SYNTH = {"synthA": (4201, True), "synthB": (4202, True), "lossy": (4203, False)}
DEC_CASES = ["default", "synthA/aux-4", "synthB/aux-4", "lossy/aux-4"] + [f"synthA/window{w}" for w in range(core_ref.N_WINDOWS)] + ["synthA/holes", "synthA/aux+4"]


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    """name -> (path of the blob, the model it holds after the round trip, x column of every output column or None)"""
    from radae_amd import engine as eng_mod
    made, base, d = {}, {}, tmp_path_factory.mktemp("probe_blobs")

    def get(name):
        if name in made:
            return made[name]
        if name == "default":
            made[name] = (eng_mod.DEFAULT_BLOB, dnnw.load_model(eng_mod.DEFAULT_BLOB), None)
            return made[name]
        syn, probe = name.split("/")
        if syn not in base:
            base[syn] = dnnw_synth.synth_model(*SYNTH[syn])
        x_cols = None
        if probe.startswith("window"):
            m = core_ref.window(base[syn], int(probe[6:])); x_cols = core_ref.window_base(int(probe[6:])) + np.arange(84)
        elif probe == "holes":
            m = core_ref.holes(base[syn]); h = core_ref.hidden_columns()
            x_cols = np.full(84, -1); x_cols[core_ref.VISIBLE[:len(h)]] = h
        else:
            m = core_ref.aux(base[syn], float(probe[3:]))
        path = core_ref.write_probe(m, d / (name.replace("/", "_") + ".bin"))
        made[name] = (path, dnnw.load_model(path), x_cols)
        return made[name]
    return get


# ---- the signal and the receiver run ----------------------------------------------------------------------------------------------------------------------------
def make_signal(eng, torch_dev):
    """One recipe for every case: synth_features -> eng.tx -> eng.channel (AWGN at 20 dB Eb/No, a few hertz of offset, a noise lead-in, an end-of-over frame); four
    streams with different features, lead-ins and lengths; stream 3 with faded pilots at 60 dB.  Returns ([B, N] complex64 padded with zeros, n int32 [B])."""
    import torch
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import sigma_from_EbNodB
    feats = np.stack([synth_features(7100 + b, 12 * N_MF) for b in range(B)])
    iq = eng.tx(dev(feats, torch_dev)).cpu().numpy()
    for mf in FADED:
        iq[3, mf * 960:mf * 960 + 192] *= np.float32(1e-4)
    rx = eng.channel(dev(iq, torch_dev), sigma_from_EbNodB(np.array(EBNO)), list(FOFF), n_pre=N_PRE, n_post=1152, with_eoo=True, seed=20240607).cpu().numpy()
    torch.cuda.synchronize()
    return pack([rx[b, LEAD_CUT[b]:rx.shape[1] - TAIL_CUT[b]] for b in range(B)])


def sentinel(shape, torch_dev):
    import torch
    t = torch.empty(shape, dtype=torch.float32, device=torch_dev)
    t.view(torch.int32).fill_(int(np.array(SENT32).view(np.int32)))
    return t


def run_rx(eng, x, n, torch_dev, per_call=False):
    """the receiver over the whole signal in one invocation, or one call per invocation (the rade_rx() usage).  Returns per stream (features [n_valid, 432],
    trace, (consumed, calls, n_valid, has_eoo, nin, state)).  Asserted on the way: rows past n_valid still hold the sentinel, the 16 pad columns of every frame
    are 0.0 exactly, everything else is finite."""
    feats, status = [], []
    if not per_call:
        fo = sentinel((B, CAP, 432), torch_dev)
        _, st, _ = eng.rx(dev(x, torch_dev), n_avail=n, features_out=fo)
        raw = fo.cpu().numpy()
        for b in range(B):
            nv = st[b].n_valid
            assert 0 < nv < CAP and np.all(raw[b, nv:].view(np.uint32) == SENT32), b
            feats.append(raw[b, :nv].copy())
            status.append((st[b].consumed, st[b].n_calls, nv, bool(st[b].has_eoo), st[b].nin, st[b].state))
    else:
        from radae_amd.engine import NIN_MAX
        pos, nin, calls, rows, eoo, st = np.zeros(B, int), np.full(B, 960), np.zeros(B, int), [[] for _ in range(B)], np.zeros(B, bool), None
        while True:
            go = pos + nin <= n
            if not go.any():
                break
            buf = np.zeros((B, NIN_MAX), np.complex64)
            for b in np.flatnonzero(go):
                buf[b, :nin[b]] = x[b, pos[b]:pos[b] + nin[b]]
            fo = sentinel((B, 1, 432), torch_dev)
            _, st, _ = eng.rx(dev(buf, torch_dev), n_avail=np.where(go, nin, 0), max_calls=1, features_out=fo)
            raw = fo.cpu().numpy()
            for b in range(B):
                assert st[b].n_calls == int(go[b]) and st[b].consumed == (nin[b] if go[b] else 0), b
                if st[b].n_valid:
                    rows[b].append(raw[b, 0].copy())
                else:
                    assert np.all(raw[b].view(np.uint32) == SENT32), b
                calls[b] += st[b].n_calls; pos[b] += st[b].consumed; nin[b] = st[b].nin; eoo[b] |= bool(st[b].has_eoo)
        for b in range(B):
            feats.append(np.array(rows[b], np.float32).reshape(-1, 432))
            status.append((int(pos[b]), int(calls[b]), len(rows[b]), bool(eoo[b]), int(nin[b]), st[b].state))
    traces = [eng.rx_trace(b) for b in range(B)]
    for b in range(B):
        f = feats[b].reshape(-1, 12, 36)
        assert np.all(f[:, :, 20:].view(np.uint32) == 0), ("pad columns", b)          # 0.0, not -0.0, not a sentinel
        assert np.isfinite(f).all(), b
        assert len(traces[b]["ret"]) < TRACE_CALLS and int(np.sum(traces[b]["ret"] & 1)) == len(feats[b]) == len(traces[b]["z_hat"]), b
    return feats, traces, status


def dense1_bound(model, z):
    """|K - F| on a column that shows dense1: gemm_bound's forward bound of the K = 80 dot product that dq2_dense1 forms from float32 operands on
    v_mfma_f32_32x32x2_f32 (no operand rounding: r = 0) through the 1-Lipschitz tanh, gate_tanh's measured epsilon, the 22-bit hi + lo planes the result is kept
    in (split16_act: 2^-22 |v|), and the float32 rounding of the output row (the selecting output layer adds one non-zero product, exactly).  [rows, 96]."""
    W, bias, z = np.asarray(model.dec_dense1.w, np.float64), np.asarray(model.dec_dense1.b, np.float64), np.asarray(z, np.float64)
    y64, S = z @ W.T + bias, np.abs(z) @ np.abs(W).T
    return gemm_bound(80, S, y64, 0.0) + EPS_TANH_HW + (2.0 ** -22 + U) * np.abs(np.tanh(y64))


def decode_L(eng, zs, flags, torch_dev):
    """BatchEngine.decode over the streams' k-th segments together, reset once per segment"""
    segs = [core_ref.segments(f) for f in flags]
    out = [np.zeros((len(z), 84), np.float32) for z in zs]
    for k in range(max(len(s) for s in segs)):
        T = max(s[k][1] - s[k][0] for s in segs if len(s) > k)
        zin = np.zeros((B, T, 80), np.float32)
        for b in range(B):
            if len(segs[b]) > k:
                lo, hi = segs[b][k]; zin[b, :hi - lo] = zs[b][lo:hi]
        o = eng.decode(dev(zin, torch_dev), 84, reset=True).cpu().numpy()
        for b in range(B):
            if len(segs[b]) > k:
                lo, hi = segs[b][k]; out[b][lo:hi] = o[b, :hi - lo]
    return out


def decode_S(path, zs, flags):
    from radae_amd.core import CoreDecoder
    dec = CoreDecoder(path, 84)
    try:
        out = []
        for z, f in zip(zs, flags):
            rows = np.zeros((len(z), 84), np.float32)
            for i in range(len(z)):
                if f[i] or i == 0:
                    dec.reset()
                rows[i] = dec.step(z[i])
            out.append(rows)
    finally:
        dec.close()
    return out


# ---- the decoders -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DEC_CASES)
def test_decoders_per_element(engine, torch_dev, blobs, case):
    path, model, x_cols = blobs(case)
    eng = engine(B, max_tx_mf=CAP, blob=path, rx_trace_calls=TRACE_CALLS)
    x, n = make_signal(eng, torch_dev)
    feats, traces, status = run_rx(eng, x, n, torch_dev)
    zs = [t["z_hat"].reshape(-1, 80) for t in traces]
    flags = [core_ref.row_resets(core_ref.resets_from_trace(t["ret"], t["state_before"], t["state_after"])) for t in traces]
    plans = [core_ref.chunk_plan(t) for t in traces]
    print(f"\n[core-model] {case}: status {status}  max |z_hat| {[float(np.abs(z).max()) for z in zs]}")
    assert status[0][3] and not status[1][3] and not status[2][3]                             # the end-of-over frame: seen by stream 0, cut off streams 1 and 2
    assert len({len(z) for z in zs}) >= 3 and all(f[0] for f in flags)
    assert np.abs(zs[3]).max() > 256.0, [float(np.abs(z).max()) for z in zs]            # the faded pilots really produced out-of-range latents

    Fo = [core_ref.Decoder(model).run(z, f) for z, f in zip(zs, flags)]
    F = [o for o, _ in Fo]
    K80 = [f.reshape(-1, 12, 36)[:, :, :20].reshape(-1, 80) for f in feats]                   # the 80 columns of each row that a valid call keeps
    L = decode_L(eng, zs, flags, torch_dev)
    S = decode_S(path, zs, flags)
    vis = core_ref.VISIBLE
    if x_cols is not None:                                                                   # a probe: F's rows are columns of F's x, exactly
        for b in range(B):
            sel = np.flatnonzero((x_cols >= 0) & (np.arange(84) != core_ref.UW_COL))
            assert np.array_equal(F[b][:, sel], Fo[b][1][:, x_cols[sel]])

    # the unique-word sums of the trace from F's column 20 (aux and the probes decide by a margin of 3 or more; the shipped blob at 20 dB decides as F does)
    for b in range(B):
        idx, want = core_ref.uw_errors_from_rows(traces[b], F[b])
        assert len(idx) and np.array_equal(traces[b]["uw_errors"][idx], want), (case, b)
    lost = [int(np.sum((t["state_before"] == 2) & (t["state_after"] == 0) & ((t["ret"] & 1) == 1))) for t in traces]
    mid = [int(np.sum(f & (p[0][:, 0] != 0))) for f, p in zip(flags, plans)]                  # reset flags on a row that is not the first of its chunk
    if case.endswith("aux+4"):
        # every window fails: sync is lost with the failing call's three rows pending, and the re-entry's reset lands on row 3 of a chunk (a bit above bit 0 of rstmask)
        assert min(lost[:3]) >= 1 and max(lost[:3]) >= 2 and min(mid[:3]) >= 1, (lost, mid)
        for b in range(3):
            t = traces[b]
            chk = (t["state_before"] == 2) & (t["synced_count"] % 8 == 0) & (t["synced_count"] > 0)
            assert chk.any() and np.all(t["state_after"][chk] == 0), b
            assert all(p == 3 for p in plans[b][0][np.flatnonzero(flags[b])[1:], 0]), b
    elif case != "default":
        assert sum(lost[:3]) == 0 and all(int(t["uw_errors"].max()) == 0 for t in traces[:3])

    # per element
    # (d1: the visible columns that show dense1: held to the derived bound as well as to the measured rule)
    xv = None if x_cols is None else x_cols[vis]
    d1 = np.zeros(80, bool) if xv is None else (xv >= 0) & (xv < 96)
    e = {"K": 0.0, "L": 0.0, "S": 0.0, "K dense1": 0.0, "L84": 0.0, "S84": 0.0}
    for b in range(B):
        e["L84"] = max(e["L84"], float(np.abs(L[b] - F[b]).max())); e["S84"] = max(e["S84"], float(np.abs(S[b] - F[b]).max()))
        for door, got in (("K", K80[b]), ("L", L[b][:, vis]), ("S", S[b][:, vis])):
            err = np.abs(got.astype(np.float64) - F[b][:, vis])
            e[door] = max(e[door], float(err.max()))
            if door == "K":
                e["K dense1"] = max(e["K dense1"], float(err[:, d1].max(initial=0.0)))
    ratio = e["K"] / max(e["L"], 2.0 ** -24)
    print(f"\n[core-model] {case}: e_K {e['K']:.3e}  e_L {e['L']:.3e}  e_S {e['S']:.3e}  e_K / max(e_L, 2^-24) {ratio:.2f}  e_K on dense1 columns {e['K dense1']:.3e}  all 84 columns: max |L - F| {e['L84']:.3e} max |S - F| {e['S84']:.3e}  "
          f"valid calls {[len(f) for f in feats]}  queues {[p[1] for p in plans]}  lost {lost}  mid-chunk resets {mid}")
    for b in range(B):
        kw = dict(stream=b, chunk_pos=plans[b][0])
        core_ref.check_elements("L", case, L[b], F[b], LIM_L, x_cols=x_cols, **kw)
        core_ref.check_elements("S", case, S[b], F[b], LIM_S, x_cols=x_cols, **kw)
        lim = np.full((len(F[b]), 80), C_K * max(e["L"], 2.0 ** -24))
        if d1.any():
            bound = dense1_bound(model, zs[b])[:, xv[d1]]
            print(f"[core-model] {case}: stream {b} dense1: largest |K - F| / bound {float((np.abs(K80[b][:, d1] - F[b][:, vis][:, d1]) / bound).max()):.3f}, bound {bound.min():.2e} .. {bound.max():.2e}")
            lim[:, d1] = np.minimum(lim[:, d1], bound)
        core_ref.check_elements("K", case, K80[b], F[b][:, vis], lim, out_cols=vis, x_cols=xv, **kw)
    # on top: the bar every door has been held to
    for b in range(B):
        want = core_ref.rows_to_features(F[b])
        for door, got in (("K", feats[b]), ("L", core_ref.rows_to_features(L[b])), ("S", core_ref.rows_to_features(S[b]))):
            assert core_ref.passes_rms_criterion(got, want), (door, case, b)


# ---- how the work is cut ----------------------------------------------------------------------------------------------------------------------------------------
CUTS = [("dec_rows", 3), ("dec_rows", 6), ("dec_rows", 9), ("dec_rows", 12), ("dec_rows", 15), ("dec_rows", 18), ("dec_rows", 21), ("round_calls", 1),
        ("round_calls", 7), ("per_call", 1)]
_baseline = {}


@pytest.mark.parametrize("cut", CUTS, ids=lambda c: f"{c[0]}{c[1]}")
@pytest.mark.parametrize("case", ["default", "synthA/aux+4"])
def test_decoder_stage_is_invariant_to_how_the_rows_are_cut(engine, torch_dev, blobs, monkeypatch, case, cut):
    """K bit for bit -- features, every INT_KEYS entry of the trace, the status -- across RADE_DEC_ROWS (queues of 3, 6, 9, 12 and 12 + 3 .. 12 + 12 rows: with
    +4 the mid-chunk reset at row 3 against the same reset at row 0), RADE_ROUND_CALLS (1, 7, default) and one call per invocation."""
    path = blobs(case)[0]
    for v in ("RADE_DEC_ROWS", "RADE_ROUND_CALLS"):
        monkeypatch.delenv(v, raising=False)
    if case not in _baseline:
        eng = engine(B, max_tx_mf=CAP, blob=path, rx_trace_calls=TRACE_CALLS)
        x, n = make_signal(eng, torch_dev)
        _baseline[case] = (x, n, run_rx(eng, x, n, torch_dev))
        eng.close()
    x, n, (f0, t0, s0) = _baseline[case]
    assert any(24 in core_ref.chunk_plan(t)[1] for t in t0)                                   # the default: 12 + 12
    kind, val = cut
    if kind == "dec_rows":
        monkeypatch.setenv("RADE_DEC_ROWS", str(val))
        assert any(val in core_ref.chunk_plan(t, dec_rows=val)[1] for t in t0)                # a queue of exactly that many rows is decoded
    if kind == "round_calls":
        monkeypatch.setenv("RADE_ROUND_CALLS", str(val))
    eng = engine(B, max_tx_mf=CAP, blob=path, rx_trace_calls=TRACE_CALLS)
    f1, t1, s1 = run_rx(eng, x, n, torch_dev, per_call=(kind == "per_call"))
    for b in range(B):
        assert s1[b] == s0[b], (b, s1[b], s0[b])
        for k in INT_KEYS:
            assert np.array_equal(t1[b][k], t0[b][k]), (b, k)
        assert np.array_equal(t1[b]["z_all"].view(np.uint32), t0[b]["z_all"].view(np.uint32)), b
        assert f1[b].shape == f0[b].shape and np.array_equal(f1[b].view(np.uint32), f0[b].view(np.uint32)), (b, int(np.argmax(np.any(f1[b] != f0[b], axis=1))))


# ---- the encoders -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "synthA/aux-4", "synthB/aux-4"])
def test_encoders_per_element(engine, torch_dev, blobs, case):
    """Engine.encode at B = 1 and B = 3, CoreEncoder.step plain and under bottleneck 1, and k_tx_frame3 (rade_tx: its samples equal, bit for bit, the modulator's
    on the step kernel's latents of the same rows, which is where test_tx_frame3_equals_core_step_and_ofdm_mod takes them) against core_ref.Encoder, 24 steps
    from reset, per element."""
    from radae_amd import api
    from radae_amd.channel_tools import synth_features
    from radae_amd.core import CoreEncoder
    path, model, _ = blobs(case)
    f36 = [synth_features(7300 + b, 96) for b in range(3)]
    rows = np.stack([np.concatenate([f[:, :20], -np.ones((96, 1), np.float32)], 1).reshape(24, 84) for f in f36])      # rade_tx's packing: 4 x (20 features, -1)
    F = [core_ref.Encoder(model).run(r) for r in rows]
    F1 = core_ref.Encoder(model).run(rows[0], bottleneck=1)
    got = {}
    e1 = engine(1, max_tx_mf=8, blob=path)
    got["encode B=1"] = [(0, e1.encode(dev(rows[:1], torch_dev)).cpu().numpy()[0], F[0])]
    e3 = engine(3, max_tx_mf=8, blob=path)
    z3 = e3.encode(dev(rows, torch_dev)).cpu().numpy()
    got["encode B=3"] = [(b, z3[b], F[b]) for b in range(3)]
    enc = CoreEncoder(path, 84)
    try:
        zS = []
        for b in range(3):
            enc.reset()
            zS.append(np.stack([enc.step(r) for r in rows[b]]))
        enc.reset()
        zS1 = np.stack([enc.step(r, bottleneck=1) for r in rows[0]])
    finally:
        enc.close()
    got["step"] = [(b, zS[b], F[b]) for b in range(3)]
    got["step bottleneck 1"] = [(0, zS1, F1)]
    tx = api.radae_tx(model_name=path)
    out = np.zeros((8, 960), np.complex64)
    for k in range(8):
        tx.do_radae_tx(f36[0][12 * k:12 * k + 12].ravel(), out[k])
    tx.h.close()
    ref = e1.tx_latents(dev(zS[0].reshape(1, 24, 80), torch_dev)).cpu().numpy().reshape(8, 960)
    assert np.abs(out).max() > 0.1 and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    got["tx_frame3"] = [(0, zS[0], F[0])]
    line = []
    for door, runs in got.items():
        line.append((door, max(float(np.abs(z.astype(np.float64) - f).max()) for _, z, f in runs)))
    print(f"\n[core-model] encoders {case}: " + "  ".join(f"{d} {v:.3e}" for d, v in line) + f"  max |z| {max(float(np.abs(f).max()) for f in F):.2f}")
    for door, runs in got.items():
        for b, z, f in runs:
            assert z.shape == f.shape and np.abs(f).max() > 0.1
            err = np.abs(z.astype(np.float64) - f)
            r, c = np.unravel_index(int(np.argmax(err)), err.shape)
            assert err[r, c] <= LIM_ENC[door], f"door {door}, blob {case}, stream {b}, step {r}, latent {c}: got {z[r, c]!r}, float64 model {f[r, c]!r}, |difference| {err[r, c]:.3e} > {LIM_ENC[door]:.3e}"
