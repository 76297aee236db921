"""GPU tests (-m gpu) of batched loss evaluation (rade_batch_loss, rade_loss.hip: loss.py:find_loss over distortion_loss for every stream in one launch,
bit-equal to oracle/rade_oracle.c) and of per-stream channel conditions (rade_batch_channel_streams / rade_batch_tx_channel_streams): stream b of a
per-stream call equals stream b of a uniform call with its values, and a loss-vs-Eb/No curve runs as one batch."""
import glob
import os

import numpy as np
import pytest

from gpu_kit import REPO, engine, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def ragged(arrays, width=36):
    """(rows, <= width) float32 arrays -> one zero-padded [B, max rows, width] batch"""
    out = np.zeros((len(arrays), max(max(len(a) for a in arrays), 1), width), np.float32)
    for b, a in enumerate(arrays):
        out[b, :len(a), :a.shape[1]] = a
    return out


def c20(a):
    """the contiguous 20-column copy oracle.find_loss needs (one stride for both arrays)"""
    return np.ascontiguousarray(np.asarray(a, np.float32)[:, :20])


def golden_pairs(golden):
    """(name, features_in, decoded features as rows of 36) of every rxtrace golden that carries features_in"""
    out = []
    for path in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "rxtrace_*.npz"))):
        g = golden(os.path.basename(path)[:-4])
        if "features_in" in g.files:
            out.append((os.path.basename(path)[8:-4], np.asarray(g["features_in"], np.float32), np.asarray(g["features_out"], np.float32).reshape(-1, 36)))
    return out


def run_loss(eng, torch_dev, fs, hs, **kw):
    import torch
    return eng.loss(torch.tensor(ragged(fs), device=torch_dev), torch.tensor(ragged(hs), device=torch_dev),
                    n_in=[len(f) for f in fs], n_hat=[len(h) for h in hs], **kw)


def dev_bits(x):
    """gpu_kit.bits without the copy to the host: int32 words on the device, for torch.equal"""
    import torch
    return torch.view_as_real(x).contiguous().view(torch.int32) if x.is_complex() else x.contiguous().view(torch.int32)


def test_loss_parity_ragged_golden_batch(engine, torch_dev, golden, oracle):
    """nine streams of 168..6000 input rows (20 or 36 columns) in one call: loss bit-equal to the oracle as a double, the same start; numpy within 1e-6"""
    from radae_amd.loss import find_loss
    pairs = golden_pairs(golden)
    assert len(pairs) == 9 and {p[1].shape[1] for p in pairs} == {20, 36} and max(len(p[1]) for p in pairs) == 6000
    eng = engine(len(pairs))
    loss, start, fl = run_loss(eng, torch_dev, [p[1] for p in pairs], [p[2] for p in pairs])
    assert fl is None and loss.dtype == np.float64
    for b, (name, f, h) in enumerate(pairs):
        lo, so = oracle.find_loss(c20(f), c20(h))
        assert loss[b] == lo and start[b] == so, (name, loss[b], lo, start[b], so)
        ln, sn = find_loss(f, h)
        assert sn == so and abs(ln - lo) <= 1e-6 * lo, (name, ln, lo)


def test_frame_loss_curve(engine, torch_dev, golden, oracle):
    """loss.py:85-90: distortion_loss of each frame pair at the chosen start, n_hat - start frames, bit-equal to the oracle's; NaN after"""
    pairs = golden_pairs(golden)
    eng = engine(len(pairs))
    loss, start, fl = run_loss(eng, torch_dev, [p[1] for p in pairs], [p[2] for p in pairs], frame_loss=True)
    fl = fl.cpu().numpy()
    assert fl.shape == (len(pairs), max(len(p[2]) for p in pairs))
    assert any(start[b] >= len(p[2]) for b, p in enumerate(pairs))                 # (a start past n_hat leaves no frame to plot)
    for b, (name, f, h) in enumerate(pairs):
        s = int(start[b]); n = max(len(h) - s, 0)
        want = np.array([oracle.distortion_loss(c20(f[s + k:s + k + 1]), c20(h[k:k + 1])) for k in range(n)])
        assert np.array_equal(fl[b, :n].astype(np.float64), want), name
        assert np.all(np.isnan(fl[b, n:])), name


def test_edge_cases(engine, torch_dev, oracle):
    from radae_amd.channel_tools import synth_features
    rng = np.random.default_rng(5)
    base = synth_features(11, 400)
    noisy = lambda a: (a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32)
    period = np.tile(synth_features(12, 10), (40, 1))                             # 400 rows of period 10: offsets s and s + 10 give bit-equal losses
    cases = [
        ("regular", base[:300], noisy(base[37:237])),
        ("n_hat == n_in", base[:100], noisy(base[:100])),
        ("n_hat == 0", base[:100], base[:0]),
        ("regular 2", base[50:350], noisy(base[120:300])),
        ("n_hat > n_in", base[:30], noisy(base[:40])),
        ("n_hat == 1", base[:50], base[20:21]),
        ("best at n_in - n_hat", base[:120], base[80:120]),                          # exact match only at the offset the reference never tries
        ("tied offsets", period[:300], noisy(period[23:223])),
    ]
    eng = engine(len(cases))
    loss, start, _ = run_loss(eng, torch_dev, [c[1] for c in cases], [c[2] for c in cases])
    for b, (name, f, h) in enumerate(cases):
        if not 0 < len(h) <= len(f):
            assert np.isnan(loss[b]) and start[b] == -1, name
            continue
        lo, so = oracle.find_loss(c20(f), c20(h))
        assert loss[b] == lo and start[b] == so, (name, loss[b], lo, start[b], so)
    assert start[1] == 0 and start[5] == 20 and loss[5] == 0.0
    assert start[6] != 80 and loss[6] > 0.0
    assert oracle.distortion_loss(c20(period[3:203]), c20(cases[7][2])) == oracle.distortion_loss(c20(period[13:213]), c20(cases[7][2]))
    assert start[7] == 3                                                           # the earliest of the tied offsets 3, 13, 23, ...


def test_clip_start_clip_end(engine, torch_dev, golden, oracle):
    """loss.py --clip_start / --clip_end: features_hat[clip_start : n_hat - clip_end]; a stream clipped to nothing is not scored"""
    pairs = golden_pairs(golden)
    fs, hs = [p[1] for p in pairs], [p[2] for p in pairs]
    hs[0] = hs[0][:20]                                                            # 20 rows: nothing left after clipping 12 + 10
    eng = engine(len(pairs))
    loss, start, fl = run_loss(eng, torch_dev, fs, hs, clip_start=12, clip_end=10, frame_loss=True)
    assert np.isnan(loss[0]) and start[0] == -1 and np.all(np.isnan(fl[0].cpu().numpy()))
    for b in range(1, len(pairs)):
        lo, so = oracle.find_loss(c20(fs[b]), c20(hs[b][12:len(hs[b]) - 10]))
        assert loss[b] == lo and start[b] == so, pairs[b][0]


def test_stream_results_do_not_depend_on_the_batch(engine, torch_dev, golden):
    """a stream alone (B = 1) gives what it gives inside B = 64 with other lengths around it, bit for bit (frame curve included)"""
    pairs = golden_pairs(golden)
    B = 64
    fs = [pairs[b % 9][1][b // 9:] for b in range(B)]
    hs = [pairs[b % 9][2][:max(len(pairs[b % 9][2]) - 11 * (b // 9), 0)] for b in range(B)]
    eng = engine(B)
    loss, start, fl = run_loss(eng, torch_dev, fs, hs, frame_loss=True)
    fl = fl.cpu().numpy()
    one = engine(1)
    for b in range(B):
        l1, s1, f1 = run_loss(one, torch_dev, [fs[b]], [hs[b]], frame_loss=True)
        assert np.array_equal(l1, loss[b:b + 1], equal_nan=True) and s1[0] == start[b], b
        n = f1.shape[1]
        assert np.array_equal(f1.cpu().numpy()[0], fl[b, :n], equal_nan=True), b
    assert np.sum(start >= 0) >= 48


SIG = np.float32([0.0, 0.05, 0.1, 0.2, 0.3, 0.15, 0.07, 0.4])
FOFF = np.float32([0.0, -11.0, 5.5, 20.0, -3.25, 0.0, 37.0, -50.0])
DFDT = np.float32([0.0, 0.5, -0.8, 0.0, 1.5, -2.0, 0.25, 0.0])


def test_per_stream_channel_equals_uniform_channel(engine, torch_dev):
    """B = 8, eight distinct (sigma, freq_offset, df_dt) triples: stream b of the per-stream call is bit-equal to stream b of a uniform call with its values --
    with and without G, noise framing and the EOO frame, explicit noise and Philox, rade_batch_channel and both paths of rade_batch_tx_channel"""
    import torch
    from radae_amd.channel_tools import synth_features
    B, n_mf = 8, 4
    n_sig = n_mf * 960
    eng = engine(B, max_tx_mf=n_mf)
    feats = torch.tensor(np.stack([synth_features(100 + b, 12 * n_mf) for b in range(B)]), device=torch_dev)
    eng.tx_reset()
    iq = eng.tx(feats)
    G = eng.multipath_gen("mpp", n_sig, seed=3)
    gen = torch.Generator(device=torch_dev).manual_seed(4)
    for G_, pre, post, eoo, explicit in [(None, 0, 0, False, False), (G, 0, 0, False, True), (None, 800, 1152, True, True), (G, 800, 1152, True, False)]:
        kw = dict(n_pre=pre, n_post=post, with_eoo=eoo, G=G_)
        if explicit:
            kw["noise"] = torch.randn((B, pre + n_sig + (1152 if eoo else 0) + post), dtype=torch.complex64, device=torch_dev, generator=gen)
        else:
            kw["seed"] = 77
        per = eng.channel(iq, SIG, FOFF, df_dt=DFDT, **kw)
        for b in range(B):
            uni = eng.channel(iq, float(SIG[b]), float(FOFF[b]), df_dt=float(DFDT[b]), **kw)
            assert torch.equal(dev_bits(per[b]), dev_bits(uni[b])), ("channel", G_ is not None, pre, explicit, b)
    for G_ in (G, None):                                                          # fused modulator + channel; the two calls back to back
        kw = dict(n_pre=800, n_post=1152, with_eoo=True, G=G_, seed=5)
        eng.tx_reset()
        per = eng.tx_channel(feats, SIG, FOFF, df_dt=DFDT, **kw)
        for b in range(B):
            eng.tx_reset()
            uni = eng.tx_channel(feats, float(SIG[b]), float(FOFF[b]), df_dt=float(DFDT[b]), **kw)
            assert torch.equal(dev_bits(per[b]), dev_bits(uni[b])), ("tx_channel", G_ is not None, b)
    # a scalar among sequences is every stream's value; a wrong B is refused before anything runs
    part = eng.channel(iq, SIG, 0.0, G=G, seed=77)
    assert torch.equal(dev_bits(part[3]), dev_bits(eng.channel(iq, float(SIG[3]), 0.0, G=G, seed=77)[3]))
    with pytest.raises(ValueError):
        eng.channel(iq, SIG[:7], 0.0)


def test_loss_curve_in_one_batch(engine, torch_dev):
    """4 Eb/No points x {AWGN, MPP} x 2 utterances = 16 streams through one tx_channel -> rx -> loss pass.  Each condition applied uniformly to the same
    batch (same features, G, seed) gives its streams bit-equal decoded features; every stream's device loss and start equal numpy find_loss's."""
    import torch
    from radae_amd.channel_tools import synth_features
    from radae_amd.engine import sigma_from_EbNodB
    from radae_amd.loss import find_loss
    B, n_mf = 16, 12
    n_sig = n_mf * 960
    conds = [(e, ch, u) for e in (0.0, 3.0, 6.0, 10.0) for ch in ("awgn", "mpp") for u in range(2)]
    sig = sigma_from_EbNodB(np.float32([c[0] for c in conds]))
    foff = np.float32([0.0 if c[1] == "awgn" else -11.0 for c in conds])
    dfdt = np.zeros(B, np.float32)
    feats_np = np.stack([synth_features(500 + c[2], 12 * n_mf) for c in conds])
    feats = torch.tensor(feats_np, device=torch_dev)
    eng = engine(B, max_tx_mf=n_mf)
    G = eng.multipath_gen("mpp", n_sig, seed=9)
    awgn = [b for b, c in enumerate(conds) if c[1] == "awgn"]
    G[awgn, :, 0] = 1.0                                                           # G covers all streams or none: (1, 0) rows for the AWGN streams
    G[awgn, :, 1] = 0.0

    def run(s, f, d):
        eng.reset()
        rx = eng.tx_channel(feats, s, f, df_dt=d, n_pre=1600, n_post=1152, with_eoo=True, G=G, seed=21)
        fo, st, _ = eng.rx(rx)
        return fo, st
    fo, st = run(sig, foff, dfdt)
    loss, start, _ = eng.loss(feats, fo)                                          # n_hat = 12 x n_valid of that rx() call
    fo_np = fo.cpu().numpy()
    scored = 0
    for b in range(B):
        h = fo_np[b, :st[b].n_valid].reshape(-1, 36)
        if not 0 < len(h) <= 12 * n_mf:
            assert np.isnan(loss[b]) and start[b] == -1, b
            continue
        ln, sn = find_loss(feats_np[b], h)
        assert start[b] == sn and abs(loss[b] - ln) <= 1e-6 * ln, (conds[b], loss[b], ln, start[b], sn)
        scored += 1
    assert scored >= 12
    for k in range(0, B, 2):                                                      # each condition: streams k, k + 1 (the two utterances)
        fu, su = run(float(sig[k]), float(foff[k]), float(dfdt[k]))
        for b in (k, k + 1):
            n = st[b].n_valid
            assert su[b].n_valid == n and torch.equal(dev_bits(fu[b, :n]), dev_bits(fo[b, :n])), conds[b]
