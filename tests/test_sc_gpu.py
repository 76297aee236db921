"""GPU parity tests (-m gpu) of the single-carrier modem for BBFM symbols (reference radae/dsp.py:579-860)."""
import numpy as np
import pytest

from gpu_kit import torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


SC_RX_CASES = ["clean", "noisy_foff", "drift", "drift_pos", "lose_sync"]


@pytest.mark.gpu
def test_sc_rrc_and_tx_golden(torch_dev, golden):
    import torch
    from radae_amd.sc import SingleCarrierBatch
    for name in ("bpsk_1500", "analog_0"):
        g = golden("sc_tx_" + name)
        m = SingleCarrierBatch(2, fcentreHz=float(g["fcentre"]))
        assert np.abs(m.rrc() - g["rrc"]).max() < 1e-12
        sy = torch.tensor(np.stack([g["symbs"], g["symbs"][::-1].copy()]), device=torch_dev)
        # two calls (3 + rest frames): filter memory and LO phase carry across calls
        a = m.tx(sy[:, :3].contiguous()); b = m.tx(sy[:, 3:].contiguous())
        tx = torch.cat([a, b], dim=1).cpu().numpy()
        assert np.abs(tx[0] - g["tx"].reshape(-1)).max() < 2e-6
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC_RX_CASES)
def test_sc_rx_golden(torch_dev, golden, name):
    """HIP receiver against the reference's per-frame outputs: discrete outputs exact, symbols to 1e-5."""
    import torch
    from radae_amd.sc import SingleCarrierBatch
    g = golden("sc_rx_" + name)
    m = SingleCarrierBatch(1, fcentreHz=float(g["fcentre"]))
    pay, zh, fr, st = m.rx(torch.tensor(g["rx_in"][None], device=torch_dev))
    nf = st[0].n_frames
    assert nf == len(g["state"]) and st[0].consumed == int(g["consumed"])
    f = fr[0, :nf]
    for k in ("state", "nin", "fs_s"):
        assert np.array_equal(f[k], g[k]), k
    assert np.abs(f["norm_rx_timing"] - g["norm_rx_timing"]).max() < 1e-5
    assert np.abs(f["phase_ambiguity"] - g["phase_ambiguity"]).max() < 1e-6
    assert np.abs(f["g"] - g["g"]).max() < 1e-5 * np.abs(g["g"]).max()
    assert np.abs((f["max_cs_re"] + 1j * f["max_cs_im"]) - g["max_Cs"]).max() < 1e-5
    p = pay.cpu().numpy()[0, :nf]
    assert np.abs(p - g["payload"]).max() < 1e-5 * max(1.0, np.abs(g["payload"]).max())
    z = zh.cpu().numpy()[0, :nf]
    ref = np.where(g["state"][:, None] == 1, g["g"][:, None] * g["payload"].real, 0.0)
    assert np.abs(z - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    m.close()


@pytest.mark.gpu
def test_sc_loopback_batch_vs_oracle_and_chunking(torch_dev):
    """64 streams with different symbols / impairments: tx on the GPU == oracle tx; rx frame by frame (one call per frame,
    the sc_rx.py usage) == whole stream at once == oracle; bit errors of the synced frames are zero at this SNR."""
    import torch
    from oracle import sc_oracle as SC
    from radae_amd.sc import SingleCarrierBatch
    B, NF = 64, 10
    rng = np.random.default_rng(5)
    sy = (1 - 2 * (rng.random((B, NF, 80)) > 0.5)).astype(np.float32)
    m = SingleCarrierBatch(B, fcentreHz=1500.0)
    tx = m.tx(torch.tensor(sy, device=torch_dev)).cpu().numpy()
    for b in (0, 17, 63):
        o = SC.SingleCarrier(fcentreHz=1500.0)
        assert np.abs(np.concatenate([o.tx(s) for s in sy[b]]) - tx[b]).max() < 2e-6
    n = tx.shape[1]
    t = np.arange(n)
    rx = np.zeros((B, n + 64), np.complex64)
    for b in range(B):
        lead = int(rng.integers(0, 64))
        ph = 2 * np.pi * rng.uniform(-2, 2) * t / 9600 + rng.uniform(-3, 3)
        y = (0.3 + 2 * rng.random()) * (tx[b] * np.exp(1j * ph) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))
        rx[b, lead:lead + n] = y
    rxd = torch.tensor(rx, device=torch_dev)
    pay, zh, fr, st = m.rx(rxd)
    nf = st[0].n_frames
    assert all(s.n_frames == nf and s.consumed == nf * 384 or abs(s.consumed - nf * 384) <= nf for s in st)
    for b in (0, 17, 40, 63):
        o = SC.SingleCarrier(fcentreHz=1500.0)
        out, consumed = SC.run_rx_stream(o, rx[b])
        k = st[b].n_frames
        assert k == len(out["state"]) and consumed == st[b].consumed
        for key in ("state", "nin", "fs_s"):
            assert np.array_equal(fr[b, :k][key], out[key]), key
        assert np.abs(pay.cpu().numpy()[b, :k] - out["payload"]).max() < 2e-5 * max(1.0, np.abs(out["payload"]).max())
    # payload bits of synced frames: frame i of the receiver carries tx frame i - 1 or i - 2 depending on the lead
    z = zh.cpu().numpy(); errs = 0; bits = 0
    for b in range(B):
        for i in range(2, st[b].n_frames):
            if fr[b, i]["state"] == 1:
                best = min(int(np.sum(z[b, i] * sy[b, j] < 0)) for j in range(NF))
                errs += best; bits += 80
    assert bits > B * 5 * 80 and errs == 0
    # one frame per call == all at once
    # (streams slip independently, so the frame-by-frame run uses stream 0 alone)
    m1 = SingleCarrierBatch(1, fcentreHz=1500.0)
    p0 = 0; outs = []; nin = 384
    while p0 + nin <= rx.shape[1]:
        p, _, f1, s1 = m1.rx(rxd[:1, p0:p0 + nin].contiguous(), max_frames=1)
        assert s1[0].n_frames == 1 and s1[0].consumed == nin
        outs.append(p.cpu().numpy()[0, 0]); p0 += nin; nin = s1[0].nin
    assert len(outs) == st[0].n_frames
    assert np.array_equal(np.stack(outs), pay.cpu().numpy()[0, :len(outs)])
    m.close(); m1.close()


@pytest.mark.gpu
def test_sc_edge_cases(torch_dev, golden):
    """Short input (no whole frame), max_frames cap, reset, and argument checking of the single-carrier entry points."""
    import torch
    from radae_amd.sc import SingleCarrierBatch
    g = golden("sc_rx_clean")
    x = torch.tensor(g["rx_in"][None], device=torch_dev)
    m = SingleCarrierBatch(1, fcentreHz=float(g["fcentre"]))
    pay, zh, fr, st = m.rx(x[:, :383].contiguous(), max_frames=4)          # fewer than nin samples: nothing consumed
    assert st[0].n_frames == 0 and st[0].consumed == 0 and st[0].nin == 384 and st[0].state == 0
    pay, zh, fr, st = m.rx(x, max_frames=3)                                   # capped: the caller resumes at `consumed`
    assert st[0].n_frames == 3 and st[0].consumed == int(np.sum(np.concatenate([[384], g["nin"][:2]])))
    pay2, zh2, fr2, st2 = m.rx(x[:, st[0].consumed:].contiguous())
    nf = len(g["state"])
    assert st2[0].n_frames == nf - 3
    assert np.array_equal(np.concatenate([fr[0, :3]["state"], fr2[0, :nf - 3]["state"]]), g["state"])
    p = np.concatenate([pay.cpu().numpy()[0, :3], pay2.cpu().numpy()[0, :nf - 3]])
    assert np.abs(p - g["payload"]).max() < 1e-5
    m.reset()                                                                  # back to the constructor state: same answer again
    pay3, _, fr3, st3 = m.rx(x)
    assert st3[0].n_frames == nf and np.abs(pay3.cpu().numpy()[0, :nf] - g["payload"]).max() < 1e-5
    # argument errors are reported, not crashed on
    L = m.L
    assert L.rade_sc_tx(m.h, None, 1, None, 384, None) == -1
    assert L.rade_sc_rx(m.h, None, 0, 0, 1, None, None, None, None, None) == -1
    assert not L.rade_sc_open(0, 2400.0, 9600.0, 0.0, 0.25, 0)
    assert not L.rade_sc_open(1, 2400.0, 8000.0, 0.0, 0.25, 0)              # Fs must be 4 Rs
    m.close()


@pytest.mark.gpu
def test_sc_wire_filters_match_reference_scripts(golden):
    """latents | sc_tx | sc_rx with the reference's own scripts (tests/golden/sc_wire.npz) vs the GPU filters: int16 samples equal up
    to the truncation of values within float rounding of an integer, z_hat equal to the quantisation noise that leaves."""
    from radae_amd.sc import sc_tx_stream, sc_rx_stream
    g = golden("sc_wire")
    t = sc_tx_stream(g["z"])
    assert t.dtype == np.int16 and t.shape == g["t_int16"].shape
    d = np.abs(t.astype(int) - g["t_int16"].astype(int))
    assert d.max() <= 1 and (d == 0).mean() > 0.97
    zh = sc_rx_stream(g["t_int16"])                       # the reference's samples in: isolates the receiver
    assert zh.shape == g["zhat"].shape and np.abs(zh - g["zhat"]).max() < 2e-5 * max(1.0, np.abs(g["zhat"]).max())
    zh2 = sc_rx_stream(t)                                  # our own samples: +-1 LSB differences only
    assert zh2.shape == g["zhat"].shape and np.abs(zh2 - g["zhat"]).max() < 2e-3
