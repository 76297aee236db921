"""The reference project as the fixture generators use it: where it is, how it is patched, and the drivers they share.

TEST INFRASTRUCTURE -- never imported by the product.  The reference does not exist where the GPU tests run; only the files under tests/golden/ travel there.
Importing this module touches nothing: `find()` locates the reference and `enter()`, which a generator calls first, does once what makes it deterministic:
  * the repository and the reference at the head of `sys.path`, `os.chdir` into the reference (its modules expect cwd-relative imports), one torch thread,
    matplotlib on Agg (MPLBACKEND=Agg for the reference's scripts run as child processes);
and with `patched=True` also
  * `radae.radae_base.n` (radae_base.py:80-81) replaced by clamp-only: the reference adds uniform noise in eval mode, which makes it non-deterministic;
  * `np.random.randint` (used unseeded by dsp.py:293) replaced by the documented LCG x <- x*1664525+1013904223 mod 2^32, row = (x>>8) % Nmf, seed 1, reset by `new_rx`.
Nothing is restored: the command runs every generator in an interpreter of its own (oracle/golden/__main__.py).

Drivers: weights are `weights/model19_check3.bin` (byte copy of the reference's bin/model19_check3.bin), de-quantised by radae_amd.dnnw and loaded into the
reference's own torch modules (`load_into`).  Channel noise: `RADAE.forward` draws torch.randn_like internally (radae.py:578); `channel_case` re-seeds torch and
regenerates the identical tensor so that a fixture can carry the noise explicitly.
"""
import functools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = None                          # set by find()


def find(arg=None):
    """--reference DIR, else $RADAE_REFERENCE, else /root/reference: the first that is given must hold radae/dsp.py."""
    global REF
    d = arg or os.environ.get("RADAE_REFERENCE") or "/root/reference"
    if not os.path.isfile(os.path.join(d, "radae", "dsp.py")):
        sys.exit(f"oracle.golden: no reference at {d} (radae/dsp.py not found): give --reference DIR or set RADAE_REFERENCE")
    REF = os.path.abspath(d)
    return REF


def golden(root, name):
    return os.path.join(root, "tests", "golden", name)


class Lcg:
    def __init__(self, seed=1):
        self.x = seed & 0xFFFFFFFF

    def randint(self, n):
        self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
        return (self.x >> 8) % n


lcg = Lcg(1)


def enter(patched=True):
    os.environ["MPLBACKEND"] = "Agg"
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF or find())
    sys.path.insert(0, REPO)
    import torch
    torch.set_num_threads(1)
    os.chdir(REF)
    if patched:
        import radae.radae_base as rb
        rb.n = lambda x: torch.clamp(x, min=-1.0, max=1.0)
        np.random.randint = lambda n: lcg.randint(n)


def load_into(model, m):
    """De-quantised blob tensors -> reference torch modules."""
    import torch
    enc = model.core_encoder.module
    dec = model.core_decoder.module
    T = torch.tensor
    with torch.no_grad():
        enc.dense_1.weight.copy_(T(m.enc_dense1.w)); enc.dense_1.bias.copy_(T(m.enc_dense1.b))
        enc.z_dense.weight.copy_(T(m.enc_zdense.w)); enc.z_dense.bias.copy_(T(m.enc_zdense.b))
        dec.dense_1.weight.copy_(T(m.dec_dense1.w)); dec.dense_1.bias.copy_(T(m.dec_dense1.b))
        dec.output.weight.copy_(T(m.dec_output.w)); dec.output.bias.copy_(T(m.dec_output.b))
        for i in range(5):
            for mod, G, C in ((enc, m.enc_gru[i], m.enc_conv[i]), (dec, m.dec_gru[i], m.dec_conv[i])):
                g = getattr(mod, f"gru{i+1}")
                g.weight_ih_l0.copy_(T(G.w_ih)); g.weight_hh_l0.copy_(T(G.w_hh))
                g.bias_ih_l0.copy_(T(G.b_ih)); g.bias_hh_l0.copy_(T(G.b_hh))
                c = getattr(mod, f"conv{i+1}").conv
                c.weight.copy_(T(C.w)); c.bias.copy_(T(C.b))
            gate = getattr(dec, f"glu{i+1}").gate
            W = T(m.dec_glu[i].w)
            gate.parametrizations.weight.original1.copy_(W)
            gate.parametrizations.weight.original0.copy_(W.norm(dim=1, keepdim=True))
    model.core_encoder_statefull_load_state_dict()
    model.core_decoder_statefull_load_state_dict()


def c64(x):
    return np.asarray(x).astype(np.complex64)


def with_aux(feat36):
    """(T,36) -> (1,T,21) with the aux symbol -1 appended (radae_txe.py:114-121)."""
    import torch
    f = feat36[:, :20]
    return torch.tensor(np.concatenate([f, -np.ones((f.shape[0], 1), np.float32)], axis=1)[None])


@functools.cache
def m19():
    from radae_amd import dnnw
    return dnnw.load_model(os.path.join(REPO, "weights", "model19_check3.bin"))


def new_tx(**kw):
    import radae_txe
    tx = radae_txe.radae_tx("unused", bypass_enc=True, **kw)
    tx.bypass_enc = False
    tx.n_floats_in = 432
    load_into(tx.model, m19())
    return tx


def new_rx():
    import radae_rxe
    rx = radae_rxe.radae_rx("unused", bypass_dec=True, v=0)
    rx.bypass_dec = False
    rx.n_floats_out = 432
    load_into(rx.model, m19())
    lcg.x = 1
    return rx


def channel_case(name, T, EbNodB, freq_offset, chan, seed, prepend_s=1.0, append_s=0.3, df_dt=0.0):
    """inference.py-equivalent channel simulation through the reference's RADAE.forward
    (radae.py:457-602) + the write_rx tail of inference.py:253-290."""
    import torch
    from radae import RADAE
    from radae_amd.channel_tools import multipath_g, synth_features
    feat36 = synth_features(seed, T)
    model = RADAE(21, 80, EbNodB, rate_Fs=True, freq_offset=freq_offset, df_dt=df_dt, pilots=True, pilot_eq=True,
                  eq_mean6=False, cyclic_prefix=0.004, time_offset=-16, coarse_mag=True, bottleneck=3,
                  correct_freq_offset=True)
    load_into(model, m19())
    model.eval()
    features = with_aux(feat36)
    nRs = model.num_timesteps_at_rate_Rs(T)
    nFs = model.num_timesteps_at_rate_Fs(nRs)
    H = torch.ones((1, nRs, model.Nc))
    if chan == "awgn":
        G = np.ones((nFs, 2), np.complex64); G[:, 1] = 0
    else:
        G = multipath_g(chan, 8000, nFs, seed + 7)
    Gt = torch.tensor(G[None])
    torch.manual_seed(seed)
    with torch.inference_mode():
        out = model(features, H, Gt)
    torch.manual_seed(seed)
    noise = torch.randn(1, nFs, dtype=torch.complex64)
    sigma = float(out["sigma"].item())
    rx = out["rx"]
    assert torch.allclose(rx, (rx - sigma * noise) + sigma * noise)
    # write_rx tail: EOO with continued phase, then real-valued pre/post noise (inference.py:263-284)
    eoo = model.eoo
    freq = torch.zeros_like(eoo)
    freq[:, ] = model.freq_offset * torch.ones_like(eoo) + model.df_dt * torch.arange(eoo.shape[1]) / model.Fs
    omega = freq * 2 * torch.pi / model.Fs
    lin_phase = torch.exp(1j * torch.cumsum(omega, dim=1))
    eoo_rot = eoo * lin_phase * model.final_phase
    n_eoo = torch.randn_like(eoo_rot)
    eoo_rx = eoo_rot + sigma * n_eoo
    n_pre = torch.randn(1, int(model.Fs * prepend_s))
    n_post = torch.randn(1, int(model.Fs * append_s))
    rx_full = torch.concatenate([sigma * n_pre, rx, eoo_rx, sigma * n_post], dim=1)
    d = dict(features=feat36, G=G, noise=c64(noise.numpy()[0]), sigma=np.float64(sigma),
             EbNodB=np.float64(EbNodB), freq_offset=np.float64(freq_offset), df_dt=np.float64(df_dt),
             tx=c64(out["tx"].numpy()[0]), rx=c64(rx.numpy()[0]), noise_eoo=c64(n_eoo.numpy()[0]),
             noise_pre=n_pre.numpy()[0].astype(np.float32), noise_post=n_post.numpy()[0].astype(np.float32),
             rx_full=c64(rx_full.numpy()[0]), z_fwd=out["z_hat"].numpy()[0].astype(np.float32),
             final_phase=c64(model.final_phase.numpy()))
    return d


def run_rx(rx_stream, foff_err=0.0, disable_unsync=0.0):
    """Drive the reference radae_rx exactly like radae_rxe.py:349-356 and record a per-call trace."""
    rx = new_rx()
    rx.foff_err = foff_err
    rx.disable_unsync = disable_unsync          # radae_rxe.py:65, :277-281
    zlog = []
    orig = rx.receiver.receiver_one
    def hook(r, eoo, _o=orig):
        z = _o(r, eoo); zlog.append(z.detach().numpy().reshape(-1).copy()); return z
    rx.receiver.receiver_one = hook
    floats_out = np.zeros(432, np.float32)
    names = ["state_before", "state_after", "nin_before", "nin_after", "ret", "tmax", "f_ind_max", "valid_count",
             "uw_errors", "synced_count", "snr_int"]
    tr = {k: [] for k in names}
    trf = {k: [] for k in ["fmax", "Dthresh", "Dtmax12", "Dtmax12_eoo", "snrdB_3k_est"]}
    z_hat, feats_out, eoo_out = [], [], []
    st = {"search": 0, "candidate": 1, "sync": 2}
    pos = 0
    while pos + rx.get_nin() <= len(rx_stream):
        nin = rx.get_nin()
        buf = np.zeros(rx.get_nin_max(), np.csingle)
        buf[:nin] = rx_stream[pos:pos + nin]
        pos += nin
        sb = st[rx.state]
        ret = rx.do_radae_rx(buf, floats_out)
        tr["state_before"].append(sb); tr["state_after"].append(st[rx.state])
        tr["nin_before"].append(nin); tr["nin_after"].append(rx.get_nin()); tr["ret"].append(int(ret))
        tr["tmax"].append(int(rx.tmax)); tr["f_ind_max"].append(int(rx.acq.f_ind_max) if hasattr(rx.acq, "f_ind_max") else -1)
        tr["valid_count"].append(int(rx.valid_count)); tr["uw_errors"].append(int(rx.uw_errors))
        tr["synced_count"].append(int(rx.synced_count)); tr["snr_int"].append(int(rx.get_snrdB_3k_est()))
        trf["fmax"].append(float(rx.fmax)); trf["Dthresh"].append(float(rx.acq.Dthresh))
        trf["Dtmax12"].append(float(rx.acq.Dtmax12)); trf["Dtmax12_eoo"].append(float(rx.acq.Dtmax12_eoo))
        trf["snrdB_3k_est"].append(float(rx.receiver.snrdB_3k_est))
        if ret & 1:
            z_hat.append(zlog[-1].copy()); feats_out.append(floats_out.copy())
        if ret & 2:
            eoo_out.append(floats_out[:180].copy())
    d = {k: np.array(v, np.int32) for k, v in tr.items()}
    d.update({k: np.array(v, np.float64) for k, v in trf.items()})
    d["z_hat"] = np.array(z_hat, np.float32).reshape(-1, 240)
    d["features_out"] = np.array(feats_out, np.float32).reshape(-1, 432)
    d["eoo_out"] = np.array(eoo_out, np.float32).reshape(-1, 180)
    return d


def thin(tr, every=4):
    """keep features_out / z_hat of every `every`-th valid call (the discrete trace stays whole)"""
    n = len(tr["features_out"])
    rows = np.arange(0, n, every)
    tr = dict(tr)
    tr["rows_kept"] = rows.astype(np.int32); tr["n_valid_total"] = np.int32(n)
    tr["features_out"] = tr["features_out"][rows]; tr["z_hat"] = tr["z_hat"][rows]
    return tr
