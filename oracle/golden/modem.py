"""The model19 modem end to end, made by IMPORTING the reference: constants, encoder + transmitter, channel + receiver traces, the ctests' test-mode knobs,
decoder + loss, the model05 and BBFM configurations, the int16 wire converters.  How the reference is driven and what is patched: oracle/golden/reference.py.

(weights_check.npz belongs to dnnw_export.py: from a checkpoint run through the reference's own exporter, not from radae_amd/dnnw.py's reading of model19_check3.bin.)
"""
import os
import sys

import numpy as np

from . import reference as R
from .reference import c64, channel_case, golden, load_into, new_rx, new_tx, run_rx, with_aux


def gen_consts(src, dst):
    R.enter()
    import torch
    tx = new_tx()
    rx = new_rx()
    md = tx.model
    rng = np.random.default_rng(65647)
    bits = np.sign(rng.random(180) - 0.5).astype(np.float32)
    eoo_default = c64(md.eoo.numpy().flatten())
    md.set_eoo_bits(torch.tensor(bits))
    eoo_bits = c64(md.eoo.numpy().flatten())
    np.savez(
        golden(dst, "consts.npz"),
        w=md.w.numpy().astype(np.float32), Winv=c64(md.Winv.numpy()), Wfwd=c64(md.Wfwd.numpy()),
        P=c64(md.P.numpy()), Pend=c64(md.Pend.numpy()), p=c64(md.p.numpy()), pend=c64(md.pend.numpy()),
        p_cp=c64(md.p_cp.numpy()), pend_cp=c64(md.pend_cp.numpy()),
        pilot_gain=np.float64(md.pilot_gain),
        eoo_default=eoo_default, eoo_bits_in=bits, eoo_with_bits=eoo_bits,
        Pmat=c64(rx.receiver.Pmat.numpy()),
        bpf_h=c64(rx.bpf.h), bpf_alpha=np.float64(rx.bpf.alpha), bpf_phase_vec_exp=c64(rx.bpf.phase_vec_exp[:1120]),
        acq_p_w=c64(rx.acq.p_w), acq_fcoarse=rx.acq.fcoarse_range.astype(np.float64), acq_sigma_p=np.float64(rx.acq.sigma_p),
        Nmf=np.int32(rx.Nmf), Nmf_unsync=np.int32(rx.Nmf_unsync),
    )
    print("consts ok")


def gen_enc_tx(src, dst):
    """Encoder (stateful, 12 frames per call = radae_txe.do_radae_tx) + transmitter_one."""
    R.enter()
    import torch
    from radae_amd.channel_tools import synth_features
    nutt, T = 2, 120
    feats = np.stack([synth_features(100 + u, T) for u in range(nutt)])  # (2,120,36)
    z_all, tx_all, z_stateless = [], [], []
    for u in range(nutt):
        tx = new_tx()
        out = np.zeros(960, np.csingle)
        zs, txs = [], []
        enc = tx.model.core_encoder_statefull
        orig = enc.forward
        def hook(x, _o=orig, _zs=zs):
            z = _o(x); _zs.append(z.detach().numpy().copy()); return z
        enc.forward = hook
        for k in range(T // 12):
            tx.do_radae_tx(feats[u, 12 * k:12 * k + 12].flatten(), out)
            txs.append(out.copy())
        enc.forward = orig
        z_all.append(np.concatenate(zs, axis=1)[0])
        tx_all.append(np.stack(txs))
        with torch.inference_mode():
            z_stateless.append(tx.model.core_encoder(with_aux(feats[u])).numpy()[0])
        if u == 0:
            mod = tx.model.core_encoder_statefull.module
            gru_states = np.stack([getattr(mod, f"gru{i}").states.numpy().reshape(-1) for i in range(1, 6)])
            conv_states = [getattr(mod, f"conv{i}").states.numpy()[0] for i in range(1, 6)]
    np.savez(golden(dst, "enc_tx.npz"), features=feats, z=np.stack(z_all).astype(np.float32),
             z_stateless=np.stack(z_stateless).astype(np.float32), tx=c64(np.stack(tx_all)),
             gru_states_u0=gru_states.astype(np.float32),
             **{f"conv{i+1}_state_u0": conv_states[i].astype(np.float32) for i in range(5)})
    d = np.abs(np.stack(z_all) - np.stack(z_stateless)).max()
    print(f"enc_tx ok  (stateful vs stateless max diff {d:.2e})")


def gen_chan_rx(src, dst):
    R.enter()
    from scipy.signal import resample_poly
    cases = {
        # name: (T frames, EbNodB, freq_offset, channel, seed, prepend_s)
        "mpp": (240, 3.0, -11.0, "mpp", 1000, 1.0),       # config 3 / ctest radae_rx_mpp
        "awgn": (168, 10.0, 11.0, "awgn", 1001, 1.0),     # ctest radae_rx_basic
    }
    for name, (T, eb, fo, ch, seed, pre) in cases.items():
        d = channel_case(name, T, eb, fo, ch, seed, prepend_s=pre)
        tr = run_rx(d["rx_full"])
        np.savez_compressed(golden(dst, f"chan_{name}.npz"), **d)
        np.savez_compressed(golden(dst, f"rxtrace_{name}.npz"), rx_in=d["rx_full"], features_in=d["features"], **tr)
        print(f"chan/rx {name}: calls {len(tr['ret'])} valid {int((tr['ret'] & 1).sum())} eoo {int((tr['ret'] >> 1).sum())}"
              f" states {tr['state_after'].tolist()}")
    # timing slips (ctests radae_rx_slip_plus / _minus) -- sox is absent, scipy polyphase resampler instead
    for name, (up, dn, pre) in {"slip_plus": (1601, 1600, 0.06425), "slip_minus": (1599, 1600, 0.10675)}.items():
        d = channel_case(name, 480, 10.0, 11.0, "awgn", 1002, prepend_s=pre, append_s=0.3)
        x = d["rx_full"]
        xr = (resample_poly(x.real.astype(np.float64), up, dn) + 1j * resample_poly(x.imag.astype(np.float64), up, dn)).astype(np.complex64)
        tr = run_rx(xr)
        np.savez_compressed(golden(dst, f"rxtrace_{name}.npz"), rx_in=xr, features_in=d["features"], **tr)
        print(f"rx {name}: calls {len(tr['ret'])} valid {int((tr['ret'] & 1).sum())} nin set {sorted(set(tr['nin_after'].tolist()))}"
              f" tmax range {tr['tmax'].min()}..{tr['tmax'].max()}")
    # false-sync / UW failure path: rade_api.c:263-264 RADE_FOFF_TEST => foff_err = 10 Hz on first sync
    d = channel_case("foff", 240, 10.0, 11.0, "awgn", 1003, prepend_s=0.5)
    tr = run_rx(d["rx_full"], foff_err=10.0)
    np.savez_compressed(golden(dst, "rxtrace_foff.npz"), rx_in=d["rx_full"], features_in=d["features"], **tr)
    print(f"rx foff: states {tr['state_after'].tolist()} uw {tr['uw_errors'].tolist()}")


def gen_knobs(src, dst):
    """The test-mode knobs the reference's ctests use and the first fixture set left at their defaults:
    df_dt (frequency drift, radae.py:547-552 + inference.py:270; ctest radae_rx_dfdt, CMakeLists.txt:363-371) and
    --disable_unsync (radae_rxe.py:277-281; ctests radae_rx_mpp / radae_rx_mpg, CMakeLists.txt:326-347)."""
    R.enter()
    keep = ("features", "noise", "sigma", "EbNodB", "freq_offset", "df_dt", "tx", "rx", "noise_eoo", "noise_pre", "noise_post", "rx_full", "final_phase")
    for name, dfdt in (("dfdt_pos", 0.5), ("dfdt_neg", -0.5)):
        d = channel_case(name, 120, 10.0, 13.0, "awgn", 1010, prepend_s=0.5, append_s=0.2, df_dt=dfdt)
        np.savez_compressed(golden(dst, f"chan_{name}.npz"), **{k: d[k] for k in keep})
        print(f"chan {name}: final phase {d['final_phase']}")
    # receiver trace through a drifting offset, the ctest's recipe at reduced length (Eb/No 1 dB, +13 Hz, 0.1 Hz/s)
    d = channel_case("dfdt", 240, 1.0, 13.0, "awgn", 1011, prepend_s=1.0, append_s=0.3, df_dt=0.1)
    tr = run_rx(d["rx_full"])
    np.savez_compressed(golden(dst, "rxtrace_dfdt.npz"), rx_in=d["rx_full"], features_in=d["features"], **tr)
    print(f"rx dfdt: calls {len(tr['ret'])} valid {int((tr['ret'] & 1).sum())} fmax {tr['fmax'][[10, -3]]}")
    # --disable_unsync: MPP at 0 dB with a deep fade, unsync paths switched off after 0.5 s of sync (41 frames at the ctest's 5 s
    # would outlast a short fixture); the same samples without the flag lose sync, so the pair pins both branches
    d = channel_case("nounsync", 504, 0.0, -11.0, "mpp", 1012, prepend_s=0.5, append_s=0.3)
    x = d["rx_full"].copy()
    n0 = int(0.5 * 8000) + 14 * 960                     # 14 frames into the signal: 27 frames of noise only (valid_count runs out after 25)
    x[n0:n0 + 27 * 960] = d["sigma"] * d["noise"][:27 * 960]
    tr_on = run_rx(x, disable_unsync=0.5); tr_off = run_rx(x)
    assert not np.array_equal(tr_on["state_after"], tr_off["state_after"]), "fixture does not exercise the flag"
    np.savez_compressed(golden(dst, "rxtrace_nounsync.npz"), rx_in=c64(x), features_in=d["features"], disable_unsync=np.float64(0.5), **tr_on)
    print(f"rx nounsync: states with flag {tr_on['state_after'].tolist()}\n            without {tr_off['state_after'].tolist()}")


def gen_dec_loss(src, dst):
    R.enter()
    import torch
    from radae import distortion_loss
    rng = np.random.default_rng(5)
    g = np.load(golden(src, "rxtrace_awgn.npz"))
    z = g["z_hat"][:10].reshape(1, 30, 80)
    rx = new_rx()
    dec = rx.model.core_decoder_statefull
    outs = []
    with torch.inference_mode():
        for k in range(10):
            outs.append(dec(torch.tensor(z[:, 3 * k:3 * k + 3])).numpy()[0])
        stateless = rx.model.core_decoder(torch.tensor(z)).numpy()[0]
    feats = np.concatenate(outs)  # (120,21)
    mod = dec.module
    gru_states = np.stack([getattr(mod, f"gru{i}").states.numpy().reshape(-1) for i in range(1, 6)])
    a = torch.tensor(rng.standard_normal((1, 50, 20)).astype(np.float32))
    b = torch.tensor(rng.standard_normal((1, 50, 20)).astype(np.float32))
    a21 = torch.tensor(rng.standard_normal((1, 50, 21)).astype(np.float32))
    b21 = torch.tensor(rng.standard_normal((1, 50, 21)).astype(np.float32))
    np.savez(golden(dst, "dec_loss.npz"), z_hat=z[0].astype(np.float32), features=feats.astype(np.float32),
             features_stateless=stateless.astype(np.float32), gru_states=gru_states.astype(np.float32),
             la=a.numpy()[0], lb=b.numpy()[0], loss20=np.float64(distortion_loss(a, b).item()),
             la21=a21.numpy()[0], lb21=b21.numpy()[0], loss21=np.float64(distortion_loss(a21, b21).item()))
    print(f"dec ok (stateful vs stateless max diff {np.abs(feats - stateless).max():.2e})")


def gen_model05(src, dst):
    """Config 1: inference.py plumbing with model05 -- RADAE(20, 80, EbNodB) defaults: rate Rs, Nc=20, Ns=6, no
    pilots, bottleneck 1 (radae.py:604-634).  H = 1 (AWGN) and a multipath-magnitude H."""
    R.enter()
    import torch
    from radae import RADAE, distortion_loss
    from radae_amd import dnnw
    from radae_amd.channel_tools import synth_features
    m05 = dnnw.load_model(os.path.join(R.REPO, "weights", "model05.bin"))
    T = 900                                                  # 9.0 s, stand-in for wav/peter.wav
    feat36 = synth_features(2000, T)
    features = torch.tensor(feat36[None, :, :20])
    out = {}
    for tag, EbNodB, use_h in (("awgn", 10.0, False), ("mp", 6.0, True)):
        model = RADAE(20, 80, EbNodB)
        load_into(model, m05)
        model.eval()
        nRs = model.num_timesteps_at_rate_Rs(T)
        H = torch.ones((1, nRs, model.Nc))
        if use_h:                                            # inference.py --mp_test style magnitudes (:133-143)
            for c in range(model.Nc):
                H[0, :, c] = abs(1 + np.exp(-1j * 2 * np.pi * c * 0.002 * model.Rs))
        torch.manual_seed(77)
        with torch.inference_mode():
            o = model(features, H)
            z = model.core_encoder(features)
        torch.manual_seed(77)
        noise = torch.randn(1, nRs, model.Nc, dtype=torch.complex64)
        sigma = 10 ** (-EbNodB / 20)
        nz = torch.view_as_real(noise).numpy().reshape(-1).astype(np.float32)     # (re,im) interleaved == z layout
        out.update({f"{tag}_H": H.numpy()[0].astype(np.float32), f"{tag}_noise": nz, f"{tag}_sigma": np.float64(sigma),
                    f"{tag}_z_hat": o["z_hat"].numpy()[0].astype(np.float32), f"{tag}_features_hat": o["features_hat"].numpy()[0].astype(np.float32)})
        out["z"] = z.numpy()[0].astype(np.float32)
        out[f"{tag}_loss"] = np.float64(distortion_loss(features, o["features_hat"]).item())
    np.savez_compressed(golden(dst, "model05.npz"), features=feat36[:, :20].astype(np.float32), **out)
    print("model05 ok", {k: float(v) for k, v in out.items() if k.endswith("loss")})


def gen_bbfm(src, dst):
    """Config 5: BBFM(20, 80, CNRdB) (bbfm.py:42-197).  No trained weights exist, so seeded random weights
    (torch default init + orthogonal weight_hh, radae_base.py:72-77,136-147) are exported to a DNNw blob with
    radae_amd.dnnw.write_blob, and the de-quantised blob is what both the reference modules and the engine load."""
    R.enter()
    import torch
    from radae import BBFM
    from radae_amd import dnnw
    from radae_amd.channel_tools import doppler_spread, synth_features
    torch.manual_seed(20240501)
    model = BBFM(20, 80, 20.0)
    enc, dec = model.core_encoder.module, model.core_decoder.module
    sd = lambda t: t.detach().numpy().astype(np.float32).copy()
    mk_gru = lambda g: dnnw.GRU(sd(g.weight_ih_l0), sd(g.weight_hh_l0), sd(g.bias_ih_l0), sd(g.bias_hh_l0))
    m = dnnw.Model(
        enc_dense1=dnnw.Dense(sd(enc.dense_1.weight), sd(enc.dense_1.bias)),
        enc_gru=[mk_gru(getattr(enc, f"gru{i}")) for i in range(1, 6)],
        enc_conv=[dnnw.Conv(sd(getattr(enc, f"conv{i}").conv.weight), sd(getattr(enc, f"conv{i}").conv.bias), dnnw.ENC_DILATION[i - 1]) for i in range(1, 6)],
        enc_zdense=dnnw.Dense(sd(enc.z_dense.weight), sd(enc.z_dense.bias)),
        dec_dense1=dnnw.Dense(sd(dec.dense_1.weight), sd(dec.dense_1.bias)),
        dec_gru=[mk_gru(getattr(dec, f"gru{i}")) for i in range(1, 6)],
        dec_glu=[dnnw.Dense(sd(getattr(dec, f"glu{i}").gate.weight), np.zeros(96, np.float32)) for i in range(1, 6)],
        dec_conv=[dnnw.Conv(sd(getattr(dec, f"conv{i}").conv.weight), sd(getattr(dec, f"conv{i}").conv.bias), 1) for i in range(1, 6)],
        dec_output=dnnw.Dense(sd(dec.output.weight), sd(dec.output.bias)))
    blob = os.path.join(dst, "weights", "bbfm_random_seed20240501.bin")
    dnnw.write_blob(m, blob)
    mq = dnnw.load_model(blob)
    T = 480
    feat36 = synth_features(2100, T)
    features = torch.tensor(feat36[None, :, :20])
    nsym = T * 20
    rng = np.random.default_rng(4)
    Hray = np.abs(doppler_spread(50.0, 2000, nsym, rng)); Hray = (Hray / np.sqrt(np.mean(Hray ** 2))).astype(np.float32)
    out = {}
    for tag, CNRdB, Hn in (("awgn", 20.0, np.ones(nsym, np.float32)), ("ray", 14.0, Hray)):
        model = BBFM(20, 80, CNRdB)
        load_into(model, mq)
        model.eval()
        torch.manual_seed(88)
        with torch.inference_mode():
            o = model(features, torch.tensor(Hn.reshape(1, nsym, 1)))
            z = model.core_encoder(features)
        torch.manual_seed(88)
        noise = torch.randn(1, nsym, 1).numpy().reshape(-1).astype(np.float32)
        out.update({f"{tag}_H": Hn, f"{tag}_noise": noise, f"{tag}_CNRdB": np.float64(CNRdB), f"{tag}_z_hat": o["z_hat"].numpy()[0].astype(np.float32),
                    f"{tag}_features_hat": o["features_hat"].numpy()[0].astype(np.float32), f"{tag}_sigma": o["sigma"].numpy().reshape(-1).astype(np.float32)})
        out["z"] = z.numpy()[0].astype(np.float32)
    np.savez_compressed(golden(dst, "bbfm.npz"), features=feat36[:, :20].astype(np.float32), Gfm=np.float64(model.Gfm), **out)
    print("bbfm ok Gfm", model.Gfm, "frac below FM threshold (ray):", float(np.mean(20 * np.log10(Hray) + 14.0 < 12)))


def gen_wire(src, dst):
    """int16 <-> f32 converters: the reference's own scripts (int16tof32.py, f32toint16.py) run as subprocesses on fixed bytes."""
    R.enter()
    import subprocess
    rng = np.random.default_rng(5)
    i16 = rng.integers(-32768, 32767, 2001, dtype=np.int16).tobytes()             # odd count: the trailing sample is dropped
    f32 = np.concatenate([rng.uniform(-1.2, 1.2, 600), [0.99999, -0.99999, 1.0, -1.0, 0.5 / 32767, -0.5 / 32767]]).astype(np.float32).tobytes()
    run = lambda script, args, data: subprocess.run([sys.executable, os.path.join(R.REF, script)] + args, input=data, stdout=subprocess.PIPE, check=True).stdout
    np.savez_compressed(golden(dst, "wire.npz"), i16=np.frombuffer(i16, np.uint8), f32=np.frombuffer(f32, np.uint8),
                        i2f=np.frombuffer(run("int16tof32.py", [], i16), np.uint8), i2f_zp=np.frombuffer(run("int16tof32.py", ["--zeropad"], i16), np.uint8),
                        f2i=np.frombuffer(run("f32toint16.py", [], f32), np.uint8), f2i_real=np.frombuffer(run("f32toint16.py", ["--real"], f32), np.uint8),
                        f2i_scale=np.frombuffer(run("f32toint16.py", ["--scale", "8192"], f32), np.uint8))
    print("wire ok")
