"""The reference's remaining streaming edge cases, made by IMPORTING the reference through the drivers of oracle/golden/reference.py
(`channel_case` = RADAE.forward + inference.py's write_rx tail, `run_rx` = radae_rxe.py:349-356 with a per-call trace).

  rxtrace_slipdrops.npz  ctest radae_rx_slip_plus_drops (CMakeLists.txt:397-407; the reference's regression for "timing slips + dropped frames over a long
                         enough period -> unable to regain sync"): 62 s of a REAL-valued int16 signal (the ctest feeds a mono wav through
                         `int16tof32.py --zeropad`) at 8020 Hz (sox is absent: scipy polyphase resampler, 401/400), with three drop-outs of 0.5 / 1.2 / 2.0 s
                         (noise only); the stream ends inside the signal, and the trace's last state must be `sync` (the ctest's `grep 'state: sync'`).
                         The fixture carries the int16 samples; the tests convert them with radae_amd.wire.int16_to_f32(zeropad=True) like the ctest does.
  rxtrace_dfs8001.npz    ctest radae_rx_dfs (:374-382): 8001 Hz receive clock (f32toint16 --scale 8192 | sox 8000 -> 8001 | int16tof32, both channels), 10 dB AWGN,
                         +11 Hz; the start is placed so that the one-sample-per-second drift crosses the tmax >= Nmf - M limit (radae_rxe.py:211-214) inside the run.
  rxtrace_eoo_mpp.npz    ctest radae_eoo_data_mpp (:595-607): five overs, each ending in an EOO frame that carries the seeded data bits of
                         `radae_txe.py --eoo_data_test` (:157-163), through the MPP two-path channel + AWGN at 6 dB SNR (Eb/No 7.76 dB, the ctest's level); per detected EOO the soft bits.
  bypass.npz             `radae_rxe.py --bypass_dec` (:300-302, :315: z_hat out, no UW accounting) and `radae_txe.py --bypass_enc` (:124-126: latents in):
                         the receiver trace of the awgn fixture's samples with bypass_dec, and transmit frames from supplied latents.
Long traces keep every call's discrete outputs, thresholds and fmax, and `features_out` / `z_hat` of every 4th valid call (`rows_kept`).
"""
import numpy as np

from . import reference as R
from .reference import c64, channel_case, golden, new_tx, run_rx, thin


def gen_slipdrops(src, dst):
    R.enter()
    from scipy.signal import resample_poly
    from radae_amd import wire
    T = 6000                                                               # 60 s of feature frames
    d = channel_case("slipdrops", T, 10.0, 11.0, "awgn", 1020, prepend_s=1.0, append_s=0.0)
    n_pre = 8000
    x = np.concatenate([d["sigma"] * d["noise_pre"].astype(np.complex64), d["rx"]])            # no EOO: the over is still running when the file ends
    rng = np.random.default_rng(1021)
    for t0, dur in ((12.0, 0.5), (30.0, 1.2), (47.0, 2.0)):                # drop-outs: the signal gone, the channel noise stays
        a, n = n_pre + int(t0 * 8000), int(dur * 8000)
        x[a:a + n] = d["sigma"] * ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)
    i16_8000 = np.frombuffer(wire.f32_to_int16(c64(x).tobytes(), scale=8192.0, real=True), np.int16)    # f32toint16.py --real --scale 8192
    y = resample_poly(i16_8000.astype(np.float64), 401, 400)                                   # 8000 -> 8020 Hz
    i16 = np.clip(np.round(y), -32768, 32767).astype(np.int16)
    i16 = i16[:(len(i16) // 2) * 2]
    rx_in = np.frombuffer(wire.int16_to_f32(i16.tobytes(), zeropad=True), np.complex64)        # int16tof32.py --zeropad
    tr = run_rx(rx_in)
    st = tr["state_after"]
    resyncs = int(np.sum((st[1:] == 2) & (st[:-1] != 2)))
    print(f"slipdrops: {len(rx_in)} samples, calls {len(tr['ret'])} valid {int((tr['ret'] & 1).sum())} nin set {sorted(set(tr['nin_after'].tolist()))} "
          f"entries into sync {resyncs} final state {st[-1]} uw max {tr['uw_errors'].max()}")
    assert st[-1] == 2 and resyncs >= 2 and 1120 in tr["nin_after"]
    np.savez_compressed(golden(dst, "rxtrace_slipdrops.npz"), rx_i16=i16, features_in=d["features"][:, :20].astype(np.float16), **thin(tr))


def gen_dfs(src, dst):
    R.enter()
    from scipy.signal import resample_poly
    from radae_amd import wire
    for pre in (0.064,):
        d = channel_case("dfs", 1440, 10.0, 11.0, "awgn", 1022, prepend_s=pre, append_s=0.3)
        raw = np.frombuffer(wire.f32_to_int16(c64(d["rx_full"]).tobytes(), scale=8192.0), np.int16).reshape(-1, 2)      # f32toint16.py --scale 8192
        y = np.stack([resample_poly(raw[:, k].astype(np.float64), 8001, 8000) for k in range(2)], axis=1)              # sox -r 8000 -> -r 8001, two channels
        i16 = np.clip(np.round(y), -32768, 32767).astype(np.int16)
        rx_in = np.frombuffer(wire.int16_to_f32(np.ascontiguousarray(i16).tobytes()), np.complex64)                    # int16tof32.py
        tr = run_rx(rx_in)
        print(f"dfs8001 prepend {pre}: calls {len(tr['ret'])} valid {int((tr['ret'] & 1).sum())} nin set {sorted(set(tr['nin_after'].tolist()))} "
              f"tmax {tr['tmax'][tr['state_after'] == 2][:3]} .. {tr['tmax'].max()} final state {tr['state_after'][-1]}")
    assert 1120 in tr["nin_after"]
    np.savez_compressed(golden(dst, "rxtrace_dfs8001.npz"), rx_i16=i16, features_in=d["features"][:, :20].astype(np.float16), **thin(tr))


def gen_eoo_mpp(src, dst):
    R.enter()
    from radae_amd.channel_tools import multipath_g, synth_features
    seed = 65647; rng = np.random.default_rng(seed)                        # radae_txe.py:158-160
    tx = new_tx()
    bits = np.sign(rng.random(tx.get_Neoo_bits()) - 0.5).astype(np.float32)
    tx.set_eoo_bits(bits)
    feats = synth_features(1030, 96)
    frames = []
    out = np.zeros(tx.Nmf, np.csingle); eoo = np.zeros(tx.Neoo, np.csingle)
    for k in range(8):
        tx.do_radae_tx(feats[12 * k:12 * k + 12].ravel(), out); frames.append(out.copy())
    tx.do_eoo(eoo)
    over = np.concatenate(frames + [eoo])                                  # what radae_tx writes for one over
    txs = np.concatenate([over] * 5)                                       # `cat tx.f32 tx.f32 tx.f32 tx.f32 tx.f32`
    n = len(txs)
    Gm = multipath_g("mpp", 8000, n, 1031)
    dly = 16                                                               # 2 ms (multipath_samples.m:13-14)
    x2 = np.concatenate([np.zeros(dly, np.complex64), txs[:-dly]])
    sig = Gm[:, 0] * txs + Gm[:, 1] * x2
    EbNodB = 7.76                                                          # 6 dB SNR in 3 kHz, the ctest's "about 6 dB SNR" (`ch --No -24`): SNR = Eb/No + 10 log10(2000 / 3000)
    sigma = np.sqrt(8000.0 / (10 ** (EbNodB / 10) * 2000.0)) * np.sqrt(np.mean(np.abs(txs) ** 2))      # at the transmit power (radae.py:570-573)
    nr = np.random.default_rng(1032)
    npre, npost = 8000, 2400
    noise = ((nr.standard_normal(npre + n + npost) + 1j * nr.standard_normal(npre + n + npost)) / np.sqrt(2)).astype(np.complex64)
    y = np.concatenate([np.zeros(npre, np.complex64), sig, np.zeros(npost, np.complex64)])
    y = y * np.exp(2j * np.pi * (-11.0) * np.arange(len(y)) / 8000.0)
    rx_in = c64(y + sigma * noise)
    tr = run_rx(rx_in)
    bers = [float(np.mean(e * bits < 0)) for e in tr["eoo_out"]]
    print(f"eoo_mpp: calls {len(tr['ret'])} valid {int((tr['ret'] & 1).sum())} EOO frames {len(tr['eoo_out'])} BER {bers}")
    assert len(bers) >= 2 and min(bers) < 0.05
    np.savez_compressed(golden(dst, "rxtrace_eoo_mpp.npz"), rx_in=rx_in, tx_bits=bits, eoo_ber=np.array(bers), **tr)


def gen_bypass(src, dst):
    R.enter()
    g = np.load(golden(src, "rxtrace_awgn.npz"))
    # --bypass_dec: the constructor path radae_rxe.py:113-123 (no decoder state dict), floats_out = 240 latents per valid call (:315), UW errors never summed
    import radae_rxe
    rx = radae_rxe.radae_rx("unused", bypass_dec=True, v=0)
    R.load_into(rx.model, R.m19())
    R.lcg.x = 1
    floats_out = np.zeros(rx.get_n_floats_out(), np.float32)
    assert rx.get_n_floats_out() == 240
    x = g["rx_in"]; pos = 0
    ret_l, z_l, uw_l, st_l, eoo_l = [], [], [], [], []
    stn = {"search": 0, "candidate": 1, "sync": 2}
    while pos + rx.get_nin() <= len(x):
        nin = rx.get_nin()
        buf = np.zeros(rx.get_nin_max(), np.csingle); buf[:nin] = x[pos:pos + nin]; pos += nin
        ret = rx.do_radae_rx(buf, floats_out)
        ret_l.append(int(ret)); uw_l.append(int(rx.uw_errors)); st_l.append(stn[rx.state])
        if ret & 1: z_l.append(floats_out.copy())
        if ret & 2: eoo_l.append(floats_out[:180].copy())
    assert np.array_equal(np.array(ret_l), g["ret"]) and max(uw_l) == 0
    # --bypass_enc: latents in, transmit frames out (radae_txe.py:124-126)
    import radae_txe
    tx = radae_txe.radae_tx("unused", bypass_enc=True)
    assert tx.n_floats_in == 240
    rng = np.random.default_rng(1040)
    zin = np.clip(0.5 * rng.standard_normal((6, 240)), -1.5, 1.5).astype(np.float32)
    out = np.zeros(tx.Nmf, np.csingle); txo = []
    for k in range(6):
        tx.do_radae_tx(zin[k], out); txo.append(out.copy())
    np.savez_compressed(golden(dst, "bypass.npz"), rx_in=x, ret=np.array(ret_l, np.int32), state_after=np.array(st_l, np.int32), uw_errors=np.array(uw_l, np.int32),
                        z_hat_out=np.array(z_l, np.float32), eoo_out=np.array(eoo_l, np.float32).reshape(-1, 180), z_in=zin, tx=c64(np.array(txo)))
    print(f"bypass: rx calls {len(ret_l)} valid {len(z_l)} eoo {len(eoo_l)}; tx frames {len(txo)} peak {np.abs(np.array(txo)).max():.3f}")
