"""CPU half of the transmit / channel / row kernel unit tests (tests/test_tx_units_gpu.py is the device half).  Two jobs:

1. Pin the float64 references of tests/tx_ref.py to the reference project's recordings under tests/golden/ (modulator, end-of-over frame, channel) and to
   radae_amd.channel_tools (multipath generator).  The bars are the recordings' own float32 arithmetic: twice the largest residual found when the references
   were written (1.14e-6 on enc_tx, 2.5e-7 on the EOO frame, 1.04e-5 on chan_mpp's rx, where the recording adds float32 omegas in a float32 cumsum).
2. Prove that every checker the device tests call can fail: the float32 rounding of the reference passes, and each stand-in for a plausible kernel bug is
   rejected with a message that names the first wrong sample."""
import re

import numpy as np
import pytest

import kernel_ref as kr
import tx_ref as tx


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


@pytest.fixture(scope="module")
def tab(lib):
    return tx.Tab(lib)


def rejects(call, *needles):
    """the checker raises, and its message holds every needle"""
    with pytest.raises(AssertionError) as e:
        call()
    msg = str(e.value)
    for n in needles:
        assert n in msg, f"the message does not name {n!r}: {msg}"
    return msg


def f32(x):
    """the float32 (complex64) rounding of a reference"""
    return np.asarray(x).astype(np.complex64 if np.iscomplexobj(x) else np.float32)


# ================================================================================================================================================================
# 1. the references against the recordings
# ================================================================================================================================================================
def test_mod_ref_against_recordings(tab, golden):
    g = golden("enc_tx")
    want, _ = tx.mod_ref(tab, g["z"], linear=False)
    d = np.abs(want - g["tx"].reshape(2, -1)).max()
    print(f"enc_tx: largest |reference - recording| {d:.3g}")
    assert d < 2e-6
    g = golden("bypass")
    want, _ = tx.mod_ref(tab, g["z_in"].reshape(1, -1, 80), linear=False)
    d = np.abs(want[0] - g["tx"].ravel()).max()
    print(f"bypass: {d:.3g}")
    assert d < 2e-6


def test_eoo_ref_against_recording(tab, golden):
    c = golden("consts")
    want, bound = tx.eoo_ref(tab, c["eoo_bits_in"][None])
    d = np.abs(want[0] - c["eoo_with_bits"]).max()
    print(f"eoo_with_bits: {d:.3g}")
    assert d < 5e-7
    assert not bound[0, :2 * tx.SYM].any() and not bound[0, 5 * tx.SYM:].any() and bound[0, 2 * tx.SYM:5 * tx.SYM].all()


@pytest.mark.parametrize("name", ["mpp", "awgn"])
def test_chan_ref_against_recordings(tab, golden, name):
    g = golden("chan_" + name)
    sigma, f0 = float(g["sigma"]), float(g["freq_offset"])
    assert float(g["df_dt"]) == 0
    rx, _, fin = tx.chan_ref(g["tx"][None], g["noise"][None], G=g["G"][None], sigma=sigma, freq_offset=f0)
    d = np.abs(rx[0] - g["rx"]).max()
    noise = np.concatenate([g["noise_pre"].astype(np.complex64), g["noise"], g["noise_eoo"], g["noise_post"].astype(np.complex64)])
    full, _, _ = tx.chan_ref(g["tx"][None], noise[None], len(g["noise_pre"]), len(g["noise_post"]), eoo=tab.eoo32[None], G=g["G"][None], sigma=sigma, freq_offset=f0)
    d2 = np.abs(full[0] - g["rx_full"]).max()
    d3 = abs(fin[0] - g["final_phase"][0])
    print(f"chan_{name}: rx {d:.3g}, rx_full {d2:.3g}, final_phase {d3:.3g}")
    assert d < 2e-5 and d2 < 2e-5 and d3 < 2e-5


@pytest.mark.parametrize("name", ["dfdt_pos", "dfdt_neg"])
def test_chan_ref_against_drift_recordings(tab, golden, name):
    """the bars of test_hip_parity.py::test_channel_df_dt_golden, whose docstring derives them: the recording sums float32 omegas, the closed form differs from
    that by <= 2e-7 rad before both are rounded to float32, and at ~800 rad one float32 step is 6e-5 rad"""
    g = golden("chan_" + name)
    noise = np.concatenate([g["noise_pre"].astype(np.complex64), g["noise"], g["noise_eoo"], g["noise_post"].astype(np.complex64)])
    full, _, _ = tx.chan_ref(g["tx"][None], noise[None], len(g["noise_pre"]), len(g["noise_post"]), eoo=tab.eoo32[None], sigma=float(g["sigma"]),
                             freq_offset=float(g["freq_offset"]), df_dt=float(g["df_dt"]))
    d = full[0] - g["rx_full"]
    print(f"chan_{name}: rms {np.sqrt(np.mean(np.abs(d) ** 2)):.3g}, max {np.abs(d).max():.3g}, share above 1e-5 {np.mean(np.abs(d) > 1e-5):.3g}")
    assert np.sqrt(np.mean(np.abs(d) ** 2)) < 1e-5 and np.abs(d).max() < 2e-4
    assert np.mean(np.abs(d) > 1e-5) < 0.01


@pytest.mark.parametrize("channel,n_out", [("mpp", 8000), ("lmr60", 1501)])
def test_mpgen_ref_against_channel_tools(channel, n_out):
    """the generator reference on channel_tools' own noise draw: the float64 composition doppler_spread / np.var to 1e-12, and multipath_g / multipath_h (which
    round to float32) to that rounding"""
    from radae_amd import channel_tools as ct
    spread, delay = ct.PRESETS[channel]
    taps, ratio, n_low = ct.doppler_plan(spread, 8000, n_out)
    assert n_low == tx.n_low_of(ratio, n_out)
    rng = np.random.default_rng(5)
    x = np.empty((1, 2, n_low + len(taps)), np.complex128)
    for p in range(2):
        x[0, p] = rng.standard_normal(n_low + len(taps)) + 1j * rng.standard_normal(n_low + len(taps))
    G, _ = tx.mpgen_ref(x, taps, ratio, n_out)
    rng = np.random.default_rng(5)
    g1 = ct.doppler_spread(spread, 8000, n_out, rng); g2 = ct.doppler_spread(spread, 8000, n_out, rng)
    want = np.stack([g1, g2], axis=1) / np.sqrt(np.var(g1) + np.var(g2))
    assert np.abs(G[0] - want).max() < 1e-12 * np.abs(want).max()
    g32 = ct.multipath_g(channel, 8000, n_out, 5)
    assert np.abs(G[0] - g32).max() <= (2 * tx.U + 1e-12) * np.abs(want).max()
    m, nc = 4, 3
    n_sym = (n_out - 1) // m + 1
    for cplx in (False, True):
        H, _ = tx.mph_ref(G[:, :(n_sym - 1) * m + 1], m, n_sym, nc, delay * 2000.0, cplx, f32_phase=False)
        # multipath_h draws (n_sym - 1) m + 1 samples: the same process only when that is n_out
        if (n_sym - 1) * m + 1 == n_out:
            hw = ct.multipath_h(channel, 8000, 2000, nc, n_sym, 5, cplx)
            assert np.abs(H[0] - hw).max() <= 4 * tx.U * np.abs(H).max()
        g = G[0].astype(np.complex128)
        h64 = g[::m, 0][:n_sym, None] + g[::m, 1][:n_sym, None] * np.exp(-2j * np.pi * np.arange(nc)[None, :] * delay * 2000.0)
        assert np.abs(H[0] - (h64 if cplx else np.abs(h64))).max() < 1e-12 * np.abs(h64).max()


# ================================================================================================================================================================
# 2. the checkers can fail
# ================================================================================================================================================================
def mod_standin(tab, z, linear, pilot_gain_always=False, limit_always=False, prefix_from=128):
    """a modulator with a chosen bug"""
    z = np.asarray(z, np.float32); B = z.shape[0]; n_mf = z.shape[1] * z.shape[2] // tx.ZMF
    data = tx.c128(z.reshape(B, n_mf, 4, 30, 2)).reshape(B, n_mf, 4, 30)
    pg = tab.pilot_gain if (pilot_gain_always or not linear) else 1.0
    sym = np.concatenate([np.broadcast_to(tab.P * pg + 0j, (B, n_mf, 1, 30)), data], axis=2)
    x = sym @ tab.Winv
    if limit_always or not linear:
        x = tx.limiter(x)
    return np.concatenate([x[..., prefix_from:prefix_from + 32], x], axis=-1).reshape(B, n_mf * 960).astype(np.complex64)


@pytest.fixture(scope="module")
def mod_case(tab):
    rng = np.random.default_rng(11)
    z = rng.uniform(-1, 1, (2, 6, 80)).astype(np.float32)
    return z, {lin: tx.mod_ref(tab, z, lin) for lin in (0, 1)}


def test_check_mod_rejects_stand_ins(tab, mod_case):
    z, ref = mod_case
    for lin in (0, 1):
        r = tx.check_mod(f32(ref[lin][0]), ref[lin], f"mod linear={lin}")
        assert r < 0.5                                             # the rounding alone is u |x| / 2 against gamma_60 S
    rejects(lambda: tx.check_mod(mod_standin(tab, z, 0, prefix_from=127), ref[0], "prefix from 127"), "stream 0, frame 0, sample 0")
    rejects(lambda: tx.check_mod(mod_standin(tab, z, 1, pilot_gain_always=True), ref[1], "pilot gain when linear"), "stream 0, frame 0, sample 0")
    rejects(lambda: tx.check_mod(mod_standin(tab, z, 1, limit_always=True), ref[1], "limiter when linear"), "stream 0, frame 0, sample")
    got = f32(ref[0][0]); got[1, 960 + 2 * 192 + 5] = got[1, 960 + 2 * 192 + 4]                 # one prefix sample that is not its body's: inside the bound or not, never a bit copy
    rejects(lambda: tx.check_prefix(got, "one prefix sample"), "stream 1, frame 1, symbol 2, sample 5")
    got = f32(ref[0][0]); got[1, 1919] = np.nan
    rejects(lambda: tx.check_mod(got, ref[0], "a NaN"), "stream 1, frame 1, sample 959")


def test_check_eoo_rejects_stand_ins(tab):
    rng = np.random.default_rng(12)
    bits = np.sign(rng.standard_normal((3, 180))).astype(np.float32); bits[2] *= rng.uniform(0, 8, 180).astype(np.float32)
    ref = tx.eoo_ref(tab, bits)
    tx.check_eoo(f32(ref[0]), ref, "eoo")
    got = f32(ref[0]); got[1, 7] = np.nextafter(got[1, 7].real, np.float32(2)) + 1j * got[1, 7].imag          # the table's part is a bit copy: one ulp is too much
    rejects(lambda: tx.check_eoo(got, ref, "table sample off by an ulp"), "stream 1, symbol 0, sample 7")
    got = f32(ref[0]); got[:, 2 * 192:5 * 192] = f32(tx.limiter((tx.c128(bits.reshape(3, 3, 30, 2)).reshape(3, 3, 30) @ tab.Winv)))[..., list(range(128, 160)) + list(range(160))].reshape(3, -1)
    rejects(lambda: tx.check_eoo(got, ref, "no pilot gain on the data symbols"), "stream 0, symbol 2, sample 0")


def test_check_mp_rejects_stand_ins(tab, mod_case):
    rng = np.random.default_rng(13)
    z, ref = mod_case
    txs = f32(ref[0][0])                                           # "the kernel's own tx"
    G = ((rng.standard_normal((2, 1920, 2)) + 1j * rng.standard_normal((2, 1920, 2))) / np.sqrt(2)).astype(np.complex64)
    mp, _ = tx.mp_ref(txs, G)
    part = tx.part_ref(txs, f32(mp))
    r, r2 = tx.check_mp(f32(mp), part, txs, G, "mp")
    assert r < 1 and r2 == 0
    rejects(lambda: tx.check_mp(f32(tx.mp_ref(txs, G, 15)[0]), part, txs, G, "delay 15"), "mp:", "stream 0, frame 0, sample 15")
    rejects(lambda: tx.check_mp(f32(tx.mp_ref(txs, G, 17)[0]), part, txs, G, "delay 17"), "stream 0, frame 0, sample 16")
    got = f32(mp); got[:, :16] += (tx.c128(txs[:, 944:960]) * tx.c128(G[:, 944:960, 1])).astype(np.complex64)
    rejects(lambda: tx.check_mp(got, part, txs, G, "a second path in the first 16 samples"), "stream 0, frame 0, sample 0")
    got = f32(mp); got[:, 960:976] = (tx.c128(txs[:, 960:976]) * tx.c128(G[:, 960:976, 0]) + tx.c128(txs[:, 1904:1920]) * tx.c128(G[:, 1904:1920, 1])).astype(np.complex64)
    rejects(lambda: tx.check_mp(got, part, txs, G, "the frame's own tail as second path"), "stream 0, frame 1, sample 0")
    bad = part.copy(); bad[1, 1, 1] *= 1 + 6 * tx.U
    rejects(lambda: tx.check_mp(f32(mp), bad, txs, G, "a part sum 6 u off"), "part", "stream 1, frame 1, sum 1")


CH = dict(n_pre=3, n_post=2, n_sig=1920)


@pytest.fixture(scope="module")
def chan_case(tab, mod_case):
    rng = np.random.default_rng(14)
    txs = np.concatenate([f32(mod_case[1][0][0]), f32(mod_case[1][0][0][:1, ::-1])])                       # B = 3
    B, n_sig, n_pre, n_post = 3, CH["n_sig"], CH["n_pre"], CH["n_post"]
    n_total = n_pre + n_sig + 1152 + n_post                        # 3077: odd
    G = ((rng.standard_normal((B, n_sig, 2)) + 1j * rng.standard_normal((B, n_sig, 2))) / np.sqrt(2)).astype(np.complex64)
    noise = ((rng.standard_normal((B, n_total)) + 1j * rng.standard_normal((B, n_total))) / np.sqrt(2)).astype(np.complex64)
    noise[:, :n_pre] = noise[:, :n_pre].real; noise[:, n_total - n_post:] = noise[:, n_total - n_post:].real     # real-valued, as inference.py:277-284 has them
    ps = np.array([[0.5, 0.3, 0.7], [-7, 20, 0], [0, 0.5, 0.5]], np.float32)                                # stream 2: the case the reference leaves unrotated
    eoo = np.broadcast_to(tab.eoo32, (B, 1152)).copy()
    kw = dict(n_pre=n_pre, n_post=n_post, eoo=eoo, G=G, ps=ps)
    return txs, noise, kw, tx.chan_ref(txs, noise, **kw), tx.chan_ref(txs, 0 * noise, **kw)


def test_check_chan_rejects_stand_ins(tab, chan_case):
    txs, noise, kw, ref, ref0 = chan_case
    n_pre, n_sig = CH["n_pre"], CH["n_sig"]; e0 = n_pre + n_sig; n_total = ref[0].shape[1]
    assert n_total % 2 == 1
    assert tx.check_chan(f32(ref[0]), ref, "channel") < 1
    got = f32(ref[0]); got[:, -1] = np.nan
    rejects(lambda: tx.check_chan(got, ref, "odd n_total: last sample dropped"), f"stream 0, sample {n_total - 1}")
    fin = ref[2]; assert abs(fin[0] - 1) > 0.1 and fin[2] == 1
    got = ref[0].copy(); got[:, e0:e0 + 1152] += ref0[0][:, e0:e0 + 1152] * (1 / fin[:, None] - 1)
    rejects(lambda: tx.check_chan(f32(got), ref, "EOO phase restarts at 1"), f"stream 0, sample {e0}")
    mp, _ = tx.mp_ref(txs, kw["G"]); gain = np.sqrt((np.abs(tx.c128(txs)) ** 2).sum(1) / (np.abs(mp) ** 2).sum(1))
    got = ref[0].copy(); got[:, e0:e0 + 1152] += ref0[0][:, e0:e0 + 1152] * (gain[:, None] - 1)
    rejects(lambda: tx.check_chan(f32(got), ref, "EOO times the multipath gain"), f"stream 0, sample {e0}")
    ph = tx.chan_phase(np.arange(n_sig), 0.0, 0.5)
    got = ref[0].copy(); got[2, n_pre:e0] += ref0[0][2, n_pre:e0] * (np.exp(1j * ph) - 1)
    first = n_pre + int(np.argmax(np.abs(ref0[0][2, n_pre:e0] * (np.exp(1j * ph) - 1)) > 2 * ref[1][2, n_pre:e0]))
    assert n_pre < first < n_pre + 200                             # the drift's phase is 2.5e-8 i (i + 1) rad: beyond a few u within the first frame's pilot
    msg = rejects(lambda: tx.check_chan(f32(got), ref, "drift applied at freq_offset 0"), "stream 2, sample ")
    assert n_pre < int(re.search(r"stream 2, sample (\d+)", msg).group(1)) <= first
    ps0 = kw["ps"].copy(); ps0[0] = ps0[0, 0]
    rejects(lambda: tx.check_chan(f32(tx.chan_ref(txs, noise, **dict(kw, ps=ps0))[0]), ref, "sigma of stream 0 everywhere"), "stream 1, sample 0")
    got = ref[0].copy(); got[:, :n_pre] = kw["ps"][0][:, None].astype(np.float64) * tx.c128(noise[:, :n_pre]).real * (1 + 1j) / np.sqrt(2)
    rejects(lambda: tx.check_chan(f32(got), ref, "real n_pre noise made complex"), "stream 0, sample 0")


def mpgen_standin(x, taps, ratio, n_out, clamp=False, n_low_delta=0, per_path_ddof1=False):
    """a generator with a chosen bug; the interpolation bugs keep the reference's gain, so that the first wrong sample is the first one they touch"""
    x = np.asarray(x, np.complex128); n_taps = len(taps); n_low = tx.n_low_of(ratio, n_out)
    pos = np.arange(n_out) / ratio
    i0 = np.minimum(pos.astype(np.int64), n_low + n_low_delta - 2); fr = pos - i0
    if clamp:
        fr = np.minimum(fr, 1.0)
    out = np.empty((x.shape[0], n_out, 2), np.complex128)
    for b in range(x.shape[0]):
        good = [np.convolve(x[b, p], taps)[n_taps:][:n_low] for p in range(2)]
        g = [y[i0] + (y[i0 + 1] - y[i0]) * fr for y in good]
        pos0 = np.minimum(pos.astype(np.int64), n_low - 2)
        ref = [y[pos0] + (y[pos0 + 1] - y[pos0]) * (pos - pos0) for y in good]
        var = np.var(ref[0], ddof=1) + np.var(ref[1], ddof=1) if per_path_ddof1 else np.var(ref[0]) + np.var(ref[1])
        out[b] = np.stack(g, axis=1) / np.sqrt(var)
    return out.astype(np.complex64)


def test_check_mpgen_and_mph_reject_stand_ins():
    rng = np.random.default_rng(15)
    ratio, n_out, n_taps = 7, 100, 5                               # n_low = 15: samples 99 (pos 14.14) extrapolates past the last low-rate point
    n_low = tx.n_low_of(ratio, n_out); assert ratio * (n_low - 1) < n_out - 1
    taps = rng.standard_normal(n_taps).astype(np.float32)
    x = (rng.standard_normal((2, 2, n_low + n_taps)) + 1j * rng.standard_normal((2, 2, n_low + n_taps))).astype(np.complex64)
    ref = tx.mpgen_ref(x, taps, ratio, n_out)
    assert tx.check_mpgen(f32(ref[0]), ref, "generator") <= 1
    assert np.array_equal(mpgen_standin(x, taps, ratio, n_out), f32(ref[0]))
    rejects(lambda: tx.check_mpgen(mpgen_standin(x, taps, ratio, n_out, clamp=True), ref, "clamped"), f"stream 0, sample {ratio * (n_low - 1) + 1}, path 0")
    rejects(lambda: tx.check_mpgen(mpgen_standin(x, taps, ratio, n_out, n_low_delta=-1), ref, "n_low one short"), f"stream 0, sample {ratio * (n_low - 2) + 1}, path 0")
    rejects(lambda: tx.check_mpgen(mpgen_standin(x, taps, ratio, n_out, per_path_ddof1=True), ref, "variance with n - 1"), "stream 0, sample 0, path 0")
    G = f32(ref[0])
    for cplx in (0, 1):
        m, nc = 4, 3; n_sym = (n_out - 1) // m + 1
        h = tx.mph_ref(G, m, n_sym, nc, 0.004 * 2000, cplx)
        assert tx.check_mph(f32(h[0]), h, "H") < 1
        got = f32(tx.mph_ref(np.roll(G, -1, axis=1), m, n_sym, nc, 0.004 * 2000, cplx)[0])                  # G[t M + 1]
        rejects(lambda: tx.check_mph(got, h, "H from the next sample"), "stream 0, symbol 0, carrier 0")
        got = f32(tx.mph_ref(G, m, n_sym, nc, -0.004 * 2000, cplx)[0])                                       # the delay's sign: carrier 0 is unaffected
        rejects(lambda: tx.check_mph(got, h, "H with the conjugate phasor"), "stream 0, symbol 0, carrier 1")


def test_check_rows_rejects_stand_ins():
    rng = np.random.default_rng(16)
    B, T = 2, 3
    feats = rng.standard_normal((B, 4 * T, 36)).astype(np.float32)
    want = tx.pack_ref(feats)
    assert np.array_equal(want[1, 2, 21:42], np.append(feats[1, 9, :20], np.float32(-1))) and not want[:, :, 84:].any()
    rows = kr.Rows(B, T, 96, 96, T * 96 + 192)
    tx.check_rows(rows, rows.fill(want).words, want, "pack")
    bad = np.zeros_like(want)
    for fr in range(4):
        bad[:, :, 22 * fr:22 * fr + 21] = feats[:, fr::4, :21]; bad[:, :, 22 * fr + 21] = -1
    bad[:, :, 88:] = 0
    rejects(lambda: tx.check_rows(rows, kr.Rows(B, T, 96, 96, T * 96 + 192).fill(bad).words, want, "aux at 21"), "stream 0, row 0, column 20")
    over = rows.fill(want).words.copy(); over[rows.base + T * 96:rows.base + T * 96 + 96] = want[0, 0].view(np.uint32)
    rejects(lambda: tx.check_rows(rows, over, want, "a row past T"), "written outside the documented rows", "stream 0, step 3")
    # padding
    src = rng.standard_normal((5, 84)).astype(np.float32)
    pw = tx.pad_ref(src, 88)
    assert np.array_equal(pw[:, :84], src) and not pw[:, 84:].any()
    # carrying: T = 1 < nhist = 2, source rows 1, 2 and destination rows 0, 1 overlap
    W, nhist, Tcap = 8, 2, 4
    x = rng.standard_normal((B, nhist + Tcap, W)).astype(np.float32)
    want = tx.carry_ref(x, nhist, 1)
    assert np.array_equal(want[:, 0], x[:, 1]) and np.array_equal(want[:, 1], x[:, 2]) and np.array_equal(want[:, 2:], x[:, 2:])
    crow = kr.Rows(B, nhist + Tcap, W, W, (nhist + Tcap) * W)
    tx.check_rows(crow, crow.fill(want).words, want, "carry")
    bad = x.copy()
    for k in (1, 0):                                               # row 1 written before row 0 has read it
        bad[:, k] = bad[:, 1 + k]
    rejects(lambda: tx.check_rows(crow, kr.Rows(B, nhist + Tcap, W, W, (nhist + Tcap) * W).fill(bad).words, want, "written before read"), "stream 0, row 0, column 0")
    left = tx.carry_ref(x, nhist, 3, n_rows=[0, -1])
    assert np.array_equal(left, x)
