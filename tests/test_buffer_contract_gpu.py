"""GPU tests (-m gpu) of the buffer contract of include/rade_batch.h ("Buffers, strides and alignment"): strides, alignment and "nothing outside the rows is
written, no input is written".

Every case calls the C entry points directly (eng.lib / eng.h over ctypes) on buffers laid out by tests/bands.py -- rows at a stride larger than the row, a
base pointer at the smallest offset the contract allows (an odd element offset and an odd stride for complex64 buffers that need natural alignment only), NaN
sentinels in the guards, the gaps and the rows -- and compares with the same call on dense buffers (through the wrapper, or stride = row length): the rows are
bit-equal, the band checks pass (tests/test_host_cpu.py shows the checker reports every kind of fault), the inputs are bit-equal to a snapshot.
Pointers the contract forbids are only ever passed to show that the HOST refuses them (return < 0, nothing launched, outputs still all sentinel)."""
import ctypes as C

import numpy as np
import pytest

from bands import Band
from gpu_kit import INT_KEYS, bits, crandn, engine, stream, sync, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu

TX_BPF, BYPASS_DEC = 0x400, 0x800


def odd(n):
    return n | 1


class Inputs:
    """input buffers in bands of their own; unchanged() compares every word (rows, gaps, guards) with the snapshot taken when they were filled"""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def put(self, values, elem_bytes, stride=None, off=None):
        """values [B, row]; stride None: ONE dense row of everything (a buffer without a stride argument).  off: bytes past a 16-byte boundary (default: one element)"""
        v = np.ascontiguousarray(values)
        v = v.reshape(v.shape[0], -1) if stride is not None else v.reshape(1, -1)
        row = v.shape[1] * v.dtype.itemsize // elem_bytes
        bd = Band(v.shape[0], row, stride if stride is not None else row, elem_bytes, self.dev, base_offset_bytes=elem_bytes % 16 if off is None else off).fill(v)
        self.items.append((bd, bd.host().copy()))
        return bd

    def unchanged(self):
        for i, (bd, snap) in enumerate(self.items):
            assert np.array_equal(bd.host(), snap), f"input buffer {i} was written"


def feats(B, n_mf, seed=3):
    from radae_amd.channel_tools import synth_features
    return np.stack([synth_features(seed + b, 12 * n_mf) for b in range(B)]).astype(np.float32)


# ---- transmit side ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, TX_BPF])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_tx_family(torch_dev, B, flags):
    """rade_batch_tx, rade_batch_tx_eoo, rade_batch_tx_latents with n_mf = 3 of max_tx_mf = 4 (rows of the engine's capacity stay unused), with and without
    RADE_BATCH_TX_BPF: iq_out at an odd stride and an odd sample offset, z_out 16-byte aligned behind its guard, features and latents at a 4-byte offset."""
    import torch
    from radae_amd.engine import BatchEngine
    n_mf, cap = 3, 4
    f = feats(B, n_mf)
    eng = BatchEngine(B, max_tx_mf=cap, flags=flags)
    iq_d, z_d = eng.tx(torch.tensor(f, device=torch_dev), want_z=True)
    eoo_d = eng.tx_eoo()
    eng.tx_reset()
    lat_d = eng.tx_latents(z_d)
    eng.close()

    eng = BatchEngine(B, max_tx_mf=cap, flags=flags)
    L, h = eng.lib, eng.h
    ins = Inputs(torch_dev)
    fb = ins.put(f, 4)
    iq = Band(B, 960 * n_mf, odd(960 * n_mf + 6), 8, torch_dev, base_offset_bytes=8)
    z = Band(1, B * 3 * n_mf * 80, B * 3 * n_mf * 80, 4, torch_dev, base_offset_bytes=0)
    # refused: z_out_dev 4 bytes off a 16-byte boundary -- rade_enc.hip encf_emit: `*(f32x4 *)(a.y + (size_t)b * a.y_sb + (size_t)t * a.y_st + ch0) = v;`
    assert L.rade_batch_tx(h, fb.ptr, n_mf, iq.ptr, iq.stride, z.ptr + 4, stream()) < 0
    sync(); iq.untouched("iq_out of a refused call"); z.untouched("z_out of a refused call")
    assert L.rade_batch_tx(h, fb.ptr, n_mf, iq.ptr, iq.stride, z.ptr, stream()) == 960 * n_mf
    sync()
    iq.check(what="iq_out"); z.check(what="z_out"); ins.unchanged()
    assert np.array_equal(iq.rows(), bits(iq_d)) and np.array_equal(z.rows().reshape(B, -1), bits(z_d))
    eoo = Band(B, 1152, odd(1152 + 4), 8, torch_dev, base_offset_bytes=8)
    assert L.rade_batch_tx_eoo(h, eoo.ptr, eoo.stride, stream()) == 1152
    sync()
    eoo.check(what="eoo iq_out"); assert np.array_equal(eoo.rows(), bits(eoo_d))
    eng.tx_reset()
    zin = ins.put(z_d.cpu().numpy(), 4)                               # latents in: natural alignment (k_ofdm_mod reads them one float at a time)
    iq2 = Band(B, 960 * n_mf, odd(960 * n_mf + 10), 8, torch_dev, base_offset_bytes=8)
    assert L.rade_batch_tx_latents(h, zin.ptr, n_mf, iq2.ptr, iq2.stride, stream()) == 960 * n_mf
    sync()
    iq2.check(what="iq_out of tx_latents"); ins.unchanged()
    assert np.array_equal(iq2.rows(), bits(lat_d))
    eng.close()


def test_encode_decode(torch_dev):
    """rade_batch_encode / rade_batch_decode with n_steps = 5 of 3 * max_tx_mf = 12: dense buffers behind guards, the 16-byte rules refused on the host"""
    import torch
    from radae_amd.engine import BatchEngine
    B, n = 3, 5
    rng = np.random.default_rng(2)
    f = (0.5 * rng.standard_normal((B, n, 84))).astype(np.float32)
    eng = BatchEngine(B, max_tx_mf=4)
    z_d = eng.encode(torch.tensor(f, device=torch_dev))
    fo_d = eng.decode(z_d, 84)
    eng.close()
    eng = BatchEngine(B, max_tx_mf=4)
    L, h = eng.lib, eng.h
    ins = Inputs(torch_dev)
    fb = ins.put(f, 4)
    z = Band(1, B * n * 80, B * n * 80, 4, torch_dev)
    # refused: z_out_dev off a 16-byte boundary -- rade_enc.hip encf_emit: `*(f32x4 *)(a.y + (size_t)b * a.y_sb + (size_t)t * a.y_st + ch0) = v;`
    assert L.rade_batch_encode(h, fb.ptr, n, z.ptr + 8, stream()) < 0
    sync(); z.untouched("z_out of a refused call")
    assert L.rade_batch_encode(h, fb.ptr, n, z.ptr, stream()) == n
    sync()
    z.check(what="z_out"); ins.unchanged(); assert np.array_equal(z.rows().reshape(B, -1), bits(z_d))
    zin = ins.put(z_d.cpu().numpy(), 4, off=0)
    fo = Band(1, B * n * 84, B * n * 84, 4, torch_dev, base_offset_bytes=4)
    # refused: z_dev off a 16-byte boundary -- rade_kernels.hip k_gemm_splitk: `const f32x4 av = *(const f32x4 *)p;` with p in the caller's z rows (decoder dense1)
    assert L.rade_batch_decode(h, zin.ptr + 4, n, fo.ptr, 1, stream()) < 0
    sync(); fo.untouched("features_out of a refused call")
    assert L.rade_batch_decode(h, zin.ptr, n, fo.ptr, 1, stream()) == n
    sync()
    fo.check(what="features_out"); ins.unchanged(); assert np.array_equal(fo.rows().reshape(B, -1), bits(fo_d))
    eng.close()


def test_encoder_large_and_small_calls(engine, torch_dev):
    """B = 72 x n_mf = 84 = 18144 rows reaches rade_enc.hip's 16-byte stores into z_out_dev (max_tx_mf = 90: capacity unused); one modem frame on the same engine
    takes the float32-row kernels.  Both: guards around z_out and iq_out intact, bit-equal to the dense call after the matching reset."""
    import torch
    B, cap = 72, 90
    eng = engine(B, max_tx_mf=cap)
    L, h = eng.lib, eng.h
    for n_mf in (84, 1):
        f = feats(B, n_mf, seed=40)
        assert (B * 3 * n_mf > 16384) == (n_mf == 84)
        eng.tx_reset()
        iq_d, z_d = eng.tx(torch.tensor(f, device=torch_dev), want_z=True)
        eng.tx_reset()
        ins = Inputs(torch_dev)
        fb = ins.put(f, 4)
        iq = Band(B, 960 * n_mf, odd(960 * n_mf + 2), 8, torch_dev, base_offset_bytes=8)
        z = Band(1, B * 3 * n_mf * 80, B * 3 * n_mf * 80, 4, torch_dev)
        # refused at every size: rade_enc.hip encf_emit: `*(f32x4 *)(a.y + (size_t)b * a.y_sb + (size_t)t * a.y_st + ch0) = v;`
        assert L.rade_batch_tx(h, fb.ptr, n_mf, iq.ptr, iq.stride, z.ptr + 4, stream()) < 0
        sync(); z.untouched("z_out of a refused call"); iq.untouched("iq_out of a refused call")
        assert L.rade_batch_tx(h, fb.ptr, n_mf, iq.ptr, iq.stride, z.ptr, stream()) == 960 * n_mf
        sync()
        z.check(what=f"z_out, n_mf {n_mf}"); iq.check(what=f"iq_out, n_mf {n_mf}"); ins.unchanged()
        assert np.array_equal(z.rows().reshape(B, -1), bits(z_d)) and np.array_equal(iq.rows(), bits(iq_d))


# ---- channel -------------------------------------------------------------------------------------------------------------------------------------------
def chan_params(n_sig, n_pre, n_post, with_eoo, sigma=0.0, fo=0.0, dfdt=0.0, G=None, noise=None, seed=0):
    from radae_amd.engine import ChannelParams
    return ChannelParams(n_sig, n_pre, n_post, int(with_eoo), sigma, fo, dfdt, G, noise, seed, 0.0, 0.0, 1.0)


def chan_streams(per):
    from radae_amd.engine import ChannelStreams
    return ChannelStreams(*(per[k].ctypes.data for k in ("sigma", "freq_offset", "df_dt")))


# (n_pre, n_post, with_eoo, G, explicit noise): n_total even and odd; with the odd stride and the odd sample offset below the rows of even and odd streams sit
# on different sides of a 16-byte boundary, so every call takes both stores of k_chan_apply, and the tail store when n_total is odd
CHAN_CASES = [(0, 0, False, False, True), (1, 0, True, True, False), (801, 1152, True, True, True), (1, 1152, False, False, False), (0, 1152, True, False, True)]


@pytest.mark.parametrize("flags", [0, TX_BPF])
@pytest.mark.parametrize("B", [3, 5])
def test_channel_calls(engine, torch_dev, B, flags):
    """rade_batch_channel and rade_batch_channel_streams: banded rx_out and tx_dev, G and noise at an 8-byte offset, n_total even and odd, with and without
    G_dev, with_eoo, explicit noise and Philox"""
    import torch
    n_mf = 2; n_sig = 960 * n_mf
    rng = np.random.default_rng(7)
    eng = engine(B, max_tx_mf=n_mf, flags=flags)
    L, h = eng.lib, eng.h
    tx_d = eng.tx(torch.tensor(feats(B, n_mf), device=torch_dev))
    tx_np = tx_d.cpu().numpy()
    per = {"sigma": np.linspace(0.1, 0.9, B).astype(np.float32), "freq_offset": np.linspace(-20, 30, B).astype(np.float32), "df_dt": np.linspace(-1, 1, B).astype(np.float32)}
    took = set()
    for n_pre, n_post, with_eoo, with_G, with_noise in CHAN_CASES:
        n_total = n_pre + n_sig + (1152 if with_eoo else 0) + n_post
        G_np = crandn(rng, B, n_sig, 2) if with_G else None
        nz_np = crandn(rng, B, n_total) if with_noise else None
        seed = 0 if with_noise else 11
        kw = dict(n_pre=n_pre, n_post=n_post, with_eoo=with_eoo, G=torch.tensor(G_np, device=torch_dev) if with_G else None,
                  noise=torch.tensor(nz_np, device=torch_dev) if with_noise else None, seed=seed)
        ins = Inputs(torch_dev)
        txb = ins.put(tx_np, 8, stride=odd(n_sig + 4))
        Gb = ins.put(G_np, 8) if with_G else None                     # rade_batch_channel reads G by element: 8 bytes are enough
        nzb = ins.put(nz_np, 8) if with_noise else None
        for streams in (False, True):
            rx_d = eng.channel(tx_d, per["sigma"] if streams else 0.4, per["freq_offset"] if streams else 12.5, df_dt=per["df_dt"] if streams else 0.5, **kw)
            rx = Band(B, n_total, odd(n_total + 2), 8, torch_dev, base_offset_bytes=8)
            p = chan_params(n_sig, n_pre, n_post, with_eoo, 0.4, 12.5, 0.5, Gb.ptr if Gb else None, nzb.ptr if nzb else None, seed)
            if streams:
                ps = chan_streams(per)
                r = L.rade_batch_channel_streams(h, txb.ptr, txb.stride, rx.ptr, rx.stride, C.byref(p), C.byref(ps), stream())
            else:
                r = L.rade_batch_channel(h, txb.ptr, txb.stride, rx.ptr, rx.stride, C.byref(p), stream())
            assert r == n_total
            sync()
            rx.check(what=f"rx_out {n_pre, n_post, with_eoo, with_G, with_noise, streams}"); ins.unchanged()
            assert np.array_equal(rx.rows(), bits(rx_d)), (n_pre, n_post, with_eoo, with_G, with_noise, streams)
            took |= {((rx.ptr + 8 * b * rx.stride) % 16 == 0, n_total % 2) for b in range(B)}
    assert took == {(True, 0), (True, 1), (False, 0), (False, 1)}      # the 16-byte and the 8-byte store, each with and without the tail store


@pytest.mark.parametrize("flags", [0, TX_BPF])
@pytest.mark.parametrize("with_G", [False, True])
def test_tx_channel_calls(torch_dev, flags, with_G):
    """rade_batch_tx_channel and rade_batch_tx_channel_streams (the fused modulator with G_dev on an engine without the Tx band-pass filter, else the two calls):
    banded iq_out and rx_out, n_mf = 3 of max_tx_mf = 4, odd n_total, G_dev 16-byte aligned as the contract asks, and refused when it is not"""
    import torch
    from radae_amd.engine import BatchEngine
    B, n_mf, cap = 3, 3, 4
    n_sig, n_pre, n_post = 960 * n_mf, 801, 1152
    rng = np.random.default_rng(8)
    f = feats(B, n_mf, seed=9)
    G_np = crandn(rng, B, n_sig, 2) if with_G else None
    per = {"sigma": np.array([0.2, 0.5, 0.8], np.float32), "freq_offset": np.array([5, -7, 31], np.float32), "df_dt": np.array([0, 0.5, -0.5], np.float32)}
    for streams in (False, True):
        with_eoo = not streams
        n_total = n_pre + n_sig + (1152 if with_eoo else 0) + n_post
        nz_np = crandn(rng, B, n_total)
        eng = BatchEngine(B, max_tx_mf=cap, flags=flags)
        L, h = eng.lib, eng.h
        rx_d, iq_d = eng.tx_channel(torch.tensor(f, device=torch_dev), per["sigma"] if streams else 0.3, per["freq_offset"] if streams else -9.0, n_pre, n_post, with_eoo,
                                    G=torch.tensor(G_np, device=torch_dev) if with_G else None, noise=torch.tensor(nz_np, device=torch_dev),
                                    df_dt=per["df_dt"] if streams else 0.25, want_iq=True)
        eng.tx_reset()
        ins = Inputs(torch_dev)
        fb = ins.put(f, 4); nzb = ins.put(nz_np, 8)
        Gb = ins.put(G_np, 8, off=0) if with_G else None
        iq = Band(B, n_sig, odd(n_sig + 8), 8, torch_dev, base_offset_bytes=8)
        rx = Band(B, n_total, odd(n_total + 4), 8, torch_dev, base_offset_bytes=8)
        ps = chan_streams(per)
        if with_G:
            # refused: G_dev 8 bytes off a 16-byte boundary -- rade_kernels.hip k_ofdm_mod_mp: `const f32x4 *Gb = (const f32x4 *)G + (size_t)b * n_mf * RD_NMF;`
            p = chan_params(n_sig, n_pre, n_post, with_eoo, 0.3, -9.0, 0.25, Gb.ptr + 8, nzb.ptr)
            assert L.rade_batch_tx_channel(h, fb.ptr, n_mf, iq.ptr, iq.stride, rx.ptr, rx.stride, C.byref(p), stream()) < 0
            assert L.rade_batch_tx_channel_streams(h, fb.ptr, n_mf, iq.ptr, iq.stride, rx.ptr, rx.stride, C.byref(p), C.byref(ps), stream()) < 0
            sync(); iq.untouched("iq_out of a refused call"); rx.untouched("rx_out of a refused call")
        p = chan_params(n_sig, n_pre, n_post, with_eoo, 0.3, -9.0, 0.25, Gb.ptr if Gb else None, nzb.ptr)
        if streams:
            r = L.rade_batch_tx_channel_streams(h, fb.ptr, n_mf, iq.ptr, iq.stride, rx.ptr, rx.stride, C.byref(p), C.byref(ps), stream())
        else:
            r = L.rade_batch_tx_channel(h, fb.ptr, n_mf, iq.ptr, iq.stride, rx.ptr, rx.stride, C.byref(p), stream())
        assert r == n_total
        sync()
        iq.check(what="iq_out"); rx.check(what="rx_out"); ins.unchanged()
        assert np.array_equal(iq.rows(), bits(iq_d)) and np.array_equal(rx.rows(), bits(rx_d)), streams
        eng.close()


def test_per_stream_channel_values_across_workgroups_of_64(engine, torch_dev):
    """B = 65: stream 64 is the first of k_chan_gain's second workgroup.  Its row of a per-stream call (banded, odd stride, odd n_total, Philox noise keyed by
    (seed, stream)) equals, bit for bit, its row of a uniform call carrying its values -- rade_batch_channel_streams and rade_batch_tx_channel_streams."""
    import torch
    B, n_mf = 65, 1
    n_sig, n_pre, n_post = 960, 1, 0
    n_total = n_pre + n_sig + 1152 + n_post
    rng = np.random.default_rng(65)
    f = feats(B, n_mf, seed=100)
    G_np = crandn(rng, B, n_sig, 2)
    per = {"sigma": rng.uniform(0.1, 1.0, B).astype(np.float32), "freq_offset": rng.uniform(-40, 40, B).astype(np.float32), "df_dt": rng.uniform(-1, 1, B).astype(np.float32)}
    eng = engine(B, max_tx_mf=2)
    L, h = eng.lib, eng.h
    ft, Gt = torch.tensor(f, device=torch_dev), torch.tensor(G_np, device=torch_dev)
    tx_d = eng.tx(ft)
    ins = Inputs(torch_dev)
    fb = ins.put(f, 4); Gb = ins.put(G_np, 8, off=0); txb = ins.put(tx_d.cpu().numpy(), 8, stride=odd(n_sig + 2))
    ps = chan_streams(per)
    p = chan_params(n_sig, n_pre, n_post, True, 0.0, 0.0, 0.0, Gb.ptr, None, seed=5)
    rx = Band(B, n_total, odd(n_total + 2), 8, torch_dev, base_offset_bytes=8)
    assert L.rade_batch_channel_streams(h, txb.ptr, txb.stride, rx.ptr, rx.stride, C.byref(p), C.byref(ps), stream()) == n_total
    sync(); rx.check(what="rx_out"); ins.unchanged()
    assert np.array_equal(rx.rows(), bits(eng.channel(tx_d, per["sigma"], per["freq_offset"], n_pre, n_post, True, G=Gt, seed=5, df_dt=per["df_dt"])))
    for b in (0, 63, 64):
        uni = eng.channel(tx_d, float(per["sigma"][b]), float(per["freq_offset"][b]), n_pre, n_post, True, G=Gt, seed=5, df_dt=float(per["df_dt"][b]))
        assert np.array_equal(rx.rows()[b], bits(uni)[b]), b
    eng.tx_reset()
    rx2 = Band(B, n_total, odd(n_total + 6), 8, torch_dev, base_offset_bytes=8)
    iq = Band(B, n_sig, odd(n_sig + 2), 8, torch_dev, base_offset_bytes=8)
    assert L.rade_batch_tx_channel_streams(h, fb.ptr, n_mf, iq.ptr, iq.stride, rx2.ptr, rx2.stride, C.byref(p), C.byref(ps), stream()) == n_total
    sync(); rx2.check(what="rx_out (tx_channel)"); iq.check(what="iq_out (tx_channel)"); ins.unchanged()
    for b in (0, 63, 64):
        eng.tx_reset()
        uni, uiq = eng.tx_channel(ft, float(per["sigma"][b]), float(per["freq_offset"][b]), n_pre, n_post, True, G=Gt, seed=5, df_dt=float(per["df_dt"][b]), want_iq=True)
        assert np.array_equal(rx2.rows()[b], bits(uni)[b]), b
        assert np.array_equal(iq.rows(), bits(uiq))


def test_channel_8_byte_store_branch_against_the_oracle(engine, torch_dev, oracle, oracle_model):
    """odd rx_stride, odd n_total, explicit noise: stream 1's row starts 8 bytes off a 16-byte boundary, so k_chan_apply writes it with the two 8-byte stores and
    the tail store.  Its samples against oracle.channel + oracle.channel_eoo at test_full_chain_vs_oracle_fresh_inputs' bar (max abs < 5e-5)."""
    import torch
    from radae_amd.channel_tools import multipath_g
    from radae_amd.engine import sigma_from_EbNodB
    B, n_mf = 2, 4
    n_sig, n_pre, n_post = 960 * n_mf, 801, 1152
    n_total = n_pre + n_sig + 1152 + n_post
    assert n_total % 2 == 1
    rng = np.random.default_rng(31)
    f = feats(B, n_mf, seed=50)
    G_np = np.stack([multipath_g("mpp", 8000, n_sig, 60 + b) for b in range(B)]).astype(np.complex64)
    nz_np = crandn(rng, B, n_total)
    sigma, fo = sigma_from_EbNodB(6.0), -11.0
    eng = engine(B, max_tx_mf=n_mf)
    L, h = eng.lib, eng.h
    tx_d = eng.tx(torch.tensor(f, device=torch_dev))
    ins = Inputs(torch_dev)
    txb = ins.put(tx_d.cpu().numpy(), 8, stride=odd(n_sig + 2)); Gb = ins.put(G_np, 8); nzb = ins.put(nz_np, 8)
    rx = Band(B, n_total, odd(n_total + 2), 8, torch_dev, base_offset_bytes=0)
    assert (rx.ptr + 8 * rx.stride) % 16 == 8                           # stream 1: the 8-byte stores
    p = chan_params(n_sig, n_pre, n_post, True, sigma, fo, 0.0, Gb.ptr, nzb.ptr)
    assert L.rade_batch_channel(h, txb.ptr, txb.stride, rx.ptr, rx.stride, C.byref(p), stream()) == n_total
    sync(); rx.check(what="rx_out"); ins.unchanged()
    tx = oracle.Tx(oracle_model)
    sig = np.concatenate([tx.frame(f[1, 12 * k:12 * k + 12].ravel())[0] for k in range(n_mf)])
    assert np.abs(tx_d.cpu().numpy()[1] - sig).max() < 5e-5
    nz = nz_np[1]
    r, fin = oracle.channel(sig, G_np[1], nz[n_pre:n_pre + n_sig], sigma, fo)
    e = oracle.channel_eoo(tx.eoo(), nz[n_pre + n_sig:n_pre + n_sig + 1152], sigma, fo, 0.0, fin)
    full = np.concatenate([sigma * nz[:n_pre], r, e, sigma * nz[-n_post:]]).astype(np.complex64)
    got = rx.rows(np.complex64)[1]
    print("8-byte-store branch against the oracle: max abs", np.abs(got - full).max())
    assert np.abs(got - full).max() < 5e-5


# ---- symbol-domain channels and the Doppler generator -----------------------------------------------------------------------------------------------------
def test_channel_symbol_and_multipath(engine, torch_dev):
    """rade_batch_channel_symbol (both modes), rade_batch_multipath_gen, rade_batch_multipath_h: guards around the outputs, inputs untouched; n_out not a
    multiple of low_ratio and the smallest n_out (1: two low-rate points are still made)"""
    import torch
    from radae_amd.channel_tools import PRESETS, doppler_plan
    B, n = 3, 5
    rng = np.random.default_rng(12)
    eng = engine(B, max_tx_mf=2)
    L, h = eng.lib, eng.h
    z_np = np.tanh(rng.standard_normal((B, n, 80))).astype(np.float32)
    zt = torch.tensor(z_np, device=torch_dev)
    for mode, hw in (("rs", 40), ("bbfm", 80)):
        H_np = (0.5 + rng.random((B, n * hw))).astype(np.float32)
        nz_np = rng.standard_normal((B, n * 80)).astype(np.float32)
        for explicit in (True, False):
            p0, p1 = (0.3, 0.0) if mode == "rs" else (20.0, 10.0)
            d = eng.channel_symbol(zt, mode, p0, p1, H=torch.tensor(H_np, device=torch_dev), noise=torch.tensor(nz_np, device=torch_dev) if explicit else None, seed=0 if explicit else 9)
            ins = Inputs(torch_dev)
            zb = ins.put(z_np, 4); Hb = ins.put(H_np, 4); nzb = ins.put(nz_np, 4)
            out = Band(1, B * n * 80, B * n * 80, 4, torch_dev, base_offset_bytes=4)
            assert L.rade_batch_channel_symbol(h, zb.ptr, Hb.ptr, nzb.ptr if explicit else None, out.ptr, n, 0 if mode == "rs" else 1, p0, p1, 0 if explicit else 9, stream()) == n
            sync(); out.check(what=f"z_hat {mode}"); ins.unchanged()
            assert np.array_equal(out.rows().reshape(B, -1), bits(d)), (mode, explicit)
    for n_out in (1, 1001, 1600):
        taps, ratio, n_low = doppler_plan(PRESETS["mpp"][0], 8000, n_out)
        assert (n_out % ratio != 0) == (n_out != 1600) and n_low >= 2
        tp = np.ascontiguousarray(taps, np.float32)
        nl_np = (rng.standard_normal((B, 2, n_low + len(tp))) + 1j * rng.standard_normal((B, 2, n_low + len(tp)))).astype(np.complex64)
        for explicit in (True, False):
            d = eng.multipath_gen("mpp", n_out, seed=4, noise_low=torch.tensor(nl_np, device=torch_dev) if explicit else None)
            ins = Inputs(torch_dev)
            nlb = ins.put(nl_np, 8)
            G = Band(1, B * n_out * 2, B * n_out * 2, 8, torch_dev, base_offset_bytes=8)
            assert L.rade_batch_multipath_gen(h, tp.ctypes.data_as(C.POINTER(C.c_float)), len(tp), ratio, n_out, nlb.ptr if explicit else None, 4, G.ptr, stream()) == n_out
            sync(); G.check(what=f"G_out n_out {n_out}"); ins.unchanged()
            assert np.array_equal(G.rows().reshape(B, -1), bits(d)), (n_out, explicit)
    n_g, M, n_sym, Nc = 25, 4, 7, 3
    G_np = crandn(rng, B, n_g, 2)
    Gt = torch.tensor(G_np, device=torch_dev)
    for cplx in (0, 1):
        d = torch.empty((B, n_sym * Nc * (1 + cplx)), dtype=torch.float32, device=torch_dev)
        assert L.rade_batch_multipath_h(h, Gt.data_ptr(), n_g, M, n_sym, Nc, 0.002, 2000.0, cplx, d.data_ptr(), stream()) == n_sym
        ins = Inputs(torch_dev)
        Gb = ins.put(G_np, 8)
        H = Band(1, B * n_sym * Nc * (1 + cplx), B * n_sym * Nc * (1 + cplx), 4, torch_dev, base_offset_bytes=4)
        assert L.rade_batch_multipath_h(h, Gb.ptr, n_g, M, n_sym, Nc, 0.002, 2000.0, cplx, H.ptr, stream()) == n_sym
        sync(); H.check(what="H_out"); ins.unchanged()
        assert np.array_equal(H.rows().reshape(B, -1), bits(d)) and np.isfinite(H.rows(np.float32)).all()


# ---- receivers ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [("awgn", 0), ("awgn", BYPASS_DEC), ("mpp", 0)])
def test_rx(torch_dev, golden, name, flags):
    """rade_batch_rx on a golden rxtrace input: banded rx_dev (rx_stride > n_avail, odd, odd sample offset), feat_stride not a multiple of 432 (capacity is the
    floor; a multiple of 240 under RADE_BATCH_BYPASS_DEC), guards around features_out and eoo_out, rows past n_valid and the whole row of a stream whose
    n_avail is too small for one call stay sentinel; the integer trace keys equal the golden's, so the dense run is itself anchored."""
    import torch
    from radae_amd.engine import BatchEngine, RxStatus
    g = golden("rxtrace_" + name)
    x = g["rx_in"].astype(np.complex64)
    B, N = 3, len(x)
    row = 240 if flags & BYPASS_DEC else 432
    avail = np.array([N, N - 1000, 500], np.int32)                    # stream 2: fewer samples than one call needs (rade_nin: 960 in search)
    xs = np.stack([x, x, x])
    eng = BatchEngine(B, rx_trace_calls=64, flags=flags)
    fd, st_d, eoo_d = eng.rx(torch.tensor(xs, device=torch_dev), n_avail=avail)
    tr = eng.rx_trace(0)
    for k in INT_KEYS if not flags else []:                          # (the golden traces are the decoding receiver's: UW errors are not counted under BYPASS_DEC)
        assert np.array_equal(tr[k], g[k]), k
    nv = [s.n_valid for s in st_d]
    assert nv[0] == len(g["features_out"]) and 0 < nv[1] <= nv[0] and nv[2] == 0 and st_d[2].n_calls == 0 and st_d[2].consumed == 0
    eng.close()

    eng = BatchEngine(B, rx_trace_calls=64, flags=flags)
    L, h = eng.lib, eng.h
    ins = Inputs(torch_dev)
    xb = ins.put(xs, 8, stride=odd(N + 10))
    cap = nv[0] + 2
    fstride = row * cap + (0 if flags & BYPASS_DEC else 101)
    fo = Band(B, row * cap, fstride, 4, torch_dev, base_offset_bytes=4)
    eoo = Band(B, 180, 180, 4, torch_dev, base_offset_bytes=4)
    st = (RxStatus * B)()
    assert L.rade_batch_rx(h, xb.ptr, xb.stride, avail.ctypes.data_as(C.POINTER(C.c_int)), 1 << 20, fo.ptr, fstride, eoo.ptr, st, stream()) == 0
    sync()
    for a, b in zip(st, st_d):
        assert [getattr(a, k) for k, _ in RxStatus._fields_] == [getattr(b, k) for k, _ in RxStatus._fields_]
    fo.check(written=[row * v for v in nv], what="features_out"); ins.unchanged()
    eoo.check(written=[180 if s.has_eoo else 0 for s in st], what="eoo_out")
    assert (g["eoo_out"].size > 0) == bool(st[0].has_eoo)
    for b in range(B):
        assert np.array_equal(fo.rows()[b, :row * nv[b]], bits(fd)[b, :row * nv[b]]), b
        if st[b].has_eoo:
            assert np.array_equal(eoo.rows()[b], bits(eoo_d)[b]), b
    tr2 = eng.rx_trace(0)
    for k in INT_KEYS:
        assert np.array_equal(tr2[k], g[k] if not flags else tr[k]), k
    # a capacity below what the stream would fill: it pauses, and nothing is written past the floor of feat_stride / row rows
    eng.rx_reset()
    cap2 = nv[0] - 3
    fo2 = Band(B, row * cap2, row * cap2 + row - 1, 4, torch_dev, base_offset_bytes=4)
    assert L.rade_batch_rx(h, xb.ptr, xb.stride, avail.ctypes.data_as(C.POINTER(C.c_int)), 1 << 20, fo2.ptr, fo2.stride, None, st, stream()) == 0
    sync()
    assert st[0].n_valid == cap2 and st[0].consumed < N
    fo2.check(written=[row * min(v, cap2) for v in nv], what="features_out at capacity"); ins.unchanged()
    assert np.array_equal(fo2.rows()[0], bits(fd)[0, :row * cap2])
    eng.close()


@pytest.mark.parametrize("n_mf", [2, 9])
def test_rx_ideal(engine, torch_dev, golden, n_mf):
    """rade_batch_rx_ideal: rx_stride > n_mf * 960 (odd, odd sample offset), n_mf = 2 (the minimum) and a larger one, guards around z_hat_dev and
    features_out_dev, n_errors_host written for exactly B entries (host guards)"""
    import torch
    from radae_amd.engine import IdealRxParams
    g = golden("chan_mpp")
    B = 3
    rx_np = np.stack([np.roll(g["rx"][:n_mf * 960 + 960], -960 * b)[:n_mf * 960] for b in range(B)]).astype(np.complex64)
    fo_np = np.array([float(g["freq_offset"]), 0.0, -3.0], np.float32); df_np = np.array([0.0, 0.5, 0.0], np.float32)
    zref_np = np.sign(np.random.default_rng(1).standard_normal((B, 3 * n_mf, 80))).astype(np.float32)
    eng = engine(B, max_tx_mf=12)
    L, h = eng.lib, eng.h
    f_d, z_d, e_d = eng.rx_ideal(torch.tensor(rx_np, device=torch_dev), n_mf, freq_offset=fo_np, df_dt=df_np, z_ref=torch.tensor(zref_np, device=torch_dev))
    assert e_d.min() > 0
    ins = Inputs(torch_dev)
    xb = ins.put(rx_np, 8, stride=odd(n_mf * 960 + 20)); zr = ins.put(zref_np, 4)
    zh = Band(1, B * 3 * n_mf * 80, B * 3 * n_mf * 80, 4, torch_dev)
    ft = Band(1, B * 3 * n_mf * 84, B * 3 * n_mf * 84, 4, torch_dev, base_offset_bytes=4)
    nerr = Band(1, B, B, 8)                                             # host: C long
    p = IdealRxParams(-16, 0, 1, fo_np.ctypes.data, df_np.ctypes.data, zr.ptr, nerr.ptr)
    # refused: z_hat_dev off a 16-byte boundary while the decoder is asked for -- rade_kernels.hip k_gemm_splitk: `const f32x4 av = *(const f32x4 *)p;` (decoder dense1 reads z_hat rows)
    assert L.rade_batch_rx_ideal(h, xb.ptr, xb.stride, n_mf, C.byref(p), zh.ptr + 4, ft.ptr, stream()) < 0
    sync(); zh.untouched("z_hat of a refused call"); ft.untouched("features_out of a refused call"); nerr.untouched("n_errors of a refused call")
    assert L.rade_batch_rx_ideal(h, xb.ptr, xb.stride, n_mf, C.byref(p), zh.ptr, ft.ptr, stream()) == n_mf
    sync()
    zh.check(what="z_hat"); ft.check(what="features_out"); nerr.check(what="n_errors_host"); ins.unchanged()
    assert np.array_equal(zh.rows().reshape(B, -1), bits(z_d)) and np.array_equal(ft.rows().reshape(B, -1), bits(f_d))
    assert np.array_equal(nerr.rows(np.int64)[0], e_d)
    # without the decoder z_hat_dev needs its natural alignment only
    zh2 = Band(1, B * 3 * n_mf * 80, B * 3 * n_mf * 80, 4, torch_dev, base_offset_bytes=4)
    p = IdealRxParams(-16, 0, 1, fo_np.ctypes.data, df_np.ctypes.data, None, None)
    assert L.rade_batch_rx_ideal(h, xb.ptr, xb.stride, n_mf, C.byref(p), zh2.ptr, None, stream()) == n_mf
    sync(); zh2.check(what="z_hat without the decoder"); ins.unchanged()
    assert np.array_equal(zh2.rows().reshape(B, -1), bits(z_d))


# ---- scoring ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f_row,h_row", [(20, 36), (36, 37), (37, 20)])
def test_loss(engine, torch_dev, oracle, f_row, h_row):
    """rade_batch_loss: f_row / h_row in {20, 36, 37}, f_stride / h_stride above the minimum, fl_stride larger than every n_hat; frame-loss entries past
    n_hat - start and the rows of unscored streams stay sentinel; loss_host / start_host between host guards; loss and start equal oracle.find_loss"""
    from radae_amd.channel_tools import synth_features
    rng = np.random.default_rng(5)
    base = synth_features(11, 400)[:, :20]
    noisy = lambda a: (a + 0.05 * rng.standard_normal(a.shape)).astype(np.float32)
    cases = [(base[:300], noisy(base[37:237])), (base[:100], base[:0]), (base[:30], noisy(base[:40])), (base[50:350], noisy(base[120:300])), (base[:50], base[20:21])]
    B = len(cases)
    n_in = np.array([len(c[0]) for c in cases], np.int32); n_hat = np.array([len(c[1]) for c in cases], np.int32)
    scored = (n_hat > 0) & (n_hat <= n_in)

    def pack(arrs, w):
        out = rng.standard_normal((B, max(len(a) for a in arrs), w)).astype(np.float32)      # columns past 20 hold noise: they must not matter
        for b, a in enumerate(arrs):
            out[b, :len(a), :20] = a
        return out
    F, H = pack([c[0] for c in cases], f_row), pack([c[1] for c in cases], h_row)
    eng = engine(B)
    L, h = eng.lib, eng.h
    ins = Inputs(torch_dev)
    Fb = ins.put(F, 4, stride=F.shape[1] * f_row + 13); Hb = ins.put(H, 4, stride=H.shape[1] * h_row + 7)
    fl = Band(B, int(n_hat.max()) + 5, int(n_hat.max()) + 8, 4, torch_dev, base_offset_bytes=4)
    loss, start = Band(1, B, B, 8), Band(1, B, B, 4)                    # host
    r = L.rade_batch_loss(h, Fb.ptr, Fb.stride, f_row, n_in.ctypes.data, Hb.ptr, Hb.stride, h_row, n_hat.ctypes.data, loss.ptr, start.ptr, fl.ptr, fl.stride, stream())
    assert r == int(scored.sum()) == 3
    sync()
    loss.check(what="loss_host"); start.check(what="start_host"); ins.unchanged()
    lv, sv = loss.rows(np.float64)[0], start.rows(np.int32)[0]
    fl.check(written=[max(int(n_hat[b] - sv[b]), 0) if scored[b] else 0 for b in range(B)], what="frame_loss")
    for b, (f, hh) in enumerate(cases):
        if not scored[b]:
            assert np.isnan(lv[b]) and sv[b] == -1, b
            continue
        lo, so = oracle.find_loss(np.ascontiguousarray(f), np.ascontiguousarray(hh))
        assert lv[b] == lo and sv[b] == so, (b, lv[b], lo, sv[b], so)
        want = np.array([oracle.distortion_loss(np.ascontiguousarray(f[so + k:so + k + 1]), np.ascontiguousarray(hh[k:k + 1])) for k in range(len(hh) - so)])
        assert np.array_equal(fl.rows(np.float32)[b, :len(want)].astype(np.float64), want), b
    # the dense call (stride = the buffer's rows, through the wrapper) gives the same bits
    import torch
    l2, s2, fl2 = eng.loss(torch.tensor(F, device=torch_dev), torch.tensor(H, device=torch_dev), n_in=n_in, n_hat=n_hat, frame_loss=True)
    assert np.array_equal(l2.view(np.int64), lv.view(np.int64)) and np.array_equal(s2, sv)
    for b in np.flatnonzero(scored):
        k = max(int(n_hat[b] - sv[b]), 0)
        assert np.array_equal(bits(fl2)[b, :k], fl.rows()[b, :k])
    # fl_stride below a scored n_hat is refused on the host: rade_loss.hip k_loss_frames writes `a.frame_loss[(size_t)b * a.fl_stride + f]` for f < n_hat - start
    fl3 = Band(B, int(n_hat.max()) - 1, int(n_hat.max()) - 1, 4, torch_dev)
    assert L.rade_batch_loss(h, Fb.ptr, Fb.stride, f_row, n_in.ctypes.data, Hb.ptr, Hb.stride, h_row, n_hat.ctypes.data, loss.ptr, start.ptr, fl3.ptr, fl3.stride, stream()) < 0
    sync(); fl3.untouched("frame_loss of a refused call")


# ---- single-carrier modem ---------------------------------------------------------------------------------------------------------------------------------
def test_sc_tx_rx(torch_dev):
    """rade_sc_tx / rade_sc_rx: iq_stride and rx_stride above the row (odd, odd sample offset), guards around every output, the frames past status.n_frames of
    payload / zhat / frames stay sentinel, symbols and samples in are untouched"""
    import torch
    from radae_amd.sc import ScStatus, SingleCarrierBatch, _FRAME_DT
    B, NF = 3, 4
    rng = np.random.default_rng(6)
    sy = (1 - 2 * (rng.random((B, NF, 80)) > 0.5)).astype(np.float32)
    m = SingleCarrierBatch(B, fcentreHz=1500.0)
    tx_d = m.tx(torch.tensor(sy, device=torch_dev))
    n = NF * 384
    rx_np = np.zeros((B, n + 40), np.complex64)
    for b in range(B):
        rx_np[b, 7 * b:7 * b + n] = tx_d.cpu().numpy()[b] * np.exp(1j * (0.3 + b)) + 0.02 * crandn(rng, n)
    F = NF + 2
    pay_d, zh_d, fr_d, st_d = m.rx(torch.tensor(rx_np, device=torch_dev), max_frames=F)
    m.close()
    m = SingleCarrierBatch(B, fcentreHz=1500.0)
    L, h = m.L, m.h
    ins = Inputs(torch_dev)
    sb = ins.put(sy, 4)
    iq = Band(B, n, odd(n + 4), 8, torch_dev, base_offset_bytes=8)
    # refused on the host (rade_sc_tx's own argument check): k_sc_tx writes `out[(size_t)b * out_stride + (size_t)f * SC_NFRAME * SC_M + i]` for f < n_frames
    assert L.rade_sc_tx(h, sb.ptr, NF, iq.ptr, n - 1, m._stream()) < 0
    sync(); iq.untouched("iq_out of a refused call")
    assert L.rade_sc_tx(h, sb.ptr, NF, iq.ptr, iq.stride, m._stream()) == n
    sync(); iq.check(what="sc iq_out"); ins.unchanged()
    assert np.array_equal(iq.rows(), bits(tx_d))
    xb = ins.put(rx_np, 8, stride=odd(n + 40 + 2))
    pay = Band(B, F * 80, F * 80, 8, torch_dev, base_offset_bytes=8)
    zh = Band(B, F * 80, F * 80, 4, torch_dev, base_offset_bytes=4)
    fr = Band(B, F, F, _FRAME_DT.itemsize, torch_dev)
    st = (ScStatus * B)()
    assert L.rade_sc_rx(h, xb.ptr, xb.stride, n + 40, F, pay.ptr, zh.ptr, fr.ptr, C.cast(st, C.c_void_p), m._stream()) == 0
    sync()
    nf = [s.n_frames for s in st]
    assert nf == [s.n_frames for s in st_d] and 0 < max(nf) < F
    pay.check(written=[80 * k for k in nf], what="sc payload"); zh.check(written=[80 * k for k in nf], what="sc zhat"); fr.check(written=nf, what="sc frames"); ins.unchanged()
    for b in range(B):
        assert np.array_equal(pay.rows()[b, :160 * nf[b]], bits(pay_d)[b, :160 * nf[b]]) and np.array_equal(zh.rows()[b, :80 * nf[b]], bits(zh_d)[b, :80 * nf[b]])
        assert np.array_equal(fr.rows()[b, :12 * nf[b]], fr_d[b, :nf[b]].view(np.int32).ravel())
        assert [getattr(st[b], k) for k, _ in ScStatus._fields_] == [getattr(st_d[b], k) for k, _ in ScStatus._fields_]
    m.close()
