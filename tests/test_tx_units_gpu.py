"""GPU unit tests (-m gpu) of the transmit half of the timed step, the channel and the row kernels, each called alone through its launch shim of
radae_amd/csrc/rade_dev.h on synthetic operands: k_encf_dense1; k_enc_pack, k_pad_rows, k_carry_rows; k_ofdm_mod<linear|limiter>, k_ofdm_mod_mp<...>, k_eoo_build,
k_copy_eoo; k_chan_power / k_chan_gain / k_chan_apply behind rd_launch_channel; k_multipath_gen, k_multipath_h.  The companion of tests/test_kernel_units_gpu.py
(the Dev helper, sync and stream of both are tests/gpu_kit.py's): torch tensors are the device memory, every output sits in a NaN-sentinel buffer and must leave everything
outside its documented elements untouched, every input must be unchanged, and every sample is held to a float64 reference -- bit for bit where the operation is
data movement or an exact grid, within the bound tests/tx_ref.py derives otherwise.  The checkers are those of tests/tx_ref.py; tests/test_tx_units_host.py shows
that each of them rejects the bugs it is there for.  One engine per module supplies the device copy of the constant tables (rd_batch_tables).

Shapes are the smallest at which a kernel can still go wrong (a row past a 32-row tile, a frame boundary, an odd last sample, one point past DG_MAXLOW), not the
workload's.  The generated-noise paths stay with tests/test_device_noise_gpu.py: every channel case passes an explicit noise tensor."""
import ctypes as C

import numpy as np
import pytest

import dev_abi
import kernel_ref as kr
import tx_ref as tx
from gpu_kit import Dev, host32, stream, sync, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(torch_dev):
    return dev_abi.load()


@pytest.fixture(scope="module")
def tab(L):
    return tx.Tab(L)


@pytest.fixture(scope="module")
def dtab(L, torch_dev):
    """the engine's device copy of rd_tables"""
    from radae_amd.engine import BatchEngine
    eng = BatchEngine(3, max_tx_mf=1)
    p = L.rd_batch_tables(eng.h)
    assert p
    yield p
    eng.close()


def crows(B, n, stride, off=2, T=1):
    """complex64 rows: n samples of stream b at sample b stride of a pointer `off` floats into a sentinel-filled allocation"""
    return kr.Rows(B, T, 2 * n, 2 * stride, 2 * stride * T, off=off)


def dense(n_words):
    """a dense output of n_words float32 words between two guards of sentinels"""
    return kr.Rows(1, 1, n_words, n_words, n_words)


def cplx(rows, words):
    """the complex64 samples [B][n] of a crows buffer"""
    v = np.ascontiguousarray(rows.view(words)[:, 0])
    return v.view(np.complex64)


def crand(rng, shape, scale=1.0):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * (scale / np.sqrt(2))).astype(np.complex64)


# ================================================================================================================================================================
# A. k_encf_dense1
# ================================================================================================================================================================
def run_dense1(L, dev, B, T, Kin, ycol, X, W, bias, act):
    """X [B][T][Kin] float32 rows -> the 64 outputs as (joined float32 [B][T][64], (hi, lo) planes) after the sentinel and input checks"""
    NQ = 1 + (T + 31) // 32
    d = Dev(dev)
    wp = kr.pack_f32(L, W)
    assert wp.size >= (Kin // 8) * 512                                 # what the kernel streams: Kin / 8 k-blocks of two column tiles
    x_d, w_d, b_d = d.put(np.ascontiguousarray(X, np.float32)), d.put(wp), d.put(bias)
    yf0 = kr.frag_new(B, NQ)
    y_d = d.put(yf0, check=False)
    a = kr.EncfArgs()
    a.NQ, a.B, a.T, a.N, a.act, a.Kin, a.ycol = NQ, B, T, 64, act, Kin, ycol
    a.xin, a.Wp, a.bias, a.yf = x_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), y_d.data_ptr()
    assert L.rd_launch_encf_dense1(C.byref(a), stream()) == 0
    sync()
    d.unchanged()
    what = f"k_encf_dense1 B={B} T={T} Kin={Kin} ycol={ycol} act={act}"
    buf = y_d.cpu().numpy().view(np.uint16).reshape(B, NQ, kr.EF_TILE)
    kr.frag_untouched_except(buf, yf0, [kr.frag_index(np.arange(T), ycol, 64)], what)       # rows T.. of the last tile, the history tile, every other column
    hi, lo = kr.frag_get(buf, np.arange(T), ycol, 64)
    return kr.join16(hi, lo), (hi, lo), what


@pytest.mark.parametrize("Kin", [8, 16, 96])
@pytest.mark.parametrize("B", [1, 3])
def test_encf_dense1(L, torch_dev, B, Kin):
    """Kin = 8: one k-block, the prefetch branch never taken; 96: the engine's.  Exact grid (act 0; sums below 2^22 quanta, so that the two planes hold the
    result exactly): the planes equal split16 of the float64 result.  Random (act 1, tanhf): stream b's inputs are +-300, +-1e5 (the unbounded operand this
    kernel exists for), +-1; tanh is monotone, so a pre-activation within +-d of y (d = kernel_ref.gemm_bound) gives an output between tanh(y - d) and
    tanh(y + d) -- never looser than the 1-Lipschitz d -- plus tanhf's epsilon and the 2^-22 of the planes; |out| <= 1."""
    for T in (1, 31, 32, 33, 70):
        for ycol in (0, 160):
            rng = np.random.default_rng(1000 * B + 10 * T + Kin)
            X, W, _, bias = kr.exact_gemm_operands(rng, B * T, Kin, 64, "int8", 22)
            y64, _ = kr.gemm_ref(X, W, bias)
            want = y64.astype(np.float32).reshape(B, T, 64)
            assert np.array_equal(want.astype(np.float64).ravel(), y64.ravel()) and np.array_equal(kr.join16(*kr.split16(want)), want)
            got, planes, what = run_dense1(L, torch_dev, B, T, Kin, ycol, X.reshape(B, T, Kin), W, bias, 0)
            kr.encf_check_exact(got, planes, want, what + " exact grid")
            _, W, _, bias = kr.random_gemm_operands(rng, 1, Kin, 64)
            X = rng.uniform(-1, 1, (B, T, Kin)).astype(np.float32) * np.array([300.0, 1e5, 1.0], np.float32)[np.arange(B) % 3][:, None, None]
            y64, S = kr.gemm_ref(X.reshape(B * T, Kin), W, bias)
            dlt = kr.gemm_bound(Kin, S, y64, 0.0)
            t64 = np.tanh(y64)
            bound = np.maximum(np.tanh(y64 + dlt) - t64, t64 - np.tanh(y64 - dlt)) + kr.EPS_TANH_LIBM + 2.0 ** -22 * np.abs(t64) + 2.0 ** -33
            got, _, what = run_dense1(L, torch_dev, B, T, Kin, ycol, X, W, bias, 1)
            assert np.all(np.abs(got) <= 1), what + ": |out| > 1"
            r = tx.check_close(got, t64.reshape(B, T, 64), bound.reshape(B, T, 64), what + " random", ("stream", "step", "column"))
            print(f"{what}: largest error / bound {r:.3f}")


# ================================================================================================================================================================
# B. row kernels: bit-exact data movement
# ================================================================================================================================================================
@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (4, 2800)], ids=["1x1", "3x5", "grid-stride"])
def test_enc_pack(L, torch_dev, B, T):
    """features [B][4 T][36] -> [B][T][96]; 4 x 2800 rows of 96 are more than 4096 x 256 elements: the grid-stride loop runs twice for some threads"""
    rng = np.random.default_rng(B + T)
    feats = rng.standard_normal((B, 4 * T, 36)).astype(np.float32)
    out = kr.Rows(1, B * T, 96, 96, B * T * 96)
    d = Dev(torch_dev)
    f_d, o_d = d.put(feats), d.put(out.words, check=False)
    assert L.rd_launch_enc_pack(f_d.data_ptr(), o_d.data_ptr() + 4 * out.base, B, T, stream()) == 0
    sync()
    d.unchanged()
    tx.check_rows(out, host32(o_d), tx.pack_ref(feats).reshape(1, B * T, 96), f"k_enc_pack B={B} T={T}")


@pytest.mark.parametrize("R,K,Kpad", [(1, 80, 80), (15, 80, 80), (1, 84, 88), (15, 84, 88), (1, 1, 8), (15, 1, 8), (11200, 84, 96)])
def test_pad_rows(L, torch_dev, R, K, Kpad):
    rng = np.random.default_rng(R + K)
    src = rng.standard_normal((R, K)).astype(np.float32)
    out = kr.Rows(1, R, Kpad, Kpad, R * Kpad)
    d = Dev(torch_dev)
    s_d, o_d = d.put(src), d.put(out.words, check=False)
    assert L.rd_launch_pad_rows(s_d.data_ptr(), o_d.data_ptr() + 4 * out.base, R, K, Kpad, stream()) == 0
    sync()
    d.unchanged()
    tx.check_rows(out, host32(o_d), tx.pad_ref(src, Kpad).reshape(1, R, Kpad), f"k_pad_rows R={R} K={K} Kpad={Kpad}")


CARRY_TCAP = 5


def run_carry(L, dev, x, W, nhist, T, n_rows):
    B = x.shape[0]
    rows = kr.Rows(B, nhist + CARRY_TCAP, W, W, (nhist + CARRY_TCAP) * W).fill(x)
    d = Dev(dev)
    x_d = d.put(rows.words, check=False)
    n_d = d.put(np.asarray(n_rows, np.int32)) if n_rows is not None else None
    r = L.rd_launch_carry_rows(x_d.data_ptr() + 4 * rows.base, B, CARRY_TCAP, W, nhist, T, n_d.data_ptr() if n_rows is not None else None, stream())
    sync()
    d.unchanged()
    return r, rows, host32(x_d)


@pytest.mark.parametrize("W,nhist", [(864, 2), (736, 1)])
def test_carry_rows(L, torch_dev, W, nhist):
    """rows [T, T + nhist) -> rows [0, nhist) in place, every other word of the buffer unchanged; T = 1 with nhist = 2: source and destination overlap;
    a stream with n_rows 0 or -1 is left alone"""
    rng = np.random.default_rng(W)
    B = 3
    x = rng.standard_normal((B, nhist + CARRY_TCAP, W)).astype(np.float32)
    for T in (1, 2, 3, CARRY_TCAP):
        for n_rows in (None, [T, 0, -1], [1, T, CARRY_TCAP]):
            r, rows, words = run_carry(L, torch_dev, x, W, nhist, T if n_rows is None else 0, n_rows)
            assert r == 0
            tx.check_rows(rows, words, tx.carry_ref(x, nhist, T, n_rows), f"k_carry_rows W={W} nhist={nhist} T={T} n_rows={n_rows}")


@pytest.mark.parametrize("W,nhist", [(864, 3), (2049, 1), (864, 0), (864, -1)])
def test_carry_rows_refuses_what_it_cannot_hold(L, torch_dev, W, nhist):
    """a workgroup holds nhist W <= 2048 floats in registers: beyond that (and for nhist < 1) the shim returns -1, launches nothing, and the buffer is untouched"""
    rng = np.random.default_rng(W)
    x = rng.standard_normal((2, max(nhist, 0) + CARRY_TCAP, W)).astype(np.float32)
    rows = kr.Rows(2, x.shape[1], W, W, x.shape[1] * W).fill(x)
    d = Dev(torch_dev)
    x_d = d.put(rows.words)
    assert L.rd_launch_carry_rows(x_d.data_ptr() + 4 * rows.base, 2, CARRY_TCAP, W, nhist, 1, None, stream()) == -1
    sync()
    d.unchanged()


# ================================================================================================================================================================
# C. modulator and end-of-over frame
# ================================================================================================================================================================
def mod_latents(rng, B, n_mf):
    """stream b: the same uniform +-1 latents x (1, 8: deep in the limiter, 2^-10: its cancelling region); frame 1 of stream 0 is all zeros (n_mf = 1: see the zero case)"""
    z = rng.uniform(-1, 1, (1, 3 * n_mf, 80)).astype(np.float32) * np.array([1.0, 8.0, 2.0 ** -10], np.float32)[np.arange(B) % 3][:, None, None]
    if n_mf > 1:
        z[0, 3:6] = 0
    return z


def run_mod(L, dev, dtab, z, linear):
    B, n_mf = z.shape[0], z.shape[1] // 3
    out = crows(B, 960 * n_mf, 960 * n_mf + 7)
    d = Dev(dev)
    z_d, o_d = d.put(z), d.put(out.words, check=False)
    assert L.rd_launch_ofdm_mod(dtab, z_d.data_ptr(), o_d.data_ptr() + 4 * out.base, 960 * n_mf + 7, B, n_mf, linear, stream()) == 0
    sync()
    d.unchanged()
    words = host32(o_d)
    out.check_outside(words, f"k_ofdm_mod linear={linear} B={B} n_mf={n_mf}")
    return cplx(out, words)


@pytest.mark.parametrize("linear", [0, 1])
@pytest.mark.parametrize("B,n_mf", [(1, 1), (1, 2), (1, 5), (3, 1), (3, 2), (3, 5)])
def test_ofdm_mod(L, torch_dev, dtab, tab, B, n_mf, linear):
    """every sample within the derived bound, every prefix a bit copy of samples 128..159; a frame of zero latents gives data samples that are exactly 0
    (the limiter's mag == 0 branch)"""
    rng = np.random.default_rng(10 * B + n_mf)
    for z in (mod_latents(rng, B, n_mf), np.zeros((B, 3 * n_mf, 80), np.float32)):
        got = run_mod(L, torch_dev, dtab, z, linear)
        what = f"k_ofdm_mod linear={linear} B={B} n_mf={n_mf}" + ("" if z.any() else " zero latents")
        r = tx.check_mod(got, tx.mod_ref(tab, z, linear), what)
        print(f"{what}: largest error / bound {r:.3f}")
        zero = ~z.reshape(B, n_mf, 240).any(axis=2)
        data = got.reshape(B, n_mf, 5, 192)[:, :, 1:]
        assert not data[zero].view(np.float32).any(), what + ": a frame of zero latents has non-zero data samples"


def test_limiter_sweep(L, torch_dev, dtab, tab):
    """pa_limit over 2^16 magnitudes, log-spaced from 2^-20 to 2^5, each on carrier 7 of one data symbol (real part; every other latent 0): the IDFT chain is then
    ONE rounded product per component (acc = fma(a, w, 0); every other term adds 0 exactly), so the float32 argument of the limiter is known exactly and the
    error against float64 is the limiter's own.  This measures tx_ref.EPS_PA_LIMIT."""
    B, n_mf, c = 16, 1024, 7
    mags = np.exp2(-20 + 25 * np.arange(65536) / 65535.0)
    a = (mags * 160).astype(np.float32)
    z = np.zeros((B, n_mf, 4, 30, 2), np.float32); z[:, :, :, c, 0] = a.reshape(B, n_mf, 4)
    got = run_mod(L, torch_dev, dtab, z.reshape(B, 3 * n_mf, 80), 0).reshape(B, n_mf, 5, 192)[:, :, 1:, 32:]
    w32 = tab.Winv[c].astype(np.complex64)
    x32 = (a[:, None] * w32.real[None, :]).astype(np.float32) + 1j * (a[:, None] * w32.imag[None, :]).astype(np.float32)      # complex64: the products rounded as the kernel rounds them
    want = tx.limiter(x32.astype(np.complex128)).reshape(B, n_mf, 4, 160)
    err = np.abs(got - want)
    i = np.unravel_index(np.argmax(err), err.shape)
    at = abs(x32.reshape(B, n_mf, 4, 160)[i])
    print(f"MEASURED pa_limit: largest |error| {err.max():.4g} at |x| = {at!r} (EPS_PA_LIMIT {tx.EPS_PA_LIMIT:.4g}, ceiling 2^-20 = {2.0 ** -20:.4g})")
    assert tx.EPS_PA_LIMIT <= 2.0 ** -20
    assert err.max() <= tx.EPS_PA_LIMIT, f"pa_limit: |error| {err.max():.4g} at |x| = {at!r} exceeds {tx.EPS_PA_LIMIT:.4g}"


@pytest.mark.parametrize("linear", [0, 1])
@pytest.mark.parametrize("B,n_mf", [(1, 1), (3, 2), (3, 5)])
def test_ofdm_mod_mp(L, torch_dev, dtab, tab, B, n_mf, linear):
    """with tx given and tx = NULL: tx bit-equal to k_ofdm_mod's; mp against the two-path model of that tx (two products and a sum: the first 16 samples of a
    stream have no second path, samples 0..15 of a frame mf > 0 take it from tx[base - 16 ..], the tail the kernel re-synthesises); part within 4 u relative.
    G around 1 in magnitude; stream 1 has G2 = 0."""
    rng = np.random.default_rng(100 * B + n_mf)
    z = mod_latents(rng, B, n_mf)
    n = 960 * n_mf
    G = crand(rng, (B, n, 2))
    if B > 1:
        G[1, :, 1] = 0
    tx0 = run_mod(L, torch_dev, dtab, z, linear)
    first = None
    for with_tx in (1, 0):
        what = f"k_ofdm_mod_mp linear={linear} B={B} n_mf={n_mf} tx={'given' if with_tx else 'NULL'}"
        txo, mpo, pto = crows(B, n, n + 7), dense(2 * B * n), dense(2 * 2 * B * n_mf)
        d = Dev(torch_dev)
        z_d, g_d = d.put(z), d.put(G)
        t_d, m_d, p_d = d.put(txo.words, check=False), d.put(mpo.words, check=False), d.put(pto.words, check=False)
        assert (m_d.data_ptr() + 4 * mpo.base) % 8 == 0 and (p_d.data_ptr() + 4 * pto.base) % 8 == 0
        assert L.rd_launch_ofdm_mod_mp(dtab, z_d.data_ptr(), t_d.data_ptr() + 4 * txo.base if with_tx else None, n + 7, B, n_mf, g_d.data_ptr(),
                                       m_d.data_ptr() + 4 * mpo.base, p_d.data_ptr() + 4 * pto.base, linear, stream()) == 0
        sync()
        d.unchanged()
        tw, mw, pw = host32(t_d), host32(m_d), host32(p_d)
        for rows, words in ((txo, tw), (mpo, mw), (pto, pw)):
            rows.check_outside(words, what)
        if with_tx:
            tx.check_bits(cplx(txo, tw), tx0, what + " tx against k_ofdm_mod", ("stream", "component of sample"))
        else:
            assert np.all(tw == kr.SENT32), what + ": tx written"
        mp = cplx(mpo, mw).reshape(B, n)
        part = np.ascontiguousarray(pto.view(pw)[0, 0]).view(np.float64).reshape(B, n_mf, 2)
        r, r2 = tx.check_mp(mp, part, tx0, G, what)
        print(f"{what}: mp largest error / bound {r:.3f}, part {r2:.3f}")
        if first is None:
            first = (mp, part)
        else:
            tx.check_bits(mp, first[0], what + " mp against the run with tx", ("stream", "component of sample"))
            assert np.array_equal(part, first[1]), what + ": part differs from the run with tx"


def run_eoo(L, dev, dtab, bits, B):
    out = dense(2 * B * 1152)
    d = Dev(dev)
    o_d = d.put(out.words, check=False)
    b_d = d.put(bits) if bits is not None else None
    assert L.rd_launch_eoo_build(dtab, b_d.data_ptr() if bits is not None else None, o_d.data_ptr() + 4 * out.base, B, stream()) == 0
    sync()
    d.unchanged()
    words = host32(o_d)
    out.check_outside(words, "k_eoo_build")
    return cplx(out, words).reshape(B, 1152)


def test_eoo_build(L, torch_dev, dtab, tab):
    """bits = NULL: a bit copy of the table for every stream; with bits (+-1 for two streams, amplitudes up to 8 for the third): the table's symbols bit for bit,
    symbols 2..4 = limiter(pilot_gain (bits @ Winv)) within the bound, their prefixes bit copies"""
    B = 3
    got = run_eoo(L, torch_dev, dtab, None, B)
    tx.check_bits(got, np.broadcast_to(tab.eoo32, (B, 1152)), "k_eoo_build bits=NULL", ("stream", "component of sample"))
    rng = np.random.default_rng(3)
    bits = np.sign(rng.standard_normal((B, 180))).astype(np.float32); bits[2] *= rng.uniform(0, 8, 180).astype(np.float32)
    got = run_eoo(L, torch_dev, dtab, bits, B)
    r = tx.check_eoo(got, tx.eoo_ref(tab, bits), "k_eoo_build")
    print(f"k_eoo_build: largest error / bound {r:.3f}")


def test_copy_eoo(L, torch_dev):
    rng = np.random.default_rng(4)
    B = 3
    eoo = crand(rng, (B, 1152))
    out = crows(B, 1152, 1152 + 5)
    d = Dev(torch_dev)
    e_d, o_d = d.put(eoo), d.put(out.words, check=False)
    assert L.rd_launch_copy_eoo(e_d.data_ptr(), o_d.data_ptr() + 4 * out.base, 1152 + 5, B, stream()) == 0
    sync()
    d.unchanged()
    words = host32(o_d)
    out.check_outside(words, "k_copy_eoo")
    tx.check_bits(cplx(out, words), eoo, "k_copy_eoo", ("stream", "component of sample"))


# ================================================================================================================================================================
# D. channel
# ================================================================================================================================================================
CHAN_B = 3
N_SIG = (1, 16, 17, 63, 64, 65, 960, 1000, 1921)
PRE_POST = ((0, 0), (1, 0), (3, 2))
FREQ = ((0.0, 0.0), (-7.0, 0.0), (20.0, 0.5), (0.0, 0.5), (-7.0, -0.5), (20.0, 0.0))          # (0, 0.5): the case the reference leaves unrotated


def _chan_cases():
    """The named cases: in each mode -- with G, without, with mp and per-frame part sums as k_ofdm_mod_mp leaves them (n_sig then a multiple of 960) -- every
    n_sig, (n_pre, n_post), with_eoo, freq_offset, df_dt, scalars / per-stream ps, the sine with rx_gain 0.5, and an odd rx_stride appear at least once
    (test_channel_case_table_covers_every_value); the cycles below have different lengths, so the values meet in different combinations, not the cross product."""
    cases = {}
    for mode, sigs, k0 in (("G", N_SIG, 0), ("awgn", N_SIG, 1), ("mp", (960, 1920, 960, 1920, 960, 1920), 2)):
        for k, n_sig in enumerate(sigs):
            q = k + k0
            pre, post = PRE_POST[q % 3]; f0, dd = FREQ[q % 6]
            c = dict(mode=mode, n_sig=n_sig, n_pre=pre, n_post=post, with_eoo=(q // 2) % 2, f0=f0, df_dt=dd, ps=(q % 4) in (1, 2), sine=q % 5 in (0, 3), odd_stride=q % 3 != 1)
            name = f"{mode}-n{n_sig}-pre{pre}-post{post}" + ("-eoo" if c["with_eoo"] else "") + f"-f{f0:g}-d{dd:g}" + ("-ps" if c["ps"] else "") + ("-sine" if c["sine"] else "") + ("-odd" if c["odd_stride"] else "")
            assert name not in cases
            cases[name] = c
    return cases


CHAN_CASES = _chan_cases()


def test_channel_case_table_covers_every_value():
    for mode in ("G", "awgn", "mp"):
        cs = [c for c in CHAN_CASES.values() if c["mode"] == mode]
        assert {c["n_sig"] for c in cs} >= (set(N_SIG) if mode != "mp" else {960})
        assert {(c["n_pre"], c["n_post"]) for c in cs} == set(PRE_POST)
        assert {(n_tot(c) % 2) for c in cs} == {0, 1}
        for key, vals in (("with_eoo", {0, 1}), ("f0", {0.0, -7.0, 20.0}), ("df_dt", {0.0, 0.5, -0.5}), ("ps", {False, True}), ("sine", {False, True}), ("odd_stride", {False, True})):
            assert {c[key] for c in cs} == vals, (mode, key)
        assert any(c["f0"] == 0 and c["df_dt"] == 0.5 for c in cs)
    assert 20 <= len(CHAN_CASES) <= 28


def n_tot(c):
    return c["n_pre"] + c["n_sig"] + (1152 if c["with_eoo"] else 0) + c["n_post"]


@pytest.mark.parametrize("name", list(CHAN_CASES))
def test_channel(L, torch_dev, dtab, tab, name):
    """rd_launch_channel (k_chan_power unless mp is given, k_chan_gain, k_chan_apply) with an explicit noise tensor, B = 3: every sample of rx within the bound
    chan_ref carries through the kernel's steps; everything beyond n_total of each stream still the sentinel (an odd rx_stride puts stream 1 on the 8-byte store
    branch and streams 0, 2 on the 16-byte one); tx, G, mp, noise, eoo and ps unchanged"""
    c = CHAN_CASES[name]
    B, n_sig, n_pre, n_post = CHAN_B, c["n_sig"], c["n_pre"], c["n_post"]
    n_total = n_tot(c)
    rng = np.random.default_rng(sum(map(ord, name)))
    txs = crand(rng, (B, n_sig), 0.8)
    G = crand(rng, (B, n_sig, 2)) if c["mode"] != "awgn" else None
    noise = crand(rng, (B, n_total))
    noise[:, :n_pre] = noise[:, :n_pre].real; noise[:, n_total - n_post:] = noise[:, n_total - n_post:].real       # real-valued, as inference.py:277-284 draws them
    eoo = np.broadcast_to(tab.eoo32, (B, 1152)).copy(); eoo[1] = crand(rng, 1152, 0.7)
    ps = np.array([[0.5, 0.3, 0.7], [c["f0"], 3.0 - c["f0"] / 2, 0.0], [c["df_dt"], 0.5, 0.5]], np.float32) if c["ps"] else None
    sine_amp, sine_freq, rx_gain = (0.3, 1234.5, 0.5) if c["sine"] else (0.0, 0.0, 1.0)
    mp = part = None
    if c["mode"] == "mp":
        mp = tx.mp_ref(txs, G)[0].astype(np.complex64); part = tx.part_ref(txs, mp)
    stride = n_total + 3
    if (stride % 2 == 1) != c["odd_stride"]:
        stride += 1
    rxo, txi = crows(B, n_total, stride, off=0), crows(B, n_sig, n_sig + 3).fill(txs.view(np.float32).reshape(B, 1, 2 * n_sig))
    n_part = max(64, n_sig // 960)
    scratch = np.zeros(2 * B * (1 + n_part) + 8, np.float64)
    if part is not None:
        scratch[2 * B:2 * B + part.size] = part.ravel()
    d = Dev(torch_dev)
    t_d, n_d, e_d = d.put(txi.words), d.put(noise), d.put(eoo)
    g_d = d.put(G) if G is not None else None
    m_d = d.put(mp) if mp is not None else None
    p_d = d.put(ps) if ps is not None else None
    s_d, r_d = d.put(scratch, check=False), d.put(rxo.words, check=False)
    a = tx.ChanArgs()
    a.tab, a.tx, a.tx_stride, a.rx, a.rx_stride = dtab, t_d.data_ptr() + 4 * txi.base, n_sig + 3, r_d.data_ptr() + 4 * rxo.base, stride
    a.G, a.noise, a.eoo, a.scratch = (g_d.data_ptr() if G is not None else None), n_d.data_ptr(), e_d.data_ptr(), s_d.data_ptr()
    a.mp = m_d.data_ptr() if mp is not None else None
    a.B, a.n_sig, a.n_pre, a.n_post, a.with_eoo = B, n_sig, n_pre, n_post, c["with_eoo"]
    a.sigma, a.freq_offset, a.df_dt, a.seed = (0.0, 0.0, 0.0, 0) if c["ps"] else (0.6, c["f0"], c["df_dt"], 0)
    a.sine_amp, a.sine_freq, a.rx_gain = sine_amp, sine_freq, rx_gain
    a.ps = p_d.data_ptr() if ps is not None else None
    assert (a.rx % 16 == 0) and L.rd_launch_channel(C.byref(a), stream()) == 0
    sync()
    d.unchanged()
    words = host32(r_d)
    rxo.check_outside(words, name)
    ref = tx.chan_ref(txs, noise, n_pre, n_post, eoo=eoo if c["with_eoo"] else None, G=G, mp=mp, part=part, sigma=0.6, freq_offset=c["f0"], df_dt=c["df_dt"], ps=ps,
                      sine_amp=sine_amp, sine_freq=sine_freq, rx_gain=rx_gain)
    r = tx.check_chan(cplx(rxo, words), ref, f"rd_launch_channel {name}")
    print(f"rd_launch_channel {name}: largest error / bound {r:.3f}")


# ================================================================================================================================================================
# E. multipath generator
# ================================================================================================================================================================
MPGEN_CASES = [(1, 2), (4, 2), (4, 9), (7, 1000), (15, 15 * 2048), (15, 15 * 2048 + 1)]


def run_mpgen(L, dev, taps, ratio, n_out, noise, use_ybuf):
    import torch
    B = noise.shape[0]
    out = dense(4 * B * n_out)
    d = Dev(dev)
    t_d, n_d, o_d = d.put(taps), d.put(noise), d.put(out.words, check=False)
    y_d = torch.zeros(B * 2 * tx.n_low_of(ratio, n_out) * 2, dtype=torch.float64, device=dev) if use_ybuf else None
    r = L.rd_launch_multipath_gen(t_d.data_ptr(), len(taps), ratio, n_out, n_d.data_ptr(), 0, o_d.data_ptr() + 4 * out.base, y_d.data_ptr() if use_ybuf else None, B, stream())
    sync()
    d.unchanged()
    words = host32(o_d)
    out.check_outside(words, f"k_multipath_gen ratio={ratio} n_out={n_out}")
    return r, words, np.ascontiguousarray(out.view(words)[0, 0]).view(np.complex64).reshape(B, n_out, 2)


@pytest.mark.parametrize("n_taps", [5, 101])
@pytest.mark.parametrize("ratio,n_out", MPGEN_CASES)
def test_multipath_gen(L, torch_dev, ratio, n_out, n_taps):
    """explicit noise_low and the test's own taps.  (7, 1000) and the two long ones extrapolate past the last low-rate point; n_low = 2048 is the last size kept
    in LDS, 2049 needs ybuf: rd_multipath_gen_needs_scratch says so and the shim refuses without it, launching nothing.  Where both are legal the LDS and the
    ybuf path must agree bit for bit.  n_out = 1 is left out on purpose: the variance of one sample is 0 -- in the reference too -- and the gain infinite."""
    rng = np.random.default_rng(ratio + n_out + n_taps)
    B = 2
    n_low = tx.n_low_of(ratio, n_out)
    taps = (rng.standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)
    noise = crand(rng, (B, 2, n_low + n_taps), np.sqrt(2))
    ref = tx.mpgen_ref(noise, taps, ratio, n_out)
    needs = bool(L.rd_multipath_gen_needs_scratch(ratio, n_out))
    assert needs == (n_low > 2048)
    what = f"k_multipath_gen ratio={ratio} n_out={n_out} n_taps={n_taps}"
    r, words, got_lds = run_mpgen(L, torch_dev, taps, ratio, n_out, noise, False)
    if needs:
        assert r == -1 and np.all(words == kr.SENT32), what + ": launched without the scratch it needs"
    else:
        assert r == 0
        print(f"{what} LDS: largest error / bound {tx.check_mpgen(got_lds, ref, what + ' LDS'):.3f}")
    r, _, got = run_mpgen(L, torch_dev, taps, ratio, n_out, noise, True)
    assert r == 0
    print(f"{what} ybuf: largest error / bound {tx.check_mpgen(got, ref, what + ' ybuf'):.3f}")
    if not needs:
        tx.check_bits(got, got_lds, what + ": ybuf against LDS", ("stream", "sample", "component of path"))


@pytest.mark.parametrize("want_complex", [0, 1])
@pytest.mark.parametrize("Nc", [1, 3, 20])
@pytest.mark.parametrize("M", [1, 4, 160])
def test_multipath_h(L, torch_dev, M, Nc, want_complex):
    """H[t][c] = G1[t M] + G2[t M] exp(-2 pi j c d Rs) as a magnitude or complex; n_g = (n_sym - 1) M + 1 is the last legal length, one less is refused"""
    rng = np.random.default_rng(M + Nc)
    B, n_sym, dRs = 2, 7, 0.1
    n_g = (n_sym - 1) * M + 1
    G = crand(rng, (B, n_g, 2))
    w = (2 if want_complex else 1) * B * n_sym * Nc
    what = f"k_multipath_h M={M} Nc={Nc} complex={want_complex}"
    for n in (n_g, n_g - 1):
        out = dense(w)
        d = Dev(torch_dev)
        g_d, o_d = d.put(G), d.put(out.words, check=False)
        r = L.rd_launch_multipath_h(g_d.data_ptr(), n, M, n_sym, Nc, dRs, want_complex, o_d.data_ptr() + 4 * out.base, B, stream())
        sync()
        d.unchanged()
        words = host32(o_d)
        if n < n_g:
            assert r == -1 and np.all(words == kr.SENT32), what + ": n_g one short was not refused"
            continue
        assert r == 0
        out.check_outside(words, what)
        h = np.ascontiguousarray(out.view(words)[0, 0])
        got = h.view(np.complex64).reshape(B, n_sym, Nc) if want_complex else h.reshape(B, n_sym, Nc)
        print(f"{what}: largest error / bound {tx.check_mph(got, tx.mph_ref(G, M, n_sym, Nc, np.float32(dRs), want_complex), what):.3f}")
