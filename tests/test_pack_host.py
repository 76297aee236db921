"""The host's operand packers (radae_amd/csrc/rade_pack.c) against the numpy model of the layout (kernel_ref.frag_layout, split16), bit for bit; their refusals; the
two constant tables whose values need no libm; and the correlator tables from eight threads at once.  CPU only."""
import ctypes as C
import threading

import numpy as np
import pytest

import dev_abi
from dev_abi import Tables
from kernel_ref import FRAG_A16, FRAG_B16, FRAG_F32, SENT16, SENT32, frag_pack, split16

NS = (1, 15, 16, 17, 31, 32, 33, 84)
GUARD = 64                                   # sentinel words behind every output: a packer writes its size and no more


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return dev_abi.load()


@pytest.fixture(scope="module")
def tables(lib):
    T = Tables()
    lib.rd_tables_fill(C.byref(T))
    return T


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _weights(rng, N, K, grid):
    """(W, row scales): "int8" = q s_n on an exact grid (integer |q| <= 127, s_n a power of two), "float" = normal weights with the model's 1 / sqrt(K), as they are
    for the two-plane packers and quantised to their own row maximum / 127 (an int8 layer of a blob) for the one-plane packers"""
    if grid == "int8":
        sc = np.exp2(rng.integers(-9, -4, N)).astype(np.float32)
        return (rng.integers(-127, 128, (N, K)).astype(np.float32) * sc[:, None]).astype(np.float32), sc
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    sc = (np.abs(W).max(1) / 127).astype(np.float32)
    return W, sc


def _model_split(W, frag, scale=1024.0, order="k"):
    return frag_pack(np.stack(split16(W, scale)), **frag, order=order)


def _model_int8(W, sc, frag):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(W == 0, np.float32(0), np.rint(W / sc[:, None])).astype(np.float32)
    assert (np.abs(q) <= 127).all() and np.array_equal(q * sc[:, None], W), "the test's own weights are not int8-exact"
    scale_out = np.zeros(-(-len(sc) // frag["R"]) * frag["R"], np.float32); scale_out[:len(sc)] = sc
    return frag_pack(q.astype(np.float16).view(np.uint16)[None], **frag), scale_out


def _call(fn, size, dtype, W, sc=False, n_scales=0):
    """fn on W [N][K] into sentinel-filled buffers: (return value, the first `size` words, scale_out); everything behind them must keep the sentinel"""
    sent = SENT32 if dtype == np.float32 else SENT16
    out = np.full(size + GUARD, sent, np.uint32 if dtype == np.float32 else np.uint16)
    scales = np.full(n_scales + GUARD, SENT32, np.uint32)
    N, K = W.shape
    ret = fn(_p(W), N, K, _p(out)) if sc is False else fn(_p(W), _p(sc), N, K, _p(out), _p(scales))
    assert (out[size:] == sent).all() and (scales[n_scales:] == SENT32).all(), "written past the documented size"
    return ret, out[:size], scales[:n_scales].view(np.float32)


@pytest.mark.parametrize("grid", ["int8", "float"])
def test_float32_packer_is_the_model(lib, grid):
    rng = np.random.default_rng(1)
    for N, K in ((1, 8), (33, 88), (84, 88)):
        W, _ = _weights(rng, N, K, grid)
        size = lib.rd_packed_size(N, K)
        ret, out, _ = _call(lib.rd_pack_weights, size, np.float32, W)
        want = frag_pack(W.view(np.uint32)[None], **FRAG_F32)
        assert ret == size == want.size and np.array_equal(out, want), (N, K)


@pytest.mark.parametrize("grid", ["int8", "float"])
@pytest.mark.parametrize("name,frag,size_fn,Ks", [("rd_pack_weights_f16x2", FRAG_B16, "rd_packed16_size", (16, 32, 96)),
                                                  ("rd_pack_weights_f16x2_a16", FRAG_A16, "rd_packed16a_size", (32, 96))])
def test_two_plane_packers_are_the_model(lib, name, frag, size_fn, Ks, grid):
    rng = np.random.default_rng(2)
    for N in NS:
        for K in Ks:
            W, _ = _weights(rng, N, K, grid)
            size = getattr(lib, size_fn)(N, K)
            ret, out, _ = _call(getattr(lib, name), size, np.uint16, W)
            want = _model_split(W, frag)
            assert ret == size == want.size and np.array_equal(out, want), (N, K)


@pytest.mark.parametrize("grid", ["int8", "float"])
@pytest.mark.parametrize("name,frag,size_fn,Ks", [("rd_pack_weights_q16", FRAG_B16, "rd_packed16_size", (16, 32, 96)),
                                                  ("rd_pack_weights_q16_a16", FRAG_A16, "rd_packed16a_size", (32, 96))])
def test_one_plane_packers_are_the_model(lib, name, frag, size_fn, Ks, grid):
    """the integers of an int8-exact layer in ONE plane (half the two-plane size), scale_out = the row scales and zero past N"""
    rng = np.random.default_rng(3)
    for N in NS:
        for K in Ks:
            W, sc = _weights(rng, N, K, grid)
            if grid == "float":
                W = (np.rint(W / sc[:, None]).astype(np.float32) * sc[:, None]).astype(np.float32)
            size = getattr(lib, size_fn)(N, K) // 2
            want, want_sc = _model_int8(W, sc, frag)
            ret, out, scales = _call(getattr(lib, name), size, np.uint16, W, sc, want_sc.size)
            assert ret == size == want.size and np.array_equal(out, want), (N, K)
            assert np.array_equal(scales.view(np.uint32), want_sc.view(np.uint32)) and not scales[N:].any(), (N, K)


def test_padded_rows_are_zero(lib):
    """stated apart from the model: rows N .. of the last tile hold zeros in every plane (N = 17: 15 of the 32, 15 of the second 16)"""
    rng = np.random.default_rng(4)
    W, sc = _weights(rng, 17, 32, "int8")
    for name, frag, planes, sc_arg in (("rd_pack_weights_f16x2", FRAG_B16, 2, False), ("rd_pack_weights_f16x2_a16", FRAG_A16, 2, False),
                                       ("rd_pack_weights_q16", FRAG_B16, 1, sc), ("rd_pack_weights_q16_a16", FRAG_A16, 1, sc)):
        R, tiles = frag["R"], -(-17 // frag["R"])
        size = tiles * (32 * R // 64 // 8) * planes * 512
        _, out, _ = _call(getattr(lib, name), size, np.uint16, W, sc_arg, tiles * R if sc_arg is not False else 0)
        lanes = out.reshape(-1, planes, 64 // R, R, 8)                       # [block][plane][lane / R][lane % R][j]; block = k-step tiles + tile
        rows = (np.arange(lanes.shape[0]) % tiles)[:, None] * R + np.arange(R)[None, :]
        assert not lanes.transpose(0, 3, 1, 2, 4)[rows >= 17].any() and lanes.transpose(0, 3, 1, 2, 4)[rows < 17].any()


def test_packers_refuse(lib):
    """each of these returns below 0"""
    rng = np.random.default_rng(5)
    N, K = 33, 32
    W, sc = _weights(rng, N, K, "int8")
    out = np.zeros(lib.rd_packed16_size(N, K) + lib.rd_packed16a_size(N, K), np.uint16); scales = np.zeros(64, np.float32)
    two = [lib.rd_pack_weights_f16x2, lib.rd_pack_weights_f16x2_a16]
    one = [lib.rd_pack_weights_q16, lib.rd_pack_weights_q16_a16]

    def with_w(n, k, v):
        B = W.copy(); B[n, k] = v
        return B

    for fn in two:
        assert fn(_p(W), N, K, _p(out)) > 0
        assert fn(_p(with_w(32, 31, np.nan)), N, K, _p(out)) < 0                                   # a NaN weight
        for s in (1, -1):
            assert fn(_p(with_w(7, 9, np.float32(s * 65504.0 / 1024.0))), N, K, _p(out)) < 0       # 2^10 w = 65504: the high plane's limit itself
            assert fn(_p(with_w(7, 9, np.nextafter(np.float32(s * 65504.0 / 1024.0), np.float32(0)))), N, K, _p(out)) > 0
    for fn in one:
        assert fn(_p(W), _p(sc), N, K, _p(out), _p(scales)) > 0
        assert fn(_p(W), None, N, K, _p(out), _p(scales)) < 0                                      # no row scales: not an int8 layer
        z = sc.copy(); z[5] = 0
        assert np.any(W[5] != 0) and fn(_p(W), _p(z), N, K, _p(out), _p(scales)) < 0               # a zero scale under a non-zero weight
        Wz = W.copy(); Wz[5] = 0
        assert fn(_p(Wz), _p(z), N, K, _p(out), _p(scales)) > 0                                    # ... and under a zero row it is fine
        for s in (1, -1):
            assert fn(_p(with_w(32, 0, np.float32(s * 128) * sc[32])), _p(sc), N, K, _p(out), _p(scales)) < 0     # |q| = 128
            assert fn(_p(with_w(32, 0, np.float32(s * 127) * sc[32])), _p(sc), N, K, _p(out), _p(scales)) > 0
            assert fn(_p(with_w(0, 31, np.float32(s * 3.5) * sc[0])), _p(sc), N, K, _p(out), _p(scales)) < 0      # half a quantum off
        assert fn(_p(with_w(1, 1, np.nan)), _p(sc), N, K, _p(out), _p(scales)) < 0


def test_dft_and_bandpass_tables_are_the_model(lib, tables):
    """rd_wfwd16_table_fill and rd_bpf16_table_fill from rd_tables' float32 Wfwd and bpf_h: their scales are powers of two, so the model is exact"""
    Wf = np.ctypeslib.as_array(tables.Wfwd).reshape(160, 30, 2)
    R = np.zeros((30, 320), np.float32); R[:, 0::2] = Wf[:, :, 0].T; R[:, 1::2] = -Wf[:, :, 1].T     # R[c][2 n + comp] = (wr, -wi)
    out = np.full(2 * 10 * 2 * 512 + GUARD, SENT16, np.uint16)
    lib.rd_wfwd16_table_fill(C.byref(tables), _p(out))
    assert np.array_equal(out[:-GUARD], _model_split(R, FRAG_A16, 4096.0, "tile")) and (out[-GUARD:] == SENT16).all()
    h = np.ctypeslib.as_array(tables.bpf_h)[:101]
    Tm = np.zeros((16, 128), np.float32)
    for r in range(16):
        Tm[r, r:r + 101] = h                                                                          # T[r][m] = h[m - r]
    out = np.full(4 * 2 * 512 + GUARD, SENT16, np.uint16)
    lib.rd_bpf16_table_fill(C.byref(tables), _p(out))
    assert np.array_equal(out[:-GUARD], _model_split(Tm, FRAG_A16, 1024.0, "tile")) and (out[-GUARD:] == SENT16).all()


def test_correlator_tables_from_eight_threads(lib, tables):
    """Engines open on concurrent threads (rade_multi.c), and every open fills both correlator tables: each call works on a basis of its own, so eight threads that
    fill and check at once get the single thread's bytes and value every time."""
    def once():
        q16 = np.zeros(2 * 10 * 2 * 512, np.uint16); a16 = np.zeros(5 * 2 * 512, np.uint16)
        lib.rd_corrq16_table_fill(C.byref(tables), _p(q16)); lib.rd_corra16_table_fill(C.byref(tables), _p(a16))
        return q16.tobytes(), a16.tobytes(), lib.rd_corr_tables_check(C.byref(tables))

    want = once()
    bad = []

    def worker():
        for _ in range(20):
            if once() != want:
                bad.append(1)

    threads = [threading.Thread(target=worker) for _ in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, f"{len(bad)} of 160 concurrent fills differ from the single-thread tables"
