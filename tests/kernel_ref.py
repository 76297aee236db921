"""References, operand generators and layout codecs for the kernel unit tests (tests/test_kernel_units_gpu.py; their host-side halves are tested in
tests/test_host_cpu.py).  numpy only; holds no fixtures.

Two kinds of operands
---------------------
EXACT GRID.  a = m 2^-abits (integer |m| < 2^abits), w[n][k] = q s_n (integer |q| <= qmax, s_n a power of two per output column), bias_n an integer multiple of
the column's quantum 2^-abits s_n, and   sum_k |m_k||q_nk| + |bias_n| / quantum < 2^24   for every output element (exact_gemm_operands asserts it).  Every
product, every partial sum in ANY order and the biased result are then integer multiples of the quantum below 2^24 quanta: float32 accumulation is exact
whatever the order, the split of 2^8 a (and of 2^10 w) into hi + lo binary16 planes is exact, and a kernel's output must EQUAL the float64 reference cast to
float32 bit for bit.  Three grids:
    "int8"  abits 12, |q| <= 31 for K <= 128 and |q| <= 1 beyond (K up to 1728): the int8-exact layers (one weight plane + Wscale) and the float32 kernels;
            the activation's low plane is in use
    "w12"   two-plane layers, 12-bit weights w = n 2^-12 against 3-bit activations a = m 2^-3: the weights' low plane is in use
    "a12"   the other way round.  (Both at 12 bits is not exact by design: the kernels omit lo x lo.)

RANDOM.  a uniform in [-1, 1], w normal with the standard deviation 1 / sqrt(K) of the model's layers.  Every output element is held to the forward bound of
a length-K dot product that holds for every summation order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: gamma_K |a|.|w| with
gamma_K = K u / (1 - K u), u = 2^-24; doubled and padded here for the split-K second stage, the scale and the bias of the epilogue):
    |y - y64| <= ((2 K + 16) 2^-24 + r) sum_k |a_k w_k| + 2^-24 |y64|,
r = 0 for the float32 kernels and r = 3 2^-22 for the split-binary16 kernels (2^-22 for each operand's 22-bit hi + lo representation and 2^-22 for the
omitted lo x lo product, which is below 2^-11 2^-11 |a w|).  The bound is derived, not measured.  With an activation the epsilon of that activation below is
added (tanh and the sigmoid are 1-Lipschitz; the GLU multiplicand has magnitude <= 1).

The activation epsilons are the largest absolute errors MEASURED on an MI355X over the dense sweep of 2^16 arguments in [-12, 12]
(test_kernel_units_gpu.py::test_gemm_activation_sweep), each rounded up to the next power of two."""
import ctypes as C

import numpy as np

from dev_abi import EncfArgs, GemmArgs, ScanArgs  # noqa: F401  (the records of rade_dev.h, stated in tests/dev_abi.py)

U = 2.0 ** -24
R_F16 = 3 * 2.0 ** -22
# measured maxima (MI355X, against float64 tanh / 1 / (1 + exp(-x))), and the bound each test holds them to
EPS_TANH_HW = 2.0 ** -22       # gate_tanh (exp2 / rcp units), k_gemm16 / k_gemm16p / k_encf_gemm / k_gru_scan: measured 1.964e-07 (at x = -2.8766)
EPS_SIG_HW = 2.0 ** -23        # gate_sigmoid: measured 9.957e-08 (at x = 3.5900)
EPS_TANH_LIBM = 2.0 ** -23     # tanhf, k_gemm / k_gemm_splitk: measured 7.502e-08 (at x = -0.6449)
EPS_SIG_LIBM = 2.0 ** -23      # sigmoid_f = 1 / (1 + expf(-x)): measured 8.907e-08 (at x = 8.6689)

SENT32 = np.uint32(0xFFC0DEAD)     # a float32 NaN no kernel produces
SENT16 = np.uint16(0xFDAD)         # a binary16 NaN
EF_KB = 864 // 16
EF_TILE = EF_KB * 1024             # RD_EF_TILE of rade_dev.h


vp = C.c_void_p


def _p(a):
    return a.ctypes.data_as(vp)


def pack_f32(L, W):
    """rd_pack_weights of W [N][K] (K a multiple of 8)"""
    W = np.ascontiguousarray(W, np.float32); N, K = W.shape
    out = np.empty(L.rd_packed_size(N, K), np.float32)
    assert L.rd_pack_weights(_p(W), N, K, _p(out)) == out.size
    return out


def pack_f16x2(L, W):
    W = np.ascontiguousarray(W, np.float32); N, K = W.shape
    out = np.empty(L.rd_packed16_size(N, K), np.uint16)
    assert L.rd_pack_weights_f16x2(_p(W), N, K, _p(out)) == out.size
    return out


def pack_q16(L, W, scale):
    """rd_pack_weights_q16: (plane, scale_out), or None when the packer refuses the matrix"""
    W = np.ascontiguousarray(W, np.float32); N, K = W.shape
    ntt = (N + 31) // 32
    out = np.empty((K // 16) * ntt * 512, np.uint16); sc = np.empty(ntt * 32, np.float32)
    n = L.rd_pack_weights_q16(_p(W), _p(np.ascontiguousarray(scale, np.float32)), N, K, _p(out), _p(sc))
    if n < 0:
        return None
    assert n == out.size
    return out, sc


# ---- the matrix-core operand layouts of rade_pack.c (rade_pack.h: rd_frag), as numpy ---------------------------------------------------------------------------------
FRAG_F32 = dict(R=32, E=4)         # float32, k_gemm
FRAG_B16 = dict(R=32, E=8)         # B operand of v_mfma_f32_32x32x16_f16
FRAG_A16 = dict(R=16, E=8)         # A operand of v_mfma_f32_16x16x32_f16


def frag_layout(R, E, planes, order, tiles, steps):
    """Where element (plane, row, k) of an operand M lies: offsets [planes][R tiles][(64 E / R) steps].  THE LANE MAP: a lane holds E consecutive k of one row,
        row = R tile + lane % R,     k = (64 E / R) step + E (lane / R) + j,   j = 0 .. E - 1
    at ((block planes + plane) 64 + lane) E + j with block = step tiles + tile (order "k": k-step-major) or tile steps + step (order "tile")."""
    kstep = 64 * E // R
    row, k = np.arange(R * tiles)[:, None], np.arange(kstep * steps)[None, :]
    tile, step = row // R, k // kstep
    lane, j = row % R + R * (k % kstep // E), k % E
    block = step * tiles + tile if order == "k" else tile * steps + step
    assert order in ("k", "tile")
    return ((block * planes + np.arange(planes)[:, None, None]) * 64 + lane) * E + j


def frag_pack(vals, R, E, order="k"):
    """vals [planes][N][K] -> the operand words: rows padded to whole tiles and K to whole k-steps with zeros"""
    vals = np.asarray(vals); P, N, K = vals.shape
    idx = frag_layout(R, E, P, order, -(-N // R), -(-K // (64 * E // R)))
    out = np.zeros(idx.size, vals.dtype)
    out[idx[:, :N, :K]] = vals
    return out


def frag_unpack(words, R, E, planes, order, tiles, steps):
    """the operand words back as [planes][R tiles][(64 E / R) steps]"""
    return np.asarray(words)[frag_layout(R, E, planes, order, tiles, steps)]


def unpack16(plane_words, N, K, planes):
    """The packed B operands of k_gemm16 back to `planes` float32 matrices [32 ntt][K] of the binary16 values."""
    return frag_unpack(np.asarray(plane_words, np.uint16).view(np.float16).astype(np.float32), **FRAG_B16, planes=planes, order="k", tiles=(N + 31) // 32, steps=K // 16)


# ---- sentinel-filled strided buffers -----------------------------------------------------------------------------------------------------------------------------
class Rows:
    """float32 rows (b, t, 0..width) at element b sb + t st of a pointer that sits `off` elements into a row of a flat, sentinel-filled allocation; `lead`
    rows before t = 0 belong to every stream too (a conv history).  view() is the [B][lead + T][width] window, outside() the mask of every other word."""

    def __init__(self, B, T, width, st, sb, off=0, lead=0, guard=4096):
        assert st >= width + off and sb >= (T + lead) * st and guard % 4 == 0
        self.B, self.T, self.width, self.st, self.sb, self.lead = B, T, width, st, sb, lead
        self.base = guard + lead * st + off
        self.n = self.base + (B - 1) * sb + T * st + guard
        self.words = np.full(self.n, SENT32, np.uint32)

    def _win(self, arr):
        return np.lib.stride_tricks.as_strided(arr[self.base - self.lead * self.st:], (self.B, self.lead + self.T, self.width),
                                               (self.sb * arr.itemsize, self.st * arr.itemsize, arr.itemsize))

    def fill(self, values):
        self._win(self.words.view(np.float32))[...] = np.asarray(values, np.float32).reshape(self.B, self.lead + self.T, self.width)
        return self

    def view(self, words=None):
        return self._win((self.words if words is None else words).view(np.float32))

    def outside(self):
        m = np.ones(self.n, bool)
        self._win(m)[...] = False
        return m

    def check_outside(self, words, what):
        bad = np.flatnonzero(self.outside() & (words != SENT32))
        if bad.size:
            i = int(bad[0]) - self.base
            b = min(max(i // self.sb, 0), self.B - 1); r = i - b * self.sb
            raise AssertionError(f"{what}: {bad.size} words written outside the documented rows, the first at stream {b}, step {r // self.st}, column {r % self.st}")


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------------------------
GRIDS = {"int8": dict(abits=12, wbits=None), "w12": dict(abits=3, wbits=12), "a12": dict(abits=12, wbits=3)}


def exact_gemm_operands(rng, rows, K, N, grid="int8", f16_bits=24, conv=None):
    """(a [rows][K], W [N][K], scale [N], bias [N]) on an exact grid; asserts the grid's invariant sum_k |m||q| + |bias| < 2^f16_bits quanta for every element.
    conv = (B, T, dil, lead): a is X [B][lead + T][K / 2] instead and row (b, t) of the product is [X[b][lead + t - dil] | X[b][lead + t]] (two conv taps).
    f16_bits < 24 narrows the activations until the sums stay below 2^f16_bits (the instruction-width question of tests/test_kernel_units_gpu.py)."""
    g = GRIDS[grid]
    abits = g["abits"]
    if g["wbits"] is None:
        qmax = 31 if K <= 128 else 1
        scale = np.exp2(rng.integers(-8, -5, N)).astype(np.float32)                # a power of two per column
    else:
        qmax = 2 ** g["wbits"] - 1
        scale = np.full(N, 2.0 ** -g["wbits"], np.float32)
    lim = 2 ** f16_bits
    while abits > 1 and K * (2 ** abits - 1) * qmax + 1 >= lim:
        assert f16_bits < 24, f"K = {K} does not fit grid {grid}"
        abits -= 1
    mmax = 2 ** abits - 1
    q = rng.integers(-qmax, qmax + 1, (N, K)).astype(np.float32)
    if conv is None:
        m = rng.integers(-mmax, mmax + 1, (rows, K)).astype(np.float32)
        full = m
    else:
        B, T, dil, lead = conv
        m = rng.integers(-mmax, mmax + 1, (B, lead + T, K // 2)).astype(np.float32)
        full = conv_rows(m, T, dil, lead)
    bmax = min(2 ** 20, lim - 1 - K * mmax * qmax)
    bq = rng.integers(-bmax, bmax + 1, N).astype(np.float64)
    total = np.abs(full).astype(np.float64) @ np.abs(q).astype(np.float64).T + np.abs(bq)     # exact in float64
    assert total.max() < lim, "exact grid: a partial sum can leave the 24-bit range"
    a = m * np.float32(2.0 ** -abits)
    W = q * scale[:, None]
    bias = (bq * 2.0 ** -abits * scale.astype(np.float64)).astype(np.float32)
    assert np.array_equal(bias.astype(np.float64), bq * 2.0 ** -abits * scale)
    return a, W.astype(np.float32), scale, bias


def conv_rows(X, T, dil, lead):
    """X [B][lead + T][Kc] -> the product's rows [B T][2 Kc] = [tap 0 = the row dil steps earlier | tap 1 = the row itself]"""
    B, _, Kc = X.shape
    return np.concatenate([X[:, lead - dil:lead - dil + T], X[:, lead:lead + T]], axis=2).reshape(B * T, 2 * Kc)


def random_gemm_operands(rng, rows, K, N, int8=False):
    """a uniform in [-1, 1], W normal with the model's 1 / sqrt(K); int8: W = q scale with |q| <= 127 (an int8-exact layer), scale = row maximum / 127"""
    a = rng.uniform(-1, 1, (rows, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    scale = None
    if int8:
        scale = (np.abs(W).max(1) / 127).astype(np.float32)
        W = (np.rint(W / scale[:, None]).astype(np.float32) * scale[:, None]).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    return a, W, scale, bias


def gemm_ref(a, W, bias):
    """float64 y = a W^T + bias and S = |a| |W|^T (the condition sum of the forward bound)"""
    a64, W64 = a.astype(np.float64), W.astype(np.float64)
    return a64 @ W64.T + (0 if bias is None else bias.astype(np.float64)), np.abs(a64) @ np.abs(W64).T


def gemm_bound(K, S, y64, r):
    return ((2 * K + 16) * U + r) * S + U * np.abs(y64)


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    return np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))


def sweep_args():
    """2^16 arguments over [-12, 12): (i - 2^15) 3 2^-13, 17 significant bits (exactly hi + lo after the kernels' 2^8), values beyond the clamp included"""
    return ((np.arange(65536) - 32768) * 3).astype(np.float32) * np.float32(2.0 ** -13)


# ---- GRU ---------------------------------------------------------------------------------------------------------------------------------------------------------
def gru_step64(gi, Whh, bhh, h, eps_sig=0.0, eps_tanh=0.0):
    """One float64 GRU step in torch's gate order (r, z, n), gi = W_ih x + b_ih [.., 3H], h [.., H]; returns (h', bound), bound being the first-order bound on
    |kernel - h'| of a float32 evaluation of this step FROM THE SAME h:
        s_g = W_g h over K = H terms in any order:   d s_g <= (2 H + 16) u S_g,   S_g = |W_g| |h|                                          (the dot-product bound)
        p_g = (s_g + b_g) + gi_g, g = r, z:          d p_g <= d s_g + 2 u (|s_g| + |b_g| + |gi_g|)                                      (two rounded additions)
        r = sigmoid(p_r), z likewise:                d r  <= d p_r / 4 + eps_sig                                              (|sigmoid'| <= 1 / 4, measured epsilon)
        p_n = gi_n + (s_n + b_n) r:                  d p_n <= (d s_n + u |s_n + b_n|) |r| + |s_n + b_n| d r + u |(s_n + b_n) r| + u |p_n|
        n = tanh(p_n):                               d n  <= d p_n + eps_tanh                                                                     (|tanh'| <= 1)
        h' = (h - n) z + n:                          d h' <= (1 - z) d n + |h - n| d z + u (2 |h - n| |z| + |h'|) + u |h'|       (three rounded operations, the store)
    u = 2^-24.  Terms of second order in u are dropped; the factor 2 in (2 H + 16) and the unit Lipschitz constant of tanh leave room for them."""
    gi, Whh, bhh, h = (np.asarray(v, np.float64) for v in (gi, Whh, bhh, h))
    H = h.shape[-1]
    s = h @ Whh.T
    S = np.abs(h) @ np.abs(Whh).T
    ds = (2 * H + 16) * U * S
    sl = [slice(g * H, (g + 1) * H) for g in range(3)]
    p = [(s[..., sl[g]] + bhh[sl[g]]) + gi[..., sl[g]] for g in range(2)]
    dp = [ds[..., sl[g]] + 2 * U * (np.abs(s[..., sl[g]]) + np.abs(bhh[sl[g]]) + np.abs(gi[..., sl[g]])) for g in range(2)]
    r, z = sigmoid64(p[0]), sigmoid64(p[1])
    dr, dz = dp[0] / 4 + eps_sig, dp[1] / 4 + eps_sig
    sb = s[..., sl[2]] + bhh[sl[2]]
    pn = gi[..., sl[2]] + sb * r
    dpn = (ds[..., sl[2]] + U * np.abs(sb)) * np.abs(r) + np.abs(sb) * dr + U * np.abs(sb * r) + U * np.abs(pn)
    n = np.tanh(pn)
    dn = dpn + eps_tanh
    h1 = (h - n) * z + n
    bound = (1 - z) * dn + np.abs(h - n) * dz + U * (2 * np.abs(h - n) * np.abs(z) + np.abs(h1)) + U * np.abs(h1)
    return h1, bound


# ---- the operand-fragment layout of rade_enc.hip ----------------------------------------------------------------------------------------------------------------
def split16(x, scale=256.0):
    """float32 x -> the two binary16 planes of scale x = hi + lo (scale a power of two: 2^8 for the kernels' activations, 2^10 for the host's weights, 2^12 for its
    correlator and DFT tables), as the kernels and rade_pack.c form them (round to nearest even twice); returned as uint16 words"""
    x = np.float32(scale) * np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def join16(hi, lo, scale=256.0):
    """the float32 value (hi + lo) / scale of two planes (exact: 22 bits)"""
    return (np.asarray(hi, np.uint16).view(np.float16).astype(np.float32) + np.asarray(lo, np.uint16).view(np.float16).astype(np.float32)) * np.float32(1.0 / scale)


def frag_new(B, NQ):
    return np.full((B, NQ, EF_TILE), SENT16, np.uint16)


def frag_index(steps, col0, ncols):
    """half-word offsets [len(steps)][ncols] of the HIGH plane inside a stream's [NQ][EF_TILE] (low plane: + 512): step t >= 0 in tile 1 + t / 32, row t % 32;
    t = -2, -1 in rows 30, 31 of tile 0; [tile][col / 16][plane][(col % 16) / 8][row][col % 8]"""
    t = np.asarray(steps)[:, None]; c = (col0 + np.arange(ncols))[None, :]
    tile = np.where(t >= 0, 1 + t // 32, 0); row = np.where(t >= 0, t % 32, 32 + t)
    return tile * EF_TILE + (c >> 4) * 1024 + ((c >> 3) & 1) * 256 + row * 8 + (c & 7)


def frag_put(buf, steps, col0, x):
    """x [B][len(steps)][ncols] float32 into the fragment buffer [B][NQ][EF_TILE]"""
    B = buf.shape[0]; idx = frag_index(steps, col0, x.shape[-1])
    hi, lo = split16(x)
    flat = buf.reshape(B, -1)
    flat[:, idx] = hi; flat[:, idx + 512] = lo
    return idx


def frag_get(buf, steps, col0, ncols):
    """(hi, lo) words [B][len(steps)][ncols]"""
    idx = frag_index(steps, col0, ncols); flat = buf.reshape(buf.shape[0], -1)
    return flat[:, idx], flat[:, idx + 512]


def frag_untouched_except(buf, before, idx_list, what):
    """every half-word outside the given high-plane offsets (and their low-plane partners) still equals `before`"""
    flat, ref = buf.reshape(buf.shape[0], -1), before.reshape(before.shape[0], -1)
    m = np.ones(flat.shape[1], bool)
    for idx in idx_list:
        m[idx.ravel()] = False; m[idx.ravel() + 512] = False
    bad = np.argwhere((flat != ref) & m[None, :])
    if bad.size:
        b, o = bad[0]
        raise AssertionError(f"{what}: {len(bad)} half-words written outside the documented positions, the first in stream {b} at tile {o // EF_TILE}, offset {o % EF_TILE}")


# ---- reports and checks shared by the kernel unit tests -------------------------------------------------------------------------------------------------------------
def first_bad(bad, what, got, want, extra=""):
    b, t, n = np.argwhere(bad)[0]
    return f"{what}: {int(bad.sum())} elements differ, the first at stream {b}, step {t}, column {n}: got {got[b, t, n]!r}, reference {want[b, t, n]!r}{extra}"


def encf_check_exact(got, planes, want, what):
    if planes is None:
        bad = got.view(np.int32) != want.view(np.int32)
    else:
        whi, wlo = split16(want)
        bad = (planes[0] != whi) | (planes[1] != wlo)
    assert not bad.any(), first_bad(bad, what, got, want)
