"""GPU unit tests (-m gpu) of the feed-forward and recurrent kernels, each called alone through its launch shim of radae_amd/csrc/rade_dev.h on synthetic
operands: the GEMM family behind rd_launch_gemm (k_gemm, k_gemm16, k_gemm16p, k_gemm_splitk), k_gru_scan<64|96> behind rd_launch_gru_scan, and k_encf_gemm /
k_encf_hist behind rd_launch_encf_gemm / rd_launch_encf_hist.  Torch tensors are the device memory; references, generators and layout codecs are
tests/kernel_ref.py (its docstring states the two kinds of operands and derives the bound of the random ones).

EXACT-GRID cases require bit equality with the float64 reference, so a dropped plane product, a k-block read twice or skipped, a tile tail off by one or a
register set consumed in the wrong block shows as "this kernel, this shape, this element".  RANDOM cases hold every element to the derived forward bound.
Every output sits in a buffer pre-filled with a NaN sentinel: everything outside the documented rows (the columns N.. of a ragged tile, rows past B T, the
gaps of the strides) must still be the sentinel afterwards, and the inputs must be unchanged.

GEMM_CASES / ENCF_CASES name the kernel instantiation the dispatcher picks for each case; test_every_dispatcher_branch_is_covered checks the tables against a
copy of the dispatch rule and that every instantiation has an exact-grid and a random case.

The 24-bit question.  The exact grids assume that v_mfma_f32_32x32x16_f16 and v_mfma_f32_32x32x2_f32 keep 24 bits across the addends of one instruction.
Measured on the MI355X: it holds for both.  Every exact case -- sums up to 2^24 - 1 quanta over K = 864 and over two taps of 160, on every binary16 kernel and every
float32 kernel -- is bit-equal to float64, so F16_EXACT_BITS below stays 24 and no grid was narrowed.

Left out on purpose: the `reset` and `n_rows` members of rd_gemm_args / rd_scan_args.  Since the single-stream layer-wise and by-step launch paths were
retired no caller passes them (decoder_layers gets NULL, NULL); every case here passes NULL."""
import ctypes as C

import numpy as np
import pytest

import dev_abi
import kernel_ref as kr
from gpu_kit import Dev, host32, stream, sync, torch_dev  # noqa: F401
from kernel_ref import encf_check_exact, first_bad

pytestmark = pytest.mark.gpu

F16_EXACT_BITS = 24        # width of the exact grids on the binary16 matrix instruction (24: the full float32 significand holds)
NAN = float("nan")


@pytest.fixture(scope="module")
def L(torch_dev):
    return dev_abi.load()


# ================================================================================================================================================================
# rd_launch_gemm
# ================================================================================================================================================================
def gemm_kernel(rows, K0, K1, N, wmode):
    """the dispatch rule of rd_launch_gemm (rade_kernels.hip), copied: which instantiation a case reaches"""
    ntt = (N + 31) // 32
    nt = 3 if ntt % 3 == 0 else 2 if ntt % 2 == 0 else 1
    if rows <= 16384:
        return f"k_gemm_splitk<{nt}>"
    if wmode != "f32" and K0 % 16 == 0 and K1 % 16 == 0:
        if ((K0 + K1) // 16) % 2 == 0 and (K0 // 16) % 2 == 0 and ntt % 3 == 0:
            return "k_gemm16p<3,1,true>" if wmode == "q16" else "k_gemm16p<3,2,false>"
        return f"k_gemm16<{nt},2>"
    return f"k_gemm<{nt}>"


BIG_ROWS = [(5, 3277), (7, 2347), (5477, 3)]          # 16385: one valid row in the last tile; 16429, prime T: every tile spans two streams; 16431: a tile spans eleven
SMALL_ROWS = [(1, 1), (1, 31), (1, 32), (1, 33), (3, 5)]
# name -> (K0, K1, N, wmode, [(B, T)], expected kernel).  wmode: f32 = Wp only; q16 = one plane + Wscale; f16x2 = two planes.
GEMM_CASES = {}
for _N, _nt in ((32, 1), (64, 2), (80, 3), (84, 3), (96, 3), (160, 1), (192, 3)):
    for _K1 in (8, 80, 96, 864):
        GEMM_CASES[f"small-N{_N}-K{_K1}"] = (0, _K1, _N, "f32", SMALL_ROWS, f"k_gemm_splitk<{_nt}>")
    GEMM_CASES[f"small-N{_N}-conv160"] = (160, 160, _N, "f32", SMALL_ROWS, f"k_gemm_splitk<{_nt}>")
GEMM_CASES.update({
    "big-f32-N32": (0, 80, 32, "f32", BIG_ROWS, "k_gemm<1>"),
    "big-f32-N64": (0, 80, 64, "f32", BIG_ROWS, "k_gemm<2>"),
    "big-f32-N80": (0, 80, 80, "f32", BIG_ROWS, "k_gemm<3>"),
    "big-f32-conv160-N96": (160, 160, 96, "f32", BIG_ROWS[1:2], "k_gemm<3>"),
    "big-2p-K80-N64": (0, 80, 64, "f16x2", BIG_ROWS, "k_gemm16<2,2>"),
    "big-2p-K80-N32": (0, 80, 32, "f16x2", BIG_ROWS, "k_gemm16<1,2>"),
    "big-1p-K80-N96": (0, 80, 96, "q16", BIG_ROWS, "k_gemm16<3,2>"),
    "big-2p-K96-N96": (0, 96, 96, "f16x2", BIG_ROWS, "k_gemm16p<3,2,false>"),
    "big-1p-K864-N80": (0, 864, 80, "q16", BIG_ROWS, "k_gemm16p<3,1,true>"),
    "big-1p-conv160-N96": (160, 160, 96, "q16", BIG_ROWS, "k_gemm16p<3,1,true>"),
})
ALL_GEMM_KERNELS = {"k_gemm_splitk<1>", "k_gemm_splitk<2>", "k_gemm_splitk<3>", "k_gemm<1>", "k_gemm<2>", "k_gemm<3>", "k_gemm16<1,2>", "k_gemm16<2,2>",
                    "k_gemm16<3,2>", "k_gemm16p<3,2,false>", "k_gemm16p<3,1,true>"}


def run_gemm(L, dev, B, T, K0, K1, N, wmode, X, W, scale, bias, act=0):
    """X [B][lead + T][K1] (lead = 1 with a conv tap: a0 is a1 one row earlier).  Returns the y rows [B][T][N] after the sentinel and input checks."""
    lead = 1 if K0 else 0
    st = K1 + 12; sb = (T + lead) * st + 2 * st                       # a1_sb > T a1_st; the pointer 4 floats into a wider row
    xa = kr.Rows(B, T, K1, st, sb, off=4, lead=lead).fill(X)
    yst = N + 37; ysb = T * yst + 53              # y into a wider row at a column offset, odd strides (scalar stores: natural alignment)
    ya = kr.Rows(B, T, N, yst, ysb, off=5)
    d = Dev(dev)
    x_d = d.put(xa.words); y_d = d.put(ya.words, check=False)
    wp_d = d.put(kr.pack_f32(L, W)); b_d = d.put(bias)
    a = kr.GemmArgs()
    a.a1 = x_d.data_ptr() + 4 * xa.base; a.a1_sb, a.a1_st, a.K1 = sb, st, K1
    if K0:
        a.a0 = a.a1 - 4 * st; a.a0_sb, a.a0_st, a.K0 = sb, st, K0
    a.Wp, a.bias = wp_d.data_ptr(), b_d.data_ptr()
    if wmode == "q16":
        plane, sc = kr.pack_q16(L, W, scale)
        p_d, s_d = d.put(plane), d.put(sc); a.Wp16, a.Wscale = p_d.data_ptr(), s_d.data_ptr()
    elif wmode == "f16x2":
        p_d = d.put(kr.pack_f16x2(L, W)); a.Wp16 = p_d.data_ptr()
    a.y = y_d.data_ptr() + 4 * ya.base; a.y_sb, a.y_st, a.N = ysb, yst, N
    a.B, a.T, a.act = B, T, act
    assert L.rd_launch_gemm(C.byref(a), stream()) == 0
    sync()
    what = f"{gemm_kernel(B * T, K0, K1, N, wmode)} B={B} T={T} K0={K0} K1={K1} N={N} act={act}"
    yw = host32(y_d)
    ya.check_outside(yw, what)
    d.unchanged()
    return ya.view(yw).copy(), what


def gemm_exact(L, dev, rng, B, T, K0, K1, N, wmode, grid):
    K = K0 + K1
    bits = 24 if wmode == "f32" or B * T <= 16384 else F16_EXACT_BITS
    X, W, scale, bias = kr.exact_gemm_operands(rng, B * T, K, N, grid, bits, conv=(B, T, 1, 1) if K0 else None)
    A = kr.conv_rows(X, T, 1, 1) if K0 else X
    y64, _ = kr.gemm_ref(A, W, bias)
    want = y64.astype(np.float32).reshape(B, T, N)
    assert np.array_equal(want.astype(np.float64).ravel(), y64.ravel())
    got, what = run_gemm(L, dev, B, T, K0, K1, N, wmode, X, W, scale, bias)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), first_bad(bad, what + f" exact grid {grid}", got, want)


def gemm_random(L, dev, rng, B, T, K0, K1, N, wmode, act=0):
    K = K0 + K1
    f16 = wmode != "f32" and B * T > 16384
    lead = 1 if K0 else 0
    _, W, scale, bias = kr.random_gemm_operands(rng, 1, K, N, int8=wmode == "q16")
    X = rng.uniform(-1, 1, (B, T + lead, K1)).astype(np.float32)
    A = kr.conv_rows(X, T, 1, 1) if K0 else X.reshape(B * T, K1)
    y64, S = kr.gemm_ref(A, W, bias)
    bound = kr.gemm_bound(K, S, y64, kr.R_F16 if f16 else 0.0)
    if act == 1:
        y64 = np.tanh(y64); bound = bound + (kr.EPS_TANH_HW if f16 else kr.EPS_TANH_LIBM)
    elif act == 2:                                                     # GLU: a1[r][n] sigmoid(.), |a1| <= 1; one more rounded product
        y64 = A[:, K0:K0 + N] * kr.sigmoid64(y64); bound = bound + (kr.EPS_SIG_HW if f16 else kr.EPS_SIG_LIBM) + kr.U * np.abs(y64)
    got, what = run_gemm(L, dev, B, T, K0, K1, N, wmode, X, W, scale, bias, act)
    err = np.abs(got.astype(np.float64) - y64.reshape(B, T, N))
    print(f"{what}: largest error / bound {np.nanmax(err / bound.reshape(B, T, N)):.3f}")
    bad = ~(err <= bound.reshape(B, T, N))
    assert not bad.any(), first_bad(bad, what + " random", got, y64.reshape(B, T, N), f" bound {bound.reshape(B, T, N)[tuple(np.argwhere(bad)[0])]:.3g}")


def test_every_dispatcher_branch_is_covered():
    """the case tables against the dispatch rules: every case reaches the kernel it names, every instantiation has cases (each case runs exact AND random)"""
    seen = set()
    for name, (K0, K1, N, wmode, rows, kernel) in GEMM_CASES.items():
        for B, T in rows:
            assert gemm_kernel(B * T, K0, K1, N, wmode) == kernel, name
        seen.add(kernel)
    assert seen == ALL_GEMM_KERNELS
    assert {encf_kernel(*c[:5], c[6], c[7]) for c in ENCF_CASES.values()} == ALL_ENCF_KERNELS
    for name, c in ENCF_CASES.items():
        assert encf_kernel(*c[:5], c[6], c[7]) == c[8], name


@pytest.mark.parametrize("N", [32, 64, 80, 84, 96, 160, 192])
def test_gemm_splitk(L, torch_dev, N):
    """k_gemm_splitk<1|2|3>: K1 = 8 (fewer k-blocks than wavefronts), 80, 96, 864 and the two-tap conv shape, rows 1, 31, 32, 33 and 3 x 5; exact and random"""
    rng = np.random.default_rng(N)
    for name, (K0, K1, N_, wmode, rows, _) in GEMM_CASES.items():
        if name.startswith(f"small-N{N}-"):
            for B, T in rows:
                gemm_exact(L, torch_dev, rng, B, T, K0, K1, N, wmode, "int8")
                gemm_random(L, torch_dev, rng, B, T, K0, K1, N, wmode)
    gemm_random(L, torch_dev, rng, 3, 5, 0, 96, N if N <= 96 else 96, "f32", act=1)
    gemm_random(L, torch_dev, rng, 1, 33, 0, 192 if N > 96 else 96, N if N <= 96 else 96, "f32", act=2)


@pytest.mark.parametrize("name,rows", [(n, r) for n in GEMM_CASES if n.startswith("big-") for r in GEMM_CASES[n][4]], ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_gemm_many_rows(L, torch_dev, name, rows):
    """more than 16384 rows: k_gemm<1|2|3> (no binary16 copy), k_gemm16<NT,2> (an odd number of k-blocks), k_gemm16p (k-blocks in pairs)"""
    K0, K1, N, wmode, _, _ = GEMM_CASES[name]
    B, T = rows
    rng = np.random.default_rng(B + K1 + N)
    for grid in (("int8",) if wmode != "f16x2" else ("w12", "a12")):
        gemm_exact(L, torch_dev, rng, B, T, K0, K1, N, wmode, grid)
    gemm_random(L, torch_dev, rng, B, T, K0, K1, N, wmode)
    if rows == BIG_ROWS[1]:                                            # the epilogues with an activation, once per kernel
        gemm_random(L, torch_dev, rng, B, T, K0, K1, N, wmode, act=1)
        if K1 >= N:
            gemm_random(L, torch_dev, rng, B, T, K0, K1, N, wmode, act=2)


SWEEP = [("k_gemm_splitk<1>", 2048, 32, "f32", "LIBM"), ("k_gemm<1>", 16385, 32, "f32", "LIBM"),
         ("k_gemm16<1,2>", 16385, 32, "f16x2", "HW"), ("k_gemm16p<3,2,false>", 16385, 96, "f16x2", "HW"), ("k_gemm16p<3,1,true>", 16385, 96, "q16", "HW")]


@pytest.mark.parametrize("kernel,rows,N,wmode,unit", SWEEP, ids=[s[0] for s in SWEEP])
def test_gemm_activation_sweep(L, torch_dev, kernel, rows, N, wmode, unit):
    """The epilogues act = 1 (tanh + clamp) and act = 2 (GLU) over a dense sweep: a selector weight matrix makes the pre-activation an exact copy of an input
    (act 2: W[n][N + n] = 1, K1 = 2 N, the multiplicand columns 1), 2^16 arguments over [-12, 12) go through gate_tanh / gate_sigmoid (the binary16 kernels)
    and tanhf / sigmoid_f (the float32 kernels).  The bound is the maximum measured on the MI355X rounded up to a power of two (kernel_ref.EPS_*)."""
    x = kr.sweep_args()
    args = np.resize(x, rows * N).reshape(1, rows, N)
    for act, K1, ref in ((1, N, np.tanh), (2, 2 * N, kr.sigmoid64)):
        assert gemm_kernel(rows, 0, K1, N, wmode) == kernel
        W = np.zeros((N, K1), np.float32); W[np.arange(N), K1 - N + np.arange(N)] = 1
        X = np.ones((1, rows, K1), np.float32); X[:, :, K1 - N:] = args
        got, what = run_gemm(L, torch_dev, 1, rows, 0, K1, N, wmode, X, W, np.ones(N, np.float32), np.zeros(N, np.float32), act)
        err = np.abs(got.astype(np.float64) - ref(args.astype(np.float64)))
        eps = getattr(kr, f"EPS_{'TANH' if act == 1 else 'SIG'}_{unit}")
        i = np.unravel_index(np.argmax(err), err.shape)
        print(f"MEASURED {what}: largest |error| {err.max():.4g} at x = {args[i]!r} (bound {eps:.4g})")
        assert np.all(np.abs(got) <= 1) and err.max() <= eps, f"{what}: |error| {err.max():.4g} at x = {args[i]!r} exceeds {eps:.4g}"


# ================================================================================================================================================================
# rd_launch_gru_scan
# ================================================================================================================================================================
SCAN_B = 3


class Scan:
    """operands of one scan on the device: gi rows at strides larger than the rows, out at column offset 64 of 864-wide rows"""

    def __init__(self, L, dev, H, T, seed=0):
        rng = np.random.default_rng(1000 * H + T + seed)
        self.L, self.dev, self.H, self.T = L, dev, H, T
        B = SCAN_B
        self.gi = rng.standard_normal((B, T, 3 * H)).astype(np.float32)
        self.Whh = (rng.standard_normal((3 * H, H)) / np.sqrt(H)).astype(np.float32)       # gates stay away from saturation
        self.bhh = rng.uniform(-0.3, 0.3, 3 * H).astype(np.float32)
        self.h0 = rng.uniform(-0.99, 0.99, (B, H)).astype(np.float32)
        st = 3 * H + 20
        self.gi_rows = kr.Rows(B, T, 3 * H, st, T * st + 3 * st, off=4).fill(self.gi)
        self.d = Dev(dev)
        self.gi_d, self.W_d, self.b_d = self.d.put(self.gi_rows.words), self.d.put(self.Whh), self.d.put(self.bhh)

    def run(self, cuts=None, outf_col=None, NQ=0):
        """one launch per entry of cuts (default: one launch of T steps), the state carried in a.h; returns (out rows or fragment buffer, final h)"""
        B, H, T = SCAN_B, self.H, self.T
        d = Dev(self.dev)
        out = kr.Rows(B, T, H, 864, T * 864 + 2 * 864, off=64)
        h_d = d.put(self.h0, check=False)
        if outf_col is None:
            o_d = d.put(out.words, check=False)
        else:
            o_d = d.put(kr.frag_new(B, NQ), check=False)
        t0 = 0
        for n in cuts or [T]:
            a = kr.ScanArgs()
            a.gi = self.gi_d.data_ptr() + 4 * (self.gi_rows.base + t0 * self.gi_rows.st); a.gi_sb, a.gi_st = self.gi_rows.sb, self.gi_rows.st
            a.Whh, a.bhh, a.h = self.W_d.data_ptr(), self.b_d.data_ptr(), h_d.data_ptr()
            a.B, a.T, a.H = B, n, H
            if outf_col is None:
                a.out = o_d.data_ptr() + 4 * (out.base + t0 * out.st); a.out_sb, a.out_st = out.sb, out.st
            else:
                assert t0 == 0
                a.outf, a.outf_NQ, a.outf_col = o_d.data_ptr(), NQ, outf_col
            assert self.L.rd_launch_gru_scan(C.byref(a), stream()) == 0
            t0 += n
        assert t0 == T
        sync()
        self.d.unchanged()
        h = h_d.cpu().numpy().view(np.float32).reshape(B, H)
        if outf_col is not None:
            return o_d.cpu().numpy().view(np.uint16).reshape(B, NQ, kr.EF_TILE), h
        ow = host32(o_d)
        out.check_outside(ow, f"k_gru_scan<{H}> T={T} cuts={cuts}")
        return out.view(ow).copy(), h


SCAN_T = [1, 3, 4, 5, 8, 9, 12, 13, 33]       # blocks of 4 steps, two alternating register sets of 8


@pytest.mark.parametrize("H", [64, 96])
def test_gru_scan_teacher_forced(L, torch_dev, H):
    """every out[t] against ONE float64 GRU step from the kernel's own out[t - 1] (h0 for t = 0): errors cannot compound, so the bound is the first-order one
    derived in kernel_ref.gru_step64; the final state equals out[T - 1] bit for bit."""
    for T in SCAN_T:
        s = Scan(L, torch_dev, H, T)
        out, h = s.run()
        assert np.abs(out).max() < 1, "the clamp must not be active: out[t] is h_t itself"
        prev = np.concatenate([s.h0[:, None], out[:, :-1]], axis=1)
        want, bound = kr.gru_step64(s.gi, s.Whh, s.bhh, prev, kr.EPS_SIG_HW, kr.EPS_TANH_HW)
        err = np.abs(out - want)
        print(f"k_gru_scan<{H}> T={T}: largest error / bound {np.max(err / bound):.3f}")
        bad = ~(err <= bound)
        assert not bad.any(), first_bad(bad, f"k_gru_scan<{H}> T={T}", out, want)
        assert np.array_equal(h.view(np.int32), out[:, -1].view(np.int32)), f"k_gru_scan<{H}> T={T}: final state differs from out[T - 1]"


@pytest.mark.parametrize("H", [64, 96])
def test_gru_scan_cutting_invariance(L, torch_dev, H):
    """one launch of T steps = the same steps cut into (1, T - 1), (3, 4, 5, ...) and T launches of one step, bit for bit"""
    for T in SCAN_T:
        s = Scan(L, torch_dev, H, T)
        out, h = s.run()
        ramp, n = [], 3
        while sum(ramp) < T:
            ramp.append(min(n, T - sum(ramp))); n += 1
        for cuts in ([1, T - 1] if T > 1 else [1], ramp, [1] * T):
            o2, h2 = s.run(cuts)
            bad = o2.view(np.int32) != out.view(np.int32)
            assert not bad.any(), first_bad(bad, f"k_gru_scan<{H}> T={T} cut into {cuts}", o2, out)
            assert np.array_equal(h2.view(np.int32), h.view(np.int32)), f"k_gru_scan<{H}> T={T} cut into {cuts}: final state"


@pytest.mark.parametrize("H", [64, 96])
def test_gru_scan_fragment_output(L, torch_dev, H):
    """outf: the same steps as binary16 planes in the encoder's fragment layout, one step late in the kernel (pend / tpend) and flushed after the loop:
    equal to numpy's split of 256 out[t], every other half-word (history tile, other columns, rows past T) untouched"""
    for T in (1, 31, 32, 33, 65):
        s = Scan(L, torch_dev, H, T, seed=7)
        out, h = s.run()
        NQ = 1 + (T + 31) // 32
        for col in (64, 224):
            buf, h2 = s.run(outf_col=col, NQ=NQ)
            what = f"k_gru_scan<{H}> outf T={T} col={col}"
            hi, lo = kr.frag_get(buf, np.arange(T), col, H)
            whi, wlo = kr.split16(out)
            bad = (hi != whi) | (lo != wlo)
            assert not bad.any(), first_bad(bad, what, kr.join16(hi, lo), out)
            kr.frag_untouched_except(buf, kr.frag_new(SCAN_B, NQ), [kr.frag_index(np.arange(T), col, H)], what)
            assert np.array_equal(h2.view(np.int32), h.view(np.int32)), what + ": final state"


# ================================================================================================================================================================
# rd_launch_encf_gemm / rd_launch_encf_hist
# ================================================================================================================================================================
def encf_kernel(K0, K1, N, wmode, seq, B, T):
    if wmode == "f16x2":
        return "k_encf_gemm<two planes>"
    return "k_encf_gemm<one plane, taps alternating>" if K0 > 0 and K0 == K1 and not seq else "k_encf_gemm<one plane>"


# name -> (K0, K1, N, wmode, seq_taps, outputs, B, T, kernel); every case runs for T in ENCF_T and B in ENCF_B, B and T here only feed the dispatch copy
ENCF_T, ENCF_B = (1, 31, 32, 33, 70), (1, 3, 9)
ENCF_CASES = {
    "conv-alternating": (160, 160, 96, "q16", 0, "yf", 3, 33, "k_encf_gemm<one plane, taps alternating>"),
    "conv-sequential": (160, 160, 96, "q16", 1, "yf", 3, 33, "k_encf_gemm<one plane>"),
    "gi-192": (0, 96, 192, "q16", 0, "y", 3, 33, "k_encf_gemm<one plane>"),
    "z-864-80": (0, 864, 80, "q16", 0, "y", 3, 33, "k_encf_gemm<one plane>"),
    "two-plane": (0, 96, 96, "f16x2", 0, "both", 3, 33, "k_encf_gemm<two planes>"),
}
ALL_ENCF_KERNELS = {"k_encf_gemm<one plane, taps alternating>", "k_encf_gemm<one plane>", "k_encf_gemm<two planes>"}
YCOL = 160


def run_encf(L, dev, B, T, K0, K1, N, wmode, X, W, scale, bias, dil, to_yf, seq=0, no_pair=0, act=0):
    """X [B][2 + T][K1]: steps -2 .. T - 1 of columns 0 .. K1 - 1.  Returns float32 rows [B][T][N] (to_yf: the joined planes, and their words)."""
    NQ = 1 + (T + 31) // 32
    xf = kr.frag_new(B, NQ)
    kr.frag_put(xf, np.arange(-2, T), 0, X)
    d = Dev(dev)
    x_d, b_d = d.put(xf), d.put(bias)
    a = kr.EncfArgs()
    a.xf, a.NQ, a.B, a.T, a.K0, a.K1, a.dil = x_d.data_ptr(), NQ, B, T, K0, K1, dil
    if wmode == "q16":
        plane, sc = kr.pack_q16(L, W, scale)
        p_d, s_d = d.put(plane), d.put(sc); a.Wp16, a.Wscale = p_d.data_ptr(), s_d.data_ptr()
    else:
        p_d = d.put(kr.pack_f16x2(L, W)); a.Wp16 = p_d.data_ptr()
    a.bias, a.N, a.act, a.seq_taps, a.no_pair = b_d.data_ptr(), N, act, seq, no_pair
    what = f"{encf_kernel(K0, K1, N, wmode, seq, B, T)} B={B} T={T} K0={K0} K1={K1} dil={dil} N={N} {'yf' if to_yf else 'y'} no_pair={no_pair}"
    if to_yf:
        yf0 = kr.frag_new(B, NQ)
        y_d = d.put(yf0, check=False); a.yf, a.ycol = y_d.data_ptr(), YCOL
    else:
        yst = N + 12; ya = kr.Rows(B, T, N, yst, T * yst + 2 * yst, off=4)       # 16-byte stores: offsets and strides multiples of 4 floats
        y_d = d.put(ya.words, check=False); a.y = y_d.data_ptr() + 4 * ya.base; a.y_sb, a.y_st = ya.sb, ya.st
    assert L.rd_launch_encf_gemm(C.byref(a), stream()) == 0
    sync()
    d.unchanged()
    if to_yf:
        buf = y_d.cpu().numpy().view(np.uint16).reshape(B, NQ, kr.EF_TILE)
        kr.frag_untouched_except(buf, yf0, [kr.frag_index(np.arange(T), YCOL, N)], what)
        hi, lo = kr.frag_get(buf, np.arange(T), YCOL, N)
        return kr.join16(hi, lo), (hi, lo), what
    yw = host32(y_d)
    ya.check_outside(yw, what)
    return ya.view(yw).copy(), None, what


@pytest.mark.parametrize("B", ENCF_B)
@pytest.mark.parametrize("name", list(ENCF_CASES))
def test_encf_gemm_exact(L, torch_dev, name, B):
    """k_encf_gemm on exact-grid fragments built by the numpy codec (rows 30, 31 of the history tile feed the taps of t < dil): bit equality with float64.
    The sequential tap order must equal the alternating one bit for bit on the exact grid (same seeds, same operands, same reference)."""
    K0, K1, N, wmode, seq, outs, _, _, _ = ENCF_CASES[name]
    for T in ENCF_T:
        for dil in ((1, 2) if K0 else (0,)):
            for grid in (("int8",) if wmode == "q16" else ("w12", "a12")):
                rng = np.random.default_rng(T + 100 * dil + N)
                X, W, scale, bias = kr.exact_gemm_operands(rng, B * T, K0 + K1, N, grid, F16_EXACT_BITS, conv=(B, T, dil, 2) if K0 else None)
                if not K0:
                    X = np.concatenate([np.full((B, 2, K1), NAN, np.float32), X.reshape(B, T, K1)], axis=1)     # no tap reads the history
                A = kr.conv_rows(X, T, dil, 2) if K0 else X[:, 2:].reshape(B * T, K1)
                want = kr.gemm_ref(A, W, bias)[0].astype(np.float32).reshape(B, T, N)
                for to_yf in ((True,) if outs == "yf" else (False,) if outs == "y" else (True, False)):
                    for no_pair in ((0, 1) if N == 192 else (0,)):
                        got, planes, what = run_encf(L, torch_dev, B, T, K0, K1, N, wmode, X, W, scale, bias, dil, to_yf, seq, no_pair)
                        encf_check_exact(got, planes, want, what + f" exact grid {grid}")


@pytest.mark.parametrize("name", list(ENCF_CASES))
def test_encf_gemm_random(L, torch_dev, name):
    """random operands (the activations as the 22-bit values the fragments hold), act = 1 on the conv shapes as the encoder has it: the derived bound; a
    fragment output adds the 2^-22 of its own two planes"""
    K0, K1, N, wmode, seq, outs, _, _, _ = ENCF_CASES[name]
    rng = np.random.default_rng(len(name))
    for B, T in ((3, 33), (9, 70)):
        dil = 2 if K0 else 0
        _, W, scale, bias = kr.random_gemm_operands(rng, 1, K0 + K1, N, int8=wmode == "q16")
        X = kr.join16(*kr.split16(rng.uniform(-1, 1, (B, 2 + T, K1)).astype(np.float32)))
        A = kr.conv_rows(X, T, dil, 2) if K0 else X[:, 2:].reshape(B * T, K1)
        act = 1 if K0 else 0
        y64, S = kr.gemm_ref(A, W, bias)
        bound = kr.gemm_bound(K0 + K1, S, y64, kr.R_F16)
        if act:
            y64 = np.tanh(y64); bound = bound + kr.EPS_TANH_HW
        for to_yf in ((True,) if outs == "yf" else (False,) if outs == "y" else (True, False)):
            got, _, what = run_encf(L, torch_dev, B, T, K0, K1, N, wmode, X, W, scale, bias, dil, to_yf, seq, 0, act)
            bnd = (bound + (2.0 ** -22 * np.abs(y64) + 2.0 ** -33 if to_yf else 0)).reshape(B, T, N)
            err = np.abs(got.astype(np.float64) - y64.reshape(B, T, N))
            print(f"{what}: largest error / bound {np.max(err / bnd):.3f}")
            bad = ~(err <= bnd)
            assert not bad.any(), first_bad(bad, what + " random", got, y64.reshape(B, T, N))


@pytest.mark.parametrize("B", [1, 3])
def test_encf_hist_rows_to_planes(L, torch_dev, B):
    """dir 0: the two float32 history rows -> rows 30, 31 of the history tile, as the codec splits them; nothing else written"""
    rng = np.random.default_rng(B)
    NQ, T = 3, 40
    rows = rng.uniform(-1, 1, (B, 2, 864)).astype(np.float32)
    xr = kr.Rows(B, 1, 2 * 864, 2 * 864 + 8, 2 * 864 + 24, off=4).fill(rows)
    xf0 = kr.frag_new(B, NQ)
    d = Dev(torch_dev)
    r_d, f_d = d.put(xr.words), d.put(xf0, check=False)
    assert L.rd_launch_encf_hist(f_d.data_ptr(), NQ, r_d.data_ptr() + 4 * xr.base, xr.sb, B, T, 0, stream()) == 0
    sync()
    d.unchanged()
    buf = f_d.cpu().numpy().view(np.uint16).reshape(B, NQ, kr.EF_TILE)
    hi, lo = kr.frag_get(buf, np.array([-2, -1]), 0, 864)
    whi, wlo = kr.split16(rows)
    bad = (hi != whi) | (lo != wlo)
    assert not bad.any(), first_bad(bad, "k_encf_hist dir 0", kr.join16(hi, lo), rows)
    kr.frag_untouched_except(buf, xf0, [kr.frag_index(np.array([-2, -1]), 0, 864)], "k_encf_hist dir 0")


@pytest.mark.parametrize("T", [2, 33])
def test_encf_hist_planes_to_rows(L, torch_dev, T):
    """dir 1: steps T - 2, T - 1 -> the history tile and the float32 rows.  The planes hold (hi, lo) pairs that are NOT what a split of their sum would give, so
    a kernel that re-splits instead of copying fails: the planes are copied bit for bit, the rows are 2^-8 (hi + lo)."""
    rng = np.random.default_rng(T)
    B, NQ = 3, 1 + (T + 31) // 32
    xf0 = kr.frag_new(B, NQ)
    steps = np.arange(-2, T)
    idx = kr.frag_index(steps, 0, 864)
    hi = rng.uniform(-256, 256, (B, len(steps), 864)).astype(np.float16); lo = rng.uniform(-1, 1, hi.shape).astype(np.float16)
    flat = xf0.reshape(B, -1); flat[:, idx] = hi.view(np.uint16); flat[:, idx + 512] = lo.view(np.uint16)
    rs = kr.split16(kr.join16(hi.view(np.uint16), lo.view(np.uint16)))
    assert (rs[1] != lo.view(np.uint16)).mean() > 0.5, "the planted planes must differ from a fresh split"
    xr = kr.Rows(B, 1, 2 * 864, 2 * 864 + 8, 2 * 864 + 24, off=4)
    d = Dev(torch_dev)
    r_d, f_d = d.put(xr.words, check=False), d.put(xf0, check=False)
    assert L.rd_launch_encf_hist(f_d.data_ptr(), NQ, r_d.data_ptr() + 4 * xr.base, xr.sb, B, T, 1, stream()) == 0
    sync()
    buf = f_d.cpu().numpy().view(np.uint16).reshape(B, NQ, kr.EF_TILE)
    want = xf0.copy()
    wf = want.reshape(B, -1); hidx = kr.frag_index(np.array([-2, -1]), 0, 864)
    wf[:, hidx] = hi[:, -2:].view(np.uint16); wf[:, hidx + 512] = lo[:, -2:].view(np.uint16)
    bad = np.argwhere(buf.reshape(B, -1) != wf)
    assert not bad.size, f"k_encf_hist dir 1 T={T}: {len(bad)} half-words differ from a bit copy of steps T - 2, T - 1 into the history tile, the first in stream {bad[0][0]} at offset {bad[0][1]}"
    rw = host32(r_d)
    xr.check_outside(rw, f"k_encf_hist dir 1 T={T}")
    rows = xr.view(rw).reshape(B, 2, 864)
    wrow = kr.join16(hi[:, -2:].view(np.uint16), lo[:, -2:].view(np.uint16))
    bad = rows.view(np.int32) != wrow.view(np.int32)
    assert not bad.any(), first_bad(bad, f"k_encf_hist dir 1 T={T} float32 rows", rows, wrow)
