"""complex_bpf.bpf (the reference's dsp.py:39-102) for a stream cut into calls, restated for the unit tests of the streaming band-pass filter (k_bpf_chain, k_bpf_fir,
k_bpf_advance of radae_amd/csrc/rade_rx.hip; rx2_bpf_own of rade_bpf.h): tests/test_bpf_ref_host.py holds the model to the reference's recordings and shows that the
per-sample check rejects what it is there for, tests/test_bpf_units_gpu.py holds the device to the model.  numpy only; holds no fixtures.  The checkers are tx_ref's.

The model
---------
State (mem, mem_len, phase).  The taps are radae_amd.acq.bpf_design()'s float32 words and E[j] = exp(-1j alpha (j + 1)), j < 1152, the complex64 table of rd_tables_fill
(the argument alpha (j + 1) formed in double and rounded to float32, its cosine and sine rounded once); both are taken as exact numbers.

PHASES, in explicit float32 without fused multiply-adds (cmul32: re = ar br - ai bi, each product and the difference rounded; the device's cmul_nc):  a call of n
samples that starts at phase P mixes sample j down by ph[j] = P E[j] and leaves P E[n - 1].  The reference forms the same products in complex64 and rounds there, so the
model takes ph[j] as the reference defines it, and the device is held to the chain bit for bit.

SAMPLES, in float64 given those complex64 phases: w = [mem | x ph], y[i] = conj(ph[i]) sum_{t < 101} h[t] w[i + t], mem <- the last 102 of w.  The memory is 100 zeros
before the first call (dsp.py:55) and 102 samples after it (dsp.py:96), and the strided window always starts at index 0: from the second call on y[i] is the filter's
output two samples earlier, mixed up with the phase of its own position.  clip: min(|y|, 1) exp(1j angle(y)) (radae_txe.py:132).

STATE AFTER advance (k_bpf_advance), in float32: the last 102 baseband samples x (P E) in the kernel's order, cmul32(x, cmul32(P, E[j])); the phase after the last whole
block; mem_len 102.  The device is held to these bit for bit.

The per-sample bound (counted, not fitted)
------------------------------------------
S[i] = sum_t |h[t]| |w[i + t]| over the float64 window; X = the largest |component| of the call's window [mem | block] (what bpf_stage_planes scales by).  u = 2^-24.
The model and the kernel differ in these roundings and in nothing else; the count follows include/rade_batch.h's for k_file_bpf (same staging, same tile function), less
the mixer table's own error (E is an operand here, not a function value), in units of 2^-20 S:
    down mixer    x ph in float32, two products and a difference per component, 2 sqrt 2 u |x| as a modulus                                           0.177
    operand split hi = binary16(v), lo = binary16(v - hi): 2^-11 x 2^-11 of |v| per component                                                        0.25
    taps' planes  2^10 h the same way                                                                                                                  0.25
    lo x lo       dropped: at most 2^-11 |v| 2^-11 |h|                                                                                                 0.25
    hi x hi       four dependent matrix instructions (K = 32), ASSUMED as for the acquisition: each returns its 33-term sum within 2^-23 of the sum of
                  the terms' moduli                                                                                                                    0.5
    hi x lo, lo x hi  the same chains on operands 2^-10 smaller: 8 x 2^-23 x 2^-10                                                                     0.001
    three-way sum two float32 additions                                                                                                                0.125
    up mixer      conj(ph) y in float32 on |y| <= S (times the power of two that undoes the scales: exact); this is also the final store                0.177
    sum 1.73, times 1.01 for the terms of second order:   EPS = 1.75 x 2^-20 = 1.67e-6.
What binary16 underflow leaves: a plane entry below 2^-14 (in operand scale, where X sits in [2^7, 2^8)) is a multiple of 2^-24, so a sample component is off by up
to 2^-25 x 2^-7 X = 2^-32 X (sqrt 2 sum |h| = 2.9 of them per output) and a tap by 2^-25 x 2^-10 (101 of them on components <= X, sqrt 2 as a modulus): under
2^-28 X + 2^-30 X;   TINY = 2^-27, rade_batch.h's RADE_FILE_BPF_TINY.
    |y^[i] - y[i]| <= EPS S[i] + TINY max(X, XFLOOR) + DENORM.
The window differs from k_file_bpf's (102 + one block of up to 1152 samples, not 1024 outputs + 100): X is taken over that window.  The exponent clamps differ too:
bpf_stage_planes clamps the biased exponent e of X to [32, 222].  Inside, 2^-95 <= X < 2^96, the scale 2^(134 - e) puts X into [2^7, 2^8) and the above holds.
Below, X < 2^-95, the scale stays 2^102: X sits below 2^7, the planes' floor 2^-25 no longer shrinks with X, and the second term stays TINY x XFLOOR, XFLOOR = 2^-95 --
a relative error that grows as the block fades, all of the block lost below 2^-127.  Above, the scale stays 2^-88: X sits in [2^(7 + e - 222), ..), the relative terms are
unchanged (binary16 keeps 11 bits wherever the operand lies) and the floor term only shrinks, so the bound holds as it stands while every plane entry is finite:
X < 65520 x 2^88, a little under 2^104.  From there on binary16 overflows and the block's outputs are infinities and NaNs.  DENORM = 16 x 2^-149 covers float32's own
underflow in the mixers (a rounding of a subnormal product is off by up to 2^-150, not by u of it).

Clip (k_bpf_fir, clip = 1): m2 = re^2 + im^2 in float32; m2 > 1: y / sqrt(m2).  The exact clip is the projection onto the unit disc, 1-Lipschitz, so the filter's
error passes through unamplified.  Its own evaluation: m2 within 2 u (two products and a sum of positive terms), the square root halves that and adds its ulp (2 u), the
reciprocal adds 2 u, the product u: 6 u of a value of modulus 1, CLIP = 6 u.  Where the float32 decision and the exact one differ, |y| is within 2 u of 1 and clipping
moves it by less than that: covered.

Run as a program (python tests/bpf_ref.py REFERENCE_DIR) the model is held to the reference's own complex_bpf over a few call partitions and the gap is printed."""
import ctypes as C
import functools
import os
import sys

import numpy as np

from dev_abi import BpfArgs, BpfState, Tables  # noqa: F401  (the records of rade_dev.h, stated in tests/dev_abi.py)
from kernel_ref import U, vp

NTAP, NMF, NEOO, MEM = 101, 960, 1152, 102
EPS = 1.75 * 2.0 ** -20
TINY = 2.0 ** -27
XFLOOR = 2.0 ** -95            # biased exponent 32: below it the operand scale no longer follows the block
XCEIL = 65520.0 * 2.0 ** 88    # the first value a plane entry cannot hold (binary16 rounds 65520 to infinity) under the scale of biased exponent 222
DENORM = 16 * 2.0 ** -149
CLIP = 6 * U
EB_MIN, EB_MAX = 32, 222       # bpf_stage_planes' clamps of the biased exponent of X


_taps = None


def use_taps(h32=None):
    """the float32 taps the model filters with: None = radae_amd.acq.bpf_design()'s (the reference's own words); the device tests hand in the words the kernels read
    (rd_tables_fill's bpf_h), which tests/test_bpf_ref_host.py holds to the former"""
    global _taps
    _taps = None if h32 is None else np.asarray(h32, np.float32).astype(np.float64)


@functools.lru_cache(None)
def _design():
    from radae_amd.acq import bpf_design
    h, alpha = bpf_design()
    arg = (np.float64(np.float32(alpha)) * np.arange(1, NEOO + 1)).astype(np.float32).astype(np.float64)
    E = np.empty(NEOO, np.complex64)
    E.real, E.imag = np.cos(arg).astype(np.float32), (-np.sin(arg)).astype(np.float32)
    return h.astype(np.float64), float(alpha), E


def design():
    """(h float64 [101] -- the float32 taps, alpha, E complex64 [1152] -- rd_tables_fill's bpf_E restated)"""
    h, alpha, E = _design()
    return (h if _taps is None else _taps), alpha, E


def cmul32(a, b):
    """complex64 product in explicit float32, every product, the difference and the sum rounded on their own (cmul_nc of rade_devutil.h)"""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    ar, ai, br, bi = a.real.astype(np.float32), a.imag.astype(np.float32), b.real.astype(np.float32), b.imag.astype(np.float32)
    out = np.empty(np.broadcast(a, b).shape, np.complex64)
    out.real = (ar * br).astype(np.float32) - (ai * bi).astype(np.float32)
    out.imag = (ar * bi).astype(np.float32) + (ai * br).astype(np.float32)
    return out


def blocks_of(len0, avail):
    """the block grid of an invocation: len0, then 960s, the last one partial"""
    sizes, pos = [], 0
    while pos < avail:
        n = min(len0 if not sizes else NMF, avail - pos)
        sizes.append(n); pos += n
    return sizes


def chain(phase, len0, avail, chain_stride=1 << 30):
    """k_bpf_chain: the phases c[1 + k], k = 0 .. up to and including the first block beyond the input; every block steps by its WHOLE length (E[len0 - 1], E[959])"""
    _, _, E = design()
    P, out, start, k = np.complex64(phase), [], 0, 0
    while k + 1 < chain_stride:
        out.append(P)
        if start >= avail:
            break
        P = cmul32(P, E[(min(max(len0, 1), NEOO) if k == 0 else NMF) - 1])[()]
        start += NMF if k else len0
        k += 1
    return np.array(out, np.complex64)


class State:
    """what complex_bpf carries: mem complex128 [mem_len] (float32 values when it came from a device record), phase complex64"""

    def __init__(self, mem=None, phase=1.0 + 0.0j):
        self.mem = np.zeros(NTAP - 1, np.complex128) if mem is None else np.asarray(mem, np.complex128).copy()
        self.phase = np.complex64(phase)

    @property
    def mem_len(self):
        return len(self.mem)

    def copy(self):
        return State(self.mem, self.phase)


def taps_lo():
    """the low binary16 plane of the taps, 2^-10 (2^10 h - binary16(2^10 h)): what the lo x hi product carries"""
    h = design()[0]
    v = (h * 1024).astype(np.float32)
    return (v - v.astype(np.float16).astype(np.float32)).astype(np.float16).astype(np.float64) / 1024


def call(st, x, bug=None):
    """one call of complex_bpf.bpf on State st (advanced in place) -> (y complex128 [n], S [n], X).  bug = one mistake, for the host tests (run())"""
    h, _, E = design()
    x = np.asarray(x, np.complex64); n = len(x)
    kind = bug[0] if bug else None
    P = cmul32(st.phase, E[n - 1])[()] if kind == "phase_next" else st.phase
    ph = cmul32(P, E[:n]).astype(np.complex128)
    mem = np.concatenate([np.zeros(2), st.mem]) if kind == "first_delay" and st.mem_len == NTAP - 1 else st.mem
    w = np.concatenate([mem, x.astype(np.complex128) * ph])
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([w, np.zeros(NTAP, np.complex128)]), NTAP)[:n]
    acc = win @ h
    if kind == "tap":
        acc[bug[1]] -= h[bug[2]] * win[bug[1], bug[2]]
    if kind == "lohi":
        acc -= win @ taps_lo()
    y = acc * np.conj(ph)
    S = np.abs(win) @ np.abs(h)
    X = float(max(np.abs(w.real).max(), np.abs(w.imag).max())) if len(w) else 0.0
    st.mem = w[-MEM - 1:-1] if kind == "mem_shift" else w[-MEM:]
    if n:
        st.phase = np.complex64(cmul32(st.phase, E[n - 1])[()])
    return y, S, X


def clip(y):
    m = np.abs(y)
    return np.where(m > 1, y / np.where(m > 1, m, 1), y)


def bound(S, X):
    return EPS * S + TINY * np.maximum(X, XFLOOR) + DENORM


def run(x, sizes, st=None, do_clip=False, bug=None):
    """the stream x cut into calls of the given sizes -> (y complex128, bound, final State).  The bound is the device's (module docstring), CLIP added when clipping.
    bug = (call index, kind, ...) plants one mistake in that call (tests/test_bpf_ref_host.py): "tap", i, t -- tap t's product missing from output i; "lohi" -- the
    taps' low plane times the samples dropped; "first_delay" -- a first call filtered as if its memory had 102 samples; "phase_next" -- the block mixed with its
    successor's phase; "mem_shift" -- the memory it leaves one sample late"""
    st = State() if st is None else st.copy()
    ys, bs, pos = [], [], 0
    for k, n in enumerate(sizes):
        n = int(n)
        y, S, X = call(st, x[pos:pos + n], bug[1:] if bug and bug[0] == k else None)
        pos += n
        ys.append(y); bs.append(bound(S, X))
    y = np.concatenate(ys) if ys else np.zeros(0, np.complex128)
    b = np.concatenate(bs) if bs else np.zeros(0)
    return (clip(y), b + CLIP, st) if do_clip else (y, b, st)


def cond(x, sizes, st=None):
    """S[i] = sum |h| |w| per sample alone (the host tests' yardstick)"""
    st = State() if st is None else st.copy()
    out, pos = [], 0
    for n in sizes:
        out.append(call(st, x[pos:pos + int(n)])[1]); pos += int(n)
    return np.concatenate(out)


def state32(x, len0, avail, mem, mem_len, phase):
    """the record k_bpf_advance leaves after an invocation (len0, avail) that started from (mem float32-valued complex [102], mem_len, phase): (mem complex64 [102],
    mem_len, phase complex64).  avail < 102 or len0 <= 0: the record stays as it was (the device's contract, rd_bpf_args)"""
    if avail < MEM or len0 <= 0:
        return np.asarray(mem, np.complex64).copy(), mem_len, np.complex64(phase)
    _, _, E = design()
    c = chain(phase, len0, avail)
    q = np.arange(avail - MEM, avail)
    k = np.where(q < len0, 0, 1 + (q - len0) // NMF)
    sk = np.where(k > 0, len0 + (k - 1) * NMF, 0)
    m = cmul32(np.asarray(x, np.complex64)[q], cmul32(c[k], E[q - sk]))
    nb = 1 if avail <= len0 else 1 + (avail - len0 + NMF - 1) // NMF
    return m, MEM, c[nb]


BPF16_HALFS = 4 * 2 * 64 * 8        # rd_bpf16_table_fill's table


def host_tables(L):
    """(h float32 [101], E complex64 [1152], the binary16 tap table as uint16 [4096]) from rd_tables_fill / rd_bpf16_table_fill"""
    T = Tables()
    L.rd_tables_fill(C.byref(T))
    t16 = np.zeros(BPF16_HALFS, np.uint16)
    L.rd_bpf16_table_fill(C.byref(T), t16.ctypes.data_as(vp))
    return np.ctypeslib.as_array(T.bpf_h)[:NTAP].copy(), np.ctypeslib.as_array(T.bpf_E).view(np.complex64).copy(), t16


def live(ref_dir):
    """the model against the reference's own complex_bpf, call by call, over a few partitions (a child process where the reference exists)"""
    os.environ["MPLBACKEND"] = "Agg"
    sys.path.insert(0, ref_dir)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.chdir(ref_dir)
    from radae.dsp import complex_bpf
    f = np.float32
    w = (f(2 * np.pi) * (15 + np.arange(30, dtype=f)) / f(160)).astype(f)
    bandwidth, centre = f(1.2) * (w[29] - w[0]) * f(8000) / f(2 * np.pi), (w[29] + w[0]) * f(8000) / f(2 * np.pi) / f(2)
    rng = np.random.default_rng(7)
    worst = 0.0
    for sizes in ([960] * 4, [800, 960, 1120, 960], [1120, 800, 800, 960, 1152], [960, 300, 101, 102, 960]):
        n = sum(sizes)
        x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.5).astype(np.complex64)
        ref = complex_bpf(NTAP, 8000, bandwidth, centre, 8000)
        got, pos = [], 0
        for k in sizes:
            got.append(np.array(ref.bpf(x[pos:pos + k]), np.complex64)); pos += k
        y, _, _ = run(x, sizes)
        gap = float((np.abs(np.concatenate(got) - y) / cond(x, sizes)).max())
        worst = max(worst, gap)
        print(f"complex_bpf {sizes}: largest |reference - model| = {gap / U:.2f} x 2^-24 of sum |h| |w|")
    print(f"live ok: worst {worst / U:.2f} x 2^-24")


if __name__ == "__main__":
    live(sys.argv[1])
