"""float64 restatement of the rational rate converter (include/rade_batch.h: rade_batch_rate_convert, rade_rate_count, rade_rate_taps), shared by
tests/test_rate_host.py and tests/test_rate_gpu.py.  Everything the header pins is restated here from its text: the integer time base in Python integers, the
Kaiser-windowed sinc table (np.i0) with the exact-impulse rule, zero extension, the three input formats and the rounding bound of the float32 kernel.  Holds no
fixtures and needs no GPU."""
from math import gcd

import numpy as np

C64, S16_REAL, S16_IQ = 0, 1, 2
BETA = 10.0
EPS = 2.0 ** -24                                        # half an ulp of 1: the relative error of one float32 rounding


def reduce(L, M):
    """(L, M, K, T) of the reduced pair: K = ceil(M / L), T = 32 K"""
    g = gcd(L, M)
    L, M = L // g, M // g
    K = -(-M // L)
    return L, M, K, 32 * K


def positions(n0, n_out, L, M):
    """(i, ph) of outputs n0 .. n0 + n_out - 1 as integer arrays: i = floor(n M / L), ph = (n M) mod L, in Python integers"""
    L, M, _, _ = reduce(L, M)
    pos = [n * M for n in range(n0, n0 + n_out)]
    return np.array([p // L for p in pos], np.int64), np.array([p % L for p in pos], np.int64)


def count(in_end, L, M):
    """outputs n >= 0 with n M < in_end L, in closed form (the brute-force loop is in the host test)"""
    return 0 if in_end <= 0 else -(-(in_end * L) // M)


def taps64(L, M):
    """C [L, T] in float64: g(t_j) / sum_j g(t_j), t_j = j - (T / 2 - 1) - ph / L, g(t) = sinc(t / W) I0(10 sqrt(1 - (t / H)^2)) / I0(10) for |t| <= H = 16 K,
    W = max(1, M / L).  For M <= L sin(pi t) is formed from the fraction f = ph / L alone (sin(pi (k - f)) = -(-1)^k sin(pi f), and sin(pi f) = sin(pi (1 - f))),
    so that row 0 is the exact unit impulse at j = 15."""
    L, M, K, T = reduce(L, M)
    H, W = 16.0 * K, max(1.0, M / L)
    C = np.zeros((L, T))
    k = np.arange(T) - (T // 2 - 1)
    for ph in range(L):
        f = ph / L
        t = k - f
        with np.errstate(divide="ignore", invalid="ignore"):
            if M <= L:
                sf = np.sin(np.pi * (f if 2 * ph <= L else 1.0 - f))
                sinc = np.where(t == 0.0, 1.0, np.where(k % 2 == 1, sf, -sf) / (np.pi * t))
            else:
                sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t / W) / (np.pi * t / W))
        g = np.where(np.abs(t) <= H, sinc * np.i0(BETA * np.sqrt(np.maximum(1.0 - (t / H) ** 2, 0.0))) / np.i0(BETA), 0.0)
        C[ph] = g / g.sum()
    return C


def operand(x, fmt=C64, gain=1.0):
    """the complex operands of a stream, as float32 values in complex128: complex64 as it is; int16 [n] -> (gain (float)s, +0); int16 [n, 2] -> gain (float)(I, Q),
    one float32 multiply per component"""
    x = np.asarray(x)
    if fmt == C64:
        return x.astype(np.complex64).astype(np.complex128)
    g = np.float32(gain)
    v = (g * x.astype(np.float32)).astype(np.float32).astype(np.float64)
    return v.astype(np.complex128) if fmt == S16_REAL else v[:, 0] + 1j * v[:, 1]


def gather(x, idx):
    """x[idx] with zeros outside [0, len(x))"""
    x = np.asarray(x)
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0, 0)


def convert(x, n_out, L, M, n0=0, in_base=0, C=None, fmt=C64, gain=1.0):
    """float64 restatement for one stream: x in the given input format, C the table to use (the library's float32 one for the kernel tests; default taps64()).
    Returns (y complex128 [n_out], mag float64 [n_out, 2]): mag is, per real component, sum_j |C[ph][j]| |x[i + j - (T / 2 - 1)]|, what the rounding bound multiplies."""
    L, M, _, T = reduce(L, M)
    x = operand(x, fmt, gain)
    C = taps64(L, M) if C is None else np.asarray(C, np.float64)
    assert C.shape == (L, T)
    i, ph = positions(n0, n_out, L, M)
    y = np.zeros(n_out, np.complex128)
    mag = np.zeros((n_out, 2))
    for j in range(T):
        xj = gather(x, i + j - (T // 2 - 1) - in_base)
        y += C[ph, j] * xj
        mag += np.abs(C[ph, j])[:, None] * np.stack([np.abs(xj.real), np.abs(xj.imag)], axis=-1)
    return y, mag


def kernel_bound(L, M, mag):
    """float32 kernel against the float64 restatement on the same table, per real component: T fused terms with one rounding each (a running sum bounded by the sum of
    magnitudes), plus one to absorb second-order terms -> (T + 1) 2^-24 mag"""
    return (reduce(L, M)[3] + 1) * EPS * mag


def prototype(C, L):
    """the table laid out at the rate L Fin: p[u - u_min] = C[ph][j] at u = (j - (T / 2 - 1)) L - ph (time in 1 / L input samples), u_min = -(T / 2 - 1) L - (L - 1);
    length L T"""
    C = np.asarray(C, np.float64)
    T = C.shape[1]
    p = np.zeros(L * T)
    for ph in range(L):
        p[np.arange(T) * L - ph + (L - 1)] = C[ph]
    return p
