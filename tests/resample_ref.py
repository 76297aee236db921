"""float64 restatement of the fractional resampler (include/rade_batch.h: rade_batch_resample, rade_resample_count, rade_resample_taps), shared by
tests/test_resample_host.py and tests/test_resample_gpu.py.  Everything the header pins is restated here from its text: the Q32.32 time base in Python integers,
the Kaiser-windowed sinc table (np.i0), both modes with zero extension, and the rounding bounds of the float32 kernel.  Holds no fixtures and needs no GPU."""
import numpy as np

SINC32, LINEAR = 0, 1
TAPS, PHASES, BETA = 32, 256, 10.0
EPS = 2.0 ** -24                                        # half an ulp of 1: the relative error of one float32 rounding
PPM_8020 = (8000.0 / 8020.0 - 1.0) * 1e6                # `sox -r 8000 .. -r 8020`: -2493.77


def q32(t0, ppm):
    """(step_q, t0_q): llrint of the doubles (round half to even, like Python's round)"""
    return round((1.0 + ppm * 1e-6) * 4294967296.0), round(t0 * 4294967296.0)


def positions(n0, n_out, t0, ppm):
    """(i, mu) of outputs n0 .. n0 + n_out - 1 as Python-integer arrays: pos_q = t0_q + n step_q, i = pos_q >> 32 (floor), mu = pos_q & 0xffffffff"""
    step_q, t0_q = q32(t0, ppm)
    pos = [t0_q + n * step_q for n in range(n0, n0 + n_out)]
    return np.array([p >> 32 for p in pos], np.int64), np.array([p & 0xffffffff for p in pos], np.int64)


def count(in_end, t0, ppm):
    """outputs n >= 0 with pos_q(n) < in_end 2^32, in closed form (the brute-force loop is in the host test)"""
    step_q, t0_q = q32(t0, ppm)
    need = (in_end << 32) - t0_q
    return 0 if need <= 0 else -(-need // step_q)


def taps64():
    """T [257, 32] in float64: g(j - 15 - p / 256) / sum_j g, g(t) = sinc(t) I0(10 sqrt(1 - (t / 16)^2)) / I0(10).  sin(pi t) is formed from the fraction p / 256 alone
    (sin(pi (k - f)) = -(-1)^k sin(pi f), and sin(pi f) = sin(pi (1 - f))), so that it is an exact 0 at both integer ends: rows 0 and 256 are exact impulses."""
    T = np.zeros((PHASES + 1, TAPS))
    k = np.arange(TAPS) - 15
    for p in range(PHASES + 1):
        f = p / 256.0
        sf = np.sin(np.pi * (f if p <= 128 else 1.0 - f))
        t = k - f
        with np.errstate(divide="ignore", invalid="ignore"):
            sinc = np.where(t == 0.0, 1.0, np.where(k % 2 == 1, sf, -sf) / (np.pi * t))
        g = sinc * np.i0(BETA * np.sqrt(np.maximum(1.0 - (t / 16.0) ** 2, 0.0))) / np.i0(BETA)
        T[p] = g / g.sum()
    return T


def gather(x, idx):
    """x[idx] with zeros outside [0, len(x))"""
    x = np.asarray(x)
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0, 0)


def resample(x, n_out, ppm, t0=0.0, mode=SINC32, n0=0, in_base=0, T=None):
    """float64 restatement for one stream: x complex (float32 values), T the table to use (the library's float32 one for the kernel tests; default taps64()).
    Returns (y complex128 [n_out], mag float64 [n_out, 2]): mag is, per real component, the sum of |coefficient| |operand| terms that the rounding bounds below
    multiply: sum_j (|T[p][j]| + |T[p+1][j]|) |x[i+j-15]| (sinc32), (1 - f) |x[i]| + f |x[i+1]| (linear)."""
    x = np.asarray(x).astype(np.complex128)
    i, mu = positions(n0, n_out, t0, ppm)
    comp = lambda v: np.stack([np.abs(v.real), np.abs(v.imag)], axis=-1)
    if mode == LINEAR:
        f = np.float32(mu / 4294967296.0).astype(np.float64)
        x0, x1 = gather(x, i - in_base), gather(x, i + 1 - in_base)
        return (1.0 - f) * x0 + f * x1, (1.0 - f)[:, None] * comp(x0) + f[:, None] * comp(x1)
    T = taps64() if T is None else np.asarray(T, np.float64)
    p, w = mu >> 24, (mu & 0xffffff) / 16777216.0
    y = np.zeros(n_out, np.complex128)
    mag = np.zeros((n_out, 2))
    for j in range(TAPS):
        xj = gather(x, i + j - 15 - in_base)
        y += (T[p, j] + w * (T[p + 1, j] - T[p, j])) * xj
        mag += (np.abs(T[p, j]) + np.abs(T[p + 1, j]))[:, None] * comp(xj)
    return y, mag


# float32 kernel against the float64 restatement on the same table, per real component:
#   sinc32: 32 products accumulated (fused or not: at most one rounding per term of a running sum bounded by the sum of magnitudes) + 4 for the coefficient's three
#           roundings and w  ->  36 eps sum_j (|T[p][j]| + |T[p+1][j]|) |x[i+j-15]|
#   linear: 2 products + 3 roundings (f, 1 - f, the sum)  ->  5 eps ((1 - f) |x[i]| + f |x[i+1]|)
KERNEL_ROUNDINGS = {SINC32: 36, LINEAR: 5}


def reference_bound(N, x):
    """the restatement's linear mode against dsp.py's sample_clock_offset over N outputs: the Q32.32 rounding of the step (2^-33 per output, accumulated N times), the
    reference's own accumulated double tin (N additions of about N 2^-52 each), both times the largest step of the input, plus float32 arithmetic on the sample"""
    x = np.asarray(x)
    return (N * 2.0 ** -33 + N * N * 2.0 ** -52) * np.abs(np.diff(x)).max() + 4 * EPS * np.abs(x).max()
