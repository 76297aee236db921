"""Float64 restatement of the channel and the Doppler generator in pieces (rade_batch_channel_piece, rade_batch_multipath_piece; radae_amd/csrc/rade_chanp.hip), its
bounds and its checkers.  numpy only, no GPU; holds no fixtures.  tests/test_chan_piece_host.py pins it (the phase against Python integers, the gain against its closed
form and against realised sequences) and proves that every checker can fail; tests/test_chan_piece_gpu.py holds the kernels to it sample by sample.

Every quantity is a function of the ABSOLUTE sample index n (64 bit).  Operands are the float32 words the kernel reads, taken as exact numbers; the arithmetic is float64 /
complex128 (2^-53 per operation: ignored against the float32 bounds).  A complex sample is compared by the magnitude of the difference, a Doppler sample per component.
u = U = 2^-24; CMUL, PHASOR, SQ2 and phase32 are tests/tx_ref.py's.

Bounds (derived; the measured constants are noise_ref.EPS, the Box-Muller of the device against float64, and EPS_CIS, the 32-bit phasor against float64 -- four times
EPS_CIS_MEASURED of tests/test_fm_gpu.py, restated here because test modules are not imported)
-------------------------------------------------------------------------------------------------------------------------------------------------------------------
Generator, per component of G_p[n] = (float)(hf_gain (y0 + (y1 - y0) fr)):
    u hf_gain (|y0| + |y1|)                          the one rounding to float32: |g| <= (1 - fr) |y0| + fr |y1| <= |y0| + |y1|  (multiple of u: 1)
  + hf_gain EPS sum |taps|                           each draw is within EPS of the float64 Box-Muller per component; the interpolation is a convex combination of two sums
  + hf_gain (n_taps + 8) 2^-53 XMAX sum |taps|       the FIR in double, k ascending, contracted or not, and the four operations of the interpolation; XMAX = 8 bounds a
                                                     component of a draw (sqrt(-2 ln 2^-33) = 6.8)
Channel, in the kernel's order (tests/tx_ref.py's chan_ref, with the integer phase in place of the float32 one):
    two-path    CMUL (|tx[n]| |G1[n]| + |tx[n-16]| |G2[n-16]|) + SQ2 u |m|
    gain        u |v|
    phase       (EPS_CIS + CMUL) |v|: the phase itself is an integer, exact; the phasor of its top 32 bits is within EPS_CIS; one complex product
    noise       explicit: SQ2 2 u (|v| + sigma |noise|) (product and sum).  Generated: SQ2 sigma EPS for the draw (complex: each component sigma 0.70710678f EPS, as a
                magnitude sigma EPS; real: sigma EPS) + SQ2 3 u (|v| + |sigma g|) (two products and a sum)
    tone        its float32 phase as the kernel forms it (tx_ref.phase32), sincosf to 1 ulp per component: (PHASOR + slack + SQ2 u) |s| + SQ2 u |v + s|
    rx_gain     u |v|
"""
import numpy as np

import noise_ref as nr
import fm_ref as fr
import tx_ref as tx
from tx_ref import CMUL, PHASOR, SQ2, check_bits, check_close  # noqa: F401
from kernel_ref import U

EPS_CIS = 4 * 7.753e-08          # EPS_CIS of tests/test_fm_gpu.py
XMAX = 8.0
DELAY = 16
NOISE_COMPLEX, NOISE_REAL = 0, 1
M64 = (1 << 64) - 1
HALF32 = float(np.float32(0.70710678))


# ---- the expected-value gain -------------------------------------------------------------------------------------------------------------------------------------------
def multipath_gain(taps):
    """1 / sqrt(2 ((2/3) R0 + (1/3) R1)), R0 = 2 sum t^2, R1 = 2 sum t[k] t[k + 1], t the float32 taps widened to double"""
    t = np.asarray(taps, np.float32).astype(np.float64)
    R0, R1 = 2.0 * np.sum(t * t), 2.0 * np.sum(t[:-1] * t[1:])
    return 1.0 / np.sqrt(2.0 * ((2.0 / 3.0) * R0 + (1.0 / 3.0) * R1))


# ---- the integer phase ---------------------------------------------------------------------------------------------------------------------------------------------------
def phase_q(f0, df_dt):
    """(f0q, dq) as Python integers below 2^64, two's complement: llrint(turns 2^64) and llrint(df_dt / 8000^2 2^64) in double, turns = the rate the whole call turns at:
    without a drift the float32 omega ((f0 * 2) * pi) / 8000 over 2 pi, with one the double f0 / 8000"""
    f0, df_dt = np.float32(f0), np.float32(df_dt)
    if df_dt == 0:
        turns = np.float64(((f0 * np.float32(2.0)) * np.float32(np.pi)) / np.float32(8000.0)) / (2.0 * np.pi)
    else:
        turns = np.float64(f0) / 8000.0
    f0q = int(np.rint(turns * 18446744073709551616.0))
    dq = int(np.rint(np.float64(np.float32(df_dt)) / 64000000.0 * 18446744073709551616.0))
    return f0q & M64, dq & M64


def phase(n, f0q, dq, inclusive=True):
    """ph[n] = (n + 1) f0q + T(n) dq mod 2^64, T(n) = n (n + 1) / 2 formed by halving the even factor first, in wrapping uint64 arithmetic as the kernel has it.
    inclusive=False is the planted bug: the sum up to n - 1."""
    n = np.atleast_1d(np.asarray(n, dtype=np.uint64))
    one = np.uint64(1)
    with np.errstate(over="ignore"):
        if not inclusive:
            n = n - one                      # n = 0 wraps to 2^64 - 1: (n + 1) = 0 and T = 0, the empty sum
        T = np.where((n & one).astype(bool), n * ((n + one) >> one), (n >> one) * (n + one))
        return (n + one) * np.uint64(f0q) + T * np.uint64(dq)


def rotor(n, f0, df_dt, inclusive=True):
    """the float64 phasor of the top 32 bits of the phase"""
    f0q, dq = phase_q(f0, df_dt)
    return fr.cis((phase(n, f0q, dq, inclusive) >> np.uint64(32)).astype(np.uint32))


# ---- draws ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def low_draws(seed, b, p, xi):
    """x_p[xi] of stream b, complex128: words 0-1 of counter (xi & 0xffffffff, 2 b + p, 1, xi >> 32)"""
    k0, k1 = nr._key(seed)
    xi = np.asarray(xi, dtype=np.uint64)
    r = nr.philox4x32_10(xi & nr.MASK, 2 * b + p, 1, xi >> np.uint64(32), k0, k1)
    x, y = nr.gauss_pair(r[0], r[1])
    return x + 1j * y


def chan_draws(seed, b, n):
    """the unit Gaussians (g.x, g.y) of the samples of absolute indices n of stream b: counter (P & 0xffffffff, b, 0, P >> 32), P = n >> 1, words 0-1 for even n, 2-3 odd"""
    k0, k1 = nr._key(seed)
    n = np.asarray(n, dtype=np.uint64)
    P = n >> np.uint64(1)
    r = nr.philox4x32_10(P & nr.MASK, b, 0, P >> np.uint64(32), k0, k1)
    odd = (n & np.uint64(1)).astype(bool)
    ex, ey = nr.gauss_pair(r[0], r[1]); ox, oy = nr.gauss_pair(r[2], r[3])
    return np.where(odd, ox, ex), np.where(odd, oy, ey)


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------------------------------------
def dopp_ref(taps, ratio, hf_gain, seed, b, n0, n_out, i0_bug=0):
    """(G complex128 [n_out][2], bound per component [n_out][2][2]) of stream b over absolute indices [n0, n0 + n_out).  i0_bug = 1 is the planted off-by-one in i0."""
    t = np.asarray(taps, np.float32).astype(np.float64); n_taps = len(t)
    n = n0 + np.arange(n_out, dtype=np.int64)
    i0 = n // ratio
    frac = (n - i0 * ratio).astype(np.float64) / float(ratio)
    i0 = i0 + i0_bug
    lo = int(i0.min())
    ny = int(i0.max()) - lo + 2
    st = np.abs(t).sum()
    G = np.empty((n_out, 2), np.complex128); bound = np.empty((n_out, 2, 2))
    for p in range(2):
        x = low_draws(seed, b, p, lo + 1 + np.arange(ny - 1 + n_taps))         # x[lo + 1 ..]
        # y[i] = sum_k t[k] x[i + n_taps - k], i = lo .. lo + ny - 1: index of x[i + n_taps - k] in the array = (i - lo) + n_taps - 1 - k
        y = np.array([np.dot(t, x[i + n_taps - 1 - np.arange(n_taps)]) for i in range(ny)])
        y0, y1 = y[i0 - lo], y[i0 - lo + 1]
        G[:, p] = hf_gain * (y0 + (y1 - y0) * frac)
        for c, part in enumerate((np.real, np.imag)):
            bound[:, p, c] = hf_gain * (U * (np.abs(part(y0)) + np.abs(part(y1))) + st * nr.EPS + (n_taps + 8) * 2.0 ** -53 * XMAX * st)
    return G, bound


def check_dopp(got, ref, what):
    """k_dopp_piece's pairs [n_out][2] complex64 of one stream against dopp_ref, per component; returns the largest error / bound"""
    g = np.ascontiguousarray(got, np.complex64).view(np.float32).reshape(got.shape + (2,))
    want = np.stack([ref[0].real, ref[0].imag], axis=-1)
    return check_close(g, want, ref[1], what, ("sample", "path", "component"))


# ---- the channel -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _at(row, base, n):
    """row[n - base] where that lies inside the row and n >= 0, else 0"""
    row = np.asarray(row)
    g = n - base
    ok = (g >= 0) & (g < len(row)) & (n >= 0)
    return np.where(ok, row[np.clip(g, 0, max(len(row) - 1, 0))] if len(row) else 0, 0)


def chan_ref(txs, in_base, n0, n_out, b=0, G=None, g_base=0, gain=1.0, sigma=0.0, freq_offset=0.0, df_dt=0.0, noise=None, seed=0, noise_mode=NOISE_COMPLEX,
             sine_amp=0.0, sine_freq=0.0, rx_gain=1.0, bug=None):
    """One stream of rade_batch_channel_piece: txs complex64 [n_in] (sample g = absolute index in_base + g), G complex64 [n_g][2] (pair g = absolute index g_base + g)
    or None, noise complex64 [>= n_out] or None (then generated from seed, 0 = none).  Returns (rx complex128 [n_out], bound [n_out]).
    bug: a planted one -- "delay" (the second path taken at n instead of n - 16), "exclusive" (the phase sum without its last term), "imag" (the real noise mode on the
    imaginary part)."""
    txs = tx.c128(np.asarray(txs, np.complex64))
    n = n0 + np.arange(n_out, dtype=np.int64)
    x0 = _at(txs, in_base, n)
    if G is None:
        v = x0.astype(np.complex128); e = np.zeros(n_out)
    else:
        G = np.asarray(G, np.complex64).astype(np.complex128)
        d = 0 if bug == "delay" else DELAY
        x1, g1, g2 = _at(txs, in_base, n - d), _at(G[:, 0], g_base, n), _at(G[:, 1], g_base, n - d)
        late = n >= DELAY
        v = x0 * g1 + np.where(late, x1 * g2, 0)
        e = CMUL * (np.abs(x0) * np.abs(g1) + np.where(late, np.abs(x1) * np.abs(g2), 0)) + SQ2 * U * np.abs(v)
    gain = np.float64(np.float32(gain)); gain = 1.0 if gain == 0 else gain
    v = v * gain; e = e * abs(gain) + U * np.abs(v)
    if np.float32(freq_offset) != 0 or np.float32(df_dt) != 0:
        v = v * rotor(n, freq_offset, df_dt, inclusive=bug != "exclusive"); e = e + np.abs(v) * (EPS_CIS + CMUL)
    sg = np.float64(np.float32(sigma))
    if noise is not None:
        nz = sg * tx.c128(np.asarray(noise, np.complex64))[:n_out]
        e = e + SQ2 * 2 * U * (np.abs(v) + np.abs(nz)); v = v + nz
    elif seed:
        gx, gy = chan_draws(seed, b, n)
        if noise_mode == NOISE_REAL:
            nz = sg * gx * (1j if bug == "imag" else 1.0) + 0j
        else:
            nz = sg * HALF32 * (gx + 1j * gy)
        e = e + SQ2 * sg * nr.EPS + SQ2 * 3 * U * (np.abs(v) + np.abs(nz)); v = v + nz
    if sine_amp != 0:
        cyc = n.astype(np.float64) * np.float64(np.float32(sine_freq)) / 8000.0
        ph, slack = tx.phase32(6.283185307179586 * (cyc - np.floor(cyc)))
        s = np.float64(np.float32(sine_amp)) * np.exp(1j * ph)
        e = e + np.abs(s) * (PHASOR + slack + SQ2 * U) + SQ2 * U * np.abs(v + s); v = v + s
    g = np.float64(np.float32(rx_gain)); g = 1.0 if g == 0 else g
    v = v * g; e = e * abs(g) + SQ2 * U * np.abs(v)
    return v, e


def check_chan(got, ref, what):
    """k_chan_piece's samples [n_out] complex64 of one stream against chan_ref; returns the largest error / bound"""
    return check_close(np.asarray(got, np.complex64), ref[0], ref[1], what, ("sample",))
