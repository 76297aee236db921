"""float64 restatement of the analog FM stage (include/rade_batch.h: rade_batch_fm_mod, rade_batch_fm_demod, rade_fm_taps, rade_fm_sigma), shared by
tests/test_fm_host.py and tests/test_fm_gpu.py.  It restates the reference's fm.m line by line -- the design of fm.m:8-47, analog_fm_mod (:74-94), analog_fm_demod
(:97-126), the test-tone measurement of :180-196 -- plus the bit-level rules the header adds: the 32-bit NCO increments, the quadrant-exact phasor, the window zeros,
the de-emphasis folded into the output filter.  numpy only; holds no fixtures and needs no GPU."""
from fractions import Fraction

import numpy as np

import noise_ref as nr

F32, C64 = 0, 1
OUT_COMPLEX, OUT_REAL = 0, 1
U = 2.0 ** -24                                          # half an ulp of 1: the relative error of one float32 rounding
TC = 50e-6                                              # fm.m:17
TWO32 = 4294967296.0


# ---- design (fm.m:8-47) ----------------------------------------------------------------------------------------------------------------------------------------
def firls(numtaps, bands, desired):
    """Least-squares linear-phase FIR, type I (numtaps odd), unit weights, in closed form: what Octave's / scipy's firls solve.  bands: edges in units of the Nyquist
    rate, pairs; desired: the amplitude at each edge, linear in between.  A(f) = sum_i c_i cos(pi i f), i = 0..M; the normal equations Q c = r with
        Q[i, j] = 1/2 sum_bands [q(i - j) + q(i + j)],  q(k) = int cos(pi k f) df = f1 sinc(k f1) - f0 sinc(k f0)
        r[i]    = sum_bands int (s f + d0) cos(pi i f) df
    and h[M] = c_0, h[M +- i] = c_i / 2."""
    assert numtaps % 2 == 1
    M = (numtaps - 1) // 2
    bands = np.asarray(bands, np.float64).reshape(-1, 2)
    desired = np.asarray(desired, np.float64).reshape(-1, 2)
    k = np.arange(2 * M + 1, dtype=np.float64)
    q = np.zeros(2 * M + 1)
    r = np.zeros(M + 1)
    i = np.arange(1, M + 1, dtype=np.float64)
    for (f0, f1), (a0, a1) in zip(bands, desired):
        q += f1 * np.sinc(k * f1) - f0 * np.sinc(k * f0)
        s = (a1 - a0) / (f1 - f0)
        d0 = a0 - s * f0
        r[0] += (0.5 * s * f1 * f1 + d0 * f1) - (0.5 * s * f0 * f0 + d0 * f0)
        w = np.pi * i
        r[1:] += ((s * f1 + d0) * np.sin(w * f1) / w + s * np.cos(w * f1) / w ** 2) - ((s * f0 + d0) * np.sin(w * f0) / w + s * np.cos(w * f0) / w ** 2)
    ii, jj = np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing="ij")
    Q = 0.5 * (q[np.abs(ii - jj)] + q[ii + jj])
    c = np.linalg.solve(Q, r)
    return np.concatenate([0.5 * c[:0:-1], c[:1], 0.5 * c[1:]])


def design_bands(Fs, fm_max, fd):
    """(bands of bin, bands of bout, amplitudes): fm.m:41-47"""
    fc1, fc2 = (fd + fm_max) / (Fs / 2), fm_max / (Fs / 2)            # Bfm / 2 = fd + fm_max (fm.m:16)
    return [0, fc1 * (1 - 0.05), fc1 * (1 + 0.05), 1], [0, 0.95 * fc2, 1.05 * fc2, 1], [1, 1, 0.01, 0.01]


def deemph_len(Fs, tc=TC):
    """K: the first power of a = 1 - 1 / (tc Fs) below 2^-30"""
    a, p, K = 1.0 - 1.0 / (tc * Fs), 1.0, 0
    while True:
        K += 1
        p *= a
        if p < 2.0 ** -30:
            return K


def design(Fs, fm_max, fd, ntaps=201, de_emp_tc=0.0):
    """(bin, bout) in float64; de_emp_tc > 0: bout convolved with a^k, k < K (filter(1, prede, .) of fm.m:123-125 cut off below 2^-30)"""
    b_in, b_out, amp = design_bands(Fs, fm_max, fd)
    bin_, bout = firls(ntaps, b_in, amp), firls(ntaps, b_out, amp)
    if de_emp_tc > 0:
        a = 1.0 - 1.0 / (de_emp_tc * Fs)
        bout = np.convolve(bout, a ** np.arange(deemph_len(Fs, de_emp_tc)))
    return bin_, bout


def sigma(CNdB, Fs, fm_max, fd):
    """fm.m:160-162: sqrt(variance), variance = Fs / (CN Bfm)"""
    return np.sqrt(Fs / (10.0 ** (CNdB / 10.0) * 2.0 * (fd + fm_max)))


# ---- modulator ---------------------------------------------------------------------------------------------------------------------------------------------------
def mod_fm_m(mod, Fs, fc, fd):
    """analog_fm_mod (fm.m:74-94) as it stands: float64 accumulate and wrap -> complex128"""
    wc, wd = 2 * np.pi * fc / Fs, 2 * np.pi * fd / Fs
    ph, out = 0.0, np.empty(len(mod), np.complex128)
    for i, m in enumerate(np.asarray(mod, np.float64)):
        ph += wc + wd * m
        ph -= np.floor(ph / (2 * np.pi)) * 2 * np.pi
        out[i] = np.exp(1j * ph)
    return out


def _rint_fma_exact(m, kd, kc):
    """rint(fma(m, kd, kc)) of one element in exact arithmetic: the product and the sum exactly, ONE rounding to double, then round-half-even to an integer"""
    v = float(Fraction(float(m)) * Fraction(kd) + Fraction(kc))       # int / int true division: correctly rounded
    return int(np.rint(v))


def nco_inc(m, Fs, fc, fd):
    """inc[k] = (uint32)(int64) rint(fma((double)m[k], kd, kc)) for float32 m; a sample that is not finite or has |m| > 2^16 counts as 0.  Vectorised in extended
    precision, and exactly (fractions) for every element that comes within 1e-4 of a half-integer, where the rounding of the fused sum could decide."""
    kd, kc = fd / Fs * TWO32, fc / Fs * TWO32
    m = np.asarray(m, np.float32).copy()
    m[~(np.abs(m) <= 65536.0)] = 0.0
    v = m.astype(np.longdouble) * np.longdouble(kd) + np.longdouble(kc)
    r = np.rint(v).astype(np.int64)
    near = np.abs(np.abs(v - np.floor(v)) - 0.5) < 1e-4
    if np.finfo(np.longdouble).nmant < 60:
        near[:] = True
    for i in np.flatnonzero(near):
        r[i] = _rint_fma_exact(m[i], kd, kc)
    return (r & 0xFFFFFFFF).astype(np.uint32)


def nco_phase(m, Fs, fc, fd, ph0=0):
    """ph[i] = ph0 + sum_{k <= i} inc[k] mod 2^32 (inclusive: fm.m:90-92 adds before it takes the exponential)"""
    return ((np.cumsum(nco_inc(m, Fs, fc, fd).astype(np.uint64)) + np.uint64(int(ph0))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def cis(ph):
    """the phasor of a 32-bit phase in float64: the quadrant from the top two bits by swap and negate, the angle (pi / 2) 2^-30 r of the low 30 bits"""
    ph = np.asarray(ph, np.uint32)
    q, r = ph >> np.uint32(30), (ph & np.uint32(0x3FFFFFFF)).astype(np.float64)
    ang = r * (np.pi / 2 / 2.0 ** 30)
    c, s = np.cos(ang), np.sin(ang)
    re = np.choose(q, [c, -s, -c, s]) + 0.0
    im = np.choose(q, [s, c, -s, -c]) + 0.0
    return re + 1j * im


def mod(m, Fs, fc, fd, ph0=0):
    """(tx complex128, ph uint32): the modulator without noise; m float32 (of a complex input the real part)"""
    m = np.asarray(m)
    ph = nco_phase(m.real if np.iscomplexobj(m) else m, Fs, fc, fd, ph0)
    return cis(ph), ph


def mod_noise(seed, B, n, n0=0):
    """the generated unit noise of the modulator -> (g0, g1) float64 [B, n]: counter (p, b, 3, p >> 32), p = (n0 + i) >> 1, words 0-1 for the even sample of the
    pair, words 2-3 for the odd one (tests/noise_ref.py)"""
    k0, k1 = nr._key(seed)
    a = np.uint64(n0) + np.arange(n, dtype=np.uint64)[None, :]
    p = a >> np.uint64(1)
    b = np.arange(B, dtype=np.uint64)[:, None]
    r = nr.philox4x32_10(p & nr.MASK, b, 3, p >> np.uint64(32), k0, k1)
    odd = (a & np.uint64(1)).astype(bool) & np.ones((B, 1), bool)
    ex, ey = nr.gauss_pair(r[0], r[1])
    ox, oy = nr.gauss_pair(r[2], r[3])
    return np.where(odd, ox, ex), np.where(odd, oy, ey)


def add_noise(tx, g0, g1, sig, mode):
    """fm.m:171 (complex: tx + sigma / sqrt 2 (g0 + j g1)) and fm.m:321-324 (real: Re tx + sigma g0), with the float32 scale factors the call uses"""
    if mode == OUT_REAL:
        return (tx.real + float(np.float32(sig)) * g0) + 0j
    s = float(np.float32(sig / np.sqrt(2.0)))
    return tx + s * (g0 + 1j * g1)


# ---- demodulator -------------------------------------------------------------------------------------------------------------------------------------------------
def fcq_of(Fs, fc):
    return int(np.rint(fc / Fs * TWO32)) & 0xFFFFFFFF


def wd_of(Fs, fd):
    """(wd, 1 / wd) as the float32 values the call uses"""
    wd = 2 * np.pi * fd / Fs
    return float(np.float32(wd)), float(np.float32(1.0 / wd))


def causal_fir(b, x):
    """filter(b, 1, x): y[n] = sum_k b[k] x[n - k], zeros in front"""
    return np.convolve(x, np.asarray(b, np.float64))[:len(x)]


def mix(x, Fs, fc, in_base=0):
    """fm.m:104 with the integer phase: x[n] cis(-(fcq n mod 2^32)), n = in_base + g; samples in front of absolute index 0 are zero"""
    n = in_base + np.arange(len(x), dtype=np.int64)
    prod = (np.uint64(fcq_of(Fs, fc)) * (n & 0xFFFFFFFF).astype(np.uint64)) & np.uint64(0xFFFFFFFF)      # (uint64 products wrap: the low 32 bits are what counts)
    ph = ((np.uint64(1 << 32) - prod) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return np.where(n >= 0, np.asarray(x, np.complex128) * cis(ph), 0.0)


def discriminate(bb, Fs, fd, dont_limit=False, bb_before=0.0):
    """fm.m:110-118: angle of bb[n] conj(bb[n - 1]) (bb_before in front of the first sample: 0 at the start of a stream, which gives angle 0), clamped to +-wd
    unless dont_limit, times 1 / wd"""
    wd, inv = wd_of(Fs, fd)
    d = bb * np.conj(np.concatenate([[bb_before], bb[:-1]]))
    a = np.where(d == 0, 0.0, np.arctan2(d.imag, d.real))            # d = 0 gives 0 whatever the signs of its zeros
    if not dont_limit:
        a = np.clip(a, -wd, wd)
    return a * inv, d


def demod(x, Fs, fc, fd, b1, b2, dont_limit=False, in_base=0):
    """analog_fm_demod (fm.m:97-126) of a whole stream that starts at absolute index in_base (zeros in front of it) -> (y float64, bb complex128, d complex128)"""
    bb = causal_fir(b1, mix(x, Fs, fc, in_base))
    a, d = discriminate(bb, Fs, fd, dont_limit)
    return causal_fir(b2, a), bb, d


def stage1_bound(b1, xmax, eps_cis):
    """|bb - bb64| per component: the mix's two roundings and the phasor's error, then N1 fused terms: ((N1 + 2) u + EPS_CIS) sum |b1| max |x|"""
    b1 = np.asarray(b1, np.float64)
    return ((len(b1) + 2) * U + eps_cis) * np.abs(b1).sum() * xmax


def stage2_bound(b2, Fs, fd, eps_atan):
    """|y - y64(device bb)|: (EPS_ATAN + 3 u) / wd sum |b2| for the angle (three roundings ahead of atan2), (N2 + 1) u sum |b2| for the clamp's / the multiply's rounding
    and the N2 fused terms (|a / wd| <= 1 when clamped; with ph_dont_limit |a / wd| <= pi / wd scales the second term)"""
    b2 = np.asarray(b2, np.float64)
    return (eps_atan + 3 * U) / wd_of(Fs, fd)[0] * np.abs(b2).sum() + (len(b2) + 1) * U * np.abs(b2).sum()


# ---- the test-tone measurement of fm.m:180-196 ------------------------------------------------------------------------------------------------------------------
def notch_filter(x, Fs, f=1000.0, beta=0.99):
    """filter([1 -2cos(w) 1], [1 -2 beta cos(w) beta^2], x)"""
    w = 2 * np.pi * f / Fs
    b, a1, a2 = (1.0, -2 * np.cos(w), 1.0), -2 * beta * np.cos(w), beta * beta
    y = np.zeros(len(x) + 2)
    xp = np.concatenate([[0.0, 0.0], x])
    for i in range(len(x)):
        y[i + 2] = b[0] * xp[i + 2] + b[1] * xp[i + 1] + b[2] * xp[i] - a1 * y[i + 1] - a2 * y[i]
    return y[2:]


def tone_snr_dB(rx_out, Fs, f=1000.0, settle=1000):
    """fm.m:180-192: power with and without the test tone -> 10 log10((sinad - nad) / nad)"""
    rx_out = np.asarray(rx_out, np.float64)
    notch = notch_filter(rx_out, Fs, f)
    sinad, nad = np.mean(rx_out[settle:] ** 2), np.mean(notch[settle:] ** 2)
    return 10 * np.log10((sinad - nad) / nad)


def snr_theory_dB(CNdB, fm_max, fd):
    """fm.m:196 (the Gfm of bbfm.py:80): C/N + 10 log10(3 m^2 (m + 1)), m = fd / fm_max"""
    m = fd / fm_max
    return CNdB + 10 * np.log10(3 * m * m * (m + 1))
