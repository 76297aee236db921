"""Float64 references, ctypes records and checkers for the unit tests of the transmit, channel and row kernels (tests/test_tx_units_gpu.py on the device;
tests/test_tx_units_host.py pins these references to the reference project's recordings and proves that every checker can fail).  numpy only; holds no
fixtures.  Rows, the fragment codec, pack_f32 and U come from tests/kernel_ref.py, the records and the declared library from tests/dev_abi.py.

Operands
--------
Every reference takes the float32 words the kernel reads (latents, G, noise, the tables of rd_tables_fill: Winv, P, pilot_gain, the EOO frame) as exact
numbers and works in float64 / complex128; its error (2^-53 per operation) is ignored against the float32 bounds below.  A complex sample is compared by the
MAGNITUDE of the difference; a bound stated per component is multiplied by sqrt 2 (SQ2).  u = U = 2^-24 is the unit roundoff of float32, gamma_n = n u / (1 - n u).
The kernels are compiled with contraction allowed, so a product followed by an addition is one rounding or two: every bound below counts two.

Bounds (derived, none fitted to the code under test)
-----------------------------------------------------
IDFT (k_ofdm_mod, k_ofdm_mod_mp, k_eoo_build).  Each component of a sample is a chain of 60 dependent float32 multiply-adds over the 30 carriers,
x.re = sum_c s_c.re w_c.re - s_c.im w_c.im.  The forward bound of a length-60 dot product in any order (Higham, Accuracy and Stability of Numerical Algorithms,
section 3.1) is gamma_60 sum |terms|, and |s.re w.re| + |s.im w.im| <= |s| |w| (Cauchy-Schwarz):  |dx| <= SQ2 gamma_60 S,  S = sum_c |sym_c| |Winv_c|.
The pilot symbol's P pilot_gain is itself rounded to float32 before the sum: u S more.  The EOO data symbols are scaled after the sum: u |x| more.

Limiter.  L(x) = tanh(|x|) x / |x| is 1-Lipschitz on the complex plane (radial derivative 1 - tanh^2 <= 1, tangential tanh(m) / m <= 1), so the error of its
argument passes through unamplified; its own evaluation (hardware square root, exp2, reciprocal, a subtraction 1 - e^{-2m} that cancels at small m) has no
a-priori figure in this project and is MEASURED, as kernel_ref.EPS_* are: EPS_PA_LIMIT is the largest |pa_limit(x) - L(x)| over the sweep of 2^16 magnitudes
2^-20 .. 2^5 (test_tx_units_gpu.py::test_limiter_sweep, x the float32 argument the kernel formed) on an MI355X, rounded up to the next power of two.  It may not
exceed 2^-20 (four times gate_tanh's 2^-22: the same exp2 / rcp units, plus the square root and the cancelling subtraction).

Complex product a b.  Each component is two products and an addition: gamma_2 (|a.re b.re| + |a.im b.im|) + u |result| <= 3 u |a| |b|; as a magnitude
3 SQ2 u |a| |b| =: CMUL |a| |b|.  Two-path sample  mp = tx G1 + tx' G2:  CMUL (|tx| |G1| + |tx'| |G2|) + SQ2 u |mp|  (two products and a sum).

Part sums (k_ofdm_mod_mp, k_chan_power).  Terms hypotf(x)^2 formed in float32, added in float64 (2^-53 per addition: ignored).  All terms are positive, so the
relative error of a sum is at most that of a term: 4 u (hypotf within 1.5 u, squared: 3 u, and the rounding of the square).

Gain  powf(float(p0 / n) / float(p1 / n), 0.5f):  (rel p0 + rel p1 + 3 u) / 2 for the two casts and the division under the square root, + 2 u for powf
(1 ulp).  rel p0 = 4 u; rel p1 = 4 u + sum_i 2 |mp_i| d_i / p1 with d_i the two-path bound above when k_chan_power forms mp itself, 0 when k_ofdm_mod_mp left
mp and its sums (then the sums ARE the operands, and rel p0 = rel p1 = 0).

Phasor.  The phase is a double (chan_phase_acc: float32 omega times i + 1, or the closed form with a drift), rounded to float32 and handed to sincosf.  The
reference forms the same double, rounds it the same way and takes the exact sine and cosine of that float32 number, so what is left is sincosf's own error,
1 ulp of a value <= 1 per component: PHASOR = SQ2 2 u.  Where the double lies within 2^-50 relative of a float32 rounding boundary (a contracted multiply-add on
the device can land on the other side) the neighbouring float32 phase is admitted: phase32 returns that slack, 0 for all but one argument in 2^26.

Channel sample, in the kernel's order: two-path (or mp) sample, x gain (u), x phasor (PHASOR + CMUL), + sigma noise (product and sum: 2 u of both terms, SQ2 as a
magnitude), + sine (its phasor to 2 u per component, product and sum), x rx_gain (u).  chan_ref carries the bound through these steps next to the value.

Generator (k_multipath_gen).  Double arithmetic throughout and one rounding to float32: u |component|, plus DBL = 2^-36 of the stream's largest |G| for the
double part (2^17 x 2^-53: 2^5 for the 101-term FIR sums and the tree over n_out / 256 partial sums per thread, and a cancellation of up to 2^12 in
E |g|^2 - |E g|^2 -- two samples a quarter of a low-rate step apart vary little -- which mpgen_ref asserts for its operands).  k_multipath_h: float32; phasor argument formed in float32 as the kernel forms it (-2 pi c, times d Rs); one phasor, one
complex product, one sum; the magnitude adds 4 u |H| (squares, sum, square root)."""
import ctypes as C

import numpy as np

from dev_abi import ChanArgs, Tables  # noqa: F401  (the records of rade_dev.h, stated in tests/dev_abi.py)
from kernel_ref import U

SQ2 = np.sqrt(2.0)
G60 = 60 * U / (1 - 60 * U)
CMUL = 3 * SQ2 * U
PHASOR = 2 * SQ2 * U
DBL = 2.0 ** -36
EPS_PA_LIMIT = 2.0 ** -21      # pa_limit (sqrt / exp2 / rcp units), every kernel that synthesises a transmit sample: measured 2.629e-07 (at |x| = 7.2483)

M, NCP, SYM, NC, NS, NMF, NEOO, ZMF = 160, 32, 192, 30, 4, 960, 1152, 240


class Tab:
    """what the references read of rd_tables_fill's tables: the float32 words as float64 / complex128"""

    def __init__(self, L):
        T = Tables()
        L.rd_tables_fill(C.byref(T))
        self.Winv = np.ctypeslib.as_array(T.Winv).view(np.complex64).reshape(NC, M).astype(np.complex128)
        self.P = np.ctypeslib.as_array(T.P).astype(np.float64)
        self.pilot_gain = float(T.pilot_gain)
        self.eoo32 = np.ctypeslib.as_array(T.eoo).view(np.complex64).copy()
        self.eoo = self.eoo32.astype(np.complex128)


def c128(x):
    """complex64 words (or their float32 pairs) as complex128"""
    x = np.asarray(x)
    if x.dtype == np.float32:
        x = np.ascontiguousarray(x).view(np.complex64)
    return x.astype(np.complex128)


# ---- modulator and EOO ---------------------------------------------------------------------------------------------------------------------------------------------
def limiter(x):
    """tanh(|x|) x / |x|, 0 at |x| == 0"""
    m = np.abs(x)
    return np.where(m == 0, 0, np.tanh(m) / np.where(m == 0, 1, m)) * x


def with_prefix(body):
    """[..][160] symbol bodies -> [..][192]: the 32-sample prefix is a copy of samples 128..159"""
    return np.concatenate([body[..., M - NCP:], body], axis=-1)


def mod_ref(tab, z, linear):
    """z [B][3 n_mf][80] float32 -> (tx complex128 [B][960 n_mf], bound [B][960 n_mf]).  A frame = the pilot symbol P pilot_gain (gain 1 when linear) and four
    data symbols, carrier c of data symbol t = (zf[2 (30 t + c)], zf[2 (30 t + c) + 1]) of the frame's 240 latents; sym @ Winv; the limiter unless linear."""
    z = np.asarray(z, np.float32)
    B = z.shape[0]; n_mf = z.shape[1] * z.shape[2] // ZMF
    data = c128(z.reshape(B, n_mf, NS, NC, 2)).reshape(B, n_mf, NS, NC)
    pg = 1.0 if linear else tab.pilot_gain
    sym = np.concatenate([np.broadcast_to(tab.P * pg + 0j, (B, n_mf, 1, NC)), data], axis=2)            # [B][n_mf][5][30]
    x = sym @ tab.Winv
    S = np.abs(sym) @ np.abs(tab.Winv)
    rel = np.full(NS + 1, G60); rel[0] += 0.0 if linear else U                                             # the pilot row's own rounding
    bound = SQ2 * rel[None, None, :, None] * S
    if not linear:
        x = limiter(x); bound = bound + EPS_PA_LIMIT
    return with_prefix(x).reshape(B, n_mf * NMF), with_prefix(bound).reshape(B, n_mf * NMF)


def eoo_ref(tab, bits):
    """bits [B][180] float32 -> (eoo complex128 [B][1152], bound); the table everywhere (bound 0: a bit copy) but symbols 2..4 = limiter(pilot_gain (bits @ Winv))"""
    bits = np.asarray(bits, np.float32)
    B = bits.shape[0]
    sym = c128(bits.reshape(B, 3, NC, 2)).reshape(B, 3, NC)
    raw = sym @ tab.Winv
    x = limiter(tab.pilot_gain * raw)
    bnd = SQ2 * tab.pilot_gain * (G60 * (np.abs(sym) @ np.abs(tab.Winv)) + U * np.abs(raw)) + EPS_PA_LIMIT
    out = np.broadcast_to(tab.eoo, (B, NEOO)).copy(); bound = np.zeros((B, NEOO))
    out[:, 2 * SYM:5 * SYM] = with_prefix(x).reshape(B, 3 * SYM); bound[:, 2 * SYM:5 * SYM] = with_prefix(bnd).reshape(B, 3 * SYM)
    return out, bound


# ---- two-path model --------------------------------------------------------------------------------------------------------------------------------------------------
def mp_ref(tx, G, delay=16):
    """tx [B][n] complex, G [B][n][2] complex -> (mp, bound):  mp[i] = tx[i] G1[i] + (i >= 16) tx[i - 16] G2[i - 16]"""
    tx, G = np.asarray(tx, np.complex128), np.asarray(G, np.complex128)
    mp = tx * G[:, :, 0]; cond = np.abs(tx) * np.abs(G[:, :, 0])
    n = tx.shape[1]
    if n > delay:
        mp[:, delay:] += tx[:, :n - delay] * G[:, :n - delay, 1]; cond[:, delay:] += np.abs(tx[:, :n - delay]) * np.abs(G[:, :n - delay, 1])
    return mp, CMUL * cond + SQ2 * U * np.abs(mp)


def part_ref(tx, mp):
    """per-frame sums [B][n_mf][2] of |tx|^2 and |mp|^2 (n a multiple of 960)"""
    B, n = tx.shape
    return np.stack([(np.abs(np.asarray(v, np.complex128)) ** 2).reshape(B, n // NMF, NMF).sum(2) for v in (tx, mp)], axis=2)


# ---- channel -----------------------------------------------------------------------------------------------------------------------------------------------------------
def phase32(phi):
    """a double phase as the float32 the kernel hands to sincosf -> (that number as float64, slack): slack = the distance to the neighbouring float32 where phi
    is within 2^-50 relative of the rounding boundary, else 0"""
    phi = np.asarray(phi, np.float64)
    lo, hi = (phi * (1 - 2.0 ** -50)).astype(np.float32).astype(np.float64), (phi * (1 + 2.0 ** -50)).astype(np.float32).astype(np.float64)
    return phi.astype(np.float32).astype(np.float64), np.abs(hi - lo)


def chan_phase(i, f0, df_dt):
    """chan_phase_acc of rade_devutil.h for sample indices i: the double the kernel forms"""
    i = np.asarray(i, np.float64); f0, df_dt = np.float32(f0), np.float32(df_dt)
    if df_dt == 0:
        om = ((f0 * np.float32(2.0)) * np.float32(np.pi)) / np.float32(8000.0)               # float32 arithmetic
        return (i + 1) * np.float64(om)
    n = i + 1
    return (2.0 * np.pi / 8000.0) * (n * np.float64(f0) + (np.float64(df_dt) / 8000.0) * 0.5 * i * n)


def chan_ref(tx, noise, n_pre=0, n_post=0, eoo=None, G=None, mp=None, part=None, sigma=0.0, freq_offset=0.0, df_dt=0.0, ps=None,
             sine_amp=0.0, sine_freq=0.0, rx_gain=1.0):
    """All of rd_launch_channel with an explicit noise tensor: tx [B][n_sig], noise [B][n_total] complex64, eoo [B][1152] or None, G [B][n_sig][2] or None, mp /
    part = what k_ofdm_mod_mp left ([B][n_sig], [B][n_sig / 960][2]), ps [3][B] = sigma, freq_offset, df_dt per stream in place of the scalars.
    Returns (rx complex128 [B][n_total], bound [B][n_total], final phasor [B]).
    The signal is not rotated at all when freq_offset == 0, whatever df_dt (radae.py:546); the EOO frame restarts the phase at its sample 0, times the signal's
    final phasor (1 when the signal was not rotated), and IS rotated by the drift alone when freq_offset == 0 (inference.py:269-274 has no such condition);
    neither gain nor two-path model on it.  n_pre and n_post are noise only."""
    tx = c128(tx); B, n_sig = tx.shape
    noise = c128(noise)
    n_eoo = NEOO if eoo is not None else 0
    n_total = n_pre + n_sig + n_eoo + n_post
    assert noise.shape == (B, n_total)
    val = np.zeros((B, n_total), np.complex128); err = np.zeros((B, n_total)); fin = np.ones(B, np.complex128)
    for b in range(B):
        sg, f0, dd = (np.float32(ps[0][b]), np.float32(ps[1][b]), np.float32(ps[2][b])) if ps is not None else (np.float32(sigma), np.float32(freq_offset), np.float32(df_dt))
        # the two-path sample and the gain
        if mp is not None:
            m = c128(mp[b:b + 1])[0]; dm = np.zeros(n_sig); p0, p1 = np.asarray(part[b], np.float64).sum(0); rel0 = rel1 = 0.0
        else:
            if G is not None:
                m, dm = (v[0] for v in mp_ref(tx[b:b + 1], c128(G[b:b + 1])))
            else:
                m, dm = tx[b], np.zeros(n_sig)
            p0, p1 = (np.abs(tx[b]) ** 2).sum(), (np.abs(m) ** 2).sum(); rel0 = 4 * U; rel1 = 4 * U + (2 * np.abs(m) * dm).sum() / p1 if p1 > 0 else 0.0
        gain, grel = (np.sqrt(p0 / p1), (rel0 + rel1 + 3 * U) / 2 + 2 * U) if G is not None else (1.0, 0.0)
        v = m * gain; e = dm * gain + np.abs(v) * (grel + U); fslack = 0.0
        if f0 != 0:
            ph, slack = phase32(chan_phase(np.arange(n_sig), f0, dd))
            v = v * np.exp(1j * ph); e = e + np.abs(v) * (PHASOR + CMUL + slack)
            if n_sig > 0:
                fin[b] = np.exp(1j * ph[-1]); fslack = slack[-1]
        val[b, n_pre:n_pre + n_sig] = v; err[b, n_pre:n_pre + n_sig] = e
        if n_eoo:
            ph, slack = phase32(chan_phase(np.arange(NEOO), f0, dd))
            ve = c128(eoo[b:b + 1])[0] * np.exp(1j * ph) * fin[b]                                 # two phasors, two products
            val[b, n_pre + n_sig:n_pre + n_sig + NEOO] = ve
            err[b, n_pre + n_sig:n_pre + n_sig + NEOO] = np.abs(ve) * (2 * PHASOR + 2 * CMUL + slack + fslack)
        nz = np.float64(sg) * noise[b]
        err[b] += SQ2 * 2 * U * (np.abs(val[b]) + np.abs(nz)); val[b] += nz
        if sine_amp != 0:
            j = np.arange(n_total, dtype=np.float64)
            cyc = j * np.float64(np.float32(sine_freq)) / 8000.0
            ph, slack = phase32(6.283185307179586 * (cyc - np.floor(cyc)))
            s = np.float64(np.float32(sine_amp)) * np.exp(1j * ph)
            err[b] += np.abs(s) * (PHASOR + slack + SQ2 * U) + SQ2 * U * np.abs(val[b] + s); val[b] += s
        g = np.float64(np.float32(rx_gain))
        val[b] *= g; err[b] = err[b] * abs(g) + SQ2 * U * np.abs(val[b])
    return val, err, fin


# ---- multipath generator -------------------------------------------------------------------------------------------------------------------------------------------------
def n_low_of(ratio, n_out):
    return max((n_out + ratio - 1) // ratio, 2)


def mpgen_ref(noise_low, taps, ratio, n_out):
    """noise_low [B][2][n_low + n_taps] complex, taps [n_taps] -> (G complex128 [B][n_out][2], bound per COMPONENT [B][n_out][2]): per path
    y = np.convolve(x, taps)[n_taps:], linear interpolation at n / ratio with i0 = min(int(pos), n_low - 2) (the last segment extrapolates), hf_gain =
    1 / sqrt(population variance of path 1 + of path 2)"""
    x = np.asarray(noise_low, np.complex128); taps = np.asarray(taps, np.float64)
    B = x.shape[0]; n_taps = len(taps); n_low = n_low_of(ratio, n_out)
    assert x.shape == (B, 2, n_low + n_taps)
    pos = np.arange(n_out) / ratio
    i0 = np.minimum(pos.astype(np.int64), n_low - 2); fr = pos - i0
    G = np.empty((B, n_out, 2), np.complex128)
    for b in range(B):
        g = []
        for p in range(2):
            y = np.convolve(x[b, p], taps)[n_taps:][:n_low]
            g.append(y[i0] + (y[i0 + 1] - y[i0]) * fr)
        var = np.var(g[0]) + np.var(g[1])
        assert sum(np.mean(np.abs(v) ** 2) for v in g) < 2.0 ** 12 * var, "the variance cancels by more than DBL allows for"
        G[b] = np.stack(g, axis=1) / np.sqrt(var)
    comp = np.stack([G.real, G.imag], axis=-1)
    return G, U * np.abs(comp) + DBL * np.abs(G).max(axis=(1, 2))[:, None, None, None]


def mph_ref(G, M_, n_sym, Nc, dRs, want_complex, f32_phase=True):
    """G [B][n_g][2] complex -> (H [B][n_sym][Nc] complex128 or its magnitude, bound): H[t][c] = G1[t M] + G2[t M] exp(-2 pi j c d Rs); f32_phase: the phase as the
    kernel forms it in float32"""
    G = np.asarray(G, np.complex128)
    g1, g2 = G[:, :(n_sym - 1) * M_ + 1:M_, 0][:, :, None], G[:, :(n_sym - 1) * M_ + 1:M_, 1][:, :, None]
    c = np.arange(Nc)
    ph = ((np.float32(-6.283185307179586) * c.astype(np.float32)) * np.float32(dRs)).astype(np.float64) if f32_phase else -2 * np.pi * c * dRs
    H = g1 + g2 * np.exp(1j * ph)[None, None, :]
    e = np.broadcast_to((PHASOR + CMUL) * np.abs(g2) + SQ2 * U * (np.abs(g1) + np.abs(g2)), H.shape)
    return (H, e) if want_complex else (np.abs(H), e + 4 * U * np.abs(H))


# ---- rows ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def pack_ref(features):
    """features [B][4 T][36] -> [B][T][96]: 4 x (20 features, -1), zero pad"""
    f = np.asarray(features, np.float32); B, T = f.shape[0], f.shape[1] // 4
    out = np.zeros((B, T, 96), np.float32)
    for fr in range(4):
        out[:, :, 21 * fr:21 * fr + 20] = f[:, fr::4, :20]; out[:, :, 21 * fr + 20] = -1
    return out


def pad_ref(src, Kpad):
    src = np.asarray(src, np.float32)
    out = np.zeros((src.shape[0], Kpad), np.float32); out[:, :src.shape[1]] = src
    return out


def carry_ref(x, nhist, T, n_rows=None):
    """x [B][nhist + Tcap][W]: rows [Tb, Tb + nhist) -> rows [0, nhist) of every stream with Tb = n_rows[b] (or T) > 0, all read before any is written"""
    out = np.array(x, copy=True)
    for b in range(out.shape[0]):
        Tb = T if n_rows is None else int(n_rows[b])
        if Tb > 0:
            out[b, :nhist] = x[b, Tb:Tb + nhist]
    return out


# ---- checkers: the GPU tests and the host self-tests call the same ones ----------------------------------------------------------------------------------------------------
def _where(idx, names):
    return ", ".join(f"{n} {int(i)}" for n, i in zip(names, idx))


def check_close(got, want, bound, what, names=("stream", "sample"), split=None):
    """|got - want| <= bound for every element (a NaN fails); names the first offender.  split = (frame length, name): the last index is reported as frame and
    sample within it."""
    got = np.asarray(got); err = np.abs(got.astype(np.complex128 if np.iscomplexobj(got) else np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    bad = ~(err <= bound)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))) if err.size else 0.0
    if bad.any():
        idx = tuple(np.argwhere(bad)[0])
        pos, nm = list(idx), list(names)
        if split:
            pos = pos[:-1] + [idx[-1] // split[0], idx[-1] % split[0]]; nm = nm[:-1] + [split[1], nm[-1]]
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound, the first at {_where(pos, nm)}: got {got[idx]!r}, reference {want[idx]!r}, "
                             f"error {err[idx]:.4g}, bound {bound[idx]:.4g}")
    return ratio


def check_bits(got, want, what, names=("stream", "row", "column")):
    """bit equality of float32 (or complex64) arrays; names the first offender"""
    g, w = (np.ascontiguousarray(v).view(np.uint32) for v in (got, want))
    bad = g != w
    if bad.any():
        idx = tuple(np.argwhere(bad)[0])
        fg, fw = (np.ascontiguousarray(v).view(np.float32) for v in (got, want))
        raise AssertionError(f"{what}: {int(bad.sum())} words differ, the first at {_where(idx, names)}: got {fg[idx]!r}, reference {fw[idx]!r}")


def check_prefix(got, what, n_sym=5):
    """every symbol's 32-sample prefix is bit-equal to its samples 128..159: got complex64 [B][192 k]"""
    g = np.ascontiguousarray(got, np.complex64).view(np.uint32).reshape(got.shape[0], -1, SYM, 2)
    bad = g[:, :, :NCP] != g[:, :, M:]
    if bad.any():
        b, s, k, _ = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: prefix differs from samples 128..159 at stream {b}, frame {s // n_sym}, symbol {s % n_sym}, sample {k}: "
                             f"{got[b, s * SYM + k]!r} against {got[b, s * SYM + M + k]!r}")


def check_mod(got, ref, what, prefix=True):
    """k_ofdm_mod / k_ofdm_mod_mp's tx against mod_ref's (want, bound): every sample within its bound, every prefix a bit copy.  Returns the largest error / bound."""
    r = check_close(got, ref[0], ref[1], what, ("stream", "sample"), (NMF, "frame"))
    if prefix:
        check_prefix(got, what)
    return r


def check_eoo(got, ref, what):
    """k_eoo_build against eoo_ref: the table's samples bit for bit (bound 0), the data symbols within the bound, their prefixes bit copies"""
    r = check_close(got, ref[0], ref[1], what, ("stream", "sample"), (SYM, "symbol"))
    check_prefix(np.asarray(got)[:, 2 * SYM:5 * SYM], what + " data symbols", n_sym=3)
    return r


def check_mp(got_mp, got_part, tx, G, what):
    """k_ofdm_mod_mp's mp and part against the two-path model of the kernel's OWN tx: mp within two products and a sum, part within 4 u relative of the float64
    sums of |tx|^2 and of the kernel's own |mp|^2"""
    want, bound = mp_ref(c128(tx), c128(G))
    r = check_close(got_mp, want, bound, what + " mp", ("stream", "sample"), (NMF, "frame"))
    wp = part_ref(c128(tx), c128(got_mp))
    r2 = check_close(got_part, wp, 4 * U * wp, what + " part", ("stream", "frame", "sum"))
    return r, r2


def check_chan(got, ref, what):
    """rd_launch_channel's rx [B][n_total] against chan_ref's (value, bound, ..); the sample index is reported from the start of rx"""
    return check_close(got, ref[0], ref[1], what, ("stream", "sample"))


def check_mpgen(got, ref, what):
    """k_multipath_gen's G [B][n_out][2] complex64 against mpgen_ref, per component"""
    g = np.ascontiguousarray(got, np.complex64).view(np.float32).reshape(got.shape + (2,))
    want = np.stack([ref[0].real, ref[0].imag], axis=-1)
    return check_close(g, want, ref[1], what, ("stream", "sample", "path", "component"))


def check_mph(got, ref, what):
    return check_close(got, ref[0], ref[1], what, ("stream", "symbol", "carrier"))


def check_rows(rows, words, want, what):
    """a row kernel's output in a sentinel buffer: nothing written outside the documented rows, the rows bit-equal to want [B][lead + T][width]"""
    rows.check_outside(words, what)
    check_bits(rows.view(words), np.asarray(want, np.float32).reshape(rows.B, rows.lead + rows.T, rows.width), what)
