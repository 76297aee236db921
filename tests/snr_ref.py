"""Float64 restatement of the reference's est_snr.py (:45-124, :163-180), of receiver_one.est_pilots (dsp.py:400-435) and of update_snr_est (dsp.py:438-456), with the
counter mapping of the generated noise and the error bound of the device's six sums (include/rade_batch.h: rade_batch_snr_trials; radae_amd/csrc/rade_snr.hip).
numpy only, holds no fixtures.  The tests hold the library and the kernel to this file; run as a script with the reference's directory as its argument, this file
checks itself against the reference live (receiver_one.est_pilots on Nw = 8 windows, and Pmat, within 5e-6 of the largest value).

What counts as exact here: the constants as the reference itself holds them -- w[c] and the angles w[c] a are float32 (radae.py:172-174 is float32 tensor arithmetic,
dsp.py:408 multiplies in complex64), the entries of the matrix A are complex64 values, P = float32(sqrt 2) x Barker, pilot_gain and the products pilot_gain P[c]
are float32 (est_snr.py:49 forms them in complex64).  Everything behind these constants is float64."""
import sys

import numpy as np

import noise_ref as nr

NC, NS, FS, M_SYM, NCP = 30, 4, 8000, 160, 32
U = 2.0 ** -24
A_DELAY = 20.0                                                                    # a = 0.0025 Fs (dsp.py:407, :428)
BARKER13 = (1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1)
W32 = (np.float32(2.0 * np.pi) * (15 + np.arange(NC)).astype(np.float32)) / np.float32(160.0)      # radae.py:172-174
ANG = -(W32 * np.float32(A_DELAY)).astype(np.float64)                             # -(w a), the product in float32
P = float(np.float32(np.sqrt(2.0))) * np.array([BARKER13[c % 13] for c in range(NC)], np.float64)
PG = float(np.float32(10.0 ** (-2.0 / 20.0) * 160.0 / np.sqrt(30.0)))            # radae.py:196-199
PGP = (np.float32(PG) * P.astype(np.float32)).astype(np.float64)                  # pilot_gain P[c], one float32 product
CMID = np.clip(np.arange(NC), 1, NC - 2)
ROT = np.exp(1j * ANG)                                                            # e^{-j w[c] a}
MISTAKES = ("conj", "wrap", "sign", "norot")                                      # the planted mistakes of est_pilots / the phase correction; "words": gen_noise
FIELDS = ("S1", "S1_sig", "S1_cross", "S1_noise", "S2_genie", "S2_est")


def pmat(conj=False):
    """Pmat[c] = inv(A^T A) A^T, A = [[1, e^{-j w[c_mid - 1 + k] a}]] k = 0..2, plain transpose (dsp.py:400-412) -> complex128 [30, 2, 3].  The entries of A are the
    complex64 values the reference holds.  conj: the conjugate transpose, a planted mistake."""
    E = np.cos(ANG).astype(np.float32).astype(np.float64) + 1j * np.sin(ANG).astype(np.float32).astype(np.float64)
    out = np.zeros((NC, 2, 3), np.complex128)
    for c in range(NC):
        cm = CMID[c]
        Am = np.stack([np.ones(3, np.complex128), E[cm - 1:cm + 2]], axis=1)
        At = Am.conj().T if conj else Am.T
        out[c] = np.linalg.inv(At @ Am) @ At
    return out


PMAT = pmat()


def est_pilots(x, mistake=None):
    """receiver_one.est_pilots (dsp.py:418-435) on pilot rows x [rows, 30] -> complex128 [rows, 30]"""
    x = np.asarray(x, np.complex128)
    Pm = pmat(conj=True) if mistake == "conj" else PMAT
    q = x / P
    r = np.empty_like(x)
    for c in range(NC):
        cm = c if mistake == "wrap" else CMID[c]
        g = q[:, [(cm - 1) % NC, cm, (cm + 1) % NC]] @ Pm[c].T
        r[:, c] = g[:, 0] + (g[:, 1] if mistake == "norot" else g[:, 1] * ROT[c])
    return r


def elements(h, n, sigma, mistake=None):
    """(s, n sigma, x, r, e) of pilot rows: h [rows, 30] complex or None (h = 1), n [rows, 30] the unit noise, sigma the noise per component"""
    n = np.asarray(n, np.complex128)
    h = np.ones_like(n) if h is None else np.asarray(h, np.complex128)
    s = h * PGP
    nn = float(sigma) * n
    x = s + nn
    r = est_pilots(x, mistake)
    e = (x * np.exp((1j if mistake == "sign" else -1j) * np.angle(r))).imag      # np.angle(0) = 0
    return s, nn, x, r, e


def trial_sums(h, n, sigma, Nw, mistake=None):
    """the six sums of every window of Nw rows (est_snr.py:63-105) -> float64 [rows // Nw, 6] in the order of FIELDS"""
    s, nn, x, _, e = elements(h, n, sigma, mistake)
    t = np.stack([np.abs(x) ** 2, np.abs(s) ** 2, 2.0 * (s * nn).real, np.abs(nn) ** 2, ((np.abs(s / PGP) * PGP) + nn).imag ** 2, e ** 2], axis=-1)
    return t.reshape(-1, Nw * NC, 6).sum(axis=1)


def bounds(h, n, sigma, Nw, dg=0.0):
    """The bound on each of the six sums of every window -> float64 [rows // Nw, 6], counted from the kernel's roundings as include/rade_batch.h derives it (u = 2^-24;
    dg: how far each component of the unit noise the kernel used may lie from n, noise_ref.EPS for generated draws).  Per element, in modulus:
        e_s = 2 u |s|                  pilot_gain P one rounding, h times it another
        e_n = u |n| + sqrt 2 sigma dg
        e_x = e_s + e_n + u |x|        the sum's own rounding
        e_r = u sum_j (10 |Pmat_0j| + 14 |Pmat_1j|) |q_j| + sum_j (|Pmat_0j| + |Pmat_1j|) e_x[j] / |P_j|
              table entry u, quotient 3 u (covers a hardware reciprocal), complex product 3 u, two sums 2 u: 9 u along g_0; g_1 then meets e^{-j w a} (u + 3 u); the last sum u
        e_e = e_x + |x| (pi / 2) e_r / |r| + 10 u |x|       where e_r < |r|, else 2 |x| (1 + 10 u) + e_x: nothing is claimed about the angle of an r inside its own error
              |r|^2 2 u, root u + 2 u (a hardware square root), reciprocal 3 u, the phasor's products u: modulus 7 u, angle u; the final products and sum 2 u
    and a square-and-add is two roundings.  Each sum's bound is 1.01 times the first-order total."""
    s, nn, x, r, e = elements(h, n, sigma)
    a_s, a_n, a_x, a_r = np.abs(s), np.abs(nn), np.abs(x), np.abs(r)
    e_s = 2 * U * a_s
    e_n = U * a_n + np.sqrt(2.0) * float(sigma) * dg
    e_ny = U * np.abs(nn.imag) + float(sigma) * dg
    e_x = e_s + e_n + U * a_x
    aq = a_x / np.abs(P)
    e_r = np.zeros_like(a_x)
    for c in range(NC):
        cm = CMID[c]
        for j in range(3):
            w0, w1 = abs(PMAT[c, 0, j]), abs(PMAT[c, 1, j])
            e_r[:, c] += U * (10 * w0 + 14 * w1) * aq[:, cm - 1 + j] + (w0 + w1) * e_x[:, cm - 1 + j] / abs(P[cm - 1 + j])
    with np.errstate(divide="ignore", invalid="ignore"):
        turn = np.where(e_r < a_r, a_x * (np.pi / 2) * e_r / a_r, np.inf)
    e_e = np.minimum(e_x + turn + 10 * U * a_x, 2 * a_x * (1 + 10 * U) + e_x)
    e_e = np.where((a_r == 0) & (e_r == 0), e_x, e_e)                              # every x of the row's neighbourhood is exactly 0: r = 0 on both sides, angle 0
    b = np.stack([2 * U * a_x ** 2 + 2 * a_x * e_x + e_x ** 2,
                  6 * U * a_s ** 2,
                  2 * (2 * U * a_s * a_n + e_s * a_n + e_n * a_s + e_s * e_n),
                  2 * U * a_n ** 2 + 2 * a_n * e_n + e_n ** 2,
                  U * nn.imag ** 2 + 2 * np.abs(nn.imag) * e_ny + e_ny ** 2,
                  U * e ** 2 + 2 * np.abs(e) * e_e + e_e ** 2], axis=-1)
    return 1.01 * b.reshape(-1, Nw * NC, 6).sum(axis=1)


# ---- the script's formulas behind the sums ----------------------------------------------------------------------------------------------------------------------
def sigma(snrdB):
    """est_snr.py:57-59: sqrt(Es / snr) / sqrt 2, Es = sum (pg P)^2 / Nc"""
    Es = np.sum(PGP ** 2) / NC
    return float(np.sqrt(Es / 10.0 ** (snrdB / 10.0)) / 2 ** 0.5)


def _snr_est(S1, S2):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.float64(S1) / (2 * np.float64(S2)) - 1
    return 0.1 if v <= 0 else v


def finish(sums, eq_ls=False, c=0.0, m=1.0):
    """est_snr.py:96-122 over one window's six sums -> (snrdB_genie, snrdB_est, NdB_genie, NdB_est)"""
    S1, S1_sig, _, S1_noise, S2_genie, S2_est = (np.float64(v) for v in sums)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (10 * np.log10(S1_sig / S1_noise), (10 * np.log10(_snr_est(S1, S2_est if eq_ls else S2_genie)) - c) / m, 10 * np.log10(2 * S2_genie),
                10 * np.log10(2 * S2_est))


def fit(x, y):
    """est_snr.py:178 -> (m, c)"""
    z = np.polyfit(np.asarray(x, np.float64), np.asarray(y, np.float64), 1)
    return float(z[0]), float(z[1])


def track(S1, S2_est, c=2.513, m=0.8070, state=0.0):
    """dsp.py:438-456 over the sums of windows of Nw = 1 in turn -> the smoothed 3 kHz figure after each frame"""
    out = []
    for a, b in zip(S1, S2_est):
        snrdB_est = (10 * np.log10(_snr_est(a, b + 1e-12)) - c) / m
        Rs = FS / M_SYM
        snrdB_3k = snrdB_est + 10 * np.log10(Rs * NC / 3000) + 10 * np.log10((M_SYM + NCP) / M_SYM)
        state = 0.9 * state + 0.1 * snrdB_3k
        out.append(state)
    return np.array(out, np.float64)


def finish_bounds(sums, bnd, eq_ls=False, m=1.0):
    """|d| of the four outputs of finish() when every sum may move by its bound: d log10(v) <= dv / ((v - dv) ln 10); for snr_est the interval of S1 / (2 S2) - 1 over
    S1 +- b, S2 -+ b.  Infinite where a bound reaches its sum or the interval of snr_est reaches the clamp at 0 (nothing is pinned there)."""
    S1, S1_sig, _, S1_noise, S2_genie, S2_est = (float(v) for v in sums)
    b1, bs, _, bn, bg, be = (float(v) for v in bnd)
    k = 10 / np.log(10)

    def dlog(v, dv):
        return k * dv / (v - dv) if v > dv else np.inf
    S2, b2 = (S2_est, be) if eq_ls else (S2_genie, bg)
    if S2 <= b2:
        d_est = np.inf
    else:
        lo, v, hi = (S1 - b1) / (2 * (S2 + b2)) - 1, S1 / (2 * S2) - 1, (S1 + b1) / (2 * (S2 - b2)) - 1
        d_est = 0.0 if hi <= 0 else (np.inf if lo <= 0 else max(10 * np.log10(hi / v), 10 * np.log10(v / lo)) / abs(m))
    return dlog(S1_sig, bs) + dlog(S1_noise, bn), d_est, dlog(S2_genie, bg), dlog(S2_est, be)


def fit_bounds(x, y, bx, by):
    """(|dm|, |dc|) of fit(x, y) when x_i may move by bx_i and y_i by by_i, to first order times 1.01: m = Sxy / Sxx with dm/dy_i = (x_i - mx) / Sxx and
    dm/dx_i = ((y_i - my) - 2 m (x_i - mx)) / Sxx; c = my - m mx"""
    x, y, bx, by = (np.asarray(v, np.float64) for v in (x, y, bx, by))
    mx, my = x.mean(), y.mean()
    Sxx = np.sum((x - mx) ** 2)
    m = np.sum((x - mx) * (y - my)) / Sxx
    dm = np.sum(np.abs(x - mx) * by + np.abs((y - my) - 2 * m * (x - mx)) * bx) / Sxx
    dc = by.mean() + abs(m) * bx.mean() + abs(mx) * dm
    return 1.01 * dm, 1.01 * dc


# ---- the generated noise ---------------------------------------------------------------------------------------------------------------------------------------
def counters(b, row0, rows):
    """the Philox counters of stream b's pilot rows row0 .. row0 + rows - 1 -> uint64 [rows, 15, 4]: (q & 0xffffffff, b, 4, q >> 32), q = 15 R + (c >> 1)"""
    R = np.uint64(int(row0)) + np.arange(rows, dtype=np.uint64)
    q = np.uint64(15) * R[:, None] + np.arange(15, dtype=np.uint64)[None, :]
    return np.stack([q & nr.MASK, np.full_like(q, b), np.full_like(q, 4), q >> np.uint64(32)], axis=-1)


def gen_noise(seed, b, row0, rows, mistake=None):
    """the unit-variance draws of stream b -> complex128 [rows, 30]: words 0-1 of a counter make the even carrier, words 2-3 the odd one ("words": the other way round)"""
    k0, k1 = nr._key(seed)
    ctr = counters(b, row0, rows)
    w = nr.philox4x32_10(ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3], k0, k1)
    g = np.empty((rows, NC), np.complex128)
    for half in range(2):
        src = 1 - half if mistake == "words" else half
        x, y = nr.gauss_pair(w[2 * src], w[2 * src + 1])
        g[:, half::2] = x + 1j * y
    return g


# ---- this file against the reference, live ------------------------------------------------------------------------------------------------------------------------
def live(ref_dir):
    import os
    sys.path.insert(0, ref_dir)
    os.chdir(ref_dir)
    import torch
    from radae import RADAE, receiver_one
    torch.set_num_threads(1)
    model = RADAE(20, 80, EbNodB=100, rate_Fs=True, pilots=True, cyclic_prefix=0.004, bottleneck=3)       # est_snr.py:128
    rx = receiver_one(model.latent_dim, model.Fs, model.M, model.Ncp, model.Wfwd, model.Nc, model.Ns, model.w, model.P, model.Pend, model.bottleneck,
                      model.pilot_gain, model.time_offset, model.coarse_mag)                              # dsp.py:384: 14 arguments (est_snr.py:131 passes 13)
    assert model.Nc == NC and model.Ns == NS and model.M == M_SYM and model.Ncp == NCP and abs(model.Tmf - 0.12) < 1e-12
    assert np.array_equal(np.asarray(model.w, np.float32), W32) and np.array_equal(np.asarray(model.P).real.astype(np.float64), P) and not np.asarray(model.P).imag.any()
    assert abs(float(model.pilot_gain) - PG) <= 2 * U * PG
    ref_P = rx.Pmat.numpy().astype(np.complex128)
    dP = np.abs(ref_P - PMAT).max()
    assert dP <= 5e-6 * np.abs(PMAT).max(), dP
    rng = np.random.default_rng(7)
    Nw, worst = 8, 0.0
    for snrdB in (-5.0, 5.0, 19.0):
        h = (rng.standard_normal((Nw, NC)) + 1j * rng.standard_normal((Nw, NC))) / np.sqrt(2)
        n = rng.standard_normal((Nw, NC)) + 1j * rng.standard_normal((Nw, NC))
        x = (h * PGP + sigma(snrdB) * n).astype(np.complex64)
        sym = torch.zeros((1, 1, Nw * (NS + 1), NC), dtype=torch.complex64)
        sym[0, 0, ::NS + 1, :] = torch.tensor(x)
        got = rx.est_pilots(sym, Nw - 1, NC, NS + 1).numpy().astype(np.complex128)                        # est_snr.py:70-72
        mine = est_pilots(x)
        d = np.abs(got - mine).max() / np.abs(mine).max()
        worst = max(worst, d)
        assert d <= 5e-6, (snrdB, d)
        for mk in MISTAKES[:2] + ("norot",):
            assert np.abs(got - est_pilots(x, mk)).max() / np.abs(mine).max() > 5e-3, mk                 # the planted mistakes are not the reference
    print(f"Pmat {dP:.3g} absolute, est_pilots {worst:.3g} of the largest pilot")
    print("live ok")


if __name__ == "__main__":
    live(sys.argv[1])
