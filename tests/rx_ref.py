"""Float64 restatement of one call of the live receiver (radae_rxe.py:171-330; dsp.py: detect_pilots, refine, check_pilots, receiver_one / do_pilot_eq_one), teacher-forced by
a trace, for tests/test_rx_ref_host.py (held to the reference's recorded traces there) and tests/test_rx_stage_model_gpu.py (k_rx_sync2 is compared against it call by call).

replay(filtered, trace, lcg_seed, foff_err) walks the calls of a trace.  rx_buf (2112 samples, zeros after a reset) is rebuilt from the filtered samples and nin_before;
every value of a call is computed here in complex128 / float64 from that buffer, the tables and the scalars carried from call to call (fmax, tmax, the phase angle, the two
960-entry row sums, the SNR state, the LCG).  Only the discrete decisions come from the trace: state and nin before the call, the cell the device chose, ret.  check()
then holds a trace's values to the records, and the cells it names to the model's own surfaces.  Nothing of the kernel's algebra is here: no moment tables, no binary16
planes, no polynomial expansion, no factored phasor.  The tables are the engine's own float32 words (rd_tables_fill; tests/test_host_cpu.py holds them to the reference's)
taken as exact, as in acq_ref; the least-squares matrices are formed here from the reference's statement (dsp.py:400-412) with its complex64 A.

THE BOUNDS.  Counted from the kernel's stated arithmetic (u = 2^-24, the float32 unit roundoff), never fitted to a device; tests/test_rx_stage_model_gpu.py records how far
below them the MI355X stays (WORST_MEASURED).  ASSUMED, as in include/rade_batch.h: a matrix instruction returns its 33-term sum within 2^-23 of the sum of the terms' moduli.
  Planes.  A sample scaled by the power of two that puts X (the largest |component| of the filtered samples of this call and the two before it, rx2_operand_scale) into
    [2^7, 2^8) is kept as hi + lo in binary16: 2^-22 relative per component, but never better than half a subnormal step, 2^-25 scaled = 2^-32 X: FLOOR = sqrt 2 x 2^-32 X
    per complex sample.  Ten bits below X the planes stop being 22 bits wide: a sample 60 dB under a click keeps 2^-32 X / |x| = 2^-22 x 1000, i.e. it loses 10 bits.
  Surface cells (rx2_detect_q, check2_rows_q).  The header's count for RADE_ACQ_EPS with ONE difference (rade_rx_search.h, rade_rx_check.h): hi x hi, lo x hi and hi x lo
    share one accumulator, a chain of 30 instructions on the full-size sum where the file kernel has 10 + a small chain of 20.  Stage 1 per real component: planes and the
    dropped product 0.75, the chain 30 x 2^-23 = 3.75: 4.5 x 2^-20, sqrt 2 in modulus 6.36; stage 2 1.24, the magnitude 0.19 as in the header: 7.79, with 1.01 for second
    order SEARCH_EPS = 8 x 2^-20.  | |D|^ - |D| | <= SEARCH_EPS A[t][f] + RADE_ACQ_TAB sum |x| + FLOOR sum_m |p[m]| G[f][m], A and G as in acq_ref.weight.
    Dtmax12 of a search call: the bounds of its two cells + u Dtmax12 (one float32 addition).  A row sum: the sum of its 40 cells' bounds + 12 u rowsum (ten additions in
    the lane, two exchanges).  Rows that a call does not refresh keep value and bound.  Dthresh: the 1920 rows' bounds through the same linear map + 6 u Dthresh (the
    float32 mean, two divisions, the sum and the constant).
  refine() (rx2_refine): double sums; each Dt rounded to complex64 (u |Dt|), one float32 addition (u |D|), hypotf (2 u |D|); the double part -- 80-step three-term
    recurrences, which amplify 2^-53 by at most 80^2, and the eighth-order expansion's remainder (0.063^8 / 8! < 2^-47) -- REFINE_F64 = 2^-40 sum |x| |p|.
  The four correlations at (tmax, fmax): double sums of float32 samples against cis_reduced(-w n): the angle reduced in double, rounded to float32 (u pi), sincosf within
    one ulp per component (sqrt 2 x 2 u): CIS_EPS = (pi + 2.83) u < 6 u; CORR: 6 u sum |x| |p| per window.
  Demodulator.  Window phasor cisA x cisB: 2 CIS_EPS + one complex product (sqrt 5 u) = 14.2 u, the sample's product sqrt 5 u: 16.4 u = 1.03 x 2^-20 in modulus.  Per real
    component of the DFT: window planes, wfwd16 planes, dropped lo x lo 0.75; the hi x hi chain 10 x 2^-23 = 1.25, the two cross chains 2 x 10 x 2^-33 = 0.02, the two joining
    additions 0.125: 2.15, sqrt 2 in modulus 3.03.  SYM_R = 1.01 (1.03 + 3.03) = 4.1 x 2^-20: e_sym(s, c) <= SYM_R sum_n |x_s[n]| + 160 FLOOR, the same for every carrier.
  rp, mag, z_hat: first order, per element.  e_rp(c) = sum_k (|Pmat[c][0][k]| + |Pmat[c][1][k]|) (e_sym(cm - 1 + k) / |P| + EQ_U u |h_k|), EQ_U = 10: the division, the table
    entry, a product (sqrt 5), three running additions, the rotation's product and addition.  e_ch(k) = (1 - k / 5) e_rp0 + (k / 5) e_rp1 + 4 u (|rp0| + |rp1|).
    e_mag = sum |rp| e_rp / (60 mag0) + 12 u mag (two hypotf, the squares, the 6-level sum, powf, product, division).
    e_z(k, c) = (e_sym(k, c) + |sym| (min(2, e_ch / |ch|) + 8 u)) / mag + |z| e_mag / mag.  End of over: the same without mag, e_s from the three pilot rows.
  SNR estimate.  q_c = Im(sym0 conj(rp0) / |rp0|), e_q = e_sym0 + |sym0| (e_rp0 / |rp0| + 8 u); dS1 = sum 2 |sym0| e_sym0 + 6 u S1, dS2 = sum (2 |q| e_q + e_q^2) + 6 u S2;
    d snr = dS1 / (2 S2) + S1 dS2 / (2 S2 (S2 - dS2)): unbounded once dS2 reaches S2 (a clean channel: S2 is rounding noise), and so is the decibel once d snr reaches snr.
    The bound then says inf; the estimate's state is taken from the trace on that call (counted by check(): `snr_reseeded`), so the later calls are held again.

Reuse.  acq_ref.surface (the complex surface), acq_ref.weight (A[t][f] at the peak, `A_peak`), acq_ref.moment_gain and acq_ref.consts are used as they are.  The rest is
stated here because acq_ref's forms do not fit a live call: its cell bound carries the file kernel's RADE_ACQ_EPS (4.5 x 2^-20, two accumulators) and no FLOOR; acq_ref.refine
walks one 80 x 3 grid with skipping of windows outside the file and returns the winner only, where a call needs both grids whole (cells and bounds, for the lead rule) inside
rx_buf; acq_ref.bpf filters a whole file in one piece, where the live filter's memory quirk depends on the call sizes (bpf_calls); file_ref.demod equalises a whole file
frame against frame with the last frame's quirk and float64 angles w a, where one call has two pilot rows, the reference's float32 product w[c] a, and needs rp, mag and the
symbols beside their bounds.

The `bug` argument switches on one mistake (BUGS): tests/test_rx_ref_host.py shows that each breaks a bound against the unperturbed model.
"""
import functools
import math
import os

import numpy as np

import acq_ref as R

FS, M, NCP, NMF, NC, NS, NFC, RXBUF, SYM, NEOO = 8000, 160, 32, 960, 30, 4, 40, 2112, 192, 1152
SEARCH, CANDIDATE, SYNC = 0, 1, 2
U = 2.0 ** -24
SEARCH_EPS = 8.0 / 2 ** 20
FLOOR = math.sqrt(2.0) * 2.0 ** -32
REFINE_F64 = 2.0 ** -40
CIS_EPS = 6.0 * U
SYM_R = 4.1 / 2 ** 20
EQ_U = 10.0
K1, K2 = math.sqrt(-math.log(1e-5 / 5.0)), math.sqrt(-math.log(1e-4 / 5.0))
BUGS = ("win_late", "dft_11bit", "eq_edge_noclamp", "phase_960", "row_off", "pend_p", "peak_cell_off", "mag_nogain")


@functools.lru_cache(None)
def tables():
    """the engine's float32 tables as float64 / complex128, and the equaliser's matrices from the reference's statement"""
    import ctypes as C
    import dev_abi
    L, T = dev_abi.load(), dev_abi.Tables()
    L.rd_tables_fill(C.byref(T))
    cx = lambda a, *s: np.ctypeslib.as_array(a).view(np.complex64).reshape(*s).astype(np.complex128)
    t = dict(Wfwd=cx(T.Wfwd, M, NC), p=cx(T.p, M), pend=cx(T.pend, M), P=np.ctypeslib.as_array(T.P).astype(np.float64), Pend=np.ctypeslib.as_array(T.Pend).astype(np.float64),
             pilot_gain=float(T.pilot_gain), snr_c=float(T.snr_c1) + float(T.snr_c2))
    w32 = (np.float32(2.0 * np.pi) * (15 + np.arange(NC)).astype(np.float32)) / np.float32(160.0)        # radae.py:172-174, float32 tensor arithmetic
    ang = (w32 * np.float32(20.0)).astype(np.float64)                                                  # w[c] a, a = 0.0025 Fs, a float32 product (dsp.py:411, :433)
    e = np.exp(-1j * ang).astype(np.complex64).astype(np.complex128)                                   # the reference's A is complex64
    Pmat = np.zeros((NC, 2, 3), np.complex128)
    for c in range(NC):
        cm = min(max(c, 1), NC - 2)
        A = np.stack([np.ones(3, np.complex128), e[cm - 1:cm + 2]], axis=1)
        Pmat[c] = np.linalg.inv(A.T @ A) @ A.T
    t.update(Pmat=Pmat, rot=e, w0=(np.abs(t["p"])[None, :] * R.moment_gain()).sum(axis=1))
    return t


def bpf_calls(x, sizes):
    """complex_bpf.bpf (dsp.py:63-102) driven call by call, in float64 with the float32 taps of radae_amd.acq.bpf_design.  The reference allocates 100 samples of filter
    memory (dsp.py:55) and keeps the last 102 (dsp.py:96: [-Ntap-1:]), so from the second call on every output is the filter's output two samples earlier, mixed up
    with the phase of its own position: restated as written"""
    from radae_amd.acq import bpf_design
    h, alpha = bpf_design()
    h = h.astype(np.float64)
    mem, phase, out, pos = np.zeros(R.NTAP - 1, np.complex128), 1.0 + 0.0j, [], 0
    for n in sizes:
        n = int(n)
        pv = phase * np.exp(-1j * alpha * np.arange(1, n + 1))
        xm = np.concatenate([mem, np.asarray(x[pos:pos + n], np.complex128) * pv])
        pos += n
        out.append((np.lib.stride_tricks.sliding_window_view(xm, R.NTAP)[:n] @ h) * np.conj(pv))
        mem, phase = xm[-R.NTAP - 1:], pv[-1]
    return np.concatenate(out) if out else np.zeros(0, np.complex128)


# the crafted streams' targets: the edges of the 16-timing tiles, of the groups of 5 tiles, of a wavefront's 240 timings and of the slip rule; the edges of the 8-frequency tiles
TIMINGS = (0, 1, 15, 16, 79, 80, 159, 160, 239, 240, 479, 480, 719, 720, 799, 800, 943, 944, 959)
FREQS = (0, 7, 8, 15, 16, 23, 24, 31, 32, 39)


def targets(B):
    """B (timing, frequency index) pairs; from B = 19 on every timing and every index occurs"""
    return [(TIMINGS[i % len(TIMINGS)], FREQS[i % len(FREQS)]) for i in range(B)]


def crafted(t, fi, n_calls=11, seed=0, noise_db=-40.0):
    """Pilot-only modem frames (p_cp at the transmitter's pilot gain, then zeros) delayed so that the pilot search finds them at timing t, shifted by the coarse grid's
    frequency fi, over white noise noise_db below the pilot symbol's power.  Delay: rx_buf's origin lies 1152 samples (mod 960: 192) before the stream's, the band-pass
    delays by 50 and, from the second call on, by the reference's two more (bpf_calls); the correlation skips the cyclic prefix: t = d + 192 + 52 + 32 (mod 960)."""
    c = np.load(os.path.join(R.GOLDEN, "consts.npz"))
    pilot = c["p_cp"].astype(np.complex128) * float(c["pilot_gain"])
    n = n_calls * NMF + 2 * M
    d = (t - 276) % NMF
    x = np.zeros(n + NMF, np.complex128)
    for k in range(n // NMF + 1):
        s = d + NMF * k
        if s + SYM <= len(x):
            x[s:s + SYM] = pilot
    x = x[:n] * np.exp(2j * np.pi * (-50.0 + 2.5 * fi) / FS * np.arange(n))
    rng = np.random.default_rng(1000 * seed + 40 * t + fi)
    sigma = math.sqrt(np.mean(np.abs(pilot) ** 2)) * 10 ** (noise_db / 20)
    return (x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)).astype(np.complex64)


N_CALLS = 12                                                 # of a crafted stream in the GPU tests: search, candidate, entry, and four synchronised calls or more
LEVELS = (2.0 ** -14, 1.0, 2.0 ** 10, 32767.0, 1.0, 1.0, 2.0 ** -14, 32767.0)
LEVEL_AT = 9 * NMF + 400                                     # inside the synchronised part of streams 4 and 5 (sync from call 6 or 7 on)


def crafted_batch(B, scales=None):
    """(targets, streams) of the peak-placement recipe, each stream scaled as a whole where `scales` says so"""
    tg = targets(B)
    rows = [crafted(t, fi, n_calls=N_CALLS, seed=b) for b, (t, fi) in enumerate(tg)]
    if scales is not None:
        rows = [(r.astype(np.complex128) * s).astype(np.complex64) for r, s in zip(rows, scales)]
    return tg, rows


def level_batch():
    """the level streams: the recipe at LEVELS; stream 4 drops by 2^8 at LEVEL_AT, stream 5 carries a single click there, 60 dB above its RMS"""
    tg, rows = crafted_batch(len(LEVELS), LEVELS)
    rows[4] = np.concatenate([rows[4][:LEVEL_AT], rows[4][LEVEL_AT:] * np.float32(2.0 ** -8)])
    rows[5] = rows[5].copy()
    rows[5][LEVEL_AT] += np.complex64(1000.0 * np.sqrt(np.mean(np.abs(rows[5]) ** 2)))
    return tg, rows


def decidable(recs):
    """for every arg-max a replay takes (search surface, entry grid, in-sync grid): (call, what, lead, the sum of the bounds of the maximum and of the runner-up).  A call whose
    lead exceeds that sum cannot come out undecided in check(): whichever other cell a device names, the cell rule calls it wrong, not undecided"""
    out = []

    def one(i, what, val, bnd):
        v, b = np.asarray(val).ravel(), np.asarray(bnd).ravel()
        o = np.argsort(v)
        out.append((i, what, float(v[o[-1]] - v[o[-2]]), float(b[o[-1]] + b[o[-2]])))
    for r in recs:
        if r["kind"] == "search":
            one(r["call"], "search", r["S"], r["b12"])
            if "entry" in r:
                one(r["call"], "entry", r["entry"]["V"], r["entry"]["bV"])
        else:
            one(r["call"], "refine", r["V"], r["bV"])
    return out


def z_all_of(g):
    """the per-call 240-float rows of a stored trace (z_hat rows where ret & 1, the end-of-over symbols where ret & 2)"""
    z = np.zeros((len(g["ret"]), 240), np.float64)
    if len(g["z_hat"]) == int(np.sum((g["ret"] & 1) == 1)):
        z[(g["ret"] & 1) == 1] = g["z_hat"]
    if g["eoo_out"].size:
        z[(g["ret"] & 2) == 2, :g["eoo_out"].shape[1]] = g["eoo_out"]
    return z


def lcg_rows(state):
    """check_pilots' 48 row draws (oracle/golden/reference.py): x <- 1664525 x + 1013904223 mod 2^32, row (x >> 8) mod 960"""
    rows = []
    for _ in range(48):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        rows.append((state >> 8) % NMF)
    return rows, state


def rx_bufs(filtered, nin_before):
    """rx_buf after each call (radae_rxe.py:196-197), complex64 [n_calls, 2112]"""
    buf, out, pos = np.zeros(RXBUF, np.complex64), [], 0
    for nin in nin_before:
        nin = int(nin)
        buf = np.concatenate([buf[nin:], np.asarray(filtered[pos:pos + nin], np.complex64)])
        assert len(buf) == RXBUF, "the trace consumed more samples than were given"
        pos += nin
        out.append(buf)
    return np.array(out).reshape(-1, RXBUF)


def _sliding(a, t0, n):
    return np.lib.stride_tricks.sliding_window_view(a[t0:t0 + n + M - 1], M)


def surface(buf, X, frame, rows=None):
    """(|Dt| [n, 40], the cells' bounds [n, 40]) of one frame of rx_buf (0: Dt1, 1: Dt2), every timing or the given rows"""
    t = tables()
    p, p_w = R.consts()
    idx = np.arange(NMF) if rows is None else np.asarray(rows)
    W = np.ascontiguousarray(_sliding(buf, frame * NMF, NMF)[idx])
    A = np.abs(W)
    D = np.abs(np.conj(W.astype(np.complex128)) @ p_w)
    return D, SEARCH_EPS * (A @ (np.abs(p)[None, :] * R.moment_gain()).T) + R.TAB * A.sum(axis=1)[:, None] + FLOOR * X * t["w0"][None, :]


def _argmax_first(a):
    """the arg-max of a flat array under the reference's strict `>` from 0, and the lead over the best other entry"""
    i = int(np.argmax(a))
    rest = np.delete(a, i)
    return i, float(a[i] - (rest.max() if rest.size else 0.0))


def refine_grid(buf, tgrid, fgrid, bug=None):
    """acquisition.refine's |Dt1 + Dt2| [len(f), len(t)] (the reference's loop order: frequency outer) and the cells' bounds"""
    p = tables()["p"]
    x = buf.astype(np.complex128)
    m = np.arange(M)
    w = 2 * np.pi * np.asarray(fgrid, np.float64) / FS
    Q = np.exp(-1j * w[:, None] * m[None, :]) * np.conj(p)[None, :]
    X1 = np.array([x[t:t + M] for t in tgrid]); X2 = np.array([x[t + NMF:t + NMF + M] for t in tgrid])
    D1 = Q @ X1.T
    D2 = (Q @ X2.T) * np.exp(-1j * w * NMF)[:, None]
    V = np.abs(D1 + D2)
    wt = (np.abs(X1) @ np.abs(p))[None, :] + (np.abs(X2) @ np.abs(p))[None, :]
    return V, U * (np.abs(D1) + np.abs(D2)) + 3 * U * V + REFINE_F64 * wt


def sync_cell(tr, i, fm, tm, fgrid, t0, nt):
    """the cell a synchronised call's trace row names: (timing before the slip rule, grid frequency index or None when fmax is no 0.9 fm + 0.1 f of the grid)"""
    fi = [k for k, f in enumerate(fgrid) if 0.9 * fm + 0.1 * float(f) == float(tr["fmax"][i])]
    t = int(tr["tmax"][i])
    cands = [c for c in (t, t + M, t - M) if t0 <= c < t0 + nt and slip(c)[1] == t]
    return (cands[0] if cands else None), (fi[0] if fi else None)


def slip(t):
    """radae_rxe.py:208-218: (nin, tmax) after the slip rule"""
    nin = NMF
    if t >= NMF - M:
        nin, t = NMF + M, t - M
    if t < M:
        nin, t = NMF - M, t + M
    return nin, t


def _unit(c):
    a = np.abs(c)
    return np.where(a > 0, np.conj(c) / np.where(a > 0, a, 1.0), 1.0)


def demod(buf, t2, theta, w, X, eoo, snr_state, bug=None):
    """receiver_one on the frequency-corrected window: a dict with sym, e_sym, rp, mag, z (240 floats, or 180 on an end-of-over call), e_z per float, the SNR estimate and its bound"""
    t = tables()
    n = np.arange(NEOO)
    x = buf.astype(np.complex128)[t2 - NCP:t2 - NCP + NEOO]
    rx1 = x * np.exp(1j * (theta - w * (n + 1)))
    off = NCP - 16 + (1 if bug == "win_late" else 0)
    win = np.array([rx1[SYM * s + off:SYM * s + off + M] for s in range(6)])
    if bug == "dft_11bit":
        sc = 2.0 ** (np.floor(np.log2(max(X, 1e-300))) - 7)
        f16 = lambda v: (v / sc).astype(np.float16).astype(np.float64) * sc
        win = f16(win.real) + 1j * f16(win.imag)
    sym = win @ t["Wfwd"]
    e_sym = np.repeat((SYM_R * np.abs(win).sum(axis=1) + M * FLOOR * X)[:, None], NC, axis=1)
    out = dict(sym=sym, e_sym=e_sym, wsum=np.abs(win).sum(axis=1))
    P, Pe = t["P"], t["Pend"]
    if eoo:
        s = sym[0] / P + sym[1] / Pe + sym[5] / Pe
        e_s = (e_sym[0] + e_sym[1] + e_sym[5]) / np.abs(P) + 5 * U * (np.abs(sym[0]) + np.abs(sym[1]) + np.abs(sym[5])) / np.abs(P)
        v = sym[2:5] * _unit(s)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(np.abs(s) > 0, np.minimum(2.0, e_s / np.abs(s)), 2.0)
        e_v = e_sym[2:5] + np.abs(sym[2:5]) * (rel[None, :] + 8 * U)
        out.update(z=np.stack([v.real, v.imag], axis=-1).ravel(), e_z=np.repeat(e_v.ravel(), 2), snr=snr_state[0], e_snr=snr_state[1])
        return out
    rp, e_rp = np.zeros((2, NC), np.complex128), np.zeros((2, NC))
    for c in range(NC):
        cm = c if bug == "eq_edge_noclamp" else min(max(c, 1), NC - 2)
        idx = np.clip(np.arange(cm - 1, cm + 2), 0, NC - 1) if bug == "eq_edge_noclamp" else np.arange(cm - 1, cm + 2)
        for i, row in enumerate((0, 5)):
            h = sym[row, idx] / P[idx]
            g = t["Pmat"][c] @ h
            rp[i, c] = g[0] + g[1] * t["rot"][c]
            pm = np.abs(t["Pmat"][c]).sum(axis=0)
            e_rp[i, c] = (pm * (e_sym[row, idx] / np.abs(P[idx]) + EQ_U * U * np.abs(h))).sum()
    mag0 = math.sqrt(np.mean(np.abs(rp) ** 2)) + 1e-6
    gain = 1.0 if bug == "mag_nogain" else abs(P[0]) / t["pilot_gain"]
    mag = mag0 * gain
    e_mag = ((np.abs(rp) * e_rp).sum() / (60 * mag0) + 12 * U * mag0) * gain
    k = np.arange(1, NS + 1)[:, None]
    ch = (rp[1] - rp[0])[None, :] / 5 * k + rp[0][None, :]
    e_ch = (1 - k / 5) * e_rp[0][None, :] + (k / 5) * e_rp[1][None, :] + 4 * U * (np.abs(rp[0]) + np.abs(rp[1]))[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(np.abs(ch) > 0, np.minimum(2.0, e_ch / np.abs(ch)), 2.0)
    z = sym[1:5] * _unit(ch) / mag
    e_z = (e_sym[1:5] + np.abs(sym[1:5]) * (rel + 8 * U)) / mag + np.abs(z) * e_mag / mag
    # SNR estimate (dsp.py:438-456)
    q = (sym[0] * _unit(rp[0])).imag
    with np.errstate(divide="ignore", invalid="ignore"):
        e_q = e_sym[0] + np.abs(sym[0]) * (np.where(np.abs(rp[0]) > 0, np.minimum(2.0, e_rp[0] / np.abs(rp[0])), 2.0) + 8 * U)
    S1, S2 = float((np.abs(sym[0]) ** 2).sum()), float((q ** 2).sum()) + 1e-12
    dS1 = float((2 * np.abs(sym[0]) * e_sym[0]).sum()) + 6 * U * S1
    dS2 = float((2 * np.abs(q) * e_q + e_q ** 2).sum()) + 6 * U * S2
    raw = S1 / (2 * S2) - 1
    d_snr = dS1 / (2 * S2) + S1 * dS2 / (2 * S2 * (S2 - dS2)) if dS2 < S2 else math.inf
    snr = raw if raw > 0 else 0.1                             # "remove occasional illegal values"
    if raw - d_snr > 0:
        e_db = (10 / math.log(10)) * d_snr / (raw - d_snr)
    elif raw + d_snr <= 0:
        e_db = 0.0                                            # the clip holds whatever the rounding
    else:
        e_db = math.inf
    db =(10 * math.log10(snr) - 2.513) / 0.8070 + t["snr_c"]
    e_new = e_db / 0.8070 + 8 * U * (abs(db) + 10.0)          # log10f, the subtraction, the division, the two constants
    out.update(rp=rp, e_rp=e_rp, mag=mag, e_mag=e_mag, z=np.stack([z.real, z.imag], axis=-1).ravel(), e_z=np.repeat(e_z.ravel(), 2), S1=S1, S2=S2, dS2=dS2,
               snr=0.9 * snr_state[0] + 0.1 * db, e_snr=0.9 * snr_state[1] + 0.1 * e_new + 3 * U * (abs(snr_state[0]) + abs(db)))
    return out


def replay(filtered, trace, lcg_seed=1, foff_err=0.0, bug=None):
    """One record (a dict) per call of `trace`; see the module's docstring.  `kind` is "search" (search and candidate calls; `entry` holds the sync entry's grid) or "sync"."""
    tr = trace
    n_calls = len(tr["ret"])
    bufs = rx_bufs(filtered, tr["nin_before"][:n_calls])
    tb = tables()
    p, pend = tb["p"], tb["pend"]
    rs, rb = np.zeros((2, NMF)), np.zeros((2, NMF))           # row sums and their bounds
    tm, fm, theta, lcg, snr_state, prev_search, pos, prev_dt2 = 0, 0.0, 0.0, int(lcg_seed), (0.0, 0.0), False, 0, None
    xmax, recs = [0.0, 0.0, 0.0], []
    for i in range(n_calls):
        nin, state = int(tr["nin_before"][i]), int(tr["state_before"][i])
        new = np.asarray(filtered[pos:pos + nin]); pos += nin
        xmax = [float(max(np.abs(new.real).max(), np.abs(new.imag).max())), xmax[0], xmax[1]]
        X, buf = max(xmax), bufs[i]
        rec = dict(call=i, state=state, nin=nin, X=X)
        if state != SYNC:
            D1, B1 = prev_dt2 if prev_search else surface(buf, X, 0)          # a cached call reads the previous call's |Dt2| back: same samples, that call's bound
            D2, B2 = surface(buf, X, 1)
            prev_dt2 = (D2, B2)
            D, B = np.array([D1, D2]), np.array([B1, B2])
            S = D[0] + D[1]
            b12 = (B[0] + B[1] + U * S).astype(np.float64)
            am, lead = _argmax_first(S.ravel())
            if S.ravel()[am] <= 0:
                am = 0
            if bug == "peak_cell_off":
                am = min(am + NFC, NMF * NFC - 1)
            rs, rb = D.sum(axis=2), B.sum(axis=2) + 12 * U * D.sum(axis=2)
            sig = (rs[0].sum() + rs[1].sum()) / (NMF * NFC) / math.sqrt(math.pi / 2) / 2
            Dth = 2 * sig * K1
            rec.update(kind="search", S=S, b12=b12, argmax=(am // NFC, am % NFC), lead=lead, Dthresh=Dth, e_Dthresh=2 * K1 * rb.sum() / (NMF * NFC) / math.sqrt(math.pi / 2) / 2 + 6 * U * Dth,
                       cached=prev_search, Dtmax12=float(S.ravel()[am]), snr=snr_state[0], e_snr=snr_state[1],
                       A_peak=tuple(float(R.weight(buf, fr * NMF + am // NFC, 1)[0, am % NFC]) for fr in range(2)))      # the header's A[t][f] of either frame at the peak
            entry = state == CANDIDATE and int(tr["state_after"][i]) == SYNC
            if entry:
                ctm, cfm = am // NFC, -50.0 + 2.5 * (am % NFC)
                tgrid = np.arange(max(0, ctm - 1), ctm + 2)
                fgrid = np.arange(cfm - 10, cfm + 10, 0.25)
                V, bV = refine_grid(buf, tgrid, fgrid)
                k, elead = _argmax_first(V.ravel())
                kt, kf = k % len(tgrid), k // len(tgrid)
                rec.update(entry=dict(V=V, bV=bV, tgrid=tgrid, fgrid=fgrid, argmax=(int(tgrid[kt]), kf), lead=elead, fmax=float(fgrid[kf]) + foff_err, foff_err=foff_err))
                # the device's decision: its refined timing, and the grid frequency whose value + foff_err is the trace's fmax
                tm = int(tr["tmax"][i])
                fi = [j for j, f in enumerate(fgrid) if float(f) + foff_err == float(tr["fmax"][i])]
                fm = float(tr["fmax"][i]) if fi else float(fgrid[kf]) + foff_err
                rec["entry"]["cell"] = (tm, fi[0] if fi else None)
                foff_err = 0.0
            else:
                tm, fm = int(tr["tmax"][i]), -50.0 + 2.5 * int(tr["f_ind_max"][i])
            prev_search = int(tr["state_after"][i]) != SYNC
            recs.append(rec)
            continue
        prev_search = False
        t0 = max(0, tm - 8)
        tgrid, fgrid = np.arange(t0, tm + 8), np.arange(fm - 1, fm + 1, 0.1)
        V, bV = refine_grid(buf, tgrid, fgrid)
        k, lead = _argmax_first(V.ravel())
        kt, kf = k % len(tgrid), k // len(tgrid)
        # the device's cell: the grid frequency f for which 0.9 fm + 0.1 f has the trace's fmax bit for bit.  Where one exists, rec["fmax"] is built from it, so check()'s
        # "fmax bits" comparison then holds by construction: what is checked is that such a grid point exists (else "fmax is no 0.9 fm + 0.1 f of the grid") and that it is the
        # arg-max (the cell rule).  The same holds for the entry call's `fi` above.
        dt, df = sync_cell(tr, i, fm, tm, fgrid, t0, len(tgrid))
        rec.update(kind="sync", V=V, bV=bV, tgrid=tgrid, fgrid=fgrid, argmax=(int(tgrid[kt]), kf), lead=lead, cell=(dt, df), fm_before=fm, tm_before=tm)
        tnew = dt if dt is not None else int(tgrid[kt])
        fhat = float(fgrid[df]) if df is not None else float(fgrid[kf])
        fm = 0.9 * fm + 0.1 * fhat
        rec.update(fmax=fm, tmax_refined=tnew)
        # check_pilots (dsp.py:273-320): 48 rows of both surfaces, the thresholds, the four correlations
        rows, lcg = lcg_rows(lcg)
        src = [min(t + 1, NMF - 1) if bug == "row_off" and j == 17 else t for j, t in enumerate(rows)]
        for fr in range(2):
            D, B = surface(buf, X, fr, src)
            rs[fr, rows] = D.sum(axis=1); rb[fr, rows] = B.sum(axis=1) + 12 * U * D.sum(axis=1)
        sig = (rs[0].sum() + rs[1].sum()) / (NMF * NFC) / math.sqrt(math.pi / 2) / 2
        Dth, Dth_eoo = 2 * sig * K2, 2 * sig * K1
        e_sig = rb.sum() / (NMF * NFC) / math.sqrt(math.pi / 2) / 2
        w = 2 * np.pi * fm / FS
        xw = buf.astype(np.complex128)
        wv = np.exp(-1j * w * np.arange(M))
        corr = lambda a, q: (abs(np.dot(np.conj(wv * xw[a:a + M]), q)), (CIS_EPS + REFINE_F64) * float(np.abs(xw[a:a + M]) @ np.abs(q)), float(np.abs(xw[a:a + M]) @ np.abs(q)))
        pe = p if bug == "pend_p" else pend
        c = [corr(tnew, p), corr(tnew + NMF, p), corr(tnew + M + NCP, pe), corr(tnew + NMF, pe)]
        nin_after, t2 = slip(tnew)
        eoo = bool(int(tr["ret"][i]) & 2)
        rec.update(rows=rows, Dthresh=Dth, e_Dthresh=2 * K2 * e_sig + 6 * U * Dth, Dthresh_eoo=Dth_eoo, e_Dthresh_eoo=2 * K1 * e_sig + 6 * U * Dth_eoo, Dtmax12=c[0][0] + c[1][0], e_Dtmax12=c[0][1] + c[1][1],
                   Dtmax12_eoo=c[2][0] + c[3][0], e_Dtmax12_eoo=c[2][1] + c[3][1], w_corr=tuple(q[2] for q in c), nin_after=nin_after, tmax=t2, theta_before=theta, eoo=eoo, rowsum=rs.copy())
        d = demod(buf, t2, theta, w, X, eoo, snr_state, bug)
        th = theta - w * (NMF if bug == "phase_960" else NEOO)
        theta = th - 2 * np.pi * np.rint(th / (2 * np.pi))
        rec.update(d, theta_after=theta)
        if not eoo:
            snr_state = (d["snr"], d["e_snr"])
            if not math.isfinite(snr_state[1]):              # the bound is unbounded on this call: the state restarts from the trace (see the docstring)
                snr_state = (float(tr["snrdB_3k_est"][i]), 0.0)
                rec["snr_reseeded"] = True
        tm = t2
        recs.append(rec)
    return recs


def synth_trace(recs, trace):
    """a trace whose values are the records' own (the discrete columns of `trace` kept): what a device that computed exactly these values would report"""
    t = {k: np.array(v, copy=True) for k, v in trace.items()}
    z = np.zeros((len(recs), 240), np.float64)
    for r in recs:
        i = r["call"]
        t["Dthresh"][i] = r["Dthresh"]; t["Dtmax12"][i] = r["Dtmax12"]
        if r["kind"] == "search":
            if "entry" not in r:
                t["tmax"][i], t["f_ind_max"][i] = r["argmax"]
            else:
                t["f_ind_max"][i] = r["argmax"][1]
            continue
        t["Dtmax12_eoo"][i] = r["Dtmax12_eoo"]; t["fmax"][i] = r["fmax"]; t["snrdB_3k_est"][i] = r["snr"]; t["nin_after"][i] = r["nin_after"] if int(trace["state_after"][i]) == SYNC else NMF
        t["tmax"][i] = r["tmax"]
        z[i, :len(r["z"])] = r["z"]
    t["z_all"] = z
    return t


def check(recs, trace, z=True):
    """Hold `trace` (with z_all; z=False: a trace that keeps no row per call) to the records: a dict with `fail` (a list of (call, what, error, bound); empty when every value of
    every call is inside its bound), `worst` (the largest error / bound per quantity), `largest` (the largest error per quantity), `undecided` (calls whose arg-max the model
    cannot decide) and `snr_reseeded`"""
    tr, fail, worst, largest, undecided, reseeded = trace, [], {}, {}, 0, 0

    def hold(i, what, err, bound):
        err = float(err)
        largest[what] = max(largest.get(what, 0.0), err)
        if bound > 0 and math.isfinite(bound):
            worst[what] = max(worst.get(what, 0.0), err / bound)
        if not err <= bound:
            fail.append((i, what, err, float(bound)))

    def cell_rule(i, what, val, bnd, am, lead, cell):
        """the device's cell equals the model's arg-max when the lead exceeds the two cells' bounds; otherwise undecided, and the value at its cell within that sum of the maximum"""
        nonlocal undecided
        if cell == am:
            return
        if cell is None or any(c is None for c in cell):
            fail.append((i, what + " cell not on the grid", math.inf, 0.0)); return
        two = float(bnd[am] + bnd[cell])
        if lead > two:
            fail.append((i, what + f" cell {cell} != arg-max {am}", float(val[am] - val[cell]), two)); return
        undecided += 1
        if not val[am] - val[cell] <= two:
            fail.append((i, what + " undecided cell below the maximum", float(val[am] - val[cell]), two))

    for r in recs:
        i = r["call"]
        hold(i, "Dthresh", abs(tr["Dthresh"][i] - r["Dthresh"]), r["e_Dthresh"])
        if r["kind"] == "search":
            f_dev = int(tr["f_ind_max"][i])
            if "entry" in r:
                e = r["entry"]
                cell = (r["argmax"][0], f_dev)             # the trace of an entry call holds the refined timing: the coarse one is the model's
                cell_rule(i, "search", r["S"], r["b12"], r["argmax"], r["lead"], cell)
                et, ef = e["cell"]
                ecell = None if ef is None or not e["tgrid"][0] <= et <= e["tgrid"][-1] else (ef, et - int(e["tgrid"][0]))
                am = (e["argmax"][1], e["argmax"][0] - int(e["tgrid"][0]))
                cell_rule(i, "entry", e["V"], e["bV"], am, e["lead"], ecell)
            else:
                cell = (int(tr["tmax"][i]), f_dev)
                if r["S"][r["argmax"]] <= 0:
                    cell = cell if (cell == (0, 0) and tr["fmax"][i] == 0.0) else None
                    if cell is None:
                        fail.append((i, "all-zero search call", math.inf, 0.0)); continue
                cell_rule(i, "search", r["S"], r["b12"], r["argmax"], r["lead"], cell)
            if 0 <= cell[0] < NMF and 0 <= cell[1] < NFC:
                hold(i, "Dtmax12 search", abs(tr["Dtmax12"][i] - r["S"][cell]), r["b12"][cell])
            continue
        dt, df = r["cell"]
        if df is None:
            fail.append((i, "fmax is no 0.9 fm + 0.1 f of the grid", math.inf, 0.0))
        elif dt is None:
            fail.append((i, "tmax outside the refine grid or against the slip rule", math.inf, 0.0))
        else:
            cell_rule(i, "refine", r["V"], r["bV"], (r["argmax"][1], r["argmax"][0] - int(r["tgrid"][0])), r["lead"], (df, dt - int(r["tgrid"][0])))
            if float(tr["fmax"][i]) != r["fmax"]:
                fail.append((i, "fmax bits", abs(float(tr["fmax"][i]) - r["fmax"]), 0.0))
        if int(tr["tmax"][i]) != r["tmax"]:
            fail.append((i, "slip rule: tmax", abs(int(tr["tmax"][i]) - r["tmax"]), 0.0))
        if int(tr["state_after"][i]) == SYNC and int(tr["nin_after"][i]) != r["nin_after"]:
            fail.append((i, "slip rule: nin", abs(int(tr["nin_after"][i]) - r["nin_after"]), 0.0))
        hold(i, "Dtmax12 sync", abs(tr["Dtmax12"][i] - r["Dtmax12"]), r["e_Dtmax12"])
        hold(i, "Dtmax12_eoo", abs(tr["Dtmax12_eoo"][i] - r["Dtmax12_eoo"]), r["e_Dtmax12_eoo"])
        margin = r["Dtmax12_eoo"] - r["Dthresh_eoo"]
        if abs(margin) > r["e_Dtmax12_eoo"] + r["e_Dthresh_eoo"] and (margin > 0) != r["eoo"]:
            fail.append((i, "end-of-over decision", abs(margin), r["e_Dtmax12_eoo"] + r["e_Dthresh_eoo"]))
        if z:
            err = np.abs(np.asarray(tr["z_all"][i], np.float64)[:len(r["z"])] - r["z"])
            what = "eoo symbols" if r["eoo"] else "z_hat"
            j = int(np.argmax(err - r["e_z"]))
            worst[what] = max(worst.get(what, 0.0), float((err / r["e_z"]).max()))
            largest[what] = max(largest.get(what, 0.0), float(err.max()))
            if not np.all(err <= r["e_z"]):
                fail.append((i, f"{what}[{j}]", float(err[j]), float(r["e_z"][j])))
        if not r["eoo"]:
            if r.get("snr_reseeded"):
                reseeded += 1
            else:
                hold(i, "snrdB_3k_est", abs(tr["snrdB_3k_est"][i] - r["snr"]), r["e_snr"])
    return dict(fail=fail, worst=worst, largest=largest, undecided=undecided, snr_reseeded=reseeded, calls=len(recs))
