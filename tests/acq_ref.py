"""Float64 restatement of the whole-file acquisition stage (include/rade_batch.h: rade_batch_acq_detect, rade_acq_track, rade_batch_acq_refine, rade_acq_stats; the
band-pass of radae_amd/acq.py), for tests/test_acq_host.py (pinned to tests/golden/acq.npz there) and tests/test_acq_gpu.py (the device is compared against it).

The `bug` arguments switch on one mistake each, so that the host tests can show that the fixture comparison rejects it:
  detect: "hop961" hop offsets of 961 k; "dt2_own" Dt2 taken from the hop's own block; "s1_only" the threshold from S1 alone; "ties_last" equal cells resolved to the last
  refine: "no_phase" Dt2 without e^{-j w 960}
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FS, M, NCP, NMF, NFC, NTAP = 8000, 160, 32, 960, 40, 101
RXBUF = 2 * NMF + M + NCP
EPS = 4.5 / 2 ** 20                      # RADE_ACQ_EPS of include/rade_batch.h
TAB = 1e-8                               # RADE_ACQ_TAB: how far the two tables' product may lie from p_w (tests/test_host_cpu.py holds rd_corr_tables_check below it)
NQ = 16
RECORDINGS = ("mpp", "awgn", "foff", "dfdt")
SIX = RECORDINGS + ("noise", "sine")
ALL = SIX + ("awgn320", "dfdt320")
TARGETS = {"awgn320": (11.0, 2.0), "dfdt320": (13.25, 2.0)}      # (fmax_target, acq_time_target) of the fixture's runs; (0.0, 1.0) otherwise


@functools.lru_cache(None)
def consts():
    """(p [160], p_w [160, 40]) as the engine holds them: the float32 words of rd_tables_fill, taken as exact (tests/test_acq_host.py holds them to the reference's
    tables, tests/golden/consts.npz: p, acq_p_w)"""
    import ctypes as C
    import dev_abi
    L, T = dev_abi.load(), dev_abi.Tables()
    L.rd_tables_fill(C.byref(T))
    return (np.ctypeslib.as_array(T.p).view(np.complex64).astype(np.complex128), np.ctypeslib.as_array(T.p_w).view(np.complex64).reshape(M, NFC).astype(np.complex128))


@functools.lru_cache(None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "acq.npz")))


@functools.lru_cache(None)
def fixture_input(name):
    if name in ("noise", "sine"):
        return fixture()["x_" + name]
    x = np.load(os.path.join(GOLDEN, f"rxtrace_{name[:4]}.npz"))["rx_in"].astype(np.complex64)
    return x[320:] if name.endswith("320") else x


def hops(n):
    k = 0
    while n >= RXBUF:                    # rx.py:146 with the deviation of the header; rx = rx[Nmf:-1]
        n -= NMF + 1
        k += 1
    return k


def surface(x, t0, n_rows):
    """D[t][f] = sum_m conj(x[t + m]) p_w[m][f], t = t0 .. t0 + n_rows, complex128"""
    _, p_w = consts()
    X = np.lib.stride_tricks.sliding_window_view(np.conj(np.asarray(x, np.complex128))[t0:t0 + n_rows + M - 1], M)
    return X @ p_w


@functools.lru_cache(None)
def moment_gain():
    """G[f][m] = sum_r |alpha[r][f]| |q_r(x_m)| of the two-stage correlator (rade_pack.c, rd_corr_basis_fill: 16 polynomials orthonormal on x_m = (m - 79.5) / 80, alpha[r][f] =
    sum_m q_r(x_m) e^{j w_f m}): how much the moment form amplifies a rounding error of stage 1 on its way to frequency f.  1 at 0 Hz, 4.4 at -50 Hz"""
    xm = (np.arange(M) - 79.5) / 80
    q = np.zeros((NQ, M)); q[0] = 1; q[1] = xm
    for r in range(1, NQ - 1):
        q[r + 1] = ((2 * r + 1) * xm * q[r] - r * q[r - 1]) / (r + 1)
    for r in range(NQ):
        for _ in range(2):
            for u in range(r):
                q[r] -= (q[u] @ q[r]) * q[u]
        q[r] /= np.sqrt(q[r] @ q[r])
    w = 2 * np.pi * (-50 + 2.5 * np.arange(NFC)) / FS
    alpha = np.array([[(q[r] * np.exp(1j * w[k] * np.arange(M))).sum() for k in range(NFC)] for r in range(NQ)])
    return np.abs(alpha).T @ np.abs(q)


def weight(x, t0, n_rows):
    """A[t][f] = sum_m |x[t + m]| (|p[m]| G[f][m] + TAB / EPS): EPS A[t][f] is the header's bound on the cell (t, f)"""
    p, _ = consts()
    X = np.lib.stride_tricks.sliding_window_view(np.abs(np.asarray(x, np.complex128))[t0:t0 + n_rows + M - 1], M)
    return X @ (np.abs(p)[None, :] * moment_gain() + TAB / EPS).T


def detect(x, pacq_error1=1e-5, bug=None):
    """Every hop of x: a list of dicts with Dtmax12, tmax, f_ind, fmax, S1, S2, Dthresh, candidate; and for the decidability rules of the GPU tests `second`, `second_at` (the best
    cell's runner-up and its flat index 40 t + f), `b12` [960, 40] (the bound on every cell's |Dt1| + |Dt2|) and `A1`, `A2` (the sum of A over the cells of either block)"""
    x = np.asarray(x)
    H = hops(len(x))
    step = NMF + 1 if bug == "hop961" else NMF
    out = []
    mag = {}

    def block(t0):
        if t0 not in mag:
            mag[t0] = (np.abs(surface(x, t0, NMF)), weight(x, t0, NMF))
        return mag[t0]
    for k in range(H):
        (d1, a1), (d2, a2) = block(step * k), block(step * k if bug == "dt2_own" else step * k + NMF)
        s = d1 + d2
        flat = s.ravel()
        i = int(np.argmax(flat)) if bug != "ties_last" else int(flat.size - 1 - np.argmax(flat[::-1]))
        if flat[i] <= 0:
            i = 0
        S1, S2 = d1.sum(), d2.sum()
        sigma_r = (2 * S1 if bug == "s1_only" else S1 + S2) / (NMF * NFC) / np.sqrt(np.pi / 2) / 2
        Dthresh = 2 * sigma_r * np.sqrt(-np.log(pacq_error1 / 5))
        rest = flat.copy()
        rest[i] = -1.0
        out.append(dict(Dtmax12=float(flat[i]), tmax=i // NFC, f_ind=i % NFC, fmax=(-50 + 2.5 * (i % NFC)) if flat[i] > 0 else 0.0, S1=float(S1), S2=float(S2),
                        Dthresh=float(Dthresh), candidate=bool(flat[i] > Dthresh), second=float(rest.max()), second_at=int(np.argmax(rest)),
                        b12=EPS * (a1 + a2) + 2.0 ** -24 * s, cells=s, A1=float(a1.sum()), A2=float(a2.sum())))
    return out


def track(candidate, tmax, f_ind, acq_test):
    """rx.py:151-188: (events [(hop, tmax, f_ind)], log [(state, tmax_candidate, valid_count) before each hop's update])"""
    state, tmax_candidate, valid_count = 0, 0, 0
    events, log = [], []
    for k in range(len(tmax)):
        log.append((state, tmax_candidate, valid_count))
        nxt = state
        if state == 0:
            if candidate[k]:
                nxt, tmax_candidate, valid_count = 1, int(tmax[k]), 1
        elif candidate[k] and abs(int(tmax[k]) - tmax_candidate) < 0.02 * M:
            valid_count += 1
            if valid_count > 3:
                events.append((k, int(tmax[k]), int(f_ind[k])))
                if not acq_test:
                    break
                nxt = 0
        else:
            nxt = 0
        state = nxt
    return events, log


def refine(x, t_abs, fmax, bug=None):
    """acquisition.refine in float64: (t, f, Dmax, |Dt1| of the winning timing [80], runner-up of Dmax); timings whose windows leave [0, n) are skipped"""
    p, _ = consts()
    x = np.asarray(x, np.complex128)
    m = np.arange(M)
    best, second, win = 0.0, 0.0, None
    d1 = np.zeros((80, 3))
    for fi in range(80):
        f = (fmax - 10.0) + fi * 0.25
        w = 2 * np.pi * f / FS
        q = np.exp(-1j * w * m) * np.conj(p)
        for ti in range(3):
            t = t_abs - 1 + ti
            if t < 0 or t + NMF + M > len(x):
                continue
            D1 = np.dot(x[t:t + M], q)
            D2 = np.dot(x[t + NMF:t + NMF + M], q) * (1.0 if bug == "no_phase" else np.exp(-1j * w * NMF))
            d1[fi, ti] = abs(D1)
            v = abs(D1 + D2)
            if v > best:
                second, best, win = best, v, (t, f, ti)
            elif v > second:
                second = v
    if win is None:
        return t_abs, fmax, 0.0, d1[:, 0], 0.0
    return win[0], win[1], best, d1[:, win[2]], second


def stats(events, refined, n_hops, ntap, fmax_target=0.0, acq_time_target=1.0):
    """rx.py:134, :170-171, :190-195: (passes, fails, pfail, mean_acq_time, passed); events [(hop, ..)], refined [(t absolute, f)]"""
    target = NCP + ntap / 2
    ok = [abs((t - NMF * e[0]) - target) < 0.0025 * FS and abs(f - fmax_target) <= 5.0 for e, (t, f) in zip(events, refined)]
    passes, fails = sum(ok), len(ok) - sum(ok)
    pfail = fails / (passes + fails) if ok else 0.0
    mean = (NMF * (n_hops + 1) / FS) / passes if passes else np.inf
    return passes, fails, pfail, mean, bool(pfail < 0.2 and mean < acq_time_target)


def bpf(x):
    """complex_bpf(101, Fs, bandwidth, centre, len(x)).bpf(x) in float64, with the float32 taps of radae_amd.acq.bpf_design"""
    from radae_amd.acq import bpf_design
    h, alpha = bpf_design()
    pv = np.exp(-1j * alpha * np.arange(1, len(x) + 1))
    mem = np.concatenate([np.zeros(NTAP - 1, np.complex128), np.asarray(x, np.complex128) * pv])
    return np.convolve(mem, h.astype(np.float64)[::-1], "valid") * np.conj(pv)


@functools.lru_cache(None)
def fixture_detect(name):
    """detect() of a fixture input without the band-pass, computed once and shared (read-only) by the tests"""
    return detect(fixture_input(name))
