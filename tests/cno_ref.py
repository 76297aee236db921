"""Float64 restatement of the reference's est_CNo.py (:23-73) and chirp.py (:50-65), and of the block identity the device kernel rests on (include/rade_batch.h:
rade_batch_cno_est, rade_chirp; radae_amd/csrc/rade_cno.hip).  numpy only; the tests hold the library and the kernel to this file, and this file to the recorded
output of the two scripts (tests/golden/cno.npz, oracle/golden/cno.py)."""
import numpy as np

FS = 8000
HOP = FS // 4
B3K = 3000


def plan(window_time=4.0, flow=400.0, fhigh=2000.0):
    """est_CNo.py:25, :34-42: (N, flow_bin, fhigh_bin, noise_st, noise_en) with Python's int()"""
    N = int(FS * window_time)
    bins_per_Hz = N / FS
    flow_bin = int(bins_per_Hz * flow)
    fhigh_bin = int(bins_per_Hz * fhigh)
    noise_st = fhigh_bin + int(0.1 * fhigh_bin)
    noise_en = noise_st + int(0.1 * fhigh_bin)
    return N, flow_bin, fhigh_bin, noise_st, noise_en


def starts(n, N):
    """est_CNo.py:31"""
    return np.arange(0, n - N, HOP)


def band_sums(rx, window_time=4.0, flow=400.0, fhigh=2000.0):
    """[n_windows, 2] float64: (C + N, band sum of No) of every window, np.fft.fft of the window in float64 (est_CNo.py:32, :38, :45 before the division)"""
    N, flow_bin, fhigh_bin, noise_st, noise_en = plan(window_time, flow, fhigh)
    out = []
    for st in starts(len(rx), N):
        Rx = np.abs(np.fft.fft(np.asarray(rx[st:st + N], np.complex128))) ** 2
        out.append((np.sum(Rx[flow_bin:fhigh_bin]), np.sum(Rx[noise_st:noise_en])))
    return np.array(out, np.float64).reshape(-1, 2)


def finish(bands, window_time=4.0, flow=400.0, fhigh=2000.0):
    """est_CNo.py:44-55, :71 over band sums.  Returns a dict: st and CNodB of the windows with C > 0 (the printed lines), C of every window, max_st, max_CNodB, max_SNRdB"""
    N, flow_bin, fhigh_bin, noise_st, noise_en = plan(window_time, flow, fhigh)
    bins_per_Hz = N / FS
    Nbw = (noise_en - noise_st) / bins_per_Hz
    max_CNodB, max_st = 0, 0
    st_l, cno_l, C_l = [], [], []
    for w, (C_plus_N, Sn) in enumerate(np.asarray(bands, np.float64).reshape(-1, 2)):
        No = Sn / Nbw
        C = C_plus_N - No * (fhigh - flow)
        C_l.append(C)
        if C > 0:
            CNodB = 10 * np.log10(C) - 10 * np.log10(No)
            if CNodB > max_CNodB:
                max_CNodB, max_st = CNodB, w * HOP
            st_l.append(w * HOP); cno_l.append(CNodB)
    return dict(st=np.array(st_l, np.int64), CNodB=np.array(cno_l, np.float64), C=np.array(C_l, np.float64), n_windows=len(C_l), max_st=max_st,
                max_CNodB=float(max_CNodB), max_SNRdB=float(max_CNodB - 10 * np.log10(B3K)))


def est(rx, window_time=4.0, flow=400.0, fhigh=2000.0):
    """the whole script on complex samples"""
    r = finish(band_sums(rx, window_time, flow, fhigh), window_time, flow, fhigh)
    return r


def lines(r):
    """what the script prints for a result of finish(): the `time:` lines and the two-line trailer"""
    out = [f"time: {st:8d} {st/FS:5.2f} CNodB: {c:5.2f}" for st, c in zip(r["st"], r["CNodB"])]
    out.append("           Time   C/No    SNR3k")
    out.append(f"Measured: {r['max_st']/FS:5.2f}  {r['max_CNodB']:6.2f}  {r['max_SNRdB']:6.2f}")
    return out


def chirp(nsec, flow=400.0, fhigh=2000.0, amp=0.25):
    """chirp.py:50-65"""
    Nsam = int(nsec * FS)
    x = np.zeros(Nsam, dtype=np.csingle)
    freq = flow
    delta_freq = (fhigh - flow) / FS
    phase = 0
    for n in np.arange(Nsam):
        phase += 2 * np.pi * freq / FS
        phase -= 2 * np.pi * int(phase / (2 * np.pi))
        freq += delta_freq
        if freq > fhigh:
            delta_freq = -(fhigh - flow) / FS
        if freq < flow:
            delta_freq = (fhigh - flow) / FS
        x[n] = amp * np.exp(1j * phase)
    return x


def window_by_blocks(x, st, N):
    """the N-point DFT of x[st:st + N] by the identity of rade_cno.hip, in float64: H = 2000, J = N / H, k = J q + r,
        B_b[k] = DFT_H(x[b H + n] e^{-2 pi i r n / N})[q]        X_w[k] = sum_{j < J} e^{-2 pi i r j / J} B_{w+j}[k]"""
    H = HOP
    assert N % H == 0 and st % H == 0
    J = N // H
    x = np.asarray(x, np.complex128)
    n = np.arange(H)
    X = np.zeros(N, np.complex128)
    for r in range(J):
        tw = np.exp(-2j * np.pi * r * n / N)
        acc = np.zeros(H, np.complex128)
        for j in range(J):
            b = st // H + j
            acc += np.exp(-2j * np.pi * ((r * j) % J) / J) * np.fft.fft(x[b * H:(b + 1) * H] * tw)
        X[r::J] = acc
    return X


def int16_zeropad(s16):
    """int16tof32.py --zeropad: a real int16 recording as complex64 (x, +0)"""
    return np.asarray(s16, np.int16).astype(np.float32).astype(np.complex64)


def gamma(N):
    """the per-bin error constant of the kernel's float32 path, counted in include/rade_batch.h: 1.01 (372 + 4 J) 2^-24 sqrt N"""
    J = N // HOP
    return 1.01 * (372 + 4 * J) * 2.0 ** -24 * np.sqrt(N)


def band_bound(x_w, S, nb):
    """|dS| <= 2 e sqrt(nb S) + nb e^2 with e = gamma ||x_w||_2, for a band of nb bins whose exact sum is S"""
    e = gamma(len(x_w)) * np.sqrt(np.sum(np.abs(np.asarray(x_w, np.complex128)) ** 2))
    return 2 * e * np.sqrt(nb * S) + nb * e * e


def cnodb_bound(x_w, Sc, Sn, window_time=4.0, flow=400.0, fhigh=2000.0):
    """the band bounds propagated through est_CNo.py:44-52: |dNo| <= bn / Nbw, |dC| <= bc + (fhigh - flow) bn / Nbw, and with d log10(v) <= dv / ((v - dv) ln 10):
    |dCNodB| <= 10 / ln 10 (dC / (C - dC) + dNo / (No - dNo)); infinite where dC >= C or dNo >= No (the bound does not pin the logarithm there)"""
    N, flow_bin, fhigh_bin, noise_st, noise_en = plan(window_time, flow, fhigh)
    Nbw = (noise_en - noise_st) / (N / FS)
    bc, bn = band_bound(x_w, Sc, fhigh_bin - flow_bin), band_bound(x_w, Sn, noise_en - noise_st)
    No = Sn / Nbw
    C = Sc - No * (fhigh - flow)
    dNo = bn / Nbw
    dC = bc + (fhigh - flow) * dNo
    if C <= dC or No <= dNo:
        return np.inf
    return 10 / np.log(10) * (dC / (C - dC) + dNo / (No - dNo))
