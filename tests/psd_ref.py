"""The float64 restatement of radae_plots.m: do_plots (:34-72) and bandwidth (:100-116) that the PSD tests compare the device with (include/rade_batch.h:
rade_batch_psd, rade_batch_sigstat, rade_psd_bandwidth): the Welch periodogram of a complex signal with a symmetric Hamming window zero-padded to 1024 points, the
99 % power bandwidth around 1500 Hz, mean power, PAPR and the PAPR of the first `head` samples.

pwelch's defaults for an empty window and overlap were not at hand where this was written (RECALLED, NOT VERIFIED: a Hamming window of 2^ceil(log2(sqrt(n / 0.5)))
samples at 50 % overlap), so welch() takes win and step explicitly, and its window, segment starts and density scaling are pinned against scipy.signal.welch in
tests/test_psd_host.py.

Everything here is float64 except stated_psd(), the header's float32 factorisation written out in NumPy (it shows that the arithmetic the header states is a DFT and
stays inside the counted bound; the device is compared with welch()), and sigstat_f32(), the device's float32 terms of the power sums."""
import numpy as np

FS, NFFT = 8000.0, 1024
U = 2.0 ** -24


def gamma(run):
    """the header's count: | P^[k] - P[k] | <= gamma(R) sum_s S_s^2 / (n_seg Fs sum w^2), S_s = sum_i |x[s + i] w[i]|, R the segments a workgroup adds in float32"""
    return (80 + run) * U


def segments(n, win, step):
    return len(range(0, n - win + 1, step))


def window(win):
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(win) / (win - 1))


def windowed(x, win, step):
    """[n_seg, win] complex128: the windowed segments"""
    x = np.asarray(x, np.complex128)
    st = np.arange(0, len(x) - win + 1, step)
    return x[st[:, None] + np.arange(win)[None, :]] * window(win)[None, :]


def welch(x, win, step, fs=FS):
    """[1024] float64: the two-sided density P[k], k = 0..1023 in natural order"""
    v = windowed(x, win, step)
    X = np.fft.fft(v, NFFT, axis=1)
    return (np.abs(X) ** 2).sum(axis=0) / (len(v) * fs * (window(win) ** 2).sum())


def bound(x, win, step, run, fs=FS):
    """the header's bound on every bin of the device's P"""
    v = windowed(x, win, step)
    S = np.abs(v).sum(axis=1)
    return gamma(run) * (S ** 2).sum() / (len(v) * fs * (window(win) ** 2).sum())


def octave_round(v):
    """round half away from zero, as Octave's round() does (numpy's rounds half to even)"""
    return int(np.sign(v) * np.floor(np.abs(v) + 0.5))


def bandwidth(P, fs=FS, centre_hz=1500.0, frac=0.99, trace=False):
    """bandwidth() / spec_power() as written, with one-based indices: (bw Fs / N, p / total), or None where `en` passes the last bin (the script's index error).
    trace: also the list of (bw, p / total) of every step taken."""
    P = np.asarray(P, np.float64)
    N = len(P)
    total = P.sum()
    centre = octave_round(N * centre_hz / fs)
    bw, steps = 1, []
    while True:
        bw += 1
        st = max(1, octave_round(centre - bw / 2))
        en = octave_round(centre + bw / 2)
        if en > N:
            return (None, steps) if trace else None
        p = P[st - 1:en].sum()
        steps.append((bw, p / total))
        if p > frac * total:
            return ((bw * fs / N, p / total), steps) if trace else (bw * fs / N, p / total)


def margin(P, fs=FS, centre_hz=1500.0, frac=0.99):
    """min over the deciding bw and the one before it of |p - frac total| / total: how far the spectrum is from the step of the bandwidth"""
    res, steps = bandwidth(P, fs, centre_hz, frac, trace=True)
    assert res is not None
    return min(abs(r - frac) for _, r in steps[-2:])


def sigstat(x, head=160):
    """(sum2, peak2, head_sum2, head_peak2) in float64 from the exact squares; zeros for no samples"""
    p = np.abs(np.asarray(x, np.complex128)) ** 2
    h = p[:head]
    return (float(p.sum()), float(p.max()) if len(p) else 0.0, float(h.sum()), float(h.max()) if len(h) else 0.0)


def papr_lines(x, P, head=160, fs=FS):
    """the two lines do_plots prints, from the float64 numbers"""
    s2, pk, hs2, hpk = sigstat(x, head)
    n, hn = len(x), min(len(x), head)
    with np.errstate(divide="ignore", invalid="ignore"):
        av = np.float64(s2) / n
        papr, ppapr = 10 * np.log10(np.float64(pk) / av), 10 * np.log10(np.float64(hpk) / (np.float64(hs2) / hn))
    bw = bandwidth(P, fs)
    return ("Pav: %f PAPRdB: %5.2f PilotPAPRdB: %5.2f" % (av, papr, ppapr), "bandwidth (Hz): %f power/total_power: %f" % bw)


def fma32(a, b, c):
    """float32 fma(a, b, c) for float32 arrays: the product is exact in float64; the sum is rounded to float64 and then to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def sigstat_f32(x):
    """the device's float32 term of every sample: fma(re, re, im im)"""
    x = np.asarray(x, np.complex64)
    return fma32(x.real, x.real, (x.imag * x.imag).astype(np.float32))


def stated_psd(x, win, step, run, w32, t32, fs=FS):
    """The header's factorisation in float32 NumPy: x complex64 [n], w32 the float32 window [win], t32 complex64 [1024] the table e^{-2 pi i m / 1024}.
    [1024] float32: five radix-4 Stockham stages per segment, p = fma(re, re, im im), runs of `run` segments added in float32 in ascending order, the runs in double,
    one multiply by 1 / (n_seg Fs sum w32^2) and one rounding."""
    f32 = np.float32
    x = np.asarray(x, np.complex64)
    st = np.arange(0, len(x) - win + 1, step)
    ns = len(st)

    def tw(y, w):
        re = fma32(-y.imag, w.imag.astype(f32), (y.real * w.real).astype(f32))
        im = fma32(y.imag, w.real.astype(f32), (y.real * w.imag).astype(f32))
        return (re + 1j * im).astype(np.complex64)

    t = np.arange(NFFT // 4)
    total = np.zeros(NFFT, np.float64)
    for r0 in range(0, ns, run):
        acc = np.zeros(NFFT, f32)
        for m in range(r0, min(r0 + run, ns)):
            z = np.zeros(NFFT, np.complex64)
            seg = x[st[m]:st[m] + win]
            z.real[:win] = seg.real * w32
            z.imag[:win] = seg.imag * w32
            y = z
            for ls in (0, 2, 4, 6, 8):
                s = 1 << ls
                q, p = t & (s - 1), t >> ls
                a = [y[t + 256 * j] for j in range(4)]
                e, f, g, d = a[0] + a[2], a[1] + a[3], a[0] - a[2], a[1] - a[3]
                b = [e + f, (g.real + d.imag) + 1j * (g.imag - d.real), e - f, (g.real - d.imag) + 1j * (g.imag + d.real)]
                y2 = np.zeros(NFFT, np.complex64)
                y2[q + s * (4 * p)] = b[0]
                for mm in (1, 2, 3):
                    y2[q + s * (4 * p + mm)] = tw(b[mm].astype(np.complex64), t32[mm * p * s])
                y = y2
            acc = (acc + fma32(y.real, y.real, (y.imag * y.imag).astype(f32))).astype(f32)
        total += acc.astype(np.float64)
    sw2 = (w32.astype(np.float64) ** 2).sum()
    return (total * (1.0 / (ns * fs * sw2))).astype(f32)


# ---- the two signals of the end-to-end tests: vetted on the CPU (tests/test_psd_host.py: margin) before the device is asked for the same bandwidth --------------------
E2E_N, E2E_WIN, E2E_STEP = 20000, 1024, 512
E2E_SEEDS = {"carriers": 11, "noise": 12}


def e2e_signal(name):
    """complex64 [20000]: "carriers": 30 unit carriers at the modem's carrier frequencies (tests/golden/consts.npz: w, radians per sample) with seeded phases plus
    white noise 30 dB below their total power; "noise": seeded white noise of unit power"""
    import os
    rng = np.random.default_rng(E2E_SEEDS[name])
    noise = (rng.standard_normal(E2E_N) + 1j * rng.standard_normal(E2E_N)) / np.sqrt(2)
    if name == "noise":
        return noise.astype(np.complex64)
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consts.npz"))["w"].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, len(w))
    x = np.exp(1j * (w[:, None] * np.arange(E2E_N)[None, :] + ph[:, None])).sum(axis=0)
    return (x + np.sqrt(len(w) * 10 ** (-30 / 10)) * noise).astype(np.complex64)
