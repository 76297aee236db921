"""The float64 restatement of plot_specgram.m:6-16 at Fs = 8000 that the spectrogram tests compare the device with (include/rade_batch.h: rade_batch_specgram).

plot_specgram calls the signal package's specgram and hanning.  Neither file, nor an Octave to run them, was at hand where this was written, so the two facts below are
RECALLED, NOT VERIFIED, and no fixture produced by the reference's own program could be made:
  hanning(m) = 0.5 - 0.5 cos(2 pi (1:m)' / (m + 1)): no zero end points;
  specgram(x, n, Fs, window, overlap): a scalar window becomes hanning(window); slices start at the one-based offsets 1 : step : length(x) - window; each is multiplied by
  the window, put into the first rows of an n-row column of zeros and transformed; rows 1 : n / 2 (bins 0..n/2-1) are returned; length(x) <= window is an error.
What is independent of that recollection is checked against scipy.signal.spectrogram in tests/test_specgram_host.py.

Everything here is float64 except levels(), which restates the device's float32 threshold rule, and stated_mags(), the header's float32 factorisation written out in
NumPy (it shows that the arithmetic the header states is a DFT; the device is compared with mags())."""
import numpy as np

FS, WIN, STEP, NFFT = 8000, 1280, 160, 2048
NB = NFFT // 2 - 1                      # bins 1..1023
LO, HI = 10.0 ** (-20 / 10), 10.0 ** (-3 / 10)
U = 2.0 ** -24
GAMMA = 44 * U                          # the header's count: | mag^ - |X| | <= GAMMA sum_i sqrt(v_a[i]^2 + v_b[i]^2) over the slice pair


def starts(n):
    return np.arange(0, n - WIN, STEP)


def window():
    return 0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(WIN) + 1) / (WIN + 1))


def levels_table(lo=LO, hi=HI):
    j = np.arange(1, 256)
    return lo * (hi / lo) ** ((j - 0.5) / 255)


def slices(x):
    """[n_slices, 1280] float64: the windowed slices of a real signal"""
    x = np.asarray(x, np.float64)
    st = starts(len(x))
    return x[st[:, None] + np.arange(WIN)[None, :]] * window()[None, :]


def mags(x):
    """[n_slices, 1023] float64: |X[1..1023]| of every slice"""
    return np.abs(np.fft.rfft(slices(x), NFFT, axis=1)[:, 1:NFFT // 2])


def peak(m):
    return float(m.max())


def pair_sums(x):
    """[n_slices] float64: S of the header's bound for every slice, sum_i sqrt(v_a[i]^2 + v_b[i]^2) over the pair (2 m, 2 m + 1) the slice belongs to"""
    v = slices(x)
    ns = len(v)
    S = np.zeros(ns)
    for m in range(0, ns, 2):
        vb = v[m + 1] if m + 1 < ns else np.zeros(WIN)
        S[m:m + 2] = np.sqrt(v[m] ** 2 + vb ** 2).sum()
    return S


def levels(m, pk, table):
    """The device's rule in float32: the number of j with mag >= T[j] peak, T[j] peak one rounded float32 multiply; a peak of 0 gives level 0.  m: float32 [..]."""
    m = np.asarray(m, np.float32)
    if np.float32(pk) == 0:
        return np.zeros(m.shape, np.uint8)
    thr = (np.asarray(table, np.float32) * np.float32(pk)).astype(np.float32)
    return np.where(np.isnan(m), 0, np.searchsorted(thr, m, side="right")).astype(np.uint8)        # thr does not decrease: the count of thr <= m; a NaN is >= nothing


def levels64(m, pk, lo=LO, hi=HI):
    """float64: the number of j with m >= T[j] pk"""
    return np.searchsorted(levels_table(lo, hi) * pk, m, side="right")


def band(fmin, fmax):
    k0 = max(1, int(np.ceil(fmin * NFFT / FS)))
    k1 = min(NFFT // 2 - 1, int(np.floor(fmax * NFFT / FS)))
    return k0, k1


def stated_mags(x, w32, t32):
    """The header's factorisation in float32 NumPy: x float32 [n], w32 the float32 window, t32 complex64 [2048] the table.  [n_slices, 1023] float32."""
    f32 = np.float32
    x = np.asarray(x, f32)
    st = starts(len(x))
    ns = len(st)
    out = np.zeros((ns, NB), f32)

    def tw(y, w):
        re = (y.real * w.real).astype(f32); re = (re.astype(np.float64) - y.imag.astype(np.float64) * w.imag.astype(np.float64)).astype(f32)      # fma: one rounding
        im = (y.real * w.imag).astype(f32); im = (im.astype(np.float64) + y.imag.astype(np.float64) * w.real.astype(np.float64)).astype(f32)
        return (re + 1j * im).astype(np.complex64)

    t = np.arange(512)
    for m in range(0, ns, 2):
        z = np.zeros(NFFT, np.complex64)
        z.real[:WIN] = x[st[m]:st[m] + WIN] * w32
        if m + 1 < ns:
            z.imag[:WIN] = x[st[m + 1]:st[m + 1] + WIN] * w32
        y = z
        for ls in (0, 2, 4, 6, 8):
            s = 1 << ls
            q, p = t & (s - 1), t >> ls
            a = [y[t + 512 * j] for j in range(4)]
            e, f, g, d = a[0] + a[2], a[1] + a[3], a[0] - a[2], a[1] - a[3]
            b = [e + f, (g.real + d.imag) + 1j * (g.imag - d.real), e - f, (g.real - d.imag) + 1j * (g.imag + d.real)]
            y2 = np.zeros(NFFT, np.complex64)
            y2[q + s * (4 * p)] = b[0]
            for mm in (1, 2, 3):
                y2[q + s * (4 * p + mm)] = tw(b[mm].astype(np.complex64), t32[mm * p * s])
            y = y2
        k = np.arange(1, NFFT // 2)
        zk, zn = y[k] + y[k + 1024], y[1024 - k] - y[2048 - k]
        for col, (re, im) in enumerate((((zk.real + zn.real) * f32(0.5), (zk.imag - zn.imag) * f32(0.5)), ((zk.real - zn.real) * f32(0.5), (zk.imag + zn.imag) * f32(0.5)))):
            if m + col < ns:
                ii = (im * im).astype(f32)
                out[m + col] = np.sqrt((re.astype(np.float64) * re.astype(np.float64) + ii.astype(np.float64)).astype(f32))
    return out
