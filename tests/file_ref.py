"""Float64 restatement of the stored-file receiver past the acquisition (include/rade_batch.h: rade_batch_bpf_file, rade_file_plan, rade_batch_rx_file,
rade_batch_ber_align, rade_ber_best), for tests/test_rx_file_host.py (held to the committed recordings and, where the reference is present, to the reference live) and
tests/test_rx_file_gpu.py (the device is compared against it).  The filter's restatement is acq_ref.bpf; detect, track and refine are acq_ref's.

The `bug` arguments switch on one mistake each, so that the host tests can show that their comparison rejects it:
  plan: "refine_at_event" refine at the acquiring hop instead of one frame later; "tail_kept" the stream length not shortened by the hops' tail samples
  mix: "origin0" the phase counted from sample 0 of the file instead of from `start`
  ber_align: "n_bits_syms" the denominator n_syms instead of len(z)

Run as a program (python tests/file_ref.py REFERENCE_DIR) it holds the restatements to the reference's own complex_bpf, acquisition.refine and RADAE.receiver and
prints one line per check; tests/test_rx_file_host.py starts it as a child process where the reference exists.
"""
import functools
import os
import sys

import numpy as np

import acq_ref as R

FS, M, NCP, NMF, NC, NS, ZMF = 8000, 160, 32, 960, 30, 4, 240
OK, NOT_ACQUIRED, REFINE_OUTSIDE, EARLY, SHORT = range(5)           # RADE_FILE_*
# what the reference's own classes give on the committed recordings (the issue's table; measured with acquisition, complex_bpf and RADAE.receiver):
# input -> (n, event hop, coarse tmax, coarse fmax, refined t relative to the refine's frame, refined f, n_left, n_mf)
TABLE = {
    ("mpp", False): (30752, 10, 368, -10.0, 368, -11.75, 19845, 20), ("mpp", True): (30752, 10, 418, -10.0, 418, -11.75, 19795, 20),
    ("awgn", False): (24992, 10, 352, 10.0, 352, 11.0, 14101, 14), ("awgn", True): (24992, 10, 402, 10.0, 402, 11.0, 14051, 14),
    ("foff", False): (26752, 6, 192, 10.0, 192, 11.0, 19865, 20), ("foff", True): (26752, 6, 242, 10.0, 242, 11.0, 19815, 20),
    ("dfdt", False): (30752, 11, 352, 15.0, 352, 21.25, 18900, 19), ("dfdt", True): (30752, 11, 402, 15.0, 402, 21.25, 18850, 19),
}


@functools.lru_cache(None)
def consts():
    return dict(np.load(os.path.join(R.GOLDEN, "consts.npz")))


@functools.lru_cache(None)
def recording(name, bpf):
    """a committed recording, raw or through the float64 band-pass rounded to complex64 (what the script hands its frame loop)"""
    x = R.fixture_input(name)
    return R.bpf(x).astype(np.complex64) if bpf else x


def plan_after(n, hop, t, f, freq_offset=None, bug=None):
    """rade_file_plan: (status, start, n_mf, freq, n_left)"""
    freq = f if freq_offset is None else freq_offset
    if hop < 0:
        return NOT_ACQUIRED, 0, 0, freq, 0
    base, length = NMF * (hop + 1), n - (0 if bug == "tail_kept" else hop + 1)
    if t < 0 or t + NMF + M > length:
        return REFINE_OUTSIDE, 0, 0, freq, 0
    if t - base < NCP:
        return EARLY, 0, 0, freq, 0
    start = t - NCP
    n_left = length - start
    n_mf = (n_left // (M + NCP)) // (NS + 1)
    if n_mf < 2:
        return SHORT, 0, 0, freq, n_left
    return OK, start, n_mf, freq, n_left


def plan(x, freq_offset=None, bug=None, det=None):
    """rx.py's normal run up to the trim (rx.py:146-223) on one stream: a dict with hop, tmax, fmax (coarse), t (absolute), f, Dmax, second (refine's runner-up), status,
    start, n_mf, freq, n_left.  hop -1: not acquired"""
    x = np.asarray(x)
    det = R.detect(x) if det is None else det
    events, _ = R.track([h["candidate"] for h in det], [h["tmax"] for h in det], [h["f_ind"] for h in det], False)
    if not events:
        st = plan_after(len(x), -1, 0, 0.0, freq_offset)
        return dict(hop=-1, tmax=0, fmax=0.0, t=0, f=0.0, Dmax=0.0, second=0.0, status=st[0], start=0, n_mf=0, freq=st[3], n_left=0)
    k, tmax, _ = events[0]
    fmax = det[k]["fmax"]
    adv = k if bug == "refine_at_event" else k + 1                   # rx = rx[Nmf:-1]; mf += 1 runs once more after the acquiring hop
    length = len(x) - (0 if bug == "tail_kept" else adv)
    t, f, Dmax, _, second = R.refine(x[:length], NMF * adv + tmax, fmax)
    hop = adv - 1
    status, start, n_mf, freq, n_left = plan_after(len(x), hop, t, f, freq_offset, bug)
    return dict(hop=k, tmax=tmax, fmax=fmax, t=t, f=f, Dmax=Dmax, second=second, status=status, start=start, n_mf=n_mf, freq=freq, n_left=n_left, base=NMF * adv)


@functools.lru_cache(None)
def recording_plan(name, bpf):
    """plan() of a committed recording, computed once and shared (read-only) by the tests"""
    return plan(recording(name, bpf), det=None if bpf else R.fixture_detect(name))


def mix(x, start, freq, bug=None):
    """rx[start:] * exp(-1j w arange(len)) (rx.py:223-228) in complex128, rounded once to complex64"""
    y = np.asarray(x)[start:].astype(np.complex128)
    m = np.arange(len(y)) + (start if bug == "origin0" else 0)
    return (y * np.exp(-1j * (2 * np.pi * freq / FS) * m)).astype(np.complex64) if freq != 0 else y.astype(np.complex64)


def demod(rx, eq="ls", coarse_mag=True, time_offset=-16, bottleneck=3, n_mf=None, quirk=True):
    """RADAE.receiver up to z_hat, the project's one NumPy restatement of it (complex128): cyclic prefix removal, DFT, do_pilot_eq for the four EQ modes, coarse_mag at
    both bottleneck scalings, the demapper: [3 n_mf, 80].  Every frame but the last interpolates towards the next frame's pilot; the last one reuses the loop's final
    slope (carrier Nc - 1, frame n_mf - 2) for every carrier.  quirk = False: what a per-carrier last slope would give (tests/test_ideal_rx_host.py pins the quirk)"""
    c = consts()
    P, Wfwd, w = c["P"].real.astype(np.float64), c["Wfwd"].astype(np.complex128), c["w"].astype(np.float64)
    n_mf = (len(rx) // (M + NCP)) // (NS + 1) if n_mf is None else n_mf
    r = np.asarray(rx)[:n_mf * NMF].reshape(n_mf * (NS + 1), M + NCP)[:, NCP + time_offset:NCP + time_offset + M]
    sym = (r.astype(np.complex128) @ Wfwd).reshape(n_mf, NS + 1, NC)
    if eq != "none":
        h = sym[:, 0, :] / P
        rp = np.zeros((n_mf, NC), np.complex128)
        a = 0.0025 * FS
        for c_ in range(NC):
            cm = min(max(c_, 1), NC - 2)
            if eq == "all":
                rp[:, c_] = h.mean(axis=1)
            elif eq == "mean6":
                rp[:, c_] = h[:, cm - 1:cm + 2].mean(axis=1)
            else:
                A = np.stack([np.ones(3), np.exp(-1j * w[cm - 1:cm + 2] * a)], axis=1)
                g = h[:, cm - 1:cm + 2] @ (np.linalg.inv(A.T @ A) @ A.T).T
                rp[:, c_] = g[:, 0] + g[:, 1] * np.exp(-1j * w[c_] * a)
        s = np.arange(1, NS + 1)
        for i in range(n_mf):
            if i < n_mf - 1:
                slope = (rp[i + 1] - rp[i]) / (NS + 1)
            else:
                slope = np.full(NC, (rp[i, NC - 1] - rp[i - 1, NC - 1]) / (NS + 1)) if quirk else (rp[i] - rp[i - 1]) / (NS + 1)
            sym[i, 1:] *= np.exp(-1j * np.angle(slope[None, :] * s[:, None] + rp[i][None, :]))
        if coarse_mag:
            mag = np.sqrt(np.mean(np.abs(rp) ** 2))
            if bottleneck == 3:
                mag *= abs(P[0]) / (10 ** (-2 / 20) * M / NC ** 0.5)
            sym = sym / mag
    d = sym[:, 1:, :].reshape(n_mf * 3, 40)
    z = np.zeros((n_mf * 3, 80))
    z[:, ::2], z[:, 1::2] = d.real, d.imag
    return z


def ber_align(z, z_hat, bug=None):
    """rx.py:266-276, the script's loop: (n_errors [20], -1 where no reference symbol is left (the script would divide by zero); best shift or -1; best BER)"""
    z, z_hat = np.asarray(z, np.float32).ravel(), np.asarray(z_hat, np.float32).ravel()
    errs, best_f, best_BER = [], -1, 1
    for f in np.arange(20):
        if len(z) == 0:
            errs.append(-1)
            continue
        n_syms = min(len(z), len(z_hat))
        n_errors = int(np.sum(-z[:n_syms] * z_hat[:n_syms] > 0))
        n_bits = n_syms if bug == "n_bits_syms" else len(z)
        BER = n_errors / n_bits
        if BER < best_BER:
            best_BER, best_f = BER, int(f)
        errs.append(n_errors)
        z = z[ZMF:]
    return np.array(errs, np.int64), best_f, float(best_BER)


def check_z(z, ref, what):
    """the rule both fixed-timing receivers' latents are held to: RMS within 1e-5 of the latents' own scale (1e-5 absolute for unit-scale latents), signs equal wherever
    |ref| > 1e-3.  Bottleneck-3 latents without a unit magnitude (no coarse_mag; coarse_mag of model19's waveform leaves an RMS of ~23) are compared relative to their
    RMS: the reference computed them in float32, and an exact (float64) restatement misses them by 1.2e-5 absolute already (tests/test_ideal_rx_host.py)"""
    z = np.asarray(z, np.float64); ref = np.asarray(ref, np.float64)
    assert z.shape == ref.shape, (what, z.shape, ref.shape)
    rms = float(np.sqrt(np.mean((z - ref) ** 2)))
    assert rms <= 1e-5 * max(1.0, float(np.sqrt(np.mean(ref ** 2)))), (what, rms)
    big = np.abs(ref) > 1e-3
    assert np.array_equal(np.sign(z[big]), np.sign(ref[big])), what
    return rms


def live(ref_dir):
    """the restatements against the reference's own classes (a child process of the host test: the reference's modules want its directory and import matplotlib)"""
    os.environ["MPLBACKEND"] = "Agg"
    sys.path.insert(0, ref_dir)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.chdir(ref_dir)
    import torch
    from radae import RADAE
    from radae.dsp import acquisition, complex_bpf
    torch.set_num_threads(1)
    c = consts()
    w = c["w"]
    bandwidth, centre = 1.2 * (w[NC - 1] - w[0]) * FS / (2 * np.pi), (w[NC - 1] + w[0]) * FS / (2 * np.pi) / 2
    acq = acquisition(FS, 50, M, NCP, NMF, c["p"], c["pend"])
    for name in R.RECORDINGS:
        x = R.fixture_input(name)
        y = complex_bpf(R.NTAP, FS, bandwidth, centre, len(x)).bpf(x)
        # the stated DEVIATION: the script forms the mixers' argument alpha (i + 1) in float32, so either mixer's phase is off by up to half an ulp of alpha n (2^-9 rad
        # behind sample 23,900); against the exact phase that is |dy[i]| <= 2 delta S[i], S[i] = sum_t |h[t]| |x[i - 100 + t]|, plus complex64's own roundings
        from radae_amd.acq import bpf_design
        h, alpha = bpf_design()
        delta = float(np.spacing(np.float32(alpha * len(x)))) / 2
        S = np.convolve(np.concatenate([np.zeros(R.NTAP - 1), np.abs(x).astype(np.float64)]), np.abs(h.astype(np.float64)), "valid")
        d = np.abs(y - R.bpf(x))
        assert np.all(d <= (2 * delta + 1e-5) * S), (name, float((d / S).max()), delta)
        err = d.max() / np.abs(y).max()
        print(f"complex_bpf {name}: {err:.2e} of the peak")
        for bpf in (False, True):
            xr = recording(name, bpf)
            p = plan(xr)
            k = p["hop"] + 1
            seg = xr[NMF * k:len(xr) - k]
            tmax, fmax = p["tmax"], p["fmax"]
            t2, f2 = acq.refine(seg, tmax, fmax, np.arange(tmax - 1, tmax + 2), np.arange(fmax - 10, fmax + 10, 0.25))
            assert (NMF * k + t2, f2) == (p["t"], p["f"]), (name, bpf, t2, f2, p)
            print(f"refine {name} bpf={bpf}: t {t2} f {f2}")
    rx = np.load(os.path.join(R.GOLDEN, "chan_mpp.npz"))["rx"]
    model = RADAE(21, 80, 100.0, rate_Fs=True, pilots=True, cyclic_prefix=0.004, time_offset=-16, coarse_mag=True, bottleneck=3, pilot_eq=True, eq_mean6=False)
    del model._modules["core_decoder"]
    model.core_decoder = lambda z: z
    for start, freq in ((0, 0.0), (37, 7.25)):
        xs = np.concatenate([np.zeros(start, np.complex64), (rx * np.exp(1j * 2 * np.pi * freq / FS * np.arange(len(rx)))).astype(np.complex64)])
        mixed = mix(xs, start, freq)
        with torch.inference_mode():
            _, z_hat = model.receiver(torch.tensor(mixed))
        rms = check_z(demod(mixed), z_hat.numpy()[0], f"receiver start {start}")
        print(f"RADAE.receiver start {start} freq {freq}: rms {rms:.2e}")
    print("live ok")


if __name__ == "__main__":
    live(sys.argv[1])
