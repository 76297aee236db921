"""Write tests/golden/cno.npz: what the reference's own chirp.py and est_CNo.py write and print, run as child processes (MPLBACKEND=Agg), on one chirp and three
int16 recordings expanded by the reference's `int16tof32.py --zeropad`.

Arrays:
    chirp                complex64 [20000]: `chirp.py OUT 2.5` at the defaults (up-sweep, turn, down-sweep, turn again)
    rec0, rec1, rec2     int16: 6.5 s (1.5 s of noise, the real part of a 4.5 s chirp, noise to the end; about 40 dB C/No), 3 s (0.5 s of noise, 1.5 s of chirp, noise; about
                         25 dB) and 3 s of noise only
    window_time          float64 [3]: 4.0, 1.0, 1.0 (the script's --window_time)
    st0.., cno0..        int64 / float64: the `time:` lines the script printed for each recording: start sample and the printed C/No
    measured             float64 [3, 3]: the `Measured:` line's Time, C/No, SNR3k as printed
    text0..              the script's standard output, line by line
    skip2                int64: start samples of the windows of rec2 with |C| < 1e-4 S_c in float64 (at most one): the sign of C, and so whether the script prints the window,
                         is not pinned there

The margins the tests rely on are asserted here in float64 (tests/cno_ref.py): the best window of every recording beats the second best by at least 1e-3 dB, and
no window has |C| < 1e-4 S_c except those listed in skip2.  If a seed fails them, change the seed, not the margin.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

from . import reference as R
from .reference import golden

SEED = 20241019


def ref_chirp(td, nsec, amp=None):
    path = os.path.join(td, f"chirp_{nsec}_{amp}.f32")
    subprocess.run([sys.executable, os.path.join(R.REF, "chirp.py"), path, str(nsec)] + (["--amp", repr(float(amp))] if amp is not None else []), check=True, cwd=td)
    return np.fromfile(path, np.complex64)


def ref_zeropad(s16):
    out = subprocess.run([sys.executable, os.path.join(R.REF, "int16tof32.py"), "--zeropad"], input=s16.tobytes(), check=True, capture_output=True).stdout
    return np.frombuffer(out, np.complex64)


def ref_est(td, rx, window_time):
    path = os.path.join(td, "rx.f32")
    rx.tofile(path)
    out = subprocess.run([sys.executable, os.path.join(R.REF, "est_CNo.py"), path, "--window_time", str(window_time)], check=True, capture_output=True, text=True, cwd=td).stdout
    text = [l for l in out.split("\n") if l.strip()]
    st, cno, measured = [], [], None
    for l in text:
        m = re.match(r"time:\s+(\d+)\s+([-\d.]+) CNodB:\s*([-\d.a-z]+)$", l)
        if m:
            st.append(int(m.group(1))); cno.append(float(m.group(3)))
        m = re.match(r"Measured:\s+([-\d.]+)\s+([-\d.]+)\s+([-\d.]+)$", l)
        if m:
            measured = [float(m.group(k)) for k in (1, 2, 3)]
    assert measured is not None and len(st) + 2 == len(text), out
    return np.array(st, np.int64), np.array(cno, np.float64), np.array(measured), np.array(text)


def recording(rng, n, chirp_re, at, sigma):
    x = sigma * rng.standard_normal(n)
    x[at:at + len(chirp_re)] += chirp_re
    assert np.abs(x).max() < 32767
    return np.rint(x).astype(np.int16)


def main(src, dst):
    R.enter(patched=False)
    sys.path.insert(0, os.path.join(R.REPO, "tests"))
    import cno_ref as cr
    OUT = golden(dst, "cno.npz")
    rng = np.random.default_rng(SEED)
    with tempfile.TemporaryDirectory() as td:
        chirp = ref_chirp(td, 2.5)
        assert chirp.shape == (20000,)
        # C / No = (A^2 / 4) 8000 / sigma^2 for a real chirp of amplitude A in real noise of deviation sigma
        c0 = ref_chirp(td, 4.5, 4000.0).real.astype(np.float64)
        c1 = ref_chirp(td, 1.5, 1500.0).real.astype(np.float64)
        recs = [recording(rng, 52000, c0, 12000, 4000.0 * np.sqrt(2000.0 / 10 ** 4.0)),
                recording(rng, 24000, c1, 4000, 1500.0 * np.sqrt(2000.0 / 10 ** 2.5)),
                recording(rng, 24000, np.zeros(0), 0, 3000.0)]
        wt = np.array([4.0, 1.0, 1.0])
        d = dict(chirp=chirp, window_time=wt)
        measured = []
        for k, (s16, w) in enumerate(zip(recs, wt)):
            rx = ref_zeropad(s16)
            assert rx.dtype == np.complex64 and np.array_equal(rx, cr.int16_zeropad(s16))
            st, cno, m, text = ref_est(td, rx, w)
            # the margins, in float64
            bands = cr.band_sums(rx, w)
            r = cr.finish(bands, w)
            assert np.array_equal(r["st"], st), (r["st"], st)
            top = np.sort(r["CNodB"])[::-1]
            assert len(top) < 2 or top[0] - top[1] >= 1e-3, f"recording {k}: best two windows {top[:2]}"
            close = np.flatnonzero(np.abs(r["C"]) < 1e-4 * bands[:, 0]) * cr.HOP
            assert close.size == 0 or (k == 2 and close.size <= 1), f"recording {k}: windows {close} have |C| < 1e-4 S_c"
            if k == 2:
                d["skip2"] = close.astype(np.int64)
            d[f"rec{k}"] = s16; d[f"st{k}"] = st; d[f"cno{k}"] = cno; d[f"text{k}"] = text
            measured.append(m)
            print(f"recording {k}: {len(s16)} samples, window {w} s, {r['n_windows']} windows, {len(st)} printed; {text[-1]}")
        d["measured"] = np.stack(measured)
    np.savez_compressed(OUT, **d)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes")
    assert size < 400 * 1024
