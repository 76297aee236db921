"""Write tests/golden/clock_offset.npz: the reference's sample-clock offset, radae/dsp.py:564-575 sample_clock_offset (linear interpolation at tin = n (1 + ppm 1e-6),
tin accumulated in double), on one 2000-sample complex64 input for ppm = +100, -625 and the ppm of `sox -r 8000 .. -r 8020`.

Arrays: x complex64 [2000] (six tones in the modem's band, 700..2300 Hz, plus noise at -20 dB); ppm float64 [3]; y complex64 [3, 2000], the function's returns (zeros behind
the last output it produced); n int64 [3], the outputs it produced (its loop `while tin + 1 < len(tx) and tout < len(rx)`, replayed here with the same double additions).
The reference is imported without the n() and randint patches.
"""
import os

import numpy as np

from . import reference as R
from .reference import golden

N = 2000


def produced(n_in, ppm):
    tin, tout = 0, 0
    while tin + 1 < n_in and tout < n_in:
        tout += 1
        tin += 1 + ppm / 1E6
    return tout


def main(src, dst):
    R.enter(patched=False)
    from radae.dsp import sample_clock_offset
    OUT = golden(dst, "clock_offset.npz")
    rng = np.random.default_rng(20241018)
    t = np.arange(N)
    x = sum(np.exp(1j * (2 * np.pi * f / 8000.0 * t + ph)) for f, ph in zip((700, 1020, 1340, 1660, 1980, 2300), rng.uniform(0, 2 * np.pi, 6))) / 6.0
    x = (x + 0.1 * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) / np.sqrt(2)).astype(np.complex64)
    ppm = np.array([100.0, -625.0, (8000.0 / 8020.0 - 1.0) * 1e6])
    y = np.stack([sample_clock_offset(x, p) for p in ppm])
    n = np.array([produced(N, p) for p in ppm], np.int64)
    assert y.dtype == np.complex64 and y.shape == (3, N)
    for k in range(3):
        assert np.all(y[k, n[k]:] == 0) and (n[k] == N or n[k] < N) and np.count_nonzero(y[k, :n[k]]) == n[k]
    np.savez_compressed(OUT, x=x, ppm=ppm, y=y, n=n)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; outputs produced {n.tolist()} for ppm {ppm.tolist()}")
