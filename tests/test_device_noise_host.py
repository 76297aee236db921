"""The reference of the device noise generator (tests/noise_ref.py) against what is published: the known answers of Philox4x32-10 (the Random123
distribution's kat_vectors, the three philox4x32-10 lines) and the normal distribution.  No GPU: tests/test_device_noise_gpu.py pins the kernels to this
reference sample by sample, so the distribution checked here is the device's."""
import numpy as np
import pytest

import noise_ref as nr

KAT = nr.KNOWN_ANSWERS


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = nr.philox4x32_10(*ctr, *key)
        assert [int(w) for w in got] == list(want), [hex(int(w)) for w in got]
    # vectorised over counters and keys: the three at once
    c = np.array([k[0] for k in KAT], np.uint64).T
    k = np.array([k[1] for k in KAT], np.uint64).T
    got = np.stack(nr.philox4x32_10(*c, *k), axis=1)
    assert got.dtype == np.uint32 and np.array_equal(got, np.array([k[2] for k in KAT], np.uint32))


def test_uniforms_are_the_device_float32_values():
    a, bq = nr.uniforms(np.uint32([0, 1, 1 << 24, (1 << 24) + 1, 0xffffff7f, 0xffffff80, 0xffffffff]), np.uint32([0, 0, 0, 0, 0, 0, 0xffffffff]))
    assert a.dtype == np.float32 and bq.dtype == np.float32
    assert a[0] == np.float32(2.0 ** -33) and a[1] == np.float32(1.5 * 2.0 ** -32)
    assert a[2] == np.float32(2.0 ** -8)                          # 2^24 + 0.5 ties to even: 2^24
    assert a[3] == np.float32(2.0 ** -8)                          # float32(2^24 + 1) is already 2^24
    assert a[4] < 1.0 and a[5] == 1.0 and a[6] == 1.0             # a = 1 is reachable (the top 128 words), a = 0 is not
    assert bq[-1] == 1.0 and a.min() > 0.0


@pytest.fixture(scope="module")
def sample():
    """key (1234, 0), counters (0 .. 2^20 - 1, 0, 0, 0), both Gaussian pairs of every counter: [2 pairs][2 components][2^20]"""
    r = nr.philox4x32_10(np.arange(1 << 20), 0, 0, 0, 1234, 0)
    g = np.array([nr.gauss_pair(r[0], r[1]), nr.gauss_pair(r[2], r[3])])
    g.setflags(write=False)
    return g


def test_reference_distribution(sample):
    from math import sqrt
    from scipy import stats
    v = sample.ravel()
    n, N = v.size, sample.shape[2]
    assert n == 4194304
    mean, var = v.mean(), v.var()
    kurt = np.mean((v - mean) ** 4) / var ** 2 - 3.0
    ks = stats.kstest(v, "norm").statistic
    tail = np.mean(np.abs(v) > 3.0)
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} excess kurtosis {kurt:.3e} KS {ks:.3e} (bar {1.95 / sqrt(n):.3e}) P(|v|>3) {tail:.7f} max|v| {np.abs(v).max():.3f}")
    assert abs(mean) <= 5 / sqrt(n)
    assert abs(var - 1) <= 5 * sqrt(2 / n)
    assert abs(kurt) <= 5 * sqrt(96 / n)
    for p in range(2):                                            # g.x against g.y of one pair
        assert abs(np.corrcoef(sample[p, 0], sample[p, 1])[0, 1]) <= 5 / sqrt(N)
    for cx in range(2):                                           # pair 0 (words 0-1) against pair 1 (words 2-3)
        for cy in range(2):
            assert abs(np.corrcoef(sample[0, cx], sample[1, cy])[0, 1]) <= 5 / sqrt(N)
    assert ks < 1.95 / sqrt(n)
    assert abs(tail / 0.0026998 - 1) <= 0.05


def test_reference_extremes():
    lo, hi = np.uint32(0), np.uint32(0xffffffff)
    x, y = nr.gauss_pair(lo, lo)                                  # a = 2^-33: the largest radius; bq = 2^-33 revolutions
    assert abs(np.hypot(x, y) - np.sqrt(66 * np.log(2))) < 1e-12
    x, y = nr.gauss_pair(hi, np.uint32(12345))                    # a = 1: exactly zero
    assert x == 0.0 and y == 0.0
    x, y = nr.gauss_pair(lo, hi)                                  # bq = 1: a whole revolution
    assert abs(x - np.sqrt(66 * np.log(2))) < 1e-12 and abs(y) < 1e-14
    e = np.uint32([0, 1, 1 << 24, (1 << 24) + 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff])
    x, y = nr.gauss_pair(*np.meshgrid(e, e))
    assert np.isfinite(x).all() and np.isfinite(y).all()


def test_consumer_layouts():
    """each consumer's array is the stated words of the stated counter: a few samples spelled out by hand"""
    seed = (7 << 32) + 5
    key = (5, 7)
    a = nr.chan_fs(seed, 3, 3, 4, 0, 2)                           # n_total 9: pairs 0..4, the last feeds one sample
    assert a.shape == (3, 9)
    for b, j in ((0, 0), (2, 1), (1, 2), (1, 3), (2, 6), (0, 7), (1, 8)):
        r = nr.philox4x32_10(j // 2, b, 0, 0, *key)
        x, y = nr.gauss_pair(r[2 * (j & 1)], r[2 * (j & 1) + 1])
        want = complex(x / np.sqrt(2), y / np.sqrt(2)) if 3 <= j < 7 else complex(x, 0.0)
        assert a[b, j] == want, (b, j)
    s = nr.chan_symbol(seed, 11, "rs"); f = nr.chan_symbol(seed, 11, "bbfm")
    assert s.shape == (11,) and np.array_equal(s * np.sqrt(2.0), f)
    for i in (0, 1, 6, 9, 10):
        r = nr.philox4x32_10(i // 2, 0, 0, 0, *key)
        assert f[i] == nr.gauss_pair(r[0], r[1])[i & 1], i
    # one seed: the symbol channel draws the words of stream 0 of the rate-Fs channel (third counter word 0 in both)
    assert np.array_equal(nr.chan_symbol(seed, 8, "rs")[0::2], nr.chan_fs(seed, 1, 0, 8, 0, 0)[0, 0::2].real)
    z = nr.chan_rs(seed, 2, 3)
    assert z.shape == (2, 3, 80)
    for b, i in ((0, 0), (1, 1), (1, 20), (0, 63), (1, 119)):
        r = nr.philox4x32_10(i // 2, b, 2, 0, *key)
        x, y = nr.gauss_pair(r[2 * (i & 1)], r[2 * (i & 1) + 1])
        assert np.array_equal(z[b].ravel()[2 * i:2 * i + 2], np.array([x, y]) / np.sqrt(2)), (b, i)
    m = nr.multipath_low(seed, 2, 4, 3)
    assert m.shape == (2, 2, 7) and m.dtype == np.complex64
    for b, p, xi in ((0, 0, 0), (0, 1, 6), (1, 0, 3), (1, 1, 1)):
        r = nr.philox4x32_10(xi, 2 * b + p, 1, 0, *key)
        x, y = nr.gauss_pair(r[0], r[1])
        assert m[b, p, xi] == np.complex64(x + 1j * y)
    # the four consumers draw different words from one seed, except the pair stated above
    assert not np.array_equal(z[0].ravel()[:8], nr.chan_fs(seed, 1, 0, 4, 0, 0)[0].view(np.float64))
