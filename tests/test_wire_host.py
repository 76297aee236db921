"""Host tests of the reference of the sound-card wire (tests/wire_ref.py; rade_batch_wire_in / rade_batch_wire_out): equal to radae_amd/wire.py and to the bytes the
reference scripts produced (tests/golden/wire.npz) wherever the conversion is defined, and the header's saturation / NaN / truncation rule on a hand-made vector."""
import numpy as np

import wire_ref as wr
from radae_amd import wire


def test_reference_equals_wire_py_and_the_reference_scripts_in_range(golden):
    g = golden("wire")
    i16 = np.frombuffer(g["i16"].tobytes()[: 4 * (len(g["i16"]) // 4)], np.int16)       # the scripts read 4 bytes at a time: the trailing odd int16 is theirs to drop
    assert wr.int16_to_c64(i16).tobytes() == g["i2f_zp"].tobytes() == wire.int16_to_f32(i16.tobytes(), zeropad=True)
    assert wr.int16_to_c64(i16.reshape(-1, 2), iq=True).tobytes() == g["i2f"].tobytes() == wire.int16_to_f32(i16.tobytes())
    x = np.frombuffer(g["f32"].tobytes(), np.complex64)
    for scale, key in ((32767.0, "f2i"), (8192.0, "f2i_scale")):
        ok = wr.fits(x.view(np.float32) * np.float32(scale)).reshape(-1, 2)
        assert ok.sum() > ok.size // 2                                                  # the comparison is not empty: most of the fixture fits (a fifth of it clips at 32767)
        both, m = wr.c64_to_int16(x, scale, real=False)
        assert np.array_equal(both[ok], np.frombuffer(g[key].tobytes(), np.int16).reshape(-1, 2)[ok])
        assert np.array_equal(both[ok], np.frombuffer(wire.f32_to_int16(x.tobytes(), scale), np.int16).reshape(-1, 2)[ok])
        assert m["clipped"] == int((~ok).sum()) and m["nan"] == 0
        re, _ = wr.c64_to_int16(x, scale, real=True)
        assert np.array_equal(re, both[:, 0])
        assert np.array_equal(re[ok[:, 0]], np.frombuffer(wire.f32_to_int16(x.tobytes(), scale, real=True), np.int16)[ok[:, 0]])
    ok = wr.fits(x.view(np.float32) * np.float32(32767.0)).reshape(-1, 2)[:, 0]
    assert np.array_equal(wr.c64_to_int16(x, 32767.0)[0][ok], np.frombuffer(g["f2i_real"].tobytes(), np.int16)[ok])
    # a random in-range signal at the radio's scale: every sample
    rng = np.random.default_rng(5)
    y = (rng.uniform(-3.99, 3.99, (4096, 2)).astype(np.float32)).view(np.complex64).ravel()
    assert wr.fits(y.view(np.float32) * np.float32(8192.0)).all()
    assert wr.c64_to_int16(y, 8192.0)[0].tobytes() == wire.f32_to_int16(y.tobytes(), 8192.0, real=True)
    assert wr.c64_to_int16(y, 8192.0, real=False)[0].tobytes() == wire.f32_to_int16(y.tobytes(), 8192.0)


def test_saturation_nan_and_truncation_on_the_hand_made_vector():
    x = (wr.HAND.astype(np.complex64) + 1j * np.float32(7.0)).astype(np.complex64)       # Q is in range and must not matter in real mode
    out, m = wr.c64_to_int16(x, 1.0, real=True)
    assert np.array_equal(out, wr.HAND_I16)
    assert (m["clipped"], m["nan"], m["components"]) == (wr.HAND_CLIPPED, wr.HAND_NAN, len(wr.HAND))
    assert m["peak"] == np.inf and m["sum2"] == np.inf
    both, m2 = wr.c64_to_int16(x, 1.0, real=False)
    assert np.array_equal(both[:, 0], wr.HAND_I16) and np.all(both[:, 1] == 7) and (m2["clipped"], m2["nan"]) == (wr.HAND_CLIPPED, wr.HAND_NAN)
    # the subnormal-times-scale case: a subnormal input whose product is a normal number far below 1, and a normal input whose product is subnormal
    tiny = np.array([1e-40, -1e-40, 2e-38, -2e-38], np.float32).astype(np.complex64)
    for scale in (32767.0, 1e-3):
        out, m = wr.c64_to_int16(tiny, scale)
        assert np.all(out == 0) and m["clipped"] == 0 and m["nan"] == 0 and 0.0 < m["peak"] < 1e-30
    # truncation toward zero, never rounding: just below one, one, one and a half, both signs; and the last float32 below 32768 at the largest scale
    assert list(wr.c64_to_int16(np.array([0.99999994, -0.99999994, 1.0, -1.0, 1.5, -1.5, 32767.998, -32768.998], np.float32).astype(np.complex64), 1.0)[0]) == \
        [0, 0, 1, -1, 1, -1, 32767, -32768]
    # without the infinities the meters are finite and exact
    fin = wr.HAND[np.isfinite(wr.HAND)].astype(np.complex64)
    _, m = wr.c64_to_int16(fin, 1.0)
    assert m["peak"] == 1e9 and m["clipped"] == 4 and m["nan"] == 0 and abs(m["sum2"] - 2e18) < 1e-6 * 2e18      # the two 1e9 carry the sum


def test_in_direction_signs_zero_and_gain():
    s = np.array([0, 1, -1, 32767, -32768], np.int16)
    z = wr.int16_to_c64(s)
    assert np.array_equal(z.view(np.uint32).reshape(-1, 2)[:, 1], np.zeros(5, np.uint32))       # Q is +0.0, bit for bit
    assert np.array_equal(z.real, s.astype(np.float32))
    assert np.array_equal(wr.int16_to_c64(s, gain=0.5).real, np.float32(0.5) * s.astype(np.float32))
