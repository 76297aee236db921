"""NumPy reference of the sound-card wire (rade_batch_wire_in / rade_batch_wire_out, include/rade_batch.h): both directions and the meters.

In range it is radae_amd/wire.py's arithmetic (int16tof32.py:40-50, f32toint16.py:42-54): `astype(float32)` one way, one float32 multiply and `astype(int16)` (C
truncation) the other way.  Out of range -- where `astype(int16)` gives whatever the platform gives -- it is the header's rule: NaN -> 0, v >= 32768 -> 32767,
v <= -32769 -> -32768 (a value in (-32769, -32768) truncates to -32768 and fits).  The meters are taken over the written components in float64: the largest |v|
before saturation, the sum of v^2 (every square exact in float64, added by math.fsum: the correctly rounded sum, so that a bound on a device's sum counts the
device's additions alone), the components that saturated and the NaN ones (counted, and in neither the peak nor the sum)."""
import math

import numpy as np

# what does not fit, what is special and what sits on the edges; the float32 literals are rounded by numpy as the test's inputs are
HAND = np.array([32767.0, -32767.0, 32767.99, -32767.99, 32768.0, -32768.0, -32768.99, -32769.0, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.0, -0.0,
                 1e-40, -1e-40, 0.99999994, -0.99999994, 1.0, -1.0, 1.5, -1.5], np.float32)
HAND_I16 = np.array([32767, -32767, 32767, -32767, 32767, -32768, -32768, -32768, 32767, -32768, 32767, -32768, 0, 0, 0,
                     0, 0, 0, 0, 1, -1, 1, -1], np.int16)        # written down by hand from the rule, not computed
HAND_CLIPPED, HAND_NAN = 6, 1                                    # 32768, -32769, +-1e9, +-inf saturate (-32768.0 and -32768.99 fit); one NaN


def int16_to_c64(s, iq=False, gain=1.0):
    """s int16 [..., n] (real) or [..., n, 2] (iq) -> complex64 [..., n]: (gain s, +0) or (gain I, gain Q), one float32 multiply per component"""
    f = np.float32(gain) * np.asarray(s, np.int16).astype(np.float32)
    out = np.zeros(f.shape[:-1] if iq else f.shape, np.complex64)
    if iq:
        out.real, out.imag = f[..., 0], f[..., 1]
    else:
        out.real = f                                             # the imaginary part stays the +0.0 of np.zeros
    return out


def fits(v):
    """float32 values whose truncation is an int16"""
    v = np.asarray(v, np.float32)
    return (v > np.float32(-32769.0)) & (v < np.float32(32768.0))


def c64_to_int16(x, scale=32767.0, real=True):
    """x complex64 [n] -> (int16 [n] (real: the I component) or [n, 2], meters dict) -- one stream"""
    x = np.ascontiguousarray(x, np.complex64)
    f = x.view(np.float32).reshape(-1, 2)
    v = (f[:, 0] if real else f) * np.float32(scale)             # float32 times float32: rounded once
    nan = np.isnan(v)
    ok = fits(v)
    out = np.zeros(v.shape, np.int16)
    out[ok] = v[ok].astype(np.int16)                             # wire.py's conversion where it is defined
    out[~nan & (v >= np.float32(32768.0))] = 32767
    out[~nan & (v <= np.float32(-32769.0))] = -32768
    w = v[~nan].astype(np.float64)
    meters = {"peak": float(np.abs(w).max()) if w.size else 0.0, "sum2": math.fsum(w * w) if np.isfinite(w).all() else float("inf"),
              "clipped": int(np.sum(~nan & ~ok)), "nan": int(nan.sum()), "components": int(v.size)}
    return out, meters
