"""The reference of the device noise generator (seed != 0): Philox4x32-10, the two uniforms as the device forms them, Box-Muller in float64, and the counter
mapping of each of the four kernels that consume it.  numpy only, no GPU; holds no fixtures.  tests/test_device_noise_host.py checks this file against the
published known answers and the normal distribution; tests/test_device_noise_gpu.py holds the kernels to it sample by sample.

Philox4x32-10 is written from Salmon, Moraes, Dror and Shaw, "Parallel Random Numbers: As Easy as 1, 2, 3" (SC'11), section 3.3 and table 2: ten rounds of
    (c0, c1, c2, c3) <- (mulhi(M1, c2) ^ c1 ^ k0,  mullo(M1, c2),  mulhi(M0, c0) ^ c3 ^ k1,  mullo(M0, c0))
with the key (k0, k1) raised by the Weyl constants (W0, W1) ahead of every round but the first.

The mappings (key (seed & 0xffffffff, seed >> 32) everywhere; the third counter word tells the consumers apart):
    rate-Fs channel   k_chan_apply     counter (p, b, 0, 0)          one counter per PAIR of samples: words 0-1 -> sample 2p, words 2-3 -> sample 2p + 1
    symbol channel    k_chan_symbol    counter (i >> 1, 0, 0, 0)     i the flat index over the whole [B][n][80] call, NOT keyed by stream: words 0-1 only,
                                                                     g.x for even i, g.y for odd i
    Doppler generator k_multipath_gen  counter (xi, 2 b + p, 1, 0)   words 0-1 -> the complex low-rate input sample xi of path p of stream b
    rate-Rs channel   k_rs_pa          counter (i >> 1, b, 2, 0)     i = 20 s + c the carrier index inside the stream: words 0-1 -> even i, words 2-3 -> odd i
(the second word of the symbol channel and the fourth of the rate-Rs channel carry (i >> 1) >> 32, zero for every buffer that fits)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # the two multipliers of Philox4x32 (table 2)
W0, W1 = 0x9E3779B9, 0xBB67AE85            # the Weyl key increments: golden ratio, sqrt(3) - 1
MASK = np.uint64(0xFFFFFFFF)
# the bar of the device's gauss_pair against the float64 Box-Muller of the same uniforms (tests/test_device_noise_gpu.py states how it is used)
EPS_MEASURED = 7.093e-07   # largest |device - float64 reference| of gauss_pair over test_probe_gauss_pair's inputs on the MI355X: at u = (0x91b1, 0xc1765566), the sine
#                            component, reference -4.824733 (1.5 float32 ulps there); random pairs 7.093e-07, the crossed extremes 4.069e-07
EPS = 3e-6                 # 4 x EPS_MEASURED = 2.84e-06 rounded up to one digit; must stay <= 1e-4
# philox4x32-10 in the Random123 distribution's known-answer file: counter / key -> output
KNOWN_ANSWERS = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) under the key (k0, k1): arrays or scalars that broadcast, values below 2^32.  Four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
        p0 = np.uint64(M0) * c0             # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def uniforms(u0, u1):
    """The device's two uniforms, in float32 exactly as it forms them: (float32(u) + 0.5) 2^-32.  float32(u) rounds to nearest-even for u >= 2^24 and the
    sum rounds again: both are part of the definition.  a = 1.0 (u0 >= 0xffffff80) and bq = 1.0 are reachable, a = 0 is not (u = 0 gives 2^-33)."""
    h, s = np.float32(0.5), np.float32(2.0 ** -32)
    a = (np.asarray(u0, dtype=np.uint32).astype(np.float32) + h) * s
    bq = (np.asarray(u1, dtype=np.uint32).astype(np.float32) + h) * s
    return a, bq


def gauss_pair(u0, u1):
    """Box-Muller in float64 from those float32 uniforms: (rad cos 2 pi bq, rad sin 2 pi bq), rad = sqrt(-2 ln a).  Unit variance per component."""
    a, bq = uniforms(u0, u1)
    rad = np.sqrt(-2.0 * np.log(a.astype(np.float64)))
    ang = 2.0 * np.pi * bq.astype(np.float64)
    return rad * np.cos(ang), rad * np.sin(ang)


def _key(seed):
    seed = int(seed)
    assert 0 < seed < 1 << 64
    return seed & 0xFFFFFFFF, seed >> 32


def chan_fs(seed, B, n_pre, n_sig, n_eoo, n_post):
    """Unit-sigma noise of the rate-Fs channel (k_chan_apply) -> complex128 [B, n_pre + n_sig + n_eoo + n_post].  Inside the signal and the end-of-over frame
    the sample is complex with 1/2 per component, g / sqrt(2); in n_pre and n_post it is real-valued with the full sigma on the real part, (g.x, 0)
    (inference.py:277-284)."""
    k0, k1 = _key(seed)
    n_total = n_pre + n_sig + n_eoo + n_post
    n_pairs = (n_total + 1) // 2
    p = np.arange(n_pairs, dtype=np.uint64)[None, :]
    b = np.arange(B, dtype=np.uint64)[:, None]
    r = philox4x32_10(p, b, 0, 0, k0, k1)
    gx, gy = np.empty((B, 2 * n_pairs)), np.empty((B, 2 * n_pairs))
    for half in range(2):
        gx[:, half::2], gy[:, half::2] = gauss_pair(r[2 * half], r[2 * half + 1])
    gx, gy = gx[:, :n_total], gy[:, :n_total]
    j = np.arange(n_total)
    inside = ((j >= n_pre) & (j < n_pre + n_sig + n_eoo))[None, :]
    return np.where(inside, gx / np.sqrt(2.0), gx) + 1j * np.where(inside, gy / np.sqrt(2.0), 0.0)


def chan_symbol(seed, n_real, mode):
    """Unit-sigma noise of the symbol channel (k_chan_symbol) -> float64 [n_real], n_real = B n 80 the flat size of the whole call: the draw is not keyed by
    stream.  mode "rs": the components of complex symbols, 1/2 each (g / sqrt(2)); mode "bbfm": real symbols of unit variance."""
    k0, k1 = _key(seed)
    q = np.arange((n_real + 1) // 2, dtype=np.uint64)
    r = philox4x32_10(q & MASK, q >> np.uint64(32), 0, 0, k0, k1)
    x, y = gauss_pair(r[0], r[1])
    g = np.stack([x, y], axis=1).ravel()[:n_real]
    return g / np.sqrt(2.0) if mode == "rs" else g


def chan_rs(seed, B, n_steps):
    """Unit-sigma noise of the rate-Rs channel (k_rs_pa) in z_hat's layout -> float64 [B, n_steps, 80]: carrier c of symbol s (i = 20 s + c inside the stream) is the
    complex g / sqrt(2) at floats 40 s + 2 c (real) and 40 s + 2 c + 1 (imaginary)."""
    k0, k1 = _key(seed)
    n_car = 2 * n_steps * 20                                   # always even
    q = np.arange(n_car // 2, dtype=np.uint64)[None, :]
    b = np.arange(B, dtype=np.uint64)[:, None]
    r = philox4x32_10(q & MASK, b, 2, q >> np.uint64(32), k0, k1)
    out = np.empty((B, n_car, 2), np.float64)
    for half in range(2):
        x, y = gauss_pair(r[2 * half], r[2 * half + 1])
        out[:, half::2, 0] = x
        out[:, half::2, 1] = y
    return (out / np.sqrt(2.0)).reshape(B, n_steps, 80)


def multipath_low(seed, B, n_low, n_taps):
    """The low-rate input noise of the Doppler generator (k_multipath_gen) -> complex64 [B, 2, n_low + n_taps], the array `noise_low` takes: unit variance
    per component, sample xi of path p of stream b from words 0-1 of counter (xi, 2 b + p, 1, 0)."""
    k0, k1 = _key(seed)
    xi = np.arange(n_low + n_taps, dtype=np.uint64)[None, :]
    bp = np.arange(2 * B, dtype=np.uint64)[:, None]
    r = philox4x32_10(xi, bp, 1, 0, k0, k1)
    x, y = gauss_pair(r[0], r[1])
    return (x + 1j * y).astype(np.complex64).reshape(B, 2, n_low + n_taps)
