"""The staging lifetime of the front-end stage calls (radae_amd/csrc/rade_stages.c): a call's pinned per-stream records, its cached table and its read-back area are
shared by every later call of that stage on the engine, so a call may refill them only once the device has read what the call before it put there.

Every test issues one short sequence of calls twice, each time on a fresh engine (a stage's first use and its lazy allocations happen inside the test) and on a torch
stream other than the default one: once with torch.cuda.synchronize() after every call -- the pattern the per-stage tests pin to their float64 restatements -- and once
with no synchronise until the end.  All outputs must be equal bit for bit.  B = 3, the per-stream counts differ between streams and between consecutive calls, and one
stream has no sample (for C/No, which refuses less than a window: no window) in one of the calls."""
import numpy as np
import pytest

from gpu_kit import crandn, dev, torch_dev  # noqa: F401

pytestmark = pytest.mark.gpu
B = 3
WIRE_CALLS = 17                  # 2 x RD_WIRE_SLOTS + 1: every slot of the wire's ring is used again twice


def cmp_bits(a):
    """what np.array_equal compares: int16 as it is, everything else as the integers of its bytes"""
    a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)
    if a.dtype == np.int16:
        return a
    return a.view(np.int64 if a.dtype.itemsize == 8 and a.dtype.kind != "c" else np.int32)


def run(calls, wait):
    """the calls, each eng -> a tuple of outputs (device tensors, host arrays or None), on a fresh engine and a side stream; wait: synchronise after every call"""
    import torch
    from radae_amd.engine import BatchEngine
    eng = BatchEngine(B, max_tx_mf=1)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()                         # the inputs were made on the default stream
    outs = []
    try:
        with torch.cuda.stream(side):
            for call in calls:
                outs.append(call(eng))
                if wait:
                    torch.cuda.synchronize()
        torch.cuda.synchronize()
        return [[None if v is None else cmp_bits(v) for v in o] for o in outs]
    finally:
        eng.close()


def same_both_ways(calls):
    a, b = run(calls, True), run(calls, False)
    assert len(a) == len(b) == len(calls)
    for k, (oa, ob) in enumerate(zip(a, b)):
        assert len(oa) == len(ob)
        for j, (va, vb) in enumerate(zip(oa, ob)):
            assert (va is None) == (vb is None), (k, j)
            assert va is None or (va.shape == vb.shape and np.array_equal(va, vb)), f"call {k}, output {j}"
    return a


def wire_counts(k):
    n = np.array([(7 * k + 5) % 65, (11 * k + 3) % 65, (13 * k + 1) % 65], np.int32)
    if k == 4:
        n[1] = 0
    return n


def test_wire_in_wraps_the_slot_ring(torch_dev):
    rng = np.random.default_rng(101)
    x = [dev(rng.integers(-32768, 32768, (B, 64), dtype=np.int16), torch_dev) for _ in range(WIRE_CALLS)]
    out = same_both_ways([lambda eng, k=k: (eng.wire_in(x[k], n=wire_counts(k), gain=1.0 + k),) for k in range(WIRE_CALLS)])
    for k in range(WIRE_CALLS):                      # the counts reached the device: a row holds its n samples and zeros behind them
        got = out[k][0].view(np.complex64)
        for b, n in enumerate(wire_counts(k)):
            assert np.array_equal(got[b, :n], (x[k][b, :n].cpu().numpy() * np.float32(1.0 + k)).astype(np.complex64)) and not got[b, n:].any()


def test_wire_out_wraps_the_slot_ring(torch_dev):
    rng = np.random.default_rng(102)
    x = [dev(0.4 * crandn(rng, B, 64), torch_dev) for _ in range(WIRE_CALLS)]

    def call(eng, k):
        r = eng.wire_out(x[k], n=wire_counts(k), real=k % 2 == 0, meters=k >= WIRE_CALLS - 3)
        return (r[0],) + tuple(r[1]) if k >= WIRE_CALLS - 3 else (r,)
    out = same_both_ways([lambda eng, k=k: call(eng, k) for k in range(WIRE_CALLS)])
    for k in range(WIRE_CALLS):
        for b, n in enumerate(wire_counts(k)):
            assert out[k][0][b, :n].any() == (n > 0) and not out[k][0][b, n:].any()


def test_resample_back_to_back(torch_dev):
    rng = np.random.default_rng(103)
    x = dev(crandn(rng, B, 400), torch_dev)
    ppm = [[-2493.77, 100.0, 0.0], [50.0, -50.0, 2500.0], [0.0, 1.0, -1.0]]
    t0 = [[0.0, 0.5, 3.25], [1.0, 0.0, 0.125], [2.5, 2.5, 0.0]]
    n_out = [[380, 201, 97], [33, 0, 350], [256, 377, 1]]
    same_both_ways([lambda eng, k=k: eng.resample(x, ppm[k], t0[k], n_out=n_out[k]) for k in range(3)])


def test_rate_convert_changes_its_table(torch_dev):
    rng = np.random.default_rng(104)
    x = dev(crandn(rng, B, 600), torch_dev)
    x16 = dev(rng.integers(-32768, 32768, (B, 600), dtype=np.int16), torch_dev)
    same_both_ways([lambda eng: eng.rate_convert(x, 1, 6, n_in=[600, 431, 77]),
                    lambda eng: eng.rate_convert(x16, 80, 441, n_in=[0, 600, 599], gain=1.0 / 32768),
                    lambda eng: eng.rate_convert(x, 1, 6, n_in=[91, 600, 318])])


def test_fm_mod_phases(torch_dev):
    rng = np.random.default_rng(105)
    m = dev(rng.uniform(-1, 1, (B, 300)).astype(np.float32), torch_dev)
    same_both_ways([lambda eng: eng.fm_mod(m, 48000.0, 12000.0, 5000.0, n=[300, 0, 123], phase0=[1, 0x80000000, 12345]),
                    lambda eng: eng.fm_mod(m, 48000.0, 12000.0, 5000.0, n=[17, 299, 300], phase0=[7, 8, 0xffffffff], want_phase=False),
                    lambda eng: eng.fm_mod(m, 48000.0, 12000.0, 5000.0, n=[250, 64, 1], phase0=0xdeadbeef, sigma=0.1, seed=9)])


def test_fm_demod_changes_its_taps(torch_dev):
    rng = np.random.default_rng(106)
    x = dev(crandn(rng, B, 300), torch_dev)
    taps = [(rng.standard_normal(5), rng.standard_normal(3)), (rng.standard_normal(9), [0.5])]
    same_both_ways([lambda eng: eng.fm_demod(x, 48000.0, 12000.0, 5000.0, *taps[0], n_in=[300, 150, 7], want_bb=True),
                    lambda eng: eng.fm_demod(x, 48000.0, 12000.0, 5000.0, *taps[1], n_in=[0, 300, 299], want_bb=True),
                    lambda eng: eng.fm_demod(x, 48000.0, 12000.0, 5000.0, *taps[0], n_in=[33, 300, 200], want_bb=True)])


def test_cno_est_changes_its_window(torch_dev):
    from radae_amd.engine import chirp
    rng = np.random.default_rng(107)
    x = dev(chirp(1.0)[None, :4400] + 0.05 * crandn(rng, B, 4400), torch_dev)

    def call(eng, wt, n):
        res, bands = eng.cno_est(x, n=n, window_time=wt, bands=True)
        return (np.array([[r.n_windows, r.n_positive, r.max_st, r.max_CNodB, r.max_SNRdB] for r in res], np.float64), bands)
    out = same_both_ways([lambda eng: call(eng, 0.25, [4400, 2000, 3999]),       # (2000 samples of a 2000-sample window: no window)
                          lambda eng: call(eng, 0.5, [4001, 4400, 4000]),
                          lambda eng: call(eng, 0.25, [2001, 4400, 4400])])
    assert [o[1].shape[1] for o in out] == [2, 1, 2]


def test_channel_rs_pa_sigmas_and_stats(torch_dev):
    rng = np.random.default_rng(108)
    z = dev(rng.standard_normal((B, 3, 80)).astype(np.float32), torch_dev)
    same_both_ways([lambda eng: (eng.channel_rs_pa(z, [0.5, 1.0, 2.0], seed=3),),
                    lambda eng: eng.channel_rs_pa(z, [4.0, 0.25, 0.0], seed=4, want_stats=True)])


def test_mixed_stages_on_one_engine(torch_dev):
    """resample, then rate, then fm_mod, then wire_out, each fed by the one before it: stages whose staging helpers share code"""
    rng = np.random.default_rng(109)
    x = dev(0.5 * crandn(rng, B, 400), torch_dev)
    kept = {}

    def resample(eng):
        kept["y"], kept["ny"] = eng.resample(x, [100.0, -2493.77, 0.0], [0.0, 1.5, 0.25], n_out=[390, 0, 211])
        return kept["y"], kept["ny"]

    def rate(eng):
        kept["r"], kept["nr"] = eng.rate_convert(kept["y"], 2, 3, n_in=kept["ny"])
        return kept["r"], kept["nr"]

    def mod(eng):
        kept["tx"], ph = eng.fm_mod(kept["r"], 8000.0, 1000.0, 500.0, n=kept["nr"], phase0=[1, 2, 3])
        return kept["tx"], ph

    def wire(eng):
        out, m = eng.wire_out(kept["tx"], n=kept["nr"], real=False, scale=16384.0, meters=True)
        return (out,) + tuple(m)
    out = same_both_ways([resample, rate, mod, wire])
    assert out[3][0][0].any() and not out[3][0][1].any()
