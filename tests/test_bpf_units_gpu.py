"""GPU unit tests (-m gpu) of the streaming band-pass filter: rd_launch_bpf alone (k_bpf_chain + k_bpf_fir [+ k_bpf_advance] of radae_amd/csrc/rade_rx.hip) on synthetic
streams, then the three doors it is reached through -- the receiver's pre-pass and rx2_bpf_own behind BatchEngine.rx, and the transmit filter + clip of an engine opened
with RADE_BATCH_TX_BPF.  Every sample is held to the float64 model of tests/bpf_ref.py under its counted per-sample bound EPS sum |h| |w| + TINY X (tests/test_bpf_ref_host.py
shows that the check rejects a dropped plane product, a wrong delay, a neighbour's phase and a shifted memory); the phase chain and the state k_bpf_advance leaves are
held bit for bit.  The model filters with the float32 taps the kernels read (rd_tables_fill).

Inputs, outputs, states and the chain sit in NaN-sentinel buffers at odd strides, and every launch checks: the inputs unchanged; nothing written outside
y[b][0, avail[b]); all of that written; no NaN in it (no sentinel was read); grid_off 0; zero_acc / zero_progress cleared when given; the state record untouched when
advance = 0; the chain's entries and nothing behind them.  Each case prints its largest |dy| / bound.

Shapes: B 3 or 4, at most 17 blocks (the third workgroup of a stream: 8 blocks per workgroup)."""
import ctypes as C

import numpy as np
import pytest

import bpf_ref as M
import dev_abi
import tx_ref as tx
from gpu_kit import stream, sync, torch_dev  # noqa: F401
from kernel_ref import SENT32, U
from trace_ref import edge_case_input

pytestmark = pytest.mark.gpu

GUARD = 64                      # words of sentinel on either side of every buffer
ISENT = 0x7F0F0F0F              # sentinel of the integer buffers


@pytest.fixture(scope="module")
def L(torch_dev):
    return dev_abi.load()


@pytest.fixture(scope="module")
def tabs(L, torch_dev):
    """(device rd_tables of an engine, the binary16 tap table built on the host and uploaded, its host words); the model is given the taps the kernels read"""
    import torch
    from radae_amd.engine import BatchEngine
    eng = BatchEngine(3, max_tx_mf=1)
    dtab = L.rd_batch_tables(eng.h)
    assert dtab
    h_lib, E_lib, t16 = M.host_tables(L)
    tx.check_bits(E_lib, M.design()[2], "bpf_E", ("entry", "component"))
    M.use_taps(h_lib)
    d16 = torch.from_numpy(t16.view(np.int16).copy()).to(torch_dev)
    assert d16.data_ptr() % 16 == 0
    yield dtab, d16, t16
    M.use_taps(None)
    eng.close()


def crand(rng, n, scale=0.5):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)


def fresh():
    """the record of a stream before its first call"""
    return dict(mem=np.zeros(M.MEM, np.complex64), mem_len=100, phase=np.complex64(1))


def carried(rng, scale=0.5):
    return dict(mem=crand(rng, M.MEM, scale), mem_len=102, phase=M.design()[2][int(rng.integers(0, 1152))])


class Buf:
    """a flat word buffer between two guards, sentinel-filled, on the device"""

    def __init__(self, dev, n_words, sent=SENT32):
        import torch
        self.host = np.full(n_words + 2 * GUARD, sent, np.uint32)
        self.n, self.dev, self.t, self.torch = n_words, dev, None, torch

    @property
    def w(self):
        return self.host[GUARD:GUARD + self.n]

    def up(self):
        self.t = self.torch.from_numpy(self.host.view(np.int32).copy()).to(self.dev)
        assert self.t.data_ptr() % 16 == 0
        return self.t.data_ptr() + 4 * GUARD

    def down(self):
        got = self.t.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:GUARD], self.host[:GUARD]) and np.array_equal(got[-GUARD:], self.host[-GUARD:]), "a guard was written"
        return got[GUARD:GUARD + self.n]


def n_blocks_of(len0, avail):
    return len(M.blocks_of(len0, avail)) if len0 > 0 else 0


def run_bpf(L, dev, tabs, streams, len0, clip=0, advance=0, strided=False, generous=False, zero=True, avail_const=False, what=""):
    """One rd_launch_bpf.  streams: dicts x (complex64, avail samples), mem, mem_len, phase [, len0: the stream's own, strided form only].  Checks the launch's
    contract (module docstring) and returns y [B] complex64, the records after it, the chain [B] complex64."""
    dtab, d16, t16 = tabs
    B = len(streams)
    l0 = [int(s.get("len0", len0)) for s in streams]
    assert strided or len(set(l0)) == 1
    av = [len(s["x"]) for s in streams]
    nmax = max(av + [1])
    nb = max([n_blocks_of(l, a) for l, a in zip(l0, av)] + [1])
    if generous:
        nb = 2 + (nmax - 1) // 800
    cs = nb + 3 + (2 if generous else 0)
    xs, ys = nmax + 3, nmax + 5                                           # odd strides (in samples) when nmax is even, never equal
    srec = C.sizeof(M.BpfState)
    sstride = srec + (24 if strided else 0)
    x, y, st, ch = Buf(dev, 2 * B * xs + 2), Buf(dev, 2 * B * ys + 2), Buf(dev, B * sstride // 4), Buf(dev, 2 * B * cs)
    l0b, avb, acc, prog = Buf(dev, 3 * B, ISENT), Buf(dev, B, ISENT), Buf(dev, 4 * B, ISENT), Buf(dev, 4, ISENT)
    for b, s in enumerate(streams):
        x.w[2 + 2 * b * xs:2 + 2 * (b * xs + av[b])] = np.ascontiguousarray(s["x"], np.complex64).view(np.uint32)
        r = st.w[b * sstride // 4:b * sstride // 4 + srec // 4]
        r[0], r[1] = s["mem_len"], 5
        r[2:4] = np.array([s["phase"]], np.complex64).view(np.uint32)
        r[4:] = np.ascontiguousarray(s["mem"], np.complex64).view(np.uint32)
        l0b.w[3 * b] = np.int32(l0[b]).view(np.uint32)
        avb.w[b] = av[b]
    a = M.BpfArgs()
    a.state, a.state_stride = st.up(), sstride
    if strided:
        a.len0, a.len0_stride = l0b.up(), 12
    else:
        a.len0_const = l0[0]
    if avail_const:
        assert len(set(av)) == 1
        a.avail_const = av[0]
    else:
        a.avail = avb.up()
    a.tab, a.bpf16 = dtab, d16.data_ptr()
    a.x, a.x_stride, a.y, a.y_stride = x.up() + 8, xs, y.up() + 8, ys
    a.chain, a.chain_stride, a.n_blocks, a.B, a.clip, a.advance = ch.up(), cs, nb, B, clip, advance
    if zero:
        a.zero_acc, a.zero_progress = acc.up(), prog.up()
    assert L.rd_launch_bpf(C.byref(a), stream()) == 0
    sync()
    # the inputs
    assert np.array_equal(x.down(), x.w), f"{what}: x was written"
    assert np.array_equal(d16.cpu().numpy().view(np.uint16), t16), f"{what}: the tap table was written"
    if strided:
        assert np.array_equal(l0b.down(), l0b.w), f"{what}: len0 was written"
    if not avail_const:
        assert np.array_equal(avb.down(), avb.w), f"{what}: avail was written"
    if zero:
        assert not acc.down().any() and not prog.down().any(), f"{what}: zero_acc / zero_progress not cleared"
    # y: all of [0, avail) of a stream with len0 > 0, nothing else
    yw, mask = y.down(), np.zeros(y.n, bool)
    out = []
    for b in range(B):
        n = av[b] if l0[b] > 0 else 0
        seg = slice(2 + 2 * b * ys, 2 + 2 * (b * ys + n))
        mask[seg] = True
        assert not (yw[seg] == SENT32).any(), f"{what}: stream {b}: {int((yw[seg] == SENT32).sum())} words of y[0, {n}) not written"
        out.append(yw[seg].copy().view(np.complex64))
        assert not np.isnan(out[-1].view(np.float32)).any(), f"{what}: stream {b}: a NaN in y (a sentinel was read)"
    bad = np.flatnonzero(~mask & (yw != SENT32))
    assert bad.size == 0, f"{what}: {bad.size} words written outside y[b][0, avail), the first at word {int(bad[0]) - 2} (stride {2 * ys})"
    # the chain
    cw, cmask = ch.down(), np.zeros(ch.n, bool)
    chains = []
    for b, s in enumerate(streams):
        want = M.chain(s["phase"], l0[b], av[b], cs)
        k = slice(2 * b * cs, 2 * b * cs + 2 + 2 * len(want))
        cmask[k] = True
        assert cw[k][0] == np.int32(l0[b]).view(np.uint32) and cw[k][1] == s["mem_len"], f"{what}: stream {b}: chain header"
        tx.check_bits(cw[k][2:].view(np.complex64), want, f"{what}: stream {b}: block phases", ("block", "component"))
        chains.append(want)
    assert not (~cmask & (cw != SENT32)).any(), f"{what}: chain entries written behind the first block beyond the input"
    # the records
    sw, recs = st.down(), []
    for b, s in enumerate(streams):
        r = sw[b * sstride // 4:b * sstride // 4 + srec // 4]
        assert r[1] == 0, f"{what}: stream {b}: grid_off not cleared"
        if not advance:
            assert np.array_equal(r[[0, *range(2, srec // 4)]], st.w[b * sstride // 4:b * sstride // 4 + srec // 4][[0, *range(2, srec // 4)]]), f"{what}: stream {b}: state written with advance = 0"
        assert (sw[b * sstride // 4 + srec // 4:(b + 1) * sstride // 4] == SENT32).all(), f"{what}: words between the state records written"
        recs.append(dict(mem=r[4:].copy().view(np.complex64), mem_len=int(r[0]), phase=r[2:4].copy().view(np.complex64)[0]))
    return out, recs, chains


def hold(y, streams, len0, clip, what):
    """every stream's samples against the model under the bound; prints and returns the largest |dy| / bound"""
    worst = 0.0
    for b, s in enumerate(streams):
        l0 = int(s.get("len0", len0))
        if l0 <= 0 or len(s["x"]) == 0:
            assert len(y[b]) == 0
            continue
        want, bound, _ = M.run(s["x"], M.blocks_of(l0, len(s["x"])), M.State(s["mem"][:s["mem_len"]], s["phase"]), do_clip=bool(clip))
        worst = max(worst, tx.check_close(y[b], want, bound, f"{what}: stream {b} (len0 {l0}, avail {len(s['x'])}, mem_len {s['mem_len']})", ("sample",)))
    print(f"{what}: largest |dy| / bound = {worst:.3f}")
    return worst


def check_state32(rec, s, len0, what):
    """the record after advance = 1 against the float32 state model, bit for bit"""
    m, ml, p = M.state32(s["x"], len0, len(s["x"]), s["mem"], s["mem_len"], s["phase"])
    assert rec["mem_len"] == ml, f"{what}: mem_len {rec['mem_len']}, model {ml}"
    tx.check_bits(np.array([rec["phase"]]), np.array([p]), f"{what}: phase", ("", "component"))
    tx.check_bits(rec["mem"], m, f"{what}: mem", ("sample", "component"))


# ================================================================================================================================================================
# 1. the partition
# ================================================================================================================================================================
def avails(len0):
    return [0, 1, 101, 102, 103, 255, 256, 257, len0, len0 + 37, len0 + 960, len0 + 7 * 960 + 5, len0 + 8 * 960 + 5, len0 + 16 * 960 + 300]


@pytest.mark.parametrize("strided", [False, True], ids=["const", "strided"])
@pytest.mark.parametrize("len0", [800, 960, 1120, 1152])
def test_partition(L, torch_dev, tabs, len0, strided):
    """Every avail of the issue's list for this first block length: nothing, one sample, around the memory length, around a tile, a partial only block, whole blocks, a
    partial block shorter than the memory, the last block of the first workgroup, the first of the second (head recomputed from x and the chain), the third workgroup.
    Four streams a launch, fresh and carried states alternating; n_blocks as the caller computes it and as the receiver's generous 2 + (max - 1) / 800, in turn.  The
    strided form (the receiver's: len0 and the record at strides larger than they are) carries one more stream with len0 <= 0, which writes nothing."""
    rng = np.random.default_rng(len0 + strided)
    av = avails(len0)
    groups = [av[0:4], av[4:8], av[8:11], av[11:14]]
    worst = 0.0
    for g, grp in enumerate(groups):
        streams = [dict(x=crand(rng, n), **(fresh() if (i + g) % 2 else carried(rng))) for i, n in enumerate(grp)]
        if strided:
            streams += [dict(x=crand(rng, 300), len0=0 if g % 2 else -960, **carried(rng))] if len(streams) == 3 else []
        what = f"len0 {len0} {'strided' if strided else 'const'} avail {grp}"
        y, _, _ = run_bpf(L, torch_dev, tabs, streams, len0, strided=strided, generous=bool(g % 2), zero=bool(g % 2) != strided, what=what)
        worst = max(worst, hold(y, streams, len0, 0, what))


def test_short_first_block(L, torch_dev, tabs):
    """A first block shorter than the 102-sample memory followed by another: the hand-over keeps the end of the block's own memory (no caller of the engine's makes
    such a block; the kernel is correct for it all the same).  avail_const form."""
    rng = np.random.default_rng(5)
    for len0 in (2, 50, 101, 102, 103):
        streams = [dict(x=crand(rng, len0 + 960 + 70), **(carried(rng) if b else fresh())) for b in range(3)]
        y, _, _ = run_bpf(L, torch_dev, tabs, streams, len0, avail_const=True, what=f"short first block {len0}")
        hold(y, streams, len0, 0, f"short first block {len0}")


def test_partial_block_is_the_block_padded_with_zeros(L, torch_dev, tabs):
    """A partial last block is staged with zeros behind its samples, so it gives the bits of the same samples followed by zeros to a whole block -- in y and in the
    block's scale.  The clamped loads behind a partial block all return its last sample; were they staged, the outputs would stay (no output below n reaches them)
    but the block's maximum would follow them.  So the last sample is the block's largest, modulus 2.6, turned so that its own baseband components are 1.84 each
    (below 2) while a copy under another block phase reaches 2.6: the scale would move a binade and the bits with it.  A partial first block and a partial second one."""
    rng = np.random.default_rng(26)
    E = M.design()[2]
    streams = []
    for len0, n_last, first in ((960, 300, True), (800, 300, False)):
        st = fresh()
        start = 0 if first else len0
        x = crand(rng, start + n_last, 0.25)
        P = st["phase"] if first else M.chain(st["phase"], len0, start + 1)[1]
        ph = M.cmul32(P, E[n_last - 1])[()]
        x[-1] = np.complex64((2.6 / np.sqrt(2)) * (1 + 1j) * np.conj(ph.astype(np.complex128)))
        whole = start + (len0 if first else 960)
        streams += [dict(x=x, len0=len0, **st), dict(x=np.concatenate([x, np.zeros(whole - len(x), np.complex64)]), len0=len0, **st)]
    y, _, _ = run_bpf(L, torch_dev, tabs, streams, 0, strided=True, what="partial block against zero padding")
    hold(y, streams, 0, 0, "partial block against zero padding")
    for a in (0, 2):
        n = len(streams[a]["x"])
        tx.check_bits(y[a], y[a + 1][:n], f"partial block (avail {n}) against the block padded with zeros", ("sample", "component"))


# ================================================================================================================================================================
# 2. cutting a stream into invocations
# ================================================================================================================================================================
def test_cutting_into_invocations(L, torch_dev, tabs):
    """17 blocks in one invocation == 17 invocations of one block == 3 invocations of 8 + 8 + 1 blocks, advance = 1, bit for bit in y and in the final record: the tail
    hand-over through LDS, the workgroup seam, k_bpf_advance and the 100 -> 102 transition at once.  Three streams with first blocks of 800, 960 and 1120 samples, all
    before their first call.  After every invocation the record is the float32 state model's, bit for bit."""
    rng = np.random.default_rng(17)
    l0 = [800, 960, 1120]
    xs = [crand(rng, l + 16 * 960) for l in l0]

    def cut(pattern):
        recs = [fresh() for _ in l0]
        pos, outs, first = [0, 0, 0], [[], [], []], True
        for nblk in pattern:
            take = [(l0[b] if first else 960) + (nblk - 1) * 960 for b in range(3)]
            streams = [dict(x=xs[b][pos[b]:pos[b] + take[b]], len0=l0[b] if first else 960, **recs[b]) for b in range(3)]
            y, after, _ = run_bpf(L, torch_dev, tabs, streams, 0, advance=1, strided=True, what=f"cut {pattern}")
            for b in range(3):
                check_state32(after[b], streams[b], streams[b]["len0"], f"cut {pattern} at {pos[b]}, stream {b}")
                outs[b].append(y[b]); pos[b] += take[b]
            recs, first = after, False
        assert pos == [len(v) for v in xs]
        return [np.concatenate(o) for o in outs], recs

    y1, r1 = cut([17])
    hold(y1, [dict(x=xs[b], len0=l0[b], **fresh()) for b in range(3)], 0, 0, "17 blocks in one invocation")
    for pattern in ([1] * 17, [8, 8, 1]):
        y2, r2 = cut(pattern)
        for b in range(3):
            tx.check_bits(y2[b], y1[b], f"{pattern} against one invocation, stream {b}", ("sample", "component"))
            assert r2[b]["mem_len"] == r1[b]["mem_len"] == 102
            tx.check_bits(r2[b]["mem"], r1[b]["mem"], f"{pattern}: final memory, stream {b}", ("sample", "component"))
            tx.check_bits(np.array([r2[b]["phase"]]), np.array([r1[b]["phase"]]), f"{pattern}: final phase, stream {b}", ("", "component"))


def test_advance_leaves_short_and_empty_streams_alone(L, torch_dev, tabs):
    """advance = 1 with fewer than 102 samples, with none, or with len0 <= 0: the record stays as it was (rd_bpf_args' contract); the others advance"""
    rng = np.random.default_rng(3)
    streams = [dict(x=crand(rng, 101), len0=960, **carried(rng)), dict(x=crand(rng, 0), len0=960, **fresh()), dict(x=crand(rng, 500), len0=0, **carried(rng)),
               dict(x=crand(rng, 102), len0=960, **fresh())]
    y, after, _ = run_bpf(L, torch_dev, tabs, streams, 0, advance=1, strided=True, what="advance, short streams")
    hold(y, streams, 0, 0, "advance, short streams")
    for b, s in enumerate(streams):
        check_state32(after[b], s, s["len0"], f"advance, stream {b}")
        if b < 3:
            assert after[b]["mem_len"] == s["mem_len"] and np.array_equal(after[b]["mem"].view(np.uint32), s["mem"].view(np.uint32))
    assert after[3]["mem_len"] == 102


# ================================================================================================================================================================
# 3. dynamic range
# ================================================================================================================================================================
def test_quiet_stretch_beside_a_burst(L, torch_dev, tabs):
    """One power-of-two scale per block: a 2^-14-level stretch beside unit-level samples inside a block, across a block boundary, across the workgroup seam (block 8's
    head is recomputed from x), and blocks alternating between 2^-10 and 2^6 -- every sample under the per-sample bound, which follows the quiet stretch down where
    a bar relative to the peak does not.  A stream of zeros gives zeros."""
    rng = np.random.default_rng(14)
    len0, n = 960, 960 * 10 + 200
    q = np.float32(2.0 ** -14)
    xs = [crand(rng, n) for _ in range(4)]
    xs[0][960 + 300:960 + 700] *= q                                       # inside block 1
    xs[1][2 * 960 - 250:2 * 960 + 250] *= q                               # across the boundary of blocks 1 and 2
    xs[2][8 * 960 - 250:8 * 960 + 250] *= q                               # across the workgroup seam
    for k in range(11):
        xs[3][k * 960:(k + 1) * 960] *= np.float32(2.0 ** (-10 if k % 2 else 6))
    streams = [dict(x=v, **(fresh() if b % 2 else carried(rng))) for b, v in enumerate(xs)]
    y, _, _ = run_bpf(L, torch_dev, tabs, streams, len0, what="dynamic range")
    for b, name in enumerate(("stretch inside a block", "stretch across a block boundary", "stretch across the workgroup seam", "blocks alternating 2^-10 / 2^6")):
        hold(y[b:b + 1], streams[b:b + 1], len0, 0, name)
    zs = [dict(x=np.zeros(960 + 500, np.complex64), **fresh()), dict(x=crand(rng, 960 + 500), **fresh()), dict(x=np.zeros(2 * 960, np.complex64), **fresh())]
    y, _, _ = run_bpf(L, torch_dev, tabs, zs, len0, what="zeros")
    assert (y[0] == 0).all() and (y[2] == 0).all(), "a stream of zeros did not give zeros"          # (of either sign: the up mixer multiplies 0 by a negative component)


def grid_stream(rng, sizes):
    """integers / 1024 with |integer| <= 1023, one component of every block exactly 1: every block's window maximum X lies in [1, 2)"""
    n = sum(sizes)
    x = ((rng.integers(-1023, 1024, n) + 1j * rng.integers(-1023, 1024, n)) / 1024).astype(np.complex64)
    pos = 0
    for k in sizes:
        x[pos + k // 2] = 1.0 + x[pos + k // 2].imag * 1j
        pos += k
    return x


def test_power_of_two_scaling(L, torch_dev, tabs):
    """Exact-grid samples: 2^k x gives 2^k y bit for bit for every k that keeps each block's maximum inside bpf_stage_planes' exponent clamps.  The clamp is on the
    biased exponent e of X, 32 <= e <= 222; the blocks here have X in [1, 2), e = 127 + k, so -95 <= k <= 95: both ends, their neighbours and a few between are run.
    One k beyond each clamp is held to the bound the model gives there (below 2^-95 its second term stays TINY 2^-95; above 2^96 it holds as it stands)."""
    rng = np.random.default_rng(95)
    sizes = [800, 960, 300]
    x0 = grid_stream(rng, sizes)
    assert M.EB_MIN - 127 == -95 and M.EB_MAX - 127 == 95
    y0, _, _ = run_bpf(L, torch_dev, tabs, [dict(x=x0, **fresh())] * 3, 800, what="grid, k = 0")
    hold(y0, [dict(x=x0, **fresh())] * 3, 800, 0, "grid, k = 0")
    y0 = y0[0]
    comp = np.abs(y0.view(np.float32))
    assert comp[comp > 0].min() > 2.0 ** -30                             # 2^-95 y stays a normal float32: the comparison below is exact
    for ks in ([-95, -94, -60], [-1, 1, 60], [94, 95, 7]):
        streams = [dict(x=(x0 * np.float32(2.0) ** k).astype(np.complex64), **fresh()) for k in ks]
        for s, k in zip(streams, ks):
            assert np.array_equal(s["x"].astype(np.complex128), x0.astype(np.complex128) * 2.0 ** k)
        y, _, _ = run_bpf(L, torch_dev, tabs, streams, 800, what=f"grid, k = {ks}")
        for b, k in enumerate(ks):
            want = (y0.astype(np.complex128) * 2.0 ** k).astype(np.complex64)
            tx.check_bits(y[b], want, f"2^{k} x against 2^{k} y", ("sample", "component"))
    beyond = [dict(x=(x0 * np.float32(2.0) ** k).astype(np.complex64), **fresh()) for k in (-97, 97, -99)]
    y, _, _ = run_bpf(L, torch_dev, tabs, beyond, 800, what="grid, beyond the clamps")
    for b, k in enumerate((-97, 97, -99)):
        hold(y[b:b + 1], beyond[b:b + 1], 800, 0, f"k = {k}, beyond the clamp")


# ================================================================================================================================================================
# 4. the clip
# ================================================================================================================================================================
def m2_variants(y):
    """float32 |y|^2 as the kernel may form it: both products rounded, or either one fused into the sum"""
    re, im = y.real.astype(np.float32), y.imag.astype(np.float32)
    r2, i2 = (re * re).astype(np.float32), (im * im).astype(np.float32)
    r64, i64 = re.astype(np.float64) ** 2, im.astype(np.float64) ** 2
    return np.stack([(r2 + i2).astype(np.float32), (r64 + i2).astype(np.float32), (r2 + i64).astype(np.float32)])


def check_clip(yc, y0, what):
    """clip = 1 against the same launch with clip = 0: float32 |y|^2 <= 1 -> the same bits; > 1 -> the unclipped sample over its modulus within CLIP (so the modulus is
    within 6 u of 1 and the phase is the sample's); where the three ways to form |y|^2 disagree, either"""
    m2 = m2_variants(y0)
    keep, cut = (m2 <= 1).all(0), (m2 > 1).all(0)
    same = yc.view(np.uint64) == y0.view(np.uint64)
    z = y0.astype(np.complex128)
    near = np.abs(yc - z / np.maximum(np.abs(z), 1e-300)) <= M.CLIP
    assert same[keep].all(), f"{what}: {int((~same[keep]).sum())} samples with |y|^2 <= 1 changed by the clip"
    assert near[cut].all(), f"{what}: {int((~near[cut]).sum())} clipped samples off y / |y| by more than {M.CLIP:.2e}"
    assert (same | near)[~keep & ~cut].all(), what
    return int(keep.sum()), int(cut.sum())


def test_clip_at_its_threshold(L, torch_dev, tabs):
    """np.clip(abs(y), 0, 1) exp(1j angle(y)): the clip compares float32 |y|^2 with 1 and must keep a sample AT 1.  Streams at a level where about half the samples are
    clipped; then one known output sample is put within a few ulp of modulus 1 on either side (the input scaled by (1 + j 2^-23) / |y|, j = -6, -2, 2, 6: |y|^2 - 1
    about 4 j u, the roundings of the scaled input a few u more).  (A sample AT 1 is divided by sqrt(1) = 1 when a comparison takes it for clipped: the same bits either
    way, so `>` against `>=` is not observable.)  Held to the model + clip under the bound as well."""
    rng = np.random.default_rng(132)
    len0, n = 1152, 1152 + 960 + 100
    streams = [dict(x=crand(rng, n, 1.6), **(fresh() if b else carried(rng, 1.6))) for b in range(3)]
    y0, _, _ = run_bpf(L, torch_dev, tabs, streams, len0, clip=0, what="clip 0")
    yc, _, _ = run_bpf(L, torch_dev, tabs, streams, len0, clip=1, what="clip 1")
    hold(yc, streams, len0, 1, "clip, level 1")
    for b in range(3):
        kept, cut = check_clip(yc[b], y0[b], f"clip, stream {b}")
        assert kept > n // 10 and cut > n // 10
    # one sample within a few ulp of the threshold, on either side
    i = 1152 + 500
    x = streams[1]["x"]
    s0 = np.float64(1.0) / np.abs(y0[1][i].astype(np.complex128))
    scaled = [dict(x=(x.astype(np.complex128) * (s0 * (1 + j * 2.0 ** -23))).astype(np.complex64), **fresh()) for j in (-6, -2, 2, 6)]
    y0s, _, _ = run_bpf(L, torch_dev, tabs, scaled, len0, clip=0, what="threshold, clip 0")
    ycs, _, _ = run_bpf(L, torch_dev, tabs, scaled, len0, clip=1, what="threshold, clip 1")
    d = np.array([float(m2_variants(v[i:i + 1])[0][0]) - 1.0 for v in y0s])
    print("threshold sample: float32 |y|^2 - 1 =", " ".join(f"{v / U:+.0f}u" for v in d))
    assert (d <= 0).any() and (d > 0).any() and np.abs(d).max() <= 40 * U, "the construction did not put the sample on both sides of 1 within 40 u (20 ulp)"
    for b in range(4):
        check_clip(ycs[b], y0s[b], f"threshold stream {b}")
        one = m2_variants(y0s[b][i:i + 1])
        if (one <= 1).all():
            assert ycs[b][i] == y0s[b][i]
        elif (one > 1).all():
            assert abs(abs(complex(ycs[b][i])) - 1) <= M.CLIP
    hold(ycs, scaled, len0, 1, "clip, threshold streams")


# ================================================================================================================================================================
# 5. batch independence
# ================================================================================================================================================================
def test_batch_independence(L, torch_dev, tabs):
    """four streams with their own data, first block, length and state: each bit-equal, in y, in the chain and in the record it is left with, to its own B = 1 run"""
    rng = np.random.default_rng(4)
    spec = [(800, 800 + 8 * 960 + 5), (1120, 300), (960, 960 + 960), (1152, 1152 + 37)]
    streams = [dict(x=crand(rng, n, 2.0 ** (3 * b)), len0=l, **(carried(rng) if b % 2 else fresh())) for b, (l, n) in enumerate(spec)]
    y, recs, chains = run_bpf(L, torch_dev, tabs, streams, 0, advance=1, strided=True, what="batch of four")
    hold(y, streams, 0, 0, "batch of four")
    for b, s in enumerate(streams):
        y1, r1, c1 = run_bpf(L, torch_dev, tabs, [s], 0, advance=1, strided=True, what=f"stream {b} alone")
        tx.check_bits(y[b], y1[0], f"stream {b} in the batch against alone", ("sample", "component"))
        tx.check_bits(recs[b]["mem"], r1[0]["mem"], f"stream {b}: memory", ("sample", "component"))
        assert recs[b]["phase"] == r1[0]["phase"] and recs[b]["mem_len"] == r1[0]["mem_len"] and np.array_equal(chains[b], c1[0])


# ================================================================================================================================================================
# 6. the receiver's doors: the pre-pass and rx2_bpf_own behind BatchEngine.rx
# ================================================================================================================================================================
@pytest.fixture(scope="module")
def rx_engine(tabs):
    from radae_amd.engine import BatchEngine
    eng = BatchEngine(1, max_tx_mf=1, rx_trace_calls=640)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", ["slip_plus", "slip_minus", "slipdrops"])
def test_receiver_doors(rx_engine, torch_dev, golden, name):
    """rx_filtered of a recording whose timing slips inside the invocation (slip_plus: the 1120-sample call is call 17, past the second workgroup seam of the pre-pass;
    rx2_bpf_own filters the rest), every sample against the model driven with the traced call sizes, under the per-sample bound.  The same bits from one call per
    invocation (always on the grid) and from invocations cut at the call before and at the call after the first slip: the `leaving` branch of rx2_bpf_own, its
    carried-on branch, and a pre-pass that starts from the state either left."""
    import torch
    eng = rx_engine
    g = golden("rxtrace_" + name)
    x = np.ascontiguousarray(edge_case_input(g))
    eng.rx_reset()
    eng.rx(torch.tensor(x[None], device=torch_dev))
    sizes = [int(k) for k in eng.rx_trace(0)["nin_before"]]
    slips = [k for k, s in enumerate(sizes) if s != 960]
    assert slips, "the recording does not leave the grid"
    n = sum(sizes)
    y = eng.rx_filtered(0, n)
    want, bound, _ = M.run(x[:n], sizes)
    r = tx.check_close(y, want, bound, f"rx_filtered {name}", ("sample",))
    print(f"rx_filtered {name} ({len(sizes)} calls, first slip at call {slips[0]}, peak {np.abs(x).max():.3g}): largest |dy| / bound = {r:.3f}")

    def fed(cuts):
        """the stream fed in invocations of cuts[i] calls each (the rest in one more)"""
        eng.rx_reset()
        pos, k, outs = 0, 0, []
        for c in list(cuts) + [len(sizes) - sum(cuts)]:
            if c <= 0:
                continue
            m = sum(sizes[k:k + c])
            _, s, _ = eng.rx(torch.tensor(x[None, pos:pos + m], device=torch_dev), max_calls=c)
            assert s[0].consumed == m and s[0].n_calls == c, (cuts, k, s[0].consumed, m)
            outs.append(eng.rx_filtered(0, m)); pos += m; k += c
        return np.concatenate(outs)

    k = slips[0]
    assert len(sizes) < 640
    every = [[1] * len(sizes)] if len(sizes) <= 64 else []                # (the 510 calls of the slip + drops recording are fed around the slip only)
    for cuts in every + [[k - 1], [k], [k + 1], [k - 1, 1, 1]]:
        tx.check_bits(fed(cuts), y, f"{name} fed in invocations of {cuts[:4]}.. calls", ("sample", "component"))


# ================================================================================================================================================================
# 7. the transmit door: RADE_BATCH_TX_BPF
# ================================================================================================================================================================
def test_transmit_door(torch_dev, tabs, golden):
    """A plain engine's samples are the filter's input (the transmit side is bit-reproducible); the engine with RADE_BATCH_TX_BPF must give model + clip of them, per
    sample: six frames in one call (blocks of 960, the state advanced), then the end-of-over frame (len0 = 1152: a fifth tile); then six calls of one frame and the
    end-of-over frame again -- the state carried through k_bpf_advance -- with the same bits."""
    import torch
    from radae_amd.engine import BatchEngine
    g = golden("txbpf")
    n_mf = 6
    f2 = np.stack([g["features"], g["features"][::-1].copy()])
    plain, filt = BatchEngine(2, max_tx_mf=n_mf), BatchEngine(2, max_tx_mf=n_mf, flags=0x400)
    try:
        raw = plain.tx(torch.tensor(f2, device=torch_dev)).cpu().numpy()
        raw_eoo = plain.tx_eoo().cpu().numpy()
        iq = filt.tx(torch.tensor(f2, device=torch_dev)).cpu().numpy()
        eoo = filt.tx_eoo().cpu().numpy()
        worst = 0.0
        for b in range(2):
            xin = np.concatenate([raw[b], raw_eoo[b]])
            want, bound, _ = M.run(xin, [960] * n_mf + [1152], do_clip=True)
            worst = max(worst, tx.check_close(np.concatenate([iq[b], eoo[b]]), want, bound, f"transmit filter, stream {b}", ("sample",), (960, "frame")))
        print(f"transmit filter + clip, 6 frames and the end-of-over frame: largest |dy| / bound = {worst:.3f}")
        filt.tx_reset()
        parts = [filt.tx(torch.tensor(f2[:, 12 * k:12 * k + 12].copy(), device=torch_dev)).cpu().numpy() for k in range(n_mf)]
        tx.check_bits(np.concatenate(parts, axis=1), iq, "six calls against one", ("stream", "sample", "component"))
        tx.check_bits(filt.tx_eoo().cpu().numpy(), eoo, "end-of-over frame after six calls", ("stream", "sample", "component"))
    finally:
        plain.close(); filt.close()
