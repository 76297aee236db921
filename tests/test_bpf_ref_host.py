"""tests/bpf_ref.py -- the float64 statement of the streaming band-pass filter, call by call -- held to what the reference recorded (tests/golden/bpf.npz) and to the C
oracle's filter on the slip recordings' call sizes; its per-sample check shown to reject a missing tap product, a dropped lo x hi plane product, a wrong delay, a
neighbour's block phase and a shifted memory; its float32 state model held to the float64 one.  The comparison is never with a device.  CPU only.

The yardstick is S[i] = sum_t |h[t]| |w[i + t]|, the same that the device's bound is stated in (tests/test_bpf_units_gpu.py), so a figure here means the same next
to a quiet stretch as next to a loud one.  The reference's float32 dot product of 101 terms (np.dot on complex64: pairwise, fused) stays within REF_BAR of it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bpf_ref as M
import tx_ref as tx
from kernel_ref import U

REF_BAR = 4 * U                 # the reference's own float32 dot product and mixers; measured 2.17 u on bpf.npz, 2.03 u live (python tests/bpf_ref.py)
OLD_BAR = 2e-6                  # tests/test_hip_parity.py: max |dy| < 2e-6 max |ref|


@pytest.fixture(scope="module")
def rec(golden):
    """bpf.npz and the model's answer to it, computed once and shared (read-only)"""
    g = golden("bpf")
    x, sizes = g["x"], [int(k) for k in g["sizes"]]
    y, bound, st = M.run(x, sizes)
    return dict(x=x, sizes=sizes, y=y, bound=bound, st=st, ref=g["y"], S=M.cond(x, sizes))


# ================================================================================================================================================================
# (a) the model against the reference's recordings
# ================================================================================================================================================================
def test_model_against_the_references_recording(rec):
    """all 13,440 samples of bpf.npz (960 / 800 / 1120-sample calls) within 4 x 2^-24 of sum |h| |w|"""
    assert len(rec["y"]) == len(rec["ref"]) == 13440
    r = tx.check_close(rec["ref"], rec["y"], REF_BAR * rec["S"], "bpf.npz against the model")
    print(f"bpf.npz: largest |reference - model| = {r * REF_BAR / U:.2f} x 2^-24 of sum |h| |w|, {np.abs(rec['ref'] - rec['y']).max():.2e} absolute")


def test_explicit_float32_chain_is_numpys_complex64(rec):
    """cmul32 against numpy's complex64 product, bit for bit, for every mixer phase of the 14 calls and the phase each call leaves"""
    _, _, E = M.design()
    P = np.complex64(1)
    for n in rec["sizes"]:
        pv = P * E[:n]
        assert pv.dtype == np.complex64
        tx.check_bits(M.cmul32(P, E[:n]), pv, f"phase vector of a {n}-sample call", ("sample", "component"))
        P = pv[-1]
    tx.check_bits(np.array([P]), np.array([rec["st"].phase]), "final phase", ("", "component"))
    c = M.chain(1.0, 960, 3 * 960)
    assert len(c) == 4 and c[0] == 1 and c[1] == E[959] and c[2] == M.cmul32(E[959], E[959])


@pytest.mark.parametrize("name", ["slip_plus", "slip_minus"])
def test_model_against_the_oracle_on_slip_call_sizes(golden, oracle, name):
    """the C oracle's filter driven with the recorded nin_before (a 1120- or an 800-sample call among the 960s), the same way.  The oracle's taps are the engine's
    (rd_tables_fill), so the model is given those."""
    g = golden("rxtrace_" + name)
    sizes = [int(k) for k in g["nin_before"]]
    assert (1120 if name == "slip_plus" else 800) in sizes
    x = g["rx_in"][:sum(sizes)]
    bp = oracle.Bpf()
    pos, ref = 0, []
    for k in sizes:
        ref.append(bp.run(x[pos:pos + k])); pos += k
    y, _, _ = M.run(x, sizes)
    r = tx.check_close(np.concatenate(ref), y, REF_BAR * M.cond(x, sizes), f"oracle filter on {name}")
    print(f"{name}: largest |oracle - model| = {r * REF_BAR / U:.2f} x 2^-24 of sum |h| |w|")


def test_engine_taps_against_the_design():
    """The kernels read rd_tables_fill's taps; the model is stated on radae_amd.acq.bpf_design()'s, which are the reference's own words (tests/golden/consts.npz).
    The two differ where C's sin and numpy's float32 sinc round differently: at most 2 ulp of a tap, 0.05 x 2^-24 of sum |h| in all.  Pinned, so that the device
    tests may hand the model the words the kernels read."""
    import __graft_entry__ as ge
    ge.build()
    import dev_abi
    h_lib, E_lib, _ = M.host_tables(dev_abi.load())
    h, _, E = M.design()
    tx.check_bits(E_lib, E, "bpf_E", ("entry", "component"))
    d = np.abs(h_lib.view(np.int32).astype(np.int64) - h.astype(np.float32).view(np.int32))
    print(f"taps: {int((d > 0).sum())} of 101 words differ, by at most {int(d.max())} ulp; sum |dh| / sum |h| = {np.abs(h_lib - h).sum() / np.abs(h).sum() / U:.3f} x 2^-24")
    assert d.max() <= 2 and np.abs(h_lib - h).sum() <= 0.1 * U * np.abs(h).sum()
    assert np.array_equal(h_lib, h_lib[::-1])


def test_model_against_the_reference_live():
    """complex_bpf of the reference itself over a few call partitions (a child process: its modules want their own directory), where the reference is present"""
    ref = os.environ.get("RADAE_REFERENCE") or "/root/reference"
    if not os.path.isdir(os.path.join(ref, "radae")):
        pytest.skip("the reference is not on this machine")
    here = os.path.dirname(os.path.abspath(M.__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "bpf_ref.py"), ref], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": here})
    print(out.stdout)
    assert out.returncode == 0 and "live ok" in out.stdout, out.stderr[-2000:]


# ================================================================================================================================================================
# (b) the per-sample check rejects what it is there for
# ================================================================================================================================================================
def old_bar_accepts(got, want):
    return bool(np.abs(got - want).max() < OLD_BAR * np.abs(want).max())


# the mistake, and whether max |dy| < 2e-6 max |ref| lets it through on this recording (computed below, asserted equal to this column)
FAULTS = [
    ((5, "tap", 700, 0), False),          # the outermost tap (h[0] = 2.4e-3) of one sample in a 1120-sample call
    ((5, "tap", 700, 50), False),         # the centre tap of the same sample
    ((3, "lohi"), False),                 # one block without the taps' low plane
    ((0, "first_delay"), False),
    ((4, "phase_next"), False),
    ((2, "mem_shift"), False),
]


@pytest.mark.parametrize("bug,old_accepts", FAULTS, ids=lambda v: "-".join(str(p) for p in v) if isinstance(v, tuple) else str(v))
def test_per_sample_check_rejects(rec, bug, old_accepts):
    """each planted mistake, rounded to complex64 as a device would store it, fails the device's own per-sample bound; the unperturbed model, rounded, passes"""
    good = rec["y"].astype(np.complex64)
    r = tx.check_close(good, rec["y"], rec["bound"], "the model's own rounding")
    assert r < 0.1
    bad = M.run(rec["x"], rec["sizes"], bug=bug)[0].astype(np.complex64)
    with pytest.raises(AssertionError, match="outside the bound"):
        tx.check_close(bad, rec["y"], rec["bound"], str(bug))
    got = old_bar_accepts(bad, rec["y"])
    print(f"{bug}: max |dy| = {np.abs(bad - rec['y']).max():.3e}, {OLD_BAR:g} max |ref| = {OLD_BAR * np.abs(rec['y']).max():.3e}: the old bar {'accepts' if got else 'rejects'} it")
    assert got == old_accepts


def test_quiet_stretch_fault_passes_the_old_bar():
    """What a maximum-relative bar cannot see, and every mistake above is loud enough for it on a level signal: a block at 2^-14 (and the 160 samples before it) between
    unit-level blocks, filtered WITHOUT the taps' low plane -- the dropped lo x hi product, 2^-12 of the block.  max |dy| over the stream is far inside 2e-6 of the
    peak; the per-sample bound rejects it."""
    rng = np.random.default_rng(11)
    sizes = [960] * 4
    x = ((rng.standard_normal(4 * 960) + 1j * rng.standard_normal(4 * 960)) * 0.5).astype(np.complex64)
    x[2 * 960 - 160:3 * 960] *= np.float32(2.0 ** -14)
    y, bound, _ = M.run(x, sizes)
    tx.check_close(y.astype(np.complex64), y, bound, "the model's own rounding")
    bad = M.run(x, sizes, bug=(2, "lohi"))[0].astype(np.complex64)
    print(f"quiet block without lo x hi: max |dy| = {np.abs(bad - y).max():.3e} against {OLD_BAR:g} max |ref| = {OLD_BAR * np.abs(y).max():.3e}")
    assert old_bar_accepts(bad, y)
    with pytest.raises(AssertionError, match="outside the bound"):
        tx.check_close(bad, y, bound, "quiet stretch")


# ================================================================================================================================================================
# (c) the float32 state model
# ================================================================================================================================================================
@pytest.mark.parametrize("len0,n_more,partial", [(960, 0, 0), (800, 2, 0), (1120, 1, 0), (1152, 0, 0), (960, 3, 300)])
def test_state32_against_the_float64_model(len0, n_more, partial):
    """mem, phase and mem_len after advance against what the float64 model carries: the phase bit for bit, mem_len equal, every memory sample within the down mixer's
    float32 rounding (2 sqrt 2 u |sample|).  A partial last block leaves the phase of a WHOLE block (k_bpf_chain steps by E[959]; the transmit side's blocks are whole
    frames): the memory still agrees, the phase is the chain's."""
    rng = np.random.default_rng(len0 + n_more)
    avail = len0 + 960 * n_more + partial
    x = ((rng.standard_normal(avail) + 1j * rng.standard_normal(avail)) * 0.5).astype(np.complex64)
    mem0 = ((rng.standard_normal(102) + 1j * rng.standard_normal(102)) * 0.5).astype(np.complex64)
    ph0 = M.design()[2][123]
    for mem, mem_len in ((np.zeros(102, np.complex64), 100), (mem0, 102)):
        st = M.State(mem[:mem_len], ph0)
        sizes = M.blocks_of(len0, avail)
        _, _, fin = M.run(x, sizes, st)
        m32, ml, p32 = M.state32(x, len0, avail, mem, mem_len, ph0)
        assert ml == fin.mem_len == 102
        tx.check_close(m32, fin.mem, 2 * np.sqrt(2) * U * np.abs(fin.mem) + M.DENORM, "memory", ("sample",))
        if not partial:
            tx.check_bits(np.array([p32]), np.array([fin.phase]), "phase", ("", "component"))
        tx.check_bits(np.array([p32]), M.chain(ph0, len0, avail)[-1:], "phase against the chain", ("", "component"))
    m32, ml, p32 = M.state32(x, len0, 101, mem0, 102, ph0)                 # fewer than 102 samples: the record stays
    assert ml == 102 and p32 == ph0 and np.array_equal(m32, mem0)


def test_header_fields_reads_the_records():
    """the header parser the records' member check stands on (tests/c_decl.py: dev_abi.load() compares every mirror's names with it), on doctored text: a record's
    names in order, with another record, comments and arrays in the way"""
    import c_decl
    text = "typedef struct { int a; } other;\ntypedef struct {\n  const int *p, *q; /* x; y */ float m[102][2]; long s;   /* t */\n} rec_t;"
    assert c_decl.parse(text)[1]["rec_t"] == ["p", "q", "m", "s"]
