"""Host tests (no GPU) of the stored-file receiver past the acquisition: the float64 restatements of tests/file_ref.py against the committed recordings (the reference's
own figures on them: file_ref.TABLE) and, where the reference is present, against its classes live; that each comparison rejects the bug it is there for; and the
library's host functions rade_file_plan and rade_ber_best against the restatements."""
import os
import subprocess
import sys

import numpy as np
import pytest

import acq_ref as R
import file_ref as F

CASES = [(name, bpf) for name in R.RECORDINGS for bpf in (False, True)]


def table_row(p, n):
    return (n, p["hop"], p["tmax"], p["fmax"], p["t"] - p.get("base", 0), p["f"], p["n_left"], p["n_mf"])


@pytest.fixture(scope="module")
def plans():
    return {(name, bpf): F.recording_plan(name, bpf) for name, bpf in CASES}


def test_demod_reproduces_the_reference_recordings(golden):
    """file_ref.demod on chan_mpp.npz's rx against every a_* array of ideal_rx.npz, under the rule of tests/test_ideal_rx_gpu.py"""
    g, rx = golden("ideal_rx"), golden("chan_mpp")["rx"]
    n = 0
    for key in g.files:
        if key.startswith("a_"):
            _, eq, t, sc = key.split("_")
            F.check_z(F.demod(rx, eq, sc != "nomag", -int(t[1:]), 1 if sc == "bn1" else 3), g[key], key)
            n += 1
    assert n == 20


@pytest.mark.parametrize("name,bpf", CASES)
def test_plan_gives_the_references_figures(plans, name, bpf):
    p = plans[(name, bpf)]
    assert p["status"] == F.OK and table_row(p, len(R.fixture_input(name))) == F.TABLE[(name, bpf)]
    assert p["Dmax"] - p["second"] > 1e-6 * p["Dmax"], "the reference decides this refine in float32; so must float64, by a margin"


def test_the_plan_check_rejects_its_bugs():
    """refine at the acquiring hop (the --acq_test placement, what acquire() does) moves t, f or n_left on every recording; a tail that is not shortened moves n_left"""
    for name, bpf in CASES:
        x = F.recording(name, bpf)
        det = R.fixture_detect(name) if not bpf else None
        for bug in ("refine_at_event", "tail_kept"):
            p = F.plan(x, bug=bug, det=det)
            assert table_row(p, len(x)) != F.TABLE[(name, bpf)], (name, bpf, bug)
    p = F.plan(F.recording("mpp", False), bug="refine_at_event", det=R.fixture_detect("mpp"))
    assert p["f"] == -11.0                                             # acq.npz's refined value: the two placements disagree on this recording (-11.75 one frame later)


def test_mix_counts_its_phase_from_start(golden):
    """chan_mpp's rx behind 37 zeros, mixed up by 7.25 Hz from its own first sample: mix(start, freq) undoes it, a phase origin at sample 0 does not (7.25 Hz x 37 samples
    is 0.21 rad: the latents rotate)"""
    g, rx = golden("ideal_rx"), golden("chan_mpp")["rx"]
    start, freq = 37, 7.25
    xs = np.concatenate([np.zeros(start, np.complex64), (rx * np.exp(2j * np.pi * freq / F.FS * np.arange(len(rx)))).astype(np.complex64)])
    F.check_z(F.demod(F.mix(xs, start, freq), "none", False, -16), g["a_none_t16_nomag"], "mix")
    with pytest.raises(AssertionError):
        F.check_z(F.demod(F.mix(xs, start, freq, bug="origin0"), "none", False, -16), g["a_none_t16_nomag"], "origin0")
    assert np.array_equal(F.mix(xs, start, 0.0), xs[start:])


def test_ber_align_keeps_the_scripts_denominator():
    rng = np.random.default_rng(3)
    z = np.sign(rng.standard_normal(12 * F.ZMF)).astype(np.float32)
    z_hat = z[3 * F.ZMF:3 * F.ZMF + 6 * F.ZMF].copy()
    z_hat[5] *= -1
    err, best, ber = F.ber_align(z, z_hat)
    assert best == 3 and err[3] == 1 and ber == 1 / (9 * F.ZMF)      # n_bits = len(z) after the shift: 9 frames, not the 6 compared
    assert list(err[12:]) == [-1] * 8 and err[11] >= 0
    assert F.ber_align(z, z_hat, bug="n_bits_syms")[2] == 1 / (6 * F.ZMF)
    from radae_amd.stages import ber_best
    assert ber_best(err, len(z)) == (best, ber)
    assert ber_best(np.full(20, 10 ** 6), 240) == (-1, 1.0)


@pytest.mark.parametrize("name,bpf", CASES)
def test_library_plan_agrees_with_the_restatement(plans, name, bpf):
    from radae_amd.stages import file_plan
    p, n = plans[(name, bpf)], len(R.fixture_input(name))
    q = file_plan(n, p["hop"], p["t"], p["f"])
    assert (q.status, q.start, q.n_mf, q.freq) == (F.OK, p["start"], p["n_mf"], p["f"])
    assert file_plan(n, p["hop"], p["t"], p["f"], freq_offset=3.5).freq == 3.5


def test_library_plan_statuses():
    from radae_amd.stages import file_plan
    n, k = 30752, 10
    base = 960 * (k + 1)
    for args, want in (((n, -1, 0, 0.0), F.NOT_ACQUIRED), ((n, k, base + 31, 1.0), F.EARLY), ((n, k, base + 32, 1.0), F.OK), ((n, k, n - (k + 1) - 1120 + 1, 1.0), F.REFINE_OUTSIDE),
                       ((n, k, -1, 1.0), F.REFINE_OUTSIDE), ((base + 1919 + k + 1, k, base + 32, 1.0), F.SHORT), ((base + 1920 + k + 1, k, base + 32, 1.0), F.OK)):
        q = file_plan(*args)
        ref = F.plan_after(*args)
        assert q.status == want == ref[0] and (q.start, q.n_mf) == ref[1:3], (args, q.status, want, ref)
        if want != F.OK:
            assert (q.start, q.n_mf) == (0, 0)
    with pytest.raises(ValueError):
        file_plan(-1, 0, 0, 0.0)
    with pytest.raises(ValueError):
        file_plan(n, 0, 0, float("nan"))


def test_the_headers_agree_on_the_filters_span():
    """RADE_FILE_BPF_SPAN of the public header is RD_FILE_CHUNK x RD_FILE_NCHUNK of rade_dev.h (where the GPU tests put their edge sizes), and the bound's two constants
    are the values the header's derivation ends in"""
    import re
    import gpu_kit
    with open(os.path.join(gpu_kit.REPO, "include", "rade_batch.h")) as f:
        text = f.read()
    assert int(re.search(r"^#define RADE_FILE_BPF_SPAN (\d+)", text, re.M).group(1)) == gpu_kit.define("RD_FILE_CHUNK") * gpu_kit.define("RD_FILE_NCHUNK") == 8192
    assert "#define RADE_FILE_BPF_EPS (2.0 / 1048576.0)" in text and "#define RADE_FILE_BPF_TINY (1.0 / 134217728.0)" in text
    from radae_amd import engine
    lib = engine.load_library()
    for n in ("rade_batch_bpf_file", "rade_file_plan", "rade_batch_rx_file", "rade_batch_ber_align", "rade_ber_best"):
        assert n in engine.EXPORTED_SYMBOLS and hasattr(lib, n), n


def test_restatements_against_the_reference_live():
    """complex_bpf, acquisition.refine and RADAE.receiver of the reference itself (a child process: its modules want their own directory)"""
    ref = os.environ.get("RADAE_REFERENCE") or "/root/reference"
    if not os.path.isfile(os.path.join(ref, "radae", "dsp.py")):
        pytest.skip("the reference is not on this machine")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "file_ref.py"), ref], capture_output=True, text=True, env={**os.environ, "PYTHONPATH": here})
    assert r.returncode == 0 and r.stdout.strip().endswith("live ok"), r.stdout[-2000:] + r.stderr[-2000:]
