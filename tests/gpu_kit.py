"""Plumbing shared by the GPU test modules (tests/test_*_gpu.py): the fixtures and small helpers every stage's test needs, each stated once.  A plain module
beside bands.py, not a plugin: a test module names what it takes (`from gpu_kit import torch_dev, engines  # noqa: F401`), and a fixture imported that way
keeps module scope per importing module.  torch and radae_amd are imported inside functions, so collection works without a GPU.  Reference arithmetic lives
in the *_ref.py restatements; test modules do not import test modules."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the receiver trace's discrete outputs: equal to the oracle's bit for bit
INT_KEYS = ["state_before", "state_after", "nin_before", "nin_after", "ret", "tmax", "f_ind_max", "valid_count", "uw_errors", "synced_count", "snr_int"]


def define(name):
    """the integer value of `#define name` in radae_amd/csrc/rade_dev.h"""
    with open(os.path.join(REPO, "radae_amd", "csrc", "rade_dev.h")) as f:
        m = re.search(r"^#define %s (\d+)\b" % re.escape(name), f.read(), re.M)
    if m is None:
        raise LookupError(f"rade_dev.h has no #define {name} with an integer literal")
    return int(m.group(1))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def Engine():
    from radae_amd.engine import BatchEngine
    return BatchEngine


@pytest.fixture(scope="module")
def engines():
    """one engine per batch size (and keyword set) for the whole module, for calls that use none of the model: max_tx_mf = 1 unless asked otherwise"""
    from radae_amd.engine import BatchEngine
    made = {}

    def get(B, **kw):
        key = (B, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = BatchEngine(B, **{"max_tx_mf": 1, **kw})
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture
def engine():
    """engine(B, **kw) -> a BatchEngine of the test's own, closed when the test ends, passed or failed (BatchEngine.close may be called twice)"""
    from radae_amd.engine import BatchEngine
    made = []

    def make(B, **kw):
        made.append(BatchEngine(B, **kw))
        return made[-1]
    yield make
    for e in made:
        e.close()


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------------------------
def dev(a, torch_dev):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=torch_dev)


def bits(x):
    """int32 words on the host, complex as (re, im).  A numpy array keeps its axes (the last one doubles for complex64); a torch tensor comes as its rows
    [B, -1], the shape of Band.rows().  For a [B, N] array and the tensor of the same data the words are the same."""
    if hasattr(x, "is_complex"):
        import torch
        x = (torch.view_as_real(x) if x.is_complex() else x).contiguous().cpu().numpy()
        x = x.reshape(x.shape[0], -1)
    return np.ascontiguousarray(x).view(np.int32)


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def rms(a, b):
    return float(np.sqrt(np.mean(np.abs(np.asarray(a, np.complex128) - np.asarray(b, np.complex128)) ** 2)))


def pack(rows):
    """rows of different length -> ([B, max] complex64 padded with zeros, n int32 [B])"""
    n = np.array([len(r) for r in rows], np.int32)
    x = np.zeros((len(rows), int(n.max())), np.complex64)
    for b, r in enumerate(rows):
        x[b, :n[b]] = r
    return x, n


def sync():
    import torch
    torch.cuda.synchronize()


def stream():
    """the current torch stream as the C entry points take it"""
    from radae_amd.engine import _stream_ptr
    return _stream_ptr()


def host32(t):
    return t.cpu().numpy().view(np.uint32)


class Dev:
    """host arrays uploaded once; unchanged() compares every word with what was uploaded"""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def put(self, arr, check=True):
        import torch
        host = np.ascontiguousarray(arr)
        raw = host.view(np.int32 if host.dtype.itemsize == 4 else np.int16).ravel()
        t = torch.from_numpy(raw).to(self.dev)
        assert t.data_ptr() % 16 == 0
        if check:
            self.items.append((t, raw))
        return t

    def unchanged(self):
        for i, (t, raw) in enumerate(self.items):
            assert np.array_equal(t.cpu().numpy(), raw), f"input buffer {i} was written"
