"""Host tests (no GPU) of the data handling behind `cli train_decoder` (radae_amd/train.py: load_sequences, epoch_batches): the sequence slicing and the aux column
against the reference's RADAEDataset live (dataset.py:53-64, :105-110), the dropped ragged batch, and the command's arguments."""
import os
import subprocess
import sys

import numpy as np
import pytest

from radae_amd import train

CHILD = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1] + "/radae")
from dataset import RADAEDataset
d = RADAEDataset(sys.argv[2], int(sys.argv[3]), 1, 30, 1, auxdata=bool(int(sys.argv[4])))
np.save(sys.argv[5], np.stack([d[i][0] for i in range(len(d))]))
"""


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_cli")
    rng = np.random.default_rng(1)
    f = rng.standard_normal((4 * 37, 36)).astype(np.float32)          # 148 frames: 9 sequences of 16 and a ragged tail
    z = rng.standard_normal((37, 80)).astype(np.float32)
    f.tofile(d / "features.f32"); z.tofile(d / "z.f32")
    return d, f, z


@pytest.mark.parametrize("aux", (0, 1))
def test_slicing_and_the_aux_column_against_the_reference_live(files, aux):
    ref = os.environ.get("RADAE_REFERENCE") or "/root/reference"
    if not os.path.isfile(os.path.join(ref, "radae", "dataset.py")):
        pytest.skip("the reference is not on this machine")
    d, f, z = files
    out = str(d / f"ref{aux}.npy")
    r = subprocess.run([sys.executable, "-c", CHILD, ref, str(d / "features.f32"), "16", str(aux), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = np.load(out)
    zs, fs = train.load_sequences(str(d / "z.f32"), str(d / "features.f32"), 16, bool(aux), seed=3)
    assert fs.shape == want.shape == (9, 16, 20 + aux) and fs.dtype == want.dtype == np.float32
    assert np.array_equal(fs[..., :20], want[..., :20])
    assert np.array_equal(zs, z[:36].reshape(9, 4, 80))
    if aux:                                                          # the bits themselves are drawn unseeded there: +-1, held over 4 frames, in column 20
        for a in (fs[..., 20], want[..., 20]):
            assert set(np.unique(a)) <= {-1.0, 1.0} and np.array_equal(a.reshape(9, 4, 4), np.repeat(a.reshape(9, 4, 4)[..., :1], 4, axis=-1))
        assert np.array_equal(fs, train.load_sequences(str(d / "z.f32"), str(d / "features.f32"), 16, True, seed=3)[1]), "the seeded bits repeat"
        assert abs(fs[..., 20].mean()) < 0.6


def test_the_latent_file_bounds_the_sequences_and_the_length_is_checked(files):
    d, f, z = files
    z[:20].tofile(d / "short.f32")
    zs, fs = train.load_sequences(str(d / "short.f32"), str(d / "features.f32"), 16)
    assert zs.shape == (5, 4, 80) and fs.shape == (5, 16, 20) and np.array_equal(fs.reshape(-1, 20), f[:80, :20])
    with pytest.raises(ValueError):
        train.load_sequences(str(d / "z.f32"), str(d / "features.f32"), 18)


def test_an_epoch_is_a_permutation_without_the_ragged_batch():
    rng = np.random.default_rng(0)
    b = train.epoch_batches(37, 8, rng)
    flat = np.concatenate(b)
    assert [len(x) for x in b] == [8, 8, 8, 8] and len(set(flat.tolist())) == 32 and flat.min() >= 0 and flat.max() < 37
    assert not np.array_equal(flat, np.concatenate(train.epoch_batches(37, 8, rng))), "every epoch has its own shuffle"
    assert train.epoch_batches(7, 8, rng) == []
