"""CPU tests of batched loss evaluation (rade_batch_loss) and per-stream channel conditions (rade_batch_channel_streams, rade_batch_tx_channel_streams):
the library exports the new entry points and engine.EXPORTED_SYMBOLS lists them, the header declares them, and the Python side's argument handling --
per-stream channel values, loss row counts and clipping, the array form of sigma_from_EbNodB -- behaves without a GPU.  The kernels themselves are
checked in tests/test_batch_loss_gpu.py."""
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rade_batch_loss", "rade_batch_channel_streams", "rade_batch_tx_channel_streams")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from radae_amd import engine
    return engine.load_library()


def test_new_symbols_are_exported_and_declared(lib):
    from radae_amd import engine
    for s in NEW_SYMBOLS:
        assert s in engine.EXPORTED_SYMBOLS
        assert hasattr(lib, s)
    hdr = open(os.path.join(REPO, "include", "rade_batch.h")).read()
    for decl in ("int rade_batch_loss(", "int rade_batch_channel_streams(", "int rade_batch_tx_channel_streams(",
                 "typedef struct { const float *sigma, *freq_offset, *df_dt; } rade_channel_streams;"):
        assert decl in hdr, decl


def test_channel_stream_values_scalar_and_sequence():
    from radae_amd.engine import channel_stream_values
    assert channel_stream_values(4, 0.1, -11.0, 0) == ((0.1, -11.0, 0.0), None)
    assert channel_stream_values(2, np.float32(0.5), np.array(3.0), np.int64(1)) == ((0.5, 3.0, 1.0), None)     # numpy scalars and 0-d arrays are scalars
    scal, per = channel_stream_values(3, [0.1, 0.2, 0.3], 5.0, np.array([0, 1, -1]))
    assert scal == (0.0, 5.0, 0.0) and sorted(per) == ["df_dt", "sigma"]
    for a in per.values():
        assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (3,)
    assert np.array_equal(per["sigma"], np.float32([0.1, 0.2, 0.3])) and np.array_equal(per["df_dt"], np.float32([0, 1, -1]))
    _, per = channel_stream_values(2, 0.1, np.arange(4, dtype=np.float64)[::2], 0.0)       # strided input -> contiguous float32 copy
    assert per["freq_offset"].flags.c_contiguous and np.array_equal(per["freq_offset"], np.float32([0, 2]))


@pytest.mark.parametrize("bad", [[0.1, 0.2, 0.3], [], np.zeros((4, 1)), np.zeros(5)])
def test_channel_stream_values_rejects_a_wrong_length(bad):
    from radae_amd.engine import channel_stream_values
    with pytest.raises(ValueError):
        channel_stream_values(4, bad, 0.0, 0.0)
    with pytest.raises(ValueError):
        channel_stream_values(4, 0.1, 0.0, bad)


def test_loss_lengths_defaults_sequences_and_status():
    from radae_amd.engine import RxStatus, loss_lengths
    ni, nh = loss_lengths(3, None, None, 100, 50)
    assert ni.dtype == np.int32 and nh.dtype == np.int32 and list(ni) == [100] * 3 and list(nh) == [50] * 3
    ni, nh = loss_lengths(3, 80, [50, 0, 7], 100, 60)
    assert list(ni) == [80] * 3 and list(nh) == [50, 0, 7]
    st = (RxStatus * 3)()
    st[0].n_valid, st[1].n_valid, st[2].n_valid = 3, 0, 4
    _, nh = loss_lengths(3, None, list(st), 100, 48)                # rx()'s status: 12 rows per valid modem frame
    assert list(nh) == [36, 0, 48]


def test_loss_lengths_clipping_and_refusals():
    from radae_amd.engine import loss_lengths
    _, nh = loss_lengths(3, None, [40, 10, 12], 100, 48, clip_start=5, clip_end=7)
    assert list(nh) == [28, 0, 0]                                   # loss.py: features_hat[clip_start : n - clip_end]; nothing left -> 0 (not scored)
    with pytest.raises(ValueError):
        loss_lengths(2, [100, 101], None, 100, 48)                  # more rows than the buffer holds
    with pytest.raises(ValueError):
        loss_lengths(2, None, [10, 49], 100, 48)
    with pytest.raises(ValueError):
        loss_lengths(2, [1, 2, 3], None, 100, 48)                   # wrong B
    with pytest.raises(ValueError):
        loss_lengths(2, None, None, 100, 48, clip_start=-1)


def test_sigma_from_EbNodB_takes_arrays(lib):
    from radae_amd import engine
    e = np.array([[-3.0, 0.0, 2.5], [10.0, 100.0, 6.0]], np.float32)
    for bn in (1, 3):
        v = engine.sigma_from_EbNodB(e, bottleneck=bn)
        assert isinstance(v, np.ndarray) and v.dtype == np.float32 and v.shape == e.shape
        want = np.float32([[engine.sigma_from_EbNodB(float(x), bottleneck=bn) for x in row] for row in e])
        assert np.array_equal(v, want)
        assert isinstance(engine.sigma_from_EbNodB(3.0, bottleneck=bn), float)
    assert engine.sigma_from_EbNodB([0.0, 3.0]).shape == (2,)
    with pytest.raises(ValueError):
        engine.sigma_from_EbNodB(e, bottleneck=2)
