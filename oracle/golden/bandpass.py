"""The band-pass fixtures, made by IMPORTING the reference (how it is driven and patched: oracle/golden/reference.py).

  bpf.npz     complex_bpf (radae/dsp.py:39-102) built as radae_rxe.py:104-109 builds the receiver's input filter, driven call by call with
              the call sizes a receiver goes through (960; 800 / 1120 after timing slips): input, call sizes, output.  Pins the stand-alone
              filter (oracle: orc_bpf_run; product: k_rx_bpf / rx2_bpf_own via rade_batch_rx_filtered).
  txbpf.npz   radae_tx(..., txbpf_en=True) (radae_txe.py:74-83, :130-132, :141-143; ctest radae_tx_basic): features -> transmit samples with the
              Tx band-pass filter and the magnitude clip, frame by frame, then the end-of-over frame.
"""
import numpy as np

from . import reference as R
from .reference import c64, golden


def gen_bpf(src, dst):
    R.enter()
    from radae import RADAE
    from radae.dsp import complex_bpf
    model = RADAE(21, 80, EbNodB=100, rate_Fs=True, pilots=True, pilot_eq=True, eq_mean6=False, cyclic_prefix=0.004, coarse_mag=True, time_offset=-16, bottleneck=3)
    w = np.array(model.w); Nc = model.Nc
    bandwidth = 1.2 * (w[Nc - 1] - w[0]) * model.Fs / (2 * np.pi)           # radae_rxe.py:106-108
    centre = (w[Nc - 1] + w[0]) * model.Fs / (2 * np.pi) / 2
    bpf = complex_bpf(101, model.Fs, bandwidth, centre, model.Fs)
    sizes = np.array([960, 960, 960, 800, 960, 1120, 960, 960, 800, 800, 960, 1120, 1120, 960], np.int32)
    rng = np.random.default_rng(404)
    n = int(sizes.sum())
    t = np.arange(n)
    x = 0.7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.5 * np.exp(2j * np.pi * 1500.0 * t / 8000.0) + 0.5 * np.exp(2j * np.pi * 3100.0 * t / 8000.0)
    x = c64(x)
    y, pos = [], 0
    for k in sizes:
        y.append(np.array(bpf.bpf(x[pos:pos + k]), dtype=np.complex64)); pos += k
    np.savez_compressed(golden(dst, "bpf.npz"), x=x, sizes=sizes, y=c64(np.concatenate(y)), bandwidth=np.float64(bandwidth), centre=np.float64(centre))


def gen_txbpf(src, dst):
    R.enter()
    from radae_amd.channel_tools import synth_features
    tx = R.new_tx(txbpf_en=True)
    n_mf = 6
    feats = synth_features(77, 12 * n_mf)
    out = []
    for k in range(n_mf):
        buf = np.zeros(tx.Nmf, dtype=np.csingle)
        tx.do_radae_tx(feats[12 * k:12 * k + 12].ravel().astype(np.float32), buf)
        out.append(buf.copy())
    eoo = np.zeros(tx.Neoo, dtype=np.csingle)
    tx.do_eoo(eoo)
    np.savez_compressed(golden(dst, "txbpf.npz"), features=feats.astype(np.float32), tx=c64(np.concatenate(out)), eoo=c64(eoo))
