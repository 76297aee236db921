"""Which generator writes which fixture.  One row per generator: name, the files it writes, the committed files it reads (`needs`), the callable.
Paths are relative to the repository; a callable takes (src, dst): the tree it reads its `needs` from and the tree it writes into.
tests/test_golden_registry.py holds this table against tests/golden/.
"""
from collections import namedtuple

from . import acquisition, bandpass, clock_offset, cno, dnnw_export, ideal_rx, modem, rate_rs, single_carrier, streaming

Generator = namedtuple("Generator", "name outputs needs run")


def _g(*names):
    return tuple(f"tests/golden/{n}" for n in names)


GENERATORS = (
    Generator("consts", _g("consts.npz"), (), modem.gen_consts),
    Generator("enc_tx", _g("enc_tx.npz"), (), modem.gen_enc_tx),
    Generator("chan_rx", _g("chan_mpp.npz", "rxtrace_mpp.npz", "chan_awgn.npz", "rxtrace_awgn.npz", "rxtrace_slip_plus.npz", "rxtrace_slip_minus.npz",
                            "rxtrace_foff.npz"), (), modem.gen_chan_rx),
    Generator("knobs", _g("chan_dfdt_pos.npz", "chan_dfdt_neg.npz", "rxtrace_dfdt.npz", "rxtrace_nounsync.npz"), (), modem.gen_knobs),
    Generator("dec_loss", _g("dec_loss.npz"), _g("rxtrace_awgn.npz"), modem.gen_dec_loss),
    Generator("model05", _g("model05.npz"), (), modem.gen_model05),
    Generator("bbfm", _g("bbfm.npz") + ("weights/bbfm_random_seed20240501.bin",), (), modem.gen_bbfm),
    Generator("wire", _g("wire.npz"), (), modem.gen_wire),
    Generator("bpf", _g("bpf.npz"), (), bandpass.gen_bpf),
    Generator("txbpf", _g("txbpf.npz"), (), bandpass.gen_txbpf),
    Generator("slipdrops", _g("rxtrace_slipdrops.npz"), (), streaming.gen_slipdrops),
    Generator("dfs8001", _g("rxtrace_dfs8001.npz"), (), streaming.gen_dfs),
    Generator("eoo_mpp", _g("rxtrace_eoo_mpp.npz"), (), streaming.gen_eoo_mpp),
    Generator("bypass", _g("bypass.npz"), _g("rxtrace_awgn.npz"), streaming.gen_bypass),
    Generator("single_carrier", _g("sc_wire.npz", "sc_tx_bpsk_1500.npz", "sc_tx_analog_0.npz", "sc_rx_clean.npz", "sc_rx_noisy_foff.npz", "sc_rx_drift.npz",
                                   "sc_rx_drift_pos.npz", "sc_rx_lose_sync.npz"), (), single_carrier.main),
    Generator("dnnw_export", _g("dnnw_export_A.bin", "dnnw_export.npz", "weights_check.npz"), (), dnnw_export.main),
    Generator("acq", _g("acq.npz"), _g("rxtrace_mpp.npz", "rxtrace_awgn.npz", "rxtrace_foff.npz", "rxtrace_dfdt.npz", "consts.npz"), acquisition.main),
    Generator("clock_offset", _g("clock_offset.npz"), (), clock_offset.main),
    Generator("cno", _g("cno.npz"), (), cno.main),
    Generator("ideal_rx", _g("ideal_rx.npz"), _g("chan_mpp.npz"), ideal_rx.main),
    Generator("rate_rs", _g("rate_rs_bn3.npz"), (), rate_rs.main),
)
BY_NAME = {g.name: g for g in GENERATORS}


def ordered(names=()):
    """The named generators (all of them without names) with every generator after those whose outputs it needs."""
    owner = {o: g.name for g in GENERATORS for o in g.outputs}
    todo = [BY_NAME[n] for n in names] if names else list(GENERATORS)
    done, order = set(), []
    while todo:
        ready = [g for g in todo if all(owner[n] in done or BY_NAME[owner[n]] not in todo for n in g.needs)]
        if not ready:
            raise ValueError("the generators' needs form a cycle: " + ", ".join(g.name for g in todo))
        order += ready
        done |= {g.name for g in ready}
        todo = [g for g in todo if g not in ready]
    return order
