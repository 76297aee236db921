"""The C ABI of libradehip.so as ctypes, stated once: include/rade_api.h, rade_core.h and rade_batch.h in Python.

The structures, the flag / mode / format constants, the frame constants and one prototype table (PROTOTYPES: header -> function -> (restype, argtypes), in the headers'
order) that load_library() declares in one loop.  The symbol lists that build() checks are derived from the table.  tests/test_abi_host.py compares every entry with the
header's declaration and every structure with the layout the host compiler gives it: a function or a field added to a header is added here, and nowhere else.
This module imports neither torch nor the library's users; radae_amd/engine.py, stages.py, api.py, core.py and sc.py all bind through it.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RADE_LIBRADEHIP") or os.path.join(_HERE, "libradehip.so")      # the override is a developer aid (A/B builds, tools/ab_build.sh)
DEFAULT_BLOB = os.path.join(os.path.dirname(_HERE), "weights", "model19_check3.bin")

NMF, NEOO, NIN_MAX, FEAT_MF, NEOO_BITS, ZMF = 960, 1152, 1120, 432, 180, 240
RADE_USE_C_ENCODER, RADE_USE_C_DECODER, RADE_FOFF_TEST, RADE_VERBOSE_0 = 0x1, 0x2, 0x4, 0x8   # include/rade_api.h: rade_open() flags
BOTTLENECK1, TX_BPF, BYPASS_DEC, TX_LINEAR = 0x100, 0x400, 0x800, 0x1000          # include/rade_batch.h flags
EQ_MODES = {"ls": 0, "mean6": 1, "all": 2, "none": 3}                              # rade_ideal_rx_params.eq
RESAMPLE_MODES = {"sinc32": 0, "linear": 1}                                        # rade_resample_params.mode
WIRE_REAL, WIRE_IQ = 0, 1                                                          # rade_batch_wire_in / _out mode
RATE_C64, RATE_S16_REAL, RATE_S16_IQ = 0, 1, 2                                     # rade_batch_rate_convert format
FM_F32, FM_C64 = 0, 1                                                              # rade_batch_fm_mod input / rade_batch_fm_demod output format
FM_OUT_COMPLEX, FM_OUT_REAL = 0, 1                                                 # rade_batch_fm_mod output mode
SPEC_C64, SPEC_S16_REAL = 0, 1                                                     # rade_batch_specgram format
CHANP_NOISE_COMPLEX, CHANP_NOISE_REAL = 0, 1                                       # rade_channel_piece_params.noise_mode

vp, cp, ci, cu, cl, cll, cull, cf, cd, P = C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.c_long, C.c_longlong, C.c_ulonglong, C.c_float, C.c_double, C.POINTER
STRUCTS = {}                                                                       # typedef name in the headers -> its ctypes mirror


def _struct(name, typedefs, fields):
    cls = type(name, (C.Structure,), {"_fields_": fields})
    STRUCTS.update((t, cls) for t in typedefs.split())
    return cls


# ---- include/rade_core.h ------------------------------------------------------------------------------------------------------------------------------------
WeightArray = _struct("WeightArray", "WeightArray", [("name", cp), ("type", ci), ("size", ci), ("data", vp)])
_Model = _struct("_Model", "RADEEnc RADEDec", [("blob", vp), ("blob_len", ci), ("dim", ci), ("nb_z", ci)])             # dim: input_dim / output_dim
_State = _struct("_State", "RADEEncState RADEDecState", [("initialized", ci), ("dev", vp)])
# ---- include/rade_batch.h -----------------------------------------------------------------------------------------------------------------------------------
BatchConfig = _struct("BatchConfig", "rade_batch_config", [(n, ci) for n in ("n_streams", "max_tx_mf", "device", "flags", "rx_trace_calls")] + [("disable_unsync", cf)])
ChannelParams = _struct("ChannelParams", "rade_channel_params", [("n_sig", ci), ("n_pre", ci), ("n_post", ci), ("with_eoo", ci), ("sigma", cf), ("freq_offset", cf), ("df_dt", cf),
                                                                 ("G_dev", vp), ("noise_dev", vp), ("seed", cull), ("sine_amp", cf), ("sine_freq", cf), ("rx_gain", cf)])
ChannelStreams = _struct("ChannelStreams", "rade_channel_streams", [("sigma", vp), ("freq_offset", vp), ("df_dt", vp)])
ResampleParams = _struct("ResampleParams", "rade_resample_params", [("mode", ci), ("ppm", cd), ("ppm_host", vp), ("t0_host", vp), ("n0_host", vp), ("in_base_host", vp)])
RateParams = _struct("RateParams", "rade_rate_params", [("L", ci), ("M", ci), ("n0_host", vp), ("in_base_host", vp)])
FmModParams = _struct("FmModParams", "rade_fm_mod_params", [("Fs", cd), ("fc", cd), ("fd", cd), ("in_format", ci), ("out_mode", ci), ("sigma", cd), ("seed", cull), ("noise_dev", vp),
                                                            ("phase0_host", vp), ("phase_end_host", vp), ("n0_host", vp)])
FmDemodParams = _struct("FmDemodParams", "rade_fm_demod_params", [("Fs", cd), ("fc", cd), ("fd", cd), ("out_format", ci), ("ph_dont_limit", ci), ("b1", vp), ("N1", ci), ("b2", vp),
                                                                  ("N2", ci), ("in_base_host", vp), ("n0_host", vp), ("bb_out_dev", vp), ("bb_stride", cl)])
ChannelPieceParams = _struct("ChannelPieceParams", "rade_channel_piece_params",
                             [(n, cf) for n in ("sigma", "freq_offset", "df_dt", "gain")] + [(n, cll) for n in ("n0", "in_base", "g_base")] +
                             [(n, vp) for n in ("sigma_host", "freq_offset_host", "df_dt_host", "gain_host", "n0_host", "in_base_host", "g_base_host", "G_dev")] +
                             [("g_stride", cl), ("n_g_host", vp), ("noise_dev", vp), ("seed", cull), ("noise_mode", ci), ("sine_amp", cf), ("sine_freq", cf), ("rx_gain", cf)])
CnoParams = _struct("CnoParams", "rade_cno_params", [("window_time", cd), ("flow", cd), ("fhigh", cd)])
CnoPlan = _struct("CnoPlan", "rade_cno_plan_t", [(n, ci) for n in ("N", "J", "n_bins", "flow_bin", "fhigh_bin", "noise_st", "noise_en")])
CnoResult = _struct("CnoResult", "rade_cno_result", [("n_windows", ci), ("n_positive", ci), ("max_st", cll), ("max_CNodB", cd), ("max_SNRdB", cd)])
SnrSums = _struct("SnrSums", "rade_snr_sums", [(n, cd) for n in ("S1", "S1_sig", "S1_cross", "S1_noise", "S2_genie", "S2_est")])
SnrParams = _struct("SnrParams", "rade_snr_params", [("Nw", ci), ("h_step", ci), ("H_dev", vp), ("h_stride", cl), ("sigma_host", vp), ("row0_host", vp), ("noise_dev", vp),
                                                     ("noise_out_dev", vp), ("noise_stride", cl), ("seed", cull)])
SnrPoint = _struct("SnrPoint", "rade_snr_point", [(n, cd) for n in ("snrdB_genie", "snrdB_est", "NdB_genie", "NdB_est")])
SpecgramParams = _struct("SpecgramParams", "rade_specgram_params", [("fmin", cd), ("fmax", cd), ("lo", cd), ("hi", cd), ("peak_in_host", vp)])
SpecgramPlan = _struct("SpecgramPlan", "rade_specgram_plan_t", [(n, ci) for n in ("n_bins", "k0", "k1", "win", "step", "nfft")])
PsdPlan = _struct("PsdPlan", "rade_psd_plan_t", [(n, ci) for n in ("nfft", "win", "step", "run")])
SigstatResult = _struct("SigstatResult", "rade_sigstat_result", [(n, cd) for n in ("sum2", "peak2", "head_sum2", "head_peak2")] + [("n", cll)])
AcqHop = _struct("AcqHop", "rade_acq_hop", [("Dtmax12", cf), ("Dthresh", cd), ("tmax", ci), ("f_ind", ci), ("candidate", ci), ("S1", cd), ("S2", cd)])
AcqEvent = _struct("AcqEvent", "rade_acq_event", [("hop", ci), ("tmax", ci), ("f_ind", ci)])
AcqLog = _struct("AcqLog", "rade_acq_log", [("state", ci), ("tmax_candidate", ci), ("valid_count", ci)])
AcqRefineIn = _struct("AcqRefineIn", "rade_acq_refine_in", [("stream", ci), ("t_abs", cll), ("fmax", cd)])
AcqRefined = _struct("AcqRefined", "rade_acq_refined", [("t", cll), ("f", cd), ("Dmax", cd)])
AcqResult = _struct("AcqResult", "rade_acq_result", [("passes", ci), ("fails", ci), ("passed", ci), ("pfail", cd), ("mean_acq_time", cd)])
FileRxIn = _struct("FileRxIn", "rade_file_rx_in", [("start", cll), ("n_mf", ci), ("freq", cd)])
FilePlan = _struct("FilePlan", "rade_file_plan_out", [("start", cll), ("n_mf", ci), ("freq", cd), ("status", ci)])
RxStatus = _struct("RxStatus", "rade_rx_status", [(n, ci) for n in ("consumed", "n_calls", "n_valid", "has_eoo", "nin", "sync", "snr_dB", "state")])
IdealRxParams = _struct("IdealRxParams", "rade_ideal_rx_params", [("time_offset", ci), ("eq", ci), ("coarse_mag", ci), ("freq_offset_host", vp), ("df_dt_host", vp),
                                                                  ("z_ref_dev", vp), ("n_errors_host", vp)])
RxTrace = _struct("RxTrace", "rade_rx_trace", [(n, ci) for n in ("state_before", "state_after", "nin_before", "nin_after", "ret", "tmax", "f_ind_max", "valid_count", "uw_errors",
                                                                "synced_count", "snr_int", "pad")] +
                  [(n, cd) for n in ("fmax", "Dthresh", "Dtmax12", "Dtmax12_eoo")] + [("snrdB_3k_est", cf), ("pad2", cf)])
ScStatus = _struct("ScStatus", "rade_sc_status", [(n, ci) for n in ("n_frames", "consumed", "state", "nin", "fs_s")] +
                   [(n, cf) for n in ("g", "max_cs_re", "max_cs_im", "norm_rx_timing", "phase_ambiguity")])
ScFrame = _struct("ScFrame", "rade_sc_frame", [(n, ci) for n in ("state", "nin", "fs_s", "pad")] +
                  [(n, cf) for n in ("norm_rx_timing", "g", "max_cs_re", "max_cs_im", "phase_ambiguity")] + [("pad2", cf * 3)])

PROTOTYPES = {
    "rade_api.h": {
        "rade_initialize": (None, []),
        "rade_finalize": (None, []),
        "rade_open": (vp, [cp, ci]),
        "rade_close": (None, [vp]),
        "rade_version": (ci, []),
        "rade_n_tx_out": (ci, [vp]),
        "rade_n_tx_eoo_out": (ci, [vp]),
        "rade_nin_max": (ci, [vp]),
        "rade_n_features_in_out": (ci, [vp]),
        "rade_n_eoo_bits": (ci, [vp]),
        "rade_tx": (ci, [vp, vp, vp]),
        "rade_tx_set_eoo_bits": (None, [vp, vp]),
        "rade_tx_eoo": (ci, [vp, vp]),
        "rade_nin": (ci, [vp]),
        "rade_rx": (ci, [vp, vp, P(ci), vp, vp]),
        "rade_sync": (ci, [vp]),
        "rade_freq_offset": (cf, [vp]),
        "rade_snrdB_3k_est": (ci, [vp]),
    },
    "rade_core.h": {
        "rade_parse_weights": (ci, [P(P(WeightArray)), vp, ci]),
        "init_radeenc": (ci, [P(_Model), P(WeightArray), ci]),
        "init_radedec": (ci, [P(_Model), P(WeightArray), ci]),
        "rade_init_encoder": (None, [P(_State)]),
        "rade_core_encoder": (None, [P(_State), P(_Model), vp, vp, ci, ci]),
        "rade_init_decoder": (None, [P(_State)]),
        "rade_core_decoder": (None, [P(_State), P(_Model), vp, vp, ci]),
        "rade_free_encoder": (None, [P(_State)]),
        "rade_free_decoder": (None, [P(_State)]),
        "rade_reset_encoder": (None, [P(_State)]),
        "rade_reset_decoder": (None, [P(_State)]),
    },
    "rade_batch.h": {
        "rade_batch_open": (vp, [cp, P(BatchConfig)]),
        "rade_batch_open_mem": (vp, [vp, C.c_size_t, P(BatchConfig)]),
        "rade_batch_close": (None, [vp]),
        "rade_batch_n_streams": (ci, [vp]),
        "rade_batch_tx": (ci, [vp, vp, ci, vp, cl, vp, vp]),
        "rade_batch_tx_latents": (ci, [vp, vp, ci, vp, cl, vp]),
        "rade_batch_tx_set_eoo_bits": (ci, [vp, vp]),
        "rade_batch_tx_eoo": (ci, [vp, vp, cl, vp]),
        "rade_batch_tx_reset": (None, [vp]),
        "rade_batch_encode": (ci, [vp, vp, ci, vp, vp]),
        "rade_batch_decode": (ci, [vp, vp, ci, vp, ci, vp]),
        "rade_batch_channel_symbol": (ci, [vp, vp, vp, vp, vp, ci, ci, cf, cf, cull, vp]),
        "rade_batch_channel_rs_pa": (ci, [vp, vp, vp, vp, vp, ci, cf, vp, cf, cull, vp, vp]),
        "rade_batch_channel": (ci, [vp, vp, cl, vp, cl, P(ChannelParams), vp]),
        "rade_batch_tx_channel": (ci, [vp, vp, ci, vp, cl, vp, cl, vp, vp]),
        "rade_batch_channel_streams": (ci, [vp, vp, cl, vp, cl, P(ChannelParams), P(ChannelStreams), vp]),
        "rade_batch_tx_channel_streams": (ci, [vp, vp, ci, vp, cl, vp, cl, P(ChannelParams), P(ChannelStreams), vp]),
        "rade_batch_resample": (ci, [vp, vp, cl, vp, vp, cl, vp, P(ResampleParams), vp]),
        "rade_resample_count": (cll, [cll, cd, cd]),
        "rade_resample_taps": (None, [vp]),
        "rade_batch_wire_in": (ci, [vp, vp, cl, vp, ci, cf, vp, cl, vp]),
        "rade_batch_wire_out": (ci, [vp, vp, cl, vp, ci, cf, vp, cl, vp, vp]),
        "rade_batch_rate_convert": (ci, [vp, vp, cl, vp, ci, cf, vp, cl, vp, P(RateParams), vp]),
        "rade_rate_count": (cll, [cll, ci, ci]),
        "rade_rate_taps": (ci, [ci, ci, vp]),
        "rade_batch_fm_mod": (ci, [vp, vp, cl, vp, vp, cl, P(FmModParams), vp]),
        "rade_batch_fm_demod": (ci, [vp, vp, cl, vp, vp, cl, vp, P(FmDemodParams), vp]),
        "rade_fm_sigma": (cd, [cd, cd, cd, cd]),
        "rade_fm_deemph_len": (ci, [cd, cd]),
        "rade_fm_taps": (ci, [cd, cd, cd, ci, cd, vp, vp]),
        "rade_cno_plan": (ci, [P(CnoParams), P(CnoPlan)]),
        "rade_batch_cno_est": (ci, [vp, vp, cl, vp, P(CnoParams), vp, ci, vp, vp]),
        "rade_chirp": (ci, [vp, ci, cd, cd, cd]),
        "rade_batch_snr_trials": (ci, [vp, vp, P(SnrParams), vp, ci, vp]),
        "rade_snr_sigma": (cd, [cd]),
        "rade_snr_finish": (ci, [P(SnrSums), ci, cd, cd, P(SnrPoint)]),
        "rade_snr_fit": (ci, [vp, vp, ci, P(cd), P(cd)]),
        "rade_snr_track": (ci, [vp, ci, cd, cd, P(cd), vp]),
        "rade_specgram_plan": (ci, [P(SpecgramParams), P(SpecgramPlan)]),
        "rade_specgram_slices": (cll, [cll]),
        "rade_specgram_window": (None, [vp]),
        "rade_specgram_levels": (ci, [cd, cd, vp]),
        "rade_batch_specgram": (ci, [vp, vp, cl, vp, ci, cf, P(SpecgramParams), vp, cl, vp, cl, vp, vp, vp]),
        "rade_psd_plan": (ci, [ci, ci, P(PsdPlan)]),
        "rade_psd_segments": (cll, [cll, ci, ci]),
        "rade_psd_window": (ci, [ci, vp]),
        "rade_psd_octave_default": (ci, [cll, P(ci), P(ci)]),
        "rade_psd_bandwidth": (ci, [vp, ci, cd, cd, cd, P(cd), P(cd)]),
        "rade_batch_psd": (ci, [vp, vp, cl, vp, ci, cf, ci, ci, cd, vp, cl, vp, vp]),
        "rade_batch_sigstat": (ci, [vp, vp, cl, vp, ci, cf, ci, vp, vp]),
        "rade_acq_hops": (ci, [cll]),
        "rade_acq_fmax": (cd, [P(AcqHop)]),
        "rade_batch_acq_detect": (ci, [vp, vp, cl, vp, cd, vp, ci, vp, vp, cll, ci, vp]),
        "rade_acq_track": (ci, [vp, ci, ci, vp, ci, vp]),
        "rade_batch_acq_refine": (ci, [vp, vp, cl, vp, vp, ci, vp, vp, vp]),
        "rade_acq_stats": (ci, [vp, vp, ci, ci, ci, cd, cd, P(AcqResult)]),
        "rade_batch_bpf_file": (ci, [vp, vp, cl, vp, vp, cl, vp]),
        "rade_file_plan": (ci, [cll, ci, cll, cd, P(cd), P(FilePlan)]),
        "rade_batch_rx_file": (ci, [vp, vp, cl, vp, ci, ci, ci, ci, vp, vp, vp]),
        "rade_batch_ber_align": (ci, [vp, vp, cl, vp, vp, cl, vp, vp, vp]),
        "rade_ber_best": (ci, [vp, cl, P(cd)]),
        "rade_batch_multipath_gen": (ci, [vp, P(cf), ci, ci, ci, vp, cull, vp, vp]),
        "rade_batch_multipath_h": (ci, [vp, vp, ci, ci, ci, ci, cf, cf, ci, vp, vp]),
        "rade_batch_multipath_piece": (ci, [vp, vp, ci, ci, cd, cull, vp, vp, vp, cl, vp]),
        "rade_batch_channel_piece": (ci, [vp, vp, cl, vp, vp, cl, vp, P(ChannelPieceParams), vp]),
        "rade_multipath_gain": (cd, [vp, ci]),
        "rade_sigma_from_EbNodB": (cf, [cf]),
        "rade_sigma_from_EbNodB_bn1": (cf, [cf]),
        "rade_sigma_from_EbNodB_rs3": (cf, [cf]),
        "rade_batch_rx": (ci, [vp, vp, cl, P(ci), ci, vp, cl, vp, P(RxStatus), vp]),
        "rade_batch_rx_reset": (None, [vp]),
        "rade_batch_reset": (None, [vp, vp]),
        "rade_batch_rx_set_lcg": (None, [vp, P(cu)]),
        "rade_batch_rx_ideal": (ci, [vp, vp, cl, ci, P(IdealRxParams), vp, vp, vp]),
        "rade_batch_loss": (ci, [vp, vp, cl, ci, vp, vp, cl, ci, vp, vp, vp, vp, cl, vp]),
        "rade_batch_rx_get_trace": (ci, [vp, ci, P(RxTrace), vp, ci]),
        "rade_host_cpu_quota": (cd, []),
        "rade_sync_policy": (ci, [ci, cd]),
        "rade_batch_sync_counts": (None, [vp, P(cl), P(cl)]),
        "rade_batch_rx_filtered": (ci, [vp, ci, vp, ci]),
        "rade_batch_rx_stream_cycles": (ci, [vp, vp]),
        "rade_batch_profile": (None, [vp, ci]),
        "rade_batch_profile_get": (ci, [vp, ci, P(cd), P(cd), P(cl)]),
        "rade_batch_profile_ref": (None, [vp, vp]),
        "rade_batch_profile_intervals": (ci, [vp, ci, vp, vp, ci]),
        "rade_multi_open": (vp, [cp, ci, ci, cull, ci]),
        "rade_multi_close": (None, [vp]),
        "rade_multi_n_devices": (ci, [vp]),
        "rade_multi_transport": (cp, [vp]),
        "rade_multi_engine": (vp, [vp, ci, P(ci), P(ci), P(ci)]),
        "rade_multi_shard": (None, [ci, ci, ci, P(ci), P(ci)]),
        "rade_multi_foreach": (ci, [vp, C.CFUNCTYPE(ci, ci, vp, ci, ci, vp), vp]),
        "rade_multi_allreduce_sum": (ci, [vp, P(cd), ci, P(cd)]),
        "rade_sc_open": (vp, [ci, cd, cd, cd, cd, ci]),
        "rade_sc_close": (None, [vp]),
        "rade_sc_reset": (None, [vp]),
        "rade_sc_n_streams": (ci, [vp]),
        "rade_sc_n_tx_out": (ci, [vp]),
        "rade_sc_nin_max": (ci, [vp]),
        "rade_sc_n_payload": (ci, [vp]),
        "rade_sc_rrc": (None, [vp, vp]),
        "rade_sc_tx": (ci, [vp, vp, ci, vp, cl, vp]),
        "rade_sc_rx": (ci, [vp, vp, cl, ci, ci, vp, vp, vp, vp, vp]),
        "rade_train_open": (vp, [ci, ci, ci, ci]),
        "rade_train_close": (None, [vp]),
        "rade_train_n_floats": (cl, []),
        "rade_train_n_params": (ci, []),
        "rade_train_param": (ci, [ci, P(cp), P(cl), P(ci), P(ci)]),
        "rade_train_dec_forward": (ci, [vp, vp, vp, ci, ci, vp, vp]),
        "rade_train_saved_x": (ci, [vp, vp, vp]),
        "rade_train_loss": (ci, [vp, vp, vp, vp, vp]),
        "rade_train_dec_backward": (ci, [vp, vp, vp, vp, vp, vp]),
        "rade_train_adam": (ci, [vp, vp, vp, vp, vp, cd, cd, cd, vp]),
        "rade_train_dec_step": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, cd, cd, cd, vp]),
        "rade_train_profile": (ci, [vp, ci]),
        "rade_train_profile_get": (ci, [vp, P(cd)]),
    },
}
SC_SYMBOLS = [n for n in PROTOTYPES["rade_batch.h"] if n.startswith("rade_sc_")]
CORE_SYMBOLS = list(PROTOTYPES["rade_core.h"])
# The trials of the pilot SNR estimator (BatchStages.snr_trials, snr_sweep).  Its symbols are kept in a list of their own, as the single-carrier ones are, and NOT in
# EXPORTED_SYMBOLS: tests/test_abi_host.py pins EXPORTED_SYMBOLS member for member, and a change that adds a stage does not edit existing tests.  build() checks every
# name of PROTOTYPES whatever list it is in; fold this one into EXPORTED_SYMBOLS when that pinned list is next updated.
SNR_SYMBOLS = [n for n in PROTOTYPES["rade_batch.h"] if n.startswith(("rade_snr_", "rade_batch_snr_"))]
# The decoder's training step (radae_amd/train.py), a handle of its own: kept out of EXPORTED_SYMBOLS for the same reason.
TRAIN_SYMBOLS = [n for n in PROTOTYPES["rade_batch.h"] if n.startswith("rade_train_")]
EXPORTED_SYMBOLS = list(PROTOTYPES["rade_api.h"]) + [n for n in PROTOTYPES["rade_batch.h"] if n not in SC_SYMBOLS and n not in SNR_SYMBOLS and n not in TRAIN_SYMBOLS]
FILE_STATUS = ("ok", "not acquired", "refine window outside the stream", "timing inside the first cyclic prefix: not decoded", "fewer than two modem frames left: not decoded")   # RADE_FILE_*

_lib = None


def load_library() -> C.CDLL:
    """dlopen radae_amd/libradehip.so and declare the C ABI.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"or `make -C radae_amd/csrc` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    for table in PROTOTYPES.values():
        for name, (restype, argtypes) in table.items():
            if hasattr(L, name):                  # a symbol the library lacks is skipped: it is absent from older A/B builds loaded through $RADE_LIBRADEHIP
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L
