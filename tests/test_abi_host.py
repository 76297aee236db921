"""radae_amd/abi.py against include/rade_api.h, rade_core.h and rade_batch.h, on the CPU.  The binding states the C ABI once, as ctypes; a `c_int` where the header says
`long`, or a structure field out of place, fails nowhere on the host and smashes a stack on the device box.  So:

1. every function the headers declare has an entry in abi.PROTOTYPES and the reverse, in the headers' order, with the same number of arguments and the same class
   (pointer, i32, u32, i64, u64, f32, f64, void) of each argument and of the return value;
2. every ctypes structure of abi.STRUCTS has the size, field offsets and field sizes the host compiler gives its typedef;
3. the comparison rejects what it is for: doctored header text is reported as a mismatch that names the function or field;
4. the names the four binding modules offered before abi.py / stages.py were split off are all still there, and the derived symbol lists have the members pinned
   here, no more and no fewer (EXPORTED_SYMBOLS: every function of rade_api.h and rade_batch.h but the single-carrier modem's, which SC_SYMBOLS lists).

The header parser and the compiler's layout probe are tests/c_decl.py's, shared with the private ABI's check (tests/test_dev_abi_host.py)."""
import ctypes as C
import os

import pytest

from c_decl import c_layouts, function_mismatches, layout_mismatches, parse
from radae_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("rade_api.h", "rade_core.h", "rade_batch.h")


def header_texts():
    return {h: open(os.path.join(REPO, "include", h)).read() for h in HEADERS}


# ================================================================================================================================================================
# the comparison: a list of mismatches, each naming its function or field
# ================================================================================================================================================================
def compare_functions(texts):
    bad = []
    for h in HEADERS:
        funcs, _ = parse(texts[h])
        table = abi.PROTOTYPES[h]
        if list(funcs) != list(table):
            bad += [f"{h}: {n} is declared and has no table entry" for n in funcs if n not in table]
            bad += [f"{h}: the table's {n} is not declared" for n in table if n not in funcs]
            both = zip([n for n in funcs if n in table], [n for n in table if n in funcs])
            bad += [f"{h}: the table's order differs from the header's at {a} / {b}" for a, b in both if a != b][:1]
        bad += function_mismatches(funcs, table)
    return bad


def compare_layouts(texts, tmp):
    for h in HEADERS:
        open(os.path.join(str(tmp), h), "w").write(texts[h])
    want = c_layouts([os.path.join(str(tmp), h) for h in HEADERS], [str(tmp)], str(tmp))
    # (RADEEnc.input_dim and RADEDec.output_dim share one mirror: `dim`)
    return layout_mismatches(abi.STRUCTS, want, lambda cn, pn: cn == pn or cn.endswith("_" + pn))


# ================================================================================================================================================================
# 1, 2. the headers as they are
# ================================================================================================================================================================
def test_every_prototype_agrees_with_its_header():
    texts = header_texts()
    n = sum(len(parse(t)[0]) for t in texts.values())
    print(f"{n} functions declared in {', '.join(HEADERS)}")
    assert n >= 106 and n == sum(len(t) for t in abi.PROTOTYPES.values())
    bad = compare_functions(texts)
    assert not bad, "\n".join(bad)


def test_every_structure_has_the_compilers_layout(tmp_path):
    structures = {v for v in vars(abi).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert structures == set(abi.STRUCTS.values()), "a ctypes structure of abi.py is missing from abi.STRUCTS"
    declared = {t for text in header_texts().values() for t in parse(text)[1]}
    assert declared - {"RADE_COMP"} == set(abi.STRUCTS), "a typedef of the headers has no mirror (RADE_COMP is complex64 memory: numpy's)"
    bad = compare_layouts(header_texts(), tmp_path)
    assert not bad, "\n".join(bad)


# ================================================================================================================================================================
# 3. the checker rejects what it is for
# ================================================================================================================================================================
def doctored(header, old, new):
    texts = header_texts()
    assert texts[header].count(old) == 1, f"{old!r} is not unique in {header}"
    texts[header] = texts[header].replace(old, new)
    return texts


@pytest.mark.parametrize("header, old, new, needles", [
    ("rade_batch.h", "int rade_batch_tx_eoo(rade_batch *h, void *iq_out_dev, long iq_stride, void *stream);",
     "int rade_batch_tx_eoo(rade_batch *h, void *iq_out_dev, void *stream);", ("rade_batch_tx_eoo", "3 arguments")),                 # one parameter dropped
    ("rade_batch.h", "int rade_batch_tx_latents(rade_batch *h, const float *z_dev, int n_mf, void *iq_out_dev, long iq_stride, void *stream);",
     "int rade_batch_tx_latents(rade_batch *h, const float *z_dev, int n_mf, void *iq_out_dev, int iq_stride, void *stream);",
     ("rade_batch_tx_latents", "argument 4 is i32")),                                                                                   # a long turned int
    ("rade_batch.h", "float rade_sigma_from_EbNodB(float EbNodB);", "float rade_sigma_from_EbNodB(double EbNodB);",
     ("rade_sigma_from_EbNodB:", "argument 0 is f64")),                                                                                # a float turned double
    ("rade_api.h", "RADE_EXPORT float rade_freq_offset(struct rade *r);", "RADE_EXPORT double rade_freq_offset(struct rade *r);",
     ("rade_freq_offset", "returns f64")),
    ("rade_core.h", "void rade_free_encoder(RADEEncState *enc_state);", "void rade_free_encoder(RADEEncState *enc_state);\nvoid rade_new_entry(int x);",
     ("rade_new_entry", "no table entry")),
], ids=["parameter_dropped", "long_turned_int", "float_turned_double", "return_turned_double", "function_added"])
def test_the_function_check_rejects(header, old, new, needles):
    bad = compare_functions(doctored(header, old, new))
    assert bad and all(needles[0] in b for b in bad) and all(n in bad[0] for n in needles), bad


def test_the_function_check_names_what_it_cannot_parse():
    with pytest.raises(ValueError, match="rade_batch_n_streams"):
        compare_functions(doctored("rade_batch.h", "int rade_batch_n_streams(const rade_batch *h);", "int rade_batch_n_streams(rade_batch h);"))


def test_the_layout_check_rejects_swapped_fields(tmp_path):
    """two adjacent fields of different size: rade_fm_demod_params' `void *bb_out_dev; long bb_stride` are of one size, `const float *b1; int N1` are not"""
    bad = compare_layouts(doctored("rade_batch.h", "const float *b1; int N1;", "int N1; const float *b1;"), tmp_path)
    assert bad and all(b.startswith(("rade_fm_demod_params.N1:", "rade_fm_demod_params.b1:")) for b in bad) and len(bad) == 2, bad


# ================================================================================================================================================================
# 4. names: what `dir()` of each module held before the split (imported names left out; the private names other files use kept)
# ================================================================================================================================================================
NAMES = {
    "engine": """BOTTLENECK1 BYPASS_DEC BatchConfig BatchEngine CNO_FS CNO_HOP ChannelParams ChannelStreams ClockOffset CnoParams CnoPlan CnoResult DEFAULT_BLOB EQ_MODES
        EXPORTED_SYMBOLS FEAT_MF FM_C64 FM_DE_EMP_TC FM_F32 FM_OUT_COMPLEX FM_OUT_REAL FmDemodParams FmDemodulator FmModParams FmModulator IdealRxParams LIB_PATH NEOO NEOO_BITS
        NIN_MAX NMF RATE_C64 RATE_S16_IQ RATE_S16_REAL RESAMPLE_MODES RESAMPLE_PPM_MAX RateConverter RateParams ResampleParams RxStatus RxTrace SPEC_C64 SPEC_HI SPEC_LO SPEC_NFFT
        SPEC_S16_REAL SPEC_STEP SPEC_WIN SpecgramParams SpecgramPlan TX_BPF TX_LINEAR WIRE_IQ WIRE_REAL WireMeters ZMF _lib _per_stream _stream_ptr channel_stream_values chirp
        cno_plan cno_windows fm_deemph_len fm_pre_emphasis fm_sigma fm_taps load_library loss_lengths ppm_from_rates rate_count rate_taps resample_count resample_taps
        sigma_from_EbNodB specgram_levels specgram_plan specgram_slices specgram_window""",
    "sc": "SC_SYMBOLS ScFrame ScStatus SingleCarrierBatch _FRAME_DT main sc_rx_stream sc_tx_stream",
    "core": "CORE_SYMBOLS CoreDecoder CoreEncoder DEFAULT_BLOB WeightArray _Model _lib parse_weights",
    "api": """RADE_BATCH_TX_BPF RADE_FOFF_TEST RADE_USE_C_DECODER RADE_USE_C_ENCODER RADE_VERBOSE_0 Rade radae_rx radae_rx_bypass_dec radae_rx_engine radae_tx
        radae_tx_bypass_enc""",
}
SYMBOLS = {
    "EXPORTED_SYMBOLS": """rade_acq_fmax rade_acq_hops rade_acq_stats rade_acq_track rade_batch_acq_detect rade_batch_acq_refine
        rade_batch_ber_align rade_batch_bpf_file rade_batch_rx_file rade_ber_best rade_file_plan
        rade_batch_psd rade_batch_sigstat rade_psd_bandwidth rade_psd_octave_default rade_psd_plan rade_psd_segments rade_psd_window
        rade_batch_channel_piece rade_batch_multipath_piece rade_multipath_gain
        rade_batch_channel rade_batch_channel_rs_pa rade_batch_channel_streams rade_batch_channel_symbol rade_batch_close rade_batch_cno_est rade_batch_decode
        rade_batch_encode rade_batch_fm_demod rade_batch_fm_mod rade_batch_loss rade_batch_multipath_gen rade_batch_multipath_h rade_batch_n_streams rade_batch_open
        rade_batch_open_mem rade_batch_profile rade_batch_profile_get rade_batch_profile_intervals rade_batch_profile_ref rade_batch_rate_convert rade_batch_resample
        rade_batch_reset rade_batch_rx rade_batch_rx_filtered rade_batch_rx_get_trace rade_batch_rx_ideal rade_batch_rx_reset rade_batch_rx_set_lcg rade_batch_rx_stream_cycles
        rade_batch_specgram rade_batch_sync_counts rade_batch_tx rade_batch_tx_channel rade_batch_tx_channel_streams rade_batch_tx_eoo rade_batch_tx_latents rade_batch_tx_reset
        rade_batch_tx_set_eoo_bits rade_batch_wire_in rade_batch_wire_out rade_chirp rade_close rade_cno_plan rade_finalize rade_fm_deemph_len rade_fm_sigma rade_fm_taps
        rade_freq_offset rade_host_cpu_quota rade_initialize rade_multi_allreduce_sum rade_multi_close rade_multi_engine rade_multi_foreach rade_multi_n_devices rade_multi_open
        rade_multi_shard rade_multi_transport rade_n_eoo_bits rade_n_features_in_out rade_n_tx_eoo_out rade_n_tx_out rade_nin rade_nin_max rade_open rade_rate_count
        rade_rate_taps rade_resample_count rade_resample_taps rade_rx rade_sigma_from_EbNodB rade_sigma_from_EbNodB_bn1 rade_sigma_from_EbNodB_rs3 rade_snrdB_3k_est
        rade_specgram_levels rade_specgram_plan rade_specgram_slices rade_specgram_window rade_sync rade_sync_policy rade_tx rade_tx_eoo rade_tx_set_eoo_bits rade_version""",
    "SC_SYMBOLS": "rade_sc_close rade_sc_n_payload rade_sc_n_streams rade_sc_n_tx_out rade_sc_nin_max rade_sc_open rade_sc_reset rade_sc_rrc rade_sc_rx rade_sc_tx",
    "CORE_SYMBOLS": """init_radedec init_radeenc rade_core_decoder rade_core_encoder rade_free_decoder rade_free_encoder rade_init_decoder rade_init_encoder
        rade_parse_weights rade_reset_decoder rade_reset_encoder""",
}


@pytest.mark.parametrize("module", list(NAMES))
def test_every_earlier_name_is_still_an_attribute(module):
    import importlib
    mod = importlib.import_module("radae_amd." + module)
    missing = [n for n in NAMES[module].split() if not hasattr(mod, n)]
    assert not missing, f"radae_amd.{module} lost {missing}"


def test_the_derived_symbol_lists_kept_their_members():
    from radae_amd import core, engine, sc
    for mod, name in ((engine, "EXPORTED_SYMBOLS"), (sc, "SC_SYMBOLS"), (core, "CORE_SYMBOLS")):
        got = list(getattr(mod, name))
        assert sorted(got) == sorted(SYMBOLS[name].split()), name
