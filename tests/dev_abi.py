"""The private ABI behind the unit tests, as ctypes, stated once: the launch shims and argument records of radae_amd/csrc/rade_dev.h and the host helpers of rade_host.h.
A plain module beside gpu_kit.py; holds no tests.  The public ABI is radae_amd/abi.py's.

PROTOTYPES is not typed: it is derived from the two headers' text with c_decl.parse, every function they declare, by class --
    ptr c_void_p | i32 c_int | u32 c_uint | i64 c_longlong | u64 c_ulonglong (size_t: c_size_t) | f32 c_float | f64 c_double | void None
-- so it cannot fall behind the headers in the tree.  A pointer argument takes what the tests hand it: tensor.data_ptr(), C.byref(record), arr.ctypes.data_as(..), a
ctypes array or pointer, bytes, None.  tests/test_dev_abi_host.py holds the derivation to answers typed there.

STRUCTS mirrors the ten records the tests fill or read, not all of them.  load() refuses a mirror whose member names do not follow the header's, in order (no compiler
needed: this also runs where only the GPU tests run); sizes and offsets are held to the host compiler's in tests/test_dev_abi_host.py."""
import ctypes as C
import os

import c_decl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = [os.path.join(REPO, "radae_amd", "csrc", h) for h in ("rade_dev.h", "rade_host.h")]
INCLUDE_DIRS = [os.path.join(REPO, "include"), os.path.join(REPO, "radae_amd", "csrc")]
CTYPES = {"ptr": C.c_void_p, "i32": C.c_int, "u32": C.c_uint, "i64": C.c_longlong, "u64": C.c_ulonglong, "usize": C.c_size_t, "f32": C.c_float, "f64": C.c_double,
          "void": None}


def header_texts():
    return [open(h).read() for h in HEADERS]


def derive(texts):
    """{function: (restype, argtypes)} for every function the header texts declare"""
    table = {}
    for text in texts:
        for name, (ret, args) in c_decl.parse(text, {**c_decl.SCALARS, "size_t": "usize"})[0].items():
            table[name] = (CTYPES[ret], [CTYPES[a] for a in args])
    return table


PROTOTYPES = derive(header_texts())

# ---- the records ---------------------------------------------------------------------------------------------------------------------------------------------------
STRUCTS = {}                            # typedef name -> its ctypes mirror
vp, ci, cl, cf, pf = C.c_void_p, C.c_int, C.c_long, C.c_float, C.POINTER(C.c_float)


def _struct(name, typedef, fields):
    STRUCTS[typedef] = type(name, (C.Structure,), {"_fields_": fields})
    return STRUCTS[typedef]


GemmArgs = _struct("GemmArgs", "rd_gemm_args", [
    ("a1", vp), ("a1_sb", cl), ("a1_st", cl), ("K1", ci), ("a0", vp), ("a0_sb", cl), ("a0_st", cl), ("K0", ci),
    ("reset", vp), ("reset_sb", ci), ("n_rows", vp), ("Wp", vp), ("bias", vp), ("Wp16", vp), ("Wscale", vp),
    ("y", vp), ("y_sb", cl), ("y_st", cl), ("N", ci), ("B", ci), ("T", ci), ("act", ci)])
ScanArgs = _struct("ScanArgs", "rd_scan_args", [
    ("gi", vp), ("gi_sb", cl), ("gi_st", cl), ("Whh", vp), ("bhh", vp), ("h", vp), ("out", vp), ("out_sb", cl), ("out_st", cl),
    ("reset", vp), ("reset_sb", ci), ("n_rows", vp), ("B", ci), ("T", ci), ("H", ci), ("outf", vp), ("outf_NQ", ci), ("outf_col", ci)])
EncfArgs = _struct("EncfArgs", "rd_encf_args", [
    ("xf", vp), ("NQ", ci), ("B", ci), ("T", ci), ("K0", ci), ("K1", ci), ("dil", ci), ("Wp16", vp), ("Wscale", vp), ("bias", vp), ("N", ci), ("act", ci),
    ("y", vp), ("y_sb", cl), ("y_st", cl), ("yf", vp), ("ycol", ci), ("seq_taps", ci), ("no_pair", ci), ("pair", ci), ("xin", vp), ("Kin", ci), ("Wp", vp)])
Tables = _struct("Tables", "rd_tables", [
    ("Winv", cf * (30 * 160 * 2)), ("Wfwd", cf * (160 * 30 * 2)), ("P", cf * 30), ("Pend", cf * 30), ("p", cf * 320), ("pend", cf * 320), ("eoo", cf * 2304),
    ("Pmat", cf * 360), ("eq_rot", cf * 60), ("bpf_h", cf * 104), ("bpf_E", cf * 2304), ("p_w", cf * 12800), ("fcoarse", C.c_double * 40),
    ("pilot_gain", cf), ("snr_c1", cf), ("snr_c2", cf), ("pad", cf)])
ChanArgs = _struct("ChanArgs", "rd_chan_args", [
    ("tab", vp), ("tx", vp), ("tx_stride", cl), ("rx", vp), ("rx_stride", cl), ("G", vp), ("noise", vp), ("eoo", vp), ("scratch", vp), ("mp", vp),
    ("B", ci), ("n_sig", ci), ("n_pre", ci), ("n_post", ci), ("with_eoo", ci), ("sigma", cf), ("freq_offset", cf), ("df_dt", cf), ("seed", C.c_ulonglong),
    ("sine_amp", cf), ("sine_freq", cf), ("rx_gain", cf), ("ps", vp)])
BpfState = _struct("BpfState", "rd_bpf_state", [("mem_len", ci), ("grid_off", ci), ("phase", cf * 2), ("mem", cf * (2 * 102))])
BpfArgs = _struct("BpfArgs", "rd_bpf_args", [
    ("state", vp), ("state_stride", cl), ("len0", vp), ("len0_stride", cl), ("len0_const", ci), ("avail", vp), ("avail_const", ci), ("tab", vp), ("bpf16", vp),
    ("x", vp), ("x_stride", cl), ("y", vp), ("y_stride", cl), ("chain", vp), ("chain_stride", ci), ("n_blocks", ci), ("B", ci), ("clip", ci), ("advance", ci),
    ("zero_acc", vp), ("zero_progress", vp)])
Lin = _struct("Lin", "rd_linear", [("n_in", ci), ("n_out", ci), ("w", pf), ("b", pf), ("row_scale", pf)])
Gru = _struct("Gru", "rd_gru", [("n_in", ci), ("hid", ci), ("w_ih", pf), ("w_hh", pf), ("b_ih", pf), ("b_hh", pf), ("s_ih", pf), ("s_hh", pf)])
Model = _struct("Model", "rd_model", [
    ("enc_dense1", Lin), ("enc_zdense", Lin), ("dec_dense1", Lin), ("dec_output", Lin), ("enc_gru", Gru * 5), ("dec_gru", Gru * 5),
    ("enc_conv", Lin * 5), ("dec_conv", Lin * 5), ("dec_glu", Lin * 5)])


def name_mismatches(texts):
    """every mirror whose member names are not the header texts' record's, in order"""
    declared = {}
    for text in texts:
        declared.update(c_decl.parse(text)[1])
    return [f"{t}: the mirror's members {[n for n, _ in cls._fields_]} do not follow the header's {declared.get(t)}"
            for t, cls in STRUCTS.items() if [n for n, _ in cls._fields_] != declared.get(t)]


_lib = None


def load():
    """radae_amd.abi.load_library()'s handle with the private prototypes declared on it as well, once (a symbol the library lacks is skipped, as there)"""
    global _lib
    if _lib is None:
        bad = name_mismatches(header_texts())
        assert not bad, "\n".join(bad)
        from radae_amd import abi
        L = abi.load_library()
        for name, (restype, argtypes) in PROTOTYPES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib
