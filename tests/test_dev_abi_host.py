"""tests/dev_abi.py -- the private ABI of the unit tests: the launch shims and records of radae_amd/csrc/rade_dev.h, the host helpers of rade_host.h -- on the CPU.  A
shifted pointer in a launch record fails nowhere on the host and faults a kernel on the device box.  So:

a. every mirror of dev_abi.STRUCTS has the size, field offsets and field sizes the host compiler gives its typedef (both headers compile as plain C);
b. the prototype table is derived from the headers, so it is held to answers typed HERE once: a slip of the parser cannot agree with itself;
c. the comparisons reject what they are for: on doctored header text a `long` stride made `int`, two members swapped, a member added and an argument removed are
   each reported, naming the record or the function;
d. the library has every function of the table (a default build; rd_debug_phase_cycles2 of the -DRD_PHASE_TIMING developer build is in no header, so in no table);
e. it is stated ONCE: no .py file under tests/ but dev_abi.py assigns .argtypes / .restype or defines a ctypes.Structure."""
import ast
import glob
import os
import shutil

import pytest

import c_decl
import dev_abi

TESTS = os.path.dirname(os.path.abspath(__file__))
DEV_H, HOST_H = range(2)                # dev_abi.HEADERS


def compare_layouts(texts, tmp):
    paths = [os.path.join(str(tmp), os.path.basename(h)) for h in dev_abi.HEADERS]
    for p, text in zip(paths, texts):
        open(p, "w").write(text)
    return c_decl.layout_mismatches(dev_abi.STRUCTS, c_decl.c_layouts(paths, [str(tmp)] + dev_abi.INCLUDE_DIRS, str(tmp)))


def compare_functions(texts):
    """the table in force against what the texts derive to"""
    funcs = {}
    for t in texts:
        funcs.update(c_decl.parse(t)[0])
    return ([f"{n} is declared and has no table entry" for n in funcs if n not in dev_abi.PROTOTYPES] + [f"the table's {n} is not declared" for n in dev_abi.PROTOTYPES if n not in funcs]
            + c_decl.function_mismatches(funcs, dev_abi.PROTOTYPES))


def doctored(which, old, new):
    texts = dev_abi.header_texts()
    assert texts[which].count(old) == 1, f"{old!r} is not unique in {dev_abi.HEADERS[which]}"
    texts[which] = texts[which].replace(old, new)
    return texts


# ================================================================================================================================================================
# a. layout
# ================================================================================================================================================================
def test_every_mirror_has_the_compilers_layout(tmp_path):
    assert len(dev_abi.STRUCTS) == 10 and not dev_abi.name_mismatches(dev_abi.header_texts())
    n = sum(1 + 3 * len(cls._fields_) for cls in dev_abi.STRUCTS.values())
    print(f"{len(dev_abi.STRUCTS)} mirrors, {n} sizes and offsets compared")
    bad = compare_layouts(dev_abi.header_texts(), tmp_path)
    assert not bad, "\n".join(bad)


# ================================================================================================================================================================
# b. the derivation against known answers
# ================================================================================================================================================================
KNOWN = {
    "rd_launch_multipath_gen": ("i32", "ptr i32 i32 i32 ptr u64 ptr ptr i32 ptr"),
    "rd_launch_carry_rows": ("i32", "ptr i32 i32 i32 i32 i32 ptr ptr"),
    "rd_launch_noise_probe": ("i32", "ptr u32 u32 ptr ptr ptr i32 i32 ptr"),
    "rd_pack_weights": ("i64", "ptr i32 i32 ptr"),
    "rd_corr_tables_check": ("f64", "ptr"),
    "rd_batch_tables": ("ptr", "ptr"),
    "rd_tables_fill": ("void", "ptr"),
}


@pytest.mark.parametrize("name", list(KNOWN))
def test_the_derived_prototype_is_the_known_one(name):
    restype, argtypes = dev_abi.PROTOTYPES[name]
    assert (c_decl.ctype_class(restype), [c_decl.ctype_class(a) for a in argtypes]) == (KNOWN[name][0], KNOWN[name][1].split())


def test_the_headers_are_read_whole():
    """48 functions and 49 structures of rade_dev.h (its three inline definitions skipped), 27 and 3 of rade_host.h; every class has one ctypes type, size_t its own"""
    import ctypes as C
    dev, host = (c_decl.parse(t) for t in dev_abi.header_texts())
    assert (len(dev[0]), len(dev[1]), len(host[0]), len(host[1])) == (48, 49, 27, 3)
    assert not {"rd_rate_tile", "rd_cno_pitch", "rd_acq_hops"} & set(dev[0]) and len(dev_abi.PROTOTYPES) == 48 + 27
    assert dev[1]["rd_tables"][7] == "Pmat" and dev[1]["rd_bpf_state"] == ["mem_len", "grid_off", "phase", "mem"]
    assert dev_abi.PROTOTYPES["rd_model_parse"] == (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p])
    assert dev_abi.PROTOTYPES["rade_wait_model_step"] == (C.c_double, [C.c_void_p, C.c_double, C.c_int])
    assert all(r is None or isinstance(r, type) for r, _ in dev_abi.PROTOTYPES.values())


# ================================================================================================================================================================
# c. the comparisons reject what they are for
# ================================================================================================================================================================
def test_the_layout_check_rejects_a_long_stride_made_int(tmp_path):
    bad = compare_layouts(doctored(DEV_H, "const float *a1; long a1_sb, a1_st; int K1;", "const float *a1; int a1_sb; long a1_st; int K1;"), tmp_path)
    assert bad and all(b.startswith("rd_gemm_args.") for b in bad) and bad[0].startswith("rd_gemm_args.a1_sb: offset 8 size 4"), bad


def test_the_layout_check_rejects_swapped_members(tmp_path):
    """two adjacent members of different size, rd_chan_args' `int .. with_eoo; float sigma` being of one size: `const int *reset; int reset_sb` of rd_scan_args"""
    texts = doctored(DEV_H, "const int *reset; int reset_sb;       /* optional [B][reset_sb]: zero h before step */", "int reset_sb; const int *reset;")
    bad = compare_layouts(texts, tmp_path)
    assert bad and all(b.startswith(("rd_scan_args.reset_sb:", "rd_scan_args.reset:")) for b in bad) and len(bad) == 2, bad
    names = dev_abi.name_mismatches(texts)                              # what load() refuses, without a compiler
    assert len(names) == 1 and names[0].startswith("rd_scan_args:"), names


def test_the_layout_check_rejects_an_added_member(tmp_path):
    texts = doctored(DEV_H, "int n_blocks;                                /* blocks of the longest stream */", "int n_blocks, n_more;")
    bad = compare_layouts(texts, tmp_path)
    assert bad and all(b.startswith("rd_bpf_args") for b in bad) and "22 fields" in bad[0] and "ctypes has 21" in bad[0], bad
    names = dev_abi.name_mismatches(texts)
    assert len(names) == 1 and names[0].startswith("rd_bpf_args:"), names
    texts = doctored(HOST_H, "float *w, *b; float *row_scale; } rd_linear;", "float *w, *b; float *row_scale; int more; } rd_linear;")      # a record of rade_host.h; rd_model holds 19 of it
    bad = compare_layouts(texts, tmp_path)
    assert bad and bad[0].startswith("rd_linear: 6 fields") and {b.split(":")[0].split(".")[0] for b in bad} == {"rd_linear", "rd_model"}, bad


def test_the_function_check_rejects_a_removed_argument():
    bad = compare_functions(doctored(DEV_H, "int rd_launch_pad_rows(const float *src, float *dst, long R, int K, int Kpad, rd_stream_t s);",
                                     "int rd_launch_pad_rows(const float *src, float *dst, long R, int K, rd_stream_t s);"))
    assert bad and all(b.startswith("rd_launch_pad_rows:") for b in bad) and "5 arguments, the table has 6" in bad[0], bad
    assert not compare_functions(dev_abi.header_texts())


# ================================================================================================================================================================
# d. symbols
# ================================================================================================================================================================
def test_the_library_has_every_function_of_the_table():
    import __graft_entry__ as ge
    ge.build()
    lib = dev_abi.load()
    missing = [n for n in dev_abi.PROTOTYPES if not hasattr(lib, n)]
    assert not missing, missing
    assert "rd_debug_phase_cycles2" not in dev_abi.PROTOTYPES
    assert dev_abi.load() is lib and lib.rd_packed_size.restype is dev_abi.PROTOTYPES["rd_packed_size"][0] and lib.rd_packed_size.argtypes is not None


# ================================================================================================================================================================
# e. stated once
# ================================================================================================================================================================
ALLOWED = {("test_host_cpu.py", "libc.free.argtypes"), ("test_host_cpu.py", "libc.free.restype")}     # a condition, not a measurement: free() of CDLL(None) is not the library's ABI


def hand_bindings(path):
    """(file name, what) for every assignment to .argtypes / .restype and every ctypes.Structure defined in the file"""
    found = []
    for node in ast.walk(ast.parse(open(path).read(), path)):
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
        for t in targets:
            found += [ast.unparse(e) for e in ast.walk(t) if isinstance(e, ast.Attribute) and e.attr in ("argtypes", "restype")]
        if isinstance(node, ast.ClassDef) and any("Structure" in ast.unparse(b) or "Union" in ast.unparse(b) for b in node.bases):
            found.append(f"class {node.name}")
        if isinstance(node, ast.Call) and ast.unparse(node.func) == "type" and len(node.args) == 3 and "Structure" in ast.unparse(node.args[1]):
            found.append("type(.., (Structure,), ..)")
    return [(os.path.basename(path), f) for f in found]


def test_the_private_abi_is_stated_once(tmp_path):
    files = sorted(glob.glob(os.path.join(TESTS, "**", "*.py"), recursive=True))
    assert len(files) > 70
    found = [f for p in files if os.path.basename(p) != "dev_abi.py" for f in hand_bindings(p)]
    assert set(found) == ALLOWED and len(found) == 2, sorted(set(found) - ALLOWED)
    assert len(hand_bindings(os.path.join(TESTS, "dev_abi.py"))) == 3                 # the scan sees the one place: restype and argtypes in load(), the records' type() call
    planted = tmp_path / "tx_ref.py"                                                  # and what it is for
    shutil.copy(os.path.join(TESTS, "tx_ref.py"), planted)
    assert hand_bindings(str(planted)) == []
    with open(planted, "a") as f:
        f.write("\n\ndef declare(L):\n    L.rd_tables_fill.restype = None; L.rd_tables_fill.argtypes = [C.POINTER(Tables)]\n\n\nclass Again(C.Structure):\n    _fields_ = []\n")
    assert sorted(hand_bindings(str(planted))) == [("tx_ref.py", "L.rd_tables_fill.argtypes"), ("tx_ref.py", "L.rd_tables_fill.restype"), ("tx_ref.py", "class Again")]
