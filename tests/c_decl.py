"""What a C header declares, read from its text, and what the host compiler makes of its structures: the parser and the layout probe behind tests/test_abi_host.py
(radae_amd/abi.py against the public headers) and tests/dev_abi.py / tests/test_dev_abi_host.py (the private launch shims and host helpers of radae_amd/csrc/rade_dev.h and
rade_host.h).  A plain module beside gpu_kit.py; holds no tests and no fixtures.

A declaration is reduced to classes: pointer, i32, u32, i64, u64, f32, f64, void -- what decides how an argument travels.  A structure is reduced to its member names
in order; sizes and offsets come from the compiler (c_layouts), never from the parser."""
import ctypes as C
import os
import re
import shutil
import subprocess

SCALARS = {"void": "void", "int": "i32", "unsigned": "u32", "unsigned int": "u32", "long": "i64", "long long": "i64", "unsigned long": "u64",
           "unsigned long long": "u64", "size_t": "u64", "float": "f32", "double": "f64", "int32_t": "i32", "uint32_t": "u32", "int64_t": "i64", "uint64_t": "u64"}
BASE_WORDS = {w for k in SCALARS for w in k.split()}


# ================================================================================================================================================================
# the parser: comments and the preprocessor out, statements split at top-level semicolons, parameters at top-level commas
# ================================================================================================================================================================
def statements(text):
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = text.replace('extern "C" {', " ").replace("RADE_EXPORT", " ").replace("__host__ __device__", " ")
    out, cur, depth = [], "", 0
    for ch in text:
        depth += (ch in "{(") - (ch in "})")
        if depth < 0:                      # the brace that closes extern "C"
            depth = 0
        elif ch == "}" and depth == 0 and cur.split()[:2] == ["static", "inline"]:      # a definition with its body: not part of the ABI
            cur = ""
        elif ch == ";" and depth == 0:
            out.append(" ".join(cur.split())); cur = ""
        else:
            cur += ch
    assert not cur.strip(), f"text behind the last declaration: {cur.strip()[:80]!r}"
    return [s for s in out if s]


def split_top(s, sep=","):
    out, cur, depth = [], "", 0
    for ch in s:
        depth += (ch in "{([") - (ch in "})]")
        if ch == sep and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    return [p.strip() for p in out + [cur] if p.strip()]


def type_class(decl, pointer_types, named, scalars=SCALARS):
    """the class of a parameter (named: its name may follow the type) or of a return type; a function pointer or an array parameter is a pointer"""
    if any(c in decl for c in "*[("):
        return "ptr"
    w = [t for t in decl.split() if t not in ("const", "signed")]
    if named and len(w) > 1 and w[-1] not in BASE_WORDS:
        w.pop()
    if len(w) == 1 and w[0] in pointer_types:
        return "ptr"
    return scalars[" ".join(w)]            # KeyError: the caller names the declaration


def parse(text, scalars=SCALARS):
    """(functions {name: (return class, [argument classes])} in the text's order, structures {typedef name: [field names]}); ValueError names what it cannot read"""
    funcs, structs, pointer_types = {}, {}, set()
    for s in statements(text):
        m = re.match(r"typedef struct\s*\w*\s*\{(.*)\}\s*(\w+)$", s)
        if m:
            structs[m.group(2)] = [re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", d).group(1) for f in split_top(m.group(1), ";") for d in split_top(f)]
            continue
        m = re.match(r"typedef .*\(\s*\*\s*(\w+)\s*\)\s*\(", s) or re.match(r"typedef [^()]*\*\s*(\w+)$", s)      # a function pointer; a pointer
        if m:
            pointer_types.add(m.group(1))
            continue
        if re.match(r"(typedef struct \w+ \w+|struct \w+|enum\s*\{.*\}|extern [^()]*)$", s):      # opaque handles, enumerations, data
            continue
        m = re.match(r"(.*?)(\w+)\s*\((.*)\)$", s)
        try:
            params = [] if m.group(3).strip() == "void" else split_top(m.group(3))
            funcs[m.group(2)] = (type_class(m.group(1), pointer_types, False, scalars), [type_class(p, pointer_types, True, scalars) for p in params])
        except (AttributeError, KeyError):
            raise ValueError(f"cannot parse the declaration {s!r}") from None
    return funcs, structs


def ctype_class(t):
    if t is None:
        return "void"
    if issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p, C.Array, C._CFuncPtr)):
        return "ptr"
    return {"i": "i32", "I": "u32", "l": "i64", "q": "i64", "L": "u64", "Q": "u64", "f": "f32", "d": "f64"}[t._type_]


# ================================================================================================================================================================
# the comparisons: a list of mismatches, each naming its function or field
# ================================================================================================================================================================
def function_mismatches(funcs, table):
    """parse()'s functions against {name: (restype, argtypes)} of ctypes types, for the names both have"""
    bad = []
    for n, (ret, args) in funcs.items():
        if n not in table:
            continue
        restype, argtypes = table[n]
        if ctype_class(restype) != ret:
            bad.append(f"{n}: returns {ret}, the table says {ctype_class(restype)}")
        got = [ctype_class(a) for a in argtypes]
        if len(got) != len(args):
            bad.append(f"{n}: {len(args)} arguments, the table has {len(got)}")
        bad += [f"{n}: argument {i} is {a}, the table says {g}" for i, (a, g) in enumerate(zip(args, got)) if a != g]
    return bad


def c_layouts(headers, include_dirs, tmp):
    """{typedef: (sizeof, [(field, offset, size)])} from the host compiler, for every structure typedef of the header files (paths; compiled as plain C in this order)"""
    cc = shutil.which("cc")
    assert cc, "no host C compiler `cc` (build() needs one too)"
    structs = {}
    for h in headers:
        structs.update(parse(open(h).read())[1])
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{os.path.abspath(h)}"' for h in headers] + ["int main(void) {"]
    for t, fields in structs.items():
        lines.append(f'printf("{t} %zu\\n", sizeof({t}));')
        lines += [f'printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t} *)0)->{f}));' for f in fields]
    open(os.path.join(tmp, "layout.c"), "w").write("\n".join(lines + ["return 0; }", ""]))
    subprocess.check_call([cc] + [a for d in include_dirs for a in ("-I", d)] + ["-o", os.path.join(tmp, "layout"), os.path.join(tmp, "layout.c")])
    out = {}
    for ln in subprocess.check_output([os.path.join(tmp, "layout")], text=True).splitlines():
        name, *v = ln.split()
        if "." in name:
            out[name.split(".")[0]][1].append((name.split(".")[1], int(v[0]), int(v[1])))
        else:
            out[name] = (int(v[0]), [])
    return out


def c_values(headers, exprs, include_dirs, tmp):
    """{expression: its integer value} from the host compiler, for constant expressions over the header files' macros (function-like ones included)"""
    cc = shutil.which("cc")
    assert cc, "no host C compiler `cc` (build() needs one too)"
    lines = ["#include <stdio.h>"] + [f'#include "{os.path.abspath(h)}"' for h in headers] + ["int main(void) {"]
    lines += [f'printf("%lld\\n", (long long)({e}));' for e in exprs]
    open(os.path.join(tmp, "values.c"), "w").write("\n".join(lines + ["return 0; }", ""]))
    subprocess.check_call([cc] + [a for d in include_dirs for a in ("-I", d)] + ["-o", os.path.join(tmp, "values"), os.path.join(tmp, "values.c")])
    return dict(zip(exprs, map(int, subprocess.check_output([os.path.join(tmp, "values")], text=True).split())))


def layout_mismatches(mirrors, want, same_name=lambda c_name, mirror_name: c_name == mirror_name):
    """{typedef: ctypes structure} against c_layouts()'s answer: size, number of fields, and every field's name, offset and size"""
    bad = [f"{t}: no such typedef in the headers" for t in mirrors if t not in want]
    for t, cls in mirrors.items():
        if t not in want:
            continue
        size, fields = want[t]
        got = [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, *_ in cls._fields_]
        if C.sizeof(cls) != size or len(got) != len(fields):
            bad.append(f"{t}: {len(fields)} fields in {size} bytes, ctypes has {len(got)} in {C.sizeof(cls)}")
        for (cn, co, cs), (pn, po, ps) in zip(fields, got):
            if not same_name(cn, pn) or (co, cs) != (po, ps):
                bad.append(f"{t}.{cn}: offset {co} size {cs}, ctypes has {pn} at offset {po} size {ps}")
    return bad
