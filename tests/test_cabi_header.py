"""include/tokenhmr_hip.h against its ctypes binding (tokenhmr_amd/_cabi.py), over the WHOLE header and without a device: every struct
mirror against the layout a host compiler gives the header's struct, every mirrored constant against the header's value, every declared
function exported and typed in both builds, and the one rule that types the parameters."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tokenhmr_amd import _cabi


@pytest.fixture(scope="module")
def header():
    with open(_cabi.HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def header_structs(header):
    """{struct: [field names in order]} of every `typedef struct [tag] { ... } name;` of the header."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", header):
        decls = [d for d in (d.strip() for d in body.split(";")) if d]
        out[name] = [re.sub(r"\[[^\]]*\]|\*", " ", part).split()[-1] for d in decls for part in d.split(",")]
    return out


@pytest.fixture(scope="module")
def compiled(header, tmp_path_factory):
    """What a host compiler says of the header: {("sizeof", struct): n, ("field", struct, name): (offset, size), ("const", NAME): value}.
    One program with its own main, compiled host-only by the compiler build() uses; the fields it asks for are the mirrors' _fields_, so
    a name the header lacks fails the compile."""
    import __graft_entry__
    d = tmp_path_factory.mktemp("cabi_header")
    lines = ["#include <cstddef>", "#include <cstdio>", f'#include "{_cabi.HEADER}"', "int main() {"]
    for s, cls in _cabi.STRUCTS.items():
        lines.append(f'    printf("sizeof {s} %zu\\n", sizeof({s}));')
        lines += [f'    printf("field {s} {n} %zu %zu\\n", offsetof({s}, {n}), sizeof((({s}*)0)->{n}));' for n, *_ in cls._fields_]
    lines += [f'    printf("const {c} %lld\\n", (long long)({c}));' for c in sorted(set(re.findall(r"\bTHMR_[A-Z0-9_]+\b", header)))]
    (d / "layout.cpp").write_text("\n".join(lines + ["    return 0;", "}"]) + "\n")
    r = subprocess.run([__graft_entry__._hipcc(), "-std=c++17", str(d / "layout.cpp"), "-o", str(d / "layout")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    out = {}
    for w in subprocess.run([str(d / "layout")], capture_output=True, text=True, check=True).stdout.splitlines():
        w = w.split()
        if w[0] == "field":
            out[tuple(w[:3])] = (int(w[3]), int(w[4]))
        else:
            out[tuple(w[:2])] = int(w[2])
    return out


def test_every_struct_mirror_has_the_compilers_layout(header, compiled):
    structs = header_structs(header)
    assert set(_cabi.STRUCTS) == set(structs) and len(structs) == 21
    for s, cls in _cabi.STRUCTS.items():
        assert [n for n, *_ in cls._fields_] == structs[s], s
        assert C.sizeof(cls) == compiled[("sizeof", s)], s
        for n, *_ in cls._fields_:
            f = getattr(cls, n)
            assert (f.offset, f.size) == compiled[("field", s, n)], (s, n)


def test_every_mirrored_constant_has_the_headers_value(compiled):
    consts = {k[1][len("THMR_"):]: v for k, v in compiled.items() if k[0] == "const"}
    pairs = {n for n in consts if isinstance(getattr(_cabi, n, None), int)}
    for n in pairs:
        assert getattr(_cabi, n) == consts[n], n
    assert len(pairs) >= 30 and "ABI_VERSION" in pairs
    for family, least in (("ERR_", 5), ("CFG_", 3), ("PNG_", 5), ("RENDER_", 3), ("SHEET_", 6), ("VAL_LOSS_", 3), ("LIGHT_", 2)):
        assert sum(n.startswith(family) for n in pairs) >= least, family
    # the three name lists are indexed by the header's enum values
    for names, prefix in ((_cabi.GEMM_KINDS, "GEMM_"), (_cabi.VIT_PATHS, "VIT_PATH_"), (_cabi.ATTN_KINDS, "ATTN_")):
        assert [consts[prefix + n.upper()] for n in names] == list(range(len(names))), prefix
        assert sum(n.startswith(prefix) for n in consts) == len(names), prefix
    assert len(_cabi.PROF_NAMES) == consts["PROF_NUM"]          # the spellings are keys of the benchmark's output, not the header's


@pytest.mark.parametrize("exp", [False, True])
def test_every_declared_function_is_exported_and_typed(built_lib, header, exp):
    lib = _cabi.load(exp=exp)
    declared = _cabi.declared_functions()
    assert sorted(declared) == _cabi.declared_symbols() and len(declared) >= 90
    for name, (ret, params) in declared.items():
        assert hasattr(lib, name), name
        fn = getattr(lib, name)
        assert isinstance(fn.argtypes, list) and len(fn.argtypes) == len(params), name
        # the parameter count again, without the parser: the commas of the prototype
        (args,) = re.findall(r"\b%s\s*\(([^()]*)\)\s*;" % name, header)
        assert len(fn.argtypes) == (0 if args.strip() == "void" else args.count(",") + 1), name
        assert ret == _cabi.declared_return_types()[name]


def test_the_type_rule_on_synthetic_prototypes():
    vp, P = C.c_void_p, C.POINTER
    text = """typedef struct thmr_thing thmr_thing;   /* an opaque handle */
    int thmr_a(int a, int32_t b, int64_t c, float d, double e, size_t f);
    int64_t thmr_b(const thmr_config* cfg, thmr_png_item* item /* (n) */, const char** name, thmr_thing** out, void** ptr_dev);
    void thmr_c(size_t* a, int64_t* b, uint64_t* c);
    const char* thmr_d(void* a, const float* b, int32_t* c, const uint8_t* d, int16_t* e,
                       const thmr_thing* f);
    int  thmr_e(void);
    """
    funcs, opaque = _cabi.parse_prototypes(text)
    assert opaque == {"thmr_thing"} and {n: r for n, (r, _) in funcs.items()} == {"thmr_a": "int", "thmr_b": "int64_t", "thmr_c": "void",
                                                                                 "thmr_d": "const char*", "thmr_e": "int"}
    types = {n: [_cabi.param_ctype(t, opaque) for t in p] for n, (_, p) in funcs.items()}
    assert types["thmr_a"] == [C.c_int, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t]
    assert types["thmr_b"] == [P(_cabi.Config), P(_cabi.PngItem), P(C.c_char_p), P(vp), P(vp)]
    assert types["thmr_c"] == [P(C.c_size_t), P(C.c_int64), P(C.c_uint64)]
    assert types["thmr_d"] == [vp] * 6 and types["thmr_e"] == []
    for unknown in ("uint64_t", "long", "long*", "thmr_other*", "thmr_config", "thmr_config**", "float***", "char*", ""):
        with pytest.raises(RuntimeError, match="parameter of type"):
            _cabi.param_ctype(unknown, opaque)
    with pytest.raises(RuntimeError, match="parameter of type"):
        _cabi.param_ctype("thmr_thing*")                        # a handle only where the text declares it
    # what bind() does with a library that lacks a declared symbol
    libc = C.CDLL(None)
    with pytest.raises(RuntimeError, match="thmr_abi_version"):
        _cabi.bind(libc)
    assert _cabi.bind(libc, partial=True) is libc
