"""No-GPU checks of the binding that sap3d_tensorflow_amd/_header.py reads from include/p3d_hip.h: the type rule pinned by
signatures spelled out here, the structure layouts against the compiler's, the reader's refusals, and completeness."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from sap3d_tensorflow_amd import _header, _lib
from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_fp, _ip, _i64p, _dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
_u8p, _i32p, _u32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)

# spelled out by hand, as the binding had them before it was read from the header
PINNED = {
    "p3d_create": (C.c_int, [C.POINTER(_lib.P3dConfig), C.POINTER(C.c_void_p)]),
    "p3d_last_error": (C.c_char_p, []),
    "p3d_param_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), _ip, _i64p, _ip]),
    "p3d_debug_bn_pass": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, _fp, C.c_int, C.c_int, _fp, C.c_int, C.c_int, _fp, C.c_int,
                                    C.c_int, C.c_int, _fp, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_int, _fp, C.c_int, C.c_int,
                                    _fp, _fp, _fp, _fp, _ip]),
    "p3d_debug_wgrad_group": (C.c_int, [C.c_int, C.c_int, C.POINTER(_fp), _ip, _ip, _i64p, C.POINTER(_fp), _ip, _ip, _i64p, _ip, _ip,
                                        C.POINTER(_fp), C.POINTER(_fp), C.c_int, C.c_int, C.c_char_p, C.c_int, _ip, _ip]),
    "p3d_get_eval_extra": (C.c_int, [C.c_void_p, _ip, C.POINTER(_fp), _ip, _ip]),
    "p3d_crc32c": (C.c_uint32, [C.c_void_p, C.c_size_t, C.c_uint32]),
    "p3d_video_reframe": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _u8p, C.POINTER(_lib.P3dReframe), _i32p, _i32p,
                                    _u32p, _u8p, _u8p, _dp]),
    "p3d_debug_fused_conv": (C.c_int, [C.c_int, C.POINTER(_lib.P3dFusedConv), C.c_char_p, C.c_int, _ip]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_derived_signature_is_the_hand_written_one(name):
    res, args = _lib.SIGNATURES[name]
    want_res, want_args = PINNED[name]
    assert res is want_res
    assert len(args) == len(want_args)
    for i, (a, w) in enumerate(zip(args, want_args)):
        assert a is w, (name, i, a, w)          # ctypes caches POINTER(T): the same type is the same object


def test_bn_pass_keeps_all_28_arguments():
    assert len(PINNED["p3d_debug_bn_pass"][1]) == 28 and len(_lib.SIGNATURES["p3d_debug_bn_pass"][1]) == 28


def test_the_type_rule_row_by_row():
    h = _header.parse("typedef struct p3d_handle p3d_handle;\n"
                      "typedef struct { int a, b[2]; const double* p; unsigned char t[3]; } p3d_s;\n"
                      "void p3d_f(p3d_handle* h, void* v, const void* cv, p3d_handle** hh, char* c, const char* cc, const char** ccp,\n"
                      "           const float* f, float** ff, const float* const* fcf, const int64_t shape[5], p3d_s* s, size_t n,\n"
                      "           unsigned char u, const unsigned char* up, double d, uint64_t q, int32_t* i32);\n"
                      "const char* p3d_g(void);\nuint32_t p3d_h(int x);\n")
    assert h.functions["p3d_f"] == (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p,
                                           C.POINTER(C.c_char_p), _fp, C.POINTER(_fp), C.POINTER(_fp), _i64p, C.POINTER(h.structs["p3d_s"]),
                                           C.c_size_t, C.c_ubyte, _u8p, C.c_double, C.c_uint64, _i32p])
    assert h.functions["p3d_g"] == (C.c_char_p, []) and h.functions["p3d_h"] == (C.c_uint32, [C.c_int])
    s = h.structs["p3d_s"]
    assert s.__name__ == "P3dS" and s._fields_ == [("a", C.c_int), ("b", C.c_int * 2), ("p", _dp), ("t", C.c_ubyte * 3)]


def test_the_twelve_structures_keep_their_names():
    assert [s.__name__ for s in _lib._H.structs.values()] == [
        "P3dConfig", "P3dAugment", "P3dOpTime", "P3dFusedBn", "P3dFusedBnGrad", "P3dFusedGate", "P3dFusedConv", "P3dPostprocess",
        "P3dHistMatch", "P3dVideoTemporal", "P3dRender", "P3dReframe"]
    for s in _lib._H.structs.values():
        assert getattr(_lib, s.__name__) is s


def _host_compiler():
    """The compiler the build uses, or the system C compiler if that is what is present."""
    from sap3d_tensorflow_amd import build
    try:
        return build._hipcc()
    except RuntimeError:
        return shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")


def test_structure_layouts_are_the_compilers(tmp_path):
    """ctypes' layout rule against the compiler's, for every struct of the header: sizeof, and offsetof of every field (the 3-byte
    tail of p3d_render and the nested arrays of p3d_fused_conv among them).  Text derivation cannot prove this on its own."""
    cc = _host_compiler()
    assert cc, "no host compiler"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "p3d_hip.h"', "int main(void) {"]
    want = []
    for cname, s in _lib._H.structs.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        want.append("%s %d" % (cname, C.sizeof(s)))
        for f, _ in s._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
            want.append("%s.%s %d" % (cname, f, getattr(s, f).offset))
    lines += ["    return 0;", "}", ""]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(want) == 12 + sum(len(s._fields_) for s in _lib._H.structs.values()) and len(want) > 100
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]


HANDLE = "typedef struct p3d_handle p3d_handle;\n"


@pytest.mark.parametrize("text,offending", [
    ("int p3d_f(long n);", "long"),                                          # a type outside the closed set
    ("int p3d_f(unsigned n);", "unsigned"),
    ("int p3d_f(float*** p);", "float*** p"),                                # a third level of pointer
    ("enum { P3D_A = 0, P3D_B };", "P3D_B"),                                 # an enumerator without a value
    ("enum { P3D_A = 1 << 2 };", "P3D_A = 1 << 2"),
    ("int p3d_f(void (*cb)(int), int n);", "(*cb)"),                         # a function-pointer parameter
    ("int p3d_f(p3d_later* s);\ntypedef struct { int a; } p3d_later;", "p3d_later"),      # a struct used before its definition
    ("typedef struct { p3d_later s; } p3d_s;\ntypedef struct { int a; } p3d_later;", "p3d_later"),
    ("int p3d_counter;", "int p3d_counter"),                                 # a stray statement
    ("static const int p3d_n = 3;", "static const int p3d_n = 3"),
    ("typedef int p3d_int;", "typedef int p3d_int"),
    ("int p3d_f(int n)", "int p3d_f(int n)"),                                # no `;`
    ("int p3d_f(int);", "'int'"),                                            # a parameter without a name
    ("typedef struct { float* a, b; } p3d_s;", "float* a, b"),               # declarators after a pointer: not what it looks like
    ("typedef struct { int a : 3; } p3d_s;", "int a : 3"),                   # a bit field
    ("#if 0\nint p3d_f(int n);\n#endif", "#if 0"),                           # a conditional the reader would misread
    ("#pragma pack(1)", "#pragma pack(1)"),
])
def test_reader_refuses_what_it_cannot_place(text, offending):
    with pytest.raises(_header.HeaderError) as e:
        _header.parse(HANDLE + text)
    assert offending in str(e.value), str(e.value)


def test_defines_other_than_integers_are_skipped_by_rule():
    h = _header.parse("#ifndef P3D_X_H\n#define P3D_X_H\n#include <stdint.h>\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
                      "#define P3D_N 0x10   /* sixteen */\n#define P3D_MASK (P3D_N | 1)\nenum { P3D_A = -1, P3D_B = 2 };\n"
                      "#ifdef __cplusplus\n}\n#endif\n#endif\n")
    assert h.constants == {"P3D_N": 16, "P3D_A": -1, "P3D_B": 2} and not h.functions and not h.structs


def test_every_declared_symbol_is_derived_and_nothing_else():
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    assert len(_lib.SIGNATURES) >= 230


# Python-side name -> the header's name and its number, for every dict and scalar of _lib.py and session.py that has a header name
NAMES = {
    "LOSSES": {"smooth_l1": ("P3D_LOSS_SMOOTH_L1", 0), "bce": ("P3D_LOSS_BCE", 1), "l1": ("P3D_LOSS_L1", 2)},
    "REGULARIZATION": {"weightdecay": ("P3D_REG_WEIGHT_DECAY", 1), "l2": ("P3D_REG_L2", 2)},
    "OPTIMIZERS": {"adam": ("P3D_OPT_ADAM", 0), "momentum": ("P3D_OPT_MOMENTUM", 1), "sgd": ("P3D_OPT_SGD", 2)},
    "NORMS": {"none": ("P3D_NORM_NONE", 0), "max": ("P3D_NORM_MAX", 1), "range": ("P3D_NORM_RANGE", 2)},
    "MATCH_MODES": {"off": ("P3D_MATCH_OFF", 0), "table": ("P3D_MATCH_TABLE", 1), "density": ("P3D_MATCH_DENSITY", 2)},
    "EVAL_EXTRA": {"kldiv": ("P3D_EVAL_KLDIV", 1), "info_gain": ("P3D_EVAL_INFO_GAIN", 2)},
    "VIDEO_MODES": {"newest": ("P3D_VIDEO_NEWEST", 0), "mean": ("P3D_VIDEO_MEAN", 1)},
    "SCORE_COLUMNS": {"cc": ("P3D_SCORE_CC", 1), "sim": ("P3D_SCORE_SIM", 2), "judd": ("P3D_SCORE_JUDD", 4), "kl": ("P3D_SCORE_KL", 8),
                      "nss": ("P3D_SCORE_NSS", 16)},
    "SCORE_TIES": {"reference": ("P3D_SCORE_TIES_REFERENCE", 0), "expected": ("P3D_SCORE_TIES_EXPECTED", 1)},
    "TRAINSET_FORMATS": {"u8": ("P3D_TRAINSET_FRAMES_U8", 0), "f32": ("P3D_TRAINSET_FRAMES_F32", 1)},
    "TEMPORAL_KINDS": {"off": ("P3D_TEMPORAL_OFF", 0), "gauss": ("P3D_TEMPORAL_GAUSS", 1), "ema": ("P3D_TEMPORAL_EMA", 2)},
    "PRIOR_KINDS": {"fixations": ("P3D_PRIOR_FIXATIONS", 0), "bytes": ("P3D_PRIOR_BYTES", 1)},
    "PRIOR_MODES": {"off": ("P3D_PRIOR_OFF", 0), "mul": ("P3D_PRIOR_MUL", 1), "mix": ("P3D_PRIOR_MIX", 2)},
    "STRUCTURES": {"unet": ("P3D_STRUCTURE_UNET", 0), "concat": ("P3D_STRUCTURE_CONCAT", 1), "gn_p3d": ("P3D_STRUCTURE_GN_P3D", 2),
                   "unet++nonsa": ("P3D_STRUCTURE_UNETPP_NONSA", 3), "gn_p3d_decoder": ("P3D_STRUCTURE_GN_P3D_DECODER", 4),
                   "gn_p3d_concat": ("P3D_STRUCTURE_GN_P3D_CONCAT", 5), "unet++ds": ("P3D_STRUCTURE_UNETPP_DS", 6)},
}
SCALARS = {"P3D_COMM_ID_BYTES": 128, "P3D_LOSS_KLD_CC": 3, "P3D_LOSS_SALIENCY": 4, "P3D_BLUR_MAX_RADIUS": 255, "P3D_HIST_MAX_BINS": 1024,
           "P3D_TRAINSET_FIXATIONS": 1, "P3D_TEMPORAL_MAX_RADIUS": 24, "P3D_PRIOR_MAX_MAPS": 16000000}


def test_every_python_side_constant_is_the_headers():
    from sap3d_tensorflow_amd import session
    K = _lib._H.constants
    for table, names in NAMES.items():
        have = session.STRUCTURES if table == "STRUCTURES" else getattr(_lib, table)
        assert list(have) == list(names), table                      # the keys, in their order (a row of scores follows it)
        for key, (hname, value) in names.items():
            assert hname in K, hname
            assert have[key] == K[hname] == value, (table, key)
    for name, value in SCALARS.items():
        assert getattr(_lib, name) == K[name] == value, name
