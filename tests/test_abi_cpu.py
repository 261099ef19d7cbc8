"""C-ABI checks that need no GPU: the shared library loads and exports every symbol that
include/handmv.h declares; argument validation that happens before any HIP call."""
import ctypes
import os
import re

from handmvnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    declared = sorted(set(re.findall(r"\b(hmv_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no declarations found"
    lib = _lib.load()
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} is declared in include/handmv.h but not exported"
    assert set(declared) == set(_lib.SYMBOLS)
    assert b"gfx950" in lib.hmv_version()


def test_range_error_code():
    """HMV_ERR_RANGE (a value outside the fp16 range of its mode, include/handmv.h "Range contract") is 7 in the header and the binding."""
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    m = re.search(r"\bHMV_ERR_RANGE\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == 7
    assert _lib.HMV_ERR_RANGE == 7


def test_product_library_reads_one_environment_variable():
    """Development knobs (A/B switches, probes) exist only in a -DHMV_DEV_KNOBS build: a stray HMV_* variable on a user's box must
    not be able to change kernels, K orders or numerics.  Every "HMV_[A-Z0-9_]+" token in the product library's bytes is either the
    one variable it reads (HMV_GRAPHS) or an enum name quoted in an error message / an assertion text."""
    if os.environ.get("HMV_LIB"):
        return   # an A/B run against another build (possibly the -dev one): nothing to assert about that file
    data = open(_lib.LIB_PATH, "rb").read()
    tokens = set(m.decode() for m in re.findall(rb"HMV_[A-Z0-9_]+[a-z0-9]*", data))
    allowed = {"HMV_GRAPHS", "HMV_F32", "HMV_F16", "HMV_F32X3", "HMV_POS_SIN"}
    assert tokens <= allowed, sorted(tokens - allowed)
    assert "HMV_GRAPHS" in tokens
    # and the sources spell every other knob through the gated macro
    for f in os.listdir(os.path.join(ROOT, "handmvnet_amd", "csrc")):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(ROOT, "handmvnet_amd", "csrc", f)).read()
            for m in re.finditer(r"(?<![A-Za-z_])getenv\(\s*\"(\w+)\"", text):
                assert m.group(1) == "HMV_GRAPHS", (f, m.group(1))
    assert b"f32x3" in _lib.load().hmv_version() and b"f16" in _lib.load().hmv_version()


def test_config_struct_matches_header_and_is_validated():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.HmvConfig) == 18 * 4          # incl. the fusion kind added for cross_attn_learnable_query
    h = ctypes.c_void_p()
    c = _lib.HmvConfig()
    c.struct_size = 12                      # wrong ABI size is rejected before anything touches HIP
    assert lib.hmv_create(ctypes.byref(c), ctypes.byref(h)) == 1
    assert b"struct_size" in lib.hmv_last_error(None)
    c.struct_size = ctypes.sizeof(_lib.HmvConfig)
    c.backbone = 7
    assert lib.hmv_create(ctypes.byref(c), ctypes.byref(h)) == 1
    assert b"18, 34, 50_paper" in lib.hmv_last_error(None)
    c.backbone, c.num_views, c.fusion_layers = 2, 8, 4
    assert lib.hmv_create(ctypes.byref(c), ctypes.byref(h)) == 1
    assert b"odd" in lib.hmv_last_error(None)


def test_conv_form_struct_matches_header_and_is_validated():
    """hmv_conv_form_args: 34 int32 fields, 11 pointers and the kernel name out; a NULL args or another struct_size is refused before any HIP call."""
    lib = _lib.load()
    assert ctypes.sizeof(_lib.HmvConvFormArgs) == 34 * 4 + 12 * ctypes.sizeof(ctypes.c_void_p)
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    body = re.search(r"typedef struct hmv_conv_form_args \{(.*?)\} hmv_conv_form_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(None, 2 if decl.strip().startswith("const") else 1)[-1].split(",")]
    assert names == [("in" if n == "in_" else n) for n, _ in _lib.HmvConvFormArgs._fields_], names
    a = _lib.HmvConvFormArgs()
    a.struct_size = 12
    assert lib.hmv_op_conv2d_form(0, ctypes.byref(a), None) == 1 and b"hmv_op_conv2d_form: struct_size" in lib.hmv_last_error(None)
    assert lib.hmv_op_conv2d_form(0, None, None) == 1 and b"hmv_op_conv2d_form" in lib.hmv_last_error(None)
    for k, v in (("HMV_FORM_DUAL", 1), ("HMV_FORM_CHAIN", 2), ("HMV_FORM_POOL", 4), ("HMV_FORM_PHASES", 8), ("HMV_FORM_SPLITK", 16), ("HMV_FORM_PAIR_OUT", 32)):
        assert getattr(_lib, k) == v and re.search(rf"\b{k} = {v}\b", header), k


def test_product_package_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under handmvnet_amd/ may import or load it."""
    pkg = os.path.join(ROOT, "handmvnet_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "liboracle" not in text and "hmvo_" not in text, f
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, re.M), f
