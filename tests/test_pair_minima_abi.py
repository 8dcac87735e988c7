"""fsmc_decode_pair_minima and its slice setter / getter at the drop-in boundary, without a GPU: the header declares
them, capi.SYMBOLS lists them, the built library exports them, and the ctypes signatures are the header's."""
import ctypes as C
import os
import re

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_minima", "fsmc_ctx_set_pair_minima_slice", "fsmc_ctx_last_pair_minima_slices"]


def _header():
    text = open(os.path.join(ROOT, "include", "fastsmc_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_binding_and_library_agree():
    import __graft_entry__ as g

    g.build()
    header = _header()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name


def test_header_prototype():
    proto = re.search(r"int\s+fsmc_decode_pair_minima\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "const float* exp_coal_times", "uint64_t pair_base",
                    "float* min_mean", "int32_t* argmin_mean", "int32_t* min_map", "int32_t* argmin_map"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_minima_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)", _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_minima_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_minima.argtypes == [vp, vp, vp, C.c_uint64, vp, vp, vp, vp]
    assert lib.fsmc_ctx_set_pair_minima_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_minima_slices.argtypes == [vp, C.POINTER(C.c_int32)]
    for name in NAMES:
        assert getattr(lib, name).restype == C.c_int  # (the FSMC_* code)


def test_python_surface():
    for name in ("decode_pair_minima", "set_pair_minima_slice", "last_pair_minima_slices"):
        assert callable(getattr(capi.Context, name)), name
    import inspect

    sig = inspect.signature(capi.Context.decode_pair_minima)
    assert list(sig.parameters)[1:] == ["model", "exp_coal_times", "pair_base", "want_mean", "want_map", "state"]
    assert [sig.parameters[k].default for k in ("pair_base", "want_mean", "want_map", "state")] == [0, True, True, None]
