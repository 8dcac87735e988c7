"""fsmc_decode_pair_cdf and its slice setter / getter at the drop-in boundary, without a GPU: the header declares them,
capi.SYMBOLS lists them, the built library exports them, the ctypes signatures are the header's, and the product surface
(ASMC.decodePairs keywords, return-structure fields, HMM.setPosteriorCdf, api.tail_states) is there."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_cdf", "fsmc_ctx_set_pair_cdf_slice", "fsmc_ctx_last_pair_cdf_slices"]


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
    proto = re.search(r"int\s+fsmc_decode_pair_cdf\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "const int32_t* tail_states", "size_t n_tail",
                    "float* const* tail_rows", "const float* quantiles", "size_t n_quantiles",
                    "int32_t* const* quantile_rows"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_cdf_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)", _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_cdf_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_cdf.argtypes == [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp]
    assert lib.fsmc_ctx_set_pair_cdf_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_cdf_slices.argtypes == [vp, C.POINTER(C.c_int32)]
    for name in NAMES:
        assert getattr(lib, name).restype == C.c_int  # (the FSMC_* code)


def test_python_surface():
    for name in ("decode_pair_cdf", "set_pair_cdf_slice", "last_pair_cdf_slices"):
        assert callable(getattr(capi.Context, name)), name
    sig = inspect.signature(capi.Context.decode_pair_cdf)
    assert list(sig.parameters)[1:] == ["model", "tail_states", "quantiles", "out"]
    assert [sig.parameters[k].default for k in ("tail_states", "quantiles", "out")] == [(), (), None]


def test_product_surface():
    """ASMC.decodePairs takes tail_times and quantiles on both overloads, the return structure has the five fields,
    HMM.setPosteriorCdf exists."""
    import __graft_entry__ as g

    g.build()
    from fastsmc_amd import api

    doc = api.ASMC.decodePairs.__doc__
    signatures = [line for line in doc.splitlines() if re.match(r"\s*\d+\. decodePairs\(", line)]
    assert len(signatures) == 2, doc
    for line in signatures:
        assert "tail_times" in line and "quantiles" in line, line
        assert line.index("site_bins") < line.index("tail_times") < line.index("quantiles"), line  # (trailing keywords)
    for name in ("tail_times", "tail_states", "quantiles", "per_pair_tail_probabilities", "per_pair_quantile_states"):
        assert isinstance(getattr(api.DecodePairsReturnStruct, name), property), name
    assert callable(api.HMM.setPosteriorCdf)


def test_tail_states_helper():
    from fastsmc_amd import api

    # four states that start at 0, 30, 100, 2000 generations; the last value ends the last interval
    disc = [0.0, 30.0, 100.0, 2000.0, np.inf]
    cuts = api.tail_states(disc, [30.0, 50.0, 5000.0])
    assert cuts.dtype == np.int32
    # a time equal to a start: that state is not below it; between two starts; beyond the last start: every state
    assert cuts.tolist() == [1, 2, 4]
    assert api.tail_states(disc, [100.0, 100.5]).tolist() == [2, 3]
    assert api.tail_states(disc, 1e-3).tolist() == [1]
    # the end of the last interval is no state's start, finite or not
    assert api.tail_states([0.0, 30.0, 100.0, 2000.0, 3000.0], [1e9]).tolist() == [4]
    # the compare is in float32, as the library's
    t = np.nextafter(np.float32(30.0), np.float32(31.0))
    assert api.tail_states(disc, [float(t)]).tolist() == [2]
    assert api.tail_states(disc, [30.0 + 1e-9]).tolist() == [1]  # (rounds to 30.0f)
    for bad in ([0.0], [-5.0], [50.0, 0.0]):
        with pytest.raises(ValueError, match="no interval"):
            api.tail_states(disc, bad)
    with pytest.raises(ValueError):
        api.tail_states([0.0], [5.0])
