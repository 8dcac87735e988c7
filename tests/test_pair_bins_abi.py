"""fsmc_decode_pair_bins and its slice setter / getter at the drop-in boundary, without a GPU: the header declares
them, capi.SYMBOLS lists them, the built library exports them, and the ctypes signatures are the header's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_bins", "fsmc_ctx_set_pair_bins_slice", "fsmc_ctx_last_pair_bins_slices"]


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
    proto = re.search(r"int\s+fsmc_decode_pair_bins\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "const float* exp_coal_times", "const int32_t* bin_edges",
                    "size_t n_bins", "float* bin_mean", "float* bin_min_mean", "int32_t* bin_argmin_mean",
                    "int32_t* bin_min_map", "int32_t* bin_argmin_map"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_bins_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)", _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_bins_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_bins.argtypes == [vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
    assert lib.fsmc_ctx_set_pair_bins_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_bins_slices.argtypes == [vp, C.POINTER(C.c_int32)]
    for name in NAMES:
        assert getattr(lib, name).restype == C.c_int  # (the FSMC_* code)


def test_python_surface():
    for name in ("decode_pair_bins", "set_pair_bins_slice", "last_pair_bins_slices"):
        assert callable(getattr(capi.Context, name)), name
    sig = inspect.signature(capi.Context.decode_pair_bins)
    assert list(sig.parameters)[1:] == ["model", "exp_coal_times", "bin_edges", "want_mean", "want_min_mean",
                                        "want_min_map", "out"]
    assert [sig.parameters[k].default for k in ("want_mean", "want_min_mean", "want_min_map", "out")] == [True, True, True,
                                                                                                          None]


def test_product_surface():
    """ASMC.decodePairs takes site_bins on both overloads, the return structure has the bin fields, HMM.setSiteBins
    exists."""
    import __graft_entry__ as g

    g.build()
    from fastsmc_amd import api

    doc = api.ASMC.decodePairs.__doc__
    assert doc.count("site_bins") >= 2, doc
    for name in ("bin_edges", "bin_mean_posterior_means", "bin_min_posterior_means", "bin_argmin_posterior_means",
                 "bin_min_MAPs", "bin_argmin_MAPs"):
        assert isinstance(getattr(api.DecodePairsReturnStruct, name), property), name
    assert callable(api.HMM.setSiteBins)


def test_site_bins_helper():
    from fastsmc_amd import api

    # sites at 0, 0.4, 0.9, 1.0, 1.7, 3.2, 3.3 cM, windows of 1 cM: [0, 1) [1, 2) [2, 3) is empty [3, 4)
    edges = api.site_bins([0.0, 0.4, 0.9, 1.0, 1.7, 3.2, 3.3], 1.0)
    assert edges.dtype == np.int32 and edges.tolist() == [0, 3, 5, 7]
    # windows count from the first position, whatever it is; one window holds everything when it is wide enough
    assert api.site_bins([10.0, 10.5, 11.0], 100.0).tolist() == [0, 3]
    assert api.site_bins([10.0, 10.5, 11.0], 0.5).tolist() == [0, 1, 2, 3]
    assert api.site_bins([7.0], 1.0).tolist() == [0, 1]
    assert api.site_bins([2.0, 2.0, 2.0, 5.0], 1.0).tolist() == [0, 3, 4]  # (equal positions share a window)
    bp = np.cumsum(np.random.default_rng(0).integers(1, 5000, 1000))
    e = api.site_bins(bp, 100000)
    assert e[0] == 0 and e[-1] == 1000 and (np.diff(e) > 0).all()
    w = (bp - bp[0]) // 100000
    assert np.array_equal(e[1:-1], np.nonzero(np.diff(w))[0] + 1)  # (a new bin where the window changes)
    for bad in (lambda: api.site_bins([], 1.0), lambda: api.site_bins([1.0, 0.5], 1.0), lambda: api.site_bins([1.0], 0.0)):
        with pytest.raises(ValueError):
            bad()
