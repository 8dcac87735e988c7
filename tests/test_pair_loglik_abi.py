"""fsmc_decode_pair_loglik and its slice setter / getter at the drop-in boundary, without a GPU: the header declares
them, capi.SYMBOLS lists them, the built library exports them, the ctypes signatures are the header's, and the product
surface (ASMC.decodePairs, DecodePairsReturnStruct, HMM) has the request and its fields."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_loglik", "fsmc_ctx_set_pair_loglik_slice", "fsmc_ctx_last_pair_loglik_slices"]


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "fastsmc_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


def test_header_binding_and_library_agree():
    import __graft_entry__ as g

    g.build()
    header = _header()
    lib = capi.load()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name


def test_header_prototype_and_contract():
    proto = re.search(r"int\s+fsmc_decode_pair_loglik\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "const int32_t* bin_edges", "size_t n_bins", "double* mant",
                    "int32_t* expo", "double* bin_mant", "int32_t* bin_expo"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_loglik_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)", _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_loglik_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())
    # the definition is part of the contract: the header states the recurrence and names the reference's statements
    text = _header(strip=False)
    for needle in ("m = m * (double)sum[t]", "frexp(m, &de)", "HMM.cpp:725-784", "HMM.cpp:745 and 776-779"):
        assert needle in text, needle


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_loglik.argtypes == [vp, vp, vp, C.c_size_t, vp, vp, vp, vp]
    assert lib.fsmc_ctx_set_pair_loglik_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_loglik_slices.argtypes == [vp, C.POINTER(C.c_int32)]
    for name in NAMES:
        assert getattr(lib, name).restype == C.c_int  # (the FSMC_* code)


def test_python_surface():
    for name in ("decode_pair_loglik", "set_pair_loglik_slice", "last_pair_loglik_slices"):
        assert callable(getattr(capi.Context, name)), name
    sig = inspect.signature(capi.Context.decode_pair_loglik)
    assert list(sig.parameters)[1:] == ["model", "bin_edges", "want_total", "out"]
    assert [sig.parameters[k].default for k in ("bin_edges", "want_total", "out")] == [None, True, None]
    ll = capi.log_likelihood(np.array([0.5, 0.75, 0.0, np.nan]), np.array([1, -3, 7, 2], np.int32))
    assert ll.dtype == np.float64 and ll[0] == 0.0 and ll[1] == np.log(0.75) - 3 * np.log(2.0)
    assert ll[2] == -np.inf and np.isnan(ll[3])


def test_product_surface():
    """ASMC.decodePairs takes log_likelihoods on both overloads, the return structure has the fields (empty in a fresh
    structure), HMM.setStoreLogLikelihoods exists, and the asmc package hands out the same classes."""
    import __graft_entry__ as g

    g.build()
    import asmc
    from fastsmc_amd import api

    doc = api.ASMC.decodePairs.__doc__
    assert doc.count("log_likelihoods: bool = False") == 2, doc
    fields = ("per_pair_log_likelihoods", "per_pair_likelihood_mantissas", "per_pair_likelihood_exponents",
              "per_pair_bin_log_likelihoods", "per_pair_bin_likelihood_mantissas", "per_pair_bin_likelihood_exponents")
    for name in fields:
        assert isinstance(getattr(api.DecodePairsReturnStruct, name), property), name
    empty = api.DecodePairsReturnStruct()
    for name in fields:
        assert np.array(getattr(empty, name)).size == 0, name
    assert np.array(empty.per_pair_log_likelihoods).dtype == np.float64
    assert np.array(empty.per_pair_likelihood_exponents).dtype == np.int32
    assert callable(api.HMM.setStoreLogLikelihoods)
    assert asmc.ASMC is api.ASMC and asmc.DecodePairsReturnStruct is api.DecodePairsReturnStruct
