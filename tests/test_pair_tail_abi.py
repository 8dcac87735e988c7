"""fsmc_decode_pair_tail_summaries and its slice setter / getter at the drop-in boundary, without a GPU: the header
declares them, capi.SYMBOLS lists them, the built library exports them, the ctypes signatures are the header's, and the
product surface (ASMC.decodePairs keywords, return-structure fields, HMM.setTailSummaries, api.site_widths) is there,
off by default and empty when off."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_tail_summaries", "fsmc_ctx_set_pair_tail_slice", "fsmc_ctx_last_pair_tail_slices"]


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
    proto = re.search(r"int\s+fsmc_decode_pair_tail_summaries\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "const int32_t* tail_states", "size_t n_tail",
                    "double* tail_sum", "const int32_t* bin_edges", "size_t n_bins", "float* bin_tail_mean",
                    "const float* site_weights", "float* bin_tail_length"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_tail_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)", _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_tail_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_tail_summaries.argtypes == [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, vp, vp]
    assert lib.fsmc_ctx_set_pair_tail_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_tail_slices.argtypes == [vp, C.POINTER(C.c_int32)]
    for name in NAMES:
        assert getattr(lib, name).restype == C.c_int  # (the FSMC_* code)


def test_python_surface():
    for name in ("decode_pair_tail_summaries", "set_pair_tail_slice", "last_pair_tail_slices"):
        assert callable(getattr(capi.Context, name)), name
    sig = inspect.signature(capi.Context.decode_pair_tail_summaries)
    assert list(sig.parameters)[1:] == ["model", "tail_states", "bin_edges", "site_weights", "want_sum", "want_bin_mean",
                                        "want_bin_length", "out"]
    assert [sig.parameters[k].default for k in ("bin_edges", "site_weights", "want_sum", "out")] == [None, None, True,
                                                                                                     None]


def test_product_surface():
    """ASMC.decodePairs takes tail_summary_times and site_weights as the last keywords of both overloads, both off by
    default; the return structure has the new fields, empty in a structure nothing was decoded into; HMM.setTailSummaries
    and api.site_widths exist."""
    import __graft_entry__ as g

    g.build()
    from fastsmc_amd import api

    doc = api.ASMC.decodePairs.__doc__
    signatures = [line for line in doc.splitlines() if re.match(r"\s*\d+\. decodePairs\(", line)]
    assert len(signatures) == 2, doc
    for line in signatures:
        assert line.index("tail_times") < line.index("quantiles") < line.index("tail_summary_times") < line.index(
            "site_weights"), line  # (trailing keywords)
        assert re.search(r"tail_summary_times: [^,]+ = \[\], site_weights: [^,]+ = \[\]\) -> None", line), line
        # (both off by default, and the last two)
    fields = ("tail_summary_times", "tail_summary_states", "site_weights", "sum_of_tail_probabilities",
              "per_pair_bin_tail_means", "per_pair_bin_tail_lengths")
    for name in fields:
        assert isinstance(getattr(api.DecodePairsReturnStruct, name), property), name
    assert callable(api.HMM.setTailSummaries)
    assert callable(api.site_widths) and "site_widths" in api.__all__


def test_fields_are_empty_when_off():
    import __graft_entry__ as g

    g.build()
    from fastsmc_amd import api

    r = api.DecodePairsReturnStruct()
    sizes = [np.asarray(getattr(r, name)).size
             for name in ("tail_summary_times", "tail_summary_states", "site_weights", "sum_of_tail_probabilities",
                          "per_pair_bin_tail_means", "per_pair_bin_tail_lengths")]
    assert sizes == [0] * 6
    assert np.asarray(r.sum_of_tail_probabilities).dtype == np.float64
    assert np.asarray(r.per_pair_bin_tail_means).dtype == np.float32
