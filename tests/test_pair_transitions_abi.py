"""fsmc_decode_pair_transitions and its slice setter / getter at the drop-in boundary, without a GPU: the header declares
them, capi.SYMBOLS lists them, the built library exports them, the ctypes signatures are the header's, the wrapper checks
its arguments before it calls, and the product surface (ASMC.decodePairTransitions, DecodePairsReturnStruct, HMM) has the
request and its fields."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_transitions", "fsmc_ctx_set_pair_transitions_slice", "fsmc_ctx_last_pair_transitions_slices"]

# the lines of the contract, as the header and the kernel's header both state them
CONTRACT = ("vec[k] = b_t[k] * e[k]", "BU[K-1] = 0.f;  BU[k] = U[k] * vec[k+1] + RR[k] * BU[k+1]",
            "BL[0]   = 0.f;  BL[k] = BL[k-1] + B[k-1] * vec[k-1]", "down = up = stay = 0.f;",
            "for k ascending over the model's K states:", "down = down + delta_{t-1}[k] * BL[k]",
            "stay = stay + delta_{t-1}[k] * (D[k] * vec[k])", "up   = up   + delta_{t-1}[k] * BU[k]",
            "z = (down + stay) + up;   r = 1.0f / z", "p_down[t] = down * r;     p_up[t] = up * r",
            "p_down[0] = p_up[0] = 0.f", "(BL + D * vec) + BU", "b_{S-1}[k] = 1.f * (1.0f / sum)",
            "one separately rounded IEEE fp32 operation")


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "fastsmc_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


def _squeezed(text):
    """Without comment leaders and runs of blanks: a contract line reads the same in a C comment and a C++ one."""
    return re.sub(r"\s+", " ", re.sub(r"^\s*(\*|//)", "", text, flags=re.M))


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
    proto = re.search(r"int\s+fsmc_decode_pair_transitions\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "float* down_rows", "float* up_rows",
                    "const int32_t* bin_edges", "int32_t n_bins", "float* bin_down", "float* bin_up"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_transitions_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)",
                     _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_transitions_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())
    text = _squeezed(_header(strip=False))
    kernel = _squeezed(open(os.path.join(ROOT, "fastsmc_amd", "csrc", "fsmc_pair_transitions.h")).read())
    for needle in CONTRACT:
        assert _squeezed(needle) in text, needle
        assert _squeezed(needle) in kernel, needle
    for needle in ("down_rows[i * S + t]", "bin_down[i * n_bins + b]", "more than 128 states", "sequence-mode",
                   "No weights, no divide", "never leave the device", "FSMC_ENOMEM", "whatever IEEE gives (NaN)"):
        assert needle in text, needle
    # both say what ghost states do and which K scales b first
    for where in (text, kernel):
        assert "Ghost states" in where and "+0.f products" in where and "change nothing" in where
        assert "uses the model's K" in where


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_transitions.argtypes == [vp, vp, vp, vp, vp, C.c_int32, vp, vp]
    assert lib.fsmc_ctx_set_pair_transitions_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_transitions_slices.argtypes == [vp, C.POINTER(C.c_int32)]
    for name in NAMES:
        assert getattr(lib, name).restype == C.c_int  # (the FSMC_* code)


class _NoLibrary:
    """A library whose entry point must not be reached: the wrapper refuses the arguments first."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def _bare_context(n_pairs):
    ctx = capi.Context.__new__(capi.Context)
    ctx._L, ctx._h, ctx._n_pairs = _NoLibrary(), None, n_pairs
    return ctx


class _Model:
    S, K, _h = 10, 4, None


def test_wrapper_argument_checks():
    for name in ("decode_pair_transitions", "set_pair_transitions_slice", "last_pair_transitions_slices"):
        assert callable(getattr(capi.Context, name)), name
    sig = inspect.signature(capi.Context.decode_pair_transitions)
    assert list(sig.parameters)[1:] == ["model", "bin_edges", "want_rows", "out"]
    assert [sig.parameters[k].default for k in ("bin_edges", "want_rows", "out")] == [None, True, None]
    ctx = _bare_context(3)
    rows, cells = np.zeros((3, 10), np.float32), np.zeros((3, 2), np.float32)
    frozen = np.zeros((3, 10), np.float32)
    frozen.setflags(write=False)
    bad = [
        (np.zeros((3, 10), np.float64), None, None, None),      # another type
        (np.zeros((3, 9), np.float32), None, None, None),       # rows of another length
        (np.zeros((2, 10), np.float32), None, None, None),      # too few pairs
        (np.zeros((3, 20), np.float32)[:, ::2], None, None, None),  # not contiguous
        (np.zeros(30, np.float32), None, None, None),           # one dimension
        ([[0.0] * 10] * 3, None, None, None),                   # not an array
        (frozen, None, None, None),                             # read-only
        (rows, rows, cells, None),                              # bin outputs without edges
        (None, None, None, None),                               # nothing at all
        (rows, rows, None),                                     # three outputs
    ]
    for out in bad:
        with pytest.raises(ValueError):
            ctx.decode_pair_transitions(_Model, out=out)
    with pytest.raises(ValueError):
        ctx.decode_pair_transitions(_Model, bin_edges=[0, 5, 10], out=(rows, rows, np.zeros((3, 3), np.float32), None))
    with pytest.raises(ValueError):
        ctx.decode_pair_transitions(_Model, want_rows=False)  # nothing asked for
    # what passes the wrapper reaches the library
    with pytest.raises(AssertionError, match="fsmc_decode_pair_transitions was called"):
        ctx.decode_pair_transitions(_Model, bin_edges=[0, 5, 10], out=(np.zeros((4, 10), np.float32), None, cells, cells))
    with pytest.raises(AssertionError, match="fsmc_decode_pair_transitions was called"):
        ctx.decode_pair_transitions(_Model, bin_edges=[0, 10], want_rows=False)


def test_product_surface():
    """ASMC.decodePairTransitions exists on both overloads with rows = True and site_bins = None; decodePairs keeps its
    signature and its text; the return structure has the four fields (empty, float32, two dimensions in a fresh
    structure); HMM.setTransitionProbabilities exists; the asmc package hands out the same classes."""
    import __graft_entry__ as g

    g.build()
    import asmc
    from fastsmc_amd import api

    doc = api.ASMC.decodePairTransitions.__doc__
    assert len(re.findall(r"rows: bool = True, site_bins: [^)]* = None\)", doc)) == 2, doc
    assert "hap_indices_a" in doc and "hap_ids_a" in doc
    signatures = api.ASMC.decodePairs.__doc__.split("Decode the listed pairs")[0]
    assert "rows" not in signatures and "transition" not in api.ASMC.decodePairs.__doc__
    assert api.ASMC.decodePairs.__doc__.count("viterbi_paths: bool = False, site_bins:") == 2
    for field in ("per_pair_down_probabilities", "per_pair_up_probabilities", "bin_expected_downs", "bin_expected_ups"):
        assert isinstance(getattr(api.DecodePairsReturnStruct, field), property), field
        got = np.array(getattr(api.DecodePairsReturnStruct(), field))
        assert got.size == 0 and got.dtype == np.float32 and got.ndim == 2, field
    assert np.array(api.DecodePairsReturnStruct().bin_edges).size == 0
    assert callable(api.HMM.setTransitionProbabilities)
    assert "rows" in api.HMM.setTransitionProbabilities.__doc__ and "bins" in api.HMM.setTransitionProbabilities.__doc__
    assert asmc.ASMC is api.ASMC and asmc.DecodePairsReturnStruct is api.DecodePairsReturnStruct
    assert callable(asmc.ASMC.decodePairTransitions)
