"""fsmc_decode_pair_viterbi and its slice setter / getter at the drop-in boundary, without a GPU: the header declares
them, capi.SYMBOLS lists them, the built library exports them, the ctypes signatures are the header's, the wrapper checks
its arguments before it calls, and the product surface (ASMC.decodePairs, DecodePairsReturnStruct, HMM, api.state_runs)
has the request and its fields."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_viterbi", "fsmc_ctx_set_pair_viterbi_slice", "fsmc_ctx_last_pair_viterbi_slices"]


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
    proto = re.search(r"int\s+fsmc_decode_pair_viterbi\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "uint8_t* states", "double* mant", "int32_t* expo"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_viterbi_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)", _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_viterbi_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())
    # the definition is part of the contract: the header states the recurrences, the comparisons and the limits
    text = _header(strip=False)
    for needle in ("if (p[k] >= mC[k+1])", "if (car >= cand) MU = car", "if (d > best)", "if (l > best)",
                   "x[t-1] = psi[t][x[t]]", "the smaller predecessor index", "never chosen", "more than 128 states",
                   "sequence-mode"):
        assert needle in text, needle
    # the kernel's header states the same contract and why ghost states are never chosen
    kernel = open(os.path.join(ROOT, "fastsmc_amd", "csrc", "fsmc_pair_viterbi.h")).read()
    for needle in ("if (p[k] >= mC[k+1])", "if (l > best)", "Ghost states", "never chosen"):
        assert needle in kernel, needle


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_viterbi.argtypes == [vp, vp, vp, vp, vp]
    assert lib.fsmc_ctx_set_pair_viterbi_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_viterbi_slices.argtypes == [vp, C.POINTER(C.c_int32)]
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
    for name in ("decode_pair_viterbi", "set_pair_viterbi_slice", "last_pair_viterbi_slices"):
        assert callable(getattr(capi.Context, name)), name
    sig = inspect.signature(capi.Context.decode_pair_viterbi)
    assert list(sig.parameters)[1:] == ["model", "want_states", "want_prob", "out"]
    assert [sig.parameters[k].default for k in ("want_states", "want_prob", "out")] == [True, True, None]
    ctx = _bare_context(3)
    good = (np.zeros((3, 10), np.uint8), np.zeros(3), np.zeros(3, np.int32))
    bad = [
        good[:2],                                                     # two arrays
        (np.zeros((3, 10), np.int32),) + good[1:],                    # states of another type
        (np.zeros((3, 9), np.uint8),) + good[1:],                     # rows of another length
        (np.zeros((2, 10), np.uint8),) + good[1:],                    # too few rows
        (np.zeros((3, 20), np.uint8)[:, ::2],) + good[1:],            # not contiguous
        (good[0], np.zeros(3, np.float32), good[2]),                  # float32 mantissas
        (good[0], good[1], np.zeros(3, np.int64)),                    # int64 exponents
        (good[0], np.zeros((3, 1)), good[2]),                         # a matrix of mantissas
    ]
    for out in bad:
        with pytest.raises(ValueError):
            ctx.decode_pair_viterbi(_Model, out=out)
    frozen = np.zeros((3, 10), np.uint8)
    frozen.setflags(write=False)
    with pytest.raises(ValueError):
        ctx.decode_pair_viterbi(_Model, out=(frozen,) + good[1:])
    # the logarithm is capi.log_likelihood's
    lp = capi.log_likelihood(np.array([0.5, 0.0]), np.array([-4, 3], np.int32))
    assert lp[0] == -5 * np.log(2.0) and lp[1] == -np.inf


def test_product_surface():
    """ASMC.decodePairs takes viterbi_paths on both overloads, directly behind log_likelihoods and in front of site_bins;
    the return structure has the four fields (empty in a fresh structure); HMM.setStoreViterbiPaths exists; the asmc
    package hands out the same classes."""
    import __graft_entry__ as g

    g.build()
    import asmc
    from fastsmc_amd import api

    doc = api.ASMC.decodePairs.__doc__
    assert doc.count("viterbi_paths: bool = False") == 2, doc
    assert len(re.findall(r"log_likelihoods: bool = False, viterbi_paths: bool = False, site_bins:", doc)) == 2, doc
    fields = {"per_pair_viterbi_states": np.uint8, "per_pair_viterbi_log_probabilities": np.float64,
              "per_pair_viterbi_mantissas": np.float64, "per_pair_viterbi_exponents": np.int32}
    empty = api.DecodePairsReturnStruct()
    for name, dtype in fields.items():
        assert isinstance(getattr(api.DecodePairsReturnStruct, name), property), name
        got = np.array(getattr(empty, name))
        assert got.size == 0 and got.dtype == dtype, name
    assert np.array(empty.per_pair_viterbi_states).ndim == 2
    assert callable(api.HMM.setStoreViterbiPaths)
    assert asmc.ASMC is api.ASMC and asmc.DecodePairsReturnStruct is api.DecodePairsReturnStruct
    assert "state_runs" in api.__all__


def test_state_runs():
    from fastsmc_amd import api

    starts, ends, states = api.state_runs(np.array([3, 3, 5, 5, 5, 2], np.uint8))
    assert starts.tolist() == [0, 2, 5] and ends.tolist() == [2, 5, 6] and states.tolist() == [3, 5, 2]
    assert states.dtype == np.uint8
    starts, ends, states = api.state_runs(np.array([7], np.uint8))
    assert starts.tolist() == [0] and ends.tolist() == [1] and states.tolist() == [7]
    starts, ends, states = api.state_runs(np.zeros(0, np.uint8))
    assert starts.size == ends.size == states.size == 0
    starts, ends, states = api.state_runs([1, 2, 1, 1])
    assert starts.tolist() == [0, 1, 2] and ends.tolist() == [1, 2, 4] and states.tolist() == [1, 2, 1]
    # the runs tile the row and neighbours differ, whatever the row
    rng = np.random.default_rng(3)
    row = rng.integers(0, 3, 500).astype(np.uint8)
    starts, ends, states = api.state_runs(row)
    assert starts[0] == 0 and ends[-1] == row.size and np.array_equal(starts[1:], ends[:-1])
    assert (states[1:] != states[:-1]).all() and np.array_equal(np.repeat(states, ends - starts), row)
