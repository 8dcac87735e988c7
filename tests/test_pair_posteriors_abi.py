"""CPU-side checks of fsmc_decode_pair_posteriors at the drop-in boundary: the header declares the entry point and its
slice setter / getter, the ctypes binding lists them, the built library exports them -- and there is still no CPU
fallback behind any of it."""
import os
import re

import pytest

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["fsmc_decode_pair_posteriors", "fsmc_ctx_set_pair_posterior_slice",
               "fsmc_ctx_last_pair_posterior_slices"]


def _header():
    text = open(os.path.join(ROOT, "include", "fastsmc_hip.h")).read()
    top = text[:text.index("#ifndef FASTSMC_HIP_H")]
    return top, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_entry_point_and_the_slice_knob():
    top, code = _header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    # the argument list of the contract: context, model, coalescence times, the rows' pointers, the in/out sum
    m = re.search(r"int\s+fsmc_decode_pair_posteriors\s*\(([^)]*)\)", code)
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 5
    assert args[2].startswith("const float*") and args[3].startswith("float* const*") and args[4].startswith("float*")
    # the comment block at the top names the reference call it stands in for
    assert "fsmc_decode_pair_posteriors" in top and "writePerPairOutput" in top


def test_binding_lists_the_symbols():
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS
    for method in ("decode_pair_posteriors", "set_pair_posterior_slice", "last_pair_posterior_slices"):
        assert callable(getattr(capi.Context, method))


def test_library_exports_the_symbols():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.fsmc_decode_pair_posteriors.argtypes is not None and len(lib.fsmc_decode_pair_posteriors.argtypes) == 5
    # a null context is refused, not dereferenced
    assert lib.fsmc_decode_pair_posteriors(None, None, None, None, None) == -1  # FSMC_EINVAL
    assert lib.fsmc_ctx_set_pair_posterior_slice(None, 1) == -1
    assert lib.fsmc_ctx_last_pair_posterior_slices(None, None) == -1


def test_still_no_cpu_fallback_without_a_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.FsmcError) as ei:
        capi.Context(0)
    assert ei.value.code == -2  # FSMC_ENODEVICE
    assert "no CPU fallback" in str(ei.value)
