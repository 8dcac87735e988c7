"""fsmc_decode_pair_samples and its slice setter / getter at the drop-in boundary, without a GPU: the header declares
them, capi.SYMBOLS lists them, the built library exports them, the ctypes signatures are the header's, the wrapper checks
its arguments before it calls, and the product surface (ASMC.samplePairs, DecodePairsReturnStruct, HMM) has the request
and its field."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from fastsmc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fsmc_decode_pair_samples", "fsmc_ctx_set_pair_samples_slice", "fsmc_ctx_last_pair_samples_slices"]

# the lines of the contract, as the header and the kernel's header both state them
CONTRACT = ("Philox4x32-10, key = (seed & 0xffffffff, seed >> 32)", "counter = (t >> 2, r, hap_a, hap_b)",
            "u = float(out[t & 3] >> 8) * 2^-24", "c[-1] = 0.f;  c[i] = c[i-1] + w[i]", "x = u * c[K-1]",
            "state = min(K-1, #{ i in [0, K) : c[i] <= x })", "x[S-1] = pick(w, u(S-1))", "i > j:   w[i] = B[j] * delta_t[i]",
            "i = j:   w[j] = D[j] * delta_t[j]", "g = 1.f at i = j-1;   for i = j-2 .. 0:  g = g * cR[i+1]",
            "w[i] = (U[i] * delta_t[i]) * g", "x[t] = pick(w, u(t))")


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
    proto = re.search(r"int\s+fsmc_decode_pair_samples\s*\(([^)]*)\)", _header()).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["fsmc_ctx* ctx", "const fsmc_model* m", "int32_t n_samples", "uint64_t seed", "uint8_t* states"]
    assert re.search(r"int\s+fsmc_ctx_set_pair_samples_slice\s*\(\s*fsmc_ctx\*\s*ctx,\s*uint32_t\s+groups\s*\)", _header())
    assert re.search(r"int\s+fsmc_ctx_last_pair_samples_slices\s*\(\s*const\s+fsmc_ctx\*\s*ctx,\s*int32_t\*\s*slices\s*\)",
                     _header())
    text = _squeezed(_header(strip=False))
    kernel = _squeezed(open(os.path.join(ROOT, "fastsmc_amd", "csrc", "fsmc_pair_samples.h")).read())
    for needle in CONTRACT:
        assert _squeezed(needle) in text, needle
        assert _squeezed(needle) in kernel, needle
    for needle in ("states[(i * n_samples + r) * S + t]", "never chosen", "more than 128 states", "sequence-mode",
                   "n_samples outside 1 ... 64", "different streams", "only has states in [0, K)"):
        assert needle in text, needle
    # the kernel's header says why ghost states are never chosen and which K clamps
    for needle in ("Ghost states", "never chosen", "The clamp uses the model's K, not KT"):
        assert needle in kernel, needle


def test_ctypes_signatures():
    import __graft_entry__ as g

    g.build()
    lib = capi.load()
    vp = C.c_void_p
    assert lib.fsmc_decode_pair_samples.argtypes == [vp, vp, C.c_int32, C.c_uint64, vp]
    assert lib.fsmc_ctx_set_pair_samples_slice.argtypes == [vp, C.c_uint32]
    assert lib.fsmc_ctx_last_pair_samples_slices.argtypes == [vp, C.POINTER(C.c_int32)]
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
    for name in ("decode_pair_samples", "set_pair_samples_slice", "last_pair_samples_slices"):
        assert callable(getattr(capi.Context, name)), name
    sig = inspect.signature(capi.Context.decode_pair_samples)
    assert list(sig.parameters)[1:] == ["model", "n_samples", "seed", "out"]
    assert [sig.parameters[k].default for k in ("seed", "out")] == [0, None]
    ctx = _bare_context(3)
    bad = [
        np.zeros((3, 2, 10), np.int32),          # another type
        np.zeros((3, 2, 9), np.uint8),           # rows of another length
        np.zeros((3, 3, 10), np.uint8),          # another number of samples
        np.zeros((2, 2, 10), np.uint8),          # too few pairs
        np.zeros((3, 2, 20), np.uint8)[:, :, ::2],  # not contiguous
        np.zeros((6, 10), np.uint8),             # two dimensions
        [[0] * 10] * 6,                          # not an array
    ]
    for out in bad:
        with pytest.raises(ValueError):
            ctx.decode_pair_samples(_Model, 2, out=out)
    frozen = np.zeros((3, 2, 10), np.uint8)
    frozen.setflags(write=False)
    with pytest.raises(ValueError):
        ctx.decode_pair_samples(_Model, 2, out=frozen)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError):
            ctx.decode_pair_samples(_Model, 2, seed=seed)
    with pytest.raises(ValueError):
        ctx.decode_pair_samples(_Model, 1 << 31)
    for n, seed in ((2.5, 0), ("2", 0), (2, 0.5)):
        with pytest.raises(TypeError):
            ctx.decode_pair_samples(_Model, n, seed=seed)
    # what passes the wrapper reaches the library
    with pytest.raises(AssertionError, match="fsmc_decode_pair_samples was called"):
        ctx.decode_pair_samples(_Model, 2, seed=(1 << 64) - 1, out=np.zeros((4, 2, 10), np.uint8))


def test_product_surface():
    """ASMC.samplePairs exists on both overloads with samples = 1 and seed = 0; decodePairs keeps its signature; the
    return structure has the field (empty, uint8, three dimensions in a fresh structure); HMM.setSampledPaths exists; the
    asmc package hands out the same classes."""
    import __graft_entry__ as g

    g.build()
    import asmc
    from fastsmc_amd import api

    doc = api.ASMC.samplePairs.__doc__
    assert doc.count("samples: typing.SupportsInt") + doc.count("samples: int") == 2, doc
    assert len(re.findall(r"samples: [^,]* = 1, seed: [^,)]* = 0\)", doc)) == 2, doc
    assert "hap_indices_a" in doc and "hap_ids_a" in doc
    assert "samples" not in api.ASMC.decodePairs.__doc__.split("Decode the listed pairs")[0]
    assert isinstance(api.DecodePairsReturnStruct.per_pair_sampled_states, property)
    got = np.array(api.DecodePairsReturnStruct().per_pair_sampled_states)
    assert got.size == 0 and got.dtype == np.uint8 and got.ndim == 3
    assert callable(api.HMM.setSampledPaths)
    assert "samples" in api.HMM.setSampledPaths.__doc__ and "seed" in api.HMM.setSampledPaths.__doc__
    assert asmc.ASMC is api.ASMC and asmc.DecodePairsReturnStruct is api.DecodePairsReturnStruct
    assert callable(asmc.ASMC.samplePairs)
