"""Context.set_pair_<kind>_slice / last_pair_<kind>_slices of the nine sliced per-pair entry points, without a GPU or a
built library: each calls exactly its fsmc_ctx_* symbol with the context's handle, returns what the library stores, turns a
status code into FsmcError, says in its docstring whose setting it is -- and the kinds are capi.SYMBOLS' own."""
import re

import pytest

from fastsmc_amd import capi

# kind -> the entry point the setting belongs to (`posterior` is singular in the C and the Python names)
KINDS = {
    "posterior": "fsmc_decode_pair_posteriors", "minima": "fsmc_decode_pair_minima", "bins": "fsmc_decode_pair_bins",
    "cdf": "fsmc_decode_pair_cdf", "tail": "fsmc_decode_pair_tail_summaries", "loglik": "fsmc_decode_pair_loglik",
    "viterbi": "fsmc_decode_pair_viterbi", "samples": "fsmc_decode_pair_samples",
    "transitions": "fsmc_decode_pair_transitions",
}
HANDLE = object()


class _Recorder:
    """A library that records every call; a getter's int32 receives `stored`, every call returns `rc`."""

    def __init__(self, stored=0, rc=0):
        self.calls, self.stored, self.rc = [], stored, rc

    def fsmc_last_error(self, handle):
        return b"refused by the fake"

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + args)
            if name.startswith("fsmc_ctx_last_"):
                args[1]._obj.value = self.stored  # (args[1] is ctypes.byref(int32))
            return self.rc
        return call


def _bare_context(lib):
    ctx = capi.Context.__new__(capi.Context)
    ctx._L, ctx._h, ctx._models = lib, HANDLE, []
    return ctx


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_setter_calls_its_symbol(kind):
    lib = _Recorder()
    ctx = _bare_context(lib)  # (kept alive: closing a context calls the library too)
    assert getattr(ctx, f"set_pair_{kind}_slice")(3) is None
    assert lib.calls == [(f"fsmc_ctx_set_pair_{kind}_slice", HANDLE, 3)]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_getter_returns_what_the_library_stores(kind):
    lib = _Recorder(stored=17)
    ctx = _bare_context(lib)
    assert getattr(ctx, f"last_pair_{kind}_slices")() == 17
    assert [c[:2] for c in lib.calls] == [(f"fsmc_ctx_last_pair_{kind}_slices", HANDLE)]
    assert len(lib.calls[0]) == 3


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_status_code_raises(kind):
    ctx = _bare_context(_Recorder(rc=-3))
    for call in (lambda: getattr(ctx, f"set_pair_{kind}_slice")(3), getattr(ctx, f"last_pair_{kind}_slices")):
        with pytest.raises(capi.FsmcError) as ei:
            call()
        assert ei.value.code == -3
        assert "refused by the fake" in str(ei.value)


def test_kinds_are_the_slice_symbols():
    setters = {m.group(1) for m in (re.fullmatch(r"fsmc_ctx_set_pair_(\w+)_slice", s) for s in capi.SYMBOLS) if m}
    getters = {m.group(1) for m in (re.fullmatch(r"fsmc_ctx_last_pair_(\w+)_slices", s) for s in capi.SYMBOLS) if m}
    assert setters == getters == set(KINDS)
    assert len(capi.SYMBOLS) == len(set(capi.SYMBOLS))
    for entry in KINDS.values():
        assert entry in capi.SYMBOLS, entry


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_methods_are_attributes_with_docstrings(kind):
    for name in (f"set_pair_{kind}_slice", f"last_pair_{kind}_slices"):
        fn = vars(capi.Context)[name]  # (a real attribute of the class, not __getattr__)
        assert fn.__name__ == name
        assert re.search(r"\b" + KINDS[kind] + r"\b", fn.__doc__ or ""), name
