"""The identification kernels (fastsmc_amd/csrc/fsmc_identify.h) at their own edges: the inputs of
tests/identify_edges.py -- runs and run-outs at the 32-word chunk boundaries, chunks that alternate between the event
walk and the word-by-word walk, more reports of one tile than its LDS stage holds, a length exactly at min_m, the
deepest seed split, gaps up to INT_MAX -- against tests/test_hashing.py::restate_candidates, integer-exact and in
order; flush_word as a value; the same list from every arrival order of the atomic appends; the general kernel on the
default kernel's inputs; and the buffer protocol of fsmc_identify / fsmc_identify_fetch through the raw C ABI.
tests/test_identify_edges.py proves on the CPU that each input reaches the regime it is built for."""
import ctypes as C

import numpy as np
import pytest

import identify_edges as E
from fastsmc_amd import api, capi
from test_identify_edges import host_data, host_params

pytestmark = pytest.mark.gpu

FSMC_OK, FSMC_ESTATE, FSMC_EOVERFLOW = 0, -5, capi.FSMC_EOVERFLOW  # include/fastsmc_hip.h


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def device_inputs(c):
    words = np.ascontiguousarray(c.words[:c.n_device])
    return words, np.arange(c.n_device, dtype=np.uint32)


def as_list(rec):
    return [(int(r["hap_a"]), int(r["hap_b"]), int(r["from"]), int(r["to"])) for r in rec]


def check_order(rec, n):
    """Keys (flush_word, hap_a * n + hap_b) strictly increasing: the documented emission order, no record twice."""
    key = rec["flush_word"].astype(np.int64) * (n * n) + rec["hap_a"].astype(np.int64) * n + rec["hap_b"]
    assert np.all(np.diff(key) > 0)


def raw_identify(ctx, c, cap, out=None):
    """fsmc_identify (the default options) straight through ctypes: (return code, count, record array of ``cap``)."""
    assert set(c.kw) <= {"gap", "skip", "min_m"}
    words, ids = device_inputs(c)
    jw = capi._JobWindow(0, 1, 1, 1, 0)
    if out is None and cap:
        out = np.zeros(cap, capi.CANDIDATE_DTYPE)
    n = C.c_size_t(0)
    rc = ctx._L.fsmc_identify(ctx._h, capi._p(words), words.shape[0], words.shape[1], capi._p(ids), C.byref(jw),
                              capi._p(c.gen), c.gen.size, c.kw["gap"], c.kw.get("skip", 0.0), c.kw["min_m"],
                              capi._p(out) if cap else None, cap, C.byref(n))
    return rc, int(n.value), out


def fetch(ctx, cap):
    out = np.zeros(max(cap, 1), capi.CANDIDATE_DTYPE)
    n = C.c_size_t(0)
    rc = ctx._L.fsmc_identify_fetch(ctx._h, capi._p(out), cap, C.byref(n))
    return rc, int(n.value), out[:cap]


@pytest.mark.parametrize("name", E.NAMES)
def test_exact_list_order_and_flush_words(ctx, name):
    c = E.case(name)
    words, ids = device_inputs(c)
    rec = ctx.identify(words, ids, c.gen, **c.kw)
    assert as_list(rec) == c.want
    check_order(rec, c.n_device)
    if not c.kw.get("skip"):
        # every word takes part: an interval is reported at the first word cur with end < cur - gap, or at n_words
        assert [int(x) for x in rec["flush_word"]] == E.flush_words(c)
    assert int(rec["flush_word"].max()) <= c.n_words
    if set(c.kw) <= {"gap", "skip", "min_m"}:  # the default options: the same through fsmc_identify itself
        rc, n, out = raw_identify(ctx, c, len(c.want))
        assert (rc, n) == (FSMC_OK, len(c.want))
        assert out.tobytes() == rec.tobytes()


@pytest.mark.parametrize("name", E.names("stage_overflow"))
def test_the_arrival_order_of_the_appends_does_not_show(ctx, name):
    c = E.case(name)
    words, ids = device_inputs(c)
    first = ctx.identify(words, ids, c.gen, **c.kw)
    second = ctx.identify(words, ids, c.gen, **c.kw)
    assert first.size == len(c.want)
    assert first.tobytes() == second.tobytes()


@pytest.mark.parametrize("name", E.names("chunk_runs") + E.names("mixed_chunks"))
def test_general_kernel_on_the_default_kernels_inputs(ctx, name):
    """max_seeds above n_haps selects id_match_general_kernel<true> (fsmc_identify_ex: max_seeds > 0) and never
    splits a seed: the list, flush words included, is the default kernel's."""
    c = E.case(name)
    words, ids = device_inputs(c)
    default = ctx.identify(words, ids, c.gen, **c.kw)
    general = ctx.identify(words, ids, c.gen, max_seeds=c.n_device + 1, **c.kw)
    assert as_list(general) == c.want
    assert general.tobytes() == default.tobytes()


@pytest.mark.parametrize("name", ["chunk_runs-W100-gap1", "chunk_runs-W33-gap0"])
def test_buffer_protocol(ctx, name):
    c = E.case(name)
    count = len(c.want)
    rc, n, full = raw_identify(ctx, c, count)                       # cap == count
    assert (rc, n) == (FSMC_OK, count) and as_list(full) == c.want
    assert fetch(ctx, count)[0] == FSMC_ESTATE                      # nothing is kept after a call that fitted
    for cap in (count - 1, 0):                                      # (cap == 0 with out = NULL)
        rc, n, _ = raw_identify(ctx, c, cap)
        assert (rc, n) == (FSMC_EOVERFLOW, count)
        rc, n, _ = fetch(ctx, count - 1)                            # a short fetch keeps the list
        assert (rc, n) == (FSMC_EOVERFLOW, count)
        rc, n, out = fetch(ctx, count)
        assert (rc, n) == (FSMC_OK, count) and out.tobytes() == full.tobytes()
        rc, n, _ = fetch(ctx, count)                                # ... the full one releases it
        assert (rc, n) == (FSMC_ESTATE, 0)


def test_a_new_identify_replaces_an_unfetched_list(ctx):
    a, b = E.case("chunk_runs-W100-gap0"), E.case("chunk_runs-W96-gap32")
    assert a.want != b.want
    rc, n, _ = raw_identify(ctx, a, 0)
    assert (rc, n) == (FSMC_EOVERFLOW, len(a.want))
    rc, n, out = raw_identify(ctx, b, len(b.want))                  # fits: the second call's list, nothing kept
    assert (rc, n) == (FSMC_OK, len(b.want)) and as_list(out) == b.want
    assert fetch(ctx, len(a.want))[0] == FSMC_ESTATE
    rc, n, _ = raw_identify(ctx, a, 0)
    assert (rc, n) == (FSMC_EOVERFLOW, len(a.want))
    rc, n, _ = raw_identify(ctx, b, 1)                              # overflows too: the kept list is the second call's
    assert (rc, n) == (FSMC_EOVERFLOW, len(b.want))
    rc, n, out = fetch(ctx, len(b.want))
    assert (rc, n) == (FSMC_OK, len(b.want)) and as_list(out) == b.want


@pytest.mark.parametrize("name", ["huge_gap-default-W100-gap2147483647", "huge_gap-words-W100-gap2147483647"])
def test_huge_gap_on_the_product_path(name):
    """DecodingParams.gap reaches fsmc_identify_ex unchecked (HashingPrefilter::runOnDevice): the C ABI takes it."""
    c = E.case(name)
    data, p = host_data(c), host_params(c)
    assert p.gap == E.INT_MAX
    assert [tuple(x) for x in api.hashingCandidatesDevice(data, p)] == c.want
