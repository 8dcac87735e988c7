"""The edge inputs of the identification kernels (tests/identify_edges.py) on the CPU: every census -- the regime a
case is built for is reached, counted from the inputs and the restatement's own list -- and the host C++ restatement
(api.hashingCandidates) against tests/test_hashing.py::restate_candidates on every case.  The device runs the same
cases in tests/test_gpu_identify_edges.py."""
from collections import Counter

import numpy as np
import pytest

import identify_edges as E
from fastsmc_amd import api
from test_hashing import restate_candidates


def host_data(c):
    """api.Data of a case, no folding: its hashing words are the case's words, its genetic positions the case's."""
    S = c.alleles.shape[1]
    bp = np.arange(1, S + 1, dtype=np.int64) * 100
    cm = np.arange(S, dtype=np.float64) * (100.0 * E.GEN_STEP)
    data = api.Data.from_arrays(c.alleles, bp, cm, False, True)
    assert np.array_equal(np.asarray(data.geneticPositions, np.float32), c.gen)
    return data


def host_params(c):
    p = api.DecodingParams()
    p.gap = c.kw["gap"]
    p.min_m = c.kw["min_m"]
    p.skip = c.kw.get("skip", 0.0)
    p.haploid = c.kw.get("haploid", True)
    p.max_seeds = c.kw.get("max_seeds", 0)
    p.constReadAhead = c.kw.get("read_ahead", 10)
    return p


@pytest.mark.parametrize("name", E.NAMES)
def test_host_restatement_equals_the_python_one(name):
    c = E.case(name)
    data, p = host_data(c), host_params(c)
    assert np.array_equal(api.hashingWords(data, p), c.words)
    assert [tuple(x) for x in api.hashingCandidates(data, p)] == c.want
    assert len(c.want) > 0
    assert all(b < c.n_device for _, b, _, _ in c.want)  # (a padding haplotype takes part in nothing)


@pytest.mark.parametrize("W", E.CHUNK_RUN_WORDS)
def test_census_chunk_runs(W):
    cases = [E.case(f"chunk_runs-W{W}-gap{g}") for g in E.CHUNK_RUN_GAPS]
    # every gap value changes the list -- up to n_words - 1: from there on nothing is reported before the end
    lists = {c.kw["gap"]: tuple(c.want) for c in cases}
    below = [lists[g] for g in E.CHUNK_RUN_GAPS if g < W - 1]
    assert len(set(below)) == len(below) >= 3
    assert len({lists[g] for g in E.CHUNK_RUN_GAPS if g >= W - 1}) <= 1
    total = Counter()
    for c in cases:
        assert np.all(E.used_words(c))  # skip = 0: every chunk walks events
        total.update(E.census_runs(c))
    kinds = ["spans_31_32", "run_of_32_from_bit_0", "run_ends_at_bit_31", "runout_31", "runout_32", "open_at_n_words"]
    if W > 2 * E.CHUNK:  # (these need a third chunk)
        kinds += ["runout_63", "runout_64", "open_over_chunk_without_match"]
    for kind in kinds:
        assert total[kind] >= 1, (kind, dict(total))
    if W == 100:  # the gaps of 32 and more carry an interval over a whole chunk; the smaller ones cannot
        by_gap = {c.kw["gap"]: E.census_runs(c)["open_over_chunk_without_match"] for c in cases}
        assert by_gap[0] == by_gap[1] == 0 and by_gap[32] >= 1 and by_gap[33] >= 1, by_gap


@pytest.mark.parametrize("variant", list(E.MIXED_LOW))
def test_census_mixed_chunks(variant):
    total = Counter()
    for g in E.MIXED_GAPS:
        c = E.case(f"mixed_chunks-{variant}-gap{g}")
        used = E.used_words(c)
        assert sorted(np.flatnonzero(~used)) == sorted(E.MIXED_LOW[variant])
        k = E.census_mixed(c)
        assert k["event_chunks"] >= 1 and k["word_chunks"] >= 1, dict(k)
        assert k["carried_over_unused_boundary_word"] >= 1 and k["carried_over_unused_word"] >= 1, dict(k)
        assert k["path_changes"] >= (3 if variant == "b" else 1), dict(k)
        # the unused words change the list: the same cohort without them is chunk_runs
        plain = E.case(f"chunk_runs-W100-gap{g}") if g in E.CHUNK_RUN_GAPS else None
        assert plain is None or plain.want != c.want
        total.update(k)
    assert total["carried_over_unused_boundary_word"] >= 3


@pytest.mark.parametrize("n_haps", [64, 65])
def test_census_stage_overflow(n_haps):
    pairs = n_haps * (n_haps - 1) // 2
    direct = E.case(f"stage_overflow-direct-n{n_haps}")
    s = E.census_stage(direct)
    assert len(direct.want) == pairs * 48
    assert s.max_chunk == 16 * E.TILE * E.TILE > E.STAGE       # more than the stage holds between two chunk boundaries
    end = E.case(f"stage_overflow-end-n{n_haps}")
    s = E.census_stage(end)
    assert len(end.want) == pairs and s.max_chunk == 0
    assert s.max_end == E.TILE * E.TILE > E.STAGE               # more than the stage holds after the last word
    half = E.case(f"stage_overflow-half-n{n_haps}")
    s = E.census_stage(half)
    assert E.STAGE // 2 <= s.max_chunk <= E.STAGE               # the flush in the loop ...
    assert s.max_last_plus_end <= E.STAGE                       # ... and never a record past the stage
    assert s.per[(0, 1), 0] == s.per[(0, 1), 1] == s.per[(0, 1), 2] == 320
    if n_haps == 65:  # the tile row and column of one haplotype report too
        for c in (direct, end, half):
            assert any(t == (0, 2) for t, _ in E.census_stage(c).per), c.name


def test_census_threshold():
    base, at, above = E.case("chunk_runs-W100-gap1"), E.case("threshold-at"), E.case("threshold-above")
    assert at.kw["min_m"] == at.length < above.kw["min_m"]
    assert np.float32(above.kw["min_m"]) == np.nextafter(np.float32(at.length), np.float32(np.inf))
    exact = [x for x in base.want if E.interval_cm(x) == at.length]
    assert len(exact) >= 1
    assert at.want == [x for x in base.want if E.interval_cm(x) >= at.length]
    assert above.want == [x for x in at.want if x not in exact]
    assert 0 < len(above.want) < len(at.want) < len(base.want)


@pytest.mark.parametrize("opts", E.DEEP_OPTS, ids=lambda o: f"ra{o['read_ahead']}-{'hap' if o['haploid'] else 'ind'}")
def test_census_deep_split(opts):
    ra = opts["read_ahead"]
    c = E.case(f"deep_split-ra{ra}-{'hap' if opts['haploid'] else 'ind'}-gap{opts['gap']}")
    depth = E.depth_table(c)
    assert depth.max() == ra - 1  # the deepest split the window allows (read_ahead = 1: nothing splits)
    shared, diverge, tail = list(E.DEEP_SHARED), list(E.DEEP_DIVERGE), list(E.DEEP_TAIL)
    if ra == 32:
        # depth 31 at the last word of chunk 0: the interval's end lies 31 words ahead, in chunk 1, and the 64-bit
        # equality window of the general kernel is used up to bit 31 + 31
        assert np.all(depth[31, shared] == 31) and 31 % E.CHUNK == 31
        assert np.all(depth[39, shared] == 31)  # words 39..70 are the last 32 the six share
    pairs = {(x, y) for x, y, _, _ in c.want}
    if ra > 1:
        # the members share words 2 .. read_ahead and diverge exactly at the last word read from word 2: the seed is
        # split down to singletons there and at every later word, so with max_seeds = 1 no pair of them is extended
        assert np.all(depth[2, diverge] == ra - 1) and np.all(depth[3, diverge] == ra - 2)
        if opts["haploid"]:
            assert not pairs & {(a, b) for a in diverge for b in diverge}
        # the last words: the words read stop at n_words, and what is shared up to there is extended
        assert depth[c.n_words - 3, tail[0]] == 2 and depth[c.n_words - 1, tail[0]] == 0
    if opts["haploid"]:
        assert (tail[0], tail[1]) in pairs and (shared[0], shared[-1]) in pairs
    unsplit = restate_candidates(c.alleles, c.gen, list(range(c.words.shape[0] // 2)), **dict(c.kw, max_seeds=0))
    assert (unsplit != c.want) == (ra > 1)  # the splitting changes the list whenever anything is split


@pytest.mark.parametrize("W", E.HUGE_WORDS)
def test_census_huge_gap(W):
    lists = [E.case(f"huge_gap-default-W{W}-gap{g}").want for g in E.huge_gaps(W)]
    assert all(x == lists[0] for x in lists)  # every gap >= n_words - 1 means "never before the end"
    pairs = [(a, b) for a, b, _, _ in lists[0]]
    assert len(pairs) == len(set(pairs)) and pairs == sorted(pairs)  # every pair once, at the end
    words = E.case(f"huge_gap-default-W{W}-gap{W}").words
    sharing = {(a, b) for a in range(len(words)) for b in range(a + 1, len(words)) if np.any(words[a] == words[b])}
    assert set(pairs) == sharing
    assert lists[0] != E.case(f"chunk_runs-W{W}-gap31").want  # (a gap below n_words - 1 reports earlier)
    for kernel in ("words", "general") if W == 100 else ():
        a, b = (E.case(f"huge_gap-{kernel}-W100-gap{g}") for g in (1000, E.INT_MAX))
        assert a.want == b.want and len({(x, y) for x, y, _, _ in a.want}) == len(a.want)


def test_every_case_is_small():
    for name in E.NAMES:
        c = E.case(name)
        assert c.words.shape[0] <= 96 and c.n_words <= 100
