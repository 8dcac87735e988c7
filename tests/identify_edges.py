"""Inputs at the edges of the identification kernels (fastsmc_amd/csrc/fsmc_identify.h): runs and run-outs at the
boundaries of the 32-word LDS chunks, chunks that alternate between the event walk and the word-by-word walk, more
reports of one tile than its LDS stage holds, a length exactly at min_m, the deepest seed split the read-ahead window
allows, and gaps up to INT_MAX.

Every case is built from WORDS (uint64 [n][W]); the alleles the restatement reads are the words' bits.  The usual
shape is a pattern cohort: haplotype 0 has random words, haplotype k copies them on a given word set and is unique
elsewhere (the top byte of a word is the haplotype's number + 1, so two words are equal only where one was copied).
gen[s] = s * 2^-12 Morgans: every length is a small multiple of 100 / 4096 cM, exact in float32 and in double.

``case(name)`` returns the inputs with ``want``, the candidate list of tests/test_hashing.py::restate_candidates,
computed once per process.  Each family has a census, computed on the CPU from the inputs and ``want`` alone, that
counts how often the regime the case is built for is reached; tests/test_identify_edges.py asserts the counts, so
that a later change to a builder cannot quietly turn an edge case into a benign one.

Plain helper module imported by tests/test_identify_edges.py (CPU) and tests/test_gpu_identify_edges.py (GPU)."""
from __future__ import annotations

import functools
from collections import Counter
from types import SimpleNamespace

import numpy as np

from test_hashing import restate_candidates

CHUNK = 32   # kIdChunk: words per LDS chunk = bits of an equality mask
TILE = 32    # kIdTile: haplotypes per tile side
STAGE = 512  # kIdStage: records of one tile's LDS stage
GEN_STEP = 2.0 ** -12
INT_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- builders

def unique_words(n, W, seed):
    """Random words, no two haplotypes equal on any word (top byte = haplotype number + 1)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 56, size=(n, W), dtype=np.uint64)
    return w | ((np.arange(n, dtype=np.uint64)[:, None] + np.uint64(1)) << np.uint64(56))


def unpack(words, word_size=64):
    """uint8 alleles [n][W * word_size]: bit b of word w is the allele of site w * word_size + b."""
    n, W = words.shape
    bits = (words[:, :, None] >> np.arange(word_size, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(n, W * word_size).astype(np.uint8)


def gen_positions(n_sites):
    return (np.arange(n_sites, dtype=np.float64) * GEN_STEP).astype(np.float32)


def _case(words, n_device=None, **kw):
    """``kw``: the keywords of capi.Context.identify and of restate_candidates (the same names).  ``n_device``: the
    rows handed to the device and to the census when the last row only pads the cohort to whole individuals."""
    words = np.ascontiguousarray(words, np.uint64)
    assert words.shape[0] % 2 == 0 and words.shape[0] <= 96 and words.shape[1] <= 100
    kw.setdefault("min_m", 0.0)
    kw.setdefault("gap", 1)
    return SimpleNamespace(words=words, alleles=unpack(words), gen=gen_positions(words.shape[1] * 64), kw=kw,
                           n_device=n_device or words.shape[0], n_words=words.shape[1])


def _r(a, b):
    return list(range(a, b + 1))


# the match sets of the pattern cohort: haplotype k + 1 shares set k with haplotype 0
MATCH_SETS = [_r(0, 31), _r(1, 32), _r(31, 32), _r(0, 63), _r(32, 63), _r(20, 83),
              [31], [32], [0, 33], [0, 34], [31, 64], [31, 65],
              _r(0, 99), [99], [95, 99], _r(64, 99), [10, 45, 80],
              [30, 62, 64]]  # (run-outs at the LAST word of a chunk, 31 and 63, with gap 0; a hole of one word, the
                             #  last of chunk 1, that gap 1 closes; with gap 31 word 62 is matched exactly where the
                             #  interval of word 30 runs out)


def pattern_cohort(W, seed=1):
    sets = []
    for s in MATCH_SETS:
        s = [w for w in s if w < W]
        if s and s not in sets:
            sets.append(s)
    n = 1 + len(sets)
    n += n % 2
    words = unique_words(n, W, seed)
    for k, s in enumerate(sets):
        words[k + 1, s] = words[0, s]
    return words


CHUNK_RUN_WORDS = (100, 96, 33)  # a last chunk of 4 words, a full last chunk, a last chunk of one word
CHUNK_RUN_GAPS = (0, 1, 31, 32, 33)


def chunk_runs(W, gap):
    return _case(pattern_cohort(W), gap=gap)


# low-complexity words (two distinct values among all haplotypes): at 31 | 32 and at 63 the chunks 0 and 1 walk word by
# word and the chunks after them walk events; at 32, 63 and 97 the chunks alternate event / word / event / word.  Word 50
# lies inside the open intervals of the sets 0..63, 20..83 and 0..99.
MIXED_LOW = {"a": (31, 32, 50, 63), "b": (32, 50, 63, 97)}
MIXED_GAPS = (0, 1, 32)
MIXED_SKIP = 0.15


def mixed_chunks(variant, gap):
    words = pattern_cohort(100)
    n = words.shape[0]
    assert 2.0 / n < MIXED_SKIP
    for u in MIXED_LOW[variant]:
        words[:, u] = np.where(np.arange(n) % 2 == 0, np.uint64(0xA5A5), np.uint64(0x5A5A))
    return _case(words, gap=gap, skip=MIXED_SKIP)


STAGE_KINDS = ("direct", "end", "half")


def stage_overflow(kind, n_haps):
    """direct: every haplotype shares the even words -- 16 intervals per pair and chunk, 16 384 reports of an
    off-diagonal tile per chunk; end: all words equal -- 1024 reports of such a tile after the last word; half: 16
    haplotypes of tile 0 and 20 of tile 1 share ONE word per chunk -- 320 reports of tile (0, 1) per chunk, more than
    half the stage and never more than the stage.  n_haps = 65: a tile row and column of one haplotype (the cohort
    is padded with a haplotype that shares nothing: with skip = 0 the restatement of the 66 is that of the 65)."""
    W = 96
    n = n_haps + n_haps % 2
    words = unique_words(n, W, 7)
    if kind == "direct":
        words[:n_haps, 0::2] = words[0, 0::2]
    elif kind == "end":
        words[:n_haps, :] = words[0, :]
    else:
        group = list(range(16)) + list(range(32, 52)) + list(range(64, n_haps))
        for w in (5, 40, 70):
            words[group, w] = words[0, w]
    return _case(words, n_device=n_haps, gap=0)


def threshold(above):
    """min_m = the exact length of a candidate (kept: >=) or the next float32 above it (dropped)."""
    base = case("chunk_runs-W100-gap1")
    lengths = sorted({interval_cm(c) for c in base.want})
    length = np.float32(lengths[len(lengths) // 2])
    assert float(length) == lengths[len(lengths) // 2]  # (exact in float32)
    min_m = float(np.nextafter(length, np.float32(np.inf))) if above else float(length)
    c = _case(base.words, gap=1, min_m=min_m)
    c.length = float(length)
    return c


DEEP_SHARED = (0, 1, 2, 5, 33, 38)   # six haplotypes share the words 31..70
DEEP_DIVERGE = (3, 7, 34)            # share words 2 .. 2 + read_ahead - 2: at word 2 they diverge at 2 + read_ahead - 1
DEEP_TAIL = (4, 35, 39)              # share the last ten words: min(n_words, c + read_ahead) binds
DEEP_OPTS = [dict(read_ahead=32, haploid=True, gap=1), dict(read_ahead=32, haploid=False, gap=1),
             dict(read_ahead=32, haploid=True, gap=0), dict(read_ahead=1, haploid=True, gap=1),
             dict(read_ahead=1, haploid=False, gap=1), dict(read_ahead=7, haploid=True, gap=1)]


def deep_split(read_ahead, haploid, gap):
    W, n = 100, 40
    words = unique_words(n, W, 13)
    words[list(DEEP_SHARED), 31:71] = words[0, 31:71]
    if read_ahead > 1:
        words[list(DEEP_DIVERGE), 2:2 + read_ahead - 1] = words[DEEP_DIVERGE[0], 2:2 + read_ahead - 1]
    words[list(DEEP_TAIL), W - 10:] = words[DEEP_TAIL[0], W - 10:]
    return _case(words, gap=gap, max_seeds=1, read_ahead=read_ahead, haploid=haploid)


def huge_gaps(W):
    return (W - 1, W, 1000, INT_MAX - 1, INT_MAX)


HUGE_WORDS = (100, 33)


def huge_gap(W, gap, kernel="default"):
    """kernel: default -- id_match_kernel's event walk; words -- its word-by-word walk (low-complexity words);
    general -- id_match_general_kernel (max_seeds above n_haps: set, and never splits)."""
    words = pattern_cohort(W)
    kw = dict(gap=gap)
    if kernel == "words":
        words[:, 40 % W] = np.where(np.arange(words.shape[0]) % 2 == 0, np.uint64(0xA5A5), np.uint64(0x5A5A))
        kw["skip"] = MIXED_SKIP
    elif kernel == "general":
        kw["max_seeds"] = words.shape[0] + 1
    return _case(words, **kw)


def _case_name(fn, args):
    """The name of the case a builder makes from these arguments."""
    if fn is chunk_runs:
        return f"chunk_runs-W{args[0]}-gap{args[1]}"
    if fn is mixed_chunks:
        return f"mixed_chunks-{args[0]}-gap{args[1]}"
    if fn is stage_overflow:
        return f"stage_overflow-{args[0]}-n{args[1]}"
    if fn is threshold:
        return f"threshold-{'above' if args[0] else 'at'}"
    if fn is deep_split:
        return f"deep_split-ra{args[0]}-{'hap' if args[1] else 'ind'}-gap{args[2]}"
    return f"huge_gap-{args[2] if len(args) > 2 else 'default'}-W{args[0]}-gap{args[1]}"


def _registry():
    calls = [(chunk_runs, (W, g)) for W in CHUNK_RUN_WORDS for g in CHUNK_RUN_GAPS]
    calls += [(mixed_chunks, (v, g)) for v in MIXED_LOW for g in MIXED_GAPS]
    calls += [(stage_overflow, (k, n)) for n in (64, 65) for k in STAGE_KINDS]
    calls += [(threshold, (above,)) for above in (False, True)]
    calls += [(deep_split, (o["read_ahead"], o["haploid"], o["gap"])) for o in DEEP_OPTS]
    calls += [(huge_gap, (W, g)) for W in HUGE_WORDS for g in huge_gaps(W)]
    calls += [(huge_gap, (100, g, kernel)) for kernel in ("words", "general") for g in (1000, INT_MAX)]
    return {_case_name(fn, args): (fn, args) for fn, args in calls}


_BY_NAME = _registry()
NAMES = list(_BY_NAME)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name with ``want``, the restatement's candidate list; built once per process."""
    fn, args = _BY_NAME[name]
    c = fn(*args)
    c.name = name
    c.want = restate_candidates(c.alleles, c.gen, list(range(c.words.shape[0] // 2)), **c.kw)
    return c


def names(prefix):
    return [n for n in NAMES if n.startswith(prefix)]


# ---------------------------------------------------------------- what the restatement says about a case

def interval_cm(cand):
    """Length of a candidate (hap_a, hap_b, from, to) in centimorgans, as Match::print computes it -- exact here."""
    return (cand[3] - cand[2]) * GEN_STEP * 100.0


def intervals(c):
    """(hap_a, hap_b, first word, last word) of every candidate of ``c.want``."""
    return [(a, b, f // 64, t // 64) for a, b, f, t in c.want]


def flush_words(c):
    """The word at which each candidate of ``c.want`` is reported when every word takes part (skip = 0): the first
    word cur with end < cur - gap, or n_words (clearAllPairs)."""
    assert not c.kw.get("skip")
    return [min(e + c.kw["gap"] + 1, c.n_words) for _, _, _, e in intervals(c)]


def used_words(c):
    """bool [W]: the word takes part -- distinct values / haplotypes > skip, both float32 (FastSMC.cpp:208-212)."""
    w = c.words[:c.n_device]
    distinct = np.array([len(np.unique(w[:, k])) for k in range(c.n_words)], np.float32)
    return distinct / np.float32(w.shape[0]) > np.float32(c.kw.get("skip", 0.0))


def census_runs(c):
    """How often the intervals of a default-option case reach the edges of id_match_kernel's event walk."""
    W, g = c.n_words, c.kw["gap"]
    used = used_words(c)
    k = Counter()
    for a, b, s, e in intervals(c):
        m = (c.words[a] == c.words[b]) & used
        k["spans_31_32"] += s <= 31 and e >= 32
        runout = e + g + 1
        for r in (31, 32, 63, 64):
            k[f"runout_{r}"] += runout == r and r < W
        k["open_at_n_words"] += runout >= W
        for c0 in range(0, W - CHUNK + 1, CHUNK):
            full = bool(m[c0:c0 + CHUNK].all())
            inside = s <= c0 and c0 + CHUNK - 1 <= e
            k["run_of_32_from_bit_0"] += inside and full
            k["run_ends_at_bit_31"] += s <= c0 + CHUNK - 1 <= e and bool(m[c0 + CHUNK - 1]) and not full
            k["open_over_chunk_without_match"] += s < c0 and c0 + CHUNK <= e + g + 1 and not m[c0:c0 + CHUNK].any()
    return k


def census_mixed(c):
    used = used_words(c)
    k = Counter()
    for c0 in range(0, c.n_words, CHUNK):
        k["event_chunks" if used[c0:c0 + CHUNK].all() else "word_chunks"] += 1
    kinds = [bool(used[c0:c0 + CHUNK].all()) for c0 in range(0, c.n_words, CHUNK)]
    k["path_changes"] = sum(x != y for x, y in zip(kinds, kinds[1:]))
    boundary = [u for u in np.flatnonzero(~used) if u % CHUNK in (0, CHUNK - 1)]
    for a, b, s, e in intervals(c):
        k["carried_over_unused_boundary_word"] += any(s < u <= e for u in boundary)
        k["carried_over_unused_word"] += any(s < u <= e for u in np.flatnonzero(~used))
    return k


def census_stage(c):
    """Reports per (tile, chunk) and per (tile, "end"): what id_match_kernel stages between two chunk boundaries."""
    per = Counter()
    for (a, b, _, _), fw in zip(intervals(c), flush_words(c)):
        per[(a // TILE, b // TILE), "end" if fw == c.n_words else fw // CHUNK] += 1
    last = (c.n_words - 1) // CHUNK
    tiles = {t for t, _ in per}
    return SimpleNamespace(
        per=per,
        max_chunk=max([v for (_, bucket), v in per.items() if bucket != "end"], default=0),
        max_end=max([v for (_, bucket), v in per.items() if bucket == "end"], default=0),
        # the reports of the last chunk are still staged when clearAllPairs adds its own
        max_last_plus_end=max([per[t, last] + per[t, "end"] for t in tiles], default=0))


def depth_table(c):
    """Brute force of SeedHash.hpp:41-85: depth[word][haplotype] = the number of further words a haplotype's seed of
    that word is split by -- the first d with at most max_seeds haplotypes sharing words c .. c + d, or with
    c + d + 1 = the words read, min(n_words, c + read_ahead)."""
    w = c.words[:c.n_device]
    n, W = w.shape
    ms, ra = c.kw["max_seeds"], c.kw.get("read_ahead", 10)
    depth = np.zeros((W, n), np.int64)
    for cw in range(W):
        read = min(W, cw + ra)
        same = np.ones((n, n), bool)
        for d in range(ra):
            same &= w[:, None, cw + d] == w[None, :, cw + d]
            undecided = (same.sum(axis=1) > ms) & (cw + d + 1 < read)
            depth[cw][undecided] = d + 1
            if not undecided.any():
                break
    return depth
