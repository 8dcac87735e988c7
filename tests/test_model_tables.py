"""A model's tables as the kernels read them (fastsmc_amd/csrc/fsmc_model_tables.h) on a CPU: tests/model_tables_driver.cpp,
compiled here with plain g++, builds them from the cases below and every result is compared bit for bit -- float arrays
travel as the 32-bit patterns of their elements, so -0.0 is not +0.0 and nothing is rounded on the way.  No tolerance
appears anywhere.

The emission table is checked against numpy.float32 arithmetic written with the reference's association,
(e1 + e0m1*z) + e2m0*t for (z, t) in (0,0), (1,0), (1,1), and (h + h*0) + h*0 for the fourth row of sequence mode.  The
status codes and messages of the two checks are the texts fsmc_model_create and fsmc_worklist_upload returned before
the checks moved out of fsmc_capi.hip (the test_pair_*_abi.py tests and the host layer read them)."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from conftest import expected_member, wave_group_member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "fastsmc_amd", "csrc", "fsmc_model_tables.h")

EINVAL, EUNSUPPORTED = -1, -7
PARTS = ("D", "B", "U", "Ush", "RR")  # the order of a RowSet's parts


def _hex(a):
    return ",".join(f"{w:08x}" for w in np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("model_tables") / "model_tables_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "fastsmc_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "model_tables_driver.cpp")], check=True)

    def run(*cases):
        out = subprocess.run([exe], input="".join(c + "\n" for c in cases), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return out

    return run


def _bits(line):
    n, bits = line.split()
    words = np.array([int(w, 16) for w in bits[len("bits="):].split(",")], dtype=np.uint32)
    assert n == f"n={words.size}"
    return words


# ---- shape -----------------------------------------------------------------------------------------------------------

SHAPE_LITERALS = {2: (16, 0), 16: (16, 0), 17: (32, 0), 69: (80, 0), 128: (128, 0), 129: (192, 4), 600: (640, 8),
                  1025: (1040, 0)}
SHAPE_BY_MEMBER = (192, 193, 256, 257, 320, 321, 512, 513, 1024, 4096)


def test_shape(driver):
    ks = sorted(SHAPE_LITERALS) + list(SHAPE_BY_MEMBER)
    got = {}
    for K, line in zip(ks, driver(*(f"shapeOf K={K}" for K in ks))):
        kp, nw = (int(f.split("=")[1]) for f in line.split())
        got[K] = (kp, nw)
    for K, want in SHAPE_LITERALS.items():
        assert got[K] == want, K
    for K in SHAPE_BY_MEMBER:
        if expected_member(K) == 0:  # beyond the wave-group kernel: padded rows, no wave group
            assert got[K] == ((K + 15) // 16 * 16, 0), K
        else:
            nw, kh = wave_group_member(K)
            assert got[K] == (nw * kh, nw), K
            assert expected_member(K) == (1000 + kh if nw == 4 else 1000 * nw + kh)
    # every model's rows hold its states and are whole operand blocks
    assert all(kp >= K and kp % 16 == 0 for K, (kp, _) in got.items())


def test_shape_honours_the_diagnostic_member(driver):
    assert driver("shapeOf K=250 w2nw=4 w2kh=80", "shapeOf K=250 w2nw=7 w2kh=64", "shapeOf K=100 w2nw=4 w2kh=80") == [
        "KP=320 w2NW=4", "KP=256 w2NW=4", "KP=112 w2NW=0"]


# ---- padded rows, RowSet, ghost mask, step rows ----------------------------------------------------------------------

def _tables(K, rows, seed):
    """Four tables of distinct non-zero values (no two elements of the four share a bit pattern)."""
    rng = np.random.default_rng(seed)
    vals = rng.permutation(4 * rows * K).astype(np.float32) + np.float32(1.0)
    vals[::7] *= np.float32(-1.0)
    return {name: vals[i * rows * K:(i + 1) * rows * K].reshape(rows, K) for i, name in enumerate(("D", "B", "U", "RR"))}


@pytest.mark.parametrize("K,KP", [(5, 16), (69, 80)])
def test_row_sets_and_padding(driver, K, KP):
    rows = 3
    t = _tables(K, rows, seed=K)
    case = f"rowSets K={K} KP={KP} rows={rows} " + " ".join(f"{n}={_hex(t[n])}" for n in ("D", "B", "U", "RR"))
    lines = driver(case, *(f"padRows K={K} KP={KP} rows={rows} src={_hex(t[n])}" for n in ("D", "B", "U", "RR")),
                   f"ghostMask K={K} KP={KP}")
    rs = _bits(lines[0]).reshape(rows, len(PARTS), KP)
    part = {name: rs[:, i, :] for i, name in enumerate(PARTS)}
    for name in ("D", "B", "U", "RR"):  # the part order is D | B | U | Ush | RR
        assert np.array_equal(part[name][:, :K], t[name].view(np.uint32)), name
    u = t["U"].view(np.uint32)
    assert np.all(part["Ush"][:, 0] == 0)  # Ush[0] is +0.0
    assert np.array_equal(part["Ush"][:, 1:K], u[:, :K - 1])  # Ush[k] == U[k-1], bit for bit
    assert np.all(rs[:, :, K:] == 0)  # every pad float is +0.0 (bit pattern 0: not -0.0)
    for line, name in zip(lines[1:5], ("D", "B", "U", "RR")):
        padded = _bits(line).reshape(rows, KP)
        assert np.array_equal(padded[:, :K], t[name].view(np.uint32)) and np.all(padded[:, K:] == 0), name
    mask = _bits(lines[5])
    assert mask.size == KP and np.all(mask[:K] == np.float32(1.0).view(np.uint32)) and np.all(mask[K:] == 0)


def test_step_rows_clear_element_zero(driver):
    got = driver("stepRows src=7,1,0,3", "stepRows src=-5", "stepRows src=0,2,2", "stepRows src=2147483647,-1,5")
    assert got == ["n=4 rows=0,1,0,3", "n=1 rows=0", "n=3 rows=0,2,2", "n=3 rows=0,-1,5"]


# ---- emissions -------------------------------------------------------------------------------------------------------

def _emission_inputs(K, S, seed):
    """[S][K] inputs with the cases a wrong tabulation gets wrong in the first elements: e1 = -0.0 with negative factors
    (a folded x*0 gives +0.0), subnormals, sums that round, a zero from cancellation."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    e1 = rng.uniform(0.0, 1.0, S * K).astype(f32)
    e0m1 = rng.uniform(-1.0, 1.0, S * K).astype(f32)
    e2m0 = rng.uniform(-1.0, 1.0, S * K).astype(f32)
    tiny = f32(np.finfo(f32).smallest_subnormal)
    special = [
        (f32(-0.0), f32(-0.25), f32(-0.5)),                 # -0.0 + (-0.25 * 0) + (-0.5 * 0) = -0.0
        (f32(-0.0), f32(0.25), f32(-0.5)),                  # -0.0 + (+0.0) = +0.0
        (f32(0.0), f32(-1.0), f32(-2.0)),
        (tiny, tiny, -tiny),                                # subnormals: class 2 cancels to +0.0
        (f32(3) * tiny, f32(5) * tiny, f32(-7) * tiny),
        (f32(1.0), f32(2.0 ** -24), f32(2.0 ** -24)),       # sums that round (ties to even, twice)
        (f32(1.0), f32(3 * 2.0 ** -25), f32(3 * 2.0 ** -25)),
        (f32(0.1), f32(0.2), f32(0.3)),
        (f32(1.0), f32(-1.0), f32(-0.0)),                   # 1 - 1 = +0.0, + -0.0 = +0.0
        (f32(np.finfo(f32).max), f32(np.finfo(f32).max), f32(-np.finfo(f32).max)),  # max + max = inf, and inf - max = inf
    ]
    for i, (a, b, c) in enumerate(special[:S * K]):
        e1[i], e0m1[i], e2m0[i] = a, b, c
    hom = rng.uniform(0.0, 1.0, S * K).astype(f32)
    for i, h in enumerate([f32(-0.0), f32(0.0), tiny, f32(-3) * tiny, f32(1.0), f32(np.inf)][:S * K]):
        hom[i] = h
    return [a.reshape(S, K) for a in (e1, e0m1, e2m0, hom)]


@pytest.mark.parametrize("sequence", [0, 1])
@pytest.mark.parametrize("K,KP,S", [(5, 16, 1), (5, 16, 2), (16, 16, 2), (69, 80, 5), (3, 16, 5)])
def test_emissions(driver, K, KP, S, sequence):
    e1, e0m1, e2m0, hom = _emission_inputs(K, S, seed=100 * K + S)
    case = f"emissions K={K} KP={KP} S={S} sequence={sequence} e1={_hex(e1)} e0m1={_hex(e0m1)} e2m0={_hex(e2m0)}"
    if sequence:
        case += f" hom={_hex(hom)}"
    nc = 4 if sequence else 3
    got = _bits(driver(case)[0]).reshape(S, nc, KP)
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        for c, (z, t) in enumerate(((0, 0), (1, 0), (1, 1))):
            want = (e1 + e0m1 * f32(z)) + e2m0 * f32(t)
            assert want.dtype == np.float32
            assert np.array_equal(got[:, c, :K], want.view(np.uint32)), (c, z, t)
        if sequence:
            want = (hom + hom * f32(0)) + hom * f32(0)
            assert np.array_equal(got[:, 3, :K], want.view(np.uint32))
    assert np.all(got[:, :, K:] == 0)  # the pad columns are +0.0
    # the case a folded x*0 gets wrong is in the table, and came out -0.0: -0.0 + (-0.25 * 0) + (-0.5 * 0)
    assert got[0, 0, 0] == 0x80000000
    if sequence:
        assert got[0, 3, 0] == 0x80000000  # (-0.0 + -0.0 * 0) + -0.0 * 0


# ---- the checks ------------------------------------------------------------------------------------------------------

NULL_TABLE = "null table pointer in model description"
SEQ_NEEDS = "sequence mode needs gap_row_f, site_row_f, gap_row_b, site_row_b and hom"

DESC_CASES = [
    ("checkDesc", 0, None),
    ("checkDesc sequence=1", 0, None),
    ("checkDesc K=2 S=1 n_rows=1", 0, None),
    ("checkDesc K=4096", 0, None),
    ("checkDesc state_threshold=3 age_threshold=3", 0, None),
    ("checkDesc K=1", EINVAL, "need K >= 2, S >= 1, n_rows >= 1"),
    ("checkDesc S=0", EINVAL, "need K >= 2, S >= 1, n_rows >= 1"),
    ("checkDesc n_rows=0", EINVAL, "need K >= 2, S >= 1, n_rows >= 1"),
    ("checkDesc K=4097", EUNSUPPORTED, "more than 4096 states"),
    *[(f"checkDesc null={f}", EINVAL, NULL_TABLE)
      for f in ("pi", "col_ratios", "exp_times", "D", "B", "U", "RR", "step_row", "e1", "e0m1", "e2m0")],
    ("checkDesc state_threshold=4", EINVAL, "state/age threshold larger than K"),
    ("checkDesc age_threshold=4", EINVAL, "state/age threshold larger than K"),
    *[(f"checkDesc sequence=1 null={f}", EINVAL, SEQ_NEEDS)
      for f in ("gap_row_f", "site_row_f", "gap_row_b", "site_row_b", "hom")],
    ("checkDesc step_row=2:2", EINVAL, "step_row[2] outside the transition tables"),
    ("checkDesc step_row=3:-1", EINVAL, "step_row[3] outside the transition tables"),
    ("checkDesc sequence=1 gap_row_f=1:2", EINVAL, "gap_row_f[1] outside the transition tables"),
    ("checkDesc sequence=1 site_row_f=2:9", EINVAL, "site_row_f[2] outside the transition tables"),
    ("checkDesc sequence=1 gap_row_b=3:-2", EINVAL, "gap_row_b[3] outside the transition tables"),
    ("checkDesc sequence=1 site_row_b=1:2", EINVAL, "site_row_b[1] outside the transition tables"),
    # array mode does not look at the sequence-mode arrays; site S and beyond is not the model's
    ("checkDesc gap_row_f=1:9", 0, None),
    ("checkDesc step_row=4:9", 0, None),
    # the order of the checks: sizes, state count, pointers, thresholds, sequence mode, rows (array by array)
    ("checkDesc K=1 null=pi", EINVAL, "need K >= 2, S >= 1, n_rows >= 1"),
    ("checkDesc K=4097 null=pi", EUNSUPPORTED, "more than 4096 states"),
    ("checkDesc null=pi state_threshold=4", EINVAL, NULL_TABLE),
    ("checkDesc sequence=1 state_threshold=4 null=hom", EINVAL, "state/age threshold larger than K"),
    ("checkDesc sequence=1 null=hom step_row=1:5", EINVAL, SEQ_NEEDS),
    ("checkDesc sequence=1 step_row=3:5 gap_row_f=1:5", EINVAL, "step_row[3] outside the transition tables"),
]

G = "10:0:0:100:0:100"  # ten pairs from pair 0, the whole window scanned
WORKLIST_CASES = [
    (f"checkWorklist n_pairs=10 groups={G}", 0, None),
    ("checkWorklist n_pairs=75 groups=10:0:0:100:5:100,64:10:20:30:20:21,1:74:0:1:0:1", 0, None),
    ("checkWorklist n_pairs=4294967281 groups=" + G, EINVAL, "too many pairs for one work list"),
    ("checkWorklist n_pairs=10 groups=0:0:0:100:0:100", EINVAL, "group 0: n_pairs must be 1..64"),
    (f"checkWorklist n_pairs=75 groups={G},65:10:0:100:0:100", EINVAL, "group 1: n_pairs must be 1..64"),
    (f"checkWorklist n_pairs=20 groups={G},10:11:0:100:0:100", EINVAL,
     "group 1: groups must partition the pair list in order"),
    ("checkWorklist n_pairs=10 groups=10:1:0:100:0:100", EINVAL, "group 0: groups must partition the pair list in order"),
    ("checkWorklist n_pairs=10 groups=10:0:100:100:100:100", EINVAL, "group 0: need from <= scan_from < scan_to <= to"),
    ("checkWorklist n_pairs=10 groups=10:0:5:100:4:100", EINVAL, "group 0: need from <= scan_from < scan_to <= to"),
    ("checkWorklist n_pairs=10 groups=10:0:0:100:50:50", EINVAL, "group 0: need from <= scan_from < scan_to <= to"),
    (f"checkWorklist n_pairs=20 groups={G},10:10:0:100:0:101", EINVAL, "group 1: need from <= scan_from < scan_to <= to"),
    (f"checkWorklist n_pairs=11 groups={G}", EINVAL, "groups cover 10 pairs, list has 11"),
    (f"checkWorklist n_pairs=9 groups={G}", EINVAL, "groups cover 10 pairs, list has 9"),
    # the order: the pair count, then group by group (count, place, window), then the cover
    ("checkWorklist n_pairs=4294967281 groups=0:0:0:100:0:100", EINVAL, "too many pairs for one work list"),
    ("checkWorklist n_pairs=10 groups=65:3:9:9:9:9", EINVAL, "group 0: n_pairs must be 1..64"),
    ("checkWorklist n_pairs=10 groups=10:3:9:9:9:9", EINVAL, "group 0: groups must partition the pair list in order"),
]


@pytest.mark.parametrize("cases", [DESC_CASES, WORKLIST_CASES], ids=["description", "worklist"])
def test_checks_give_the_codes_and_messages_of_the_entry_points(driver, cases):
    got = driver(*(case for case, _, _ in cases))
    for (case, code, why), line in zip(cases, got):
        assert line == ("rc=0" if code == 0 else f'rc={code} why="{why}"'), case


def test_header_is_free_of_the_device_runtime():
    """The builders build and do nothing else: the header names no runtime call, no environment, no context and no
    clock, and neither does the header of the constants it shares with the kernels."""
    for name in ("fsmc_model_tables.h", "fsmc_constants.h"):
        text = open(os.path.join(os.path.dirname(HEADER), name)).read()
        text = text.replace('#include "../../include/fastsmc_hip.h"', "")
        for word in ("hip", "getenv", "fsmc_ctx", "chrono", "KernelFn"):
            assert word not in text.replace("chip", ""), (name, word)
