"""What the tests of the fsmc_decode_pair_* entry points and of ASMC.decodePairs share: the work list of a pair list, a
context on the standard problem, other models, and the cohorts of the product path as files."""
import copy
import gzip
import os
import shutil

import numpy as np

from fastsmc_amd import api, capi, synth
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pairs_array(pairs):
    return np.array(pairs, dtype=np.uint32).view(capi.PAIR_DTYPE).reshape(-1)


def upload(ctx, pm, pairs):
    ctx.upload_worklist(pairs_array(pairs), capi.whole_sequence_groups(len(pairs), pm.S))


def open_context(small_problem):
    ctx = capi.Context(0)
    model = ctx.create_model(small_problem["model"])
    ctx.upload_haps(small_problem["bits"], small_problem["model"].S)
    return ctx, model


def gpu_context(small_problem):
    """The body of a module's `gpu` fixture: `yield from gpu_context(small_problem)`."""
    ctx, model = open_context(small_problem)
    yield ctx, model
    ctx.close()


def problem(K, n_hap=64, S=200, seed=11):
    tables = synth.make_model_tables(K)
    haps = synth.make_haps(n_hap, S, seed=seed, cm_per_mb=25.0, switch_per_cm=0.6)
    bits, derived, flipped = synth.fold_and_pack(haps.alleles)
    folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
    gen = (haps.cm / 100.0).astype(np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, n_hap, time=200)
    return pm, bits, folded


def posterior_tables(pm, folded, pairs, acc=None):
    """(rows [n][K][S], acc): the oracle's tables of `pairs`, its sum continued in `acc` (a new zero array if None)."""
    acc = np.zeros((pm.K, pm.S), np.float32) if acc is None else acc
    rows = []
    for b0 in range(0, len(pairs), 64):
        chunk = pairs[b0:b0 + 64]
        ob = np.stack([folded[a] ^ folded[b] for a, b in chunk])
        hb = np.stack([folded[a] & folded[b] for a, b in chunk])
        post, _ = O.decode_batch(pm, ob, hb, 0, pm.S)
        _, _, pp = O.per_pair_output(pm, post, len(chunk), want_post=True, sum_of_post=acc)
        rows.append(pp)
    return np.concatenate(rows), acc


# ---------------------------------------------------------------- the product path: ASMC.decodePairs

N_HAP, SITES, N_PAIRS = 64, 700, 200
EDGES_700 = [5, 70, 71, 100, 400, 699]


def cohort_files(tmp_path):
    """A synthetic cohort of 64 haplotypes x 700 sites (not a multiple of 64) as files, with the 69-state decoding
    quantities restricted to the rows its map uses; returns (root, tables, haps, derived, folded)."""
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(N_HAP, SITES, seed=17, cm_per_mb=25.0, switch_per_cm=0.6)
    _, derived, flipped = synth.fold_and_pack(haps.alleles)
    folded = np.where(flipped[None, :], 1 - haps.alleles, haps.alleles).astype(np.uint8)
    root = str(tmp_path / "cohort")
    synth.write_haps_files(root, haps, fastsmc_map=False)
    gen_file = np.array([np.float32(np.float32(c) / np.float32(100.0)) for c in haps.cm], np.float32)
    gen_synth = (haps.cm / 100.0).astype(np.float32)
    t = copy.copy(tables)
    used = np.unique(np.concatenate([[0.0], O.step_rows(t.keys, gen_file)[1][1:], O.step_rows(t.keys, gen_synth)[1][1:]]))
    sel = np.nonzero(np.isin(t.keys, used.astype(np.float32)))[0]
    t.keys, t.D, t.B, t.U, t.RR = t.keys[sel], t.D[sel], t.B[sel], t.U[sel], t.RR[sel]
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", t)
    return root, tables, haps, derived, folded


def cohort_pairs():
    """The 200 pairs the product-path tests decode on the cohort, as (pairs, a, b)."""
    rng = np.random.default_rng(5)
    all_pairs = [(x, y) for x in range(N_HAP) for y in range(x + 1, N_HAP)]
    pairs = [all_pairs[i] for i in rng.choice(len(all_pairs), N_PAIRS, replace=False)]
    return pairs, [int(x) for x, _ in pairs], [int(y) for _, y in pairs]


def example_files(tmp_path):
    """The reference's exampleFile.n300.array.{hap.gz,map.gz,samples} (tests/golden) under a root of their own, with the
    synthetic 69-state decoding quantities restricted to the rows this map uses; returns (root, the map's centimorgans)."""
    root = str(tmp_path / "exampleFile.n300.array")
    for ext in (".hap.gz", ".map.gz", ".samples"):
        shutil.copy(os.path.join(GOLD, "exampleFile.n300.array" + ext), root + ext)
    cm = [float(line.split()[2]) for line in gzip.open(root + ".map.gz", "rt")]
    gen = np.array([np.float32(np.float32(c) / np.float32(100.0)) for c in cm], np.float32)  # (Data.cpp:186)
    t = copy.copy(synth.make_model_tables(69))
    used = np.unique(np.concatenate([[0.0], O.step_rows(t.keys, gen)[1][1:]]))
    sel = np.nonzero(np.isin(t.keys, used.astype(np.float32)))[0]
    t.keys, t.D, t.B, t.U, t.RR = t.keys[sel], t.D[sel], t.B[sel], t.U[sel], t.RR[sel]
    synth.write_decoding_quantities(root + ".decodingQuantities.gz", t)
    return root, np.array(cm)


def params(root):
    p = api.DecodingParams(root, root + ".decodingQuantities.gz", root, 1, 1, "array", False, True, False, False, 0.0,
                           False, True, False, "", False, True)
    p.useKnownSeed = True
    return p


def asmc(root):
    return api.ASMC(params(root))
