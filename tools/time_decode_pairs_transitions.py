#!/usr/bin/env python3
"""fsmc_decode_pair_transitions (per pair and site, the posterior probability of a change of state from the site before,
downwards and upwards) timed through the C ABI against its neighbours over the same resident work list: the device time of
each call's kernels (fsmc_last_kernel_ms), the calls interleaved in one process -- the change probabilities with rows,
with bins only, fsmc_decode_pair_samples with one sample (one forward pass plus one walk), fsmc_decode_per_pair (one
decode; its MAP rows), and round again -- the median of --calls rounds after one warm-up round.

  default          the C1 shape: 300 haplotypes x 6760 sites, K = 69, all 44 850 pairs
  --pairs 4096     its first 4096 pairs

Usage: tools/time_decode_pairs_transitions.py [--haps 300 --sites 6760] [--pairs N] [--bins 10] [--chunk-sites C]
                                              [--calls 5] [--built-from TEXT]
One JSON line on stdout, stamped with the library's source hash.  `roofline_fraction`: the decode's algorithmic bytes (8 K + 0.25
a pair-site) at the HBM peak of 8.0e12 B/s over what was measured, as bench.py's headline."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HBM_PEAK = 8.0e12  # bytes a second, the roofline of bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--pairs", type=int, default=0, help="0 = all pairs of the cohort")
    ap.add_argument("--bins", type=int, default=10, help="equal bins over the sequence of the bins-only call")
    ap.add_argument("--chunk-sites", type=int, default=0, help="fsmc_ctx_set_chunk_sites (0 = automatic)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--built-from", default="", help="the commit the library was built from (free text)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fastsmc_amd import capi, synth
    from fastsmc_amd.build import hip_source_hash
    from oracle import oracle as O

    K = 69
    tables = synth.make_model_tables(K)
    haps = synth.make_haps(a.haps, a.sites, seed=1234)
    n_all = a.haps * (a.haps - 1) // 2
    n_pairs = a.pairs or n_all
    assert n_pairs <= n_all, "more pairs asked for than the cohort has"
    iy, ix = np.tril_indices(a.haps, -1)  # (y ascending, x < y ascending)
    pr = np.empty(n_pairs, capi.PAIR_DTYPE)
    pr["hap_a"], pr["hap_b"] = ix[:n_pairs].astype(np.uint32), iy[:n_pairs].astype(np.uint32)
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    gen = (haps.cm / 100.0).astype(np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=100, no_conditional_age_estimates=False)
    edges = np.linspace(0, pm.S, a.bins + 1).astype(np.int32)

    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    groups = capi.whole_sequence_groups(n_pairs, pm.S)
    ctx.upload_worklist(pr, groups)
    ctx.set_chunk_sites(a.chunk_sites)
    rows = (np.zeros((n_pairs, pm.S), np.float32), np.zeros((n_pairs, pm.S), np.float32), None, None)
    cells = (None, None, np.zeros((n_pairs, a.bins), np.float32), np.zeros((n_pairs, a.bins), np.float32))
    states = np.zeros((n_pairs, 1, pm.S), np.uint8)
    ms = {"transitions_rows": [], "transitions_bins": [], "samples_1": [], "per_pair": []}
    members, plan, slices = {}, {}, {}
    wall0 = time.perf_counter()
    for _ in range(a.calls + 1):  # (the first round is the warm-up)
        ctx.decode_pair_transitions(model, out=rows)
        ms["transitions_rows"].append(ctx.last_kernel_ms())
        info = ctx.info()
        members["transitions"], slices["rows"] = ctx.last_kernel(), ctx.last_pair_transitions_slices()
        plan = {"chunk_sites": info["chunk_sites"], "max_chunks": info["max_chunks"], "slots": info["n_slots"]}
        ctx.decode_pair_transitions(model, bin_edges=edges, out=cells)
        ms["transitions_bins"].append(ctx.last_kernel_ms())
        slices["bins"] = ctx.last_pair_transitions_slices()
        ctx.decode_pair_samples(model, 1, 0, out=states)
        ms["samples_1"].append(ctx.last_kernel_ms())
        members["samples"] = ctx.last_kernel()
        _, mp = ctx.decode_per_pair(model, pm.exp_times, want_mean=False)
        ms["per_pair"].append(ctx.last_kernel_ms())
        members["per_pair"] = ctx.last_kernel()
        del mp
    wall = time.perf_counter() - wall0
    ctx.close()
    down, up = rows[0], rows[1]
    assert np.isfinite(down).all() and np.isfinite(up).all() and (down >= 0).all() and (up >= 0).all()
    assert not down[:, 0].any() and not up[:, 0].any()
    med = {k: statistics.median(v[1:]) for k, v in ms.items()}
    ideal_ms = n_pairs * pm.S * (8 * K + 0.25) / HBM_PEAK * 1e3
    rec = {"config": "decode_pairs_transitions", "haplotypes": a.haps, "sites": a.sites, "K": K, "pairs": n_pairs,
           "bins": a.bins, "groups": int(groups.size), "calls": a.calls, "lib_hash": hip_source_hash(),
           "built_from": a.built_from, "members": members, "slices": slices, "plan": plan, "kernel_ms_calls": ms,
           "kernel_ms_median": med,
           "ratio_to_samples_1": med["transitions_rows"] / med["samples_1"],
           "ratio_to_per_pair": med["transitions_rows"] / med["per_pair"],
           "bins_only_over_rows": med["transitions_bins"] / med["transitions_rows"],
           "roofline_ms": ideal_ms, "roofline_fraction": ideal_ms / med["transitions_rows"],
           "pair_sites_per_s": n_pairs * pm.S / (med["transitions_rows"] / 1e3),
           "expected_changes_per_pair": {"down": float(down.sum(axis=1, dtype=np.float64).mean()),
                                         "up": float(up.sum(axis=1, dtype=np.float64).mean())},
           "bin_checksum": float(cells[2].sum(dtype=np.float64) + cells[3].sum(dtype=np.float64)),
           "row_checksum": float(down.sum(dtype=np.float64) + up.sum(dtype=np.float64)),
           "wall_s_all_rounds": wall}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
