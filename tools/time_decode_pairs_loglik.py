#!/usr/bin/env python3
"""fsmc_decode_pair_loglik (per-pair likelihoods from the forward sweep alone) timed through the C ABI against the full
decodes of the same resident work list: the device time of each call's kernels (fsmc_last_kernel_ms), the three calls
interleaved in one process -- log-likelihoods, fsmc_decode_ibd, fsmc_decode_per_pair, and round again -- the median of
--calls rounds after one warm-up round.

  default           the C1 shape: 300 haplotypes x 6760 sites, K = 69, all 44 850 pairs
  --haps 1000 --sites 50000    the C2 shape, all 499 500 pairs: a chip-filling list (7 805 groups through a launch of 2 048 waves)
  --bins 64 | one | cm:<width> | none    the bin outputs as well: bins of 64 sites, one bin, windows of <width> cM

fsmc_decode_per_pair hands [pairs][sites] rows to the host; it is left out (and said so in the line) where the two
matrices would take more than --rows-limit-gb of host memory, as on the C2 shape.

Usage: tools/time_decode_pairs_loglik.py [--haps 300 --sites 6760] [--pairs N] [--bins none] [--calls 5]
                                         [--built-from TEXT]
One JSON line on stdout, stamped with the library's source hash; `ratio_to_ibd` and `ratio_to_per_pair` are the medians'
ratios, the expectation (one alpha step a site against an alpha step, about 1.5 beta steps and a combine) well under 0.5."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def make_edges(spec, cm):
    S = len(cm)
    if spec == "none":
        return None
    if spec == "one":
        return np.array([0, S], np.int32)
    if spec.startswith("cm:"):
        w = np.floor((np.asarray(cm, np.float64) - cm[0]) / float(spec[3:]))
        return np.concatenate([[0], np.nonzero(np.diff(w))[0] + 1, [S]]).astype(np.int32)
    return np.unique(np.concatenate([np.arange(0, S, int(spec)), [S]])).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--pairs", type=int, default=0, help="0 = all pairs of the cohort")
    ap.add_argument("--bins", default="none")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows-limit-gb", type=float, default=4.0)
    ap.add_argument("--built-from", default="", help="the commit the library was built from (free text)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fastsmc_amd import capi, synth
    from fastsmc_amd.build import hip_source_hash
    from oracle import oracle as O

    tables = synth.make_model_tables(69)
    haps = synth.make_haps(a.haps, a.sites, seed=1234)
    n_all = a.haps * (a.haps - 1) // 2
    n_pairs = a.pairs or n_all
    assert n_pairs <= n_all, "more pairs asked for than the cohort has"
    iy, ix = np.tril_indices(a.haps, -1)  # (y ascending, x < y ascending)
    pr = np.empty(n_pairs, capi.PAIR_DTYPE)
    pr["hap_a"], pr["hap_b"] = ix[:n_pairs].astype(np.uint32), iy[:n_pairs].astype(np.uint32)
    edges = make_edges(a.bins, haps.cm)
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    gen = (haps.cm / 100.0).astype(np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=100, no_conditional_age_estimates=False)
    with_rows = 8.0 * n_pairs * pm.S <= a.rows_limit_gb * 2.0 ** 30

    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    groups = capi.whole_sequence_groups(n_pairs, pm.S)
    ctx.upload_worklist(pr, groups)
    ms = {"loglik": [], "ibd": [], "per_pair": []}
    members = {}
    wall0 = time.perf_counter()
    for call in range(a.calls + 1):  # (the first round is the warm-up)
        got = ctx.decode_pair_loglik(model, edges)
        ms["loglik"].append(ctx.last_kernel_ms())
        members["loglik"], slices, slots = ctx.last_kernel(), ctx.last_pair_loglik_slices(), ctx.info()["n_slots"]
        ctx.decode_ibd_launch(model)
        n_records = int(ctx.decode_ibd_fetch().size)
        ms["ibd"].append(ctx.last_kernel_ms())
        members["ibd"] = ctx.last_kernel()
        if with_rows:
            mean, mp = ctx.decode_per_pair(model, pm.exp_times)
            ms["per_pair"].append(ctx.last_kernel_ms())
            members["per_pair"] = ctx.last_kernel()
            del mean, mp
    wall = time.perf_counter() - wall0
    ctx.close()
    ll = capi.log_likelihood(got[0], got[1])
    med = {k: statistics.median(v[1:]) for k, v in ms.items() if v}
    rec = {"config": "decode_pairs_loglik", "haplotypes": a.haps, "sites": a.sites, "K": 69, "pairs": n_pairs,
           "groups": int(groups.size), "bins": a.bins, "n_bins": 0 if edges is None else int(edges.size - 1),
           "calls": a.calls, "lib_hash": hip_source_hash(), "built_from": a.built_from, "members": members,
           "slices": slices, "slots": slots, "kernel_ms_calls": ms, "kernel_ms_median": med,
           "ratio_to_ibd": med["loglik"] / med["ibd"],
           "ratio_to_per_pair": med["loglik"] / med["per_pair"] if with_rows else None,
           "per_pair_left_out": not with_rows, "ibd_records": n_records,
           "pair_sites_per_s": n_pairs * pm.S / (med["loglik"] / 1e3),
           "log_likelihood_sum": float(ll.sum()), "exponent_sum": int(np.asarray(got[1], np.int64).sum()),
           "wall_s_all_rounds": wall}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
