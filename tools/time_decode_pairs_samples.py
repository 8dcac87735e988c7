#!/usr/bin/env python3
"""fsmc_decode_pair_samples (per pair, state paths drawn from the joint posterior: forward filtering with backward
sampling) timed through the C ABI against the other routes over the same resident work list: the device time of each
call's kernels (fsmc_last_kernel_ms), the calls interleaved in one process -- sampled paths, fsmc_decode_pair_loglik (the
forward kernel: the sampler's first sweep without its rows), fsmc_decode_per_pair (its MAP rows), and round again -- the
median of --calls rounds after one warm-up round.

  default                                  the C1 shape: 300 haplotypes x 6760 sites, K = 69, all 44 850 pairs
  --haps 1000 --sites 50000 --pairs 40000  the C2 shape, its first 40 000 pairs

fsmc_decode_per_pair hands [pairs][sites] int32 rows to the host; it is left out (and said so in the line) where they
would take more than --rows-limit-gb of host memory.

Usage: tools/time_decode_pairs_samples.py [--haps 300 --sites 6760] [--pairs N] [--samples 1] [--seed 0]
                                          [--chunk-sites C] [--calls 5] [--built-from TEXT]
One JSON line on stdout, stamped with the library's source hash; `ratio_to_loglik` and `ratio_to_per_pair` are the
medians' ratios.  The derived expectation: one forward sweep with whole sequences and two in chunks, each with a 4 K-byte
row stored a pair-site, and a walk of about 8 vector instructions a state, sample and site against the forward step's
13."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--pairs", type=int, default=0, help="0 = all pairs of the cohort")
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--chunk-sites", type=int, default=0, help="fsmc_ctx_set_chunk_sites (0 = automatic)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows-limit-gb", type=float, default=10.0)
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
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    gen = (haps.cm / 100.0).astype(np.float32)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=100, no_conditional_age_estimates=False)
    with_rows = 4.0 * n_pairs * pm.S <= a.rows_limit_gb * 2.0 ** 30

    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    groups = capi.whole_sequence_groups(n_pairs, pm.S)
    ctx.upload_worklist(pr, groups)
    ctx.set_chunk_sites(a.chunk_sites)
    out = np.zeros((n_pairs, a.samples, pm.S), np.uint8)
    ms = {"samples": [], "loglik": [], "per_pair": []}
    members, plan = {}, {}
    wall0 = time.perf_counter()
    for call in range(a.calls + 1):  # (the first round is the warm-up)
        ctx.decode_pair_samples(model, a.samples, a.seed, out=out)
        ms["samples"].append(ctx.last_kernel_ms())
        info = ctx.info()
        members["samples"], slices = ctx.last_kernel(), ctx.last_pair_samples_slices()
        plan = {"chunk_sites": info["chunk_sites"], "max_chunks": info["max_chunks"], "slots": info["n_slots"]}
        ctx.decode_pair_loglik(model)
        ms["loglik"].append(ctx.last_kernel_ms())
        members["loglik"] = ctx.last_kernel()
        if with_rows:
            _, mp = ctx.decode_per_pair(model, pm.exp_times, want_mean=False)
            ms["per_pair"].append(ctx.last_kernel_ms())
            members["per_pair"] = ctx.last_kernel()
            if call == a.calls:
                differ = float((mp != out[:, 0]).mean())  # (marginal argmax against a drawn path: a description, no check)
            del mp
    wall = time.perf_counter() - wall0
    ctx.close()
    assert (out < pm.K).all()
    changes = (out[:, :, 1:] != out[:, :, :-1]).sum(axis=2)
    med = {k: statistics.median(v[1:]) for k, v in ms.items() if v}
    rec = {"config": "decode_pairs_samples", "haplotypes": a.haps, "sites": a.sites, "K": 69, "pairs": n_pairs,
           "samples": a.samples, "seed": a.seed, "groups": int(groups.size), "calls": a.calls,
           "lib_hash": hip_source_hash(), "built_from": a.built_from, "members": members, "slices": slices, "plan": plan,
           "kernel_ms_calls": ms, "kernel_ms_median": med,
           "ratio_to_loglik": med["samples"] / med["loglik"],
           "ratio_to_per_pair": med["samples"] / med["per_pair"] if with_rows else None,
           "per_pair_left_out": not with_rows,
           "pair_sites_per_s": n_pairs * pm.S / (med["samples"] / 1e3),
           "sample_sites_per_s": n_pairs * a.samples * pm.S / (med["samples"] / 1e3),
           "state_changes_per_sample_mean": float(changes.mean()),
           "state_checksum": int(out.astype(np.uint64).sum()),
           "sites_where_map_differs": differ if with_rows else None,
           "wall_s_all_rounds": wall}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
