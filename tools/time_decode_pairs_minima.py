#!/usr/bin/env python3
"""ASMC.decodePairs for the per-site minima of posterior mean and MAP (min_posterior_means, argmin_posterior_means,
min_MAPs, argmin_MAPs), timed through the product path on files of the C1 shape (300 haplotypes x 6760 sites, K = 69):
wall time of the call (median of --calls calls after one warm-up) and the peak resident set of the process, then, for
the same pairs through the C ABI, the device time of the call's kernels (fsmc_last_kernel_ms).

  --case rows   the minima as a by-product of per_pair_posterior_means=True, per_pair_MAPs=True: every pair's rows cross
                the bus and finaliseCalculations walks them (the only way a tree without fsmc_decode_pair_minima has)
  --case min    min_posterior_means=True, min_MAPs=True: the minima alone, reduced on the device

Runs against any tree of this project (--tree: the directory that holds fastsmc_amd/), so that two builds are measured
by one script.  --abi-only skips the product path (no input files are written: cohorts whose files take minutes to
write) and times the C ABI call itself.

Usage: tools/time_decode_pairs_minima.py --case rows|min --pairs N [--calls 5] [--haps 300 --sites 6760] [--abi-only]
                                         [--tree DIR] [--built-from TEXT]
One JSON line on stdout, stamped with the library's source hash; the checksums of the four vectors let the lines of two
builds and two cases be compared."""
import argparse
import copy
import json
import os
import resource
import statistics
import sys
import tempfile
import time

import numpy as np


def checksums(min_mean, argmin_mean, min_map, argmin_map):
    return {"min_mean_sum": float(np.asarray(min_mean, np.float64).sum()),
            "argmin_mean_sum": int(np.asarray(argmin_mean, np.int64).sum()),
            "min_map_sum": int(np.asarray(min_map, np.int64).sum()),
            "argmin_map_sum": int(np.asarray(argmin_map, np.int64).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["rows", "min"], required=True)
    ap.add_argument("--pairs", type=int, required=True)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--abi-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--built-from", default="", help="the commit the tree's library was built from (free text)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from fastsmc_amd import api, capi, synth
    from fastsmc_amd.build import hip_source_hash
    from oracle import oracle as O

    has_minima = hasattr(capi.Context, "decode_pair_minima")
    if a.case == "min" and not has_minima:
        sys.exit("this tree has no fsmc_decode_pair_minima: only --case rows can be timed on it")
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(a.haps, a.sites, seed=1234)
    all_pairs = [(x, y) for y in range(a.haps) for x in range(y)][:a.pairs]
    assert len(all_pairs) == a.pairs, "more pairs asked for than the cohort has"
    ha, hb = [p[0] for p in all_pairs], [p[1] for p in all_pairs]
    rec = {"config": "decode_pairs_minima", "case": a.case, "haplotypes": a.haps, "sites": a.sites, "K": 69,
           "pairs": a.pairs, "calls": a.calls, "lib_hash": hip_source_hash(), "built_from": a.built_from,
           "has_fsmc_decode_pair_minima": has_minima, "abi_only": a.abi_only}
    gen = (haps.cm / 100.0).astype(np.float32)
    time_param = 100
    if not a.abi_only:
        with tempfile.TemporaryDirectory() as d:
            root = os.path.join(d, "syn")
            synth.write_haps_files(root, haps, fastsmc_map=False)
            gen32 = np.array([np.float32(np.float32(c) / np.float32(100.0)) for c in haps.cm], np.float32)
            used = np.unique(np.concatenate([[0.0], O.step_rows(tables.keys, gen)[1][1:],
                                             O.step_rows(tables.keys, gen32)[1][1:]]))
            t = copy.copy(tables)
            sel = np.nonzero(np.isin(t.keys, used.astype(np.float32)))[0]
            t.keys, t.D, t.B, t.U, t.RR = t.keys[sel], t.D[sel], t.B[sel], t.U[sel], t.RR[sel]
            synth.write_decoding_quantities(root + ".decodingQuantities.gz", t)
            p = api.DecodingParams(root, root + ".decodingQuantities.gz", root, 1, 1, "array", False, True, False, False,
                                   0.0, False, True, False, "", False, True)
            p.useKnownSeed = True
            time_param = p.time
            asmc = api.ASMC(p)
            walls = []
            for call in range(a.calls + 1):  # (the first is the warm-up)
                t0 = time.perf_counter()
                if a.case == "rows":
                    asmc.decodePairs(ha, hb, False, False, True, True)
                else:
                    asmc.decodePairs(ha, hb, min_posterior_means=True, min_MAPs=True)
                walls.append(time.perf_counter() - t0)
            res = asmc.get_ref_of_results()
            rec["product_path"] = checksums(res.min_posterior_means, res.argmin_posterior_means, res.min_MAPs,
                                            res.argmin_MAPs)
            rec["rows_held"] = int(np.asarray(res.per_pair_posterior_means).shape[0])
            del res, asmc
        rec["wall_s_warmup"] = walls[0]
        rec["wall_s_calls"] = walls[1:]
        rec["wall_s_median"] = statistics.median(walls[1:])
        # (peak resident set of the process after the product-path calls, before the C-ABI part below; Linux: kilobytes)
        rec["peak_rss_bytes_product_path"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024

    # the same pairs through the C ABI: device time of the call's kernels
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=time_param, no_conditional_age_estimates=False)
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    ctx.upload_worklist(np.array(all_pairs, dtype=np.uint32).view(capi.PAIR_DTYPE).reshape(-1),
                        capi.whole_sequence_groups(a.pairs, pm.S))
    rec["peak_rss_bytes_before_abi_calls"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    kms, abi_walls = [], []
    for call in range(3):
        t0 = time.perf_counter()
        if a.case == "min":
            got = ctx.decode_pair_minima(model, pm.exp_times)
            rec["slices"] = ctx.last_pair_minima_slices()
            if call == 2:
                rec["c_abi"] = checksums(*got)
        else:
            mean, mp = ctx.decode_per_pair(model, pm.exp_times)
            del mean, mp
        abi_walls.append(time.perf_counter() - t0)
        kms.append(ctx.last_kernel_ms())
    rec["member"], rec["waves_per_window"] = ctx.last_kernel(), ctx.last_waves_per_window()
    ctx.close()
    rec["kernel_ms_calls"] = kms
    rec["kernel_ms"] = min(kms[1:])
    rec["abi_wall_s_calls"] = abi_walls
    rec["peak_rss_bytes_after_abi_calls"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
