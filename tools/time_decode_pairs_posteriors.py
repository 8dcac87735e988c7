#!/usr/bin/env python3
"""ASMC.decodePairs with per-pair posteriors and / or their sum over pairs, timed through the product path on files of
the C1 shape (300 haplotypes x 6760 sites, K = 69): wall time of the call (median of --calls calls after one warm-up)
and, for the same pairs through the C ABI, the device time of the call's kernels (fsmc_last_kernel_ms).  Runs against
any tree of this project (--tree: the directory that holds fastsmc_amd/), so that two builds are measured by one script;
a tree without fsmc_decode_pair_posteriors is timed on what its host path calls instead (fsmc_decode_posteriors).

Usage: tools/time_decode_pairs_posteriors.py --case sum|rows|both --pairs N [--calls 5] [--tree DIR] [--built-from TEXT]
One JSON line per case on stdout, stamped with the library's source hash."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["sum", "rows", "both"], required=True)
    ap.add_argument("--pairs", type=int, required=True)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--built-from", default="", help="the commit the tree's library was built from (free text)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from fastsmc_amd import api, capi, synth
    from fastsmc_amd.build import hip_source_hash
    from oracle import oracle as O

    want_rows, want_sum = a.case in ("rows", "both"), a.case in ("sum", "both")
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(a.haps, a.sites, seed=1234)
    all_pairs = [(x, y) for y in range(a.haps) for x in range(y)][:a.pairs]
    assert len(all_pairs) == a.pairs, "more pairs asked for than the cohort has"
    ha, hb = [p[0] for p in all_pairs], [p[1] for p in all_pairs]
    rec = {"config": "decode_pairs_posteriors", "case": a.case, "haplotypes": a.haps, "sites": a.sites, "K": 69,
           "pairs": a.pairs, "calls": a.calls, "lib_hash": hip_source_hash(), "built_from": a.built_from,
           "has_fsmc_decode_pair_posteriors": hasattr(capi.Context, "decode_pair_posteriors")}
    with tempfile.TemporaryDirectory() as d:
        root = os.path.join(d, "syn")
        synth.write_haps_files(root, haps, fastsmc_map=False)
        gen = (haps.cm / 100.0).astype(np.float32)
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
        asmc = api.ASMC(p)
        walls = []
        for call in range(a.calls + 1):  # (the first is the warm-up)
            t0 = time.perf_counter()
            asmc.decodePairs(ha, hb, want_rows, want_sum, False, False)
            walls.append(time.perf_counter() - t0)
        res = asmc.get_copy_of_results()
        if want_sum:
            rec["sum_checksum"] = float(np.float64(np.asarray(res.sum_of_posteriors).sum()))
        if want_rows:
            rec["last_row_checksum"] = float(np.float64(np.asarray(res.per_pair_posteriors[a.pairs - 1]).sum()))
        del res, asmc
    # (peak resident set of the process after the product-path calls, before the C-ABI part below; Linux: kilobytes)
    rec["peak_rss_bytes_product_path"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    rec["wall_s_warmup"] = walls[0]
    rec["wall_s_calls"] = walls[1:]
    rec["wall_s_median"] = statistics.median(walls[1:])

    # the same pairs through the C ABI: device time of the call's kernels
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=p.time, no_conditional_age_estimates=False)
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    ctx.upload_worklist(np.array(all_pairs, dtype=np.uint32).view(capi.PAIR_DTYPE).reshape(-1),
                        capi.whole_sequence_groups(a.pairs, pm.S))
    kms = []
    for call in range(3):
        if rec["has_fsmc_decode_pair_posteriors"]:
            acc = np.zeros((pm.K, pm.S), np.float32) if want_sum else None
            if want_rows and call == 0:
                out_rows = [np.empty(pm.K * pm.S, np.float32) for _ in range(a.pairs)]
            ctx.decode_pair_posteriors(model, pm.exp_times, want_rows=want_rows, sum_into=acc,
                                       rows_out=out_rows if want_rows else None)
            rec["slices"] = ctx.last_pair_posterior_slices()
        else:
            ctx.decode_posteriors(model)
        kms.append(ctx.last_kernel_ms())
    ctx.close()
    rec["kernel_ms_calls"] = kms
    rec["kernel_ms"] = min(kms[1:])
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
