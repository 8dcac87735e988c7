#!/usr/bin/env python3
"""ASMC.decodePairs for per-pair summaries over bins of sites (bin_mean_posterior_means, bin_min_posterior_means,
bin_argmin_posterior_means, bin_min_MAPs, bin_argmin_MAPs), timed through the product path on files of the C1 shape
(300 haplotypes x 6760 sites, K = 69): wall time of the call (median of --calls calls after one warm-up) and the peak
resident set of the process, then, for the same pairs through the C ABI, the device time of the call's kernels
(fsmc_last_kernel_ms) against fsmc_decode_per_pair alone.

  --case rows   per_pair_posterior_means=True, per_pair_MAPs=True and the reduction of the rows by numpy
                (tests/pair_bins_lists.py): the only way a tree without fsmc_decode_pair_bins has.  The wall time is the
                call plus the reduction; both are also given apart.
  --case bins   site_bins=<edges> alone: reduced on the device, no rows on the host
  --bins 64 | one | cm:<width>    bins of 64 sites (the last one shorter), one bin over all sites, or windows of <width>
                cM (api.site_bins; --case rows cuts the same windows with numpy)

Runs against any tree of this project (--tree: the directory that holds fastsmc_amd/), so that two builds are measured
by one script.  --abi-only skips the product path (no input files are written: cohorts whose files take minutes to
write) and times the C ABI call itself: with --haps 1000 --sites 50000 --pairs 499500 --bins cm:1 the call no tree
could make before (the C2 shape, all pairs); its line carries the slices, the pair-sites per second and the fraction of
the HBM roofline by bench.py's count of algorithmic bytes.

Usage: tools/time_decode_pairs_bins.py --case rows|bins --pairs N [--bins 64] [--calls 5] [--haps 300 --sites 6760]
                                       [--abi-only] [--tree DIR] [--built-from TEXT]
One JSON line on stdout, stamped with the library's source hash; the checksums of the five matrices let the lines of two
builds and two cases be compared."""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

HBM_PEAK = 8.0e12  # B/s, as bench.py


def checksums(five):
    names = ("bin_mean_sum", "bin_min_mean_sum", "bin_argmin_mean_sum", "bin_min_map_sum", "bin_argmin_map_sum")
    return {n: (float(np.asarray(a, np.float64).sum()) if np.asarray(a).dtype.kind == "f"
                else int(np.asarray(a, np.int64).sum())) for n, a in zip(names, five)}


def peak_rss():
    for line in open("/proc/self/status"):
        if line.startswith("VmHWM:"):
            return int(line.split()[1]) * 1024
    return None


def make_edges(spec, cm):
    S = len(cm)
    if spec == "one":
        return np.array([0, S], np.int32)
    if spec.startswith("cm:"):
        width = float(spec[3:])
        w = np.floor((np.asarray(cm, np.float64) - cm[0]) / width)
        return np.concatenate([[0], np.nonzero(np.diff(w))[0] + 1, [S]]).astype(np.int32)
    step = int(spec)
    return np.unique(np.concatenate([np.arange(0, S, step), [S]])).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["rows", "bins"], required=True)
    ap.add_argument("--pairs", type=int, required=True)
    ap.add_argument("--bins", default="64")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--abi-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--built-from", default="", help="the commit the tree's library was built from (free text)")
    a = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(here, "tests"))  # (pair_bins_lists: the numpy statement, from THIS tree)
    sys.path.insert(0, os.path.abspath(a.tree))
    from fastsmc_amd import api, capi, synth
    from fastsmc_amd.build import hip_source_hash
    from oracle import oracle as O
    import pair_bins_lists as BL

    has_bins = hasattr(capi.Context, "decode_pair_bins")
    if a.case == "bins" and not has_bins:
        sys.exit("this tree has no fsmc_decode_pair_bins: only --case rows can be timed on it")
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(a.haps, a.sites, seed=1234)
    if a.pairs == a.haps * (a.haps - 1) // 2:
        iy, ix = np.tril_indices(a.haps, -1)  # (y ascending, x < y ascending: the order of the list below)
        ha, hb = ix.astype(np.uint32), iy.astype(np.uint32)
    else:
        all_pairs = [(x, y) for y in range(a.haps) for x in range(y)][:a.pairs]
        assert len(all_pairs) == a.pairs, "more pairs asked for than the cohort has"
        ha, hb = np.array([p[0] for p in all_pairs], np.uint32), np.array([p[1] for p in all_pairs], np.uint32)
    edges = make_edges(a.bins, haps.cm)
    rec = {"config": "decode_pairs_bins", "case": a.case, "bins": a.bins, "n_bins": int(edges.size - 1),
           "haplotypes": a.haps, "sites": a.sites, "K": 69, "pairs": a.pairs, "calls": a.calls,
           "lib_hash": hip_source_hash(), "built_from": a.built_from, "has_fsmc_decode_pair_bins": has_bins,
           "abi_only": a.abi_only}
    gen = (haps.cm / 100.0).astype(np.float32)
    time_param = 100
    if not a.abi_only:
        la, lb = [int(x) for x in ha], [int(x) for x in hb]
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
            if a.case == "bins" and a.bins.startswith("cm:"):
                assert np.array_equal(api.site_bins(haps.cm, float(a.bins[3:])), edges)
            walls, decode_s, reduce_s = [], [], []
            five = None
            for call in range(a.calls + 1):  # (the first is the warm-up)
                t0 = time.perf_counter()
                if a.case == "rows":
                    asmc.decodePairs(la, lb, False, False, True, True)
                    t1 = time.perf_counter()
                    res = asmc.get_ref_of_results()
                    five = BL.expected(np.asarray(res.per_pair_posterior_means), np.asarray(res.per_pair_MAPs), edges)
                    del res
                    decode_s.append(t1 - t0)
                    reduce_s.append(time.perf_counter() - t1)
                else:
                    asmc.decodePairs(la, lb, site_bins=edges)
                walls.append(time.perf_counter() - t0)
            res = asmc.get_ref_of_results()
            if a.case == "bins":
                five = (res.bin_mean_posterior_means, res.bin_min_posterior_means, res.bin_argmin_posterior_means,
                        res.bin_min_MAPs, res.bin_argmin_MAPs)
            rec["product_path"] = checksums(five)
            rec["rows_held"] = int(np.asarray(res.per_pair_posterior_means).shape[0])
            del res, asmc, five
        rec["wall_s_warmup"] = walls[0]
        rec["wall_s_calls"] = walls[1:]
        rec["wall_s_median"] = statistics.median(walls[1:])
        if decode_s:
            rec["decode_s_median"] = statistics.median(decode_s[1:])
            rec["numpy_reduction_s_median"] = statistics.median(reduce_s[1:])
        # (peak resident set of the process after the product-path calls, before the C-ABI part below)
        rec["peak_rss_bytes_product_path"] = peak_rss()

    # the same pairs through the C ABI: device time of the call's kernels
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=time_param, no_conditional_age_estimates=False)
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    pr = np.empty(a.pairs, capi.PAIR_DTYPE)
    pr[capi.PAIR_DTYPE.names[0]], pr[capi.PAIR_DTYPE.names[1]] = ha, hb
    ctx.upload_worklist(pr, capi.whole_sequence_groups(a.pairs, pm.S))
    kms, abi_walls = [], []
    n_calls = 2 if a.abi_only and a.pairs > 100000 else 3
    for call in range(n_calls):
        t0 = time.perf_counter()
        if a.case == "bins":
            got = ctx.decode_pair_bins(model, pm.exp_times, edges)
            rec["slices"] = ctx.last_pair_bins_slices()
            if call == n_calls - 1:
                rec["c_abi"] = checksums(got)
            del got
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
    rec["pair_sites_per_s"] = a.pairs * pm.S / (rec["kernel_ms"] / 1e3)
    # bench.py's algorithmic bytes of the decode (8 K + 0.25 a pair-site) over the span, against the HBM peak
    rec["roofline_frac"] = a.pairs * pm.S * (8 * pm.K + 0.25) / (rec["kernel_ms"] / 1e3) / HBM_PEAK
    rec["peak_rss_bytes_after_abi_calls"] = peak_rss()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
