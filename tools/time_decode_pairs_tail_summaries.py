#!/usr/bin/env python3
"""ASMC.decodePairs for the tail probabilities reduced over pairs and site bins (sum_of_tail_probabilities,
per_pair_bin_tail_means, per_pair_bin_tail_lengths), timed through the product path on files of the C1 shape
(300 haplotypes x 6760 sites, K = 69) with four tail times: wall time of the call (median of --calls calls after one
warm-up) and the peak resident set of the process, then, through the C ABI, the device time of the call's kernels
(fsmc_last_kernel_ms) of fsmc_decode_pair_tail_summaries next to that of fsmc_decode_pair_cdf on the same work list.

  --route rows       tail_times=[...] alone and the reduction of the [4][pairs][S] rows by numpy on the host: the sum
                     over the pairs in float64, and per bin the mean and the weighted sum (np.add.reduceat in float64).
                     The only way a tree without fsmc_decode_pair_tail_summaries has.  The wall time is the call plus the
                     reduction; both are also given apart.
  --route summaries  tail_summary_times=[...], site_bins=..., site_weights=api.site_widths(map): reduced on the device,
                     no rows on the host.

One route a process (the peak resident set is the process's), so the two routes of a comparison are run in turn, A B A B,
on one box.  numpy's sums are in another order than the device's defined ones: the checksums of the two routes agree to
rounding, not to the bit (the bits are what tests/test_gpu_pair_tail.py is for).

Usage: tools/time_decode_pairs_tail_summaries.py --route rows|summaries --pairs N [--calls 5] [--haps 300 --sites 6760]
                                                 [--bin-cm 1.0] [--abi-only] [--abi-pairs N] [--built-from TEXT]
One JSON line on stdout, stamped with the library's source hash."""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

TIMES = [25.0, 50.0, 100.0, 200.0]


def peak_rss():
    for line in open("/proc/self/status"):
        if line.startswith("VmHWM:"):
            return int(line.split()[1]) * 1024
    return None


def checksums(tail_sum, bin_mean, bin_length):
    return {"tail_sum": float(np.asarray(tail_sum, np.float64).sum()),
            "bin_tail_mean": float(np.asarray(bin_mean, np.float64).sum()),
            "bin_tail_length": float(np.asarray(bin_length, np.float64).sum())}


def reduce_rows(rows, edges, w):
    """The host's way: rows [n_tail][pairs][S] float32 -> (sum over pairs float64, bin means, bin weighted sums)."""
    e = np.asarray(edges, np.int64)
    tail_sum = rows.sum(axis=1, dtype=np.float64)
    n_tail, n, _ = rows.shape
    mean = np.empty((n_tail, n, e.size - 1), np.float32)
    length = np.empty((n_tail, n, e.size - 1), np.float32)
    w64 = np.asarray(w, np.float64)
    widths = np.diff(e).astype(np.float64)
    for j in range(n_tail):
        for i0 in range(0, n, 1024):  # (a block of pairs at a time: the float64 copy stays small)
            x = rows[j, i0:i0 + 1024, :e[-1]].astype(np.float64)
            mean[j, i0:i0 + 1024] = np.add.reduceat(x, e[:-1], axis=1) / widths
            length[j, i0:i0 + 1024] = np.add.reduceat(x * w64[:e[-1]], e[:-1], axis=1)
    return tail_sum, mean, length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["rows", "summaries"], required=True)
    ap.add_argument("--pairs", type=int, required=True)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--bin-cm", type=float, default=1.0, help="width of the site bins in centimorgans")
    ap.add_argument("--abi-only", action="store_true")
    ap.add_argument("--abi-pairs", type=int, default=0, help="pairs of the C-ABI part; 0 = min(--pairs, 4096)")
    ap.add_argument("--built-from", default="", help="the commit the library was built from (free text)")
    a = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from fastsmc_amd import api, capi, synth
    from fastsmc_amd.build import hip_source_hash
    sys.path.insert(0, os.path.join(here, "tests"))
    from oracle import oracle as O

    has_entry = hasattr(capi.Context, "decode_pair_tail_summaries")
    if a.route == "summaries" and not has_entry:
        sys.exit("this tree has no fsmc_decode_pair_tail_summaries: only --route rows can be timed on it")
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(a.haps, a.sites, seed=1234)
    all_pairs = [(x, y) for y in range(a.haps) for x in range(y)][:a.pairs]
    assert len(all_pairs) == a.pairs, "more pairs asked for than the cohort has"
    ha, hb = np.array([p[0] for p in all_pairs], np.uint32), np.array([p[1] for p in all_pairs], np.uint32)
    cuts = api.tail_states(tables.discretization, TIMES)
    gen = (haps.cm / 100.0).astype(np.float32)
    edges = api.site_bins(haps.cm, a.bin_cm)
    w = api.site_widths(gen)
    rec = {"config": "decode_pairs_tail_summaries", "route": a.route, "tail_times": TIMES,
           "tail_states": [int(c) for c in cuts], "bins": int(edges.size - 1), "bin_cm": a.bin_cm, "haplotypes": a.haps,
           "sites": a.sites, "K": 69, "pairs": a.pairs, "calls": a.calls, "lib_hash": hip_source_hash(),
           "built_from": a.built_from, "has_fsmc_decode_pair_tail_summaries": has_entry, "abi_only": a.abi_only}
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
            walls, decode_s, reduce_s = [], [], []
            got = None
            for call in range(a.calls + 1):  # (the first is the warm-up)
                t0 = time.perf_counter()
                if a.route == "rows":
                    asmc.decodePairs(la, lb, tail_times=TIMES)
                    t1 = time.perf_counter()
                    rows = np.asarray(asmc.get_ref_of_results().per_pair_tail_probabilities)
                    got = reduce_rows(rows, edges, w)
                    del rows
                    decode_s.append(t1 - t0)
                    reduce_s.append(time.perf_counter() - t1)
                else:
                    asmc.decodePairs(la, lb, tail_summary_times=TIMES, site_bins=[int(x) for x in edges], site_weights=w)
                    res = asmc.get_ref_of_results()
                    got = (np.asarray(res.sum_of_tail_probabilities), np.asarray(res.per_pair_bin_tail_means),
                           np.asarray(res.per_pair_bin_tail_lengths))
                    del res
                walls.append(time.perf_counter() - t0)
            rec["product_path"] = checksums(*got)
            del asmc, got
        rec["wall_s_warmup"] = walls[0]
        rec["wall_s_calls"] = walls[1:]
        rec["wall_s_median"] = statistics.median(walls[1:])
        if decode_s:
            rec["decode_s_median"] = statistics.median(decode_s[1:])
            rec["numpy_reduction_s_median"] = statistics.median(reduce_s[1:])
        # (peak resident set of the process after the product-path calls, before the C-ABI part below)
        rec["peak_rss_bytes_product_path"] = peak_rss()

    # the first pairs through the C ABI: device time of the summaries' kernels next to the tail rows' on the same list
    n_abi = a.abi_pairs or min(a.pairs, 4096)
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=time_param, no_conditional_age_estimates=False)
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    pr = np.empty(n_abi, capi.PAIR_DTYPE)
    pr[capi.PAIR_DTYPE.names[0]], pr[capi.PAIR_DTYPE.names[1]] = ha[:n_abi], hb[:n_abi]
    ctx.upload_worklist(pr, capi.whole_sequence_groups(n_abi, pm.S))
    rec["abi_pairs"] = n_abi
    cdf_ms, tail_ms = [], []
    out_cdf = (np.zeros((len(cuts), n_abi, pm.S), np.float32), np.zeros((0, n_abi, pm.S), np.int32))
    for call in range(3):
        ctx.decode_pair_cdf(model, cuts, (), out=out_cdf)
        cdf_ms.append(ctx.last_kernel_ms())
        rec["cdf_slices"] = ctx.last_pair_cdf_slices()
        if has_entry:
            got = ctx.decode_pair_tail_summaries(model, cuts, edges, w)
            tail_ms.append(ctx.last_kernel_ms())
            rec["slices"] = ctx.last_pair_tail_slices()
            if call == 2:
                rec["c_abi"] = checksums(*got)
            del got
    rec["member"], rec["waves_per_window"] = ctx.last_kernel(), ctx.last_waves_per_window()
    ctx.close()
    rec["cdf_kernel_ms_calls"] = cdf_ms
    rec["cdf_kernel_ms"] = min(cdf_ms[1:])
    if tail_ms:
        rec["tail_summaries_kernel_ms_calls"] = tail_ms
        rec["tail_summaries_kernel_ms"] = min(tail_ms[1:])
        # (both spans hold the same decode and the same pair_cdf_kernel; the cdf entry's also the waits for its row copies
        # between slices, the summaries' its two reductions)
        rec["tail_summaries_over_cdf"] = rec["tail_summaries_kernel_ms"] / rec["cdf_kernel_ms"]
    rec["peak_rss_bytes_after_abi_calls"] = peak_rss()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
