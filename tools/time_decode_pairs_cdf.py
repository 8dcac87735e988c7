#!/usr/bin/env python3
"""ASMC.decodePairs for per-pair tail probabilities and quantile states (per_pair_tail_probabilities,
per_pair_quantile_states), timed through the product path on files of the C1 shape (300 haplotypes x 6760 sites,
K = 69): wall time of the call (median of --calls calls after one warm-up) and the peak resident set of the process,
then, through the C ABI, the device time of the call's kernels (fsmc_last_kernel_ms) against fsmc_decode_posteriors of
the same work list alone.

  --case tables  per_pair_posteriors=True and the reduction of the tables by numpy: each [K][S] table is divided by the
                 expected coalescence times again (the tables are handed out multiplied by them) and goes through
                 tests/pair_cdf_lists.py.  The only way a tree without fsmc_decode_pair_cdf has.  The wall time is the
                 call plus the reduction; both are also given apart.
  --case cdf     tail_times=[--tail-time] and quantiles=[0.025, 0.5, 0.975] alone: reduced on the device, no tables
                 on the host (three quantiles and one tail: one pass of the kernel)

Runs against any tree of this project (--tree: the directory that holds fastsmc_amd/), so that two builds are measured
by one script.  --abi-only skips the product path.  The C-ABI part runs on the first --abi-pairs pairs (default: up to
1024, the dump of which fsmc_decode_posteriors copies to the host: 1.9 GB): the kernel time of fsmc_decode_pair_cdf
(decode and reduction) against that of the dump decode alone, and the ratio.

Usage: tools/time_decode_pairs_cdf.py --case tables|cdf --pairs N [--calls 5] [--haps 300 --sites 6760]
                                      [--tail-time 100] [--abi-only] [--abi-pairs N] [--tree DIR] [--built-from TEXT]
One JSON line on stdout, stamped with the library's source hash; the checksums of the outputs let the lines of two
builds and two cases be compared (the tables route divides by the expected times, which is not exact: its checksums may
differ from the device's in the last places)."""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

QS = [0.025, 0.5, 0.975]


def checksums(tail, qstate):
    return {"tail_sum": float(np.asarray(tail, np.float64).sum()), "qstate_sum": int(np.asarray(qstate, np.int64).sum())}


def peak_rss():
    for line in open("/proc/self/status"):
        if line.startswith("VmHWM:"):
            return int(line.split()[1]) * 1024
    return None


def reduce_tables(CL, tables, exp_times, cuts, qs):
    """The numpy route: the [K][S] tables of the pairs (posterior x expected time) back to posteriors, batch by batch of
    64 in the reference's layout [S][K][64], through pair_cdf_lists.reduce."""
    et = np.asarray(exp_times, np.float32)[None, :, None]
    tails, qstates = [], []
    for b0 in range(0, len(tables), 64):
        chunk = np.stack([np.asarray(t, np.float32) for t in tables[b0:b0 + 64]])  # [n][K][S]
        post = np.ascontiguousarray((chunk / et).transpose(2, 1, 0))
        t, q = CL.reduce(post, post.shape[2], cuts, qs)
        tails.append(t)
        qstates.append(q)
    return np.concatenate(tails, axis=1), np.concatenate(qstates, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["tables", "cdf"], required=True)
    ap.add_argument("--pairs", type=int, required=True)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--haps", type=int, default=300)
    ap.add_argument("--sites", type=int, default=6760)
    ap.add_argument("--tail-time", type=float, default=100.0)
    ap.add_argument("--abi-only", action="store_true")
    ap.add_argument("--abi-pairs", type=int, default=0, help="pairs of the C-ABI part; 0 = min(--pairs, 1024)")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--built-from", default="", help="the commit the tree's library was built from (free text)")
    a = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(here, "tests"))  # (pair_cdf_lists: the numpy statement, from THIS tree)
    sys.path.insert(0, os.path.abspath(a.tree))
    from fastsmc_amd import api, capi, synth
    from fastsmc_amd.build import hip_source_hash
    from oracle import oracle as O
    import pair_cdf_lists as CL

    has_cdf = hasattr(capi.Context, "decode_pair_cdf")
    if a.case == "cdf" and not has_cdf:
        sys.exit("this tree has no fsmc_decode_pair_cdf: only --case tables can be timed on it")
    tables = synth.make_model_tables(69)
    haps = synth.make_haps(a.haps, a.sites, seed=1234)
    all_pairs = [(x, y) for y in range(a.haps) for x in range(y)][:a.pairs]
    assert len(all_pairs) == a.pairs, "more pairs asked for than the cohort has"
    ha, hb = np.array([p[0] for p in all_pairs], np.uint32), np.array([p[1] for p in all_pairs], np.uint32)
    disc = np.asarray(tables.discretization, np.float32)
    cuts = [int((disc[:-1] < np.float32(a.tail_time)).sum())]
    assert cuts[0] >= 1, "no interval of the discretization starts below --tail-time"
    rec = {"config": "decode_pairs_cdf", "case": a.case, "tail_time": a.tail_time, "tail_state": cuts[0], "quantiles": QS,
           "haplotypes": a.haps, "sites": a.sites, "K": 69, "pairs": a.pairs, "calls": a.calls,
           "lib_hash": hip_source_hash(), "built_from": a.built_from, "has_fsmc_decode_pair_cdf": has_cdf,
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
            exp_times = np.asarray(asmc.hmm().getExpectedCoalTimes(), np.float32)
            walls, decode_s, reduce_s = [], [], []
            got = None
            for call in range(a.calls + 1):  # (the first is the warm-up)
                t0 = time.perf_counter()
                if a.case == "tables":
                    asmc.decodePairs(la, lb, True, False, False, False)
                    t1 = time.perf_counter()
                    res = asmc.get_ref_of_results()
                    got = reduce_tables(CL, res.per_pair_posteriors, exp_times, cuts, QS)
                    del res
                    decode_s.append(t1 - t0)
                    reduce_s.append(time.perf_counter() - t1)
                else:
                    asmc.decodePairs(la, lb, tail_times=[a.tail_time], quantiles=QS)
                walls.append(time.perf_counter() - t0)
            res = asmc.get_ref_of_results()
            if a.case == "cdf":
                got = (np.asarray(res.per_pair_tail_probabilities), np.asarray(res.per_pair_quantile_states))
                assert np.asarray(res.tail_states).tolist() == cuts
            rec["product_path"] = checksums(*got)
            rec["tables_held"] = len(res.per_pair_posteriors)
            del res, asmc, got
        rec["wall_s_warmup"] = walls[0]
        rec["wall_s_calls"] = walls[1:]
        rec["wall_s_median"] = statistics.median(walls[1:])
        if decode_s:
            rec["decode_s_median"] = statistics.median(decode_s[1:])
            rec["numpy_reduction_s_median"] = statistics.median(reduce_s[1:])
        # (peak resident set of the process after the product-path calls, before the C-ABI part below)
        rec["peak_rss_bytes_product_path"] = peak_rss()

    # the first pairs through the C ABI: device time of the call's kernels against the dump decode alone
    n_abi = a.abi_pairs or min(a.pairs, 1024)
    bits, derived, _ = synth.fold_and_pack(haps.alleles)
    pm = O.prepare_model(tables, gen, haps.bp, derived, a.haps, time=time_param, no_conditional_age_estimates=False)
    ctx = capi.Context(0)
    model = ctx.create_model(pm)
    ctx.upload_haps(bits, pm.S)
    pr = np.empty(n_abi, capi.PAIR_DTYPE)
    pr[capi.PAIR_DTYPE.names[0]], pr[capi.PAIR_DTYPE.names[1]] = ha[:n_abi], hb[:n_abi]
    ctx.upload_worklist(pr, capi.whole_sequence_groups(n_abi, pm.S))
    rec["abi_pairs"] = n_abi
    dump_ms, cdf_ms = [], []
    for call in range(3):
        post = ctx.decode_posteriors(model)
        dump_ms.append(ctx.last_kernel_ms())
        del post
        if has_cdf and a.case == "cdf":
            got = ctx.decode_pair_cdf(model, cuts, QS)
            cdf_ms.append(ctx.last_kernel_ms())
            rec["slices"] = ctx.last_pair_cdf_slices()
            if call == 2:
                rec["c_abi"] = checksums(*got)
            del got
    rec["member"], rec["waves_per_window"] = ctx.last_kernel(), ctx.last_waves_per_window()
    ctx.close()
    rec["dump_kernel_ms_calls"] = dump_ms
    rec["dump_kernel_ms"] = min(dump_ms[1:])
    if cdf_ms:
        rec["cdf_kernel_ms_calls"] = cdf_ms
        rec["cdf_kernel_ms"] = min(cdf_ms[1:])
        # the expectation: one pass of the reduction adds at most about a third to the dump decode
        rec["cdf_over_dump"] = rec["cdf_kernel_ms"] / rec["dump_kernel_ms"]
        rec["pair_sites_per_s"] = n_abi * pm.S / (rec["cdf_kernel_ms"] / 1e3)
    rec["peak_rss_bytes_after_abi_calls"] = peak_rss()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
