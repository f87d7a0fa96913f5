#!/usr/bin/env python3
"""What --alignment-mode 3 and -a cost on the bench workload (bench.py itself measures the default mode only).

  python tools/trace_cost.py [--contigs 10000 --targets 100000 --steps 2 --warmup 1]

Runs the config-2 synthetic step (bench.py's workload and parameters, the blocking mk_search) in mode 2, in mode 3 and in mode 3 with -a,
prints the step time and the kernel table of each, then sends the accepted alignments of the last mode-3 step through mk_sw_backtrace_pairs
once more to count the pairs per attempt count and the (pair, attempt) jobs per kernel class.  profiles/trace_mode3.txt holds a run."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=10000)
    ap.add_argument("--targets", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import bench
    from metaeuk_amd import api
    api.init(0)
    print("device:", api.device_name())
    base = api.default_params()
    l2 = ctypes.CDLL(None).sysconf(191)
    base.host_l2_bytes = l2 if l2 and l2 > 0 else 262144
    targets, queries, _ = bench.make_inputs(args.contigs, args.targets, args.seed, 0)
    t_res, t_off = bench.pack(targets)
    q_res, q_off = bench.pack(queries)
    db = api.TargetDB.from_codes(t_res, t_off, base)
    print("workload: %d fragments (%.1f residues on average) x %d proteins" % (len(queries), float(q_off[-1]) / max(1, len(queries)), len(targets)))
    keep = None
    for label, mode, a in (("mode 2 (default)", 0, 0), ("mode 3", 3, 0), ("mode 3 + -a", 3, 1)):
        p = api.default_params()
        p.host_l2_bytes = base.host_l2_bytes
        p.alignment_mode, p.add_backtrace = mode, a
        times = []
        for s in range(args.warmup + args.steps):
            if s == args.warmup:
                api.kernel_stats(reset=True)
            t0 = time.time()
            q = api.Queries.from_codes(q_res, q_off, p)
            (hits, hoff), (alns, aoff) = api.search(db, q, p)
            dt = time.time() - t0
            if s >= args.warmup:
                times.append(dt)
            n_aln, left = int(aoff[-1]), api.trace_left_band(q)
            if mode == 3 and a == 0 and s == args.warmup + args.steps - 1:
                rec = np.frombuffer(alns, dtype=np.dtype([("db_key", "<u4"), ("bit_score", "<i4"), ("seq_id", "<f4"), ("qcov", "<f4"), ("dbcov", "<f4"), ("pad", "<u4"),
                                                         ("evalue", "<f8"), ("q_start", "<i4"), ("q_end", "<i4"), ("q_len", "<i4"), ("db_start", "<i4"),
                                                         ("db_end", "<i4"), ("db_len", "<i4"), ("aln_len", "<i4"), ("raw_score", "<i4")]), count=n_aln).copy()
                keep = (rec, np.repeat(np.arange(q.n, dtype=np.uint32), np.diff(np.asarray(aoff)).astype(np.int64)))
            q.close()
        st = api.kernel_stats(reset=True)
        print("\n== %s: %.1f ms per step (%d steps after %d warm-up), %d alignments, %d traces left the band" %
              (label, 1e3 * sum(times) / len(times), args.steps, args.warmup, n_aln, left))
        print("%-34s %10s %9s %16s" % ("kernel (per step)", "ms", "launches", "cells"))
        for name in sorted(st, key=lambda k: -st[k]["ms"]):
            v = st[name]
            if v["launches"] and (v["ms"] / args.steps >= 0.5 or name.startswith("sw_trace")):
                print("%-34s %10.2f %9.1f %16.0f" % (name, v["ms"] / args.steps, v["launches"] / args.steps, v["cells"] / args.steps))
        for prefix in ("sw_rev", "sw_trace"):
            ms = sum(v["ms"] for k, v in st.items() if k.startswith(prefix) and v["launches"]) / args.steps
            cells = sum(v["cells"] for k, v in st.items() if k.startswith(prefix) and v["launches"]) / args.steps
            print("sum %-30s %10.2f %9s %16.0f" % (prefix + "*", ms, "", cells))
    rec, qi = keep
    in5 = np.stack([rec["raw_score"], rec["q_end"], rec["db_end"], rec["q_start"], rec["db_start"]], axis=1).astype(np.int32)
    q = api.Queries.from_codes(q_res, q_off, base)
    _, bt, ids, att, band = api.sw_backtrace_pairs(db, q, qi, rec["db_key"], in5, base, keep_ops=False)
    n = len(att)
    print("\n== the accepted alignments of one mode-3 step through mk_sw_backtrace_pairs: %d pairs" % n)
    assert np.array_equal(bt, rec["aln_len"].astype(np.uint32)), "the kernel-level entry point disagrees with the search path"
    for k in range(1, int(att.max()) + 1):
        print("attempts %2d: %9d pairs (%.3f %%)" % (k, int((att == k).sum()), 100.0 * float((att == k).sum()) / n))
    first = (band.astype(np.int64) >> (att.astype(np.int64) - 1))
    bounds = [("lds11 (band <= 4)", 4), ("lds23 (band <= 10)", 10), ("lds67 (band <= 32)", 32), ("lds259 (band <= 128)", 128), ("lds1027 (band <= 512)", 512),
              ("global rows", 1 << 30)]
    jobs = {name: 0 for name, _ in bounds}
    for k in range(int(att.max())):
        b = first[att > k] << k
        lo = 0
        for name, hi in bounds:
            jobs[name] += int(((b > lo) & (b <= hi)).sum())
            lo = hi
    total = sum(jobs.values())
    for k, v in jobs.items():
        print("class %-20s %9d jobs (%.3f %%)" % (k, v, 100.0 * v / total))
    fb = np.bincount(np.minimum(first, 40))
    print("first band (|tn - qn| + 1): " + ", ".join("%d: %.2f %%" % (b, 100.0 * c / n) for b, c in enumerate(fb) if c and b < 12) + ", >= 12: %.2f %%" % (100.0 * fb[12:].sum() / n))
    print("rectangles: rows %.1f on average (max %d), columns %.1f (max %d)" % (float((rec["q_end"] - rec["q_start"] + 1).mean()), int((rec["q_end"] - rec["q_start"] + 1).max()),
                                                                              float((rec["db_end"] - rec["db_start"] + 1).mean()), int((rec["db_end"] - rec["db_start"] + 1).max())))


if __name__ == "__main__":
    main()
