#!/usr/bin/env python3
"""What the backtrace of profile queries (mk_profile_backtrace) costs beside the search that feeds it.

  python tools/profile_trace_cost.py [--contigs 10000 --targets 100000 --profiles 2048 --steps 2 --warmup 1]

Runs bench.py's config-4 leg at a small size -- synthetic profiles as the queries, the fragments of the synthetic contigs as the indexed side,
the leg's parameters, the blocking mk_search -- and then mk_profile_backtrace over the accepted records, with and without the operation strings.
Prints the time of each call and the kernel table: the Smith-Waterman passes of the search and `trace_profile` for the same records.
profiles/trace_profile.txt holds a run."""
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
    ap.add_argument("--profiles", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import bench
    from metaeuk_amd import api, synth
    api.init(0)
    print("device:", api.device_name())
    _, fragments, _ = bench.make_inputs(args.contigs, args.targets, args.seed, 0)
    f_res, f_off = bench.pack(fragments)
    proteins, _ = synth.make_targets(args.profiles, args.seed)
    entries = synth.make_profiles(proteins, args.seed)
    p = api.default_params()                               # bench.py: config4_leg
    l2 = ctypes.CDLL(None).sysconf(191)
    p.host_l2_bytes = l2 if l2 and l2 > 0 else 262144
    p.sensitivity, p.profile_search, p.max_seqs = 4.0, 1, max(300, len(fragments))
    p.evalue_thr = float("%g" % (100.0 * (np.float32(len(fragments)) / np.float32(len(entries)))))
    db = api.TargetDB.from_codes(f_res, f_off, p)
    print("workload: %d profiles (%d columns) x %d fragments (%.1f residues on average)" % (
        len(entries), sum(len(e) // 25 for e in entries), len(fragments), float(f_off[-1]) / max(1, len(fragments))))
    t_search, t_bt, t_ids = [], [], []
    for s in range(args.warmup + args.steps):
        if s == args.warmup:
            api.kernel_stats(reset=True)
        q = api.Profiles(entries, p)
        t0 = time.time()
        _, (alns, aoff) = api.search(db, q, p)
        t1 = time.time()
        _, (ops, ops_off, ids) = api.profile_backtrace(db, q, p, keep_ops=True)
        t2 = time.time()
        api.profile_backtrace(db, q, p, keep_ops=False)
        t3 = time.time()
        if s >= args.warmup:
            t_search.append(t1 - t0); t_bt.append(t2 - t1); t_ids.append(t3 - t2)
        n_aln, n_ops, n_ids, left = int(aoff[-1]), len(ops), int(ids.sum()), api.trace_left_band(q)
        q.close()
    st = api.kernel_stats(reset=True)
    ms = lambda ts: 1e3 * sum(ts) / len(ts)
    print("\n%d accepted records, %d operations, %d identities, %d traces left the band; per step (%d steps after %d warm-up): search %.1f ms, "
          "backtrace with operations %.1f ms, identities only %.1f ms" % (n_aln, n_ops, n_ids, left, args.steps, args.warmup, ms(t_search), ms(t_bt), ms(t_ids)))
    print("%-34s %10s %9s %16s   (per step; trace_profile*: two calls per step)" % ("kernel", "ms", "launches", "cells"))
    for name in sorted(st, key=lambda k: -st[k]["ms"]):
        v = st[name]
        if v["launches"] and (v["ms"] / args.steps >= 0.1 or name.startswith("trace_profile")):
            print("%-34s %10.2f %9.1f %16.0f" % (name, v["ms"] / args.steps, v["launches"] / args.steps, v["cells"] / args.steps))


if __name__ == "__main__":
    main()
