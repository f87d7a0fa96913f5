#!/usr/bin/env python3
"""What --max-accept / --max-rejected save on the bench workload (bench.py itself measures the default limits only).

  python tools/limit_cost.py [--contigs 10000 --targets 100000 --steps 2 --warmup 1]

Runs the config-2 synthetic step (bench.py's workload and parameters, the blocking mk_search) at the default limits, with --max-accept 1 and
with -e 0.001 --max-rejected 5, and prints per run: the step time, what mk_align_statistics reports (pairs listed / scored, walks stopped,
rounds summed over the chunks) and the cells of the score pass (sw_fwd_*).  profiles/align_limits.txt holds a run."""
import argparse
import ctypes
import os
import sys
import time

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
    l2 = ctypes.CDLL(None).sysconf(191)
    l2 = l2 if l2 and l2 > 0 else 262144
    targets, queries, _ = bench.make_inputs(args.contigs, args.targets, args.seed, 0)
    t_res, t_off = bench.pack(targets)
    q_res, q_off = bench.pack(queries)
    base = api.default_params()
    base.host_l2_bytes = l2
    db = api.TargetDB.from_codes(t_res, t_off, base)
    print("workload: %d fragments (%.1f residues on average) x %d proteins" % (len(queries), float(q_off[-1]) / max(1, len(queries)), len(targets)))
    for label, kw in (("default limits", {}), ("--max-accept 1", dict(max_accept=1)), ("-e 0.001 --max-rejected 5", dict(evalue_thr=0.001, max_rejected=5))):
        p = api.default_params()
        p.host_l2_bytes = l2
        for k, v in kw.items():
            setattr(p, k, v)
        times = []
        for s in range(args.warmup + args.steps):
            if s == args.warmup:
                api.kernel_stats(reset=True)
            t0 = time.time()
            q = api.Queries.from_codes(q_res, q_off, p)
            _, (alns, aoff) = api.search(db, q, p)
            dt = time.time() - t0
            if s >= args.warmup:
                times.append(dt)
            n_aln, ast = int(aoff[-1]), api.align_statistics(q)
            q.close()
        st = api.kernel_stats(reset=True)
        fwd = {k: v for k, v in st.items() if k.startswith("sw_fwd") and v["launches"]}
        print("\n== %s: %.1f ms per step (%d steps after %d warm-up), %d alignments" % (label, 1e3 * sum(times) / len(times), args.steps, args.warmup, n_aln))
        print("   pairs listed %d, scored %d (%.1f %%), walks stopped by accept %d / by rejection %d, rounds (over the chunks) %d" %
              (ast["pairs_listed"], ast["pairs_scored"], 100.0 * ast["pairs_scored"] / max(1, ast["pairs_listed"]), ast["stopped_accept"], ast["stopped_rejected"],
               ast["rounds"]))
        print("   score pass (sw_fwd_*): %.3e cells, %.1f ms of kernel time, %.1f launches per step" %
              (sum(v["cells"] for v in fwd.values()) / args.steps, sum(v["ms"] for v in fwd.values()) / args.steps, sum(v["launches"] for v in fwd.values()) / args.steps))
        for name in ("align_limit_scan", "sw_pos", "sw_rev"):
            ms = sum(v["ms"] for k, v in st.items() if k.startswith(name) and v["launches"]) / args.steps
            n = sum(v["launches"] for k, v in st.items() if k.startswith(name)) / args.steps
            print("   %-18s %8.2f ms, %6.1f launches per step" % (name + "*", ms, n))


if __name__ == "__main__":
    main()
