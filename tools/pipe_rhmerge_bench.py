"""What merging Red Hat findings inside the pipelined pass (TVM_PIPE_RH_MERGE) costs and saves
on the C5-shaped batch (the one `bench.py --config c5` builds, RHEL family + Alpine, with the
"vulnerability" bucket loaded).

One process, one batch; each leg has its own prepared MatchBatch over the same packages, and
after warm-up the legs are timed in turn, pass by pass (leg A, leg B, ..., leg A, ...), so
drift hits every leg alike:

  off         no flag: the raw pass; tvm_pipeline_vulns runs the device merge and the export
  on          TVM_PIPE_RH_MERGE: the pass merges per chunk; tvm_pipeline_vulns copies nothing
  on_hc       the flag with HIGH | CRITICAL
  on_all5     the flag with all five severities (its difference from `on` is the predicate's price)

Per leg: median / min / max of tvm_pipeline_run's wall time, raw matches and entries returned,
D2H bytes, the time of tvm_pipeline_vulns and the time tvm_vuln_set_walk takes to consume the
set.  --legs off runs on a library without the flag (the commit before it, TVM_LIB_PATH), for
an A/B of the flag-off pass in a process of its own.  The merge kernel's own time comes from a
separate `rocprofv3 --kernel-trace --stats -- python tools/pipe_rhmerge_bench.py ...` run.

    python tools/pipe_rhmerge_bench.py --passes 20 --out profiles/rhmerge/new_1.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# leg -> (rh_merge, filter options or None)
LEGS = {"off": (False, None),
        "on": (True, None),
        "on_hc": (True, dict(severities=("HIGH", "CRITICAL"))),
        "on_all5": (True, dict())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=20, help="timed passes per leg (at least 20 for a figure)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="off,on,on_hc,on_all5")
    ap.add_argument("--packages", type=int, default=0, help="packages of the batch (0: C5's bench size)")
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    legs = [x for x in args.legs.split(",") if x]
    for x in legs:
        if x not in LEGS:
            raise SystemExit(f"unknown leg {x!r} (known: {', '.join(LEGS)})")

    import torch  # noqa: F401  first, as in bench.py: the library then binds to torch's HIP runtime
    import trivy_amd
    from bench import Mix
    from trivy_amd.batch import MatchBatch

    t0 = time.perf_counter()
    wl = Mix(args, "c5")
    db = trivy_amd.DB()
    wl.load(db, vulns=True)
    eng = trivy_amd.Engine(db.finalize(), 0)
    first = MatchBatch(eng)
    wl.fill(first)
    try:  # the exact match count first: the match buffers are sized to it, as bench.py sizes them
        total = first.pipeline_prepare(chunk_packages=args.chunk).pipeline_run()[0]
    except OverflowError as e:
        total = e.args[0]
    first.close()
    print(f"[pipe_rhmerge_bench] {wl.name}: {wl.n} packages, {total} matches ({time.perf_counter() - t0:.1f}s)",
          file=sys.stderr)
    batches = {}
    for name in legs:
        flag, opts = LEGS[name]
        mb = MatchBatch(eng)
        wl.fill(mb)
        if flag:
            mb.pipeline_prepare(match_cap=total, chunk_packages=args.chunk, rh_merge=True)
        else:  # no keyword: this leg also runs on a library and a package without the flag
            mb.pipeline_prepare(match_cap=total, chunk_packages=args.chunk)
        if opts is not None:
            mb.pipeline_set_filter(mb.filter_opts(**opts))
        batches[name] = mb

    def one(name):
        mb = batches[name]
        got, ep, ms = mb.pipeline_run()
        if got != total or ep != -1:
            raise RuntimeError(f"leg {name}: {got} matches, poisoned package {ep}; expected {total}, -1")
        vs = mb.vulns(pipeline=True)
        t = time.perf_counter()
        n_w, _ = vs.walk()
        c_ms = (time.perf_counter() - t) * 1e3
        kept, v_ms, n_grp = len(vs), vs.ms, vs.n_grp_recs
        vs.close()
        if n_w != kept:
            raise RuntimeError(f"leg {name}: the consumer walked {n_w} of {kept} records")
        return ms, v_ms, c_ms, kept, mb.pipeline_stats()["d2h_bytes"], n_grp

    for _ in range(max(1, args.warmup)):
        for name in legs:
            one(name)
    runs = {name: [] for name in legs}
    for _ in range(args.passes):
        for name in legs:  # alternated: one pass of every leg per round
            runs[name].append(one(name))
    out = {"workload": wl.name, "packages": wl.n, "raw_matches": total, "passes_per_leg": args.passes,
           "chunk_packages": args.chunk, "hip_runtime": trivy_amd.runtime_info(),
           "library": os.environ.get("TVM_LIB_PATH") or "this commit's", "legs": {}}
    for name in legs:
        ms = sorted(r[0] for r in runs[name])
        vm = sorted(r[1] for r in runs[name])
        cs = sorted(r[2] for r in runs[name])
        kept, d2h, n_grp = runs[name][-1][3:]
        out["legs"][name] = {"rh_merge": LEGS[name][0], "filter": LEGS[name][1], "pass_ms_median": statistics.median(ms),
                             "pass_ms_min": ms[0], "pass_ms_max": ms[-1], "pass_ms_p25": ms[len(ms) // 4],
                             "pass_ms_p75": ms[(3 * len(ms)) // 4], "raw": total, "entries": kept, "d2h_bytes": d2h,
                             "group_records": n_grp, "vulns_ms_median": statistics.median(vm), "vulns_ms_min": vm[0],
                             "vulns_ms_max": vm[-1], "consume_ms_median": statistics.median(cs), "consume_ms_min": cs[0],
                             "consume_ms_max": cs[-1],
                             "pass_plus_vulns_ms": statistics.median(sorted(r[0] + r[1] for r in runs[name]))}
        r = out["legs"][name]
        print(f"[pipe_rhmerge_bench] {name:8s} pass {r['pass_ms_median']:.3f} ms (min {r['pass_ms_min']:.3f}, max "
              f"{r['pass_ms_max']:.3f})  vulns {r['vulns_ms_median']:.3f} ms  entries {kept}/{total}  d2h "
              f"{d2h / 1e6:.1f} MB  groups {n_grp}  consume {r['consume_ms_median']:.2f} ms", file=sys.stderr)
    for mb in batches.values():
        mb.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
