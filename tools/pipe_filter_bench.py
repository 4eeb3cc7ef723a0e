"""What the severity / status filter inside the pipelined pass costs and saves on the C2-shaped
batch (the one `bench.py --config c2` builds, with the "vulnerability" bucket loaded).

One process, one prepared batch; after warm-up the legs are timed in turn, round after round
(leg A, leg B, ..., leg A, ...), so drift hits every leg alike:

  none        no filter set: the pass as it was before filters existed
  all5        all five severities, no ignored statuses (the kernel runs and drops only the
              findings whose severity string lies outside SeverityNames)
  hc          HIGH | CRITICAL
  hc_status   HIGH | CRITICAL, ignoring will_not_fix (5) and end_of_life (7)

Per leg: median / min / max of tvm_pipeline_run's wall time, raw and kept matches, D2H bytes,
and the time tvm_vuln_set_walk takes to consume the resulting set.  --legs none runs on a
library without the filter entry points (the commit before them), for an A/B of the unfiltered
pass.  The prefilter kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/pipe_filter_bench.py ...` run.

    python tools/pipe_filter_bench.py --passes 20 --out profiles/pipefilter/c2.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"none": None,
        "all5": dict(),
        "hc": dict(severities=("HIGH", "CRITICAL")),
        "hc_status": dict(severities=("HIGH", "CRITICAL"), ignore_statuses=(5, 7))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=20, help="timed passes per leg (at least 20 for a figure)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="none,all5,hc,hc_status")
    ap.add_argument("--keys-per-plat", type=int, default=30000)
    ap.add_argument("--targets", type=int, default=10000)
    ap.add_argument("--pkgs-per-target", type=int, default=400)
    ap.add_argument("--chunk", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    legs = [x for x in args.legs.split(",") if x]
    for x in legs:
        if x not in LEGS:
            raise SystemExit(f"unknown leg {x!r} (known: {', '.join(LEGS)})")

    import torch  # noqa: F401  first, as in bench.py: the library then binds to torch's HIP runtime
    import trivy_amd
    from bench import C2
    from trivy_amd.batch import MatchBatch

    t0 = time.perf_counter()
    wl = C2(args)
    db = trivy_amd.DB()
    wl.load(db, vulns=True)
    eng = trivy_amd.Engine(db.finalize(), 0)
    mb = MatchBatch(eng)
    wl.fill(mb)
    try:  # the exact match count first: the match buffer is sized to it, as bench.py sizes it
        total = mb.pipeline_prepare(chunk_packages=args.chunk).pipeline_run()[0]
    except OverflowError as e:
        total = e.args[0]
    mb.pipeline_prepare(match_cap=total, chunk_packages=args.chunk)
    print(f"[pipe_filter_bench] {wl.name}: {wl.n} packages, {total} matches ({time.perf_counter() - t0:.1f}s)",
          file=sys.stderr)

    def set_leg(name):
        if LEGS[name] is None:
            if hasattr(mb, "pipeline_set_filter"):
                mb.pipeline_set_filter(None)
        else:
            mb.pipeline_set_filter(mb.filter_opts(**LEGS[name]))

    def one(name):
        set_leg(name)
        got, ep, ms = mb.pipeline_run()
        if got != total or ep != -1:
            raise RuntimeError(f"leg {name}: {got} matches, poisoned package {ep}; expected {total}, -1")
        vs = mb.vulns(pipeline=True)
        t = time.perf_counter()
        n_w, _ = vs.walk()
        c_ms = (time.perf_counter() - t) * 1e3
        kept = len(vs)
        vs.close()
        if n_w != kept:
            raise RuntimeError(f"leg {name}: the consumer walked {n_w} of {kept} records")
        return ms, c_ms, kept, mb.pipeline_stats()["d2h_bytes"]

    for _ in range(max(1, args.warmup)):
        for name in legs:
            one(name)
    runs = {name: [] for name in legs}
    for _ in range(args.passes):
        for name in legs:  # alternated: one pass of every leg per round
            runs[name].append(one(name))
    out = {"workload": wl.name, "packages": wl.n, "raw_matches": total, "passes_per_leg": args.passes,
           "chunk_packages": args.chunk, "hip_runtime": trivy_amd.runtime_info(), "legs": {}}
    for name in legs:
        ms = sorted(r[0] for r in runs[name])
        cs = sorted(r[1] for r in runs[name])
        kept, d2h = runs[name][-1][2], runs[name][-1][3]
        out["legs"][name] = {"filter": LEGS[name], "pass_ms_median": statistics.median(ms), "pass_ms_min": ms[0],
                             "pass_ms_max": ms[-1], "pass_ms_p25": ms[len(ms) // 4], "pass_ms_p75": ms[(3 * len(ms)) // 4],
                             "raw": total, "kept": kept, "d2h_bytes": d2h, "consume_ms_median": statistics.median(cs),
                             "consume_ms_min": cs[0], "consume_ms_max": cs[-1],
                             "packages_per_s_pass": wl.n / (statistics.median(ms) / 1e3)}
        r = out["legs"][name]
        print(f"[pipe_filter_bench] {name:10s} pass {r['pass_ms_median']:.3f} ms (min {r['pass_ms_min']:.3f}, max "
              f"{r['pass_ms_max']:.3f})  kept {kept}/{total}  d2h {d2h / 1e6:.1f} MB  consume "
              f"{r['consume_ms_median']:.2f} ms", file=sys.stderr)
    mb.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
