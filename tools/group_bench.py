"""What an engine group (tvm_group_*, one batch sharded over several engines in one process)
costs on the C2 batch at its benchmark size (the one `bench.py --config c2` builds), on ONE GPU:
every member sits on device 0, so members share the GPU and the link and no speed-up is
expected or claimed.  A scaling curve over real GPUs is not measured here.

One process, one batch; each leg has its own prepared batch over the same packages, and after
warm-up the legs are timed in turn, pass by pass (leg A, leg B, ..., leg A, ...), so drift hits
every leg alike:

  plain   tvm_pipeline_run on a single engine
  g1      tvm_group_pipeline_run through a group of 1 (the caller's thread serves the member)
  g2, g3  the same through 2 and 3 members on the one device (report only)

Besides, once per run (skipped by --legs plain): the shard plan's time in both modes
(tvm_group_plan_host over the batch's targets; the row pre-probe as the difference between a
group add planned by rows and one planned by packages), the group add against
tvm_batch_add_targets, and tvm_group_csr_into for 2 members.

--legs plain also runs on a library without groups (the commit before them, TVM_LIB_PATH), for
an A/B of the plain pass in a process of its own: the parent's two runs give the spread a group
of 1 has to stay inside.

    python tools/group_bench.py --passes 20 --out profiles/group/new_1.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"plain": 0, "g1": 1, "g2": 2, "g3": 3}


def best_ms(f, reps=3):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=20, help="timed passes per leg (at least 20 for a figure)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="plain,g1,g2,g3")
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
    grouped = any(LEGS[x] for x in legs)

    import numpy as np
    import torch  # noqa: F401  first, as in bench.py: the library then binds to torch's HIP runtime
    from trivy_amd import _lib
    if not grouped:  # a library from before groups: bind what it exports
        have = ctypes.CDLL(_lib.LIB_PATH)
        _lib._SIG[:] = [s for s in _lib._SIG if hasattr(have, s[0])]
    import trivy_amd
    from bench import C2
    from trivy_amd.batch import MatchBatch

    t0 = time.perf_counter()
    wl = C2(args)
    db = trivy_amd.DB()
    wl.load(db, vulns=False)
    db.finalize()
    eng = trivy_amd.Engine(db, 0)
    first = MatchBatch(eng)
    wl.fill(first)
    try:  # the exact match count first: the match buffers are sized to it, as bench.py sizes them
        total = first.pipeline_prepare(chunk_packages=args.chunk).pipeline_run()[0]
    except OverflowError as e:
        total = e.args[0]
    first.close()
    print(f"[group_bench] {wl.name}: {wl.n} packages, {total} matches ({time.perf_counter() - t0:.1f}s)", file=sys.stderr)
    out = {"workload": wl.name, "packages": wl.n, "raw_matches": total, "passes_per_leg": args.passes,
           "chunk_packages": args.chunk, "hip_runtime": trivy_amd.runtime_info(), "devices": "every member on device 0",
           "library": os.environ.get("TVM_LIB_PATH") or "this commit's", "legs": {}}

    batches, groups = {}, {}
    for name in legs:
        n = LEGS[name]
        if n == 0:
            mb = MatchBatch(eng)
            wl.fill(mb)
            mb.pipeline_prepare(match_cap=total, chunk_packages=args.chunk)
        else:
            from trivy_amd.group import EngineGroup, GroupBatch
            groups[name] = EngineGroup(db, [0] * n)
            mb = GroupBatch(groups[name])
            wl.fill(mb)
            if n > 1:  # exact member capacities from a first pass, as a caller sizes them
                mb.pipeline_prepare(match_cap=1024, chunk_packages=args.chunk)
                try:
                    mb.pipeline_run()
                except OverflowError:
                    pass
                mb.pipeline_prepare(member_caps=mb.member_matches, chunk_packages=args.chunk)
            else:
                mb.pipeline_prepare(match_cap=total, chunk_packages=args.chunk)
        batches[name] = mb

    def one(name):
        got, ep, ms = batches[name].pipeline_run()
        if got != total or ep != -1:
            raise RuntimeError(f"leg {name}: {got} matches, poisoned package {ep}; expected {total}, -1")
        return ms

    for _ in range(max(1, args.warmup)):
        for name in legs:
            one(name)
    runs = {name: [] for name in legs}
    for _ in range(args.passes):
        for name in legs:  # alternated: one pass of every leg per round
            runs[name].append(one(name))
    for name in legs:
        ms = sorted(runs[name])
        r = out["legs"][name] = {"members": LEGS[name], "pass_ms_median": statistics.median(ms), "pass_ms_min": ms[0],
                                 "pass_ms_max": ms[-1], "pass_ms_p25": ms[len(ms) // 4], "pass_ms_p75": ms[(3 * len(ms)) // 4]}
        if LEGS[name]:
            r["shards"] = batches[name].shards()
            r["member_matches"] = batches[name].member_matches
        print(f"[group_bench] {name:6s} pass {r['pass_ms_median']:.3f} ms (min {r['pass_ms_min']:.3f}, max "
              f"{r['pass_ms_max']:.3f})", file=sys.stderr)
    for mb in batches.values():
        mb.close()

    if grouped:
        from trivy_amd._lib import lib
        from trivy_amd.group import PLAN_PACKAGES, PLAN_ROWS, EngineGroup, GroupBatch
        g2 = groups.get("g2") or EngineGroup(db, [0, 0])
        ends = np.array([b1 for _, _, b1 in wl.batch.targets], dtype=np.uint64)
        bounds = np.zeros(3, dtype=np.uint64)
        plan_host = best_ms(lambda: lib().tvm_group_plan_host(len(ends), ends.ctypes.data, None, 2, bounds.ctypes.data), 5)
        wl.arena()

        def add(cls, owner, **kw):
            def f():
                b = cls(owner)
                arena, noff, nlen, voff, vlen = wl.arena()
                b.add_targets([wl.sdb.platforms[p] for p, _, _ in wl.batch.targets], ends, arena, noff, nlen, voff, vlen,
                              **kw)
                f.shards = b.shards() if hasattr(b, "shards") else None
                b.close()
            return f
        single = add(MatchBatch, eng)
        by_pk, by_rows = add(GroupBatch, g2, plan=PLAN_PACKAGES), add(GroupBatch, g2, plan=PLAN_ROWS)
        out["add"] = {"tvm_batch_add_targets_ms": best_ms(single), "group_add_by_packages_ms": best_ms(by_pk),
                      "group_add_by_rows_ms": best_ms(by_rows), "members": 2,
                      "note": "each figure includes building the ctypes bucket array (the same in all three)"}
        out["plan"] = {"plan_host_packages_ms": plan_host, "targets": len(ends),
                       "row_probe_ms": out["add"]["group_add_by_rows_ms"] - out["add"]["group_add_by_packages_ms"],
                       "shards_by_packages": by_pk.shards, "shards_by_rows": by_rows.shards}
        gb = GroupBatch(g2)
        wl.fill(gb)
        gb.upload(match_cap=1024).launch()
        gb.status()
        gb.upload(member_caps=gb.member_matches).launch()
        n, ep, bits = gb.status()
        adv = torch.empty(max(n, 1), dtype=torch.int32, device="cuda:0")
        rend = torch.empty(wl.n, dtype=torch.int32, device="cuda:0")
        ms = sorted(best_ms(lambda: gb.csr_into(0, adv, rend), 1) for _ in range(10))
        out["csr_into"] = {"members": 2, "matches": n, "ms_median": statistics.median(ms), "ms_min": ms[0], "ms_max": ms[-1],
                           "bytes": 4 * n + 4 * wl.n}
        gb.close()
        print(f"[group_bench] plan {out['plan']}  add {out['add']}  csr_into {out['csr_into']}", file=sys.stderr)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
