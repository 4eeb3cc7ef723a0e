"""Host model of the dpkg fast encoder's loop cost per wave (encoder balance): over the
C2 synthetic batch, what a wave of the match kernel spends in deb_fast_key's loops under different
assignments of a tile's 256 packages to its 4 waves.

A wave's loops run to its longest version, so its cost is set by the lane maxima:
    pre-pass   ceil(n / 4) dword trips            (n = version bytes)
    emission   floor(m / 4) dword trips           (m = n - epoch prefix)
    tail       m % 4 single bytes
priced with the static instruction counts of the gfx950 build (profiles/instr/phase_counts.txt and the
loop bodies' disassembly): 35 vector instructions per pre-pass trip, 103 per emission trip, 26 per
tail byte.  A version the encoder leaves before its loops (unparsable: no leading digit) costs none.

Arrangements of a tile:
    now          lane i encodes package i
    found        only packages whose name the index holds, packed into whole waves, tile order
    found+sort   the same, longest bucket first (bucket = the version's dword count)
    sort         every package, longest bucket first
    cut12        every lane's version cut to 12 bytes (the diag_enc12 measurement build)

With --auto-ms and --cut12-ms (medians of `bench.py --sweep` on the DIAG build) it prices a unit of
loop cost on hardware and prints the bound on what found+sort can gain.  No GPU.

    python tools/encbal_model.py [--keys-per-plat N --targets N --pkgs-per-target N]
                                 [--auto-ms T --cut12-ms T --spread-ms S]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLATS = ["debian 11", "debian 12", "ubuntu 20.04", "ubuntu 22.04", "ubuntu 24.04"]  # bench.py C2
WEIGHTS = [30, 30, 13, 13, 14]
TILE, WAVE = 256, 64
VALU_PRE, VALU_MAIN, VALU_TAIL = 35, 103, 26


def lane_trips(n, r0, runs):
    """(pre-pass trips, emission trips, tail bytes) per lane; `runs`: the encoder reaches its loops."""
    m = np.maximum(n - r0, 0)
    z = np.zeros_like(n)
    return (n + 3) // 4, np.where(runs, m // 4, z), np.where(runs, m % 4, z)


def wave_cost(pre, main, tail, active):
    """Per-wave (trips, vector instructions) of lane arrays shaped (tiles, 256); inactive lanes cost 0."""
    def wmax(x):
        return np.where(active, x, 0).reshape(-1, TILE // WAVE, WAVE).max(axis=2)
    p, m, t = wmax(pre), wmax(main), wmax(tail)
    return p + m, VALU_PRE * p + VALU_MAIN * m + VALU_TAIL * t


def packed(order_key, take):
    """Per tile, the lanes' source packages when the packages in `take` are packed to the front,
    by descending order_key (stable); returns (source index per lane, lane is active)."""
    key = np.where(take, -order_key.astype(np.int64), np.iinfo(np.int64).max)
    src = np.argsort(key, axis=1, kind="stable")
    active = np.arange(TILE)[None, :] < take.sum(axis=1)[:, None]
    return src, active


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys-per-plat", type=int, default=30000)
    ap.add_argument("--targets", type=int, default=10000)
    ap.add_argument("--pkgs-per-target", type=int, default=400)
    ap.add_argument("--auto-ms", type=float, default=None, help="median ms per pass of the auto kernel")
    ap.add_argument("--cut12-ms", type=float, default=None, help="median ms per pass of diag_enc12")
    ap.add_argument("--spread-ms", type=float, default=None, help="auto's run-to-run spread in that sweep (max - min)")
    args = ap.parse_args()
    from tools.synth import make_db, make_batch
    sdb = make_db(PLATS, args.keys_per_plat)
    batch = make_batch(sdb, args.targets, args.pkgs_per_target, WEIGHTS, seed=2)
    held = {(int(sdb.key_plat[k]), sdb.key_names[k]) for k in range(len(sdb.key_names))}
    npk = len(batch)
    n = np.fromiter((len(v) for v in batch.versions), dtype=np.int64, count=npk)
    colon = np.fromiter((v.find(b":") for v in batch.versions), dtype=np.int64, count=npk)
    r0 = np.where(colon >= 0, colon + 1, 0)
    first = np.fromiter((v[c + 1] if c + 1 < len(v) else 0 for v, c in zip(batch.versions, colon.tolist())),
                        dtype=np.int64, count=npk)
    runs = (first >= 48) & (first <= 57)  # the upstream version starts with a digit
    found = np.fromiter(((p, nm) in held for p, nm in zip(batch.plat.tolist(), batch.names)), dtype=bool, count=npk)

    pad = (-npk) % TILE
    def tiles(x, fill=0):
        return np.concatenate([x, np.full(pad, fill, dtype=x.dtype)]).reshape(-1, TILE)
    n_t, r0_t, runs_t, found_t = tiles(n), tiles(r0), tiles(runs, False), tiles(found, False)
    real_t = tiles(np.ones(npk, dtype=bool), False)
    bucket = (n_t + 3) // 4
    pre, mn, tl = lane_trips(n_t, r0_t, runs_t)
    rows = {}
    rows["now"] = wave_cost(pre, mn, tl, real_t)
    for name, key, take in (("found", np.zeros_like(bucket), found_t), ("found+sort", bucket, found_t),
                            ("sort", bucket, real_t)):
        src, active = packed(key, take)
        g = lambda x: np.take_along_axis(x, src, axis=1)
        rows[name] = wave_cost(g(pre), g(mn), g(tl), active)
    n12 = np.minimum(n_t, 12)
    rows["cut12"] = wave_cost(*lane_trips(n12, np.minimum(r0_t, n12), runs_t), real_t)

    waves = rows["now"][0].size
    print(f"packages {npk} in {n_t.shape[0]} tiles, {waves} waves; name held by the index: {100.0 * found.mean():.1f} %")
    print(f"version bytes: mean {n.mean():.1f}, mean of a wave's longest {n_t.reshape(-1, WAVE).max(axis=1).mean():.1f}")
    print(f"{'arrangement':>12}  dword trips / wave  loop vector instructions / wave")
    for name, (trips, valu) in rows.items():
        print(f"{name:>12}  {trips.mean():18.2f}  {valu.mean():31.1f}")
    if args.auto_ms is not None and args.cut12_ms is not None:
        d_valu = rows["now"][1].mean() - rows["cut12"][1].mean()
        d_trips = rows["now"][0].mean() - rows["cut12"][0].mean()
        d_ms = args.auto_ms - args.cut12_ms
        print(f"measured: auto {args.auto_ms:.4f} ms, diag_enc12 {args.cut12_ms:.4f} ms: {d_ms:.4f} ms for {d_trips:.2f} dword "
              f"trips ({d_valu:.0f} loop instructions) per wave = {1e3 * d_ms / d_trips:.2f} us per trip")
        for name in ("found", "found+sort", "sort"):
            gain = d_ms * (rows["now"][1].mean() - rows[name][1].mean()) / d_valu
            print(f"bound on {name}: {gain:.4f} ms ({100.0 * gain / args.auto_ms:.1f} % of the pass), before the list's own cost")
        if args.spread_ms is not None:
            gain = d_ms * (rows["now"][1].mean() - rows["found+sort"][1].mean()) / d_valu
            verdict = "below" if gain < 2 * args.spread_ms else "at least"
            print(f"auto's spread in the sweep {args.spread_ms:.4f} ms: the found+sort bound is {verdict} twice the spread")


if __name__ == "__main__":
    main()
