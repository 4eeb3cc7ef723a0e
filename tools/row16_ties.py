"""Host count for the 16-byte prefix-stripped dpkg rows: over the C2 synthetic
batch, how many (package, row) pairs a hot row of P prefix bytes (held per key, P <= 7) + W window
bytes cannot decide.

A pair is undecided when the installed key equals the bound on its first P + W bytes and both
keys run past P + W: then the full 32-byte Row (24-byte head, then the key arena) has to be read.
Every other pair - the installed key differs from the key's prefix, the window differs, one of
the keys ends inside the window, or the row is unfixed (hi = +inf) - is decided by the hot row.

Keys come from tvm_version_key (the encoder both the flattener and the kernel run); no GPU.

    python tools/row16_ties.py [--keys-per-plat N --targets N --pkgs-per-target N]
"""
import argparse
import ctypes
import os
import sys
from collections import Counter, defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLATS = ["debian 11", "debian 12", "ubuntu 20.04", "ubuntu 22.04", "ubuntu 24.04"]  # bench.py C2
WEIGHTS = [30, 30, 13, 13, 14]
P_CAP = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys-per-plat", type=int, default=30000)
    ap.add_argument("--targets", type=int, default=10000)
    ap.add_argument("--pkgs-per-target", type=int, default=400)
    args = ap.parse_args()
    from tools.synth import make_db, make_batch
    from trivy_amd._lib import lib
    buf = ctypes.create_string_buffer(4096)
    cache = {}

    def key(v):
        k = cache.get(v)
        if k is None:
            n = lib().tvm_version_key(1, v, len(v), buf, len(buf))
            k = cache[v] = buf.raw[:n] if n >= 0 else False
        return k

    sdb = make_db(PLATS, args.keys_per_plat)
    batch = make_batch(sdb, args.targets, args.pkgs_per_target, WEIGHTS, seed=2)
    kidx = {(int(sdb.key_plat[k]), sdb.key_names[k]): k for k in range(len(sdb.key_names))}
    inst = defaultdict(Counter)  # key -> installed sort key -> packages
    for p, n, v in zip(batch.plat.tolist(), batch.names, batch.versions):
        k = kidx.get((p, n))
        if k is None:
            continue
        kv = key(v)
        if kv is not False:  # an unparsable installed version sweeps no row
            inst[k][kv] += 1

    windows = (9, 10, 11, 12, 16, 24)  # W; 16 / 24 with P = 0 are the heads round 5 measured
    pairs = bounded = 0
    undecided = {w: 0 for w in windows}
    undecided_p0 = {w: 0 for w in windows}
    off_prefix = 0  # pairs decided by the slot's prefix alone (installed key differs from it)
    keys_by_p = Counter()
    klen = Counter()
    for k in range(len(sdb.key_names)):
        bounds = [key(f) for f in sdb.adv_fixed[int(sdb.adv_begin[k]):int(sdb.adv_begin[k + 1])] if f]
        bounds = [b for b in bounds if b is not False]
        nrows = int(sdb.adv_begin[k + 1] - sdb.adv_begin[k])  # unfixed rows included (hi = +inf)
        P = 0
        if bounds:
            lo, hi = min(bounds), max(bounds)
            while P < P_CAP and P < len(lo) and P < len(hi) and lo[P] == hi[P]:
                P += 1
        keys_by_p[P] += 1
        for b in bounds:
            klen[len(b)] += 1
        if k not in inst:
            continue
        npk = sum(inst[k].values())
        pairs += npk * nrows
        bounded += npk * len(bounds)
        pre = bounds[0][:P] if bounds else b""
        for kv, c in inst[k].items():
            if kv[:P] != pre:
                off_prefix += c * len(bounds)
        for w in windows:
            for p_eff, acc in ((P, undecided), (0, undecided_p0)):
                n = p_eff + w
                heads = Counter(b[:n] for b in bounds if len(b) > n)
                if not heads:
                    continue
                for kv, c in inst[k].items():
                    if len(kv) > n:
                        acc[w] += c * heads.get(kv[:n], 0)

    print(f"packages {len(batch)}, with rows {sum(sum(c.values()) for c in inst.values())}, pairs {pairs} "
          f"({bounded} against a bounded row)")
    print("keys by P: " + ", ".join(f"P={p}: {n}" for p, n in sorted(keys_by_p.items())))
    tot = sum(klen.values())
    cum = 0
    line = []
    for n in sorted(klen):
        cum += klen[n]
        line.append(f"<={n}: {100.0 * cum / tot:.1f}%")
    print("bound key bytes (cumulative): " + ", ".join(line))
    print(f"pairs decided by the prefix alone (installed key off the key's prefix): {off_prefix} "
          f"({100.0 * off_prefix / max(pairs, 1):.3f} %)")
    for w in windows:
        print(f"W={w:2d}: undecided with the key's prefix {undecided[w]} ({100.0 * undecided[w] / max(pairs, 1):.3f} % of "
              f"pairs); without a prefix (P = 0) {undecided_p0[w]} ({100.0 * undecided_p0[w] / max(pairs, 1):.3f} %)")


if __name__ == "__main__":
    main()
