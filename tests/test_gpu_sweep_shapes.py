"""GPU: the hot-row sweep with the package windows indexed by nz rank and the pair test as one
lexicographic compare (fused_k4_m2400_wseg_rec_r16, sweep_seg REC) against the parent's sweep
(fused_k4_m2400_wseg_r16), "auto" and the Python oracle, over tiles whose pair totals sit on the
edges of the sweep's loops: 1, 63 / 64 / 65 (a wave's 64-pair unit), 255 / 256 / 257 (the four
waves' shares), 1023 / 1024 / 1025 (a round of K x 64 per wave), 4096 / 4097 (the pair map starts
to share entries) and tiles with a 10 000-row key (the per-wave match buffer overflows: the direct
re-sweep).  The tiles hold a single package with rows, 256 packages with rows, keys with prefix
lengths 0 and 7, a bound that equals its key's prefix, unfixed rows, window ties and versions
below / inside / above the prefix or unparsable.  A dpkg-grammar DB cannot hold a ROW_ALWAYS row
or an R16_FALLBACK row in a dpkg key's run: those are covered on the host (test_row16_lex_host)."""
import collections
import functools

import numpy as np
import pytest

import row16_cases as c
from test_gpu_row16 import hits_of, run_pairs, variant_index

pytestmark = pytest.mark.gpu

NEW, PARENT = "fused_k4_m2400_wseg_rec_r16", "fused_k4_m2400_wseg_r16"
AUTO = NEW  # what "auto" launches for a dpkg-only batch (match_variants.h kAutoVariant)
SIZES = (17, 16, 5, 4, 3, 2, 1)
SPECIAL = {  # key -> fixed versions ("" = unfixed)
    "p0": ["1:1.0-1", "2.0-1"],                                  # no common byte: P = 0
    "p7": ["1.2.3-1", "1.2.3-2", "1.2.3-1+deb12u1", ""],         # P = 7 (capped), an unfixed row
    "one-short": ["1", ""],                                      # the bound is the prefix
    "beyond": ["1.2.3-1ubuntu0.1", "1.2.3-1ubuntu0.3"],          # 23-byte keys that differ past the window
}
# the special packages of a tile, each with its version pinned, and what the hot rows of its key
# must say about it (db.row16_eval: [(path, matches)], path 1 = a window tie, the full row decides)
PINNED = [
    ("p0", "1:0.1", [(0, 1), (0, 0)]),                           # inside the first bound, above the second
    ("p7", "1.2.3-1+deb12u1", [(0, 0), (0, 1), (1, 0), (0, 1)]),  # equal to a bound that runs past the window: a tie
    ("p7", "x", [(0, 0)] * 4),                                   # unparsable: not even the unfixed row
    ("one-short", "0.5", [(0, 1), (0, 1)]),                      # below the prefix, the bound IS the prefix: (0,0) <= (0,0)
    ("one-short", "1", [(0, 0), (0, 1)]),                        # equal to that bound: empty window, length 0 - a miss
    ("one-short", "3", [(0, 0), (0, 1)]),                        # above the prefix: only the unfixed row
    ("beyond", "1.2.3-1ubuntu0.2", [(1, 0), (1, 1)]),            # ties both windows: the full rows decide
]
N_SPECIAL = sum(len(SPECIAL[k]) for k, _, _ in PINNED)
BIG = 10000
VERS = ["0.5", "1", "1.2.0-1", "1.2.3", "1.2.3-1", "1.2.3-2", "1.2.3-1+deb12u1", "1.2.3-1ubuntu0.2", "1.2.3-1ubuntu0.1",
        "1.2.3-1ubuntu0.3", "1.2.9-1", "1.2.16-1", "1.3", "2.0-1", "3", "1:0.1", "1:1.0-1", "2:0", "x", c.BAD, "0"]


def all_records():
    recs = [c._rec(("data-source", c.DEB), {"ID": "debian", "Name": c.DEB, "URL": "https://x"})]
    for n in SIZES:
        for i in range(n):
            recs.append(c._rec((c.DEB, f"rows-{n}", c.vuln_id(i)), {"FixedVersion": f"1.2.{i}-1"}))
    for key, fixed in SPECIAL.items():
        for i, f in enumerate(fixed):
            recs.append(c._rec((c.DEB, key, c.vuln_id(i)), {"FixedVersion": f}))
    for i in range(BIG):
        recs.append(c._rec((c.DEB, "big", f"CVE-2023-{i:05d}"), {"FixedVersion": "" if i % 97 == 0 else f"5.10.{i}-1+deb12u{i % 3}"}))
    return recs


@functools.lru_cache(maxsize=None)
def world():
    import oracle.drivers as od
    import trivy_amd
    recs = all_records()
    db = trivy_amd.DB()
    db.put_records(recs)
    db.finalize()
    st = db.row16_stats()
    assert st["fallback_rows"] == 0 and st["keys_by_p"][0] >= 1 and st["keys_by_p"][7] >= 1
    return db, trivy_amd.Engine(db, 0), od.Records(recs)


def compose(total, special):
    """Key names of one tile whose rows add up to `total` (greedy over the rows-N keys)."""
    keys = [(k, v) for k, v, _ in PINNED] if special else []
    left = total - (N_SPECIAL if special else 0)
    assert left >= 0
    for n in SIZES:
        keys += [f"rows-{n}"] * (left // n)
        left %= n
    assert len(keys) <= 256, (total, len(keys))
    return keys


def tile(keys, salt):
    """256 packages: the keys spread among absent names, versions cycling through VERS except the
    pinned ones ((key, version) entries)."""
    ents = keys + ["absent"] * (256 - len(keys))
    ents = ents[salt % 7:] + ents[:salt % 7]
    names = [e if isinstance(e, str) else e[0] for e in ents]
    return names, [VERS[(i * 5 + salt) % len(VERS)] if isinstance(e, str) else e[1] for i, e in enumerate(ents)]


TILES = {
    "1": compose(1, False), "63": compose(63, False), "64": ["rows-1"] * 64, "65": compose(65, True),
    "255": compose(255, True), "256-all": ["rows-1"] * 256, "257-all": ["rows-1"] * 255 + ["rows-2"],
    "1023": compose(1023, True), "1024-all": ["rows-4"] * 256, "1025": compose(1025, True),
    "4096-all": ["rows-16"] * 256, "4096": compose(4096, True), "4097": compose(4097, True),
    "big": ["big", "big"] + compose(200, True), "big-alone": ["big"],
}
TOTALS = {"256-all": 256, "257-all": 257, "1024-all": 1024, "4096-all": 4096, "big": 2 * BIG + 200, "big-alone": BIG}
BATCHES = [(k,) for k in TILES] + [("4097", "65"), ("1", "big"), ("1024-all", "1023")]


def rows_of(key):
    key = key if isinstance(key, str) else key[0]
    return BIG if key == "big" else len(SPECIAL[key]) if key in SPECIAL else int(key.split("-")[1])


def test_tiles_hold_their_totals():
    for name, keys in TILES.items():
        assert sum(rows_of(k) for k in keys) == TOTALS.get(name) or sum(rows_of(k) for k in keys) == int(name.split("-")[0]), name
    assert len(TILES["1"]) == 1 and len(TILES["256-all"]) == len(TILES["4096-all"]) == 256
    for name in ("65", "255", "1023", "1025", "4096", "4097", "big"):  # every special tile holds every pinned package
        n, v = tile(TILES[name], 5)
        assert sorted((a, b) for a, b in zip(n, v) if a in SPECIAL) == sorted((k, ver) for k, ver, _ in PINNED), name


def test_pinned_packages_take_their_paths():
    """The strict outcomes the special tiles are there for, from the host evaluator of the same rows."""
    import trivy_amd
    db = trivy_amd.DB()
    db.put_records(all_records())
    db.finalize()
    for key, ver, want in PINNED:
        assert db.row16_eval(c.DEB, key, ver) == want, (key, ver)


@pytest.mark.parametrize("batch", BATCHES, ids=["+".join(b) for b in BATCHES])
def test_shapes_vs_oracle(batch, oracle_built):
    import oracle.drivers as od
    db, eng, recs = world()
    names, vers = [], []
    for t, name in enumerate(batch):
        n, v = tile(TILES[name], 3 * t + len(name))
        if name.startswith("big"):  # one below every bound (10 000 matches: thousands per wave segment), one above
            v[n.index("big")] = "5.9"
            if n.count("big") > 1:
                v[n.index("big") + 1] = "6.1"
        if name == "1":  # the tile's one pair is a match
            v[n.index("rows-1")] = "0.5"
        names += n
        vers += v
    pkgs = [{"ID": f"p{i}", "Name": n, "SrcName": n, "Version": v, "SrcVersion": v} for i, (n, v) in enumerate(zip(names, vers))]
    want = collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in od.debian_detect(recs, "12", None, pkgs))
    assert max(want.values()) == 1
    if "big" in batch or "big-alone" in batch:
        assert max(collections.Counter(p for p, _ in want).values()) == BIG  # > 600 matches in every wave segment
    new, ran_new = run_pairs(eng, c.DEB, names, vers, variant_index(NEW))
    old, ran_old = run_pairs(eng, c.DEB, names, vers, variant_index(PARENT))
    auto, ran_auto = run_pairs(eng, c.DEB, names, vers, 0)
    assert (ran_new, ran_old, ran_auto) == (NEW, PARENT, AUTO)
    assert np.array_equal(new, old) and np.array_equal(new, auto)
    assert hits_of(db, new) == want
