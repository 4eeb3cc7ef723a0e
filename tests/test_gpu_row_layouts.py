"""GPU: the two load-time row layouts against the oracle on the hand-built cases of
row_layout_cases.py - rpm rows that carry their arch / CPE / ksplice predicates inline
(ROW_INLINE, read by inline_pass) next to rows of the same kinds that do not fit, and library
keys split by version class (SLOT_CLS_SPLIT, read through slot_rows in the probe) - through the
batch path and the drop-in path.  Every test asserts the layout it ran (DB.layout_stats) and
that its cases still hold matches and non-matches where a wrong layout would show."""
import collections

import numpy as np
import pytest

import row_layout_cases as rc
from conftest import canon
from test_row_layouts_host import check_sum, class_cases, class_expectations, db_of, rpm_cases, rpm_expectations

pytestmark = pytest.mark.gpu


def _batch_hits(mb, db, firsts):
    """Counter of (bucket, package index in its add, VulnerabilityID) over the batch's pairs;
    firsts: [(bucket, first index, count)]."""
    from trivy_amd.batch import advisory_vuln_id
    out = collections.Counter()
    pairs = mb.pairs().astype(np.int64)
    for bucket, first, n in firsts:
        seg = pairs[(pairs[:, 0] >= first) & (pairs[:, 0] < first + n)]
        out.update((bucket, int(a) - first, advisory_vuln_id(db, int(b))) for a, b in seg)
    return out


def test_inline_predicates_vs_oracle(oracle_built):
    import trivy_amd
    from trivy_amd.batch import MatchBatch
    from trivy_amd.detector import ospkg
    c = rpm_cases()
    want = rpm_expectations(c)  # asserts per key: matches, and predicate rejections at a passing version
    db = db_of(c.records)
    st = db.layout_stats()
    check_sum(st)
    assert st["inline_rows"] == c.inline_rows > 0 and st["interval_rows"] == c.interval_rows > c.inline_rows
    hit_keys = {v["PkgName"] for vs in want.values() for v in vs}
    assert {"rh-cpe-65534", "rh-cpe-65535", "rh-tie16"} <= hit_keys
    eng = trivy_amd.Engine(db, 0)
    # drop-in path
    got = []
    for rel in (8, 9):
        got += ospkg.Scanner(eng, "redhat").detect(str(rel), None, [p for p in c.packages["Red Hat"] if p["_rel"] == rel])
    assert canon(got) == canon(want["Red Hat"])
    assert canon(ospkg.Scanner(eng, "rocky").detect("9", None, c.packages["rocky 9"])) == canon(want["rocky 9"])
    assert canon(ospkg.Scanner(eng, "oracle").detect("8", None, c.packages["Oracle Linux 8"])) == \
        canon(want["Oracle Linux 8"])
    # batch path: one batch of the three buckets
    mb = MatchBatch(eng)
    firsts = []
    for bucket, pkgs in c.packages.items():
        names = [p["Name"].encode() for p in pkgs]
        vers = [rc.rpm_version(p).encode() for p in pkgs]
        arches = [p.get("Arch", "").encode() for p in pkgs]
        if bucket == "Red Hat":
            sets, ids = {}, []
            for p in pkgs:
                k = rc.rh_cpe_key(p)
                if k not in sets:
                    sets[k] = mb.cpe_set(list(k[0]), k[1])
                ids.append(sets[k])
            first = mb.add_many(bucket, names, vers, arches=arches, cpe_sets=np.array(ids, np.uint32))
        elif bucket == "Oracle Linux 8":
            first = mb.add_many(bucket, names, vers, ksplice=True)
        else:
            first = mb.add_many(bucket, names, vers, arches=arches)
        firsts.append((bucket, first, len(pkgs)))
    total, errp, bits = mb.run()
    assert errp == -1 and bits == 0
    from_batch = _batch_hits(mb, db, firsts)
    from_oracle = collections.Counter((b, int(v["PkgID"][1:]), v["VulnerabilityID"]) for b, vs in want.items() for v in vs)
    assert from_batch == from_oracle
    assert total == sum(from_oracle.values()) > 100
    mb.close()


@pytest.mark.parametrize("eco", ["pip", "npm"])
def test_class_split_vs_oracle(eco):
    import trivy_amd
    from test_gpu_parity import variants
    from trivy_amd._lib import lib
    from trivy_amd.batch import MatchBatch
    from trivy_amd.detector import library
    c = class_cases(eco)
    # per class matches and non-matches on the split keys; the |A| = 0 key: no class-0 match
    want, hits = class_expectations(c)
    db = db_of(c.records)
    st = db.layout_stats()
    check_sum(st)
    assert st["split_keys"] == c.split_keys == 3 and st["class0_dup_rows"] == c.class0_dup_rows > 0
    eng = trivy_amd.Engine(db, 0)
    assert canon(library.detect(eng, c.lang, c.packages)) == canon(want)
    n = len(c.packages)
    assert n < 256  # with the Maven package: one tile
    names = [p["Name"].encode() for p in c.packages]
    vers = [p["Version"].encode() for p in c.packages]
    from_oracle = collections.Counter((eco, int(i[1:]), v) for (i, v), k in hits.items() for _ in range(k))

    def run(with_maven):
        mb = MatchBatch(eng)
        firsts = [(eco, mb.add_many(eco + "::", names, vers), n)]
        if with_maven:
            mb.add_many("maven::", [rc.MAVEN_PKG["Name"].encode()], [rc.MAVEN_PKG["Version"].encode()])
        total, errp, bits = mb.run()
        assert errp == -1 and bits == 0
        pairs = mb.pairs().copy()
        got = _batch_hits(mb, db, firsts)
        mb.close()
        return pairs, got, lib().tvm_engine_last_variant(eng.h)

    vs = variants(grammar_set=8)
    assert len(vs) >= 5
    try:
        ref = None
        for v in [0] + [v for v in vs if v]:
            lib().tvm_engine_set_variant(eng.h, v)
            pairs, got, _ = run(False)
            assert got == from_oracle, lib().tvm_variant_name(v)
            ref = pairs if ref is None else ref
            assert np.array_equal(pairs, ref), lib().tvm_variant_name(v)
    finally:
        lib().tvm_engine_set_variant(eng.h, 0)
    # one Maven package in the tile: the all-grammar kernel sweeps the same pip / npm packages
    _, _, lean_v = run(False)
    pairs, got, all_v = run(True)
    sets = lib().tvm_variant_grammar_sets
    assert lean_v != all_v and sets(lean_v) & 8 and not sets(lean_v) & 4 and sets(all_v) & 4
    assert got == from_oracle
    assert np.array_equal(pairs[pairs[:, 0] < n], ref)
    assert len(pairs) == len(ref) + 1 and int(pairs[-1, 0]) == n  # the Maven package's own match


def test_split_key_with_32768_rows_vs_oracle():
    """A pip key of 16384 advisories "<i.0": 32768 rows, the first size at which the packed
    |A| | |B| << 16 count of a split key ran into the split mark (bit 31), so that the key kept
    a list B of 0 rows and every package of a class other than 0 matched nothing.  Passes only
    with the guard in DB::split_by_class (a key of 0x8000 rows or more stays one list); next to
    it the largest key that is still split, 16383 advisories."""
    import oracle.drivers as od
    import oracle.library as ol
    import trivy_amd
    from trivy_amd.detector import library
    recs, rows = rc.big_key_records(16384)
    edge, edge_rows = rc.big_key_records(16383, name="edge")
    recs += edge[1:]
    db = db_of(recs)
    st = db.layout_stats()
    check_sum(st)
    assert (rows, edge_rows) == (32768, 32766) and st["interval_rows"] == rows + edge_rows
    assert (st["split_keys"], st["class0_dup_rows"]) == (1, 16383)  # "edge" alone
    vers = ["5.0", "5.0rc1", "5.0+l", "5.0.post1", "16000.0rc1", "16383.0.dev1", "0.0", "20000.0rc1+x"]
    pkgs = [{"ID": f"p{i}", "Name": "big", "Version": v} for i, v in enumerate(vers)]
    pkgs += [{"ID": f"e{i}", "Name": "edge", "Version": v} for i, v in enumerate(["16000.0", "5.0rc1"])]
    want = ol.detect(od.Records(recs), "pip", pkgs)
    per = collections.Counter(v["PkgID"] for v in want)
    assert [per[f"p{i}"] for i in range(8)] == [16378, 16378, 16378, 16378, 383, 0, 16383, 0]
    assert [per[f"e{i}"] for i in range(2)] == [382, 16377]  # through list A, through list B
    # what a truncated list B loses: packages of a class other than 0 with many matches
    assert sum(1 for i in (1, 2, 3) if per[f"p{i}"] > 10000) >= 3
    eng = trivy_amd.Engine(db, 0)
    assert canon(library.detect(eng, "pip", pkgs)) == canon(want)
