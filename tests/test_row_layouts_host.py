"""CPU: the two load-time row layouts (ROW_INLINE rpm rows, SLOT_CLS_SPLIT library keys) are
built for exactly the hand-built cases of row_layout_cases.py that must get them
(DB.layout_stats), the packed |A| | |B| << 16 row count of a split key loses no rows at any
key size, and the case tables themselves keep what the GPU tests rely on: the oracle has
matches and non-matches for every shape and every version class."""
import collections
import ctypes
import functools

import numpy as np
import pytest

import row_layout_cases as rc


def db_of(records):
    import trivy_amd
    db = trivy_amd.DB()
    db.put_records(records)
    return db.finalize()


def rows_many(db, bucket, names):
    """tvm_db_rows_many: the interval rows of each key of one bucket."""
    from trivy_amd._lib import lib
    from trivy_amd.batch import arena_of
    arena, ((off, ln),) = arena_of([n.encode() for n in names])
    out = np.zeros(len(names), np.uint32)
    assert lib().tvm_db_rows_many(db.h, bucket.encode(), len(names), arena, off.ctypes.data, ln.ctypes.data,
                                  out.ctypes.data) == 0
    return [int(x) for x in out]


def check_sum(st):
    assert st["rows"] == st["pad_rows"] + st["interval_rows"] + st["class0_dup_rows"], st


@functools.lru_cache(maxsize=None)
def rpm_cases():
    return rc.RpmCases()


@functools.lru_cache(maxsize=None)
def class_cases(eco):
    return rc.ClassCases(eco)


# ---- layout counts -----------------------------------------------------------------------------

def test_rpm_layout_counts():
    c = rpm_cases()
    st = db_of(c.records).layout_stats()
    check_sum(st)
    assert st["inline_rows"] == c.inline_rows and 0 < c.inline_rows < c.interval_rows
    assert st["split_keys"] == 0 and st["class0_dup_rows"] == 0
    db = db_of(c.records)
    total = 0
    for bucket in ("Red Hat", "rocky 9", "Oracle Linux 8"):
        names = [k for k, v in c.keys.items() if v["bucket"] == bucket]
        got = rows_many(db, bucket, names)
        assert got == [c.keys[k]["rows"] for k in names], bucket
        total += sum(got)
    assert st["interval_rows"] == total == c.interval_rows
    # the shapes marked inline and no others: each key flattened on its own
    for name, k in c.keys.items():
        sub = [r for r in c.records if r["path"][0] in ("data-source", "Red Hat CPE") or r["path"][1] == name]
        s1 = db_of(sub).layout_stats()
        assert (s1["inline_rows"], s1["interval_rows"]) == (k["inline"], k["rows"]), name
    inline_shapes = {k["shape"] for k in c.keys.values() if "shape" in k and "cpe" not in k and k["inline"] == k["rows"]}
    assert rc.RH_SHAPES_INLINE <= inline_shapes
    assert all(na <= 3 and nc <= 3 and na + nc <= rc.INLINE_IDS for na, nc in rc.RH_SHAPES_INLINE)
    assert all(na > 3 or nc > 3 or na + nc > rc.INLINE_IDS for na, nc in set(rc.RH_SHAPES) - rc.RH_SHAPES_INLINE)
    assert [c.keys[f"rh-cpe-{x}"]["inline"] for x in (0xFFFE, 0xFFFF, 70000)] == [1, 0, 0]


@pytest.mark.parametrize("eco", ["pip", "npm"])
def test_class_layout_counts(eco):
    c = class_cases(eco)
    db = db_of(c.records)
    st = db.layout_stats()
    check_sum(st)
    assert st["split_keys"] == c.split_keys and st["class0_dup_rows"] == c.class0_dup_rows
    assert st["inline_rows"] == 0
    names = list(c.specs)
    got = rows_many(db, eco + "::", names)
    assert got == [c.layout[k][1] for k in names]
    assert st["interval_rows"] == sum(got) + rows_many(db, "maven::", [rc.MAVEN_PKG["Name"]])[0] == c.interval_rows
    # the kinds of key the cases must hold: one list, split, split with an empty class-0 list
    assert not c.split["cls-all0"] and c.split["cls-mixed"] and c.split["cls-all"]
    assert c.split["cls-nonzero"] and c.layout["cls-nonzero"][0] == 0
    for key in names:  # each key flattened on its own
        sub = [r for r in c.records if r["path"][0] == "data-source" or r["path"][1] == key]
        s1 = db_of(sub).layout_stats()
        a, b = c.layout[key]
        assert (s1["split_keys"], s1["class0_dup_rows"], s1["interval_rows"]) == \
            (int(c.split[key]), a if c.split[key] else 0, b), key


# ---- packed row counts -------------------------------------------------------------------------

@pytest.mark.parametrize("n_adv,mixed", [(16383, False), (16384, False), (24576, False), (0x7FFF, True)])
def test_packed_row_counts(n_adv, mixed):
    """A split key's two counts share one word with the split mark in bit 31: 32768 rows or more
    must not run into the mark (before the fix the 16384-advisory key reported 0 rows, the
    24576-advisory one 16384, the mixed one 16382)."""
    recs, want = rc.big_key_records(n_adv, mixed)
    assert want == (n_adv * 2 if not mixed else n_adv * 2 - (n_adv + 1) // 2)
    db = db_of(recs)
    st = db.layout_stats()
    check_sum(st)
    assert rows_many(db, "pip::", ["big"]) == [want]
    assert st["interval_rows"] == want
    # a key below 0x8000 rows is split (|A| = one row per "<" advisory), a larger one stays one list
    if want < 0x8000:
        assert (st["split_keys"], st["class0_dup_rows"]) == (1, n_adv)
    else:
        assert (st["split_keys"], st["class0_dup_rows"]) == (0, 0)


# ---- what the GPU tests rely on, from the oracle alone --------------------------------------------

def version_key(grammar, text):
    from trivy_amd._lib import lib
    buf = (ctypes.c_uint8 * 512)()
    n = lib().tvm_version_key(grammar, text.encode(), len(text.encode()), buf, len(buf))
    return None if n < 0 else bytes(buf[:n])


def test_long_keys():
    tie = version_key(3, "-".join(rc.TIE_FIXED))
    assert len(tie) > 16
    for v in rc.TIE_INSTALLED:
        k = version_key(3, f"{v}-{rc.TIE_FIXED[1]}")
        assert len(k) > 16 and k[:16] == tie[:16]
    from trivy_amd._lib import lib
    assert len(version_key(6, rc.PIP_LONG)) > 32
    assert lib().tvm_version_class(6, rc.PIP_LONG.encode(), len(rc.PIP_LONG)) == 2  # pre-release


def rpm_expectations(c):
    """The oracle's DetectedVulnerabilities per bucket, and the checks that keep the rpm cases
    honest: per key matches, and packages a predicate rejects although the version test passes."""
    import oracle.drivers as od
    db = od.Records(c.records)
    want = {"Red Hat": []}
    for rel in (8, 9):
        sub = [p for p in c.packages["Red Hat"] if p["_rel"] == rel]
        want["Red Hat"] += od.driver_detect("redhat", str(rel), None, sub, db, None)
    want["rocky 9"] = od.driver_detect("rocky", "9", None, c.packages["rocky 9"], db, None)
    want["Oracle Linux 8"] = od.driver_detect("oracle", "8", None, c.packages["Oracle Linux 8"], db, None)
    # rows per (key, VulnerabilityID) with their fixed versions, from the records
    rows = collections.defaultdict(list)
    import json
    for r in c.records:
        path = r["path"]
        if path[0] not in want:
            continue
        val = json.loads(r["value"])
        if path[0] == "Oracle Linux 8":
            rows[(path[1], path[2])].append(val["FixedVersion"])
        for e in val.get("Entries", []):
            if path[0] == "Red Hat":
                for cve in e["Cves"]:
                    rows[(path[1], cve.get("ID") or path[2])].append(e["FixedVersion"])
            else:
                rows[(path[1], path[2])].append(e["FixedVersion"])
    assert sum(len(v) for v in rows.values()) == c.interval_rows
    matched, rejected = collections.Counter(), collections.Counter()
    for bucket, pkgs in c.packages.items():
        hits = collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in want[bucket])
        for p in pkgs:
            inst = od.fmt(p)
            for (key, vid), fixed in rows.items():
                if key != p["Name"]:
                    continue
                passes = sum(1 for f in fixed if f == "" or od.rpm_cmp(inst, f) < 0)
                n = hits[(p["ID"], vid)]
                assert n <= passes
                matched[(key, vid)] += n
                rejected[(key, vid)] += passes - n
    for name, k in c.keys.items():
        vids = [vid for (key, vid) in rows if key == name]
        assert sum(matched[(name, v)] for v in vids) > 0, name
        for v in vids:  # every row's predicate rejects someone whose version passes
            assert rejected[(name, v)] > 0, (name, v)
            assert (matched[(name, v)] == 0) == (k.get("never") == v), (name, v)
    return want


def test_rpm_cases_vs_oracle():
    c = rpm_cases()
    want = rpm_expectations(c)
    assert sum(len(v) for v in want.values()) > 100
    assert sum(len(v) for v in c.packages.values()) < 1000


def class_expectations(c):
    """oracle.library.detect over the class packages, and per version class the matched and
    unmatched (package, advisory) pairs on the split keys."""
    import oracle.drivers as od
    import oracle.library as ol
    from trivy_amd._lib import lib
    want = ol.detect(od.Records(c.records), c.lang, c.packages)
    hits = collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in want)
    assert max(hits.values()) == 1
    cls_of = {v: lib().tvm_version_class(c.grammar, v.encode(), len(v.encode())) for v in c.versions}
    assert sorted(set(cls_of.values())) == [-1] + list(range(8 if c.eco == "pip" else 2))
    m, u = collections.Counter(), collections.Counter()
    for p in c.packages:
        cls, key = cls_of[p["Version"]], p["Name"]
        n = sum(hits[(p["ID"], f"CVE-2024-{4000 + j}")] for j in range(len(c.specs[key])))
        assert cls >= 0 or n == 0  # an unparsable version matches nothing here
        if c.split[key] and cls >= 0:
            m[cls] += n
            u[cls] += len(c.specs[key]) - n
        if key == "cls-nonzero" and cls >= 0:
            m[("nz", cls > 0)] += n
            u[("nz", cls > 0)] += 1 - n
    for cls in set(cls_of.values()) - {-1}:
        assert m[cls] > 0 and u[cls] > 0, cls
    # the |A| = 0 key: no class-0 package matches, some other class does
    assert m[("nz", False)] == 0 and u[("nz", False)] > 0 and m[("nz", True)] > 0
    return want, hits


@pytest.mark.parametrize("eco", ["pip", "npm"])
def test_class_cases_vs_oracle(eco):
    """The oracle has both outcomes for every class, and the load-time interval compiler agrees
    with it on every (installed version, advisory) pair of the all-specs key."""
    import json

    import oracle.library as ol
    from trivy_amd._lib import lib
    c = class_cases(eco)
    class_expectations(c)
    pairs = 0
    for v in c.versions:
        for s in c.specs["cls-all"] + ["only-pre"]:
            adv = rc.ONLY_PRE[eco] if s == "only-pre" else {"VulnerableVersions": [s]}
            j = json.dumps(adv).encode()
            got = lib().tvm_lib_is_vulnerable_host(c.grammar, v.encode(), len(v.encode()), j, len(j))
            assert got == int(ol.is_vulnerable(ol.LANG[c.lang][1], v, adv)), (v, s)
            pairs += 1
    assert pairs >= (420 if eco == "pip" else 96)
