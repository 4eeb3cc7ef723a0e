"""GPU: rpm, apk and Amazon Linux matching on the adversarial versions of os_version_cases.py
(what they reach - 16-byte head ties read from the tail slot and from the spill area, 32-byte
ties, equal keys, unparsable versions, AffectedVersion lower bounds, Red Hat merge groups whose
greatest FixedVersion is not the greatest text - is pinned on the CPU by
test_os_versions_host.py).  The oracle's drivers are the only checker: the drop-in path is
compared record by record, the batch path pair by pair under every non-ablation kernel variant
of the OS-grammar and all-grammar sets, one mixed batch against the per-family batches and the
pipelined pass, and one tile in which every key spills."""
import collections
import functools
import random

import numpy as np
import pytest

import os_version_cases as oc
import vulnset_ref as vr
from conftest import canon
from row_layout_cases import MAVEN_ROOT, _rec, rh_cpe_key

pytestmark = pytest.mark.gpu

DEB_ROOT, NPM_ROOT = "debian 12", "npm::GitHub Security Advisory npm"


@functools.lru_cache(maxsize=None)
def extra_targets():
    """A Debian and an npm target for the mixed batch, the npm one with three Maven packages (a
    batch without Maven runs on the kernels built without it; with one, the all-grammar kernel
    takes that tile and the split launch the others): (records, debian packages, npm packages,
    maven packages)."""
    rng = random.Random(77)
    recs = [_rec(("data-source", DEB_ROOT), {"ID": "debian", "Name": "Debian", "URL": "https://d"}),
            _rec(("data-source", NPM_ROOT), {"ID": "ghsa", "Name": NPM_ROOT, "URL": "https://g"}),
            _rec(("data-source", MAVEN_ROOT), {"ID": "ghsa", "Name": MAVEN_ROOT, "URL": "https://g"}),
            _rec((MAVEN_ROOT, "org.example:lib", "CVE-2024-7000"), {"VulnerableVersions": ["<2.0"]})]
    mvn = [{"ID": f"p{i}", "Name": "org.example:lib", "Version": v} for i, v in enumerate(["1.0", "2.1", "1.5-rc1"])]
    deb, npm = [], []
    for j in range(10):
        for k in range(3):
            recs.append(_rec((DEB_ROOT, f"deb-{j}", f"CVE-2024-{50000 + 10 * j + k}"),
                             {"FixedVersion": oc.amzn_version(rng, "1.2.3-4+deb12u1")}))
        recs.append(_rec((NPM_ROOT, f"npm-{j}", f"CVE-2024-{51000 + j}"), {"VulnerableVersions": [f"<1.{j}.0"]}))
    for i in range(60):
        text = oc.amzn_version(rng, "1.2.3-4+deb12u1") or "1"
        deb.append(oc._pkg(i, f"deb-{i % 12}", text))
        npm.append({"ID": f"p{i}", "Name": f"npm-{i % 12}", "Version": f"1.{rng.randint(0, 9)}.{rng.randint(0, 3)}"})
    return recs, deb, npm, mvn


@functools.lru_cache(maxsize=None)
def world():
    """One DB of every family's table (the buckets are disjoint) and one engine."""
    import trivy_amd
    db = trivy_amd.DB()
    db.put_records(oc.all_records() + extra_targets()[0])
    db.finalize()
    return db, trivy_amd.Engine(db, 0)


@functools.lru_cache(maxsize=None)
def oracle_of(fid):
    """Per target the oracle driver's DetectedVulnerabilities (computed once, never changed)."""
    import oracle.drivers as od
    fam = oc.family(fid)
    db = od.Records(fam.records)
    return [od.driver_detect(t.family, t.os_ver, t.repo, t.pkgs, db, None) for t in fam.targets]


@functools.lru_cache(maxsize=None)
def oracle_pairs(fid):
    """Counter of (target, package index, VulnerabilityID) the batch must report: the driver's
    findings; for Red Hat the advisories that enter its merge (redhat.go:122-145), one per pair."""
    import oracle.drivers as od
    fam = oc.family(fid)
    out = collections.Counter()
    if fam.kind == "mariner":  # mariner.go copies no PkgID: the driver asked package by package
        db, t = od.Records(fam.records), fam.targets[0]
        for i, p in enumerate(t.pkgs):
            out.update((0, i, v["VulnerabilityID"]) for v in od.driver_detect(t.family, t.os_ver, None, [p], db, None))
        return out
    if fam.kind != "redhat":
        for ti, vs in enumerate(oracle_of(fid)):
            out.update((ti, int(v["PkgID"][1:]), v["VulnerabilityID"]) for v in vs)
        return out
    db, t = od.Records(fam.records), fam.targets[0]
    for i, p in enumerate(t.pkgs):
        cs, nvr = rh_cpe_key(p)
        inst = od.fmt(p)
        for a in db.get_redhat(p["Name"], list(cs), [nvr]):
            if a["Arches"] and p.get("Arch", "") != "noarch" and p.get("Arch", "") not in a["Arches"]:
                continue
            if a["FixedVersion"] == "" or od.rpm_cmp(inst, a["FixedVersion"]) < 0:
                out[(0, i, a["VulnerabilityID"])] += 1
    return out


def add_rows(mb, fam, t, rows):
    """Adds batch rows (Family.batch_rows) of one target; returns the first index."""
    names = [r[1].encode() for r in rows]
    vers = [r[2].encode() for r in rows]
    arches = [(r[3] or "").encode() for r in rows]
    if fam.kind == "redhat":
        sets, ids = getattr(mb, "_sets", {}), []
        mb._sets = sets
        for r in rows:
            k = rh_cpe_key(t.pkgs[r[0]])
            if k not in sets:
                sets[k] = mb.cpe_set(list(k[0]), k[1])
            ids.append(sets[k])
        return mb.add_many(t.bucket, names, vers, arches=arches, cpe_sets=np.array(ids, np.uint32))
    if fam.kind == "oracle":
        return mb.add_many(t.bucket, names, vers, ksplice=True)
    if fam.kind == "rocky":
        return mb.add_many(t.bucket, names, vers, arches=arches)
    return mb.add_many(t.bucket, names, vers)


def family_batch(eng, fid, maven=False):
    """One MatchBatch of the family's packages (an Amazon batch: and one rpm package, so that it
    runs the OS-grammar kernels); segs: [(target index, first, rows)].  maven: a
    Maven package at the head of every tile of 256, so that the batch holds every grammar and no
    tile qualifies for the kernels built without Maven - the all-grammar kernel sweeps them all."""
    from trivy_amd.batch import MatchBatch
    fam = oc.family(fid)
    mb, segs = MatchBatch(eng), []
    for ti, t in enumerate(fam.targets):
        rows = fam.batch_rows(t)
        if not maven:
            segs.append((ti, add_rows(mb, fam, t, rows), rows))
            if fam.grammar == 1:  # a dpkg-only batch runs the dpkg-only kernels: one rpm package (no such name)
                mb.add_many("alma 9", [b"no-such-package"], [b"1.0-1.el9"])
            continue
        a = 0
        while a < len(rows):
            n = 256 - len(mb) % 256
            if n == 256:
                mb.add_many("maven::", [b"org.example:lib"], [b"1.0"])
                n = 255
            segs.append((ti, add_rows(mb, fam, t, rows[a:a + n]), rows[a:a + n]))
            a += n
    return mb, segs


def hits_of(db, pairs, segs, tag=()):
    """Counter of tag + (target, package index, VulnerabilityID) over the pairs of the segments."""
    from trivy_amd.batch import advisory_vuln_id
    out = collections.Counter()
    pk = pairs[:, 0].astype(np.int64)
    ids = {}
    for ti, first, rows in segs:
        lo, hi = np.searchsorted(pk, [first, first + len(rows)])
        for a, b in pairs[lo:hi].tolist():
            if b not in ids:
                ids[b] = advisory_vuln_id(db, b)
            out[tag + (ti, rows[a - first][0], ids[b])] += 1
    return out


def in_order(pairs):
    p = pairs.astype(np.int64)
    return bool(np.all(np.diff(p[:, 0] * (1 << 32) + p[:, 1]) > 0))


# ------------------------------------------------------------------------------------ drop-in ----
@pytest.mark.parametrize("fid", oc.FAMILY_IDS)
def test_dropin_vs_oracle(oracle_built, fid):
    """Full records: InstalledVersion, the rpm Version.String() form of FixedVersion with the odd
    epochs, and for Red Hat the merged VendorIDs and FixedVersion."""
    from trivy_amd.detector import ospkg
    _, eng = world()
    fam = oc.family(fid)
    n = 0
    for t, want in zip(fam.targets, oracle_of(fid)):
        got = ospkg.Scanner(eng, t.family).detect(t.os_ver, t.repo, t.pkgs)
        assert canon(got) == canon(want), t.bucket
        n += len(want)
    print(fid, "findings compared:", n)
    assert n > 500


# -------------------------------------------------------------------------------------- batch ----
@pytest.mark.parametrize("fid", oc.FAMILY_IDS)
def test_batch_vs_oracle_every_variant(oracle_built, fid):
    from test_gpu_parity import variants
    from trivy_amd._lib import lib
    db, eng = world()
    fam = oc.family(fid)
    want = oracle_pairs(fid)
    assert sum(want.values()) > 500
    sets = lib().tvm_variant_grammar_sets
    n_run = 0
    try:
        # the OS-grammar kernels on the family's packages alone, the all-grammar kernel on the
        # same packages with a Maven package in every tile
        for gset, maven in ((2, False), (4, True)):
            vs = variants(grammar_set=gset)
            assert len(vs) >= 2
            ref = None
            for v in vs:
                name = lib().tvm_variant_name(v).decode()
                lib().tvm_engine_set_variant(eng.h, v)
                mb, segs = family_batch(eng, fid, maven)
                n_mvn = (len(mb) + 255) // 256 if maven else 0
                assert len(mb) - sum(len(rows) for _, _, rows in segs) == (n_mvn if maven else int(fam.grammar == 1))
                total, errp, bits = mb.run()
                assert errp == -1 and bits == 0, name
                ran = lib().tvm_engine_last_variant(eng.h)  # variant 0 picks one itself
                assert (ran == v or v == 0) and sets(ran) & gset, name
                pairs = mb.pairs().copy()
                assert in_order(pairs), name
                if ref is None or not np.array_equal(pairs, ref):
                    assert hits_of(db, pairs, segs) == want, name
                    assert total == sum(want.values()) + n_mvn, name  # each Maven package: its one advisory
                    assert ref is None, name  # every variant: the same pairs in the same order
                    ref = pairs
                if fam.kind == "redhat":
                    t = fam.targets[0]
                    got = mb.redhat_result({first + k: t.pkgs[r[0]] for _, first, rows in segs for k, r in enumerate(rows)})
                    assert canon(got) == canon(oracle_of(fid)[0]), name
                mb.close()
                n_run += 1
    finally:
        lib().tvm_engine_set_variant(eng.h, 0)
    print(fid, "pairs compared:", sum(want.values()), "variants:", n_run)


# -------------------------------------------------------------------------------- mixed batch ----
def mixed_batch(eng):
    """Every family interleaved in targets of 7 to 300 packages, one Debian and one npm target
    among them; returns (batch, per family segments [(target, first, rows)], first index of the
    debian / npm / maven targets)."""
    from trivy_amd.batch import MatchBatch
    rng = random.Random(5)
    mb = MatchBatch(eng)
    todo = []
    for fid in oc.FAMILY_IDS:
        fam = oc.family(fid)
        for ti, t in enumerate(fam.targets):
            rows, a = fam.batch_rows(t), 0
            while a < len(rows):
                n = rng.choice([7, 31, 64, 100, 255, 256, 257, 300])
                todo.append((fid, ti, rows[a:a + n]))
                a += n
    rng.shuffle(todo)
    segs = collections.defaultdict(list)
    _, deb, npm, mvn = extra_targets()
    firsts = {}
    for k, (fid, ti, rows) in enumerate(todo):
        if k == len(todo) // 3:
            firsts["deb"] = mb.add_many(DEB_ROOT, [p["SrcName"].encode() for p in deb],
                                        [oc._fmt(0, p["SrcVersion"], p["SrcRelease"]).encode() for p in deb])
        if k == 2 * len(todo) // 3:
            firsts["npm"] = mb.add_many("npm::", [p["Name"].encode() for p in npm], [p["Version"].encode() for p in npm])
            firsts["mvn"] = mb.add_many("maven::", [p["Name"].encode() for p in mvn], [p["Version"].encode() for p in mvn])
        fam = oc.family(fid)
        segs[fid].append((ti, add_rows(mb, fam, fam.targets[ti], rows), rows))
    return mb, segs, firsts


def test_mixed_batch(oracle_built):
    import oracle.drivers as od
    import oracle.library as ol
    from trivy_amd._lib import lib
    from trivy_amd.batch import advisory_vuln_id
    db, eng = world()
    recs, deb, npm, mvn = extra_targets()
    mb, segs, firsts = mixed_batch(eng)
    total, errp, bits = mb.run()
    assert errp == -1 and bits == 0
    assert lib().tvm_variant_grammar_sets(lib().tvm_engine_last_variant(eng.h)) & 4  # the all-grammar kernel ran
    pairs = mb.pairs().copy()
    assert in_order(pairs)
    # every pair against the oracle
    want, got = collections.Counter(), collections.Counter()
    for fid in oc.FAMILY_IDS:
        want.update({(fid,) + k: n for k, n in oracle_pairs(fid).items()})
        got.update(hits_of(db, pairs, sorted(segs[fid], key=lambda s: s[1]), tag=(fid,)))
    extra = od.Records(recs)
    want.update(("deb", 0, int(v["PkgID"][1:]), v["VulnerabilityID"]) for v in od.driver_detect("debian", "12", None, deb, extra, None))
    want.update(("npm", 0, int(v["PkgID"][1:]), v["VulnerabilityID"]) for v in ol.detect(extra, "npm", npm))
    want.update(("mvn", 0, int(v["PkgID"][1:]), v["VulnerabilityID"]) for v in ol.detect(extra, "jar", mvn))
    for tag, n in (("deb", len(deb)), ("npm", len(npm)), ("mvn", len(mvn))):
        got.update(hits_of(db, pairs, [(0, firsts[tag], [(i,) for i in range(n)])], tag=(tag,)))
    assert got == want
    assert sum(got.values()) == total == len(pairs)
    assert sum(1 for k in got if k[0] == "deb") > 10 and sum(1 for k in got if k[0] == "npm") > 10
    assert sum(1 for k in got if k[0] == "mvn") == 2
    # a package's advisories do not depend on its neighbours: the per-family batches, same engine
    pk = pairs[:, 0].astype(np.int64)
    for fid in oc.FAMILY_IDS:
        fb, fsegs = family_batch(eng, fid)
        assert fb.run()[1:] == (-1, 0)
        fp = fb.pairs().copy()
        fb.close()
        fpk = fp[:, 0].astype(np.int64)
        alone = {}
        for ti, first, rows in fsegs:
            for k, r in enumerate(rows):
                lo, hi = np.searchsorted(fpk, [first + k, first + k + 1])
                alone[(ti, r[0])] = fp[lo:hi, 1].tolist()
        for ti, first, rows in segs[fid]:
            for k, r in enumerate(rows):
                lo, hi = np.searchsorted(pk, [first + k, first + k + 1])
                assert pairs[lo:hi, 1].tolist() == alone[(ti, r[0])], (fid, ti, r)
    mb.close()
    # the pipelined pass returns the device-resident list
    mb, _, _ = mixed_batch(eng)
    mb.pipeline_prepare(match_cap=total, chunk_packages=1024)
    got_total, errp, _ = mb.pipeline_run()
    assert errp == -1 and got_total == total
    adv, row_end = mb.pipeline_csr()
    assert np.array_equal(adv, pairs[:, 1])
    assert np.array_equal(row_end, np.cumsum(np.bincount(pk, minlength=len(mb))).astype(np.uint32))
    mb.close()
    # and with the Red Hat merge inside the pass: the set tvm_match_vulns builds from the resident list
    keys = vr.Keys()
    dev, _, _ = mixed_batch(eng)
    assert dev.run()[1:] == (-1, 0)
    vs = dev.vulns()
    want_set = vr.gpu_side(vs, keys)
    vs.close()
    dev.close()
    mb, _, _ = mixed_batch(eng)
    mb.pipeline_prepare(match_cap=total, chunk_packages=1024, rh_merge=True)
    got_total, errp, _ = mb.pipeline_run()
    assert errp == -1 and got_total == total
    vs = mb.vulns(pipeline=True)
    got_set = vr.gpu_side(vs, keys)
    assert vs.n_grp_recs > 0 and len(got_set[0]) < total  # the merge removed something
    vs.close()
    mb.close()
    assert np.array_equal(got_set[0], want_set[0]) and np.array_equal(got_set[1], want_set[1])
    print("mixed batch: packages", len(pk) and int(pk.max()) + 1, "pairs", total, "merged set", len(got_set[0]))
    assert advisory_vuln_id(db, int(pairs[0, 1])) is not None


# --------------------------------------------------------------------------- every key spills ----
def test_every_package_spills(oracle_built):
    """One tile of 256 rpm packages, every key over 32 bytes (test_os_versions_host.py): each is
    encoded a second time into the scratch Engine::scratch_words sized, and its ties with the
    FixedVersions on the 16-byte head are decided from there."""
    import oracle.drivers as od
    import trivy_amd
    from test_gpu_parity import variants
    from trivy_amd._lib import lib
    from trivy_amd.batch import MatchBatch
    from trivy_amd.detector import ospkg
    fam = oc.spill_tile()
    t = fam.targets[0]
    db = trivy_amd.DB()
    db.put_records(fam.records)
    db.finalize()
    eng = trivy_amd.Engine(db, 0)
    want = od.driver_detect(t.family, t.os_ver, None, t.pkgs, od.Records(fam.records), None)
    per = collections.Counter(v["PkgID"] for v in want)
    assert 300 < len(want) < 4 * 256 - 100 and len(per) > 128  # matches and non-matches on most packages
    assert canon(ospkg.Scanner(eng, t.family).detect(t.os_ver, None, t.pkgs)) == canon(want)
    want_pairs = collections.Counter((0, int(v["PkgID"][1:]), v["VulnerabilityID"]) for v in want)
    rows = fam.batch_rows(t)
    assert len(rows) == 256
    try:
        for v in variants(grammar_set=2):
            lib().tvm_engine_set_variant(eng.h, v)
            mb = MatchBatch(eng)
            first = add_rows(mb, fam, t, rows)
            total, errp, bits = mb.run()
            assert errp == -1 and bits == 0, lib().tvm_variant_name(v)  # bits: ERR_SPILL when the scratch is short
            assert hits_of(db, mb.pairs(), [(0, first, rows)]) == want_pairs, lib().tvm_variant_name(v)
            mb.close()
    finally:
        lib().tvm_engine_set_variant(eng.h, 0)
