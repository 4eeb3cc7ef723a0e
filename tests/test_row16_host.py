"""CPU: the 16-byte hot rows of the dpkg grammar (csrc/common.h Row16; DB::rows16).  For every
(installed version, row) of the hand-built cases of row16_cases.py the shared compare
(tvm_row16_eval_host: the code the hot-row sweep runs per pair) must equal the byte order of the
full sort keys (tvm_version_key) and the oracle's Debian / Ubuntu / Amazon drivers, and every
deciding path - the hot row, a window tie that falls back to the 32-byte row - must occur."""
import collections
import functools

import pytest

import row16_cases as c


def lcp(keys):
    if not keys:
        return 0
    lo, hi = min(keys), max(keys)
    n = 0
    while n < len(lo) and n < len(hi) and lo[n] == hi[n]:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def db():
    import trivy_amd
    d = trivy_amd.DB()
    d.put_records(c.records())
    return d.finalize()


def key_rows(bucket, key):
    """[(advisory index j, fixed version)] of the rows of a key, in row (= advisory) order."""
    return [(j, f) for j, f in enumerate(c.KEYS[key]) if c.has_row(bucket, f)]


def expected_p(bucket, key):
    bounds = [c.version_key(f) for _, f in key_rows(bucket, key) if f]
    return min(c.P_CAP, lcp(bounds), min((len(b) for b in bounds), default=0))


def test_layout():
    st = db().row16_stats()
    by_p = collections.Counter()
    rows = 0
    for bucket in (c.DEB, c.UBU, c.AMZ):
        for key in c.KEYS:
            by_p[expected_p(bucket, key)] += 1
            rows += len(key_rows(bucket, key))
    assert st["keys_by_p"] == [by_p[p] for p in range(8)]
    # the prefix lengths the cases are there for: none, short, the cap
    assert by_p[0] >= 2 and by_p[2] and by_p[5] and by_p[6] and by_p[7] >= 4
    assert expected_p(c.DEB, "p0-epochs") == 0 and expected_p(c.DEB, "p0-unfixed") == 0
    assert expected_p(c.DEB, "p7-capped") == 7 < lcp([c.version_key(f) for f in c.KEYS["p7-capped"] if f])
    assert expected_p(c.DEB, "one-short") == len(c.version_key("1")) == 6  # the bound is the prefix
    # every dpkg row has a hot row; nothing falls back by its code
    assert (st["hot_rows"], st["fallback_rows"]) == (rows, 0)
    ls = db().layout_stats()
    assert ls["rows"] == ls["pad_rows"] + ls["interval_rows"] + ls["class0_dup_rows"] and ls["interval_rows"] == rows


def test_keys_hold_the_cases():
    """What the compare cases rely on, from the encoder alone."""
    k = c.version_key
    assert 0 in k("256.0-1")[1:] and k("0:256.0-1") == k("256.0-1") and k("1.0-1")[0] == 0  # 0x00: numbers, epoch 0
    a, b = k("1.2.3-1ubuntu0.1"), k("1.2.3-1ubuntu0.3")
    assert lcp([a, b]) >= c.P_CAP + c.WINDOW and len(a) > c.P_CAP + c.WINDOW  # differ only past the window
    assert len(k("1.2-1")) <= c.P_CAP + c.WINDOW < len(k("1.2.3-1+deb12u1"))  # a bound inside / beyond the window
    assert len(k(c.LONG)) > 32 and k(c.LONG_LO) < k(c.LONG) < k(c.LONG_HI)
    assert k(c.BAD) is None and k("x1.0") is None and k("") is None
    assert len(k("1")) < c.P_CAP  # an installed key shorter than a 7-byte prefix


@pytest.mark.parametrize("bucket", [c.DEB, c.UBU, c.AMZ])
def test_compare_vs_full_keys(bucket):
    paths = collections.Counter()
    seen = collections.Counter()
    for key in c.KEYS:
        rows = key_rows(bucket, key)
        P = expected_p(bucket, key)
        pre = next((c.version_key(f)[:P] for _, f in rows if f), b"")
        for v in c.INSTALLED:
            got = db().row16_eval(bucket, key, v)
            assert got is not None and len(got) == len(rows), (key, v)
            ik = c.version_key(v)
            for (path, res), (j, f) in zip(got, rows):
                want = ik is not None and (f == "" or ik < c.version_key(f))  # bytes order = key_cmp
                assert res == int(want), (bucket, key, v, f, path)
                paths[path] += 1
                if ik is None:
                    seen["invalid"] += 1
                    continue
                if f == "":
                    seen["unfixed"] += 1
                    continue
                fk = c.version_key(f)
                n = P + c.WINDOW
                tie = ik[:n] == fk[:n] and len(ik) > n and len(fk) > n
                assert path == (1 if tie else 0), (bucket, key, v, f)
                if ik[:P] != pre:  # decided by the key's prefix alone
                    seen["below" if ik < pre else "above"] += 1
                if len(ik) < P:
                    seen["shorter-than-prefix"] += 1
                if ik == fk:
                    seen["equal-inside" if len(fk) <= n else "equal-beyond"] += 1
                if tie and ik != fk:
                    seen["tie-lt" if ik < fk else "tie-gt"] += 1
                if len(fk) == P:
                    seen["bound-is-prefix"] += 1
                if 0 in ik[1:n] or 0 in fk[1:n]:
                    seen["zero-byte"] += 1
                if len(ik) > 32:
                    seen["spill"] += 1
    assert paths[0] > 0 and paths[1] > 0 and paths[2] == 0, paths  # dpkg rows never carry the FALLBACK code
    for what in ("below", "above", "shorter-than-prefix", "equal-inside", "equal-beyond", "tie-lt", "tie-gt",
                 "bound-is-prefix", "zero-byte", "spill", "unfixed", "invalid"):
        if what == "unfixed" and bucket == c.AMZ:  # amazon.go skips an advisory without a fixed version: no row
            assert seen[what] == 0
            continue
        assert seen[what] > 0, (what, seen)
    for name in c.ABSENT:
        assert db().row16_eval(bucket, name, "1.0") is None
    assert db().row16_eval("no such bucket", "p2-majors", "1.0") is None


def test_fallback_code_on_other_grammars():
    """Rows of other grammars (here an rpm key with a predicate, an apk key with a lower bound) get
    the FALLBACK code, and the evaluator's full-row path decides them."""
    import trivy_amd
    recs = [c._rec(("alpine 3.19", "musl", "CVE-2024-1"), {"FixedVersion": "1.2.4-r2", "AffectedVersion": "1.2.0-r0"}),
            c._rec(("Photon OS 4.0", "curl", "CVE-2024-2"), {"FixedVersion": "8.0-1.ph4"})]
    d = trivy_amd.DB()
    d.put_records(recs)
    d.finalize()
    st = d.row16_stats()
    assert (sum(st["keys_by_p"]), st["hot_rows"], st["fallback_rows"]) == (0, 0, 2)
    assert d.row16_eval("alpine 3.19", "musl", "1.2.3-r0") == [(2, 1)]
    assert d.row16_eval("alpine 3.19", "musl", "1.1.0-r0") == [(2, 0)]
    assert d.row16_eval("alpine 3.19", "musl", "1.2.4-r2") == [(2, 0)]
    assert d.row16_eval("Photon OS 4.0", "curl", "7.9-1.ph4") == [(2, 1)]
    assert d.row16_eval("Photon OS 4.0", "curl", "8.0-1.ph4") == [(2, 0)]


def oracle_hits(bucket, pkgs):
    import oracle.drivers as od
    recs = od.Records(c.records())
    if bucket == c.DEB:
        got = od.debian_detect(recs, "12", None, pkgs)
    elif bucket == c.UBU:
        got = od.ubuntu_detect(recs, "22.04", None, pkgs, now=None)
    else:
        got = od.amazon_detect(recs, "2", None, pkgs)
    return collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in got)


@pytest.mark.parametrize("bucket", [c.DEB, c.UBU, c.AMZ])
def test_compare_vs_oracle(bucket, oracle_built):
    pkgs = c.packages()
    want = oracle_hits(bucket, pkgs)
    assert max(want.values()) == 1 and len(want) > 300
    got = collections.Counter()
    for p in pkgs:
        r = db().row16_eval(bucket, p["Name"], p["Version"])
        if r is None:
            assert p["Name"] in c.ABSENT
            continue
        for (path, res), (j, f) in zip(r, key_rows(bucket, p["Name"])):
            if res:
                got[(p["ID"], c.vuln_id(j))] += 1
    assert got == want
