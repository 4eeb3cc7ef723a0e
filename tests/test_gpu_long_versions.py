"""The length limits of a version (DESIGN.md "Length limits"), kept apart from the other
comparator tests so that they can be judged on their own.

A sort key's length travels in 14 bits on both sides of a comparison (match_kernel.h KI_LEN for
the installed key, common.h KEY_LEN_MASK for a bound's), and a package's version text is cut at
65535 bytes; the encoders emit up to 5n + 24 key bytes, so a version of a few thousand bytes
can pass the first limit.  The reference compares such strings exactly.  The contract pinned
here, per grammar (dpkg on the dpkg-only kernel and as Amazon Linux runs it, rpm, apk):

  * up to the limit - a key of 16383 bytes on either side, measured with tvm_version_key - the
    drop-in call and the batch give the oracle's result;
  * past it the engine refuses, visibly: an installed version whose key is longer, or whose text
    has 65535 bytes or more, fails the upload of its batch (MatchBatch.upload / run,
    pipeline_prepare, the drivers' Detect) with an error that names the package; a bound whose
    key is longer fails DB.finalize with an error that names the advisory.

Before the refusals existed both went through with the length wrapped, no status bit set: a
key of 16384 bytes kept its head and the length 0, so a tie on the head was decided as if the
key ended there - the over-limit packages below were reported 5 advisories where the oracle
has 3 or 4, and an over-limit FixedVersion matched one of the three packages it covers.
"""
import ctypes
import functools

import pytest

import oracle.drivers as od
from conftest import canon
from row_layout_cases import _rec

KEY_LIMIT = 16383
# platform id: (tvm_version_key grammar, driver family, OS version, bucket)
PLATS = {"deb": (1, "debian", "12", "debian 12"), "amzn": (1, "amazon", "2", "amazon linux 2"),
         "rpm": (3, "alma", "9.3", "alma 9"), "apk": (2, "alpine", "3.19.1", "alpine 3.19")}
# version shapes by text length n: a long alternation of letters and digits, a long run of
# one-digit components, a long digit run
SHAPES = {"alt": lambda n: "1." + "a1" * ((n - 2) // 2), "dots": lambda n: "1" + ".1" * ((n - 1) // 2),
          "digits": lambda n: "1." + "9" * (n - 2)}
MAX_TEXT = 65534  # the longest version text a batch carries whole


def klen(grammar, v):
    from trivy_amd._lib import lib
    b = v.encode()
    buf = ctypes.create_string_buffer(8)
    return lib().tvm_version_key(grammar, b, len(b), buf, len(buf))


@functools.lru_cache(maxsize=None)
def crossing(grammar, shape):
    """(longest text whose key fits KEY_LIMIT, shortest text whose key does not) of a shape; the
    second is None when even MAX_TEXT bytes fit (a dpkg or apk digit run is one number)."""
    f = SHAPES[shape]
    assert 0 < klen(grammar, f(8)) <= KEY_LIMIT
    if klen(grammar, f(MAX_TEXT)) <= KEY_LIMIT:
        return f(MAX_TEXT), None
    lo, hi = 8, MAX_TEXT  # key(f(lo)) fits, key(f(hi)) does not; the key grows with n
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if klen(grammar, f(mid)) <= KEY_LIMIT:
            lo = mid
        else:
            hi = mid
    return f(lo), f(hi)


def _pkg(i, name, text):
    v, _, r = text.partition("-")
    return {"ID": f"p{i}", "Name": name, "Version": v, "Release": r, "Epoch": 0, "SrcName": name, "SrcVersion": v,
            "SrcRelease": r, "SrcEpoch": 0, "Arch": "x86_64"}


class Case:
    """One platform's table and packages.  Per shape a name "inst-<shape>" with short bounds that
    tie with the long installed versions on the key head (a prefix of the text, and neighbours of
    it) and a name "bound-<shape>" whose FixedVersion is the longest text under the limit, with
    installed versions around it.  `over`: the shortest over-limit text per shape."""

    def __init__(self, pid, long_bound=None, long_affected=None):
        self.grammar, self.family, self.os_ver, self.bucket = PLATS[pid]
        g, b = self.grammar, self.bucket
        self.records = [_rec(("data-source", b), {"ID": pid, "Name": b, "URL": "https://x"})]
        self.pkgs, self.over = [], {}
        n = 0

        def adv(name, val):
            nonlocal n
            n += 1
            self.records.append(_rec((b, name, f"CVE-2024-{6000 + n}"), val))

        for shape in SHAPES:
            under, over = crossing(g, shape)
            self.over[shape] = over
            for fixed in ("0.1", under[:41], under[:41] + "1", under[:40] + "2", "2", under[:-1] + "5"):
                adv(f"inst-{shape}", {"FixedVersion": fixed})
            self.pkgs.append(_pkg(len(self.pkgs), f"inst-{shape}", under))
            self.pkgs.append(_pkg(len(self.pkgs), f"inst-{shape}", under[:41]))
            adv(f"bound-{shape}", {"FixedVersion": under})
            for inst in (under, under[:-4], under[:-1] + "5", under[:200], "1", "3"):
                self.pkgs.append(_pkg(len(self.pkgs), f"bound-{shape}", inst))
        if long_bound:
            adv("bound-over", {"FixedVersion": long_bound})
        if long_affected:
            adv("bound-over", {"FixedVersion": "9", "AffectedVersion": long_affected})

    def names(self):
        return [p["SrcName"].encode() for p in self.pkgs]

    def versions(self):
        return [od.fmt(p).encode() for p in self.pkgs]

    def oracle(self):
        return od.driver_detect(self.family, self.os_ver, None, self.pkgs, od.Records(self.records), None)


def _db(records):
    import trivy_amd
    db = trivy_amd.DB()
    db.put_records(records)
    return db


# ------------------------------------------------------------------------------- CPU: limits ----
@pytest.mark.parametrize("pid", list(PLATS))
def test_limit_lengths(oracle_built, pid):
    """The smallest version lengths at which a key passes 16383 bytes, from the host encoder."""
    g = PLATS[pid][0]
    for shape in SHAPES:
        under, over = crossing(g, shape)
        print(f"\n{pid} {shape}: {len(under)} bytes -> key {klen(g, under)}"
              + (f"; {len(over)} bytes -> key {klen(g, over)}" if over else "; never past the limit"))
        assert 0 < klen(g, under) <= KEY_LIMIT
        assert over is None or klen(g, over) > KEY_LIMIT
    assert crossing(g, "alt")[1] is not None and crossing(g, "dots")[1] is not None
    assert (crossing(g, "digits")[1] is not None) == (pid == "rpm")
    # what the under-limit case decides: matches and non-matches on the long keys' tails
    c = Case(pid)
    per = {}
    for v in c.oracle():
        per.setdefault(v["PkgID"], []).append(v["VulnerabilityID"])
    n_adv = {p["ID"]: sum(r["path"][1] == p["SrcName"] for r in c.records) for p in c.pkgs}
    assert sum(0 < len(per.get(p["ID"], [])) < n_adv[p["ID"]] for p in c.pkgs if p["SrcName"].startswith("inst-")) >= 3
    assert {len(per.get(p["ID"], [])) for p in c.pkgs if p["SrcName"].startswith("bound-")} == {0, 1}


@pytest.mark.parametrize("pid", list(PLATS))
def test_bound_over_limit_is_refused(pid):
    """A FixedVersion (Alpine: also an AffectedVersion) whose key passes the limit: finalize fails
    and names the advisory."""
    g = PLATS[pid][0]
    over = crossing(g, "alt")[1]
    with pytest.raises(ValueError, match=r"CVE-2024-\d+ of bucket .* sort key of 1638[4-9] bytes \(limit 16383\)"):
        _db(Case(pid, long_bound=over).records).finalize()
    if pid == "apk":
        with pytest.raises(ValueError, match=r"limit 16383"):
            _db(Case(pid, long_affected=over).records).finalize()
    _db(Case(pid).records).finalize()  # the bounds just under the limit load


# ------------------------------------------------------------------------------------- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("pid", list(PLATS))
def test_under_limit_is_exact(oracle_built, pid):
    """Installed keys and bound keys of up to 16383 bytes (and a 65534-byte digit run where a
    digit run is one number): the oracle's result on both paths."""
    import collections
    import trivy_amd
    from trivy_amd.batch import MatchBatch, advisory_vuln_id
    from trivy_amd.detector import ospkg
    c = Case(pid)
    want = c.oracle()
    db = _db(c.records).finalize()
    eng = trivy_amd.Engine(db, 0)
    assert canon(ospkg.Scanner(eng, c.family).detect(c.os_ver, None, c.pkgs)) == canon(want)
    mb = MatchBatch(eng)
    mb.add_many(c.bucket, c.names(), c.versions())
    total, errp, bits = mb.run()
    assert errp == -1 and bits == 0
    got = collections.Counter((int(a), advisory_vuln_id(db, int(b))) for a, b in mb.pairs())
    assert got == collections.Counter((int(v["PkgID"][1:]), v["VulnerabilityID"]) for v in want)
    assert total == len(want) > 10
    mb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pid", list(PLATS))
def test_installed_over_limit_is_refused(oracle_built, pid):
    """Three packages per grammar at the smallest over-limit lengths (a digit run where it has
    one) and one version of 65536 bytes, each among packages that are fine: the batch's upload,
    the pipelined pass's prepare and the driver's Detect fail and name the package; without it
    the same batch runs."""
    import trivy_amd
    from trivy_amd.batch import MatchBatch
    from trivy_amd.detector import ospkg
    c = Case(pid)
    eng = trivy_amd.Engine(_db(c.records).finalize(), 0)
    texts = [(s, t) for s, t in c.over.items() if t] + [("digits", "1." + "9" * 65534)]
    assert len(texts) >= 3 and len(texts[-1][1]) == 65536
    fine = c.pkgs[:4]
    for shape, text in texts:
        bad = _pkg(99, f"inst-{shape}", text)
        pkgs = fine[:2] + [bad] + fine[2:]
        msg = "package 2 \\(inst-" + shape + "\\).*is not compared"
        mb = MatchBatch(eng)
        mb.add_many(c.bucket, [p["SrcName"].encode() for p in pkgs], [od.fmt(p).encode() for p in pkgs])
        with pytest.raises(RuntimeError, match="tvm_batch_upload: " + msg):
            mb.run()
        with pytest.raises(RuntimeError, match="tvm_pipeline_prepare: " + msg):
            mb.pipeline_prepare()
        mb.close()
        with pytest.raises(ospkg.DetectError, match=msg):
            ospkg.Scanner(eng, c.family).detect(c.os_ver, None, pkgs)
    mb = MatchBatch(eng)
    mb.add_many(c.bucket, [p["SrcName"].encode() for p in fine], [od.fmt(p).encode() for p in fine])
    assert mb.run()[1:] == (-1, 0)
    mb.close()
