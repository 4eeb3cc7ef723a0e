"""GPU: the dpkg-only match kernel with the tile's encoder work list (packages whose name the index
may hold are listed by their version's dword count before the code table's barrier, lane i of the
tile encodes work item i into that package's key slot, and every lane picks its own slot up behind
one more barrier) against the kernel that encodes lane per package, and both against the Python
oracle.  Batches of 1 to 3 tiles: a tile with every name absent (an empty list), 256 found packages
of one length (one bucket holds the tile), a single found package in lane 255, version lengths 1 to
40 mixed with versions the fast encoder hands to the generic one (non-ASCII, a 10-digit run, a key
over 32 bytes) and unparsable ones on found and absent names, 257 and 300 packages (a partial last
tile), packages of an unknown platform interleaved, and a tile whose strings exceed a wave's
staging window (the whole tile runs lane per package)."""
import collections
import functools

import numpy as np
import pytest

import row16_cases as c
from test_gpu_row16 import hits_of, variant_index

pytestmark = pytest.mark.gpu

BAL, LANE = "fused_k4_m2400_wseg_rec_r16", "fused_k4_m2400_wseg_rec_lane_r16"
UNKNOWN = "nosuch 1"
STEM = "1.2.3-4+deb12u5~rc6.7.8.9.10.11.12.13.14"  # every prefix of it is a version
BY_LEN = [STEM[:n] for n in range(1, 41)]
FALLBACK = ["1.2é", "1.1234567890", c.LONG, "1234567890:1.0"]  # non-ASCII, 10-digit run, key > 32 bytes, long epoch
INVALID = ["x1.0", c.BAD, "1:-1", "1.0 1", ""]
FOUND = ["pkg", "other", "n" * 31, "k" * 33]


def records():
    recs = [c._rec(("data-source", c.DEB), {"ID": "debian", "Name": c.DEB, "URL": "https://x"})]
    j = 0
    for name in FOUND:  # a bound at every version the batches hold: one wrong key byte or length moves a match
        for f in BY_LEN[::3 if name != "pkg" else 1] + FALLBACK[1:3] + ["", "1.2.3-4+deb12u4", "1.2.3-5"]:
            recs.append(c._rec((c.DEB, name, c.vuln_id(j)), {"FixedVersion": f}))
            j += 1
    return recs


@functools.lru_cache(maxsize=None)
def world():
    import oracle.drivers as od
    import trivy_amd
    recs = records()
    db = trivy_amd.DB()
    db.put_records(recs)
    db.finalize()
    return db, trivy_amd.Engine(db, 0), od.Records(recs)


def run_segments(eng, segments, variant):
    """(pairs, variant that ran) of one device-resident pass over (bucket, names, versions) runs."""
    from trivy_amd._lib import lib
    from trivy_amd.batch import MatchBatch
    lib().tvm_engine_set_variant(eng.h, variant)
    try:
        mb = MatchBatch(eng)
        for bucket, names, vers in segments:
            mb.add_many(bucket, [n.encode() for n in names], [v.encode() for v in vers])
        total, errp, bits = mb.run()
        assert errp == -1 and bits == 0
        pairs = mb.pairs().copy()
        assert len(pairs) == total
        ran = lib().tvm_variant_name(lib().tvm_engine_last_variant(eng.h)).decode()
        mb.close()
    finally:
        lib().tvm_engine_set_variant(eng.h, 0)
    return pairs, ran


def check(segments, min_hits=1):
    """Both kernels give the same pair list, and it is the oracle's."""
    import oracle.drivers as od
    db, eng, recs = world()
    pkgs, i = [], 0
    for bucket, names, vers in segments:
        assert len(names) == len(vers)
        for n, v in zip(names, vers):
            if bucket == c.DEB:
                pkgs.append({"ID": f"p{i}", "Name": n, "SrcName": n, "Version": v, "SrcVersion": v})
            i += 1
    assert 1 <= i <= 3 * 256
    want = collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in od.debian_detect(recs, "12", None, pkgs))
    assert sum(want.values()) >= min_hits
    new, ran_new = run_segments(eng, segments, variant_index(BAL))
    old, ran_old = run_segments(eng, segments, variant_index(LANE))
    assert (ran_new, ran_old) == (BAL, LANE)
    assert np.array_equal(new, old)
    assert hits_of(db, new) == want
    return want


def mixed(n, salt):
    """n packages: every version length 1..40, fallback and unparsable versions, on found and absent names."""
    vers = BY_LEN + FALLBACK + INVALID
    names, out = [], []
    for i in range(n):
        k = (i * 7 + salt) % 11
        names.append(FOUND[k % 4] if k < 7 else f"absent-{i}" if k < 10 else c.ABSENT[i % len(c.ABSENT)])
        out.append(vers[(i * 13 + salt) % len(vers)])
    return names, out


def test_every_name_absent():
    names = [f"absent-{i}" for i in range(256)]
    vers = [BY_LEN[i % 40] for i in range(256)]
    assert check([(c.DEB, names, vers)], min_hits=0) == collections.Counter()
    # the tile after an empty list still gets its own
    check([(c.DEB, names + ["pkg"] * 3, vers + ["1.2.3", "1", "1.2.3-4+deb12u5"])])


@pytest.mark.parametrize("length", [1, 4, 5, 28, 29, 40])
def test_one_bucket_holds_the_tile(length):
    """256 found packages whose versions all have one length (the dword-count boundaries and the open last bucket)."""
    stems = [s[:length] for s in (STEM, "2.4.6-8+deb11u9~rc1.2.3.4.50.60.70.80.90.1", "0.2.3-4+deb12u5~rc6.7.8.9.10.11.12.13.14")]
    names = [FOUND[i % 2] for i in range(256)]
    check([(c.DEB, names, [stems[i % 3] for i in range(256)])], min_hits=256)


def test_single_found_package_in_lane_255():
    names = [f"absent-{i}" for i in range(255)] + ["pkg"]
    vers = [BY_LEN[(3 * i) % 40] for i in range(255)] + ["1.2.3-4+deb12u4"]
    want = check([(c.DEB, names, vers)])
    assert {p for p, _ in want} == {"p255"}


@pytest.mark.parametrize("n", [256, 257, 300, 768])
def test_mixed_lengths_fallbacks_and_invalid(n):
    names, vers = mixed(n, n)
    want = check([(c.DEB, names, vers)], min_hits=n)
    by_pkg = {p for p, _ in want}
    for i, (nm, v) in enumerate(zip(names, vers)):  # the generic encoder's packages match too, the unparsable never
        if nm in FOUND and v in FALLBACK[1:3]:
            assert f"p{i}" in by_pkg, (i, nm, v)
        if v in INVALID or nm not in FOUND:
            assert f"p{i}" not in by_pkg, (i, nm, v)


def test_unknown_platform_interleaved():
    names, vers = mixed(600, 3)
    segments, i, k = [], 0, 0
    while i < 600:
        run = (1, 2, 3, 5, 64, 7, 130)[k % 7]
        segments.append((UNKNOWN if k % 2 else c.DEB, names[i:i + run], vers[i:i + run]))
        i += run
        k += 1
    check(segments, min_hits=100)
    # a whole tile of the unknown platform between two known ones
    a, b = mixed(256, 1), mixed(40, 2)
    check([(c.DEB, *a), (UNKNOWN, *mixed(256, 5)), (c.DEB, *b)], min_hits=100)


def test_strings_past_the_staging_window():
    """Wave 2 of the first tile holds 64 names of 60 bytes (> 3072 bytes with their versions): its window is
    not staged and the tile runs lane per package; the second tile is packed."""
    names, vers = mixed(512, 9)
    for i in range(128, 192):
        if names[i] not in FOUND:
            names[i] = f"absent-{i:03d}-" + "y" * 50
    names[130], vers[130] = "pkg", c.LONG
    names[191], vers[191] = "pkg", "1.2.3-4+deb12u4"
    assert sum(len(n) + len(v) for n, v in zip(names[128:192], vers[128:192])) > 3072 + 16
    assert all(sum(len(n) + len(v) for n, v in zip(names[w:w + 64], vers[w:w + 64])) < 3000 for w in (0, 64, 192, 256, 320, 384, 448))
    want = check([(c.DEB, names, vers)], min_hits=200)
    assert {"p130", "p191"} <= {p for p, _ in want}
