"""GPU: the dpkg key builder's unconditional token stores next to its neighbours' LDS slots.  One
tile of 256 packages in which every other lane holds a version whose key is 30 to 33 bytes (its
last tokens land at and past the clamped position; 33 bytes takes the generic encoder) and the
lanes between them 1-byte versions, which finish first: a store that ran past a lane's 44-byte
slot would land in the finished neighbour's key.  The bounds sit right around both kinds of key,
so one wrong byte changes the match list, which must equal the Python oracle's."""
import collections

import numpy as np
import pytest

import row16_cases as c
from test_gpu_row16 import hits_of, run_pairs, variant_index

pytestmark = pytest.mark.gpu

VARIANTS = ["fused_k4_m2400_wseg_rec_r16", "fused_k4_m2400_wseg_r16", "fused_k4_m2400_wseg"]


def long_versions():
    """key length -> '1aaa..65536' with a key of that many bytes, for 30 .. 33."""
    out = {}
    for n in range(40):
        v = "1" + "a" * n + "65536"
        k = c.version_key(v)
        if 30 <= len(k) <= 33:
            out[len(k)] = v
    assert sorted(out) == [30, 31, 32, 33], sorted(out)
    return out


def records(longs):
    recs = [c._rec(("data-source", c.DEB), {"ID": "debian", "Name": c.DEB, "URL": "https://x"})]
    j = 0
    for v in longs.values():  # bounds one below, at and one above every long key's last number
        for last in ("65535", "65536", "65537"):
            recs.append(c._rec((c.DEB, "long", c.vuln_id(j)), {"FixedVersion": v[:-5] + last}))
            j += 1
    recs.append(c._rec((c.DEB, "long", c.vuln_id(j)), {"FixedVersion": ""}))
    for j, f in enumerate(["0", "1", "2", "3", ""]):
        recs.append(c._rec((c.DEB, "short", c.vuln_id(100 + j)), {"FixedVersion": f}))
    return recs


def test_long_keys_next_to_short_ones(oracle_built):
    import oracle.drivers as od
    import trivy_amd
    from trivy_amd._lib import lib
    longs = long_versions()
    recs = records(longs)
    db = trivy_amd.DB()
    db.put_records(recs)
    db.finalize()
    names, vers = [], []
    for i in range(256):
        if i % 2 == 0:
            names.append("long")
            vers.append(longs[30 + (i // 2) % 4])
        else:
            names.append("short")
            vers.append("0123"[(i // 2) % 4])
    pkgs = [{"ID": f"p{i}", "Name": n, "SrcName": n, "Version": v, "SrcVersion": v} for i, (n, v) in enumerate(zip(names, vers))]
    want = collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in od.debian_detect(od.Records(recs), "12", None, pkgs))
    by_pkg = collections.Counter(p for p, _ in want)
    assert len({by_pkg[f"p{i}"] for i in range(0, 8, 2)}) == 4 and len({by_pkg[f"p{i}"] for i in range(1, 8, 2)}) == 4
    eng = trivy_amd.Engine(db, 0)
    first = None
    for name in [None] + VARIANTS:
        pairs, ran = run_pairs(eng, c.DEB, names, vers, 0 if name is None else variant_index(name))
        assert ran == name if name else ran == lib().tvm_variant_name(lib().tvm_engine_last_variant(eng.h)).decode()
        assert hits_of(db, pairs) == want, ran
        first = pairs if first is None else first
        assert np.array_equal(pairs, first), ran
