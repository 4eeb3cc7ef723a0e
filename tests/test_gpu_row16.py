"""GPU: the hot-row sweep of dpkg-only batches (16-byte Row16 rows behind a per-key prefix; the
"auto" variant) against the parent's 32-byte-row kernel (fused_k4_m2400_wseg) and the oracle: the
hand-built cases of row16_cases.py, keys whose runs end at the edges of a 128-byte line of hot
rows, a 5000-row key whose tile overflows the pair map and the per-wave match buffers, a seeded
random batch with spilled keys, and one pipelined pass of two chunks."""
import collections

import numpy as np
import pytest

import row16_cases as c
from test_row16_host import oracle_hits

pytestmark = pytest.mark.gpu

OLD = "fused_k4_m2400_wseg"


def variant_index(name):
    from trivy_amd._lib import lib
    v = 1
    while lib().tvm_variant_name(v):
        if lib().tvm_variant_name(v).decode() == name:
            return v
        v += 1
    raise AssertionError(name)


def run_pairs(eng, bucket, names, vers, variant):
    """(pairs, name of the variant that ran) of one device-resident pass."""
    from trivy_amd._lib import lib
    from trivy_amd.batch import MatchBatch
    lib().tvm_engine_set_variant(eng.h, variant)
    try:
        mb = MatchBatch(eng)
        assert mb.add_many(bucket, [n.encode() for n in names], [v.encode() for v in vers]) == 0
        total, errp, bits = mb.run()
        assert errp == -1 and bits == 0
        pairs = mb.pairs().copy()
        assert len(pairs) == total
        ran = lib().tvm_variant_name(lib().tvm_engine_last_variant(eng.h)).decode()
        mb.close()
    finally:
        lib().tvm_engine_set_variant(eng.h, 0)
    return pairs, ran


def both_variants(eng, bucket, names, vers):
    """The pass on the auto variant (hot rows) and on the parent's kernel: identical pair lists."""
    new, ran_new = run_pairs(eng, bucket, names, vers, 0)
    old, ran_old = run_pairs(eng, bucket, names, vers, variant_index(OLD))
    assert ran_new.endswith("_r16") and ran_old == OLD
    assert np.array_equal(new, old)
    return new


def hits_of(db, pairs):
    from trivy_amd.batch import advisory_vuln_id
    return collections.Counter((f"p{int(a)}", advisory_vuln_id(db, int(b))) for a, b in pairs)


@pytest.mark.parametrize("bucket", [c.DEB, c.UBU, c.AMZ])
def test_cases_vs_oracle(bucket, oracle_built):
    import trivy_amd
    from test_row16_host import db
    eng = trivy_amd.Engine(db(), 0)
    pkgs = c.packages()
    want = oracle_hits(bucket, pkgs)
    pairs = both_variants(eng, bucket, [p["Name"] for p in pkgs], [p["Version"] for p in pkgs])
    assert hits_of(db(), pairs) == want and len(want) > 300


def edge_records():
    """Keys of 1, 7, 8, 9 and 17 rows (a 128-byte line holds 8 hot rows) and a 5000-row key."""
    recs = [c._rec(("data-source", c.DEB), {"ID": "debian", "Name": c.DEB, "URL": "https://x"})]
    for n in (1, 7, 8, 9, 17):
        for i in range(n):
            recs.append(c._rec((c.DEB, f"rows-{n}", f"CVE-2024-{i:04d}"), {"FixedVersion": f"1.2.{i}-1"}))
    for i in range(5000):
        recs.append(c._rec((c.DEB, "linux", f"CVE-2024-{i:04d}"),
                           {"FixedVersion": "" if i % 97 == 0 else f"5.10.{i}-1+deb12u{i % 3}"}))
    return recs


def test_line_edges_and_heavy_key_vs_oracle(oracle_built):
    import oracle.drivers as od
    import trivy_amd
    recs = edge_records()
    db = trivy_amd.DB()
    db.put_records(recs)
    db.finalize()
    st, ls = db.row16_stats(), db.layout_stats()
    assert st["hot_rows"] == ls["interval_rows"] == 1 + 7 + 8 + 9 + 17 + 5000 and st["fallback_rows"] == 0
    # runs in key order: linux 5000, rows-1 (+7 pad rows), rows-17 (+7), rows-7 (+1), rows-8, rows-9
    assert ls["rows"] == ls["pad_rows"] + ls["interval_rows"] and ls["pad_rows"] == 15
    names, vers = [], []
    for n in (1, 7, 8, 9, 17):
        for v in ("1.2.0-0", "1.2.0-1", f"1.2.{n - 1}-0", f"1.2.{n - 1}-1", f"1.2.{n}-1", "1.1", "x"):
            names.append(f"rows-{n}")
            vers.append(v)
    # one tile: 24 packages x 5000 rows = 120k pairs (> the 4096-entry pair map); those below every bound match
    # ~5000 rows each, thousands per wave segment (> the 600-entry per-wave match buffer: the DIRECT re-sweep)
    for i in range(24):
        names.append("linux")
        vers.append(["5.10.0-0", "5.10.2500-1+deb12u1", "5.10.4999-1+deb12u2", "5.9", "5.10.300-1+deb12u0", "6.1"][i % 6])
    assert len(names) < 256
    pkgs = [{"ID": f"p{i}", "Name": n, "SrcName": n, "Version": v, "SrcVersion": v} for i, (n, v) in enumerate(zip(names, vers))]
    want = collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in od.debian_detect(od.Records(recs), "12", None, pkgs))
    assert max(collections.Counter(p for p, _ in want).values()) == 5000 and sum(want.values()) > 40000
    eng = trivy_amd.Engine(db, 0)
    pairs = both_variants(eng, c.DEB, names, vers)
    assert hits_of(db, pairs) == want


@pytest.fixture(scope="module")
def world():
    from test_gpu_parity import build_engine
    from tools.synth import make_db
    sdb = make_db(["debian 12", "ubuntu 22.04"], 1000, seed=16)
    return sdb, build_engine(sdb)


def test_random_parity_vs_oracle(world, oracle_built):
    from oracle import match as om
    from test_gpu_parity import run_batch
    from tools.synth import make_batch
    from trivy_amd._lib import lib
    sdb, eng = world
    batch = make_batch(sdb, 20, 1000, [3, 2], seed=16, long_versions=0.05, invalid=0.01)
    opk, oad = om.match(om.Prepared(sdb, batch), n_threads=8)
    assert len(opk) > 50000
    for v in (0, variant_index(OLD)):
        lib().tvm_engine_set_variant(eng.h, v)
        try:
            pk, ad, errp, total = run_batch(eng, sdb, batch)
            ran = lib().tvm_variant_name(lib().tvm_engine_last_variant(eng.h)).decode()
        finally:
            lib().tvm_engine_set_variant(eng.h, 0)
        assert ran.endswith("_r16") if v == 0 else ran == OLD
        assert errp == -1 and np.array_equal(pk, opk) and np.array_equal(ad, oad), ran


def test_pipelined_pass_two_chunks(world, oracle_built):
    """The pipelined pass takes the same template with the result move (MOVE) compiled in."""
    from oracle import match as om
    from test_gpu_pipeline import _fill, _pairs_of
    from tools.synth import make_batch
    sdb, eng = world
    batch = make_batch(sdb, 20, 1000, [3, 2], seed=17, long_versions=0.05)
    opk, oad = om.match(om.Prepared(sdb, batch), n_threads=8)
    mb = _fill(eng, sdb, batch).pipeline_prepare(match_cap=len(opk) + 5, chunk_packages=10240)
    total, errp, ms = mb.pipeline_run()
    assert errp == -1 and total == len(opk)
    assert mb.pipeline_stats()["chunks"] == 2
    adv, rend = mb.pipeline_csr()
    pk, ad = _pairs_of(adv[:total], rend[:len(batch)])
    assert np.array_equal(pk, opk) and np.array_equal(ad, oad)
    mb.close()
