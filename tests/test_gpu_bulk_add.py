"""GPU: the parallel bulk add (tvm_batch_add_targets_attrs: every target of a fleet batch in one
call, filled on the host threads) builds the same batch as adding target by target
(tvm_batch_add_many_attrs) - same match pairs, same package side, same DetectedVulnerability
set - for the attribute-carrying workloads (Red Hat CPE sets + arches, Oracle ksplice, Rocky
arches) and the plain one; shards added as package ranges concatenate to the whole; bad
attributes are refused without touching the batch.  And the native consumer of a set
(tvm_vuln_set_walk) sees every DetectedVulnerability (its digest recomputed from the columns)."""
import numpy as np
import pytest

from tools import synth_mix as sm

pytestmark = pytest.mark.gpu


def _engine(plats, kpp, seed):
    import trivy_amd
    sdb = sm.make_mix_db(plats, kpp, seed=seed)
    return sdb, trivy_amd.Engine(sdb.put(trivy_amd.DB()).finalize(), 0)


@pytest.mark.parametrize("cfg", ["c5", "c4", "c3"])
def test_bulk_add_equals_per_target_adds(cfg):
    from trivy_amd.batch import MatchBatch
    plats, weights = {"c5": (sm.C5_PLATS, sm.C5_WEIGHTS), "c4": (sm.C4_PLATS, sm.C4_WEIGHTS),
                      "c3": (sm.C3_PLATS, sm.C3_WEIGHTS)}[cfg]
    sdb, eng = _engine(plats, 1500, seed=41)
    batch = sm.make_mix_batch(sdb, 120_000, weights, seed=43)
    one = MatchBatch(eng)
    sm.add_to(one, sdb, batch)
    bulk = MatchBatch(eng)
    cols = sm.BulkCols(sdb, batch, per_target=400)
    assert cols.add(bulk) == 0 and len(bulk) == len(one) == len(batch)
    got = []
    for mb in (one, bulk):
        total, errp, bits = mb.run()
        assert errp == -1 and bits == 0
        pairs = mb.pairs()  # the raw list (vulns() merges Red Hat packages per CVE on the device)
        vs = mb.vulns()
        got.append((pairs, mb.report(), vs.pkg.copy(), vs.rec.copy(), vs.walk(), vs.digest()))
        vs.close()
    (p1, r1, vp1, vr1, w1, d1), (p2, r2, vp2, vr2, w2, d2) = got
    assert len(p1) > 20_000 and np.array_equal(p1, p2)
    assert r1 == r2
    assert np.array_equal(vp1, vp2) and np.array_equal(vr1, vr2)
    assert w1 == (len(vp1), d1) and w2 == (len(vp2), d2)
    # two shards added as package ranges (whole targets) concatenate to the whole
    cut = int(cols.ends[len(cols.ends) // 2])
    halves = []
    for lo, hi in ((0, cut), (cut, len(batch))):
        mb = MatchBatch(eng)
        assert cols.add(mb, lo, hi) == 0 and len(mb) == hi - lo
        mb.set_package_base(lo)
        mb.run()
        halves.append(mb.pairs())
        mb.close()
    assert np.array_equal(np.concatenate(halves), p2)
    one.close()
    bulk.close()


def _outputs(mb):
    total, errp, bits = mb.run()
    assert errp == -1 and bits == 0
    pairs = mb.pairs()
    vs = mb.vulns()
    out = (pairs, mb.report(), vs.pkg.copy(), vs.rec.copy(), vs.walk(), vs.digest())
    vs.close()
    return out


@pytest.mark.parametrize("order", ["attrs_first", "plain_first"])
def test_bulk_add_appends_to_partial_group(order):
    """Bulk adds into a batch that already holds packages, at sizes that are no multiple of the
    64-package group: the partial group keeps its string offset, and the attribute column is
    back-filled with the no-attribute word when the first attribute-carrying add comes after
    plain ones (plain_first) - the batch equals the one built by add_many alone."""
    from trivy_amd.batch import MatchBatch
    sdb, eng = _engine(sm.C5_PLATS, 300, seed=61)
    batch = sm.make_mix_batch(sdb, 3000, sm.C5_WEIGHTS, seed=62)
    g = {sdb.plats[p][0]: (p, grp) for p, grp in batch.groups}
    assert len(g) == len(sm.C5_PLATS)

    def seg(bucket, lo=0, hi=None):
        p, grp = g[bucket]
        return p, lo, len(grp["key"]) if hi is None else hi

    def cols_of(segs, per_target):
        groups = [(p, {k: v[lo:hi] for k, v in g[sdb.plats[p][0]][1].items()}) for p, lo, hi in segs]
        return sm.BulkCols(sdb, sm.MixBatch(groups), per_target=per_target)

    def bulk_plain(mb, segs):  # tvm_batch_add_targets: no attribute columns at all
        c = cols_of(segs, 90)
        assert not c.flags.any()
        return mb.add_targets(c.buckets, c.ends, c.arena, c.noff, c.nlen, c.voff, c.vlen)

    def bulk_attrs(mb, segs, empty_first=False):
        c = cols_of(segs, 70)
        assert c.flags.any()
        if not empty_first:
            return c.add(mb)
        sets = np.zeros(c.n, np.uint32)
        inv = {v: k for k, v in c.combos.items()}
        for ci in np.unique(c.combo[c.combo >= 0]).tolist():
            sets[c.combo == ci] = mb.cpe_set(list(inv[ci][0]), inv[ci][1])
        return mb.add_targets([c.buckets[0]] + c.buckets, np.concatenate([[0], c.ends]).astype(np.uint64), c.arena,
                              c.noff, c.nlen, c.voff, c.vlen, flags=np.concatenate([c.flags[:1], c.flags]),
                              arch_off=c.aoff, arch_len=c.alen, cpe_sets=sets)

    def many(mb, segs):
        for p, lo, hi in segs:
            sm.add_slice(mb, sdb, p, g[sdb.plats[p][0]][1], lo, hi)

    if order == "attrs_first":
        steps = [(many, [seg("alma 8", 0, 37)]),
                 (bulk_attrs, [seg("Red Hat"), seg("Oracle Linux 8")]),
                 (many, [seg("alma 8", 37, 42)]),
                 (bulk_plain, [seg("alma 8", 42), seg("alma 9"), seg("alpine 3.19")]),
                 (lambda mb, s: bulk_attrs(mb, s, empty_first=True),
                  [seg("rocky 8"), seg("Oracle Linux 9"), seg("alpine 3.20"), seg("rocky 9")])]
    else:
        steps = [(bulk_plain, [seg("alma 9")]),
                 (many, [seg("alma 8", 0, 37)]),
                 (bulk_attrs, [seg("Red Hat"), seg("rocky 8")]),
                 (bulk_plain, [seg("alma 8", 37), seg("alpine 3.19")]),
                 (many, [seg("Oracle Linux 8"), seg("alpine 3.20", 0, 5)]),
                 (lambda mb, s: bulk_attrs(mb, s, empty_first=True),
                  [seg("Oracle Linux 9"), seg("alpine 3.20", 5), seg("rocky 9")])]
    one, mixed = MatchBatch(eng), MatchBatch(eng)
    cuts, mid = [], 0
    for fn, segs in steps:
        many(one, segs)
        begin = len(mixed)
        fn(mixed, segs)
        assert len(mixed) == len(one) == begin + sum(hi - lo for _, lo, hi in segs)
        cuts.append(len(mixed))
        mid += fn is not many and begin % 64 != 0 and len(mixed) % 64 != 0
    assert len(one) == len(batch) and all(x % 64 for x in cuts) and mid >= 1
    (p1, r1, vp1, vr1, w1, d1), (p2, r2, vp2, vr2, w2, d2) = _outputs(one), _outputs(mixed)
    assert len(p1) > 1000 and np.array_equal(p1, p2)
    assert r1 == r2
    assert np.array_equal(vp1, vp2) and np.array_equal(vr1, vr2)
    assert w1 == (len(vp1), d1) and w2 == (len(vp2), d2) and d1 == d2
    one.close()
    mixed.close()


def test_bulk_add_refuses_bad_attributes():
    import ctypes

    from trivy_amd.batch import ATTR_CPESET, ATTR_KSPLICE, MatchBatch
    sdb, eng = _engine(sm.C5_PLATS, 300, seed=5)
    batch = sm.make_mix_batch(sdb, 4000, sm.C5_WEIGHTS, seed=6)
    cols = sm.BulkCols(sdb, batch)
    mb = MatchBatch(eng)
    n = cols.n
    ends = cols.ends
    args = ([cols.buckets[t] for t in range(len(ends))], ends, cols.arena, cols.noff, cols.nlen, cols.voff, cols.vlen)
    with pytest.raises(RuntimeError):  # one attribute word: a ksplice tag or a CPE set, not both
        mb.add_targets(*args, flags=np.full(len(ends), ATTR_KSPLICE | ATTR_CPESET, np.uint32),
                       cpe_sets=np.zeros(n, np.uint32))
    with pytest.raises(RuntimeError):  # a CPE-set id the batch never registered
        mb.add_targets(*args, flags=np.full(len(ends), ATTR_CPESET, np.uint32), cpe_sets=np.full(n, 7, np.uint32))
    with pytest.raises(RuntimeError):  # arch flags without the arch columns
        mb.add_targets(*args, flags=np.full(len(ends), 1, np.uint32))
    assert len(mb) == 0
    assert cols.add(mb) == 0 and len(mb) == n  # the batch is still usable
    total, errp, bits = mb.run()
    assert errp == -1 and bits == 0 and total > 0
    del ctypes
    mb.close()


def test_walk_digest_dpkg_batch():
    """The consumer over a plain dpkg batch added by tvm_batch_add_targets (C2's form) and over
    its pipelined set: the same DetectedVulnerabilities, the same digest."""
    from test_gpu_parity import build_engine
    from tools.synth import make_batch, make_db
    from trivy_amd.batch import MatchBatch
    sdb = make_db(["debian 12", "ubuntu 22.04"], 2000, seed=12)
    eng = build_engine(sdb)
    batch = make_batch(sdb, 60, 400, [1, 1], seed=13)
    arena, noff, nlen, voff, vlen = batch.arena()
    mb = MatchBatch(eng)
    ends = np.array([b1 for _, _, b1 in batch.targets], dtype=np.uint64)
    mb.add_targets([sdb.platforms[p] for p, _, _ in batch.targets], ends, arena, noff, nlen, voff, vlen)
    total, errp, _ = mb.run()
    vs = mb.vulns()
    n1, d1 = vs.walk()
    assert n1 == len(vs) == total and d1 == vs.digest()
    vs.close()
    mb.pipeline_prepare(match_cap=total, chunk_packages=4096)
    assert mb.pipeline_run()[:2] == (total, -1)
    vp = mb.vulns(pipeline=True)
    assert vp.walk() == (n1, d1)
    vp.close()
    mb.close()
