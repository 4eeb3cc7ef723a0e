"""GPU: the ordered launch on tile-head records (one 32-byte record per grid position: the tile and
its five group offsets, read by the match kernel in place of tile_map then tile_off) against the
same batch matched without order and records, with the order alone (TVM_NO_TILE_HEAD), and against
the Python oracle.  dpkg-only batches of 3 tiles reach the ordered launch through the engine's
minimum-tile-count knob; library batches get an order from two tiles on: 3 tiles of the
all-grammar kernel with shared staging, and 12 tiles of which one holds a Maven package, which
Engine::launch splits in two launches that take the records from `head + lean tiles` on."""
import collections
import contextlib
import functools
import os

import numpy as np
import pytest

import row16_cases as c
import tile_head_cases as th
from test_gpu_row16 import hits_of

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def world():
    import oracle.drivers as od
    import trivy_amd
    recs = th.records()
    db = trivy_amd.DB()
    db.put_records(recs)
    db.finalize()
    return db, trivy_amd.Engine(db, 0), od.Records(recs)


@contextlib.contextmanager
def upload_mode(eng, min_tiles, no_head):
    from trivy_amd._lib import lib
    old = lib().tvm_engine_set_order_min_tiles(eng.h, min_tiles)
    assert old > 0
    if no_head:
        os.environ["TVM_NO_TILE_HEAD"] = "1"
    try:
        yield
    finally:
        os.environ.pop("TVM_NO_TILE_HEAD", None)
        assert lib().tvm_engine_set_order_min_tiles(eng.h, old) == min_tiles


def run_segments(eng, segments, min_tiles, no_head=False):
    from trivy_amd._lib import lib
    from trivy_amd.batch import MatchBatch
    with upload_mode(eng, min_tiles, no_head):
        mb = MatchBatch(eng)
        for bucket, names, vers in segments:
            mb.add_many(bucket, [n.encode() for n in names], [v.encode() for v in vers])
        total, errp, bits = mb.run()
        assert errp == -1 and bits == 0
        pairs = mb.pairs().copy()
        assert len(pairs) == total
        ran = lib().tvm_variant_name(lib().tvm_engine_last_variant(eng.h)).decode()
        heads = lib().tvm_engine_last_head_launches(eng.h)  # kernel launches of the pass that read records
        mb.close()
    return pairs, ran, heads


def check(segments, min_hits=1):
    """Records, the order alone and neither give one pair list, and it is the oracle's."""
    import oracle.drivers as od
    db, eng, recs = world()
    pkgs, i = [], 0
    for bucket, names, vers in segments:
        for n, v in zip(names, vers):
            if bucket == c.DEB:
                pkgs.append({"ID": f"p{i}", "Name": n, "SrcName": n, "Version": v, "SrcVersion": v})
            i += 1
    nt = (i + 255) // 256
    assert 2 <= nt <= 3
    order, heads, toff = th.host_view(db, segments, nt)  # what the upload below builds
    th.check_heads(order, heads, toff)
    want = collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in od.debian_detect(recs, "12", None, pkgs))
    assert sum(want.values()) >= min_hits
    with_heads, ran, h1 = run_segments(eng, segments, nt)
    order_only, _, h0 = run_segments(eng, segments, nt, no_head=True)
    plain, _, hp = run_segments(eng, segments, 1024)
    assert ran == "fused_k4_m2400_wseg_rec_r16"
    assert (h1, h0, hp) == (1, 0, 0)  # the kernel took the records in the first run alone
    assert np.array_equal(with_heads, plain) and np.array_equal(order_only, plain)
    assert hits_of(db, with_heads) == want
    return want, order


def test_non_identity_order():
    want, order = check(th.light_heavy_600(), min_hits=88 * 20)
    assert order.tolist() == [2, 1, 0]
    assert not any(int(p[1:]) < 256 for p, _ in want) and any(int(p[1:]) >= 512 for p, _ in want)


def test_window_sizes():
    segs, windows = th.groups_of(th.WINDOW_TARGETS)
    assert windows == th.WINDOWS and max(windows[:8]) == 3072 < windows[8]
    want, _ = check(segs, min_hits=1000)
    by_tile = collections.Counter(int(p[1:]) // 256 for p, _ in want)
    assert min(by_tile[t] for t in range(3)) > 100  # the tile with the unstaged wave matches too


def test_trailing_unknown_platform():
    segs, _ = th.groups_of([1024, 1500, 1000, 1200, 1008, 1100])
    names = [f"x{i}" for i in range(300)]
    want, _ = check(segs + [(th.UNKNOWN, names, ["1.2.3"] * 300)], min_hits=500)
    assert max(int(p[1:]) for p, _ in want) < 384


def test_tile_without_rows_under_the_order():
    heavy = (["heavy"] * 256, [f"1.2.{(3 * i) % 110}-1" for i in range(256)])
    none = ([th.absent(i) for i in range(256)], [th.BY_LEN[i % 40] for i in range(256)])
    light = ([th.FOUND[i % 2] for i in range(200)], [th.BY_LEN[(3 * i) % 40] for i in range(200)])
    want, order = check([(c.DEB, heavy[0] + none[0] + light[0], heavy[1] + none[1] + light[1])], min_hits=256 * 30)
    assert order.tolist() == [0, 2, 1]
    assert not any(256 <= int(p[1:]) < 512 for p, _ in want)


# ---- library grammars: an order (and records) from two tiles on ---------------------------------

def mix_batch(sdb, groups):
    from tools import synth_mix as sm
    return sm.MixBatch(sorted(groups, key=lambda pg: pg[0]))


def run_mix(eng, sdb, batch, no_head):
    from tools import synth_mix as sm
    from trivy_amd._lib import lib
    from trivy_amd.batch import MatchBatch
    if no_head:
        os.environ["TVM_NO_TILE_HEAD"] = "1"
    try:
        mb = MatchBatch(eng)
        firsts = sm.add_to(mb, sdb, batch)
        total, errp, bits = mb.run()
        heads = lib().tvm_engine_last_head_launches(eng.h)
    finally:
        os.environ.pop("TVM_NO_TILE_HEAD", None)
    assert errp == -1 and bits == 0
    pairs = mb.pairs().astype(np.int64)
    assert len(pairs) == total
    mb.close()
    return pairs, firsts, heads


def check_mix(sdb, db, eng, batch, min_hits, launches):
    """Records against the order alone, and every package of every group against the oracle;
    `launches`: the kernel launches of the pass, each of which must have read the records.
    A batch with a library grammar gets its order from two tiles on whatever the engine's knob
    says, and the switch that takes the order away (TVM_NO_TILE_ORDER) is read once per process,
    so these two cases have no run without an order: the oracle stands in for it."""
    import oracle.drivers as od
    import oracle.library as ol
    from tools import synth_mix as sm
    from trivy_amd.batch import advisory_vuln_id
    pairs, firsts, h1 = run_mix(eng, sdb, batch, no_head=False)
    order_only, _, h0 = run_mix(eng, sdb, batch, no_head=True)
    assert (h1, h0) == (launches, 0)
    assert np.array_equal(pairs, order_only)
    checked = 0
    for (p, g), (_, first) in zip(batch.groups, firsts):
        bucket, kind = sdb.plats[p]
        pkgs = sm.driver_packages(sdb, p, g, np.arange(len(g["key"])))
        recs = sdb.records_for({r: {x["Name"] for x in pkgs} for r in sm.C3_ROOTS.get(kind, [bucket])})
        want = ol.detect(od.Records(recs), sm.LANG_OF[kind], pkgs)
        lo, hi = np.searchsorted(pairs[:, 0], [first, first + len(g["key"])])
        got = collections.Counter((int(a) - first, advisory_vuln_id(db, int(b))) for a, b in pairs[lo:hi])
        assert got == collections.Counter((int(v["PkgID"][1:]), v["VulnerabilityID"]) for v in want), bucket
        checked += len(want)
    assert checked >= min_hits
    return len(batch)


@functools.lru_cache(maxsize=None)
def mix_world():
    import trivy_amd
    from tools import synth_mix as sm
    sdb = sm.make_mix_db(sm.C3_PLATS, 300, seed=0x7EAD)
    db = sdb.put(trivy_amd.DB()).finalize()
    return sdb, db, trivy_amd.Engine(db, 0)


def test_all_grammar_shared_staging():
    from tools import synth_mix as sm
    sdb, db, eng = mix_world()
    n = check_mix(sdb, db, eng, sm.make_mix_batch(sdb, 700, sm.C3_WEIGHTS, seed=3), min_hits=200, launches=1)
    assert (n + 255) // 256 == 3


def test_split_launch():
    """12 tiles, one Maven package among them: the lean tiles and the one all-grammar tile run as
    two launches over the two parts of the order, each on its part of the records."""
    from tools import synth_mix as sm
    sdb, db, eng = mix_world()
    lean = sm.make_mix_batch(sdb, 2900, [15, 0, 40, 25], seed=5)
    mvn = sm.make_mix_batch(sdb, 1, [0, 1, 0, 0], seed=6, miss=0.0)
    assert [sdb.plats[p][1] for p, _ in mvn.groups] == ["maven"]
    n = check_mix(sdb, db, eng, mix_batch(sdb, lean.groups + mvn.groups), min_hits=1000, launches=2)
    assert n == 2901 and (n + 255) // 256 == 12
