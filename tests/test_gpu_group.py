"""GPU: engine groups (tvm_group_*, trivy_amd/csrc/group.cpp) - one batch sharded over several
members inside one process.  Every member sits on device 0 (several members on one GPU: the
shape a one-GPU box can run; the cross-device path makes the same calls with a peer copy in
place of the device copy).  Expected values come from the oracle: tests/vulnset_ref.py over
the mixed worlds of tools/synth_mix.py, oracle.match pairs and oracle.vulninfo for the
Debian / Ubuntu world of tests/pipe_filter_cases.py."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import pipe_filter_cases as pc
import vulnset_ref as vr
from tools import synth_mix as sm
from tools.synth import SynthBatch, make_batch, make_db

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 13
CHUNK = 1024


def _csr(pk, ad, n_pkgs):
    """(adv, row_end) of pairs in (package, advisory) order."""
    return ad.astype(np.uint32), np.cumsum(np.bincount(pk, minlength=n_pkgs)).astype(np.uint32)


class DevBuf:
    """n int32 entries of device 0's memory filled with -1, allocated through the HIP runtime the
    library itself is bound to (tvm_runtime_info) - a pytest process that loaded the library
    first cannot start torch's own.  Quacks like the int32 tensor GroupBatch.csr_into takes."""

    class dtype:
        itemsize = 4

    def __init__(self, n, view_of=None):
        import ctypes
        import trivy_amd
        self.hip = ctypes.CDLL(trivy_amd.runtime_info()["libamdhip64"])
        self.n, self.owner = n, view_of
        if view_of is not None:
            self.p = view_of.p
            return
        self.p = ctypes.c_void_p()
        assert self.hip.hipSetDevice(0) == 0
        assert self.hip.hipMalloc(ctypes.byref(self.p), ctypes.c_size_t(max(4 * n, 4))) == 0
        assert self.hip.hipMemset(self.p, 0xFF, ctypes.c_size_t(4 * n)) == 0
        assert self.hip.hipDeviceSynchronize() == 0  # the union runs on the members' own streams

    def data_ptr(self):
        return self.p.value if self.n else None

    def numel(self):
        return self.n

    def head(self, n):
        """The first n entries as a buffer of their own (a smaller capacity over the same memory)."""
        return DevBuf(n, view_of=self)

    def numpy(self):
        import ctypes
        out = np.zeros(self.n, dtype=np.int32)
        if self.n:
            assert self.hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), self.p, ctypes.c_size_t(4 * self.n), 2) == 0  # D2H
        return out

    def __del__(self):
        if self.owner is None and getattr(self, "p", None):
            self.hip.hipFree(self.p)


def _tiles(gb, ends):
    """shards() tiles [0, n) on target boundaries; returns it."""
    sh = gb.shards()
    assert len(sh) == len(gb.group) + 1 and sh[0] == 0 and sh[-1] == len(gb)
    assert all(a <= b for a, b in zip(sh, sh[1:]))
    assert set(sh) <= {0} | {int(e) for e in ends}
    for k in range(len(gb.group)):
        assert (gb.member(k) is None) == (sh[k] == sh[k + 1])
    return sh


# ---- the mixed worlds: every driver family, Red Hat merged per CVE ---------------------------

MIX = {"c5": (sm.C5_PLATS, sm.C5_WEIGHTS), "c4": (sm.C4_PLATS, sm.C4_WEIGHTS)}
_mix_cache = {}


def _mix(cfg):
    """Per world, once: the DB, the bulk columns, the oracle's expected set and a single
    engine's pipelined lists."""
    if cfg in _mix_cache:
        return _mix_cache[cfg]
    import trivy_amd
    from trivy_amd.batch import MatchBatch
    plats, weights = MIX[cfg]
    sdb = sm.make_mix_db(plats, 600, seed=7)
    batch = sm.make_mix_batch(sdb, 20_000, weights, seed=9)
    db = sdb.put(trivy_amd.DB()).finalize()
    cols = sm.BulkCols(sdb, batch, per_target=70)
    keys = vr.Keys()
    want_pkg, want_rec, _ = vr.expected(sm, sdb, batch, keys, threads=8)
    eng = trivy_amd.Engine(db, 0)
    mb = MatchBatch(eng)
    cols.add(mb)
    mb.pipeline_prepare(chunk_packages=CHUNK)
    total, errp, _ = mb.pipeline_run()
    assert errp == -1
    single = mb.pipeline_csr()
    mb.close()
    eng.close()
    rh = np.zeros(cols.n, dtype=bool)  # packages of the Red Hat driver
    o = 0
    for p, g in batch.groups:
        m = len(g["key"])
        rh[o:o + m] = sdb.plats[p][1] == "redhat"
        o += m
    w = dict(sdb=sdb, db=db, cols=cols, keys=keys, want=(want_pkg, want_rec), total=total, single=single, rh=rh)
    _mix_cache[cfg] = w
    return w


def _sets_equal(gb, w):
    """The members' DetectedVulnerability sets, taken in order, against the oracle's."""
    sets = gb.vulns(pipeline=True)
    sides = [vr.gpu_side(vs, w["keys"]) for vs in sets]
    got_pkg = np.concatenate([s[0] for s in sides])
    got_rec = np.concatenate([s[1] for s in sides])
    assert np.array_equal(got_pkg, w["want"][0])
    bad = np.nonzero(got_rec != w["want"][1])[0]
    assert len(bad) == 0, (len(bad), int(got_pkg[bad[0]]))
    return sets


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("cfg", list(MIX))
def test_pipelined_group_pass_vs_oracle(cfg, n):
    from trivy_amd.group import EngineGroup, GroupBatch
    w = _mix(cfg)
    grp = EngineGroup(w["db"], [0] * n)
    assert len(grp) == n and len(grp.engines) == n
    gb = GroupBatch(grp)
    w["cols"].add(gb)
    assert len(gb) == w["cols"].n
    sh = _tiles(gb, w["cols"].ends)
    assert all(gb.member(k) is not None for k in range(n))
    gb.pipeline_prepare(match_cap=w["total"], chunk_packages=CHUNK)
    total, errp, ms = gb.pipeline_run()
    assert errp == -1 and total == w["total"] and ms > 0 and sum(gb.member_matches) == total
    adv, rend = gb.pipeline_csr()
    assert np.array_equal(rend, w["single"][1]) and np.array_equal(adv, w["single"][0])
    # a member's own row ends start at 0 and its matches are its slice of the batch's
    for k, m in gb.members():
        a, r = m.pipeline_csr()
        assert len(r) == sh[k + 1] - sh[k] and len(a) == gb.member_matches[k] == (int(r[-1]) if len(r) else 0)
    for vs in _sets_equal(gb, w):
        vs.close()
    # once more, merging Red Hat findings inside each member's pass
    gb.pipeline_prepare(match_cap=w["total"], chunk_packages=CHUNK, rh_merge=True)
    total, errp, _ = gb.pipeline_run()
    assert errp == -1 and total == w["total"]
    sets = _sets_equal(gb, w)
    rh_per = [int(w["rh"][sh[k]:sh[k + 1]].sum()) for k in range(n)]
    assert max(rh_per) > 0
    for (k, _), vs in zip(gb.members(), sets):
        if rh_per[k] == max(rh_per):
            assert vs.n_grp_recs > 0
        if rh_per[k] == 0:
            assert vs.n_grp_recs == 0
        vs.close()
    gb.close()
    grp.close()


# ---- the Debian / Ubuntu world of the filter tests ----------------------------------------

def _engine_db(sdb, seed):
    import trivy_amd
    from tools.synth_vuln import vuln_arena
    from trivy_amd._lib import lib
    db = trivy_amd.DB()
    for n, depth, arena, off, lens in (sdb.records_arena((), detail=True), sdb.source_arena(),
                                       vuln_arena(sdb.vuln_ids(), seed)):
        assert lib().tvm_db_put_arena(db.h, n, depth, arena, off.ctypes.data, lens.ctypes.data) == 0
    return db.finalize()


def _add(b, sdb, batch, n_targets=None, **kw):
    """The first n_targets targets of a SynthBatch through add_targets (group or single batch)."""
    arena, noff, nlen, voff, vlen = batch.arena()
    tg = batch.targets[:n_targets]
    n = tg[-1][2] if tg else 0
    b.add_targets([sdb.platforms[p] for p, _, _ in tg], np.array([e for _, _, e in tg], dtype=np.uint64), arena,
                  noff[:n], nlen[:n], voff[:n], vlen[:n], **kw)
    return n, [e for _, _, e in tg]


class World:
    def __init__(self, sdb, batch, seed):
        self.sdb, self.batch, self.seed = sdb, batch, seed
        self.db = _engine_db(sdb, seed)
        self.opk, self.oad = pc.oracle_pairs(sdb, batch)
        self._filled = None

    @property
    def filled(self):
        if self._filled is None:
            self._filled = pc.filled(self.sdb, self.seed, pc.detected(self.sdb, self.batch, self.opk, self.oad))
        return self._filled

    def pairs(self, n=None):
        """The oracle's pairs of packages [0, n)."""
        n = len(self.batch) if n is None else n
        keep = self.opk < n
        return self.opk[keep], self.oad[keep]


@pytest.fixture(scope="module")
def world(oracle_built):
    sdb = make_db(["debian 12", "ubuntu 22.04"], 800, seed=SEED)
    batch = make_batch(sdb, 11, 120, [1, 1], seed=SEED)
    assert len(batch) == 1320 and len(batch.targets) == 11
    return World(sdb, batch, SEED)


_groups = {}


def _group(w, n):
    from trivy_amd.group import EngineGroup
    key = (id(w), n)
    if key not in _groups:
        _groups[key] = EngineGroup(w.db, [0] * n)
    return _groups[key]


def _pass_equals(gb, pk, ad, n_pkgs):
    """One pipelined pass of a prepared group batch against expected pairs."""
    total, errp, _ = gb.pipeline_run()
    assert errp == -1
    adv, rend = gb.pipeline_csr()
    want = _csr(pk, ad, n_pkgs)
    assert np.array_equal(rend, want[1]) and np.array_equal(adv, want[0])
    return total


@pytest.mark.parametrize("n", [2, 3])
def test_filter_across_members(world, n):
    from trivy_amd.group import GroupBatch
    w = world
    mask = dict(severities=("HIGH", "CRITICAL"), ignore_statuses=(5, 7))
    keep = pc.keep_mask(w.filled, **mask)
    assert 0 < keep.sum() < len(keep)
    gb = GroupBatch(_group(w, n))
    _, ends = _add(gb, w.sdb, w.batch)
    _tiles(gb, ends)
    gb.pipeline_prepare(match_cap=len(w.opk) + 5, chunk_packages=CHUNK)
    gb.pipeline_set_filter(gb.filter_opts(**mask))
    assert _pass_equals(gb, w.opk[keep], w.oad[keep], len(w.batch)) == len(w.opk)  # n_matches stays raw
    stats = [m.pipeline_filter_stats() for _, m in gb.members()]
    assert sum(s[0] for s in stats) == len(w.opk) and sum(s[1] for s in stats) == keep.sum()
    # ignore rules need whole results: refused, and no member keeps a filter
    with pytest.raises(ValueError, match="ignore rules"):
        gb.pipeline_set_filter(gb.filter_opts(ignore_ids=["CVE-2001-1000"], **mask))
    _pass_equals(gb, w.opk, w.oad, len(w.batch))
    for _, m in gb.members():
        s = m.pipeline_filter_stats()
        assert s[0] == s[1]
    gb.close()


def test_plan_by_rows(world):
    """One target of nothing but the heavy key, the rest as they are: the row plan isolates it."""
    from trivy_amd import dist
    from trivy_amd._lib import lib
    from trivy_amd.group import PLAN_ROWS, GroupBatch
    w = world
    names = list(w.batch.names)
    p0, b0, e0 = w.batch.targets[0]
    names[b0:e0] = [b"linux"] * (e0 - b0)
    heavy = SynthBatch(w.batch.plat, names, w.batch.versions, w.batch.targets)
    opk, oad = pc.oracle_pairs(w.sdb, heavy)
    arena, noff, nlen, _, _ = heavy.arena()
    rows = np.zeros(len(heavy), dtype=np.uint32)
    for p, b, e in heavy.targets:
        assert lib().tvm_db_rows_many(w.db.h, w.sdb.platforms[p].encode(), e - b, arena, noff[b:].ctypes.data,
                                      nlen[b:].ctypes.data, rows[b:].ctypes.data) == 0
    begins = [b for _, b, _ in heavy.targets]
    for n in (2, 3):
        gb = GroupBatch(_group(w, n))
        _, ends = _add(gb, w.sdb, heavy, plan=PLAN_ROWS)
        sh = _tiles(gb, ends)
        by_pkgs = dist.target_shards(begins, len(heavy), np.ones(len(heavy)), n)
        assert sh != by_pkgs
        assert sh == dist.target_shards(begins, len(heavy), rows.astype(np.int64) + 1, n)
        gb.pipeline_prepare(match_cap=len(opk), chunk_packages=CHUNK)
        assert _pass_equals(gb, opk, oad, len(heavy)) == len(opk)
        gb.close()


@pytest.mark.parametrize("n_targets", [2, 1, 0])
def test_empty_and_degenerate_shards(world, n_targets):
    from trivy_amd.group import GroupBatch
    w = world
    gb = GroupBatch(_group(w, 3))
    n, ends = _add(gb, w.sdb, w.batch, n_targets)
    assert len(gb) == n == 120 * n_targets
    sh = _tiles(gb, ends)
    assert sum(gb.member(k) is None for k in range(3)) == 3 - n_targets
    pk, ad = w.pairs(n)
    gb.pipeline_prepare(match_cap=max(len(pk), 1), chunk_packages=CHUNK)
    assert _pass_equals(gb, pk, ad, n) == len(pk)
    assert [m for m in gb.member_matches] == [int(((pk >= sh[k]) & (pk < sh[k + 1])).sum()) for k in range(3)]
    gb.upload(match_cap=max(len(pk), 1)).launch()
    assert gb.status() == (len(pk), -1, 0)
    adv, rend = DevBuf(len(pk) + 3), DevBuf(n)
    assert gb.csr_into(2, adv, rend) == len(pk)
    want = _csr(pk, ad, n)
    assert np.array_equal(adv.numpy()[:len(pk)].astype(np.uint32), want[0])
    assert np.array_equal(rend.numpy().astype(np.uint32), want[1])
    assert (adv.numpy()[len(pk):] == -1).all()
    gb.close()


@pytest.mark.parametrize("n,root", [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)])
def test_device_resident_union(world, n, root):
    from trivy_amd import dist
    from trivy_amd.group import GroupBatch
    w = world
    total = len(w.opk)
    # from the oracle's counts: at three members some member's first list entry is no multiple
    # of 4 entries (a 16-byte line), so the copies land unaligned
    sh3 = dist.target_shards([b for _, b, _ in w.batch.targets], len(w.batch), np.ones(len(w.batch)), 3)
    assert any(int((w.opk < b).sum()) % 4 for b in sh3[1:3])
    gb = GroupBatch(_group(w, n))
    _, ends = _add(gb, w.sdb, w.batch)
    sh = _tiles(gb, ends)
    gb.upload(match_cap=total).launch()
    assert gb.status() == (total, -1, 0)
    assert gb.member_matches == [int(((w.opk >= sh[k]) & (w.opk < sh[k + 1])).sum()) for k in range(n)]
    adv, rend = DevBuf(total), DevBuf(len(w.batch))
    # a cap below the total: refused with the total, nothing written
    with pytest.raises(ValueError) as ei:
        gb.csr_into(root, adv.head(total - 7), rend)
    assert ei.value.args[0] == total
    assert (adv.numpy() == -1).all() and (rend.numpy() == -1).all()
    assert gb.csr_into(root, adv, rend) == total
    want = _csr(w.opk, w.oad, len(w.batch))
    assert np.array_equal(adv.numpy().astype(np.uint32), want[0])
    assert np.array_equal(rend.numpy().astype(np.uint32), want[1])
    # an overflowed member pass hands nothing out
    caps = list(gb.member_matches)
    caps[-1] -= 1
    gb.upload(member_caps=caps).launch()
    with pytest.raises(ValueError) as ei:
        gb.csr_into(root, adv, rend)
    assert ei.value.args[0] == total
    gb.close()


def test_overflow_reports_member_counts(world):
    from trivy_amd.group import GroupBatch
    w = world
    gb = GroupBatch(_group(w, 3))
    _add(gb, w.sdb, w.batch)
    sh = gb.shards()
    exact = [int(((w.opk >= sh[k]) & (w.opk < sh[k + 1])).sum()) for k in range(3)]
    assert min(exact) > 1
    short = list(exact)
    short[1] -= 1
    gb.pipeline_prepare(member_caps=short, chunk_packages=CHUNK)
    with pytest.raises(OverflowError) as ei:
        gb.pipeline_run()
    assert ei.value.args[0] == len(w.opk) and gb.member_matches == exact
    # a device-resident upload of the same batch with another capacity leaves the prepared
    # pipeline's capacities alone: the overflow is still reported as one, with exact counts
    gb.upload(match_cap=2 * len(w.opk)).launch()
    assert gb.status() == (len(w.opk), -1, 0)
    gb.member_matches = None
    with pytest.raises(OverflowError) as ei:
        gb.pipeline_run()
    assert ei.value.args[0] == len(w.opk) and gb.member_matches == exact
    gb.pipeline_prepare(member_caps=gb.member_matches, chunk_packages=CHUNK)
    assert _pass_equals(gb, w.opk, w.oad, len(w.batch)) == len(w.opk)
    gb.close()


def test_swap_refuses_old_batches_and_serves_the_new_db(world):
    from trivy_amd.group import EngineGroup, GroupBatch
    w = world
    grp = EngineGroup(w.db, [0, 0])
    old = GroupBatch(grp)
    _add(old, w.sdb, w.batch)
    old.pipeline_prepare(match_cap=len(w.opk), chunk_packages=CHUNK)
    _pass_equals(old, w.opk, w.oad, len(w.batch))
    sdb2 = make_db(["debian 12", "ubuntu 22.04"], 500, seed=SEED + 1)
    batch2 = make_batch(sdb2, 11, 120, [1, 1], seed=SEED + 1)
    w2 = World(sdb2, batch2, SEED + 1)
    grp.swap(w2.db)
    with pytest.raises(RuntimeError, match="built against other tables"):
        old.pipeline_run()
    with pytest.raises(RuntimeError, match="built against other tables"):
        old.pipeline_prepare(match_cap=len(w.opk), chunk_packages=CHUNK)
    old.close()
    mask = dict(severities=("HIGH", "CRITICAL"), ignore_statuses=(5, 7))
    keep = pc.keep_mask(w2.filled, **mask)
    assert 0 < keep.sum() < len(keep)
    gb = GroupBatch(grp)
    _add(gb, sdb2, batch2)
    gb.pipeline_prepare(match_cap=len(w2.opk), chunk_packages=CHUNK)
    _pass_equals(gb, w2.opk, w2.oad, len(batch2))
    gb.pipeline_set_filter(gb.filter_opts(**mask))  # the classes of the new tables
    _pass_equals(gb, w2.opk[keep], w2.oad[keep], len(batch2))
    gb.close()
    grp.close()


def test_swap_with_row_planned_adds_in_flight(world):
    """Adds planned by rows (the probe reads the served DB under member 0's shared lock) from one
    thread while another swaps the group back and forth: every add ends - built, or refused when
    the swap fell between its members - nothing hangs, and a batch built afterwards is exact."""
    from trivy_amd.group import PLAN_ROWS, EngineGroup, GroupBatch
    w = world
    sdb2 = make_db(["debian 12", "ubuntu 22.04"], 500, seed=SEED + 2)
    db2 = _engine_db(sdb2, SEED + 2)
    grp = EngineGroup(w.db, [0, 0])
    stop, done, errs = threading.Event(), [0, 0], []

    def adder():
        try:
            while not stop.is_set():
                gb = GroupBatch(grp)
                try:
                    _add(gb, w.sdb, w.batch, plan=PLAN_ROWS)
                    done[0] += 1
                except RuntimeError:  # members bound to different table generations
                    done[1] += 1
                gb.close()
        except BaseException as e:  # noqa: BLE001  reported by the main thread
            errs.append(e)
    th = threading.Thread(target=adder)
    th.start()
    for k in range(6):
        grp.swap(db2 if k % 2 == 0 else w.db)
    stop.set()
    th.join(60)
    assert not th.is_alive() and not errs and done[0] > 0
    gb = GroupBatch(grp)  # the group serves w.db again
    _add(gb, w.sdb, w.batch, plan=PLAN_ROWS)
    gb.pipeline_prepare(match_cap=len(w.opk), chunk_packages=CHUNK)
    _pass_equals(gb, w.opk, w.oad, len(w.batch))
    gb.close()
    grp.close()


def test_two_group_batches_run_concurrently(world):
    from trivy_amd.group import GroupBatch
    w = world
    grp = _group(w, 3)
    n_b = 240
    pk_b, ad_b = w.pairs(n_b)
    a, b = GroupBatch(grp), GroupBatch(grp)
    _add(a, w.sdb, w.batch)
    _add(b, w.sdb, w.batch, 2)
    a.pipeline_prepare(match_cap=len(w.opk), chunk_packages=CHUNK)
    b.pipeline_prepare(match_cap=len(pk_b), chunk_packages=256)
    errs = []

    def loop(gb, pk, ad, n):
        try:
            for _ in range(8):
                _pass_equals(gb, pk, ad, n)
        except BaseException as e:  # noqa: BLE001  reported by the main thread
            errs.append(e)
    th = [threading.Thread(target=loop, args=(a, w.opk, w.oad, len(w.batch))),
          threading.Thread(target=loop, args=(b, pk_b, ad_b, n_b))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    a.close()
    b.close()


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import trivy_amd
from tools.synth import make_batch, make_db
from trivy_amd._lib import lib
from trivy_amd.group import EngineGroup, GroupBatch
sdb = make_db(["debian 12", "ubuntu 22.04"], 300, seed=3)
batch = make_batch(sdb, 6, 100, [1, 1], seed=3)
db = trivy_amd.DB()
for n, depth, arena, off, lens in (sdb.records_arena(), sdb.source_arena()):
    assert lib().tvm_db_put_arena(db.h, n, depth, arena, off.ctypes.data, lens.ctypes.data) == 0
grp = EngineGroup(db.finalize(), [0, 0])
gb = GroupBatch(grp)
arena, noff, nlen, voff, vlen = batch.arena()
gb.add_targets([sdb.platforms[p] for p, _, _ in batch.targets], [e for _, _, e in batch.targets], arena, noff, nlen,
               voff, vlen)
gb.pipeline_prepare(chunk_packages=256)
total, errp, _ = gb.pipeline_run()
assert errp == -1 and total > 0 and all(m > 0 for m in gb.member_matches)
print("matches", total)
"""


def test_process_exits_cleanly_with_an_open_group():
    """A process that opened a group and closes nothing: the member threads are joined by
    tvm_shutdown (atexit), and the exit status is 0."""
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "matches" in r.stdout
