"""GPU: the Red Hat per-CVE merge inside the pipelined pass (TVM_PIPE_RH_MERGE; rhmerge.hip
merges each chunk's Red Hat findings per VulnerabilityID, redhat.go:146-187, behind the chunk's
match launch, and applies the severity / status filter to the merged entries when one is set).

Expected values come from the oracle only: tests/vulnset_ref.py `expected` for unfiltered sets,
and for filtered passes oracle.drivers.driver_detect per target (Red Hat per release) ->
oracle.vulninfo.fill_info -> pipe_filter_cases.keep_mask (tests/pipe_rhmerge_cases.py, pinned on
the CPU by tests/test_pipeline_rhmerge_host.py).  Records are compared as canonical keys.

World A: a C5-shaped batch of twelve tiles (Red Hat and other drivers mixed) over a DB with the
"vulnerability" bucket; World B: the same without the bucket; World C: a hand-built Red Hat DB
with a group of 151 members that straddles a 64-entry round, under 300 identical packages."""
import numpy as np
import pytest

import pipe_rhmerge_cases as rc
import vulnset_ref as vr
from oracle import mix_c
from tools import synth_mix as sm

pytestmark = pytest.mark.gpu

MODES = [(False, False), (True, False), (False, True)]  # (raw form, 4-byte indices)
MODE_IDS = ["transport-3byte", "raw-3byte", "transport-adv32"]
CHUNKS = [256, 1024]
MASKS = rc.MASKS
MASK_IDS = ["high-critical-ign5-7", "low"]


class World:
    """One DB + batch on the GPU and the oracle's view of it (computed once, never changed)."""

    def __init__(self, sdb, batch, db, targets, recs, bucket, raw, unfiltered=None):
        import trivy_amd
        self.sdb, self.batch, self.bucket = sdb, batch, bucket
        self.eng = trivy_amd.Engine(db.finalize(), 0)
        self.keys = vr.Keys()
        self.chain = rc.Chain(targets, recs, bucket)
        self.groups = rc.rh_groups(targets, recs)
        self.chain_rec = self.chain.rec_ids(self.keys)
        self.raw = raw
        # the unfiltered set: vulnset_ref.expected for the synthetic mixes, the driver chain for World C
        self.want = unfiltered(self.keys) if unfiltered else (self.chain.pkg, self.chain_rec)
        assert np.array_equal(self.want[0], self.chain.pkg) and np.array_equal(self.want[1], self.chain_rec)

    def fill(self, base=0):
        from trivy_amd.batch import MatchBatch
        mb = MatchBatch(self.eng)
        sm.add_to(mb, self.sdb, self.batch)
        if base:
            mb.set_package_base(base)
        return mb

    def expect(self, **mask):
        keep = self.chain.keep(**mask) if mask else np.ones(len(self.chain.pkg), dtype=bool)
        return self.chain.pkg[keep], self.chain_rec[keep]


def _mix_world(with_bucket):
    import trivy_amd
    from tools.synth_vuln import vuln_arena, vuln_values
    sdb = sm.make_mix_db(sm.C5_PLATS, 300, seed=0xC5C5)
    batch = sm.make_mix_batch(sdb, 3000, sm.C5_WEIGHTS, seed=31)  # twelve tiles
    db = sdb.put(trivy_amd.DB())
    bucket = {}
    if with_bucket:
        ids = sm.MixDB.vuln_ids_of(sdb)
        db.put_arena(*vuln_arena(ids))
        bucket = {k.decode(): v.decode() for k, v in vuln_values(ids)}
    targets, recs = rc.mix_targets(sdb, batch)
    # raw matches, from the oracle: every plain pair and every member of every Red Hat group
    prep = mix_c.Prepared(sm, sdb, [(p, g, np.arange(len(g["key"]))) for p, g in batch.groups])
    pk, en = mix_c.match(prep, 8, members=True)
    is_rh = np.array([f == "redhat" for f in prep.plat_family], dtype=bool)[prep.plat_of[pk]]
    raw = int((en < 0).sum() + ((en >= 0) & ~is_rh).sum())
    return World(sdb, batch, db, targets, recs, bucket, raw,
                 unfiltered=lambda keys: vr.expected(sm, sdb, batch, keys, threads=8)[:2])


@pytest.fixture(scope="module")
def world_a(oracle_built):
    return _mix_world(True)


@pytest.fixture(scope="module")
def world_b(oracle_built):
    return _mix_world(False)


@pytest.fixture(scope="module")
def world_c(oracle_built):
    import trivy_amd
    batch, targets, recs = rc.world_c_targets()
    db = trivy_amd.DB()
    db.put_records(rc.world_c_records())
    w = World(batch, batch, db, targets, recs, {}, 0)
    w.raw = sum(len(m) for m in w.groups.values())  # no CVE of World C has two unfixed advisories
    return w


def _world(request, name):
    return request.getfixturevalue("world_" + name)


def _check_pass(mb, w, want_pkg, want_rec, adv32, base=0):
    """One pass of a prepared pipeline against the oracle's entries, through every accessor;
    returns the set (the caller closes it)."""
    n, width = len(w.batch), 4 if adv32 else 3
    total, errp, _ = mb.pipeline_run()
    assert errp == -1 and total == w.raw  # n_matches stays the raw count
    vs = mb.vulns(pipeline=True)
    got_pkg, got_rec = vr.gpu_side(vs, w.keys)
    print("raw", w.raw, "entries", len(want_pkg), "got", len(got_pkg), "group records", vs.n_grp_recs)
    assert np.array_equal(got_pkg, want_pkg + base)
    bad = np.nonzero(got_rec != want_rec)[0]
    assert len(bad) == 0, (len(bad), int(got_pkg[bad[0]]))
    assert vs.rec_width == width
    assert mb.pipeline_filter_stats() == (w.raw, len(want_pkg))
    assert mb.pipeline_stats()["d2h_bytes"] == 4 * n + width * len(want_pkg)
    adv, rend = mb.pipeline_csr()
    assert np.array_equal(rend, np.cumsum(np.bincount(want_pkg, minlength=n)).astype(np.uint32))
    assert np.array_equal(adv, vs.rec)  # the result hands out the set's record indices
    araw, got_width = mb.pipeline_csr_raw()
    assert got_width == width and np.array_equal(araw, vs.rec)
    return vs


@pytest.mark.parametrize("name", ["a", "b", "c"])
@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_merge_without_filter(request, name, chunk, raw, adv32):
    w = _world(request, name)
    assert len(w.want[0]) < w.raw  # the merge removes something
    mb = w.fill().pipeline_prepare(match_cap=w.raw + 5, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=True)
    for _ in range(2):  # a second pass starts again from the raw lists and gives the same set
        vs = _check_pass(mb, w, *w.want, adv32)
        assert vs.n_grp_recs > 0
        n_multi = sum(1 for m in w.groups.values() if len(m) > 1)
        assert vs.n_grp_recs == n_multi and int((vs.rec >= vs.n_adv_recs).sum()) == n_multi
        vs.close()
    mb.close()


@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_same_set_as_the_device_merge(world_a, chunk, raw, adv32):
    """The flag-on set against the flag-off tvm_pipeline_vulns (RedHatMerge + export over the
    whole list) of the same batch on the same engine."""
    w = world_a
    seqs = []
    for flag in (True, False):
        mb = w.fill().pipeline_prepare(match_cap=w.raw, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=flag)
        total, errp, _ = mb.pipeline_run()
        assert errp == -1 and total == w.raw
        vs = mb.vulns(pipeline=True)
        seqs.append(vr.gpu_side(vs, w.keys))
        vs.close()
        mb.close()
    assert np.array_equal(seqs[0][0], seqs[1][0]) and np.array_equal(seqs[0][1], seqs[1][1])
    assert len(seqs[0][0]) == len(w.want[0])


@pytest.mark.parametrize("mask", MASKS, ids=MASK_IDS)
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_merge_and_filter(request, name, chunk, raw, adv32, mask):
    w = _world(request, name)
    keep = w.chain.keep(**mask)
    ign = mask.get("ignore_statuses", ())
    # what the case exercises, from the oracle's numbers alone
    facts = rc.group_facts(w.chain, w.groups, keep, mask["severities"], ign)
    print(dict(facts))
    assert 0 < keep.sum() < len(keep)
    assert facts["rh_emptied"] > 0 and facts["rh_whole"] > 0
    assert facts["kept_by_first_severity"] > 0 and facts["dropped_by_first_severity"] > 0
    assert facts["other_driver_filtered_in_rh_tile"] > 0
    if ign:  # a group whose first member's Status is ignored survives because a member is fixed
        assert facts["kept_by_fixed"] > 0
    mb = w.fill().pipeline_prepare(match_cap=w.raw + 5, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=True)
    mb.pipeline_set_filter(mb.filter_opts(**mask))
    _check_pass(mb, w, *w.expect(**mask), adv32).close()
    mb.close()


def _entries_of(vs, p):
    i0 = int(vs.row_end[p - 1]) if p else 0
    return [vs.record(r) for r in vs.rec[i0:int(vs.row_end[p])].tolist()]


@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_heavy_groups(world_c, chunk, raw, adv32):
    w = world_c
    oracle_big = next(v for p, v in zip(w.chain.pkg.tolist(), w.chain.det) if p == 0 and v["VulnerabilityID"] == rc.BIG_CVE)
    per_pkg = np.bincount(w.chain.pkg, minlength=len(w.batch))
    mb = w.fill().pipeline_prepare(match_cap=w.raw, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=True)
    vs = _check_pass(mb, w, *w.want, adv32)
    big = [d for d in _entries_of(vs, 0) if d["VulnerabilityID"] == rc.BIG_CVE]
    assert len(big) == 1  # 151 members, one entry
    assert big[0]["FixedVersion"] == oracle_big["FixedVersion"] == f"3.0.{rc.N_BIG_RHSA - 1}-1.el8_0"
    assert big[0]["VendorIDs"] == oracle_big["VendorIDs"] and len(big[0]["VendorIDs"]) == rc.N_BIG_RHSA
    assert big[0]["Severity"] == oracle_big["Severity"] == "HIGH" and big[0]["Status"] == 5
    # identical neighbours do not merge across packages: each of the 300 carries its own full list
    first = vs.rec[:int(vs.row_end[0])]
    assert per_pkg[0] == len(first) == rc.N_BEFORE + 1 + 3
    rows = np.split(vs.rec, vs.row_end[:-1])
    assert all(len(rows[p]) == per_pkg[0] for p in range(rc.N_REPEAT))
    ids = [[d["VulnerabilityID"] for d in _entries_of(vs, p)] for p in (0, 255, 256, rc.N_REPEAT - 1)]
    assert all(x == ids[0] for x in ids)
    vs.close()
    # its first member is will_not_fix (5), a member is fixed: FillInfo makes it Fixed (3)
    for ign, there in (((5,), True), ((3,), False)):
        mb.pipeline_set_filter(mb.filter_opts(ignore_statuses=ign))
        vs = _check_pass(mb, w, *w.expect(ignore_statuses=ign), adv32)
        assert any(d["VulnerabilityID"] == rc.BIG_CVE for d in _entries_of(vs, 0)) == there
        assert any(d["VulnerabilityID"] == rc.BIG_CVE for d in _entries_of(vs, rc.N_REPEAT - 1)) == there
        vs.close()
    mb.close()


@pytest.fixture(scope="module")
def deb_world(oracle_built):
    return rc.deb_world()


@pytest.mark.parametrize("filtered", [False, True], ids=["no-filter", "filter"])
@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_batch_without_red_hat_is_unchanged(deb_world, chunk, raw, adv32, filtered):
    """The flag changes nothing for a batch without Red Hat packages (the debian / ubuntu world
    of tests/test_gpu_pipeline_filter.py): CSR, index width, D2H bytes and statistics equal the
    flag-off pass's."""
    sdb, batch, eng = deb_world
    got = []
    for flag in (False, True):
        mb = rc.deb_fill(eng, sdb, batch).pipeline_prepare(match_cap=40 * len(batch), chunk_packages=chunk, raw=raw,
                                                           adv32=adv32, rh_merge=flag)
        if filtered:
            mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
        total, errp, _ = mb.pipeline_run()
        assert errp == -1 and total > 1000
        st = mb.pipeline_stats()
        got.append((total, mb.pipeline_csr(), mb.pipeline_csr_raw(), mb.pipeline_filter_stats(), st["d2h_bytes"],
                    st["h2d_bytes"], st["chunks"]))
        vs = mb.vulns(pipeline=True)
        assert vs.n_grp_recs == 0
        vs.close()
        mb.close()
    off, on = got
    assert off[0] == on[0] and off[3:] == on[3:] and off[2][1] == on[2][1]
    assert np.array_equal(off[1][0], on[1][0]) and np.array_equal(off[1][1], on[1][1]) and np.array_equal(off[2][0], on[2][0])
    assert (off[3][1] < off[3][0]) == filtered and off[2][1] == (4 if adv32 else 3)


@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_package_base(world_a, chunk, raw, adv32):
    w = world_a
    base = 1_000_003
    mb = w.fill(base).pipeline_prepare(match_cap=w.raw, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=True)
    vs = _check_pass(mb, w, *w.want, adv32, base=base)
    assert int(vs.pkg.min()) >= base
    vs.close()
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    _check_pass(mb, w, *w.expect(**MASKS[0]), adv32, base=base).close()
    mb.close()


@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_lifecycle(world_a, chunk, raw, adv32):
    """Filter set, changed and cleared on one prepared pipeline; a new prepare without the flag
    returns to raw passes and to the Red Hat refusal; overflow is judged on the raw count."""
    w = world_a
    mb = w.fill().pipeline_prepare(match_cap=w.raw, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=True)
    for mask in (MASKS[0], MASKS[1], dict(severities=("UNKNOWN", "MEDIUM"), ignore_statuses=(3,))):
        mb.pipeline_set_filter(mb.filter_opts(**mask))
        _check_pass(mb, w, *w.expect(**mask), adv32).close()
    mb.pipeline_set_filter(None)
    _check_pass(mb, w, *w.want, adv32).close()
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    mb.pipeline_prepare(match_cap=w.raw, chunk_packages=chunk, raw=raw, adv32=adv32)  # no flag: the mode and the filter are cleared
    total, errp, _ = mb.pipeline_run()
    assert errp == -1 and total == w.raw and mb.pipeline_filter_stats() == (w.raw, w.raw)
    assert len(mb.pipeline_csr()[0]) == w.raw
    with pytest.raises(ValueError, match="Red Hat"):
        mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    # the merged entries alone would fit, the raw matches do not
    assert len(w.want[0]) < w.raw - 1
    mb.pipeline_prepare(match_cap=w.raw - 1, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=True)
    with pytest.raises(OverflowError) as ei:
        mb.pipeline_run()
    assert ei.value.args[0] == w.raw
    mb.pipeline_prepare(match_cap=w.raw, chunk_packages=chunk, raw=raw, adv32=adv32, rh_merge=True)
    _check_pass(mb, w, *w.want, adv32).close()
    mb.close()
