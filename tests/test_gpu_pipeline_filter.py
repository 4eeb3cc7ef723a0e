"""GPU: the severity / status filter inside the pipelined pass (tvm_pipeline_set_filter:
prefilter.hip compacts each chunk's match segments to the findings that pass filter.go:113-120
before the result move).  Expected values come from the oracle only: oracle.match pairs, each
pair's DetectedVulnerability as the debian / ubuntu drivers build it, oracle.vulninfo.fill_info,
and keep iff (Severity or "UNKNOWN") in severities and Status not in ignore_statuses."""
import numpy as np
import pytest

import pipe_filter_cases as pc
from oracle import match as om
from tools.synth import SynthBatch, make_batch, make_db

pytestmark = pytest.mark.gpu

SEED = 13
MODES = [(False, False), (True, False), (False, True)]  # (raw form, 4-byte indices)
MODE_IDS = ["transport-3byte", "raw-3byte", "transport-adv32"]
CHUNKS = [256, 1024]
MASKS = [dict(severities=("HIGH", "CRITICAL"), ignore_statuses=(5, 7)), dict(severities=("LOW",))]


def _engine(sdb, seed, poison=()):
    import trivy_amd
    from tools.synth_vuln import vuln_arena
    from trivy_amd._lib import lib
    db = trivy_amd.DB()
    for n, depth, arena, off, lens in (sdb.records_arena(poison, detail=True), sdb.source_arena(),
                                       vuln_arena(sdb.vuln_ids(), seed)):
        assert lib().tvm_db_put_arena(db.h, n, depth, arena, off.ctypes.data, lens.ctypes.data) == 0
    return trivy_amd.Engine(db, 0)


def _fill(eng, sdb, batch):
    from trivy_amd.batch import MatchBatch
    mb = MatchBatch(eng)
    arena, noff, nlen, voff, vlen = batch.arena()
    for p, b0, b1 in batch.targets:
        mb.add_arena(sdb.platforms[p], b1 - b0, arena, noff[b0:], nlen[b0:], voff[b0:], vlen[b0:])
    return mb


def _csr(pk, ad, n_pkgs):
    """(adv, row_end) of pairs in (package, advisory) order."""
    return ad.astype(np.uint32), np.cumsum(np.bincount(pk, minlength=n_pkgs)).astype(np.uint32)


class World:
    def __init__(self, sdb, batch, seed, eng):
        self.sdb, self.batch, self.eng = sdb, batch, eng
        self.opk, self.oad = pc.oracle_pairs(sdb, batch)
        self.filled = pc.filled(sdb, seed, pc.detected(sdb, batch, self.opk, self.oad))

    def expect(self, severities=tuple(pc.NAMES5), ignore_statuses=()):
        """The oracle's kept (pkg, adv) and their CSR."""
        keep = pc.keep_mask(self.filled, severities, ignore_statuses)
        pk, ad = self.opk[keep], self.oad[keep]
        return pk, ad, _csr(pk, ad, len(self.batch))

    def unfiltered(self):
        """Every oracle pair (a pass without a filter drops nothing, whatever the severity)."""
        return self.opk, self.oad, _csr(self.opk, self.oad, len(self.batch))


@pytest.fixture(scope="module")
def world(oracle_built):
    sdb = make_db(["debian 12", "ubuntu 22.04"], 800, seed=SEED)
    batch = make_batch(sdb, 11, 120, [1, 1], seed=SEED)  # 1320 packages: five full tiles and a ragged sixth
    assert len(batch) == 1320
    return World(sdb, batch, SEED, _engine(sdb, SEED))


def _check_pass(mb, w, pk, ad, csr, adv32):
    """One filtered pass's result against the oracle's kept pairs, through every accessor."""
    raw, kept, width = len(w.opk), len(pk), 4 if adv32 else 3
    total, errp, _ = mb.pipeline_run()
    assert errp == -1 and total == raw  # n_matches stays the raw count
    adv, rend = mb.pipeline_csr()
    assert np.array_equal(rend, csr[1]) and np.array_equal(adv, csr[0])
    araw, got_width = mb.pipeline_csr_raw()
    assert got_width == width and np.array_equal(araw, csr[0])
    vs = mb.vulns(pipeline=True)
    assert np.array_equal(vs.pkg, pk) and np.array_equal(vs.rec, ad)
    vs.close()
    assert mb.pipeline_stats()["d2h_bytes"] == 4 * len(w.batch) + width * kept
    assert mb.pipeline_filter_stats() == (raw, kept)


@pytest.fixture(scope="module")
def bare_world(oracle_built):
    """The same packages over a DB without the "vulnerability" bucket: FillInfo finds no ID, so
    every finding keeps the detector's own severity or UNKNOWN - all inside SeverityNames."""
    import trivy_amd
    from trivy_amd._lib import lib
    sdb = make_db(["debian 12", "ubuntu 22.04"], 800, seed=SEED)
    batch = make_batch(sdb, 11, 120, [1, 1], seed=SEED)
    db = trivy_amd.DB()
    for n, depth, arena, off, lens in (sdb.records_arena(detail=True), sdb.source_arena()):
        assert lib().tvm_db_put_arena(db.h, n, depth, arena, off.ctypes.data, lens.ctypes.data) == 0
    w = World.__new__(World)
    w.sdb, w.batch, w.eng = sdb, batch, trivy_amd.Engine(db, 0)
    w.opk, w.oad = pc.oracle_pairs(sdb, batch)
    import oracle.vulninfo as vi
    vulns = pc.detected(sdb, batch, w.opk, w.oad)
    w.filled = vi.fill_info({}, [{k: x for k, x in v.items() if k != "_pair"} for v in vulns])
    return w


@pytest.mark.parametrize("bucket", [True, False], ids=["vuln-bucket", "no-vuln-bucket"])
@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_all_five_severities(world, bare_world, chunk, raw, adv32, bucket):
    """All five severities, no ignored statuses, against the same batch's unfiltered pass.

    Without the "vulnerability" bucket every severity lies inside SeverityNames: the filtered
    pass equals the unfiltered one exactly and kept == raw.  With the synthetic bucket it cannot:
    tools/synth_vuln.py gives a tenth of the records the DB severity "moderate", which FillInfo
    passes through verbatim where no vendor severity applies, and filter.go:115 drops a severity
    outside FilterOption.Severities whatever the list holds (severity index 5 passes no mask).
    The oracle puts that at raw 10553, kept 10091 for this world.  There the result must equal
    the oracle's kept list, every dropped finding must be one the oracle gives a severity
    outside SeverityNames, and every other package's list must equal the unfiltered pass's."""
    w = world if bucket else bare_world
    pk, ad, csr = w.expect()
    odd = np.array([((f.get("Vulnerability") or {}).get("Severity") or "UNKNOWN") not in pc.NAMES5 for f in w.filled])
    assert len(w.opk) - len(pk) == odd.sum() and (odd.any() == bucket)
    mb = _fill(w.eng, w.sdb, w.batch).pipeline_prepare(match_cap=len(w.opk) + 5, chunk_packages=chunk, raw=raw,
                                                       adv32=adv32)
    total, errp, _ = mb.pipeline_run()
    assert errp == -1 and total == len(w.opk)
    plain, plain_raw = mb.pipeline_csr(), mb.pipeline_csr_raw()
    assert mb.pipeline_filter_stats() == (total, total)
    assert np.array_equal(plain[0], w.oad) and np.array_equal(plain[1], _csr(w.opk, w.oad, len(w.batch))[1])
    mb.pipeline_set_filter(mb.filter_opts())  # all five severities, no ignored statuses
    total2, errp, _ = mb.pipeline_run()
    got, got_raw = mb.pipeline_csr(), mb.pipeline_csr_raw()
    assert errp == -1 and total2 == total and mb.pipeline_filter_stats() == (total, len(pk))
    assert got_raw[1] == plain_raw[1] and np.array_equal(got_raw[0], got[0])
    assert np.array_equal(got[0], csr[0]) and np.array_equal(got[1], csr[1])
    if not bucket:  # kept == raw: the unfiltered pass, exactly
        assert len(pk) == total and np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        assert np.array_equal(got_raw[0], plain_raw[0])
    else:  # package by package: the unfiltered list, but for the findings of a severity outside the names
        whole = np.ones(len(w.batch), dtype=bool)
        whole[w.opk[odd]] = False
        lists = lambda a, r: np.split(a, r[:-1])  # noqa: E731
        for p, (x, y) in enumerate(zip(lists(*got), lists(*plain))):
            assert np.array_equal(x, y) == bool(whole[p]), p
    mb.close()


@pytest.mark.parametrize("mask", MASKS, ids=["high-critical-ign5-7", "low"])
@pytest.mark.parametrize("raw,adv32", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunk", CHUNKS)
def test_filtered_pass_vs_oracle(world, chunk, raw, adv32, mask):
    w = world
    pk, ad, csr = w.expect(**mask)
    # the case filters something and keeps something, judged from the oracle's numbers: some
    # package's whole list is emptied and another's is kept whole
    n_raw, n_kept = np.bincount(w.opk, minlength=len(w.batch)), np.bincount(pk, minlength=len(w.batch))
    print("raw", len(w.opk), "kept", len(pk))
    assert 0 < len(pk) < len(w.opk)
    assert np.any((n_raw > 0) & (n_kept == 0)) and np.any((n_raw > 0) & (n_kept == n_raw))
    mb = _fill(w.eng, w.sdb, w.batch).pipeline_prepare(match_cap=len(w.opk) + 5, chunk_packages=chunk, raw=raw,
                                                       adv32=adv32)
    mb.pipeline_set_filter(mb.filter_opts(**mask))
    for _ in range(2):  # a second pass starts again from the raw lists
        _check_pass(mb, w, pk, ad, csr, adv32)
    mb.close()


def test_empty_severity_mask_keeps_nothing(world):
    w = world
    mb = _fill(w.eng, w.sdb, w.batch).pipeline_prepare(match_cap=len(w.opk), chunk_packages=512)
    mb.pipeline_set_filter(mb.filter_opts(severities=()))
    total, errp, _ = mb.pipeline_run()
    adv, rend = mb.pipeline_csr()
    assert total == len(w.opk) and errp == -1 and len(adv) == 0 and not rend.any()
    assert mb.pipeline_filter_stats() == (len(w.opk), 0)
    assert mb.pipeline_stats()["d2h_bytes"] == 4 * len(w.batch)
    mb.close()


def test_heavy_lists_compacted_in_order(oracle_built):
    """Lists of 255 advisories and more span several 64-entry rounds (and more than one group
    of rounds): they come back compacted and in order."""
    sdb = make_db(["debian 12"], 400, seed=21, max_adv=700)
    base = make_batch(sdb, 4, 300, [1], seed=2)
    names, vers = list(base.names), list(base.versions)
    for i in range(5, len(names), 97):
        names[i], vers[i] = b"linux", b"0.1"
    batch = SynthBatch(base.plat, names, vers, list(base.targets))
    w = World(sdb, batch, 21, _engine(sdb, 21))
    n_raw = np.bincount(w.opk, minlength=len(batch))
    assert n_raw.max() >= 255
    mask = dict(severities=("HIGH", "CRITICAL"), ignore_statuses=(5, 7))
    pk, ad, csr = w.expect(**mask)
    n_kept = np.bincount(pk, minlength=len(batch))
    heavy = n_raw >= 255
    assert np.all((n_kept[heavy] > 64) & (n_kept[heavy] < n_raw[heavy]))
    mb = _fill(w.eng, sdb, batch).pipeline_prepare(match_cap=len(w.opk) + 1, chunk_packages=512)
    mb.pipeline_set_filter(mb.filter_opts(**mask))
    _check_pass(mb, w, pk, ad, csr, False)
    mb.close()


def test_filter_lifecycle(world):
    """Set, change, clear, re-prepare on one batch."""
    w = world
    mb = _fill(w.eng, w.sdb, w.batch).pipeline_prepare(match_cap=len(w.opk), chunk_packages=512)
    for mask in (MASKS[0], MASKS[1], dict(severities=("UNKNOWN", "MEDIUM"), ignore_statuses=(2, 3))):
        mb.pipeline_set_filter(mb.filter_opts(**mask))
        _check_pass(mb, w, *w.expect(**mask), False)
    mb.pipeline_set_filter(None)
    _check_pass(mb, w, *w.unfiltered(), False)
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    mb.pipeline_prepare(match_cap=len(w.opk), chunk_packages=256)  # a new prepare clears the filter
    _check_pass(mb, w, *w.unfiltered(), False)
    mb.close()


def test_overflow_is_judged_on_the_raw_count(world):
    w = world
    raw = len(w.opk)
    pk, ad, csr = w.expect(**MASKS[0])
    assert len(pk) < raw - 1  # the kept findings alone would fit
    mb = _fill(w.eng, w.sdb, w.batch).pipeline_prepare(match_cap=raw - 1, chunk_packages=512)
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    with pytest.raises(OverflowError) as ei:
        mb.pipeline_run()
    assert ei.value.args[0] == raw
    with pytest.raises(RuntimeError):
        mb.pipeline_filter_stats()  # no completed pass
    mb.pipeline_prepare(match_cap=raw, chunk_packages=512)
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    _check_pass(mb, w, pk, ad, csr, False)
    mb.close()


def test_poisoned_package_still_reported(oracle_built):
    sdb = make_db(["debian 12", "ubuntu 22.04"], 300, seed=4)
    poison = [int(sdb.plat_keys[0][5]), int(sdb.plat_keys[1][7])]
    eng = _engine(sdb, 4, poison)
    batch = make_batch(sdb, 30, 300, [1, 1], seed=9, miss=0.0)
    mb = _fill(eng, sdb, batch).pipeline_prepare(match_cap=64 * len(batch), chunk_packages=700)
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    _, errp, _ = mb.pipeline_run()
    with pytest.raises(om.PoisonedKey) as ei:
        om.match(om.Prepared(sdb, batch, poisoned=poison), n_threads=1)
    assert errp == ei.value.pkg
    mb.close()


def test_refusals_leave_the_pass_unfiltered(world):
    from trivy_amd.batch import MatchBatch
    w = world
    never = MatchBatch(w.eng)
    with pytest.raises(ValueError, match="prepare"):
        never.pipeline_set_filter(never.filter_opts())
    never.close()
    mb = _fill(w.eng, w.sdb, w.batch).pipeline_prepare(match_cap=len(w.opk), chunk_packages=512)
    vid = w.filled[0]["VulnerabilityID"]
    with pytest.raises(ValueError, match="ignore rules"):
        mb.pipeline_set_filter(mb.filter_opts(severities=("LOW",), ignore_ids=(vid,)))
    with pytest.raises(ValueError, match="VEX"):
        mb.pipeline_set_filter(mb.filter_opts(severities=("LOW",), vex=([int(w.opk[0])], [vid])))
    _check_pass(mb, w, *w.unfiltered(), False)
    mb.close()


def test_red_hat_batch_refused():
    """redhat.go:146-187 merges over the unfiltered lists: a batch with a Red Hat target is
    refused, and its unfiltered pass stays what the device-resident path gives."""
    import trivy_amd
    from tools import synth_mix as sm
    from trivy_amd.batch import MatchBatch
    sdb = sm.make_mix_db(sm.C5_PLATS, 300, seed=0xC5C5)
    eng = trivy_amd.Engine(sdb.put(trivy_amd.DB()).finalize(), 0)
    batch = sm.make_mix_batch(sdb, 3000, sm.C5_WEIGHTS, seed=31)
    dev = MatchBatch(eng)
    sm.add_to(dev, sdb, batch)
    total, errp, bits = dev.run()
    assert errp == -1 and bits == 0 and total > 500
    pairs = dev.pairs()
    dev.close()
    mb = MatchBatch(eng)
    sm.add_to(mb, sdb, batch)
    mb.pipeline_prepare(match_cap=total, chunk_packages=1024)
    with pytest.raises(ValueError, match="Red Hat"):
        mb.pipeline_set_filter(mb.filter_opts(severities=("HIGH", "CRITICAL")))
    got_total, errp, _ = mb.pipeline_run()
    adv, rend = mb.pipeline_csr()
    assert errp == -1 and got_total == total and mb.pipeline_filter_stats() == (total, total)
    assert np.array_equal(adv, pairs[:, 1])
    assert np.array_equal(rend, np.cumsum(np.bincount(pairs[:, 0], minlength=len(mb))).astype(np.uint32))
    mb.close()


def test_classes_rebuilt_after_swap(oracle_built):
    """The advisory class table belongs to a table generation: after tvm_engine_swap a batch
    built on the new tables is filtered by the new DB's severities."""
    sdb1 = make_db(["debian 12", "ubuntu 22.04"], 300, seed=5)
    sdb2 = make_db(["debian 11", "debian 12", "ubuntu 22.04"], 400, seed=6)
    eng = _engine(sdb1, 5)
    b1 = make_batch(sdb1, 6, 200, [1, 1], seed=2)
    w1 = World(sdb1, b1, 5, eng)
    mb = _fill(eng, sdb1, b1).pipeline_prepare(match_cap=len(w1.opk), chunk_packages=512)
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    _check_pass(mb, w1, *w1.expect(**MASKS[0]), False)
    mb.close()
    eng2 = _engine(sdb2, 6)  # only for its DB handle
    eng.swap(eng2.db)
    b2 = make_batch(sdb2, 6, 200, [1, 1, 1], seed=3)
    w2 = World(sdb2, b2, 6, eng)
    mb = _fill(eng, sdb2, b2).pipeline_prepare(match_cap=len(w2.opk), chunk_packages=512)
    mb.pipeline_set_filter(mb.filter_opts(**MASKS[0]))
    _check_pass(mb, w2, *w2.expect(**MASKS[0]), False)
    mb.close()
