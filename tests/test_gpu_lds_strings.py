"""GPU: the dpkg-only match kernel reading its staged names and versions with LDS instructions and
keeping a listed lane's slot heads in flight across the list entry, both barriers and the packed
encode (auto, fused_k4_m2400_wseg_rec_r16) against the form that waits for the heads at the list
entry (fused_k4_m2400_wseg_rec_hw_r16), the kernel that encodes lane per package
(fused_k4_m2400_wseg_rec_lane_r16) and the Python oracle.  Batches of 1 to 3 tiles:

  1. names (found and absent) of every length 1..9, 15..17, 23..25, 31..33 with versions of 1 to 40
     bytes, ordered so that name and version starts take all four byte alignments in every wave and
     that a wave's first string starts at every offset 0..15 past its 16-byte window base (the
     first version of the batch is lengthened case by case);
  2. the last package of every wave (the last one: of the tile) a found name of 8, 16, 24 or 32
     bytes whose version, of every length mod 4, ends on the last byte of the wave's window: the
     dword reads past its end land in the two zero words behind the window;
  3. 100 distinct found names in a tile (every lane's slot heads come from another line of the
     index), absent names and an unknown platform interleaved, at 1, 257 and 300 packages.  Nothing
     in the C-ABI tells a name's home slot or the length of its chain (tvm_db_stats,
     tvm_db_layout_stats and tvm_db_row16_stats count platforms, keys, rows and layouts), so that
     both home-slot parities and a chain step occur rests on the number of names: 100 names in an
     index of at most 1/8 load leave no parity out (2^-99) and collide somewhere with probability
     about 1 - exp(-100^2 / (2 * 8 * 128)), over 99 %;
  4. the batches of 1 with one wave's strings past its staging window: that tile runs lane per
     package on global pointers, through the same helpers;
  5. an ordered launch on tile-head records, and a pipelined pass (the kernel with the result move
     compiled in) against the device-resident pairs."""
import collections
import functools

import numpy as np
import pytest

import row16_cases as c
from test_gpu_enc_balance import BY_LEN, UNKNOWN, run_segments
from test_gpu_row16 import hits_of, variant_index

pytestmark = pytest.mark.gpu

AUTO, WAIT, LANE = ("fused_k4_m2400_wseg_rec_r16", "fused_k4_m2400_wseg_rec_hw_r16",
                    "fused_k4_m2400_wseg_rec_lane_r16")
LENGTHS = list(range(1, 10)) + [15, 16, 17, 23, 24, 25, 31, 32, 33]
FOUND = {n: "abcdefghijklmnopqr"[i] * n for i, n in enumerate(LENGTHS)}
ABSENT = {n: "z" * (n - 1) + "#" for n in LENGTHS}
MANY = [f"late-{i:03d}" for i in range(100)]       # case 3: distinct found names
MANY_VERS = [BY_LEN[k] for k in (0, 4, 6, 12, 14, 23, 39)]
WAVE_WINDOW = 3072                                  # bytes of a wave's staging window


def records():
    recs = [c._rec(("data-source", c.DEB), {"ID": "debian", "Name": c.DEB, "URL": "https://x"})]
    j = 0
    for name in FOUND.values():  # a bound at every third length, the neighbours of one, and unfixed
        for f in BY_LEN[::3] + ["", "1.2.3-4+deb12u4", "1.2.3-5"]:
            recs.append(c._rec((c.DEB, name, c.vuln_id(j)), {"FixedVersion": f}))
            j += 1
    for name in MANY:  # a bound at every version these names are installed with
        for f in MANY_VERS:
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


def oracle_hits(segments):
    import oracle.drivers as od
    _, _, recs = world()
    pkgs, i = [], 0
    for bucket, names, vers in segments:
        assert len(names) == len(vers)
        for n, v in zip(names, vers):
            if bucket == c.DEB:
                pkgs.append({"ID": f"p{i}", "Name": n, "SrcName": n, "Version": v, "SrcVersion": v})
            i += 1
    assert 1 <= i <= 3 * 256
    return collections.Counter((v["PkgID"], v["VulnerabilityID"]) for v in od.debian_detect(recs, "12", None, pkgs))


def check(segments, min_hits):
    """The three kernels give one pair list, and it is the oracle's."""
    db, eng, _ = world()
    want = oracle_hits(segments)
    assert sum(want.values()) >= min_hits
    got = {}
    for name in (AUTO, WAIT, LANE):
        got[name], ran = run_segments(eng, segments, variant_index(name))
        assert ran == name
    assert np.array_equal(got[AUTO], got[WAIT]) and np.array_equal(got[AUTO], got[LANE])
    assert hits_of(db, got[AUTO]) == want
    return want


def starts(names, vers):
    """Arena offsets of every name and version: the strings lie back to back in batch order."""
    ns, vs, o = [], [], 0
    for n, v in zip(names, vers):
        ns.append(o)
        vs.append(o + len(n))
        o += len(n) + len(v)
    return ns, vs, o


def wave_sums(names, vers):
    return [sum(len(n) + len(v) for n, v in zip(names[w:w + 64], vers[w:w + 64])) for w in range(0, len(names), 64)]


def aligned_batch(n, shift):
    """n packages over the name lengths, found and absent, and the 40 version lengths; the first
    version is chosen so that wave 1 starts `shift` bytes past a 16-byte line."""
    names = [(FOUND if (i * 5 + i // 18) % 3 else ABSENT)[LENGTHS[(i * 7 + i // 64) % 18]] for i in range(n)]
    vers = [BY_LEN[(i * 13 + i // 40) % 40] for i in range(n)]
    rest = sum(len(a) + len(b) for a, b in zip(names[:64], vers[:64])) - len(vers[0])
    vers[0] = BY_LEN[(shift - rest - 1) % 16]  # 1..16 bytes
    return names, vers


def assert_alignments(names, vers, shift):
    ns, vs, _ = starts(names, vers)
    for w in range(0, len(names), 64):
        if len(names) - w >= 32:  # every whole (or half) wave: all four alignments of both strings
            assert {o % 4 for o in ns[w:w + 64]} == {0, 1, 2, 3}, w
            assert {o % 4 for o in vs[w:w + 64]} == {0, 1, 2, 3}, w
    assert ns[64] % 16 == shift
    assert max(wave_sums(names, vers)) + 15 <= WAVE_WINDOW  # every wave's window is staged


@pytest.mark.parametrize("shift", range(16))
def test_every_byte_alignment(shift):
    names, vers = aligned_batch(320, shift)
    assert_alignments(names, vers, shift)
    assert {len(x) for x in names} == set(LENGTHS) and {len(x) for x in vers} == set(range(1, 41))
    firsts = {starts(*aligned_batch(320, s))[0][w] % 16 for s in range(16) for w in (64, 128, 192, 256)}
    assert firsts == set(range(16))
    want = check([(c.DEB, names, vers)], min_hits=200)
    found = {f"p{i}" for i, x in enumerate(names) if x in FOUND.values()}
    assert {p for p, _ in want} == found  # the unfixed advisory of every found name, none of an absent one


@pytest.mark.parametrize("nlen", [8, 16, 24, 32])
def test_window_ends(nlen):
    """One tile: wave k ends with FOUND[nlen] and a version of 4 + k bytes (k = 0..3: every length
    mod 4) whose last byte is the last byte of a 16-byte line, the end of the wave's window."""
    names, vers = aligned_batch(256, 0)
    for k in range(4):
        last = 64 * k + 63
        names[last], vers[last] = FOUND[nlen], BY_LEN[3 + k]
        first = 64 * k  # the wave's first version takes up the slack
        vers[first] = BY_LEN[0]
        _, _, end = starts(names[:last + 1], vers[:last + 1])
        vers[first] = BY_LEN[(-end) % 16]  # 1 + (-end mod 16) bytes
        _, _, end = starts(names[:last + 1], vers[:last + 1])
        assert end % 16 == 0 and len(vers[last]) % 4 == k
    assert max(wave_sums(names, vers)) + 15 <= WAVE_WINDOW
    want = check([(c.DEB, names, vers)], min_hits=150)
    assert {"p63", "p127", "p191", "p255"} <= {p for p, _ in want}


def late_batch(n):
    names = [MANY[(i * 37) % 100] if i % 4 != 3 else f"gone-{i:03d}" for i in range(n)]
    vers = [MANY_VERS[(i * 3 + i // 7) % 7] if i % 9 else BY_LEN[(i * 11) % 40] for i in range(n)]
    return names, vers


@pytest.mark.parametrize("n", [1, 257, 300])
def test_heads_that_arrive_late(n):
    names, vers = late_batch(n)
    if n >= 256:
        assert len({x for x in names[:256] if x in MANY}) >= 64
    segments, i, k = [], 0, 0
    while i < n:  # runs of the unknown platform between the dpkg runs
        run = (70, 3, 61, 1, 130, 2)[k % 6]
        segments.append((UNKNOWN if k % 2 else c.DEB, names[i:i + run], vers[i:i + run]))
        i += run
        k += 1
    want = check(segments, min_hits=1 if n == 1 else n)
    assert all(names[int(p[1:])] in MANY for p, _ in want)
    # and all of one platform: 192 listed lanes in the first tile
    check([(c.DEB, names, vers)], min_hits=1 if n == 1 else 2 * n)


@pytest.mark.parametrize("shift", [1, 6, 11, 12])
def test_strings_past_the_staging_window(shift):
    """Wave 1 holds absent names of 90 bytes: its window is not staged, so tile 0 runs lane per
    package on global pointers (every alignment, as staged); tile 1 is packed."""
    names, vers = aligned_batch(320, shift)
    for i in range(64, 128):
        if names[i] not in FOUND.values():
            names[i] = f"gone-{i:03d}-" + "y" * 81
    assert_staged = wave_sums(names, vers)
    assert assert_staged[1] > WAVE_WINDOW + 16 and max(assert_staged[:1] + assert_staged[2:]) + 15 <= WAVE_WINDOW
    ns, vs, _ = starts(names, vers)
    assert {o % 4 for o in ns[:256]} == {0, 1, 2, 3} and {o % 4 for o in vs[:256]} == {0, 1, 2, 3}
    want = check([(c.DEB, names, vers)], min_hits=150)
    assert {p for p, _ in want} == {f"p{i}" for i, x in enumerate(names) if x in FOUND.values()}


def test_ordered_launch_on_tile_records():
    from test_gpu_tile_head import upload_mode
    from trivy_amd._lib import lib
    db, eng, _ = world()
    a, b = aligned_batch(300, 7), late_batch(300)
    segments = [(c.DEB, a[0] + b[0], a[1] + b[1])]
    want = oracle_hits(segments)
    assert sum(want.values()) >= 600
    plain, _ = run_segments(eng, segments, variant_index(AUTO))
    for name in (AUTO, WAIT, LANE):
        with upload_mode(eng, 3, False):
            pairs, ran = run_segments(eng, segments, variant_index(name))
            heads = lib().tvm_engine_last_head_launches(eng.h)
        assert (ran, heads) == (name, 1)
        assert np.array_equal(pairs, plain)
    assert hits_of(db, plain) == want


def test_pipelined_pass():
    """Three chunks of one tile: the launches carry the previous chunk's result move."""
    from test_gpu_pipeline import _pairs_of
    from trivy_amd._lib import lib
    from trivy_amd.batch import MatchBatch
    db, eng, _ = world()
    a, b = aligned_batch(320, 3), late_batch(300)
    names, vers = a[0] + b[0], a[1] + b[1]
    segments = [(c.DEB, names, vers)]
    want = oracle_hits(segments)
    assert sum(want.values()) >= 600
    resident, _ = run_segments(eng, segments, variant_index(AUTO))
    assert hits_of(db, resident) == want
    for name in (AUTO, WAIT, LANE):
        lib().tvm_engine_set_variant(eng.h, variant_index(name))
        try:
            mb = MatchBatch(eng)
            mb.add_many(c.DEB, [x.encode() for x in names], [x.encode() for x in vers])
            mb.pipeline_prepare(match_cap=len(resident) + 5, chunk_packages=256)
            total, errp, _ = mb.pipeline_run()
            assert errp == -1 and total == len(resident)
            assert mb.pipeline_stats()["chunks"] == 3
            assert lib().tvm_variant_name(lib().tvm_engine_last_variant(eng.h)).decode() == name
            adv, rend = mb.pipeline_csr()
            pk, ad = _pairs_of(adv[:total], rend[:len(names)])
            mb.close()
        finally:
            lib().tvm_engine_set_variant(eng.h, 0)
        assert np.array_equal(pk, resident[:, 0]) and np.array_equal(ad, resident[:, 1]), name
