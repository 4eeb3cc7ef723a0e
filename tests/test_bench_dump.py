"""bench.py --dump-outputs (dump_outputs): the files of a short match list hold all of it; a list
longer than DUMP_ROWS is sampled with a fixed seed (the same rows on every call), in float64,
below the 64 MB a dump may take."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = ["status", "matches", "match_rows", "package_matches"]


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_short_list_is_dumped_whole(tmp_path):
    pairs = np.array([[10, 7], [10, 9], [12, 1], [14, 0], [14, 3], [14, 2 ** 31 + 5]], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "o"), pairs, 10, 5, (6, -1, 0))  # a new directory is created
    got = _load(str(tmp_path / "o"))
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["status"].tolist() == [6, -1, 0]
    assert np.array_equal(got["matches"], pairs.astype(np.float64))  # exact, above 2^31 too
    assert got["match_rows"].tolist() == list(range(6))
    assert got["package_matches"].tolist() == [[10, 2], [11, 0], [12, 1], [13, 0], [14, 3]]


def test_long_list_is_sampled_the_same_way_every_time(tmp_path):
    n_pkgs = bench.DUMP_ROWS // 2 + 1000
    rng = np.random.default_rng(1)
    pkg = np.sort(rng.integers(0, n_pkgs, size=bench.DUMP_ROWS + 5000)).astype(np.uint32)
    pairs = np.stack([pkg, np.arange(len(pkg), dtype=np.uint32)], axis=1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), pairs, 0, n_pkgs, (len(pairs), -1, 0))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert all(np.array_equal(a[n], b[n]) for n in NAMES)
    rows = a["match_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0) and rows[-1] < len(pairs)
    assert np.array_equal(a["matches"], pairs[rows].astype(np.float64))
    pk = a["package_matches"][:, 0].astype(np.int64)
    assert len(pk) == bench.DUMP_ROWS // 2 and np.all(np.diff(pk) > 0)
    assert np.array_equal(a["package_matches"][:, 1], np.bincount(pkg, minlength=n_pkgs)[pk])
    assert sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) for n in NAMES) <= 64e6
