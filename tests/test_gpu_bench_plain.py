"""GPU: a plain `bench.py --gpus 1` run prints the headline figure alone (the other legs wait for
--full), times the steps it was asked for, and with --dump-outputs writes the last timed step's
match list: element for element the oracle's match (oracle/match.c) of the same seeded batch."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FULL_ONLY = ["roofline", "cpu_baseline", "vulns", "end_to_end", "fresh_batch", "fill_info", "dropin_latency", "strong"]


def test_plain_run_is_the_headline_alone_and_dumps_the_match_list(tmp_path, oracle_built):
    sys.path.insert(0, ROOT)
    import bench
    from oracle import match as om
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c2", "--keys-per-plat", "3000", "--targets", "200", "--pkgs-per-target", "400",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["metric"] == "packages matched/sec (node)" and line["unit"] == "packages/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8" and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(200 * 400 / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]

    wl = bench.C2(argparse.Namespace(keys_per_plat=3000, targets=200, pkgs_per_target=400))
    opk, oad = om.match(om.Prepared(wl.sdb, wl.batch), n_threads=8)
    got = {n: np.load(str(out / (n + ".npy"))) for n in ("status", "matches", "match_rows", "package_matches")}
    assert sorted(os.listdir(str(out))) == sorted(n + ".npy" for n in got)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["status"].tolist() == [len(opk), -1, 0] and line["config"]["matches_rank0"] == len(opk)
    assert np.array_equal(got["matches"], np.stack([opk, oad], axis=1).astype(np.float64))
    assert np.array_equal(got["match_rows"], np.arange(len(opk)))
    assert np.array_equal(got["package_matches"][:, 0], np.arange(wl.n))
    assert np.array_equal(got["package_matches"][:, 1], np.bincount(opk, minlength=wl.n))
