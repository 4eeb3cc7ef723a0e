"""CPU: the host side of engine groups (trivy_amd/csrc/group.cpp) - the shard plan
(tvm_group_plan_host) equals trivy_amd.dist.target_shards boundary for boundary, and
tvm_group_open's argument checks and its refusal to run without a GPU."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from trivy_amd import dist
from trivy_amd._lib import errbuf, lib


def plan(target_end, weights, shards):
    te = np.ascontiguousarray(target_end, dtype=np.uint64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
    out = np.full(shards + 1, 0xDEAD, dtype=np.uint64)
    rc = lib().tvm_group_plan_host(len(te), te.ctypes.data if len(te) else None, w.ctypes.data if w is not None else None,
                                   shards, out.ctypes.data)
    assert rc == 0
    return [int(x) for x in out]


def check(sizes, weights, shards):
    """One input against dist.target_shards, plus the plan's own invariants."""
    te = np.cumsum(np.asarray(sizes, dtype=np.int64)) if len(sizes) else np.zeros(0, np.int64)
    n = int(te[-1]) if len(te) else 0
    begin = [0] + [int(x) for x in te[:-1]] if len(te) else []
    w = np.ones(n, dtype=np.uint32) if weights is None else weights
    want = dist.target_shards(begin, n, w, shards)
    got = plan(te, weights, shards)
    assert got == want, (sizes, shards)
    assert got[0] == 0 and got[-1] == n and len(got) == shards + 1
    assert all(a <= b for a, b in zip(got, got[1:]))
    edges = {0, n} | {int(x) for x in te}
    assert all(b in edges for b in got)


def test_plan_equals_target_shards_random():
    rng = np.random.default_rng(20)
    cases = 0
    for _ in range(300):
        t = int(rng.integers(1, 41))
        sizes = rng.integers(0, 301, t)
        if rng.random() < 0.3:
            sizes[rng.random(t) < 0.4] = 0  # empty targets, runs of them included
        n = int(sizes.sum())
        for weights in (None, np.minimum(rng.zipf(1.3, n), 1 << 20).astype(np.uint32)):
            for shards in range(1, 9):
                check(sizes, weights, shards)
                cases += 1
    assert cases == 300 * 2 * 8


def test_plan_edges():
    for shards in range(1, 9):
        check([], None, shards)                      # zero targets
        check([137], None, shards)                   # one target: every other shard is empty
        check([0], None, shards)
        check([5, 3], None, shards)                  # more shards than targets
        check([0, 0, 0], None, shards)               # nothing but empty targets
        check([70] * 3, np.array([1] * 140 + [1000] * 70, dtype=np.uint32), shards)
    assert plan([137], None, 3).count(137) >= 2      # the single target lands whole on one shard
    got = plan([10, 20, 30, 40], None, 2)              # target ends: four targets of 10
    assert got == [0, 20, 40]


def test_plan_bad_arguments():
    te = np.array([5, 3], dtype=np.uint64)  # not ascending
    out = np.zeros(3, dtype=np.uint64)
    assert lib().tvm_group_plan_host(2, te.ctypes.data, None, 2, out.ctypes.data) == 3
    te = np.array([3, 5], dtype=np.uint64)
    assert lib().tvm_group_plan_host(2, te.ctypes.data, None, 0, out.ctypes.data) == 3
    assert lib().tvm_group_plan_host(2, te.ctypes.data, None, 2, None) == 3
    assert lib().tvm_group_plan_host(2, None, None, 2, out.ctypes.data) == 3


def _db():
    import trivy_amd
    return trivy_amd.load_fixture_files([os.path.join(ROOT, "tests/golden/fixtures/ospkg/debian/debian.json")])


def test_group_open_refuses_bad_arguments():
    db = _db()
    one = (ctypes.c_int * 9)(*([0] * 9))
    neg = (ctypes.c_int * 2)(0, -1)
    for devs, n in ((one, 0), (one, 9), (None, 1), (neg, 2)):
        e = errbuf()
        assert not lib().tvm_group_open(db.h, devs, n, e, len(e))
        assert e.value.startswith(b"tvm_group_open: ")
    assert lib().tvm_group_size(None) == 0 and not lib().tvm_group_engine(None, 0)
    lib().tvm_group_close(None)
    assert not lib().tvm_group_batch_new(None)
    lib().tvm_group_batch_free(None)


def test_group_requires_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from trivy_amd.group import EngineGroup
    with pytest.raises(RuntimeError, match="no HIP device"):
        EngineGroup(_db(), [0, 0])
