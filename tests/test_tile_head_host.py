"""CPU: the tile-head records an upload builds beside the tile order (csrc/engine.h TileHead,
through tvm_tile_heads_host): one record per grid position with the tile of the launch order and
that tile's five group offsets, the padded offsets (the arena end) in the record of a partial last
tile, and none for a batch below the ordering threshold."""
import functools

import numpy as np

import row16_cases as c
import tile_head_cases as th


@functools.lru_cache(maxsize=None)
def db():
    import trivy_amd
    d = trivy_amd.DB()
    d.put_records(th.records())
    return d.finalize()


def test_records_follow_a_non_identity_order():
    segs = th.light_heavy_600()
    order, heads, toff = th.host_view(db(), segs, 2)
    assert order.tolist() == [2, 1, 0]  # heaviest first: the 100-row key, the light keys, the absent names
    th.check_heads(order, heads, toff)
    assert np.all(np.diff(toff.astype(np.int64)) >= 0)


def test_partial_last_tile_carries_the_arena_end():
    segs = th.light_heavy_600()
    order, heads, toff = th.host_view(db(), segs, 1)
    end = sum(len(n) + len(v) for _, ns, vs in segs for n, v in zip(ns, vs))
    b = order.tolist().index(2)  # tile 2: 88 packages, groups 8 and 9 (24 packages) hold strings
    h = heads[b]
    five = [int(h["base"])] + [int(h["base"]) + int(x) for x in h["d"]]
    assert five[2:] == [end, end, end] and five[0] < five[1] < end
    assert toff[-1] == end


def test_group_sizes_reach_the_records():
    segs, windows = th.groups_of(th.WINDOW_TARGETS)
    assert windows == th.WINDOWS
    order, heads, toff = th.host_view(db(), segs, 3)
    th.check_heads(order, heads, toff)
    assert np.diff(toff.astype(np.int64)).tolist() == th.WINDOW_TARGETS


def test_unknown_platform_tiles_get_records():
    names, vers = [f"x{i}" for i in range(300)], ["1.0"] * 300
    segs = [(c.DEB, ["pkg"] * 300, ["1.2.3"] * 300), (th.UNKNOWN, names, vers)]
    order, heads, toff = th.host_view(db(), segs, 1)
    assert len(order) == 3 and order[0] == 0  # the unknown platform's packages predict no rows
    th.check_heads(order, heads, toff)


def test_below_the_threshold_builds_none():
    segs = th.light_heavy_600()
    for min_tiles in (4, 1024, 0):  # 0: the default threshold, 1 024 tiles
        order, heads, toff = th.host_view(db(), segs, min_tiles)
        assert order is None and heads is None
        assert len(toff) == 13 and toff[-1] == toff[10]
    order, _, _ = th.host_view(db(), segs, 3)
    assert order is not None
