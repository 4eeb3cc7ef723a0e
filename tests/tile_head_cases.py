"""Batches for the tile-head tests (test_tile_head_host.py, test_gpu_tile_head.py): a dpkg DB whose
keys have clearly different row counts, runs of packages with chosen string sizes per 64-package
group, and the host hook's view of what an upload builds (tvm_tile_heads_host)."""
import ctypes

import numpy as np

import row16_cases as c

UNKNOWN = "nosuch 1"
STEM = "1.2.3-4+deb12u5~rc6.7.8.9.10.11.12.13.14"  # every prefix of it is a version
BY_LEN = [STEM[:n] for n in range(1, 41)]
HEAVY_ROWS = 100
FOUND = ["pkg", "other", "n" * 31, "k" * 33]

HEAD = np.dtype([("base", "<u8"), ("tile", "<u4"), ("d", "<u4", 4), ("pad", "<u4")])
assert HEAD.itemsize == 32


def records():
    recs = [c._rec(("data-source", c.DEB), {"ID": "debian", "Name": c.DEB, "URL": "https://x"})]
    j = 0
    for name in FOUND:
        for f in BY_LEN[::3 if name != "pkg" else 1] + ["", "1.2.3-4+deb12u4", "1.2.3-5"]:
            recs.append(c._rec((c.DEB, name, c.vuln_id(j)), {"FixedVersion": f}))
            j += 1
    for i in range(HEAVY_ROWS):  # the key that makes a tile the heaviest
        recs.append(c._rec((c.DEB, "heavy", c.vuln_id(j)), {"FixedVersion": f"1.2.{i}-1"}))
        j += 1
    return recs


def absent(i, pad=0):
    return f"absent-{i:04d}" + "y" * pad


def light_heavy_600():
    """600 packages, a partial last tile: tile 0 all absent names, tile 1 light keys, tile 2 (88
    packages) the 100-row key - the predicted rows put the tiles in the order 2, 1, 0."""
    names = [absent(i) for i in range(256)] + [FOUND[i % 2] for i in range(256)] + ["heavy"] * 88
    vers = [BY_LEN[(5 * i) % 40] for i in range(512)] + [f"1.2.{(7 * i) % 120}-1" for i in range(88)]
    return [(c.DEB, names, vers)]


def group(target, salt, first):
    """64 packages whose names and versions take exactly `target` bytes: three found names in four
    with versions of 1 to 12 bytes (one in eight up to 40), the absent names padded to the sum."""
    names, vers = [], []
    for i in range(64):
        names.append(None if i % 4 == 0 else FOUND[(i + salt) % 2] if i % 16 else FOUND[2 + (i // 16 + salt) % 2])
        vers.append(BY_LEN[(i * 13 + salt) % 40] if i % 8 == 1 else BY_LEN[(7 * i + salt) % 12])
    rest = target - sum(len(n) for n in names if n) - sum(len(v) for v in vers) - 16 * len(absent(0))
    assert rest >= 0, (target, rest)
    k = 0
    for i in range(64):
        if names[i] is None:
            names[i] = absent(first + i, rest // 16 + (1 if k < rest % 16 else 0))
            k += 1
    assert sum(len(n) + len(v) for n, v in zip(names, vers)) == target
    return names, vers


def groups_of(targets):
    """One dpkg run of 64-package groups with the given string sizes; returns the segments and each
    group's staging window in bytes (from the 16-byte line its first string lies in)."""
    names, vers, windows, off = [], [], [], 0
    for g, t in enumerate(targets):
        n, v = group(t, g, 64 * g)
        names += n
        vers += v
        windows.append(off % 16 + t)
        off += t
    return [(c.DEB, names, vers)], windows


# a wave's window takes one, two or three 1024-byte steps of loads: just under and at 1024 and
# 2048 bytes, at the largest staged size (3072), and one group past it in the last tile, whose
# window is not staged (the tile runs lane per package on the record's offsets as global offsets)
WINDOW_TARGETS = [1024, 2048, 3072, 1023, 1009, 2047, 2033, 1024, 3100, 1024, 1024, 1024]
WINDOWS = [1024, 2048, 3072, 1023, 1024, 2047, 2048, 1024, 3100, 1036, 1036, 1036]


def host_view(db, segments, min_tiles):
    """(order, head records, padded group offsets) of tvm_tile_heads_host; order / heads are None
    below the ordering threshold."""
    from trivy_amd._lib import lib
    names = [n.encode() for _, ns, _ in segments for n in ns]
    vers = [v.encode() for _, _, vs in segments for v in vs]
    n = len(names)
    nt = (n + 255) // 256
    blob = b"".join(names) + b"".join(vers)
    nlen = np.array([len(x) for x in names], dtype=np.uint32)
    vlen = np.array([len(x) for x in vers], dtype=np.uint32)
    noff = np.concatenate([[0], np.cumsum(nlen[:-1], dtype=np.uint64)]).astype(np.uint64)
    voff = (int(nlen.sum()) + np.concatenate([[0], np.cumsum(vlen[:-1], dtype=np.uint64)])).astype(np.uint64)
    buckets = (ctypes.c_char_p * len(segments))(*[b.encode() for b, _, _ in segments])
    run_n = np.array([len(ns) for _, ns, _ in segments], dtype=np.uint64)
    order = np.zeros(nt, dtype=np.uint32)
    heads = np.zeros(nt, dtype=HEAD)
    toff = np.zeros(4 * nt + 1, dtype=np.uint64)
    rc = lib().tvm_tile_heads_host(db.h, len(segments), buckets, run_n.ctypes.data, blob, noff.ctypes.data,
                                   nlen.ctypes.data, voff.ctypes.data, vlen.ctypes.data, min_tiles, order.ctypes.data,
                                   heads.ctypes.data, toff.ctypes.data, nt)
    assert rc in (0, nt), rc
    return (order, heads, toff) if rc else (None, None, toff)


def check_heads(order, heads, toff):
    """Every grid position's record names order[b] and carries that tile's five group offsets."""
    nt = len(order)
    assert sorted(order.tolist()) == list(range(nt))
    for b in range(nt):
        t = int(order[b])
        h = heads[b]
        assert int(h["tile"]) == t
        five = [int(h["base"])] + [int(h["base"]) + int(x) for x in h["d"]]
        assert five == [int(x) for x in toff[4 * t:4 * t + 5]], (b, t)
