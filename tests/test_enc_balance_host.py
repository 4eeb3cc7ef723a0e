"""CPU: the arithmetic of the balanced match kernel's encoder work list (verkey.h enc_bal_bucket /
enc_bal_item through tvm_enc_bal_*_host) against a Python restatement: a version's bucket is its
dword count (the last bucket open-ended), and work item i of a tile is found by counting through the
buckets longest first.  Empty lists, one bucket holding all 256 packages of a tile, every bucket
boundary of mixed lists, and the items past the end of a list."""
import ctypes
import random

import pytest

from trivy_amd._lib import lib

TILE = 256


def n_buckets():
    return lib().tvm_enc_bal_buckets_host()


def bucket_ref(n, nb):
    return min((n + 3) // 4, nb - 1)


def item_ref(counts, item):
    """(bucket, index) of work item `item`, or None past the end: buckets from the last to the first."""
    first = 0
    for b in reversed(range(len(counts))):
        if item < first + counts[b]:
            return b, item - first
        first += counts[b]
    return None


def item_host(counts, item):
    arr = (ctypes.c_uint32 * len(counts))(*counts)
    b, i = ctypes.c_uint32(0xDEAD), ctypes.c_uint32(0xBEEF)
    rc = lib().tvm_enc_bal_item_host(arr, item, ctypes.byref(b), ctypes.byref(i))
    assert rc in (0, 1), rc
    if rc == 0:
        assert (b.value, i.value) == (0xDEAD, 0xBEEF)  # nothing written past the end
        return None
    return b.value, i.value


def check_all(counts):
    total = sum(counts)
    seen = set()
    for item in range(TILE + 2):
        got, want = item_host(counts, item), item_ref(counts, item)
        assert got == want, (counts, item, got, want)
        if item < total:
            assert got is not None and got[1] < counts[got[0]]
            seen.add(got)
        else:
            assert got is None
    assert len(seen) == total  # every entry of every region is handed out exactly once


def test_buckets_of_version_lengths():
    nb = n_buckets()
    assert nb == 8
    for n in list(range(0, 80)) + [255, 256, 1023, 4096, 65535]:
        assert lib().tvm_enc_bal_bucket_host(n) == bucket_ref(n, nb), n
    # every bucket boundary: 4b bytes still take b dwords, one more byte takes b + 1
    for b in range(1, nb - 1):
        assert lib().tvm_enc_bal_bucket_host(4 * b) == b and lib().tvm_enc_bal_bucket_host(4 * b + 1) == min(b + 1, nb - 1)
    assert lib().tvm_enc_bal_bucket_host(0) == 0 and lib().tvm_enc_bal_bucket_host(1) == 1


def test_empty_list():
    check_all([0] * n_buckets())


@pytest.mark.parametrize("bucket", range(8))
def test_one_bucket_holds_the_tile(bucket):
    counts = [0] * n_buckets()
    counts[bucket] = TILE
    check_all(counts)
    assert item_host(counts, 0) == (bucket, 0) and item_host(counts, TILE - 1) == (bucket, TILE - 1)


def test_single_entries_and_boundaries():
    nb = n_buckets()
    for b in range(nb):  # one entry in one bucket
        counts = [0] * nb
        counts[b] = 1
        check_all(counts)
    check_all([1] * nb)            # every boundary one item apart
    check_all([32] * nb)           # a full tile spread evenly
    check_all([0, 64, 0, 64, 0, 64, 0, 64])  # empty buckets between full waves
    check_all([64, 0, 63, 1, 0, 65, 0, 63])
    check_all([TILE - 1, 0, 0, 0, 0, 0, 0, 1])
    check_all([1, 0, 0, 0, 0, 0, 0, TILE - 1])


def test_longest_bucket_first():
    nb = n_buckets()
    counts = [3, 0, 5, 7, 0, 2, 1, 4]
    order = [item_host(counts, i)[0] for i in range(sum(counts))]
    assert order == sorted(order, reverse=True) and order[0] == nb - 1 and order[-1] == 0


def test_random_lists():
    rng = random.Random(5)
    nb = n_buckets()
    for _ in range(200):
        total = rng.choice([1, 63, 64, 65, 192, 255, 256])
        counts = [0] * nb
        for _ in range(total):
            counts[rng.randrange(nb) if rng.random() < 0.7 else rng.choice([2, 3, 4])] += 1
        check_all(counts)


def test_null_arguments():
    arr = (ctypes.c_uint32 * 8)()
    b = ctypes.c_uint32()
    assert lib().tvm_enc_bal_item_host(None, 0, ctypes.byref(b), ctypes.byref(b)) == -1
    assert lib().tvm_enc_bal_item_host(arr, 0, None, ctypes.byref(b)) == -1
