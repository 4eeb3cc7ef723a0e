"""CPU: edges of the match kernel's dpkg key builder (verkey.h deb_fast_key), which writes its
tokens unconditionally at a clamped position of the lane's 44-byte slot: keys that end at and past
the 32-byte cap, digit runs at the byte-count boundaries of the number token, empty revisions and
epochs.  Every case runs on a pre-filled slot (tvm_deb_fast_key_slot_host) at all four dword
alignments and is checked against the generic encoder (deb_encode through tvm_version_key) for the
key bytes, the length and the outcome, and the slot's bytes from offset 40 on must come back
untouched (the bound a wider token store would have to keep)."""
import ctypes

import pytest

from trivy_amd._lib import lib

SLOT = 64       # bytes handed to the builder (a lane's slot is the first 44)
GUARD_FROM = 40  # the builder may write [0, 40)
CAP = 32        # longest key the builder keeps
FILL = 0xEE

_BUF = ctypes.create_string_buffer(1 << 12)


def generic(v):
    n = lib().tvm_version_key(1, v, len(v), _BUF, len(_BUF))
    return None if n < 0 else _BUF.raw[:n]


def fast_slot(v, shift):
    """(outcome, key or None) of one run on a pre-filled slot; asserts the guard bytes."""
    slot = (ctypes.c_uint8 * SLOT)(*([FILL] * SLOT))
    n = lib().tvm_deb_fast_key_slot_host(v, len(v), shift, slot, SLOT)
    assert n >= -2, (v, shift, n)
    raw = bytes(slot)
    assert raw[GUARD_FROM:] == bytes([FILL]) * (SLOT - GUARD_FROM), (v, shift, raw[GUARD_FROM:])
    if n == -2:
        return "fallback", None
    if n == -1:
        return "invalid", None
    return "ok", raw[:n]


def check(v, want):
    """want: 'ok' / 'invalid' / 'fallback', stated by the case; the key comes from deb_encode."""
    key = generic(v)
    assert (key is None) == (want == "invalid") or want == "fallback", (v, want, key)
    for sh in range(4):
        got, k = fast_slot(v, sh)
        assert got == want, (v, sh, got, want)
        if want == "ok":
            assert k == key and len(k) == len(key) <= CAP, (v, sh, k, key)
    return key


FAMILIES = {
    "letters": lambda n: b"1" + b"a" * n,                    # ends on a code byte
    "run3": lambda n: b"1" + b"a" * n + b"65536",            # the closing token carries 3 value bytes
    "rev4": lambda n: b"1" + b"a" * n + b"-16777216",        # a revision whose closing token carries 4
    "dots": lambda n: b"1" + b".1" * n,                      # a token per byte pair all along the key
}


def by_length(make):
    """key length -> version of one family (n = 0 .. 48)."""
    out = {}
    for n in range(49):
        v = make(n)
        k = generic(v)
        assert k is not None, v
        out.setdefault(len(k), v)
    return out


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_keys_that_end_at_the_cap(family):
    vs = by_length(FAMILIES[family])
    step = 3 if family == "dots" else 1  # ".1" adds a code byte and a two-byte token
    hit = [L for L in (27, 28, 31, 32, 33) if L in vs]
    assert len(hit) == 5 if step == 1 else len(hit) >= 1, (family, sorted(vs))
    for L, v in sorted(vs.items()):  # every length the family reaches: below, at and far past the cap
        check(v, "ok" if L <= CAP else "fallback")
    assert max(vs) > GUARD_FROM  # keys that would run past the slot's writable bytes


RUNS = [0, 255, 256, 65535, 65536, 1 << 24, (1 << 32) - 1]


@pytest.mark.parametrize("value", RUNS)
@pytest.mark.parametrize("zeros", [0, 1, 5])
def test_digit_run_values(value, zeros):
    run = b"0" * zeros + b"%d" % value
    # a run of more than 9 significant digits is the generic encoder's (2^32 - 1 has 10)
    want = "fallback" if len(b"%d" % value) > 9 else "ok"
    keys = [check(v, want) for v in (run, b"1." + run, b"1." + run + b"-1", b"2:1-" + run, b"1." + run + b"a", b"1~" + run + b"+b2")]
    if value and zeros:  # leading zeros do not change the key
        assert keys[1] == generic(b"1." + b"%d" % value)


def test_nine_and_ten_digit_runs():
    check(b"123456789", "ok")
    check(b"1.999999999-999999999", "ok")
    check(b"1234567890", "fallback")
    check(b"1.1000000000", "fallback")
    check(b"0123456789", "ok")          # ten digits, nine significant
    check(b"1.0000000000-1", "ok")      # ten zeros: the value 0
    check(b"1-4294967296", "fallback")


def test_revisions_and_epochs():
    check(b"1.0-", "ok")                # empty revision
    check(b"1-2-", "ok")                # trailing '-': the last one splits, the revision is empty
    check(b"1-", "ok")
    assert generic(b"1.0-") == generic(b"1.0")  # an empty revision sorts as none
    check(b"1:1.0", "ok")
    check(b"1:1.0-1", "ok")
    check(b"123456789:1.0-1", "ok")     # the longest epoch the builder takes
    check(b"999999999:9", "ok")
    check(b"1234567890:1.0-1", "fallback")
    check(b"0:1.0-1", "ok")
    assert generic(b"0:1.0-1") == generic(b"1.0-1")
    check(b"-", "invalid")
    check(b"1:-1", "invalid")
    check(b"1:1.0-1:2", "invalid")      # a ':' in the revision
    check(b"1.0 1", "invalid")
    check(b"1.\xc3\xa9", "fallback")    # non-ASCII: the rune-decoding check


def test_long_keys_with_epoch_and_revision():
    """Keys of 30 to 36 bytes built from every token kind: the store of the last tokens is clamped."""
    seen = set()
    for n in range(12):
        v = b"7:" + b"1.22.333" + b"+x" * n + b"-65536~rc256"
        k = generic(v)
        assert k is not None
        seen.add(len(k))
        check(v, "ok" if len(k) <= CAP else "fallback")
    assert any(L <= CAP for L in seen) and any(CAP < L for L in seen) and any(L > GUARD_FROM - 4 for L in seen), sorted(seen)
