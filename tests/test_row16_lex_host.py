"""CPU: the hot-row pair test as one lexicographic compare (common.h row16_pkg_lex / row16_test_lex,
the REC sweep's form) against the parent's boolean form (row16_pkg / row16_test) and against
the byte order of the keys, pair by pair on raw rows (tvm_row16_pair_host).  A dpkg-grammar DB never
builds a ROW_ALWAYS row or an R16_FALLBACK row inside a dpkg key's run (test_row16_host pins
fallback_rows == 0), so these two row kinds are reachable here only, on rows written by hand."""
import itertools
import random

from trivy_amd._lib import lib

WINDOW, P_CAP = 11, 7
ROW_ALWAYS = 1 << 31
INF_ROW = (0xFFFFFFFFFFFFFFFF, 0xFFFFFF80)   # DB::row16_build: a row without a bound
FALLBACK_ROW = (0, 0xFFFFFFFF)


def bounded_row(fk, P):
    w = fk[P:P + WINDOW].ljust(WINDOW, b"\0")
    n = min(len(fk) - P, WINDOW + 1)
    return int.from_bytes(w[:8], "big"), (int.from_bytes(w[8:], "big") << 8) | n


def pfx_word(prefix):
    return (int.from_bytes(prefix.ljust(8, b"\0"), "big") & ~0xFF) | len(prefix) if prefix else 0


def pair(key, valid, pfx, adv, row, lex):
    r = lib().tvm_row16_pair_host(key, len(key), valid, pfx, adv, row[1], row[0], lex)
    assert r >= 0
    return r & 1, r >> 1


def check(pk, valid, prefix, fk, adv, stats):
    """fk: the bound's key (starts with prefix), None = no bound, 'fallback' = a fall-back row."""
    P = len(prefix)
    row = FALLBACK_ROW if fk == "fallback" else INF_ROW if fk is None else bounded_row(fk, P)
    old_m, old_slow = pair(pk, valid, pfx_word(prefix), adv, row, 0)
    new_m, new_slow = pair(pk, valid, pfx_word(prefix), adv, row, 1)
    assert old_slow == new_slow, (pk, valid, prefix, fk, adv)
    ik = pk if valid else b""
    n = P + WINDOW
    tie = fk not in (None, "fallback") and valid and ik[:n] == fk[:n] and len(ik) > n and len(fk) > n
    assert new_slow == int(fk == "fallback" or tie), (pk, valid, prefix, fk)
    if new_slow:
        stats["slow"] += 1
        return
    assert old_m == new_m, (pk, valid, prefix, fk, adv)
    want = bool(adv & ROW_ALWAYS) or (bool(valid) and (fk is None or ik < fk))
    assert new_m == int(want), (pk, valid, prefix, fk, adv)
    stats["match" if want else "miss"] += 1


def test_strict_cases():
    stats = dict.fromkeys(("slow", "match", "miss"), 0)
    pre = b"\x00\x04\x01\xae\x04\x02\x03"
    for P in (0, 3, 7):
        prefix = pre[:P]
        bounds = [prefix, prefix + b"\x00", prefix + b"\x01", prefix + b"\xff" * 11, prefix + b"\xff" * 12,
                  prefix + b"\x05" * 11, prefix + b"\x05" * 12, prefix + b"\x05" * 11 + b"\x06", prefix + b"\x05" * 10]
        pkgs = bounds + [b"", pre[:max(P - 1, 0)], prefix[:-1] + b"\xff" if P else b"\xff", prefix + b"\x05" * 20,
                         prefix + b"\xff" * 24, (prefix[:-1] + bytes([prefix[-1] - 1])) if P and prefix[-1] else b"\x00"]
        for pk, fk, valid, adv in itertools.product(pkgs, bounds + [None, "fallback"], (1, 0), (5, 5 | ROW_ALWAYS)):
            check(pk, valid, prefix, fk, adv, stats)
    assert min(stats.values()) > 50, stats


def test_random_pairs():
    rnd = random.Random(16)
    stats = dict.fromkeys(("slow", "match", "miss"), 0)
    alpha = [0, 0, 1, 2, 0xFF]
    for _ in range(6000):
        P = rnd.randint(0, P_CAP)
        prefix = bytes(rnd.choice(alpha) for _ in range(P))
        fk = prefix + bytes(rnd.choice(alpha) for _ in range(rnd.choice([0, 1, 2, 10, 11, 12, 13, 17])))
        r = rnd.random()
        if r < 0.5:      # shares the bound's first bytes: windows tie or differ late
            cut = rnd.randint(0, len(fk))
            pk = fk[:cut] + bytes(rnd.choice(alpha) for _ in range(rnd.randint(0, 14)))
        elif r < 0.6:
            pk = fk
        else:
            pk = bytes(rnd.choice(alpha) for _ in range(rnd.randint(0, 24)))
        bound = rnd.choice([fk, fk, fk, None, "fallback"])
        check(pk[:40], int(rnd.random() < 0.9), prefix, bound, 7 | (ROW_ALWAYS if rnd.random() < 0.1 else 0), stats)
    assert min(stats.values()) > 200, stats
