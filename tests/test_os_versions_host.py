"""CPU: the adversarial OS-package versions of os_version_cases.py reach the branches they are
meant for - shown from the oracle's comparators and the host build of the key encoder alone,
before any GPU sees them - and the host key order agrees with the oracle on exactly the pairs
the GPU tests compare (so a later GPU failure is the kernel's, not the encoder's).

A pair is (installed version, FixedVersion) of a package and an advisory its driver compares:
under a found name, past the driver's own exceptions (an empty FixedVersion, Alpine's "0", an
Oracle advisory of another ksplice tag, a rocky / Red Hat entry of another arch or CPE set).
Every test prints what it measured (pytest -s shows it)."""
import collections
import functools

import pytest

import oracle.drivers as od
import os_version_cases as oc
from test_verkey_host import key

CMP = {1: od.deb_cmp, 2: od.apk_cmp, 3: od.rpm_cmp}


@functools.lru_cache(maxsize=None)
def records_of(fid):
    return od.Records(oc.family(fid).records)


def compared(fam, t, db, p, name, arch):
    """The advisories (dicts with FixedVersion / AffectedVersion / VulnerabilityID) the driver of
    `fam` compares package p's version with; None when the name has no bucket."""
    if fam.kind == "redhat":
        if not db.raw("Red Hat", name):
            return None
        cs, nvr = oc.rc.rh_cpe_key(p)
        advs = db.get_redhat(name, list(cs), [nvr])
        return [a for a in advs if not (a["Arches"] and arch != "noarch" and arch not in a["Arches"])]
    if not db.raw(t.bucket, name):
        return None
    if fam.kind == "rocky":
        return db.get_rocky(t.bucket, name, arch)
    advs = db.get(t.bucket, name)
    if fam.kind == "oracle":
        advs = [a for a in advs if od.extract_ksplice(a.get("FixedVersion", "")) == od.extract_ksplice(p["Release"])]
    return advs


@functools.lru_cache(maxsize=None)
def measure(fid):
    """The family's pairs and what they reach."""
    fam, db, cmp = oc.family(fid), records_of(fid), CMP[oc.family(fid).grammar]
    st = collections.Counter()
    bad = []
    for t in fam.targets:
        for i, name, inst, arch in fam.batch_rows(t):
            p = t.pkgs[i]
            advs = compared(fam, t, db, p, name, arch)
            if advs is None:
                st["absent"] += 1
                continue
            st["found"] += 1
            ka = key(fam.grammar, inst)
            valid = cmp(inst, "1") != 2
            if (ka is None) == valid:
                bad.append((inst, "parse", valid))
            if not valid:
                st["installed_unparsable"] += 1
                continue
            st["key<=16" if len(ka) <= 16 else "key17-32" if len(ka) <= 32 else "key>32"] += 1
            groups = collections.defaultdict(list)
            for a in advs:
                fixed, aff = a.get("FixedVersion", ""), a.get("AffectedVersion", "")
                if fam.kind == "alpine" and aff != "":
                    without = od.alpine_vulnerable(inst, {"FixedVersion": fixed})
                    if od.alpine_vulnerable(inst, a) != without:
                        st["decided_by_affected"] += 1
                    kl = key(2, aff)
                    if kl is not None:  # the lower bound's order, as cmp_be sees it
                        r = od.apk_cmp(aff, inst)
                        if ((kl > ka) - (kl < ka)) != r:
                            bad.append((aff, inst, r))
                if fixed == "" or (fam.kind == "alpine" and fixed == "0"):
                    continue
                r = cmp(inst, fixed)
                kb = key(fam.grammar, fixed)
                if r == 3:
                    st["fixed_unparsable"] += 1
                    if kb is not None:
                        bad.append((fixed, "parse", False))
                    continue
                if kb is None:
                    bad.append((fixed, "parse", True))
                    continue
                st["pairs"] += 1
                st["less" if r < 0 else "equal" if r == 0 else "greater"] += 1
                if ((ka > kb) - (ka < kb)) != r:
                    bad.append((inst, fixed, r))
                if ka[:16] == kb[:16] and len(ka) > 16 and len(kb) > 16:
                    st["tie16_tail" if len(ka) <= 32 else "tie16_spill"] += 1
                if ka[:32] == kb[:32] and len(ka) > 32 and len(kb) > 32:
                    st["tie32"] += 1
                if ka == kb and inst != fixed:
                    st["equal_keys_other_text"] += 1
                if fam.kind == "redhat" and r < 0:
                    groups[a["VulnerabilityID"]].append(fixed)
            for fixes in groups.values():  # the merge: greatest FixedVersion in rpm order
                if len(fixes) > 1:
                    st["rh_groups"] += 1
                    best = fixes[0]
                    for f in fixes[1:]:
                        if od.rpm_cmp(best, f) < 0:
                            best = f
                    if od.rpm_string(best) != od.rpm_string(max(fixes)):
                        st["rh_groups_text_differs"] += 1
    return st, bad


@pytest.mark.parametrize("fid", oc.FAMILY_IDS)
def test_family_reaches_its_branches(oracle_built, fid):
    fam = oc.family(fid)
    st, bad = measure(fid)
    n_pkgs = sum(len(t.pkgs) for t in fam.targets)
    names = {r["path"][1] for r in fam.records if r["path"][0] not in ("data-source", "Red Hat CPE")}
    per_name = collections.Counter(r["path"][1] for r in fam.records if r["path"][0] not in ("data-source", "Red Hat CPE"))
    unp = st["installed_unparsable"] / st["found"]
    shares = {k: st[k] / st["pairs"] for k in ("less", "greater", "equal")}
    print(f"\n{fid}: packages {n_pkgs} (found names {st['found']}, absent {st['absent']}), pairs {st['pairs']}, "
          f"installed unparsable {unp:.1%}, fixed unparsable {st['fixed_unparsable']}, "
          + ", ".join(f"{k} {v:.1%}" for k, v in shares.items())
          + f", keys <=16 / 17-32 / >32: {st['key<=16']} / {st['key17-32']} / {st['key>32']}, ties 16 tail / 16 spill / 32 / "
          f"equal keys: {st['tie16_tail']} / {st['tie16_spill']} / {st['tie32']} / {st['equal_keys_other_text']}"
          + (f", decided by AffectedVersion {st['decided_by_affected']}" if fid == "alpine" else "")
          + (f", merge groups {st['rh_groups']} (greatest differs from text: {st['rh_groups_text_differs']})"
             if fid == "redhat" else ""))
    assert not bad, bad[:10]  # host key order == the oracle's comparator on these very pairs
    assert 1250 <= n_pkgs <= 1350 and n_pkgs > 5 * 256  # five tiles of 256 and a partial sixth
    assert len(names) <= 40 * len(fam.targets) and all(2 <= n <= 10 for n in per_name.values())
    assert 0.20 <= st["absent"] / (st["absent"] + st["found"]) <= 0.30
    if fam.grammar == 3:
        assert st["installed_unparsable"] == 0
    else:
        assert 0.03 <= unp <= 0.15
    assert shares["less"] >= 0.25 and shares["greater"] + shares["equal"] >= 0.25 and shares["equal"] >= 0.02
    assert min(st["key<=16"], st["key17-32"], st["key>32"]) >= 100
    if fid == "alpine":
        assert st["tie16_tail"] >= 50 and st["tie16_spill"] >= 50
        assert st["decided_by_affected"] >= 100
    if fid == "redhat":
        assert st["rh_groups_text_differs"] >= 30


@pytest.mark.parametrize("grammar", [3, 2, 1])
def test_grammar_tie_classes(oracle_built, grammar):
    """Summed over a grammar's families: pairs that tie on 16 bytes (rpm), on 32, and in full."""
    tot = collections.Counter()
    for fid in oc.GRAMMAR_IDS[grammar]:
        tot.update(measure(fid)[0])
    print(f"\ngrammar {grammar}: ties 16 tail {tot['tie16_tail']}, 16 spill {tot['tie16_spill']}, 32 {tot['tie32']}, "
          f"equal keys from different text {tot['equal_keys_other_text']}")
    if grammar == 3:
        assert tot["tie16_tail"] >= 50 and tot["tie16_spill"] >= 50
    assert tot["tie32"] >= 20
    assert tot["equal_keys_other_text"] >= 20


def test_spill_tile_all_spill(oracle_built):
    """The every-package-spills tile: 256 installed keys over 32 bytes, most of them tying with a
    FixedVersion on the 16-byte head."""
    fam = oc.spill_tile()
    t = fam.targets[0]
    db = od.Records(fam.records)
    assert len(t.pkgs) == 256
    ties = 0
    for i, name, inst, _ in fam.batch_rows(t):
        ka = key(3, inst)
        assert len(ka) > 32, inst
        for a in db.get("alma 9", name):
            kb = key(3, a["FixedVersion"])
            ties += ka[:16] == kb[:16] and len(kb) > 16
    print(f"\nspill tile: {ties} pairs tie on the 16-byte head")
    assert ties >= 256
