"""Adversarial versions for the OS-package grammars other than Debian / Ubuntu (no GPU import
here; the host test and the GPU tests share this data): rpm (alma, rocky, Oracle Linux, Photon,
CBL-Mariner, SLES, openSUSE Leap, Red Hat), apk (Alpine, Wolfi, Chainguard) and the dpkg grammar
as Amazon Linux runs it.

Every family is a small advisory table (fixture-format records, as row_layout_cases._rec makes
them) and about 1300 packages.  Per package name one base version is drawn; every FixedVersion
and every installed version of that name is a neighbour of the base - a few mutations (rpm,
dpkg) or one or two perturbed parts of the parse (apk) - so both sides of a comparison share
long prefixes: their sort keys tie on the 16-byte head the sweep compares first, on the 32
bytes a package keeps beside its head, and now and then in full.  What the inputs reach is
measured by tests/test_os_versions_host.py from the oracle and the host encoder alone.

Everything is seeded: the same tables and packages on every run.
"""
import functools
import json
import random

import row_layout_cases as rc
from row_layout_cases import _rec
from test_verkey_host import RPM_ATOMS, _gen

# ====================================================================================== rpm ==
RPM_BASES = [
    "7.29.0-59.0.1.el7_9.1", "3.10.0-1160.102.1.el7", "2.4.37-43.module_el8.5.0+1022+b541f3b1", "1.1.1k-9.el8_7",
    "4.18.0-477.27.1.0.1.el8_8", "1.2.3.4.5.6.7.8.9.10-1.el8", "1.0~rc1-1.el9", "1.0^20230101git-1.el9",
    "0.9.8e-12.el5_4.6", "2.28-151.0.1.ksplice1.el8", "2.9-3", "1.4-2.el8", "0.52-1", "12-4.el9", "3.6.8-5.el8",
    "2.02-142.el8_9.1", "20230101-1.el9", "5.15.0-101.103.2.1.el8uek", "1.8.0.382.b05-2.el8", "8.2p1-3",
]
RPM_SHORT = ["2.9-3", "1.4-2", "0.52-1", "12-4", "3.6", "1.4", "9", "2.0"]
RPM_KSPLICE = ["2.28-151.0.1.ksplice1.el8", "1.1.1k-9.ksplice1.el8_7", "7.61.1-30.0.2.ksplice1.el8_8.3",
               "2.28-151.0.1.ksplice2.el8", "3.6.8-5.el8", "2.9-3"]
EPOCHS = ["1:", "0:", "2:", "+2:", "-1:", "a:", ":", "99999999999999999999:"]
_ATOMS = [a.decode() for a in RPM_ATOMS]


def mutate(rng, base, atoms=_ATOMS, epochs=EPOCHS, p_epoch=0.10, tail_bias=0.6):
    """0-3 mutations of base: an atom inserted or appended, 1-3 characters deleted, one digit
    bumped; then an epoch prefix on about p_epoch of the strings.  Positions lean to the tail
    (tail_bias), so that many neighbours keep a long common prefix with the base."""
    s = base

    def pos(n):
        if n <= 0:
            return 0
        return rng.randint(n // 2, n) if rng.random() < tail_bias else rng.randint(0, n)

    for _ in range(rng.choice([0, 1, 1, 2, 2, 3])):
        k = rng.random()
        if k < 0.35:
            i = pos(len(s)) if rng.random() < 0.7 else len(s)
            s = s[:i] + rng.choice(atoms) + s[i:]
        elif k < 0.60 and len(s) > 1:
            i = pos(len(s) - 1)
            s = s[:i] + s[i + rng.randint(1, 3):]
        else:
            at = [i for i, c in enumerate(s) if c.isdigit()]
            if at:
                i = at[min(len(at) - 1, pos(len(at) - 1))] if rng.random() < tail_bias else rng.choice(at)
                s = s[:i] + str((int(s[i]) + rng.choice([1, 1, 9, 5])) % 10) + s[i + 1:]
    if rng.random() < p_epoch:
        s = rng.choice(epochs) + s
    return s


def split_evr(text):
    """(Version, Release) of a package dict whose FormatVersion is `text`: split at the first
    '-' (where the batch path takes an Oracle package's release from); a text that would not
    print back the same keeps everything in Version."""
    i = text.find("-")
    if i < 0 or i + 1 == len(text):
        return text, ""
    return text[:i], text[i + 1:]


# ====================================================================================== apk ==
APK_SUFFIXES = ["_alpha", "_beta", "_pre", "_rc", "_cvs", "_svn", "_git", "_hg", "_p"]
APK_FOREIGN = ["A", "~", "-", "_x", "..", "-r", "_", " "]


def apk_parts(rng, size):
    """A parse of the apk grammar: numeric components (as text, leading zeros kept), an optional
    letter, 0-3 suffixes with optional numbers, an optional revision.  size 0 / 1 / 2: short,
    medium, long."""
    n = {0: rng.randint(1, 2), 1: rng.randint(2, 4), 2: rng.randint(5, 12)}[size]
    nums = [str(rng.choice([0, 1, 2, 3, 9, 10, 12, 20230101] if size else [0, 1, 2, 9]))
            for _ in range(n)]
    letter = rng.choice("abz") if rng.random() < 0.25 else ""
    suf = [(rng.choice(APK_SUFFIXES), rng.choice(["", "1", "2", "10"]))
           for _ in range(rng.choice([0, 0, 0, 1] if size == 0 else [0, 1, 1, 2, 3] if size == 2 else [0, 0, 1, 2]))]
    rev = rng.choice(["", "0", "1", "2", "10"]) if size else rng.choice(["", "", "0", "1"])
    return {"nums": nums, "letter": letter, "suf": suf, "rev": rev}


def apk_render(p):
    s = ".".join(p["nums"]) + p["letter"] + "".join(a + b for a, b in p["suf"])
    return s + ("-r" + p["rev"] if p["rev"] != "" else "")


def _num_neighbour(rng, t):
    k = rng.random()
    if k < 0.3:
        return str(int(t) + 1)
    if k < 0.5:
        return str(max(int(t) - 1, 0))
    if k < 0.75:
        return "0" * rng.randint(1, 2) + t  # leading zeros
    if k < 0.85:
        return t + "0"
    return t.lstrip("0") or "0"


def apk_neighbour(rng, base, tail_bias=0.7):
    """base with one or two parts perturbed, and on about 12 % of the strings one foreign token."""
    p = {"nums": list(base["nums"]), "letter": base["letter"], "suf": list(base["suf"]), "rev": base["rev"]}
    for _ in range(rng.choice([0, 1, 1, 1, 2, 2])):
        k = rng.random()
        if k < 0.30:
            n = len(p["nums"])
            i = rng.randint(n // 2, n - 1) if rng.random() < tail_bias else rng.randint(0, n - 1)
            p["nums"][i] = _num_neighbour(rng, p["nums"][i])
        elif k < 0.40:
            if len(p["nums"]) > 1 and rng.random() < 0.5:
                p["nums"].pop()
            else:
                p["nums"].append(rng.choice(["0", "1", "00", "01"]))
        elif k < 0.50:
            p["letter"] = rng.choice(["", "a", "b", "z"])
        elif k < 0.75:
            if p["suf"] and rng.random() < 0.7:
                i = rng.randint(0, len(p["suf"]) - 1)
                a, b = p["suf"][i]
                if rng.random() < 0.5:
                    p["suf"][i] = (a, rng.choice(["", "0", "1", "01", "2", "10"]))
                elif rng.random() < 0.5:
                    p["suf"][i] = (rng.choice(APK_SUFFIXES), b)
                else:
                    p["suf"].pop(i)
            elif len(p["suf"]) < 3:
                p["suf"].append((rng.choice(APK_SUFFIXES), rng.choice(["", "1", "2"])))
        else:
            p["rev"] = rng.choice(["", "0", "00", "1", "01", "2", "10", "11"])
    s = apk_render(p)
    if rng.random() < 0.12:
        i = rng.randint(0, len(s))
        s = s[:i] + rng.choice(APK_FOREIGN) + s[i:]
    return s


# ===================================================================================== dpkg ==
AMZN_BASES = ["1.2.3-4.amzn2", "2.17.1-1.amzn2.0.1", "1:1.8.0.382.b05-1.amzn2.0.1.rc", "4.14.336-257.562.amzn2",
              "2.26-64.amzn2.0.2", "1.0-1", "3.4", "7", "2.06-14.amzn2.0.9", "6.1.66-93.164.amzn2023",
              "2.02~beta2+dfsg1-14.amzn2.0.9", "1.1.1g-12.amzn2.0.20", "20230101.git1a2b3c4-7.amzn2023.0.2",
              "1.2-3", "5.10.210+git20240101.1a2b3c-201.852.amzn2"]
_DEB_ATOMS = ["0", "1", "2", "9", "00", "10", ".", "-", "+", "~", "a", "z", "A", "amzn2", "rc", "0", "1", ".", "+",
              " ", "!"]


def amzn_version(rng, base):
    if base is None:
        return _gen(rng).decode("utf-8", "replace")
    return mutate(rng, base, atoms=_DEB_ATOMS, epochs=["1:", "0:", "2:", "1:", "0:", "-1:", "+2:", ":", "a:", "-0:"],
                  p_epoch=0.08)


# ================================================================================== families ==
N_NAMES, N_PKGS, ABSENT = 40, 1300, 0.25
ARCHES = ["x86_64", "aarch64", "noarch", "i686"]


class Target:
    """One Detect call: the driver family, its OS version and repository, the bucket the batch
    path adds its packages under, and the driver package dicts (ID "p<i>" = index in pkgs)."""

    def __init__(self, family, os_ver, repo, bucket):
        self.family, self.os_ver, self.repo, self.bucket, self.pkgs = family, os_ver, repo, bucket, []


class Family:
    """records: fixture-format records.  targets: the Detect calls (Alpine has two streams, the
    others one).  grammar: tvm_version_key's grammar id (1 dpkg, 2 apk, 3 rpm)."""

    def __init__(self, fid, grammar, kind):
        self.id, self.grammar, self.kind = fid, grammar, kind
        self.records, self.targets = [], []

    # ---- what the batch path is given: the driver's lookup name and compare version -------------
    def batch_rows(self, t):
        """[(index in t.pkgs, lookup name, version text, arch or None)] of the packages the driver
        does not skip before its lookup (alma: a modular release without a label)."""
        out = []
        for i, p in enumerate(t.pkgs):
            if self.kind == "alma" and ".module_el" in p.get("Release", "") and not p.get("Modularitylabel"):
                continue
            name = p["Name"]
            if self.kind in ("alma", "redhat"):
                name = _modular(p["Name"], p.get("Modularitylabel", ""))
            elif self.kind in ("photon", "mariner"):
                name = p["SrcName"]
            elif self.kind in ("alpine", "wolfi", "chainguard"):
                name = p.get("SrcName") or p["Name"]
            src = self.kind in ("mariner", "alpine")
            ver = _fmt(p["SrcEpoch"], p["SrcVersion"], p["SrcRelease"]) if src else _fmt(p["Epoch"], p["Version"], p["Release"])
            out.append((i, name, ver, p.get("Arch")))
        return out


def _fmt(epoch, version, release):
    v = f"{version}-{release}" if release else version
    return f"{epoch}:{v}" if epoch else v


def _modular(name, label):
    parts = label.split(":")
    return name if len(parts) < 3 else f"{parts[0]}:{parts[1]}::{name}"


def _pkg(i, name, text, arch=None, src_name=None, **extra):
    v, r = split_evr(text)
    p = {"ID": f"p{i}", "Name": name, "Version": v, "Release": r, "Epoch": 0, "SrcName": src_name or name,
         "SrcVersion": v, "SrcRelease": r, "SrcEpoch": 0}
    if arch is not None:
        p["Arch"] = arch
    p.update(extra)
    return p


def _source(fam, root):
    fam.records.append(_rec(("data-source", root), {"ID": root.split()[0].lower(), "Name": root, "URL": "https://x"}))


def _names(rng, prefix):
    return [f"{prefix}-{i:02d}" for i in range(N_NAMES)]


def _pick_names(rng, names, n):
    """n package names: a quarter absent from the table."""
    return [f"absent-{rng.randint(0, 99)}" if rng.random() < ABSENT else rng.choice(names) for _ in range(n)]


# ---- rpm families ---------------------------------------------------------------------------------
RPM_FAMILIES = {
    # id: (driver family, OS version, bucket root, kind)
    "alma": ("alma", "9.3", "alma 9", "alma"),
    "rocky": ("rocky", "9.3", "rocky 9", "rocky"),
    "oracle": ("oracle", "8.9", "Oracle Linux 8", "oracle"),
    "photon": ("photon", "4.0", "Photon OS 4.0", "photon"),
    "mariner": ("cbl-mariner", "2.0.20240101", "CBL-Mariner 2.0", "mariner"),
    "sles": ("suse linux enterprise server", "15.5", "SUSE Linux Enterprise 15.5", "suse"),
    "opensuse": ("opensuse.leap", "15.5", "openSUSE Leap 15.5", "suse"),
}


def _rpm_family(fid, seed):
    family, os_ver, root, kind = RPM_FAMILIES[fid]
    rng = random.Random(seed)
    fam = Family(fid, 3, kind)
    _source(fam, root)
    t = Target(family, os_ver, None, root)
    names = _names(rng, fid)
    bases, labels = {}, {}
    n_adv = 0
    for j, name in enumerate(names):
        pool = RPM_KSPLICE if kind == "oracle" else RPM_SHORT if j % 4 == 3 else RPM_BASES
        bases[name] = rng.choice(pool)
        key = name
        if kind == "alma" and j % 5 == 0:  # a modular key: "module:stream::name"
            labels[name] = f"mod{j}:1.{j}:8090020231201:{j:08x}"
            key = _modular(name, labels[name])
        for _ in range(rng.randint(2, 6)):
            n_adv += 1
            vid = f"CVE-2024-{10000 + n_adv}"
            fixed = mutate(rng, bases[name])
            if kind == "rocky":
                ents = [{"FixedVersion": fixed, "Arches": rng.sample(ARCHES, rng.randint(1, 3))}]
                if rng.random() < 0.5:
                    ents.append({"FixedVersion": mutate(rng, bases[name]), "Arches": rng.sample(ARCHES, rng.randint(1, 2))})
                val = {"Entries": ents}
            elif kind == "mariner" and rng.random() < 0.15:
                val = {}  # unfixed: reported whatever the installed version
            else:
                val = {"FixedVersion": fixed}
            fam.records.append(_rec((root, key, vid), val))
    for i, name in enumerate(_pick_names(rng, names, N_PKGS)):
        text = mutate(rng, bases.get(name) or rng.choice(RPM_BASES))
        extra = {}
        if name in labels and rng.random() < 0.9:
            extra["Modularitylabel"] = labels[name]
        src = name
        if kind in ("photon", "mariner"):  # these drivers look the source name up
            src, name = name, name + "-libs"
        t.pkgs.append(_pkg(i, name, text, rng.choice(ARCHES), src_name=src, **extra))
    fam.targets.append(t)
    return fam


# (FixedVersions of one CVE whose greatest differs between text order and rpm order, a version below all)
RH_ORDER = [(["1.10-1.el8", "1.9-1.el8"], "1.8-1.el8"), (["1.0~rc1-1.el8", "1.0-1.el8"], "0.9-1.el8"),
            (["1:0.9-1.el8", "2.0-1.el8"], "0.5-1.el8"), (["0:3.0-1.el8", "10.0-1.el8", "9.0-1.el8"], "2.0-1.el8")]


def _redhat_family(seed):
    """Red Hat 8 with the CPE plumbing of row_layout_cases: two to four advisories per CVE and
    package name, so that the merge has a greatest FixedVersion to pick in rpm order."""
    rng = random.Random(seed)
    fam = Family("redhat", 3, "redhat")
    _source(fam, "Red Hat")
    for r, c in rc.RH_REPOS.items():
        fam.records.append(_rec(("Red Hat CPE", "repository", r), c))
    for r, c in rc.RH_NVRS.items():
        fam.records.append(_rec(("Red Hat CPE", "nvr", r), c))
    for i in sorted({c for cs in rc.RH_REPOS.values() for c in cs}):
        fam.records.append(_rec(("Red Hat CPE", "cpe", str(i)), f"cpe:/o:redhat:test:{i}"))
    t = Target("redhat", "8.9", None, "Red Hat")
    names = _names(rng, "redhat")
    bases, n_adv = {}, 0
    for j, name in enumerate(names):
        order = RH_ORDER[j // 2 % len(RH_ORDER)] if j % 2 == 0 and j < 16 else None
        bases[name] = order[1] if order else rng.choice(RPM_SHORT if j % 4 == 3 else RPM_BASES)
        for c in range(rng.randint(1, 2)):
            cve = f"CVE-2024-{20000 + 10 * j + c}"
            fixes = list(order[0]) if order and c == 0 else []
            fixes += [mutate(rng, bases[name]) for _ in range(rng.randint(2, 4) - len(fixes))]
            rng.shuffle(fixes)
            for fixed in fixes:
                n_adv += 1
                e = {"FixedVersion": fixed, "Affected": rng.choice([[10], [12], [10, 12], [10, 11, 12, 13], [11]]),
                     "Cves": [{"ID": cve, "Severity": rng.randint(1, 4)}]}
                if rng.random() < 0.3:
                    e["Arches"] = rng.sample(ARCHES, rng.randint(1, 3))
                fam.records.append(_rec(("Red Hat", name, f"RHSA-2024:{1000 + n_adv}"), {"Entries": [e]}))
        if j % 7 == 0:  # an unfixed entry keyed by its CVE
            fam.records.append(_rec(("Red Hat", name, f"CVE-2024-{29000 + j}"),
                                    {"Entries": [{"FixedVersion": "", "Affected": [10, 12], "Status": 5,
                                                  "Cves": [{"Severity": 2}]}]}))
    sets = [(["repo-c10"], ""), (["repo-c12"], ""), (["repo-other", "repo-c10"], ""), None, None, (["repo-other"], "")]
    for i, name in enumerate(_pick_names(rng, names, N_PKGS)):
        text = mutate(rng, bases.get(name) or rng.choice(RPM_BASES), p_epoch=0.05)
        extra = {"_rel": 8}
        cs = rng.choice(sets)
        if cs is not None:
            extra["BuildInfo"] = {"ContentSets": list(cs[0]), "Nvr": cs[1], "Arch": "x86_64"}
        t.pkgs.append(_pkg(i, name, text, rng.choice(ARCHES), **extra))
    fam.targets.append(t)
    return fam


# ---- apk families ---------------------------------------------------------------------------------
def _apk_table(rng, fam, root, names, alpine):
    bases = {}
    n_adv = 0
    for j, name in enumerate(names):
        bases[name] = apk_parts(rng, j % 3)
        for _ in range(rng.randint(2, 6)):
            n_adv += 1
            val = {"FixedVersion": apk_neighbour(rng, bases[name])}
            if alpine:
                k = rng.random()
                if k < 0.05:
                    val["FixedVersion"] = "0"  # secdb's "not affected" (below every installed version)
                elif k < 0.10:
                    val["FixedVersion"] = ""
                if rng.random() < 1 / 3:
                    val["AffectedVersion"] = apk_neighbour(rng, bases[name])
            fam.records.append(_rec((root, name, f"CVE-2024-{30000 + n_adv}"), val))
    return bases


def _apk_pkgs(rng, t, names, bases, n):
    for name in _pick_names(rng, names, n):
        base = bases.get(name) or apk_parts(rng, rng.randint(0, 2))
        # Alpine and the stream drivers look the origin (SrcName) up and fall back to the name
        t.pkgs.append(_pkg(len(t.pkgs), name + "-doc", apk_neighbour(rng, base), src_name=name))


def _alpine_family(seed):
    """Two streams: "alpine 3.19" from the OS version, "alpine 3.18" from a repository release
    that differs from it (alpine.go:71-79)."""
    rng = random.Random(seed)
    fam = Family("alpine", 2, "alpine")
    for root, repo, n in (("alpine 3.19", None, N_PKGS - 500), ("alpine 3.18", {"Family": "alpine", "Release": "3.18"}, 500)):
        _source(fam, root)
        names = _names(rng, "apk" + root[-2:])
        bases = _apk_table(rng, fam, root, names, True)
        t = Target("alpine", "3.19.1", repo, root)
        _apk_pkgs(rng, t, names, bases, n)
        fam.targets.append(t)
    return fam


def _stream_family(fid, seed):
    rng = random.Random(seed)
    fam = Family(fid, 2, fid)
    _source(fam, fid)
    names = _names(rng, fid)
    bases = _apk_table(rng, fam, fid, names, False)
    t = Target(fid, "20230201", None, fid)
    _apk_pkgs(rng, t, names, bases, N_PKGS)
    fam.targets.append(t)
    return fam


# ---- Amazon Linux ---------------------------------------------------------------------------------
def _amazon_family(fid, seed):
    rel = fid.split("-")[1]
    rng = random.Random(seed)
    fam = Family(fid, 1, "amazon")
    root = "amazon linux " + rel
    _source(fam, root)
    t = Target("amazon", rel + " (Karoo)" if rel == "2" else rel, None, root)
    names = _names(rng, fid)
    bases, n_adv = {}, 0
    for j, name in enumerate(names):
        bases[name] = None if j % 10 == 0 else AMZN_BASES[(j + rng.randint(0, 2)) % len(AMZN_BASES)]  # None: test_verkey_host._gen strings
        for _ in range(rng.randint(2, 6)):
            n_adv += 1
            fam.records.append(_rec((root, name, f"ALAS{rel}-2024-{n_adv}"), {"FixedVersion": amzn_version(rng, bases[name])}))
    for i, name in enumerate(_pick_names(rng, names, N_PKGS)):
        base = bases[name] if name in bases else rng.choice(AMZN_BASES)
        t.pkgs.append(_pkg(i, name, amzn_version(rng, base) or "1", rng.choice(ARCHES)))
    fam.targets.append(t)
    return fam


SEEDS = {"alma": 101, "rocky": 102, "oracle": 103, "photon": 104, "mariner": 105, "sles": 106, "opensuse": 107,
         "redhat": 108, "alpine": 201, "wolfi": 202, "chainguard": 203, "amazon-2": 301, "amazon-2023": 303}
RPM_IDS = ["alma", "rocky", "oracle", "photon", "mariner", "sles", "opensuse", "redhat"]
APK_IDS = ["alpine", "wolfi", "chainguard"]
DEB_IDS = ["amazon-2", "amazon-2023"]
FAMILY_IDS = RPM_IDS + APK_IDS + DEB_IDS
GRAMMAR_IDS = {3: RPM_IDS, 2: APK_IDS, 1: DEB_IDS}


@functools.lru_cache(maxsize=None)
def family(fid):
    if fid == "redhat":
        return _redhat_family(SEEDS[fid])
    if fid in RPM_FAMILIES:
        return _rpm_family(fid, SEEDS[fid])
    if fid == "alpine":
        return _alpine_family(SEEDS[fid])
    if fid in ("wolfi", "chainguard"):
        return _stream_family(fid, SEEDS[fid])
    return _amazon_family(fid, SEEDS[fid])


def all_records():
    """Every family's table in one record list (the buckets are disjoint), data sources once."""
    out, seen = [], set()
    for fid in FAMILY_IDS:
        for r in family(fid).records:
            k = json.dumps(r["path"])
            if k not in seen:
                seen.add(k)
                out.append(r)
    return out


# ============================================================================ every key spills ==
def spill_tile():
    """(records, packages) of one tile of 256 alma packages whose keys all pass 32 bytes, against
    FixedVersions that tie with them on the 16-byte head."""
    rng = random.Random(404)
    fam = Family("alma-spill", 3, "alma")
    _source(fam, "alma 9")
    t = Target("alma", "9.3", None, "alma 9")
    long_bases = [b for b in RPM_BASES if len(b) >= 24 and "module" not in b]
    names = [f"spill-{i}" for i in range(8)]
    no_colon = [a for a in _ATOMS if a != ":"]  # an inserted ':' would turn the head into an epoch
    bases = {}
    for j, name in enumerate(names):
        bases[name] = long_bases[j % len(long_bases)]
        for k in range(4):
            fam.records.append(_rec(("alma 9", name, f"CVE-2024-{40000 + 10 * j + k}"),
                                    {"FixedVersion": mutate(rng, bases[name], atoms=no_colon, p_epoch=0, tail_bias=1.0)}))
    for i in range(256):
        name = names[i % len(names)]
        t.pkgs.append(_pkg(i, name, mutate(rng, bases[name], atoms=no_colon, p_epoch=0, tail_bias=1.0) + ".0.1.2.3", "x86_64"))
    fam.targets.append(t)
    return fam
