"""Hand-built tables and packages for the two load-time row layouts (no GPU import here; the
host tests and the GPU tests share this data):

  ROW_INLINE      an rpm row whose arch / CPE / ksplice predicates fit the row itself
                  (csrc/common.h; built in DB::compile_rows, read by inline_pass);
  SLOT_CLS_SPLIT  a library key whose rows differ by version class keeps a class-0 list A in
                  front of its full list B (DB::split_by_class, read through slot_rows).

Every table declares the layout it must be flattened into (inline rows, split keys, class-0
duplicate rows), so a test that passes also says which layout it ran.
"""
import json

# ============================================================================ rpm predicates ==
RH_ARCHES = ["x86_64", "aarch64", "s390x", "ppc64le"]
RH_CPES = [10, 11, 12, 13]
# repository -> CPE indices ("Red Hat CPE" / "repository"); the defaults of RHEL 8 / 9 are the
# content sets the driver assumes for a package without BuildInfo (redhat.go:112-120)
RH_REPOS = {
    "repo-c10": [10], "repo-c11": [11], "repo-c12": [12], "repo-c13": [13], "repo-other": [20], "repo-empty": [],
    "repo-fffe": [0xFFFE], "repo-ffff": [0xFFFF], "repo-70000": [70000],
    "repo-4464": [70000 - 0x10000],  # 70000 cut to 16 bits: must not meet the 70000 key
    "rhel-8-for-x86_64-baseos-rpms": [10], "rhel-8-for-x86_64-appstream-rpms": [12],
    "rhel-9-for-x86_64-baseos-rpms": [11], "rhel-9-for-x86_64-appstream-rpms": [13],
}
RH_NVRS = {"ubi8-container-8.9-1-x86_64": [11]}
INLINE_IDS = 4  # csrc/common.h kInlineIds

# Red Hat shapes (n_arch, n_cpe): inline iff n_arch <= 3, n_cpe <= 3 and n_arch + n_cpe <= 4
RH_SHAPES = [(0, 1), (0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (0, 0), (0, 4), (3, 2), (4, 0), (4, 1)]
RH_SHAPES_INLINE = {(0, 1), (0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (0, 0)}
# a fixed version of more than 16 key bytes, and installed versions that tie it on the first 16
TIE_FIXED = ("1.2.3.4.5.6.7.8.9.10", "1.el8")
TIE_INSTALLED = ["1.2.3.4.5.6.7.8.9.9", "1.2.3.4.5.6.7.8.9.10", "1.2.3.4.5.6.7.8.9.11", "1.2.3.4.5.6.7.8.8.99"]


def _rec(path, val):
    return {"path": list(path), "value": val if isinstance(val, str) else json.dumps(val)}


def _rh_entry(na, nc, fixed, cve, cpes=None, status=0):
    e = {"FixedVersion": fixed, "Affected": list(RH_CPES[:nc] if cpes is None else cpes),
         "Cves": [{"ID": cve, "Severity": 2}] if cve else [{"Severity": 3}]}
    if na:
        e["Arches"] = RH_ARCHES[:na]
    if status:
        e["Status"] = status
    return e


class RpmCases:
    """records: fixture-format records of the three buckets.  keys: per key name a dict
    {bucket, inline: rows the key must carry inline, rows: its interval rows, shape, ...}.
    packages: per bucket the driver package dicts (ID "p<i>" = index in that list)."""

    def __init__(self):
        recs, keys = [], {}
        for root in ("Red Hat", "rocky 9", "Oracle Linux 8"):
            recs.append(_rec(("data-source", root), {"ID": root.split()[0].lower(), "Name": root, "URL": "https://x"}))
        for r, c in RH_REPOS.items():
            recs.append(_rec(("Red Hat CPE", "repository", r), c))
        for r, c in RH_NVRS.items():
            recs.append(_rec(("Red Hat CPE", "nvr", r), c))
        for i in sorted({c for cs in RH_REPOS.values() for c in cs}):
            recs.append(_rec(("Red Hat CPE", "cpe", str(i)), f"cpe:/o:redhat:test:{i}"))
        n = 0

        def rh(name, entries, vid=None, **info):
            nonlocal n
            n += 1
            recs.append(_rec(("Red Hat", name, vid or f"RHSA-2024:{1000 + n}"), {"Entries": entries}))
            k = keys.setdefault(name, {"bucket": "Red Hat", "inline": 0, "rows": 0, "fixed": ("2.0", "1.el8")})
            k.update(info)
            return k

        # one key per shape; a shape without CPE indices can match no package (redhat-oval Get
        # keeps an entry only if its Affected meets the package's CPEs), so those keys carry a
        # second advisory of shape (0, 1) under another CVE: the key has matches, the shape's own
        # CVE must never be reported
        for na, nc in RH_SHAPES:
            name = f"rh-a{na}-c{nc}"
            inl = (na, nc) in RH_SHAPES_INLINE
            k = rh(name, [_rh_entry(na, nc, "2.0-1.el8", f"CVE-2024-{100 + 10 * na + nc}")], shape=(na, nc),
                   cves={f"CVE-2024-{100 + 10 * na + nc}": (na, nc)})
            k["inline"] += int(inl)
            k["rows"] += 1
            if nc == 0:
                rh(name, [_rh_entry(0, 1, "2.0-1.el8", f"CVE-2024-{900 + na}")])
                k["cves"][f"CVE-2024-{900 + na}"] = (0, 1)
                k["never"] = f"CVE-2024-{100 + 10 * na + nc}"
                k["inline"] += 1
                k["rows"] += 1
        # CPE index edges: 0xFFFE is the largest id a row holds inline (0xFFFF marks a free field)
        for cpe, inl in ((0xFFFE, True), (0xFFFF, False), (70000, False)):
            name = f"rh-cpe-{cpe}"
            k = rh(name, [_rh_entry(0, 1, "2.0-1.el8", f"CVE-2024-{cpe}", cpes=[cpe])], shape=(0, 1),
                   cves={f"CVE-2024-{cpe}": (0, 1)}, cpe=cpe)
            k["inline"] += int(inl)
            k["rows"] += 1
        # unfixed, keyed by its CVE, with arches
        k = rh("rh-unfixed", [_rh_entry(2, 1, "", None, status=5)], vid="CVE-2024-5000", shape=(2, 1),
               cves={"CVE-2024-5000": (2, 1)}, fixed=None)
        k["inline"] += 1
        k["rows"] += 1
        # the 16-byte tie: an inline row reads its upper bound's offset from DB::row_off
        k = rh("rh-tie16", [_rh_entry(1, 1, "-".join(TIE_FIXED), "CVE-2024-1616")], shape=(1, 1),
               cves={"CVE-2024-1616": (1, 1)}, fixed=TIE_FIXED)
        k["inline"] += 1
        k["rows"] += 1

        # Rocky: arch entries (trivy-db rocky Get keeps an entry only if it lists the package's arch)
        def rocky(name, entries, inline, **info):
            nonlocal n
            n += 1
            recs.append(_rec(("rocky 9", name, f"CVE-2024-{2000 + n}"), {"Entries": entries}))
            keys[name] = dict({"bucket": "rocky 9", "inline": inline, "rows": len(entries), "fixed": ("2.0", "1.el9")},
                              **info)

        for na in (1, 3, 4):
            rocky(f"rk-a{na}", [{"FixedVersion": "2.0-1.el9", "Arches": RH_ARCHES[:na]}], int(na <= 3),
                  arches=RH_ARCHES[:na])
        rocky("rk-noarch", [{"FixedVersion": "2.0-1.el9", "Arches": ["noarch"]}], 1, arches=["noarch"])
        # an arch entry with an empty list matches no package; the advisory's second entry does
        rocky("rk-empty", [{"FixedVersion": "2.0-1.el9", "Arches": []},
                           {"FixedVersion": "2.0-1.el9", "Arches": ["aarch64"]}], 2, arches=["aarch64"])

        # Oracle: ksplice tags (oracle.go:65-69)
        def ol(name, fixed, **info):
            for j, f in enumerate(fixed):
                recs.append(_rec(("Oracle Linux 8", name, f"ELSA-2024-{3000 + 10 * len(keys) + j}"), {"FixedVersion": f}))
            keys[name] = dict({"bucket": "Oracle Linux 8", "inline": len(fixed), "rows": len(fixed)}, **info)

        ol("ol-tag", ["2.0-1.0.1.ksplice1.el8"], tags=["ksplice1"])
        ol("ol-plain", ["2.0-1.el8"], tags=[""])
        ol("ol-two", ["2.0-1.0.1.ksplice1.el8", "2.0-1.0.1.ksplice2.el8"], tags=["ksplice1", "ksplice2"])
        self.records, self.keys = recs, keys
        self.inline_rows = sum(k["inline"] for k in keys.values())
        self.interval_rows = sum(k["rows"] for k in keys.values())
        self.packages = {"Red Hat": self._rh_packages(), "rocky 9": self._rocky_packages(),
                         "Oracle Linux 8": self._ol_packages()}

    # ---- packages ----
    @staticmethod
    def _pkg(i, name, version, release, arch, **extra):
        p = {"ID": f"p{i}", "Name": name, "Version": version, "Release": release, "Epoch": 0, "SrcName": name,
             "SrcVersion": version, "SrcRelease": release, "SrcEpoch": 0}
        if arch is not None:
            p["Arch"] = arch
        p.update(extra)
        return p

    def _rh_packages(self):
        out = []
        arches = ["x86_64", "s390x", "ppc64le", "noarch", "riscv64", None]  # listed .. never named, none
        for name, k in self.keys.items():
            if k["bucket"] != "Red Hat":
                continue
            na, nc = k["shape"]
            if "cpe" in k:
                hit = [f"repo-{'%x' % k['cpe'] if k['cpe'] < 0x10000 else k['cpe']}"]
            else:
                hit = [f"repo-c{RH_CPES[max(nc, 1) - 1]}"]  # the key's last CPE index (the companion's for n_cpe 0)
            if k["fixed"] == TIE_FIXED:
                vers = [(v, TIE_FIXED[1]) for v in TIE_INSTALLED]
            else:
                vers = [("1.0", "1.el8"), ("2.0", "1.el8"), ("3.0", "1.el8")]

            def add(v, arch, cs, nvr="", rel=8, bi=True):
                extra = {"_rel": rel}
                if bi:
                    extra["BuildInfo"] = {"ContentSets": list(cs), "Nvr": nvr, "Arch": "x86_64"}
                out.append(self._pkg(len(out), name, v[0], v[1], arch, **extra))

            for v in vers:  # every version x every arch, with a CPE set that meets the key
                for a in arches:
                    add(v, a, hit)
            lo = vers[0]
            # the CPE side, below the fix on a listed arch: the first index, a set that holds the
            # hit among others, one that misses, the empty set, an unknown repository, the NVR map
            # alone, and the release defaults (no BuildInfo) of RHEL 8 and 9
            for cs, nvr in ((["repo-c10"], ""), (["repo-other", *hit], ""), (["repo-other"], ""), (["repo-empty"], ""),
                            (["repo-none"], ""), ([], "ubi8-container-8.9-1"), ([], "")):
                add(lo, "x86_64", cs, nvr)
            add(lo, "x86_64", None, rel=8, bi=False)
            add(lo, "aarch64", None, rel=9, bi=False)
            add(lo, "ppc64le", ["repo-other"])  # both predicates fail
            if "cpe" in k:  # the edge indices against each other, and 70000 cut to 16 bits
                for r in ("repo-fffe", "repo-ffff", "repo-70000", "repo-4464"):
                    add(lo, "x86_64", [r], rel=9)
        return out

    def _rocky_packages(self):
        out = []
        for name, k in self.keys.items():
            if k["bucket"] != "rocky 9":
                continue
            for v in ("1.0", "2.0", "3.0"):
                for a in ["x86_64", "aarch64", "s390x", "ppc64le", "noarch", "riscv64", None]:
                    out.append(self._pkg(len(out), name, v, "1.el9", a))
        return out

    def _ol_packages(self):
        out = []
        for name, k in self.keys.items():
            if k["bucket"] != "Oracle Linux 8":
                continue
            for v in ("1.0", "2.0", "3.0"):
                for rel in ("1.0.1.ksplice1.el8", "1.0.1.ksplice2.el8", "1.0.1.ksplice9.el8", "1.el8"):
                    out.append(self._pkg(len(out), name, v, rel, "x86_64"))
        return out


def rpm_version(p):
    """The batch API's version text of a package dict (utils.FormatVersion)."""
    v = f"{p['Version']}-{p['Release']}" if p.get("Release") else p["Version"]
    return f"{p['Epoch']}:{v}" if p.get("Epoch") else v


def rh_cpe_key(p):
    """(content sets, NVR text) of a Red Hat package as the driver resolves them."""
    bi = p.get("BuildInfo")
    if bi is None:
        r = p["_rel"]
        return (f"rhel-{r}-for-x86_64-baseos-rpms", f"rhel-{r}-for-x86_64-appstream-rpms"), ""
    return tuple(bi["ContentSets"]), f"{bi['Nvr']}-{bi['Arch']}"


# =========================================================================== version classes ==
PIP_SPECS = ["<2.0", ">1.0", "==1.0", "==1.0+abc", ">=1.0,<2.0", "!=1.5", "~=1.4", "<=2.0", ">=2.0rc1", "==1.*",
             "<2.0rc2", ">1.0.post1", "<1.0.post1", "==1.5.post1"]
NPM_SPECS = ["<2.0.0", ">=1.0.0 <2.0.0", "<2.0.0-rc.2", ">=1.5.0-alpha <1.5.0", "^1.0.0", "~1.5.0-0", "*",
             ">1.0.0-rc.1"]
PIP_SUFFIXES = ["", "+abc", "rc1", ".dev1", ".post1", "rc1+abc", ".post1+abc", "rc1.post1", "rc1.post1+abc",
                ".post1.dev2+x"]  # the 8 PEP 440 classes (bits local / pre / post), two of them twice
NPM_SUFFIXES = ["", "-rc.1", "-alpha", "-rc.3"]
# more than 32 key bytes with a pre-release: the spilled key carries its class
PIP_LONG = "1.2.3.4.5.6.7.8.9.10.11.12.13.14.15.16.17.18.19.20rc1"
UNPARSABLE = {"pip": "not-a-version", "npm": "1.0"}
MAVEN_ROOT, MAVEN_PKG = "maven::GitHub Security Advisory Maven", {"Name": "org.example:lib", "Version": "1.0"}


# A pre-release below 2.0 that "<2.0" does not hold (PEP 440 keeps 2.0's own pre-releases out of
# "<2.0"; an npm pre-release needs a comparator with a pre-release of its own version): the
# Patched set removes every other class, so the key's rows admit no plain release version
ONLY_PRE = {"pip": {"VulnerableVersions": ["<2.0rc2"], "PatchedVersions": ["<2.0"]},
            "npm": {"VulnerableVersions": ["<2.0.0-rc.2"], "PatchedVersions": ["<2.0.0"]}}

# Per constraint: (interval rows, those that admit class 0, a plain release version).
# PEP 440 (classes = bits local 1 / pre 2 / post 4).  A specifier is one key-order interval for
# every class unless one of its exclusion rules applies to some classes only: "<V" with V no
# pre-release leaves V's own pre-releases out (the "pre" classes stop earlier), ">V" leaves V's
# post-releases and local versions out (the "post" / "local" classes start later).  Those are
# two rows, one of them for class 0; "!=1.5" is the two intervals around 1.5 and its local
# versions, for every class alike; "==1.0+abc" is one point no other class has a key at.
PIP_ROWS = {"<2.0": (2, 1), ">1.0": (2, 1), "==1.0": (1, 1), "==1.0+abc": (1, 1), ">=1.0,<2.0": (2, 1),
            "!=1.5": (2, 2), "~=1.4": (1, 1), "<=2.0": (1, 1), ">=2.0rc1": (1, 1), "==1.*": (1, 1),
            "<2.0rc2": (1, 1), ">1.0.post1": (2, 1), "<1.0.post1": (2, 1), "==1.5.post1": (1, 1),
            ">=1.0": (1, 1), ">=2.0": (1, 1), "only-pre": (1, 0)}
# npm (class 1 = pre-release): a pre-release matches only a comparator set that names a
# pre-release of its own [major, minor, patch].  A set without one is a single row for class 0;
# one with a pre-release bound adds the class-1 row inside that version's pre-releases
# ("~1.5.0-0": two of them, 1.5.0's pre-releases and nothing else below 1.6.0-0), unless both
# classes get the same interval (">=1.5.0-alpha <1.5.0").
NPM_ROWS = {"<2.0.0": (1, 1), ">=1.0.0 <2.0.0": (1, 1), "<2.0.0-rc.2": (2, 1), ">=1.5.0-alpha <1.5.0": (1, 1),
            "^1.0.0": (2, 1), "~1.5.0-0": (3, 1), "*": (1, 1), ">1.0.0-rc.1": (2, 1), "only-pre": (1, 0)}


class ClassCases:
    """One ecosystem's keys: specs[key] = the advisories, each a VulnerableVersions text or
    "only-pre" (ONLY_PRE).  layout[key] = (|A|, |B|): the rows that admit class 0 and every row;
    a key is split iff |A| < |B|."""

    def __init__(self, eco):
        self.eco = eco
        self.lang = {"pip": "pip", "npm": "npm"}[eco]
        self.grammar = {"pip": 6, "npm": 5}[eco]
        self.root = {"pip": "pip::GitHub Security Advisory pip", "npm": "npm::GitHub Security Advisory npm"}[eco]
        if eco == "pip":
            self.specs = {"cls-all0": [">=1.0", ">=2.0"], "cls-mixed": ["<2.0", "!=1.5", "==1.0+abc"],
                          "cls-nonzero": ["only-pre"], "cls-local-point": ["==1.0+abc"], "cls-all": PIP_SPECS}
            self.versions = [b + s for b in ("1.0", "1.5", "2.0") for s in PIP_SUFFIXES] + [PIP_LONG]
            rows = PIP_ROWS
        else:
            self.specs = {"cls-all0": ["<2.0.0", "*"], "cls-mixed": ["<2.0.0", "<2.0.0-rc.2"],
                          "cls-nonzero": ["only-pre"], "cls-all": NPM_SPECS}
            self.versions = [b + s for b in ("1.0.0", "1.5.0", "2.0.0") for s in NPM_SUFFIXES]
            rows = NPM_ROWS
        self.versions.append(UNPARSABLE[eco])
        self.layout = {k: (sum(rows[s][1] for s in sp), sum(rows[s][0] for s in sp)) for k, sp in self.specs.items()}
        self.split = {k: a < b for k, (a, b) in self.layout.items()}
        self.records = [_rec(("data-source", self.root), {"ID": "ghsa", "Name": self.root, "URL": "https://g"}),
                        _rec(("data-source", MAVEN_ROOT), {"ID": "ghsa", "Name": MAVEN_ROOT, "URL": "https://g"}),
                        _rec((MAVEN_ROOT, MAVEN_PKG["Name"], "CVE-2024-7000"), {"VulnerableVersions": ["<2.0"]})]
        for key, specs in self.specs.items():
            for j, s in enumerate(specs):
                adv = ONLY_PRE[eco] if s == "only-pre" else {"VulnerableVersions": [s]}
                self.records.append(_rec((self.root, key, f"CVE-2024-{4000 + j}"), adv))
        # classes interleaved: version-major order, so neighbouring lanes differ in key and class
        self.packages = [{"ID": f"p{i}", "Name": key, "Version": v}
                         for i, (v, key) in enumerate((v, key) for v in self.versions for key in self.specs)]
        self.split_keys = sum(self.split.values())
        self.class0_dup_rows = sum(a for k, (a, b) in self.layout.items() if self.split[k])
        self.interval_rows = sum(b for a, b in self.layout.values()) + 1  # + the Maven key's row


def big_key_records(n_adv, mixed=False, name="big"):
    """One pip key of n_adv advisories "<i.0" (2 rows each: the classes with and without
    "pre"), or alternating "==i.0+li" (1 row) and "<i.0"; returns (records, interval rows)."""
    root = "pip::GitHub Security Advisory pip"
    recs, rows = [_rec(("data-source", root), {"ID": "ghsa", "Name": root, "URL": "https://g"})], 0
    for i in range(n_adv):
        eq = mixed and i % 2 == 0
        recs.append(_rec((root, name, f"CVE-2024-{i:05d}"), '{"VulnerableVersions": ["%s"]}' %
                         (f"=={i}.0+l{i}" if eq else f"<{i}.0")))
        rows += 1 if eq else 2
    return recs, rows
