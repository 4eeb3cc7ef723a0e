"""Shared by the tests of the Red Hat merge inside the pipelined pass (TVM_PIPE_RH_MERGE,
rhmerge.hip): the oracle's view of a batch as the merged, filtered pass must return it.

Everything here comes from the oracle: oracle.drivers.driver_detect per target (Red Hat per
release), oracle.vulninfo.fill_info, pipe_filter_cases.keep_mask (filter.go:113-120 per finding;
the pass does not dedup).  Chain holds that output entry by entry; rh_groups re-derives, from
trivy-db's Get order, the members of every Red Hat entry (first member, representative), which
the tests use to show from the oracle's numbers alone that a case exercises what it claims, and
which tests/test_pipeline_rhmerge_host.py pins against driver_detect.

World C is a hand-built Red Hat DB: one name whose list holds a group of 151 members starting
at position 63 (it straddles a 64-entry round), a second name with three CVEs of two members."""
import collections
import json

import numpy as np

import oracle.drivers as od
import oracle.vulninfo as vi
import pipe_filter_cases as pc
import vulnset_ref as vr
from tools import synth_mix as sm

MASKS = [dict(severities=("HIGH", "CRITICAL"), ignore_statuses=(5, 7)), dict(severities=("LOW",))]
STATUS_FIXED = 3


def with_ids(pkgs, base):
    """Every field a driver copies is set, so the records' copy flags show (as the stub package
    of oracle.drivers.advisory_record has them)."""
    for k, pk in enumerate(pkgs):
        pk["ID"] = f"p{base + k}"
        pk["Identifier"] = {"PURL": f"pkg:x/{base + k}"}
        pk["Layer"] = {"DiffID": f"sha256:{base + k:08x}"}
    return pkgs


def _flat(v):
    """The drivers' dicts carry the embedded Vulnerability.Severity flattened (its JSON form)."""
    return dict({k: x for k, x in v.items() if k != "Severity"},
                **({"Vulnerability": {"Severity": v["Severity"]}} if "Severity" in v else {}))


class Target:
    """One result's packages: batch indices [first, first + len(pkgs)), PkgID "p<batch index>"."""

    def __init__(self, first, kind, pkgs, detect, rels=None):
        self.first, self.kind, self.pkgs, self.detect, self.rels = first, kind, pkgs, detect, rels


def mix_targets(sdb, batch):
    """The targets of a tools/synth_mix.py batch (one per platform group; Red Hat detected per
    release, as tests/test_gpu_redhat_chain.py does) and the records they read."""
    names = collections.defaultdict(set)
    for p, g in batch.groups:
        names[sdb.plats[p][0]] |= {x.decode() for x in g["name"]}
    names["Red Hat CPE"] = {"repository", "nvr", "cpe"}
    recs = od.Records(sdb.records_for(names))
    out, first = [], 0
    for p, g in batch.groups:
        bucket, kind = sdb.plats[p]
        pkgs = with_ids(sm.driver_packages(sdb, p, g, np.arange(len(g["key"]))), first)
        if kind == "redhat":
            out.append(Target(first, kind, pkgs, None, [int(r) for r in g["rhrel"]]))
        else:
            fam, fmt = sm.DRIVER_OF[kind]
            out.append(Target(first, kind, pkgs, (fam, fmt.format(bucket.split(" ")[-1]))))
        first += len(pkgs)
    return out, recs


def detect(t, recs):
    """Driver.Detect's output for target t, package by package in the driver's order."""
    if t.kind != "redhat":
        return od.driver_detect(t.detect[0], t.detect[1], None, t.pkgs, recs, None)
    vulns = []
    for rel in sorted(set(t.rels)):
        vulns += od.driver_detect("redhat", str(rel), None, [pk for pk, r in zip(t.pkgs, t.rels) if r == rel], recs, None)
    vulns.sort(key=lambda v: int(v["PkgID"][1:]))  # stable: each package's list stays in ID order
    return vulns


class Chain:
    """driver_detect -> fill_info per target: per entry its package, its record key (the
    detection's own fields, as tvm_vuln_set records hold them) and its filled form."""

    def __init__(self, targets, recs, bucket):
        self.pkg, self.det, self.filled, self.kind = [], [], [], []
        for t in targets:
            vulns = detect(t, recs)
            self.det += vulns
            self.filled += vi.fill_info(bucket, [_flat(v) for v in vulns])
            self.pkg += [int(v["PkgID"][1:]) for v in vulns]
            self.kind += [t.kind] * len(vulns)
        self.pkg = np.array(self.pkg, dtype=np.int64)

    def rec_ids(self, keys):
        memo = {}
        out = np.zeros(len(self.det), dtype=np.int64)
        for i, v in enumerate(self.det):
            k = vr.rec_key(*od.record_of(v))
            out[i] = memo[k] if k in memo else memo.setdefault(k, keys(k))
        return out

    def keep(self, severities=tuple(pc.NAMES5), ignore_statuses=()):
        return pc.keep_mask(self.filled, severities, ignore_statuses)


def rh_groups(targets, recs):
    """{(batch package, VulnerabilityID): members} of the Red Hat targets: the advisories that
    enter uniqVulns for the package (redhat.go:121-145: trivy-db Get order, the arch test, the
    version test), as oracle.drivers.redhat_detect selects them."""
    out = {}
    for t in targets:
        if t.kind != "redhat":
            continue
        for p, rel in zip(t.pkgs, t.rels):
            if p.get("Release", "").endswith(".remi"):
                continue
            name = od.add_modular_namespace(p.get("Name", ""), p.get("Modularitylabel", ""))
            bi = p.get("BuildInfo")
            if bi is None:
                cs, nvr = od.REDHAT_DEFAULT_CONTENT_SETS.get(str(rel), []), ""
            else:
                cs, nvr = bi.get("ContentSets") or [], f"{bi.get('Nvr', '')}-{bi.get('Arch', '')}"
            inst = od.fmt(p)
            for a in recs.get_redhat(name, cs, [nvr]):
                if a["Arches"] and p.get("Arch", "") != "noarch" and p.get("Arch", "") not in a["Arches"]:
                    continue
                if a["FixedVersion"] == "" or od.rpm_cmp(inst, a["FixedVersion"]) < 0:
                    out.setdefault((int(p["ID"][1:]), a["VulnerabilityID"]), []).append(a)
    # an unfixed advisory enters only when its ID is new (redhat.go:157-162): later ones are no members
    for k, mem in out.items():
        out[k] = [a for j, a in enumerate(mem) if a["FixedVersion"] or j == 0]
    return out


def sev_name(a):
    return od.SEVERITY[a["Severity"]] if 0 <= a["Severity"] < 5 else od.SEVERITY[0]


def representative(members):
    """The member whose FixedVersion the merged entry reports: the greatest in rpm order, ties
    keep the first (redhat.go:178-180 LessThan); without a fixed member the first."""
    best = None
    for a in members:
        if a["FixedVersion"] and (best is None or od.rpm_cmp(best["FixedVersion"], a["FixedVersion"]) < 0):
            best = a
    return best if best is not None else members[0]


def merged_from_members(groups, bucket, severities, ignore_statuses):
    """The merged and filtered Red Hat entries computed from the members alone, the way the
    pass's kernel is specified: per (package, VulnerabilityID) in that order one entry - the
    first member's Severity and Status, Status Fixed when any member is fixed - kept by
    filter.go:113-120 after FillInfo.  [(package, VulnerabilityID, FixedVersion, VendorIDs)]."""
    out = []
    for (p, vid), mem in sorted(groups.items(), key=lambda kv: (kv[0][0], kv[0][1].encode())):
        first, rep = mem[0], representative(mem)
        fixed = [a for a in mem if a["FixedVersion"]]
        v = {"VulnerabilityID": vid, "SeveritySource": "redhat", "Vulnerability": {"Severity": sev_name(first)}}
        if first["Status"]:
            v["Status"] = first["Status"]
        if fixed:
            v["FixedVersion"] = od.rpm_string(rep["FixedVersion"])
        f = vi.fill_info(bucket, [v])
        if pc.keep_mask(f, severities, ignore_statuses)[0]:
            ids = sorted({i for a in fixed for i in (a.get("VendorIDs") or [])})
            out.append((p, vid, v.get("FixedVersion", ""), ids))
    return out


def chain_rh_entries(chain, keep):
    """The kept Red Hat entries of a Chain in merged_from_members' form."""
    return [(int(p), v["VulnerabilityID"], v.get("FixedVersion", ""), list(v.get("VendorIDs") or []))
            for p, v, k, kind in zip(chain.pkg.tolist(), chain.det, keep.tolist(), chain.kind) if k and kind == "redhat"]


def group_facts(chain, groups, keep, severities, ignore_statuses):
    """What a filtered case exercises, judged from the oracle's numbers: counts of
    - Red Hat packages emptied / kept whole;
    - groups kept only because their Status became Fixed (first member's Status ignored, a member fixed);
    - groups kept whose first member's severity passes and whose representative's does not;
    - groups dropped whose representative's severity passes and whose first member's does not;
    - packages of other drivers that share a tile with a Red Hat package and lose a finding."""
    kept_of = {}
    for p, v, k, kind in zip(chain.pkg.tolist(), chain.det, keep.tolist(), chain.kind):
        if kind == "redhat":
            kept_of[(p, v["VulnerabilityID"])] = k
    rh_pkgs = collections.defaultdict(list)
    for (p, _), k in kept_of.items():
        rh_pkgs[p].append(k)
    facts = collections.Counter()
    facts["rh_emptied"] = sum(1 for ks in rh_pkgs.values() if not any(ks))
    facts["rh_whole"] = sum(1 for ks in rh_pkgs.values() if all(ks))
    for key, mem in groups.items():
        if len(mem) < 2:
            continue
        first, rep = mem[0], representative(mem)
        fs, rs = sev_name(first) in severities, sev_name(rep) in severities
        if kept_of[key] and first["Status"] in ignore_statuses and any(a["FixedVersion"] for a in mem):
            facts["kept_by_fixed"] += 1
        if kept_of[key] and fs and not rs:
            facts["kept_by_first_severity"] += 1
        if not kept_of[key] and rs and not fs and first["Status"] not in ignore_statuses \
                and (STATUS_FIXED not in ignore_statuses or not any(a["FixedVersion"] for a in mem)):
            facts["dropped_by_first_severity"] += 1
    rh_tiles = {p // 256 for p in rh_pkgs}
    lost = {p for p, k, kind in zip(chain.pkg.tolist(), keep.tolist(), chain.kind) if kind != "redhat" and not k}
    facts["other_driver_filtered_in_rh_tile"] = sum(1 for p in lost if p // 256 in rh_tiles)
    return facts


# ---- the debian / ubuntu world of tests/test_gpu_pipeline_filter.py (no Red Hat target) -------

DEB_SEED = 13


def deb_world():
    """(sdb, batch, engine): 1320 debian / ubuntu packages over a DB with the "vulnerability" bucket."""
    import trivy_amd
    from tools.synth import make_batch, make_db
    from tools.synth_vuln import vuln_arena
    sdb = make_db(["debian 12", "ubuntu 22.04"], 800, seed=DEB_SEED)
    batch = make_batch(sdb, 11, 120, [1, 1], seed=DEB_SEED)
    db = trivy_amd.DB()
    for arena in (sdb.records_arena((), detail=True), sdb.source_arena(), vuln_arena(sdb.vuln_ids(), DEB_SEED)):
        db.put_arena(*arena)
    return sdb, batch, trivy_amd.Engine(db.finalize(), 0)


def deb_fill(eng, sdb, batch):
    from trivy_amd.batch import MatchBatch
    mb = MatchBatch(eng)
    arena, noff, nlen, voff, vlen = batch.arena()
    for p, b0, b1 in batch.targets:
        mb.add_arena(sdb.platforms[p], b1 - b0, arena, noff[b0:], nlen[b0:], voff[b0:], vlen[b0:])
    return mb


# ---- World C --------------------------------------------------------------------------------

BIG, SMALL = "bigpkg", "smallpkg"
BIG_CVE = "CVE-2021-5000"
N_BIG_RHSA = 150
N_BEFORE = 63  # entries of BIG's list in front of the big group
N_REPEAT = 300


def world_c_records():
    """Fixture-format records ({"path", "value"}) of the hand-built Red Hat DB."""
    recs = [{"path": ["data-source", "Red Hat"], "value": json.dumps({"ID": "redhat", "Name": "Red Hat", "URL": "https://rh"})}]
    for r, cps in sm.RH_REPOS.items():
        recs.append({"path": ["Red Hat CPE", "repository", r], "value": json.dumps(cps)})
    for r, cps in sm.RH_NVRS.items():
        recs.append({"path": ["Red Hat CPE", "nvr", r], "value": json.dumps(cps)})
    for i, c in enumerate(sm.RH_CPE_NAMES):
        recs.append({"path": ["Red Hat CPE", "cpe", str(i)], "value": json.dumps(c)})
    aff = sm.RH_CPES[8]

    def put(name, vid, ent):
        recs.append({"path": ["Red Hat", name, vid], "value": json.dumps({"Entries": [dict(ent, Affected=aff)]})})

    # BIG: 63 single entries of lower CVE IDs, then the big CVE - one unfixed entry (Status 5,
    # will_not_fix) in front of 150 RHSA advisories with increasing FixedVersions - then three more
    for i in range(N_BEFORE):
        if i % 3 == 0:
            put(BIG, f"RHSA-2019:{1000 + i}", {"Cves": [{"ID": f"CVE-2019-{1000 + i}", "Severity": i % 5}],
                                             "FixedVersion": f"0:2.{i}.0-1.el8_0"})
        else:
            put(BIG, f"CVE-2019-{1000 + i}", {"Cves": [{"Severity": i % 5}], "FixedVersion": "", "Status": (5, 6)[i % 2]})
    put(BIG, BIG_CVE, {"Cves": [{"Severity": 3}], "FixedVersion": "", "Status": 5})
    for k in range(N_BIG_RHSA):
        put(BIG, f"RHSA-2021:{2000 + k}", {"Cves": [{"ID": BIG_CVE, "Severity": k % 3}],  # never HIGH: only the first member is
                                         "FixedVersion": f"0:3.0.{k}-1.el8_0"})
    for i in range(3):
        put(BIG, f"CVE-2022-{3000 + i}", {"Cves": [{"Severity": 4}], "FixedVersion": "", "Status": 6})
    # SMALL: three CVEs of two members each
    put(SMALL, "RHSA-2020:0100", {"Cves": [{"ID": "CVE-2020-0001", "Severity": 1}], "FixedVersion": "0:1.5.0-1.el8_0"})
    put(SMALL, "RHSA-2020:0200", {"Cves": [{"ID": "CVE-2020-0001", "Severity": 4}], "FixedVersion": "0:2.5.0-1.el8_0"})
    put(SMALL, "RHSA-2020:0300", {"Cves": [{"ID": "CVE-2020-0002", "Severity": 4}], "FixedVersion": "0:2.5.0-1.el8_0"})
    put(SMALL, "RHSA-2020:0400", {"Cves": [{"ID": "CVE-2020-0002", "Severity": 1}], "FixedVersion": "0:1.5.0-1.el8_0"})
    put(SMALL, "CVE-2020-0003", {"Cves": [{"Severity": 3}], "FixedVersion": "", "Status": 7})
    put(SMALL, "RHSA-2020:0500", {"Cves": [{"ID": "CVE-2020-0003", "Severity": 2}], "FixedVersion": "0:1.5.0-1.el8_0"})
    return recs


class WorldCBatch:
    """The batch in tools/synth_mix.py's group form (one Red Hat group), so sm.add_to and
    sm.driver_packages serve it: BIG below every fix 300 times, then SMALL at versions that make
    some members not match (1.0: all; 2.0: only the 2.5.0 fixes and the unfixed one; 3.0: the
    unfixed one only), then BIG again between two fixes."""

    plats = [("Red Hat", "redhat")]

    def __init__(self):
        names = [BIG] * N_REPEAT + [SMALL] * 30 + [BIG] * 3
        vers = ["1.0.0"] * N_REPEAT + ["1.0.0", "2.0.0", "3.0.0"] * 10 + ["3.0.70", "1.0.0", "3.0.200"]
        n = len(names)
        s = lambda xs: np.array([x.encode() for x in xs], dtype="S")  # noqa: E731
        g = {"key": np.zeros(n, dtype=np.int64), "name": s(names), "pname": s(names), "label": s([""] * n),
             "rhrel": np.full(n, 8), "bi": np.zeros(n, dtype=bool), "nvr": s([""] * n), "version": s(vers),
             "rel": s(["1.el8_0"] * n), "epoch": np.zeros(n, dtype=np.int64),
             "ver": s([v + "-1.el8_0" for v in vers]), "arch": s(["x86_64"] * n)}
        self.groups = [(0, g)]

    def __len__(self):
        return len(self.groups[0][1]["key"])


def world_c_targets():
    batch = WorldCBatch()
    p, g = batch.groups[0]
    pkgs = with_ids(sm.driver_packages(batch, p, g, np.arange(len(batch))), 0)
    return batch, [Target(0, "redhat", pkgs, None, [8] * len(pkgs))], od.Records(world_c_records())
