"""Shared by the tests of the pipelined pass's severity / status filter: the oracle's view of
every matched (package, advisory) pair - its DetectedVulnerability as the debian / ubuntu
drivers build it, FillInfo applied (oracle/vulninfo.py), and filter.go:113-120's two tests."""
import json

import numpy as np

import oracle.vulninfo as vi
from oracle import match as om
from tools.synth import DEBIAN_DS, UBUNTU_DS
from tools.synth_vuln import vuln_values

NAMES5 = ["UNKNOWN", "LOW", "MEDIUM", "HIGH", "CRITICAL"]


def detected(sdb, batch, opk, oad):
    """The DetectedVulnerability of every oracle pair, in detection order, with "_pair"."""
    ds_of = {p: json.loads((DEBIAN_DS if p.startswith("debian") else UBUNTU_DS).decode()) for p in sdb.platforms}
    out = []
    for pk, adv in zip(opk.tolist(), oad.tolist()):
        plat = sdb.platforms[int(batch.plat[pk])]
        v = {"VulnerabilityID": sdb.adv_vid[adv].decode(), "PkgName": batch.names[pk].decode(),
             "InstalledVersion": batch.versions[pk].decode(), "DataSource": ds_of[plat], "_pair": (pk, adv)}
        if sdb.adv_fixed[adv]:
            v["FixedVersion"] = sdb.adv_fixed[adv].decode()
        if plat.startswith("debian"):  # debian.go:89-98
            st, sev = sdb.adv_detail(adv)
            if st:
                v["Status"] = st
            if sev:
                v["SeveritySource"] = "debian"
                v["Vulnerability"] = {"Severity": NAMES5[sev]}
        out.append(v)
    return out


def filled(sdb, seed, vulns):
    """FillInfo (oracle) over detected(); "_pair" carried along."""
    bucket = {k.decode(): v.decode() for k, v in vuln_values(sdb.vuln_ids(), seed)}
    got = vi.fill_info(bucket, [{k: x for k, x in v.items() if k != "_pair"} for v in vulns])
    for f, v in zip(got, vulns):
        f["_pair"] = v["_pair"]
    return got


def keep_mask(fl, severities, ignore_statuses=()):
    """filter.go:113-120 per finding: its severity is asked for and its status is not ignored."""
    return np.array([((f.get("Vulnerability") or {}).get("Severity") or "UNKNOWN") in severities
                     and f.get("Status", 0) not in ignore_statuses for f in fl], dtype=bool)


def oracle_pairs(sdb, batch, threads=4):
    return om.match(om.Prepared(sdb, batch), n_threads=threads)
