"""CPU: the pipelined pass's severity / status filter - its C-ABI entry points exist and refuse
NULL handles, and the claim the feature rests on, at oracle level: dropping the findings that
fail filter.go:113-120 before result.Filter gives what result.Filter gives over the whole list,
for the kept list and for the ignored list."""
import ctypes

import numpy as np
import pytest

import oracle.filter as of
import pipe_filter_cases as pc
from tools.synth import SynthBatch, make_batch, make_db

TVM_EINVAL = 3


def test_entry_points_refuse_null_handles():
    from trivy_amd._lib import errbuf, lib
    L = lib()
    e = errbuf()
    assert L.tvm_pipeline_set_filter(None, None, None, e, len(e)) == TVM_EINVAL
    out = (ctypes.c_uint64 * 2)()
    assert L.tvm_pipeline_filter_stats(None, out) == TVM_EINVAL
    # a batch never prepared has no completed pass either
    b = L.tvm_batch_new()
    try:
        assert L.tvm_pipeline_filter_stats(b, out) == TVM_EINVAL
        assert L.tvm_pipeline_set_filter(None, b, None, e, len(e)) == TVM_EINVAL
    finally:
        L.tvm_batch_free(b)


@pytest.mark.parametrize("severities,statuses", [(("HIGH", "CRITICAL"), (5, 7)), (("LOW",), ()), (pc.NAMES5, ()),
                                                 ((), ())])
def test_prefilter_then_filter_equals_filter(severities, statuses, oracle_built):
    seed = 9
    sdb = make_db(["debian 12", "ubuntu 22.04"], 800, seed=seed)
    b0 = make_batch(sdb, 6, 120, [1, 1], seed=seed)
    # every result ends with copies of a quarter of its packages (same name and version): the
    # dedup of filter.go:124-134 has work to do
    plat, names, vers, targets = [], [], [], []
    for p, s, e in b0.targets:
        start = len(names)
        for i in list(range(s, e)) + list(range(s, e, 4)):
            plat.append(p)
            names.append(b0.names[i])
            vers.append(b0.versions[i])
        targets.append((p, start, len(names)))
    batch = SynthBatch(np.array(plat, dtype=np.int32), names, vers, targets)
    opk, oad = pc.oracle_pairs(sdb, batch)
    fl = pc.filled(sdb, seed, pc.detected(sdb, batch, opk, oad))
    keep = pc.keep_mask(fl, severities, statuses)
    assert len(fl) > 500
    if severities and len(severities) < 5:
        assert 0 < keep.sum() < len(fl)
    ids = sorted({f["VulnerabilityID"] for f, k in zip(fl, keep) if k})[:5] + ["CVE-0000-none"]
    findings = [{"ID": i, "Paths": [], "PURLs": [], "ExpiredAt": None, "Statement": ""} for i in ids]
    tgt_of = np.zeros(len(batch), dtype=np.int64)
    for t, (_, s, e) in enumerate(batch.targets):
        tgt_of[s:e] = t
    n_kept = n_ign = 0
    for t in range(len(batch.targets)):
        whole = [f for f in fl if tgt_of[f["_pair"][0]] == t]
        pre = [f for f, k in zip(fl, keep) if k and tgt_of[f["_pair"][0]] == t]
        want = of.filter_vulnerabilities("", whole, list(severities), statuses, findings)
        got = of.filter_vulnerabilities("", pre, pc.NAMES5, (), findings)
        assert got == want, t
        n_kept += len(want[0] or [])
        n_ign += len(want[1])
    if severities:
        assert n_kept and n_ign
