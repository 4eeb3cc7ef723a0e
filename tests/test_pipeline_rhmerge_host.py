"""CPU: the Red Hat merge inside the pipelined pass (TVM_PIPE_RH_MERGE) - what needs no GPU.

* tvm_pipeline_prepare's flag check: the new flag and an unknown bit both answer TVM_EINVAL on
  null handles (the flag is accepted by the mask only with real handles).
* The checker of tests/test_gpu_pipeline_rhmerge.py: for World C, the merged and filtered lists
  pipe_rhmerge_cases computes from the members alone (first member's Severity and Status, Fixed
  when any member is fixed, the representative's FixedVersion, the fixed members' VendorIDs)
  equal oracle.drivers.driver_detect -> oracle.vulninfo.fill_info -> keep_mask per target."""
import pytest

import pipe_rhmerge_cases as rc

TVM_EINVAL = 3


def test_prepare_flag_bits_on_null_handles():
    from trivy_amd._lib import lib
    for flags in (4, 8, 4 | 8, 1 | 2 | 4):
        assert lib().tvm_pipeline_prepare(None, None, 16, 256, flags, None, 0) == TVM_EINVAL


@pytest.fixture(scope="module")
def world_c(oracle_built):
    batch, targets, recs = rc.world_c_targets()
    return batch, targets, recs, rc.Chain(targets, recs, {}), rc.rh_groups(targets, recs)


def test_world_c_shape(world_c):
    """The big group has 151 members and starts at raw position 63 of its package's list; the
    second name has three CVEs of two members; some of its packages match only some members."""
    batch, targets, recs, chain, groups = world_c
    big = groups[(0, rc.BIG_CVE)]
    assert len(big) == 1 + rc.N_BIG_RHSA and big[0]["FixedVersion"] == "" and big[0]["Status"] == 5
    before = sum(len(m) for (p, vid), m in groups.items() if p == 0 and vid.encode() < rc.BIG_CVE.encode())
    assert before == rc.N_BEFORE == 63
    assert all(len(groups[(p, rc.BIG_CVE)]) == 151 for p in range(rc.N_REPEAT))
    small = {k: m for k, m in groups.items() if rc.N_REPEAT <= k[0] < rc.N_REPEAT + 30}
    assert sorted({len(m) for m in small.values()}) == [1, 2]
    assert {vid for _, vid in small} == {"CVE-2020-0001", "CVE-2020-0002", "CVE-2020-0003"}
    assert len(groups[(rc.N_REPEAT + 30, rc.BIG_CVE)]) == 1 + (rc.N_BIG_RHSA - 71)  # installed 3.0.70
    assert (rc.N_REPEAT + 32, rc.BIG_CVE) in groups and len(groups[(rc.N_REPEAT + 32, rc.BIG_CVE)]) == 1


@pytest.mark.parametrize("mask", [dict(), dict(ignore_statuses=(5,)), dict(ignore_statuses=(3,))] + rc.MASKS,
                         ids=["all", "ign5", "ign3", "high-critical-ign5-7", "low"])
def test_members_view_equals_driver_chain(world_c, mask):
    batch, targets, recs, chain, groups = world_c
    mask = dict({"severities": tuple(rc.pc.NAMES5), "ignore_statuses": ()}, **mask)
    keep = chain.keep(**mask)
    want = rc.chain_rh_entries(chain, keep)
    got = rc.merged_from_members(groups, {}, mask["severities"], mask["ignore_statuses"])
    assert len(want) > 0 and got == want
    # every kept or dropped entry is a group the members view knows
    assert {(int(p), v["VulnerabilityID"]) for p, v in zip(chain.pkg.tolist(), chain.det)} == set(groups)


def test_world_c_heavy_group_in_the_oracle(world_c):
    """The oracle's own entry for the 151-member group: the greatest FixedVersion, every RHSA as
    VendorIDs, the first member's severity; kept under ignore_statuses=(5,) (its Status became
    Fixed), dropped under (3,)."""
    batch, targets, recs, chain, groups = world_c
    i = next(i for i, (p, v) in enumerate(zip(chain.pkg.tolist(), chain.det)) if p == 0 and v["VulnerabilityID"] == rc.BIG_CVE)
    v = chain.det[i]
    assert v["FixedVersion"] == f"3.0.{rc.N_BIG_RHSA - 1}-1.el8_0" and v["Severity"] == "HIGH" and v["Status"] == 5
    assert v["VendorIDs"] == sorted(f"RHSA-2021:{2000 + k}" for k in range(rc.N_BIG_RHSA))
    assert chain.filled[i]["Status"] == rc.STATUS_FIXED
    assert chain.keep(ignore_statuses=(5,))[i] and not chain.keep(ignore_statuses=(3,))[i]
