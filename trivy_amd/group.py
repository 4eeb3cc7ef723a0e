"""Engine groups: one batch sharded over several GPUs inside one process (tvm_group_* of
include/trivy_amd.h).

The reference serves every concurrent scan from one process (pkg/rpc/server/server.go:45-56);
an EngineGroup lets that process cut a fleet batch over the GPUs of a node without a second
process or a collective library.  A member is a plain engine / batch: GroupBatch.member(k) is a
MatchBatch over a borrowed handle, so every accessor of trivy_amd.batch works on it, and every
package index it reports is global (its package base).  trivy_amd/dist.py stays the
one-process-per-GPU form of the same shard rule.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import lib, errbuf
from .batch import MatchBatch
from .db import Engine

PLAN_PACKAGES, PLAN_ROWS = 0, 1


class _MemberEngine(Engine):
    """Member k of a group: borrowed, closed by the group."""

    def __init__(self, h, db):  # noqa: super().__init__ would open an engine
        self.h, self.db = h, db

    def swap(self, db):
        raise RuntimeError("a group's members are swapped together: EngineGroup.swap")

    def close(self):
        self.h = None


class _MemberBatch(MatchBatch):
    """Member k's batch of a group batch: borrowed, freed by the group batch."""

    def __init__(self, engine, h):  # noqa: super().__init__ would allocate a batch
        self.engine, self.h, self.total = engine, h, None

    def close(self):
        self.h = None


class EngineGroup:
    """len(devices) engines over one DB (fails loudly without a GPU).  A device may be named
    more than once: several members on one GPU, a test and fallback shape, not a speed-up."""

    def __init__(self, db, devices=(0,)):
        if not db._finalized:
            db.finalize()
        e = errbuf()
        dv = (ctypes.c_int * max(len(devices), 1))(*devices)
        self.db = db
        self.h = lib().tvm_group_open(db.h, dv, len(devices), e, len(e))
        if not self.h:
            raise RuntimeError(f"tvm_group_open: {e.value.decode()}")
        self.engines = [_MemberEngine(lib().tvm_group_engine(self.h, k), db) for k in range(len(devices))]

    def __len__(self):
        return lib().tvm_group_size(self.h)

    def swap(self, db):
        """Every member's tables replaced (all built first; a failure swaps none)."""
        if not db._finalized:
            db.finalize()
        e = errbuf()
        if lib().tvm_group_swap(self.h, db.h, e, len(e)):
            raise RuntimeError(f"tvm_group_swap: {e.value.decode()}")
        self.db = db
        for m in self.engines:
            m.db = db

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            for m in self.engines:
                m.close()
            if _lib is not None and _lib._lib is not None:  # (None: the interpreter is tearing the module down)
                _lib._lib.tvm_group_close(h)

    def __del__(self):
        self.close()


class GroupBatch:
    """One batch of targets over a group's members; one caller at a time per GroupBatch
    (different GroupBatches of one group may run concurrently)."""

    def __init__(self, group):
        self.group = group
        self.h = lib().tvm_group_batch_new(group.h)
        if not self.h:
            raise RuntimeError("tvm_group_batch_new: the group is closed")
        self._members = {}
        self.pipe_cap = None
        self._caps = None

    # ---- building (the MatchBatch calls tools.synth_mix.BulkCols.add uses) ----
    def cpe_set(self, content_sets, nvr=""):
        from ._lib import Str, s
        keep = [s(x) for x in content_sets]
        arr = (Str * max(len(keep), 1))(*keep)
        i = lib().tvm_group_batch_cpe_set(self.h, arr, len(keep), s(nvr))
        if i < 0:
            raise RuntimeError("tvm_group_batch_cpe_set failed")
        return i

    def add_targets(self, buckets, target_end, arena, name_off, name_len, ver_off, ver_len, flags=None,
                    arch_off=None, arch_len=None, cpe_sets=None, plan=PLAN_PACKAGES):
        """MatchBatch.add_targets over the group, once per GroupBatch: plans the shards (plan =
        PLAN_PACKAGES or PLAN_ROWS) and builds the member batches from slices of the columns."""
        from ._lib import AttrCols, Str
        bl = [b.encode() if isinstance(b, str) else bytes(b) for b in buckets]
        arr = (Str * max(len(bl), 1))(*[Str(b, len(b)) for b in bl])
        te = np.ascontiguousarray(target_end, dtype=np.uint64)
        cols = [np.ascontiguousarray(c, dtype=t) for c, t in ((name_off, np.uint64), (name_len, np.uint32),
                                                              (ver_off, np.uint64), (ver_len, np.uint32))]
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32)
        ao = None if arch_off is None else np.ascontiguousarray(arch_off, dtype=np.uint64)
        al = None if arch_len is None else np.ascontiguousarray(arch_len, dtype=np.uint32)
        cs = None if cpe_sets is None else np.ascontiguousarray(cpe_sets, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        attrs = AttrCols(ptr(ao), ptr(al), ptr(cs))
        rc = lib().tvm_group_batch_add_targets(self.h, plan, len(bl), arr, ptr(fl), te.ctypes.data, arena,
                                               *[c.ctypes.data for c in cols], ctypes.byref(attrs))
        if rc:
            raise RuntimeError("tvm_group_batch_add_targets rejected the targets")
        return 0

    def __len__(self):
        return lib().tvm_group_batch_size(self.h)

    def shards(self):
        """Package boundaries: member k holds [shards()[k], shards()[k + 1])."""
        out = np.zeros(len(self.group) + 1, dtype=np.uint64)
        if lib().tvm_group_batch_shards(self.h, out.ctypes.data):
            raise RuntimeError("tvm_group_batch_shards")
        return [int(x) for x in out]

    def member(self, k):
        """Member k's batch as a MatchBatch (borrowed), None for an empty shard."""
        h = lib().tvm_group_batch_member(self.h, k)
        if not h:
            return None
        m = self._members.get(k)
        if m is None or m.h != h:
            m = self._members[k] = _MemberBatch(self.group.engines[k], h)
        m.pipe_cap = self._caps[k] if getattr(self, "_caps", None) is not None else self.pipe_cap
        return m

    def members(self):
        """[(k, MatchBatch)] of the non-empty shards, in batch order."""
        return [(k, m) for k in range(len(self.group)) for m in [self.member(k)] if m is not None]

    def _check(self, rc, e, what):
        if rc:
            raise RuntimeError(f"{what}: {e.value.decode()}")

    # ---- pipelined pass ----
    def pipeline_prepare(self, match_cap=None, chunk_packages=1 << 19, raw=False, adv32=False, rh_merge=False,
                         member_caps=None):
        e = errbuf()
        cap = match_cap if match_cap is not None else max(1024, 8 * len(self))
        flags = (1 if raw else 0) | (2 if adv32 else 0) | (4 if rh_merge else 0)
        mc = None if member_caps is None else np.ascontiguousarray(member_caps, dtype=np.uint64)
        self._check(lib().tvm_group_pipeline_prepare(self.h, cap, mc.ctypes.data if mc is not None else None,
                                                     chunk_packages, flags, e, len(e)), e, "tvm_group_pipeline_prepare")
        self.pipe_cap = cap
        self._caps = None if mc is None else [int(x) for x in mc]
        return self

    def vuln_ranks(self, str_array, n):
        return MatchBatch.vuln_ranks(_MemberBatch(self.group.engines[0], None), str_array, n)

    def filter_opts(self, *a, **kw):
        """MatchBatch.filter_opts (ranks from member 0's tables: every member holds the same DB)."""
        return MatchBatch.filter_opts(self, *a, **kw)

    def pipeline_set_filter(self, opts):
        e = errbuf()
        rc = lib().tvm_group_pipeline_set_filter(self.h, ctypes.byref(opts) if opts is not None else None, e, len(e))
        if rc == 3:  # TVM_EINVAL: a refusal; no member keeps a filter
            raise ValueError(f"tvm_group_pipeline_set_filter: {e.value.decode() or 'invalid argument'}")
        self._check(rc, e, "tvm_group_pipeline_set_filter")
        return self

    def pipeline_run(self):
        """One pass on every member at once: (matches, first poisoned package or -1, wall ms);
        self.member_matches = the members' raw counts (also set when OverflowError is raised,
        which carries the summed raw count)."""
        e = errbuf()
        n, errp, ms = ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_double()
        mm = np.zeros(len(self.group), dtype=np.uint64)
        rc = lib().tvm_group_pipeline_run(self.h, ctypes.byref(n), ctypes.byref(errp), ctypes.byref(ms), mm.ctypes.data,
                                          e, len(e))
        self.member_matches = [int(x) for x in mm]
        caps = self._caps if self._caps is not None else [self.pipe_cap] * len(mm)
        if rc == 3 and self.pipe_cap is not None and any(m > c for m, c in zip(self.member_matches, caps)):
            raise OverflowError(n.value)
        self._check(rc, e, "tvm_group_pipeline_run")
        return n.value, errp.value, ms.value

    def pipeline_csr(self):
        """(adv, row_end) of the whole batch: the members' lists concatenated, row ends rebased
        (copies; for tests - the product reads each member's lists in place)."""
        adv, rend, a0 = [], [], 0
        for _, m in self.members():
            a, r = m.pipeline_csr()
            adv.append(a)
            rend.append(r.astype(np.uint64) + np.uint64(a0))
            a0 += len(a)
        if not adv:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return np.concatenate(adv), np.concatenate(rend).astype(np.uint32)

    def vulns(self, pipeline=False):
        """The members' VulnSets in batch order (each numbers its own grp_recs)."""
        return [m.vulns(pipeline=pipeline) for _, m in self.members()]

    # ---- device-resident pass ----
    def upload(self, match_cap=None, member_caps=None):
        e = errbuf()
        cap = match_cap if match_cap is not None else max(1024, 8 * len(self))
        mc = None if member_caps is None else np.ascontiguousarray(member_caps, dtype=np.uint64)
        self._check(lib().tvm_group_upload(self.h, cap, mc.ctypes.data if mc is not None else None, e, len(e)), e,
                    "tvm_group_upload")
        return self

    def launch(self):
        e = errbuf()
        self._check(lib().tvm_group_launch(self.h, e, len(e)), e, "tvm_group_launch")
        return self

    def status(self):
        """(n_matches, first poisoned global package or -1, error bits); self.member_matches."""
        n, errp, bits = ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_uint64()
        mm = np.zeros(len(self.group), dtype=np.uint64)
        rc = lib().tvm_group_status(self.h, ctypes.byref(n), ctypes.byref(errp), ctypes.byref(bits), mm.ctypes.data)
        if rc:
            raise RuntimeError(f"tvm_group_status failed ({rc})")
        self.member_matches = [int(x) for x in mm]
        return n.value, errp.value, bits.value

    def csr_into(self, root, csr_adv, row_end):
        """The whole batch's ordered lists into int32 torch tensors on member root's device (or
        anything with their data_ptr() / numel() / dtype.itemsize; csr_adv >= the match count,
        row_end one entry per package); returns the match count.
        ValueError(total) when the tensors are too small or the lists cannot be handed out."""
        if row_end.numel() < len(self) or csr_adv.dtype.itemsize != 4 or row_end.dtype.itemsize != 4:
            raise ValueError("row_end needs one 4-byte entry per package, csr_adv 4-byte entries")
        e, n = errbuf(), ctypes.c_uint64()
        rc = lib().tvm_group_csr_into(self.h, root, csr_adv.data_ptr(), row_end.data_ptr(), csr_adv.numel(),
                                      ctypes.byref(n), e, len(e))
        if rc == 3:
            raise ValueError(n.value)
        self._check(rc, e, "tvm_group_csr_into")
        return n.value

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            for m in self._members.values():
                m.close()
            if _lib is not None and _lib._lib is not None:
                _lib._lib.tvm_group_batch_free(h)

    def __del__(self):
        self.close()
