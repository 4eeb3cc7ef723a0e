// One tile's share of the pipelined pass's severity / status filter (prefilter.hip), as a device
// function: prefilter_tiles runs it for every tile of a chunk, and the Red Hat merge kernel
// (rhmerge.hip) for the tiles of a filtered chunk that hold no Red Hat package.
#pragma once
#include "pipeline.h"

namespace tvm {

// An advisory index beyond the table (never expected): what fill_pairs_kernel decides for it,
// severity UNKNOWN and StatusAffected.
constexpr uint32_t kClsUnknown = 0u | (2u << 8);
constexpr int kPreRounds = 4;  // 64-entry rounds loaded before the first is used

// One wavefront per tile.  The wave walks its tile's segment
// [base, base + count) of the match columns 64 entries a round and stores the entries that
// pass to base + (entries kept so far) + (rank among the round's kept lanes): stable, in place.
//
// Why in place is safe.  The stores of round r land below kept + 64 <= (r + 1) * 64 within the
// segment, and every later round reads at or above that point; within a round all 64 lanes'
// loads are one instruction, which has completed before the stores that depend on its data
// issue.  Rounds are loaded kPreRounds at a time (a group), and that keeps the invariant: every
// load of the group is issued before the group's first store (a wavefront-scope fence keeps the
// compiler from sinking a load below a store), loads return in issue order, and round r's
// stores wait for round r's data - so a load still in flight when they issue belongs to a
// later round and reads at or above (r + 1) * 64.  The next group's loads are issued after this
// group's stores and read at or above 256(g + 1), where no store of groups <= g lands.
// Segments of different tiles are disjoint (one reservation per tile), so waves never touch
// each other's.  Unrolling further must keep the loads of a group ahead of its stores.
__device__ __forceinline__ void prefilter_tile_wave(const PrefilterArgs& a, uint32_t t, uint32_t lane) {
  const TileDir d = a.dir[t];
  if (d.base + d.count > a.cap) return;  // an overflowed pass: left alone, as the result move leaves it
  const uint32_t sev_mask = a.sev_mask & 0x1Fu;  // SeverityNames only: index 5 never passes
  uint32_t* __restrict__ pkg = a.pkg + d.base;
  uint32_t* __restrict__ adv = a.adv + d.base;
  uint32_t kept = 0;
  for (uint32_t i0 = 0; i0 < d.count; i0 += kPreRounds * 64) {
    uint32_t p[kPreRounds], v[kPreRounds], c[kPreRounds];
#pragma unroll
    for (int r = 0; r < kPreRounds; r++) {
      const uint32_t i = i0 + r * 64 + lane;
      p[r] = i < d.count ? pkg[i] : 0u;
      v[r] = i < d.count ? adv[i] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int r = 0; r < kPreRounds; r++) c[r] = v[r] < a.n_cls ? uint32_t(a.cls[v[r]]) : kClsUnknown;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the group's loads stay above its stores
#pragma unroll
    for (int r = 0; r < kPreRounds; r++) {
      const uint32_t i = i0 + r * 64 + lane;
      // filter.hip filter_mark's predicate (filter.go:113-120)
      const bool keep = i < d.count && ((sev_mask >> (c[r] & 0xFFu)) & 1u) && !((a.status_mask >> ((c[r] >> 8) & 31u)) & 1u);
      const unsigned long long m = __ballot(keep);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
      if (keep) {
        pkg[kept + rank] = p[r];
        adv[kept + rank] = v[r];
      }
      kept += uint32_t(__popcll(m));
    }
  }
  if (lane == 0) {
    a.dir[t].count = kept;
    if (kept) atomicAdd(a.ctl + kCtlKept, (unsigned long long)kept);
  }
}

}  // namespace tvm
