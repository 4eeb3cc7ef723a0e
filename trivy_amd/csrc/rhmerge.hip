// Red Hat per-CVE merge inside the pipelined pass (gfx950): the uniqVulns loop of
// pkg/detector/ospkg/redhat/redhat.go:146-187 applied to a chunk's match segments in HBM, behind
// the chunk's match launch and ahead of its result move, so the pass's result already is the
// DetectedVulnerability set (record indices, tvm_vuln_set.rec) and crosses the link once.
//
// A tile is 256 consecutive packages and a package's matches never leave its tile's segment; in
// a Red Hat package's list the members of one VulnerabilityID are adjacent and the IDs ascend
// (db.cpp flatten_os, redhat.hip).  The merge is therefore a stable compaction per tile, the
// shape of the severity / status filter (prefilter_tile.h), and the filter's predicate is
// applied to the merged entries in the same walk when one is set.  Tiles without Red Hat
// packages take the filter's own path (filtered pass) or are not visited (unfiltered pass).
// Integer work bound by memory latency; no MFMA, no scratch, no workgroup barrier.
#include "pipeline.h"
#include "prefilter_tile.h"
#include "redhat.h"

namespace tvm {

namespace {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr uint32_t kStatusFixed = 3;  // dbTypes.StatusFixed
constexpr int kCountRounds = 4;       // 64-entry rounds the counting walk keeps in flight

// Per package of tile t: 1 = a Red Hat package; one wave fills its own 256 flags in LDS.
__device__ __forceinline__ void tile_flags(const RhMergeArgs& a, uint32_t t, uint32_t lane, uint8_t* rhp) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t p = t * kTile + lane * 4 + k;
    const uint32_t plat = p < a.n ? a.pk[p].x : 0xFFFFFFFFu;
    rhp[lane * 4 + k] = plat < a.n_plats && a.plats[plat].drv == DRV_REDHAT;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint2 rank_of(const RhMergeArgs& a, uint32_t ad) {
  return ad < a.n_rk ? a.rk[ad] : make_uint2(kNoKey, RH_NONE);
}

// The lane's entry i of a segment of cnt entries: package p, advisory ad, and its group key -
// the VulnerabilityID rank for a Red Hat package's entry (fr = its fixed-version rank), kNoKey
// for every other entry and beyond the segment.
__device__ __forceinline__ uint32_t entry_key(const RhMergeArgs& a, const uint32_t* pkg, const uint32_t* adv, uint32_t i,
                                              uint32_t cnt, uint32_t t, const uint8_t* rhp, uint32_t& p, uint32_t& ad,
                                              uint32_t& fr) {
  fr = RH_NONE;
  p = 0xFFFFFFFFu;
  ad = 0xFFFFFFFFu;
  if (i >= cnt) return kNoKey;
  p = pkg[i];
  ad = adv[i];
  if (!rhp[(p - a.pkg_base - t * kTile) & (kTile - 1)]) return kNoKey;
  const uint2 r = rank_of(a, ad);
  fr = r.y;
  return r.x;
}

// The (package, key) of the entry before the lane's, by shuffle; lane 0 takes the previous
// round's last entry (prev_*, advanced here to this round's last).  left = entries from this
// round on.
__device__ __forceinline__ void entry_before(uint32_t lane, uint32_t p, uint32_t k, uint32_t& prev_p, uint32_t& prev_k,
                                             uint32_t left, uint32_t& pp, uint32_t& kp) {
  const uint32_t up = __shfl_up(p, 1, 64), uk = __shfl_up(k, 1, 64);
  pp = lane ? up : prev_p;
  kp = lane ? uk : prev_k;
  const int last = int((left < 64u ? left : 64u) - 1);
  prev_p = __shfl(p, last, 64);
  prev_k = __shfl(k, last, 64);
}

// One wavefront per tile, four tiles per workgroup.  A Red Hat tile's wave walks its segment
// [base, base + count) twice, 64 entries a round.
//
// Walk 1 reads only: an entry heads a group unless it is a Red Hat entry continuing its
// predecessor's (package, VulnerabilityID rank); the tile's groups of several members and their
// members are counted, and one 64-bit add on the control block reserves the tile's slots of the
// pass's group and member lists (no add for a tile without such groups).  An ID rank that
// descends inside a package is ERR_RH_ORDER, which fails the pass.
//
// Walk 2 compacts: every head lane walks ahead over its group's members for the representative
// (the greatest fixed-version rank; ties keep the first; no fixed member: the first), tests the
// filter (the first member's class; StatusFixed when any member is fixed, as FillInfo decides
// for an entry that has a FixedVersion, vulnerability.go:65-66), and the kept heads are stored
// to base + (kept so far) + (rank among the round's kept lanes) with adv = the record index.
//
// Why in place is safe.  The stores of round r land below kept + 64 <= (r + 1) * 64 within the
// segment.  Round r's own loads, its head lanes' loads ahead (which start inside round r, where
// those stores land) and the member copies all come before the round's first store in program
// order: the walk-ahead loop leaves a lane only on a loaded value, so its loads have returned;
// a member copy's store to the member list (another buffer) waits for its load, and a wave's
// memory instructions issue in order; a wavefront-scope fence keeps the compiler from sinking
// any of them below the stores.  Every later round, and every walk ahead of a later round, reads
// at or above (r + 1) * 64.  Segments of different tiles are disjoint, so waves never touch each
// other's.  Round r + 1's own entries (with their ranks and classes, which live in other
// buffers) are loaded under round r's walk: they lie at or above (r + 1) * 64, where neither
// round r's stores nor any earlier round's land, and they are issued behind round r - 1's
// stores.  No load reaches further ahead than that: a head lane's walk must start inside its own
// round, so it cannot be issued before the stores of the round before.  Walk 1 stores nothing
// to the segment and keeps four rounds in flight.
__global__ __launch_bounds__(256) void rhmerge_tiles(RhMergeArgs a) {
  __shared__ uint8_t rhp_all[4][kTile];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = a.f.t0 + blockIdx.x * 4 + wave;
  if (t >= a.f.t1) return;  // whole wavefronts; no workgroup barrier follows
  if (!a.tile_rh[t]) {
    if (a.filter) prefilter_tile_wave(a.f, t, lane);
    return;
  }
  const TileDir d = a.f.dir[t];
  if (d.base + d.count > a.f.cap) return;  // an overflowed pass: left alone, as the result move leaves it
  uint8_t* rhp = rhp_all[wave];
  tile_flags(a, t, lane, rhp);
  uint32_t* pkg = a.f.pkg + d.base;  // read ahead of and stored behind the walk: not restrict
  uint32_t* adv = a.f.adv + d.base;
  const uint32_t cnt = d.count;
  const unsigned long long lt = (1ull << lane) - 1ull;

  // walk 1: the tile's groups of several members, their members, the order check
  uint32_t n_multi = 0, n_cont = 0, prev_p = 0xFFFFFFFFu, prev_k = kNoKey, prev_h = 1;
  bool order_bad = false;
  for (uint32_t c0 = 0; c0 < cnt; c0 += kCountRounds * 64) {
    uint32_t ps[kCountRounds], as[kCountRounds], ks[kCountRounds];
#pragma unroll
    for (int r = 0; r < kCountRounds; r++) {
      const uint32_t i = c0 + r * 64 + lane;
      ps[r] = i < cnt ? pkg[i] : 0xFFFFFFFFu;
      as[r] = i < cnt ? adv[i] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int r = 0; r < kCountRounds; r++) {
      const bool rh = c0 + r * 64 + lane < cnt && rhp[(ps[r] - a.pkg_base - t * kTile) & (kTile - 1)];
      ks[r] = rh ? rank_of(a, as[r]).x : kNoKey;
    }
#pragma unroll
    for (int r = 0; r < kCountRounds; r++) {
      const uint32_t c = c0 + r * 64;
      if (c >= cnt) break;  // wave-uniform
      const bool v = c + lane < cnt;
      const uint32_t p = ps[r], k = ks[r];
      uint32_t pp, kp;
      entry_before(lane, p, k, prev_p, prev_k, cnt - c, pp, kp);
      const bool same = v && k != kNoKey && pp == p;
      order_bad |= same && kp > k;
      const unsigned long long hb = __ballot(v && !(same && kp == k)), cb = __ballot(v) & ~hb;
      n_multi += uint32_t(__popcll(cb & ((hb << 1) | prev_h)));  // a continuation right behind its head
      n_cont += uint32_t(__popcll(cb));
      const uint32_t last = (cnt - c < 64u ? cnt - c : 64u) - 1;
      prev_h = uint32_t(hb >> last) & 1u;
    }
  }
  if (__ballot(order_bad)) {
    if (lane == 0) atomicOr(a.f.ctl + 3, (unsigned long long)ERR_RH_ORDER);
    return;
  }
  const uint32_t n_mem = n_cont + n_multi;
  uint32_t gbase = 0, mbase = 0;
  if (n_multi) {  // wave-uniform
    unsigned long long got = 0;
    // one word for both counts: the member total stays below 2^32 and never carries into the group
    // half, because members are raw matches of segments inside the capacity and prepare()
    // refuses a match capacity of 2^32 or more
    if (lane == 0) got = atomicAdd(a.f.ctl + kCtlGroups, ((unsigned long long)n_multi << 32) | n_mem);
    gbase = __builtin_amdgcn_readfirstlane(uint32_t(got >> 32));
    mbase = __builtin_amdgcn_readfirstlane(uint32_t(got));
    // guard (never expected: a multi-member group holds two raw matches, the lists are sized from the capacity)
    if (uint64_t(gbase) + n_multi > a.grp_cap || uint64_t(mbase) + n_mem > a.mem_cap) {
      if (lane == 0) atomicOr(a.f.ctl + 3, (unsigned long long)ERR_BOUNDS);
      return;
    }
  }

  // walk 2: representatives, the filter, the compaction
  const uint32_t sev_mask = a.f.sev_mask & 0x1Fu;
  uint32_t kept = 0, gdone = 0, mdone = 0;
  prev_p = 0xFFFFFFFFu;
  prev_k = kNoKey;
  uint32_t p, ad, fr, k, cw;  // the round's entries, loaded under the round before
  k = entry_key(a, pkg, adv, lane, cnt, t, rhp, p, ad, fr);
  cw = !a.filter ? 0u : ad < a.f.n_cls ? uint32_t(a.f.cls[ad]) : kClsUnknown;
  for (uint32_t c = 0; c < cnt; c += 64) {
    const uint32_t i = c + lane;
    const bool v = i < cnt;
    uint32_t np, nad, nfr, pp, kp;
    const uint32_t nk = entry_key(a, pkg, adv, i + 64, cnt, t, rhp, np, nad, nfr);
    const uint32_t ncw = !a.filter ? 0u : nad < a.f.n_cls ? uint32_t(a.f.cls[nad]) : kClsUnknown;
    entry_before(lane, p, k, prev_p, prev_k, cnt - c, pp, kp);
    const bool h = v && (k == kNoKey || pp != p || kp != k);
    // the entry behind the lane's (lane 63: the next round's first), from registers: a head walks
    // ahead only when that entry continues its group, which one group in a hundred does
    const uint32_t dp = __shfl_down(p, 1, 64), dk = __shfl_down(k, 1, 64);
    const uint32_t fp = __shfl(np, 0, 64), fk = __shfl(nk, 0, 64);
    const bool more = k != kNoKey && (lane < 63 ? dp == p && dk == k : fp == p && fk == k);
    uint32_t len = 1, best = RH_NONE, best_r = 0;
    if (h && k != kNoKey) {
      if (fr != RH_NONE) best = ad, best_r = fr;
      for (uint32_t j = i + 1; more && j < cnt && pkg[j] == p; j++) {
        const uint32_t aj = adv[j];
        const uint2 rj = rank_of(a, aj);
        if (rj.x != k) break;
        if (rj.y != RH_NONE && (best == RH_NONE || rj.y > best_r)) best = aj, best_r = rj.y;
        len++;
      }
    }
    bool keep = h;
    if (a.filter) {  // filter.hip filter_mark's predicate (filter.go:113-120) on the merged entry
      const uint32_t status = best != RH_NONE ? kStatusFixed : (cw >> 8) & 31u;
      keep = h && ((sev_mask >> (cw & 0xFFu)) & 1u) && !((a.f.status_mask >> status) & 1u);
    }
    const bool multi = keep && len > 1;
    const unsigned long long mb = __ballot(multi);
    uint32_t rec = best != RH_NONE ? best : ad;
    if (mb) {  // wave-uniform: the round's kept groups of several members take their slots
      uint32_t x = multi ? len : 0u;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= uint32_t(o)) x += y;
      }
      const uint32_t tot = __shfl(x, 63, 64);
      // guard (never expected: walk 1 counted these groups): nothing is written beyond the reservation
      if (gdone + uint32_t(__popcll(mb)) > n_multi || mdone + tot > n_mem) {
        if (lane == 0) atomicOr(a.f.ctl + 3, (unsigned long long)ERR_BOUNDS);
        return;
      }
      if (multi) {
        const uint32_t g = gbase + gdone + uint32_t(__popcll(mb & lt)), mo = mbase + mdone + (x - len);
        a.groups[g] = make_uint4(ad, rec, mo, len);
        for (uint32_t m = 0; m < len; m++) a.members[mo + m] = adv[i + m];
        rec = a.n_adv_recs + g;
      }
      gdone += uint32_t(__popcll(mb));
      mdone += tot;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the round's loads stay above its stores
    const unsigned long long kb = __ballot(keep);
    if (keep) {
      const uint32_t o = kept + uint32_t(__popcll(kb & lt));
      pkg[o] = p;
      adv[o] = rec;
    }
    kept += uint32_t(__popcll(kb));
    p = np, ad = nad, fr = nfr, k = nk, cw = ncw;
  }
  // slots reserved for groups the filter dropped: empty, so the host builds nothing from a stale list
  for (uint32_t s = gdone + lane; s < n_multi; s += 64) a.groups[gbase + s] = make_uint4(0, 0, 0, 0);
  if (lane == 0) {
    a.f.dir[t].count = kept;
    if (a.filter) {
      if (kept) atomicAdd(a.f.ctl + kCtlKept, (unsigned long long)kept);
    } else if (kept != cnt) {
      atomicAdd(a.f.ctl + kCtlMerged, (unsigned long long)(cnt - kept));
    }
  }
}

}  // namespace

void launch_rhmerge(hipStream_t st, const RhMergeArgs& a) {
  if (a.f.t1 <= a.f.t0) return;
  hipLaunchKernelGGL(rhmerge_tiles, dim3((a.f.t1 - a.f.t0 + 3) / 4), dim3(256), 0, st, a);
}

}  // namespace tvm
