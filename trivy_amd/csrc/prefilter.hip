// Severity / status filter inside the pipelined pass (gfx950): the first two per-finding tests of
// filterVulnerabilities (pkg/result/filter.go:108-120) applied to a chunk's match segments in
// HBM, before the result move carries them over the link.
//
// Both tests read only what FillInfo decides from the advisory (vulninfo.h adv_items ->
// fill_pair_severity and the decision's status), so every DB advisory has one class word
// `severity index | status << 8` (the side word fill_pairs_kernel hands the batch filter),
// built once per table generation by running FillInfo over the identity list 0..n_advs-1.
// A finding is then tested with one 2-byte gather, and a tile's segment is compacted in place;
// the result move (engine.h copy_out_tiles) reads only dir[].count, pkg and adv, so its
// offsets, row ends and 16-byte realignment come out for the survivors.  Integer work bound by
// memory latency; no MFMA.
#include "pipeline.h"
#include "vulninfo.h"

#include <algorithm>

namespace tvm {

namespace {

// An advisory index beyond the table (never expected): what fill_pairs_kernel decides for it,
// severity UNKNOWN and StatusAffected.
constexpr uint32_t kClsUnknown = 0u | (2u << 8);
constexpr int kPreRounds = 4;  // 64-entry rounds loaded before the first is used

// One wavefront per tile, four tiles per workgroup.  The wave walks its tile's segment
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
__global__ __launch_bounds__(256) void prefilter_tiles(PrefilterArgs a) {
  const uint32_t lane = threadIdx.x & 63, t = a.t0 + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= a.t1) return;  // whole wavefronts
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

// adv[i] = i and the list's length, for FillEngine::launch_pairs over every advisory
__global__ __launch_bounds__(256) void identity_kernel(uint32_t* adv, unsigned long long* n_dev, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *n_dev = n;
  if (i < n) adv[i] = i;
}

__global__ __launch_bounds__(256) void narrow_kernel(const uint2* side, uint16_t* cls, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) cls[i] = uint16_t(side[i].y);
}

bool hip_ok(hipError_t e, const char* what, std::string& err) {
  if (e == hipSuccess) return true;
  err = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}

}  // namespace

void launch_prefilter(hipStream_t st, const PrefilterArgs& a) {
  if (a.t1 <= a.t0) return;
  hipLaunchKernelGGL(prefilter_tiles, dim3((a.t1 - a.t0 + 3) / 4), dim3(256), 0, st, a);
}

uint16_t* build_class_table(FillEngine& fill, hipStream_t st, std::string& err) {
  const uint32_t n = fill.dev().n_advs;
  void* cls = nullptr;
  if (!hip_ok(hipSetDevice(fill.device()), "hipSetDevice", err) ||
      !hip_ok(hipMalloc(&cls, std::max<size_t>(n, 1) * sizeof(uint16_t)), "hipMalloc(advisory classes)", err))
    return nullptr;
  if (n == 0) return static_cast<uint16_t*>(cls);
  // scratch: the list's length (16 bytes), the decisions, the side words, the identity list
  uint8_t* tmp = nullptr;
  const size_t o_out = 16, o_side = o_out + size_t(n) * sizeof(uint4), o_adv = o_side + size_t(n) * sizeof(uint2);
  bool ok = hip_ok(hipMalloc(reinterpret_cast<void**>(&tmp), o_adv + size_t(n) * 4), "hipMalloc(advisory classes scratch)", err);
  if (ok) {
    auto* n_dev = reinterpret_cast<unsigned long long*>(tmp);
    auto* adv = reinterpret_cast<uint32_t*>(tmp + o_adv);
    auto* side = reinterpret_cast<uint2*>(tmp + o_side);
    const uint32_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(identity_kernel, dim3(blocks), dim3(256), 0, st, adv, n_dev, n);
    ok = hip_ok(hipGetLastError(), "advisory classes: identity launch", err) &&
         fill.launch_pairs(adv, nullptr, n_dev, n, reinterpret_cast<uint4*>(tmp + o_out), side, st, err);
    if (ok) {
      hipLaunchKernelGGL(narrow_kernel, dim3(blocks), dim3(256), 0, st, side, static_cast<uint16_t*>(cls), n);
      ok = hip_ok(hipGetLastError(), "advisory classes: narrow launch", err);
    }
    ok = hip_ok(hipStreamSynchronize(st), "advisory classes", err) && ok;
  }
  if (tmp) (void)hipFree(tmp);
  if (!ok) {
    (void)hipFree(cls);
    return nullptr;
  }
  return static_cast<uint16_t*>(cls);
}

}  // namespace tvm
