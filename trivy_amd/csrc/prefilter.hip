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
#include "prefilter_tile.h"
#include "vulninfo.h"

#include <algorithm>

namespace tvm {

namespace {

// One wavefront per tile, four tiles per workgroup (prefilter_tile.h: the tile's compaction and
// why it is safe in place).
__global__ __launch_bounds__(256) void prefilter_tiles(PrefilterArgs a) {
  const uint32_t lane = threadIdx.x & 63, t = a.t0 + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= a.t1) return;  // whole wavefronts
  prefilter_tile_wave(a, t, lane);
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
