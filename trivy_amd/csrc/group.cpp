// Engine groups: one batch sharded over several engines (one per GPU) inside one process.
//
// The layer composes the single-engine C-ABI (capi.cpp): a member is a tvm_engine, a member
// batch a tvm_batch with a package base, and every pass, filter, merge and accessor on a member
// is the stand-alone call.  What lives here is the shard plan (dist.py target_shards in C++),
// the concurrent member adds and passes (one host thread per member, LaneThreads), the two-step
// swap, and the union of the members' ordered lists on one device (tvm_group_csr_into: the order
// kernel with rebased row ends per member, then device copies - the in-process CSRGather).
#include "../../include/trivy_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "capi_hooks.h"
#include "host_par.h"
#include "pool.h"

using namespace tvm;

struct tvm_group {
  std::vector<tvm_engine*> eng;
  std::mutex swap_mu;         // one tvm_group_swap at a time
  std::unique_ptr<LaneThreads> lanes;
};

struct tvm_group_batch {
  tvm_group* g = nullptr;
  std::vector<tvm_batch*> mb;     // one per member (an empty shard's stays unused)
  std::vector<uint64_t> bounds;   // member k holds packages [bounds[k], bounds[k + 1])
  std::vector<size_t> tbounds;    // ... which are targets [tbounds[k], tbounds[k + 1]) of the add
  std::vector<uint64_t> caps;     // match capacity of member k's prepared pipeline
  std::vector<uint64_t> counts;   // tvm_group_status: member k's match count
  uint64_t n = 0;
  int64_t n_cpe_sets = 0;
  bool added = false, prepared = false, uploaded = false;
  bool empty(int k) const { return bounds[size_t(k) + 1] == bounds[size_t(k)]; }
  std::vector<int> members() const {  // the members that hold packages
    std::vector<int> ks;
    for (int k = 0; k < int(mb.size()); k++)
      if (!empty(k)) ks.push_back(k);
    return ks;
  }
};

namespace {

void set_err(char* err, size_t errlen, const std::string& msg) {
  if (!err || errlen == 0) return;
  const size_t n = std::min(errlen - 1, msg.size());
  memcpy(err, msg.data(), n);
  err[n] = 0;
}

// Live groups: tvm_shutdown joins their member threads (nothing of the library's may be left
// running for the process's own teardown).
std::mutex& reg_mu() {
  static std::mutex* m = new std::mutex();
  return *m;
}
std::vector<tvm_group*>& registry() {
  static std::vector<tvm_group*>* r = new std::vector<tvm_group*>();
  return *r;
}

struct Msg {
  char s[512];
  Msg() { s[0] = 0; }
};

// dist.py balanced_shards over per-target weights, in the same float64 arithmetic (the weights
// are integers below 2^53, so every sum is exact): boundary k = the first target at which the
// running sum reaches total * k / shards, plus one, clamped to be monotone.
void balanced(const std::vector<double>& w, int shards, std::vector<size_t>& tb) {
  const size_t T = w.size();
  tb.assign(size_t(shards) + 1, 0);
  if (T == 0) return;
  std::vector<double> c(T);
  double run = 0;
  for (size_t t = 0; t < T; t++) c[t] = run += w[t];
  const double total = c[T - 1];
  for (int k = 1; k < shards; k++) {
    const double x = total * double(k) / double(shards);
    tb[size_t(k)] = size_t(std::lower_bound(c.begin(), c.end(), x) - c.begin()) + 1;
  }
  tb[size_t(shards)] = T;
  for (int k = 1; k <= shards; k++) tb[size_t(k)] = std::min(std::max(tb[size_t(k)], tb[size_t(k) - 1]), T);
}

int plan(size_t n_targets, const uint64_t* target_end, const uint32_t* pkg_weight, int n_shards, uint64_t* bounds_out,
         std::vector<size_t>* tbounds_out = nullptr) {
  if (n_shards < 1 || !bounds_out || (n_targets && !target_end)) return TVM_EINVAL;
  for (size_t t = 1; t < n_targets; t++)
    if (target_end[t] < target_end[t - 1]) return TVM_EINVAL;
  std::vector<double> tw(n_targets);
  for (size_t t = 0; t < n_targets; t++) {
    const uint64_t p0 = t ? target_end[t - 1] : 0, p1 = target_end[t];
    if (!pkg_weight) {
      tw[t] = double(p1 - p0);
      continue;
    }
    uint64_t s = 0;
    for (uint64_t p = p0; p < p1; p++) s += pkg_weight[p];
    tw[t] = double(s);
  }
  std::vector<size_t> tb;
  balanced(tw, n_shards, tb);
  for (int k = 0; k <= n_shards; k++) bounds_out[k] = tb[size_t(k)] ? target_end[tb[size_t(k)] - 1] : 0;
  if (tbounds_out) tbounds_out->swap(tb);
  return TVM_OK;
}

// TVM_GROUP_PLAN_ROWS: per package its predicted advisory rows + 1, from the host index (the
// lookup behind tvm_db_rows_many), per run of equal-bucket targets, cut into pieces for the
// host threads.
bool row_weights(const tvm_db* db, size_t n_targets, const tvm_str* buckets, const uint64_t* target_end, const char* arena,
                 const uint64_t* name_off, const uint32_t* name_len, std::vector<uint32_t>& w) {
  struct Piece {
    size_t run;
    uint64_t p0, p1;
  };
  const uint64_t n = n_targets ? target_end[n_targets - 1] : 0;
  w.assign(n, 0);
  std::vector<std::string> run_bucket;
  std::vector<Piece> pieces;
  constexpr uint64_t kPiece = 1 << 14;
  for (size_t t = 0; t < n_targets;) {
    size_t u = t + 1;
    while (u < n_targets && buckets[u].n == buckets[t].n &&
           (buckets[t].n == 0 || memcmp(buckets[u].p, buckets[t].p, buckets[t].n) == 0))
      u++;
    run_bucket.emplace_back(buckets[t].p ? buckets[t].p : "", buckets[t].p ? buckets[t].n : 0);
    const uint64_t p0 = t ? target_end[t - 1] : 0, p1 = target_end[u - 1];
    for (uint64_t p = p0; p < p1; p += kPiece) pieces.push_back({run_bucket.size() - 1, p, std::min(p + kPiece, p1)});
    t = u;
  }
  std::atomic<bool> bad{false};
  WorkerPool::get().parallel_for(pieces.size(), [&](size_t i) {
    const Piece& pc = pieces[i];
    if (tvm_db_rows_many(db, run_bucket[pc.run].c_str(), size_t(pc.p1 - pc.p0), arena, name_off + pc.p0,
                         name_len + pc.p0, w.data() + pc.p0))
      bad.store(true);
  });
  if (bad.load()) return false;
  for (uint64_t p = 0; p < n; p++) w[p] = w[p] == 0xFFFFFFFFu ? w[p] : w[p] + 1;
  return true;
}

}  // namespace

namespace tvm {
namespace capi_hooks {
void shutdown_groups() {
  std::lock_guard<std::mutex> g(reg_mu());
  for (tvm_group* gr : registry())
    if (gr->lanes) gr->lanes->stop();
}
}  // namespace capi_hooks
}  // namespace tvm

extern "C" {

// ---- group ------------------------------------------------------------------------------------

tvm_group* tvm_group_open(tvm_db* db, const int* devices, int n, char* err, size_t errlen) {
  if (n < 1 || n > 8 || !devices) {
    set_err(err, errlen, "tvm_group_open: 1 to 8 devices");
    return nullptr;
  }
  for (int k = 0; k < n; k++)
    if (devices[k] < 0) {
      set_err(err, errlen, "tvm_group_open: negative device");
      return nullptr;
    }
  std::unique_ptr<tvm_group> g(new tvm_group());
  for (int k = 0; k < n; k++) {
    tvm_engine* e = tvm_engine_open(db, devices[k], err, errlen);  // the tables once per member
    if (!e) {
      for (tvm_engine* o : g->eng) tvm_engine_close(o);
      return nullptr;
    }
    g->eng.push_back(e);
  }
  g->lanes.reset(new LaneThreads(n));
  std::lock_guard<std::mutex> lk(reg_mu());
  registry().push_back(g.get());
  return g.release();
}

void tvm_group_close(tvm_group* g) {
  if (!g) return;
  {
    std::lock_guard<std::mutex> lk(reg_mu());
    auto& r = registry();
    r.erase(std::remove(r.begin(), r.end(), g), r.end());
  }
  g->lanes.reset();  // joins the member threads
  for (tvm_engine* e : g->eng) tvm_engine_close(e);
  delete g;
}

int tvm_group_size(const tvm_group* g) { return g ? int(g->eng.size()) : 0; }

tvm_engine* tvm_group_engine(tvm_group* g, int k) {
  return g && k >= 0 && k < int(g->eng.size()) ? g->eng[size_t(k)] : nullptr;
}

int tvm_group_swap(tvm_group* g, tvm_db* db, char* err, size_t errlen) {
  if (!g || !capi_hooks::db_finalized(db)) return TVM_EINVAL;
  std::lock_guard<std::mutex> one(g->swap_mu);
  const size_t n = g->eng.size();
  std::vector<capi_hooks::SwapTables> fresh(n);
  std::string msg;
  for (size_t k = 0; k < n; k++)  // every member's tables first: a failure swaps nobody
    if (!capi_hooks::swap_build(g->eng[k], db, fresh[k], msg)) {
      for (size_t j = 0; j < k; j++) capi_hooks::swap_discard(g->eng[j], fresh[j]);
      set_err(err, errlen, msg);
      return TVM_EDEVICE;
    }
  for (size_t k = 0; k < n; k++) capi_hooks::swap_commit(g->eng[k], db, fresh[k]);
  return TVM_OK;
}

int tvm_group_plan_host(size_t n_targets, const uint64_t* target_end, const uint32_t* pkg_weight, int n_shards,
                        uint64_t* bounds_out) {
  return plan(n_targets, target_end, pkg_weight, n_shards, bounds_out);
}

// ---- group batch ------------------------------------------------------------------------------

tvm_group_batch* tvm_group_batch_new(tvm_group* g) {
  if (!g) return nullptr;
  auto* gb = new tvm_group_batch();
  gb->g = g;
  const size_t n = g->eng.size();
  for (size_t k = 0; k < n; k++) gb->mb.push_back(tvm_batch_new());
  gb->bounds.assign(n + 1, 0);
  gb->caps.assign(n, 0);
  gb->counts.assign(n, 0);
  return gb;
}

void tvm_group_batch_free(tvm_group_batch* gb) {
  if (!gb) return;
  for (tvm_batch* b : gb->mb) tvm_batch_free(b);
  delete gb;
}

int64_t tvm_group_batch_cpe_set(tvm_group_batch* gb, const tvm_str* content_sets, size_t n, tvm_str nvr) {
  if (!gb || gb->added) return -1;
  int64_t id = -1;
  for (size_t k = 0; k < gb->mb.size(); k++) {  // the same order on every member: the same id
    const int64_t i = tvm_batch_cpe_set(gb->mb[k], gb->g->eng[k], content_sets, n, nvr);
    if (i < 0 || (k && i != id)) return -1;
    id = i;
  }
  gb->n_cpe_sets = id + 1;
  return id;
}

int tvm_group_batch_add_targets(tvm_group_batch* gb, uint32_t plan_mode, size_t n_targets, const tvm_str* buckets,
                                const uint32_t* target_flags, const uint64_t* target_end, const char* arena,
                                const uint64_t* name_off, const uint32_t* name_len, const uint64_t* ver_off,
                                const uint32_t* ver_len, const tvm_attr_cols* attrs) {
  if (!gb || gb->added || (plan_mode != TVM_GROUP_PLAN_PACKAGES && plan_mode != TVM_GROUP_PLAN_ROWS) ||
      (n_targets && (!buckets || !target_end)))
    return TVM_EINVAL;
  const uint64_t n = n_targets ? target_end[n_targets - 1] : 0;
  if (n >= (uint64_t(1) << 32) || (n && (!arena || !name_off || !name_len || !ver_off || !ver_len))) return TVM_EINVAL;
  // the single-batch call's refusals (capi.cpp add_targets_bulk), before any member is touched
  const uint32_t known = TVM_ATTR_ARCH | TVM_ATTR_KSPLICE | TVM_ATTR_CPESET;
  uint32_t any_flags = 0;
  for (size_t t = 0; t < n_targets; t++) {
    if (t && target_end[t] < target_end[t - 1]) return TVM_EINVAL;
    const uint32_t f = target_flags ? target_flags[t] : 0u;
    if ((f & ~known) || ((f & TVM_ATTR_KSPLICE) && (f & TVM_ATTR_CPESET))) return TVM_EINVAL;
    any_flags |= f;
  }
  if (((any_flags & TVM_ATTR_ARCH) && (!attrs || !attrs->arch_off || !attrs->arch_len)) ||
      ((any_flags & TVM_ATTR_CPESET) && (!attrs || !attrs->cpe_set)))
    return TVM_EINVAL;
  if (any_flags & TVM_ATTR_CPESET)
    for (size_t t = 0; t < n_targets; t++)
      if (target_flags[t] & TVM_ATTR_CPESET)
        for (uint64_t p = t ? target_end[t - 1] : 0; p < target_end[t]; p++)
          if (int64_t(attrs->cpe_set[p]) >= gb->n_cpe_sets) return TVM_EINVAL;
  const int N = int(gb->mb.size());
  std::vector<uint32_t> w;
  if (plan_mode == TVM_GROUP_PLAN_ROWS && N > 1) {
    // The probe reads the host index of the tables member 0 serves, under member 0's shared lock
    // like any other call on that engine: tvm_group_swap (swap_commit takes the lock exclusively)
    // returns only after a probe in flight has left the old DB, so the caller may free it.
    bool ok = false;
    capi_hooks::with_engine_db(gb->g->eng[0], [&](const tvm_db* db) {
      ok = row_weights(db, n_targets, buckets, target_end, arena, name_off, name_len, w);
    });
    if (!ok) return TVM_EINVAL;
  }
  if (plan(n_targets, target_end, w.empty() ? nullptr : w.data(), N, gb->bounds.data(), &gb->tbounds)) return TVM_EINVAL;
  gb->added = true;
  gb->n = n;
  std::vector<int> rc(size_t(N), 0);
  // member k: its slice of the caller's columns, its targets' ends counted from its first package
  gb->g->lanes->run(gb->members(), [&](int k) {
    const uint64_t p0 = gb->bounds[size_t(k)], p1 = gb->bounds[size_t(k) + 1];
    const size_t t0 = gb->tbounds[size_t(k)], t1 = gb->tbounds[size_t(k) + 1];
    std::vector<uint64_t> te(target_end + t0, target_end + t1);
    for (uint64_t& x : te) x -= p0;
    tvm_attr_cols cols{nullptr, nullptr, nullptr};
    if (attrs) {
      cols.arch_off = attrs->arch_off ? attrs->arch_off + p0 : nullptr;
      cols.arch_len = attrs->arch_len ? attrs->arch_len + p0 : nullptr;
      cols.cpe_set = attrs->cpe_set ? attrs->cpe_set + p0 : nullptr;
    }
    const int64_t first =
        tvm_batch_add_targets_attrs(gb->mb[size_t(k)], gb->g->eng[size_t(k)], t1 - t0, buckets + t0,
                                    target_flags ? target_flags + t0 : nullptr, te.data(), arena, name_off + p0,
                                    name_len + p0, ver_off + p0, ver_len + p0, attrs ? &cols : nullptr);
    if (first != 0 || tvm_batch_size(gb->mb[size_t(k)]) != int64_t(p1 - p0) ||
        tvm_batch_set_package_base(gb->mb[size_t(k)], uint32_t(p0)))
      rc[size_t(k)] = TVM_EINVAL;
  });
  for (int k = 0; k < N; k++)
    if (rc[size_t(k)]) return rc[size_t(k)];  // stale tables (a swap since tvm_group_batch_new), or out of memory
  return TVM_OK;
}

int64_t tvm_group_batch_size(const tvm_group_batch* gb) { return gb ? int64_t(gb->n) : 0; }

int tvm_group_batch_shards(const tvm_group_batch* gb, uint64_t* bounds) {
  if (!gb || !bounds) return TVM_EINVAL;
  std::copy(gb->bounds.begin(), gb->bounds.end(), bounds);
  return TVM_OK;
}

tvm_batch* tvm_group_batch_member(tvm_group_batch* gb, int k) {
  if (!gb || k < 0 || k >= int(gb->mb.size()) || !gb->added || gb->empty(k)) return nullptr;
  return gb->mb[size_t(k)];
}

// ---- pipelined group pass ---------------------------------------------------------------------

int tvm_group_pipeline_prepare(tvm_group_batch* gb, uint64_t match_cap, const uint64_t* member_caps,
                               uint32_t chunk_packages, uint32_t flags, char* err, size_t errlen) {
  if (!gb || !gb->added) return TVM_EINVAL;
  gb->prepared = false;
  const std::vector<int> ks = gb->members();
  for (int k : ks) {
    const uint64_t cap = member_caps ? member_caps[k] : match_cap;
    const int rc = tvm_pipeline_prepare(gb->g->eng[size_t(k)], gb->mb[size_t(k)], cap, chunk_packages, flags, err, errlen);
    if (rc) {
      for (int j : ks) capi_hooks::pipeline_drop(gb->mb[size_t(j)]);  // no member stays prepared
      return rc;
    }
    gb->caps[size_t(k)] = cap;
  }
  gb->prepared = true;
  return TVM_OK;
}

int tvm_group_pipeline_set_filter(tvm_group_batch* gb, const tvm_filter_opts* o, char* err, size_t errlen) {
  if (!gb || !gb->added) return TVM_EINVAL;
  if (!gb->prepared) {
    set_err(err, errlen, "tvm_pipeline_set_filter: tvm_pipeline_prepare the batch first");
    return TVM_EINVAL;
  }
  const std::vector<int> ks = gb->members();
  for (int k : ks) {
    const int rc = tvm_pipeline_set_filter(gb->g->eng[size_t(k)], gb->mb[size_t(k)], o, err, errlen);
    if (rc) {  // one filter for the whole batch, or none
      for (int j : ks) (void)tvm_pipeline_set_filter(gb->g->eng[size_t(j)], gb->mb[size_t(j)], nullptr, nullptr, 0);
      return rc;
    }
  }
  return TVM_OK;
}

int tvm_group_pipeline_run(tvm_group_batch* gb, uint64_t* n_matches, int64_t* err_pkg, double* ms,
                           uint64_t* member_matches, char* err, size_t errlen) {
  if (!gb || !gb->added || !gb->prepared) return TVM_EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t N = gb->mb.size();
  std::vector<uint64_t> cnt(N, 0);
  std::vector<int64_t> ep(N, -1);
  std::vector<int> rc(N, 0);
  std::vector<Msg> msg(N);
  // one host thread per member for the length of its pass; tvm_pipeline_run selects the device
  gb->g->lanes->run(gb->members(), [&](int k) {
    const size_t i = size_t(k);
    rc[i] = tvm_pipeline_run(gb->g->eng[i], gb->mb[i], &cnt[i], &ep[i], nullptr, msg[i].s, sizeof(msg[i].s));
  });
  uint64_t total = 0;
  int64_t first_ep = -1;
  int fail = -1, over = -1;
  for (size_t k = 0; k < N; k++) {
    const bool overflow = rc[k] == TVM_EINVAL && cnt[k] > gb->caps[k];
    if (rc[k] && !overflow) {
      if (fail < 0) fail = int(k);  // every member was left to finish; the first error is the call's
      continue;
    }
    if (overflow && over < 0) over = int(k);
    total += cnt[k];
    // a member's poisoned package is counted from its own first package: make it global
    if (ep[k] >= 0) {
      const int64_t gp = ep[k] + int64_t(gb->bounds[k]);
      if (first_ep < 0 || gp < first_ep) first_ep = gp;
    }
    if (member_matches) member_matches[k] = cnt[k];
  }
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (fail >= 0) {
    set_err(err, errlen, msg[size_t(fail)].s);
    return rc[size_t(fail)];
  }
  if (n_matches) *n_matches = total;
  if (err_pkg) *err_pkg = first_ep;
  if (over >= 0) {
    set_err(err, errlen, "tvm_group_pipeline_run: member " + std::to_string(over) +
                             "'s match buffer is too small (prepare again with member_caps = member_matches)");
    return TVM_EINVAL;
  }
  return TVM_OK;
}

// ---- device-resident group pass and the union lists on one device -----------------------------

int tvm_group_upload(tvm_group_batch* gb, uint64_t match_cap, const uint64_t* member_caps, char* err, size_t errlen) {
  if (!gb || !gb->added) return TVM_EINVAL;
  gb->uploaded = false;
  for (int k : gb->members()) {
    const uint64_t cap = member_caps ? member_caps[k] : match_cap;
    // (the upload's capacity lives in the member batch; `caps` stays the prepared pipeline's)
    const int rc = tvm_batch_upload(gb->g->eng[size_t(k)], gb->mb[size_t(k)], cap, err, errlen);
    if (rc) return rc;
  }
  gb->uploaded = true;
  return TVM_OK;
}

int tvm_group_launch(tvm_group_batch* gb, char* err, size_t errlen) {
  if (!gb || !gb->uploaded) return TVM_EINVAL;
  for (int k : gb->members()) {  // asynchronous: every member's pass is in flight when this returns
    const int rc = tvm_match_launch(gb->g->eng[size_t(k)], gb->mb[size_t(k)], err, errlen);
    if (rc) return rc;
  }
  return TVM_OK;
}

int tvm_group_status(tvm_group_batch* gb, uint64_t* n_matches, int64_t* err_pkg, uint64_t* err_bits,
                     uint64_t* member_matches) {
  if (!gb || !gb->uploaded) return TVM_EINVAL;
  uint64_t total = 0, bits = 0;
  int64_t first_ep = -1;
  std::fill(gb->counts.begin(), gb->counts.end(), 0);
  for (int k : gb->members()) {
    uint64_t n = 0, b = 0;
    int64_t ep = -1;
    const int rc = tvm_match_status(gb->g->eng[size_t(k)], gb->mb[size_t(k)], &n, &ep, &b);
    if (rc) return rc;
    gb->counts[size_t(k)] = n;
    total += n;
    bits |= b;
    if (ep >= 0) {
      const int64_t gp = ep + int64_t(gb->bounds[size_t(k)]);
      if (first_ep < 0 || gp < first_ep) first_ep = gp;
    }
  }
  if (member_matches) std::copy(gb->counts.begin(), gb->counts.end(), member_matches);
  if (n_matches) *n_matches = total;
  if (err_pkg) *err_pkg = first_ep;
  if (err_bits) *err_bits = bits;
  return TVM_OK;
}

int tvm_group_csr_into(tvm_group_batch* gb, int root, void* csr_adv_dev, void* row_end_dev, uint64_t cap,
                       uint64_t* n_out, char* err, size_t errlen) {
  if (n_out) *n_out = 0;
  if (!gb || !gb->uploaded || root < 0 || root >= int(gb->mb.size())) return TVM_EINVAL;
  uint64_t total = 0;
  int rc = tvm_group_status(gb, &total, nullptr, nullptr, nullptr);
  if (rc) return rc;
  if (n_out) *n_out = total;
  const std::vector<int> ks = gb->members();
  for (int k : ks)  // an overflowed member pass, or a merged list (as tvm_match_order_into)
    if (capi_hooks::order_refusal(gb->mb[size_t(k)], gb->counts[size_t(k)])) return TVM_EINVAL;
  if (total >= (uint64_t(1) << 31)) {
    set_err(err, errlen, "tvm_group_csr_into: row ends are 32-bit: gather below 2^31 matches at a time");
    return TVM_EINVAL;
  }
  if (total > cap || (gb->n && !row_end_dev) || (total && !csr_adv_dev)) return TVM_EINVAL;
  const int root_dev = capi_hooks::engine_device(gb->g->eng[size_t(root)]);
  struct Part {
    int k, dev;
    void *adv = nullptr, *re = nullptr;
  };
  std::vector<Part> parts;
  std::string msg;
  uint64_t a0 = 0;
  rc = TVM_OK;
  for (int k : ks) {
    tvm_engine* e = gb->g->eng[size_t(k)];
    tvm_batch* b = gb->mb[size_t(k)];
    const uint64_t nk = gb->counts[size_t(k)], p0 = gb->bounds[size_t(k)], np = gb->bounds[size_t(k) + 1] - p0;
    Part pt;
    pt.k = k;
    pt.dev = capi_hooks::engine_device(e);
    // group-owned buffers on the member's device, sized to the member's own counts
    pt.adv = pool_device_get(pt.dev, size_t(std::max<uint64_t>(nk, 1)) * 4, "group csr_adv", msg);
    pt.re = pt.adv ? pool_device_get(pt.dev, size_t(np) * 4, "group row_end", msg) : nullptr;
    parts.push_back(pt);
    if (!pt.adv || !pt.re) {
      set_err(err, errlen, msg);
      rc = TVM_EDEVICE;
      break;
    }
    // the order kernel stores the member's row ends already rebased by a0; copies do the rest
    rc = capi_hooks::order_into(e, b, pt.adv, pt.re, std::max<uint64_t>(nk, 1), nk, uint32_t(a0), false, err, errlen);
    if (!rc) rc = capi_hooks::copy_from_engine(e, static_cast<char*>(csr_adv_dev) + a0 * 4, root_dev, pt.adv, size_t(nk) * 4, err, errlen);
    if (!rc) rc = capi_hooks::copy_from_engine(e, static_cast<char*>(row_end_dev) + p0 * 4, root_dev, pt.re, size_t(np) * 4, err, errlen);
    if (rc) break;
    a0 += nk;
  }
  // every member's stream is drained before its buffers go back (also after a failure: what was
  // enqueued still runs), the root's last: the union is complete when this returns
  auto drain = [&](int k) {
    const int s = tvm_engine_sync(gb->g->eng[size_t(k)], rc ? nullptr : err, rc ? 0 : errlen);
    if (s && !rc) rc = s;
  };
  for (const Part& pt : parts)
    if (pt.k != root) drain(pt.k);
  drain(root);
  for (const Part& pt : parts) {
    if (pt.adv) pool_device_put(pt.dev, pt.adv);
    if (pt.re) pool_device_put(pt.dev, pt.re);
  }
  return rc;
}

}  // extern "C"
