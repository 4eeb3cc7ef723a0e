// What group.cpp needs from capi.cpp beyond the C-ABI itself: the engine swap in its two
// steps, the order kernel with rebased row ends, and the hook tvm_shutdown calls.  The
// handles stay opaque here (their layouts live in capi.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>

#include "../../include/trivy_amd.h"

namespace tvm {
class Engine;
class FillEngine;

namespace capi_hooks {

// Fresh tables for an engine's device, built while the engine keeps serving calls.
struct SwapTables {
  Engine* eng = nullptr;
  FillEngine* fill = nullptr;
};
bool swap_build(tvm_engine* e, tvm_db* db, SwapTables& out, std::string& msg);  // false: nothing left in `out`
void swap_commit(tvm_engine* e, tvm_db* db, SwapTables& t);  // takes the exclusive lock; cannot fail
void swap_discard(tvm_engine* e, SwapTables& t);
int engine_device(const tvm_engine* e);
// f(the DB the engine serves) under the engine's shared lock, as every single-engine call reads
// it: a swap of the engine waits until f has returned.
void with_engine_db(tvm_engine* e, const std::function<void(const tvm_db*)>& f);
bool db_finalized(const tvm_db* db);

// tvm_match_order_into on a batch whose match count the caller has read (n, at most the
// batch's match capacity and at most cap): the order kernel with row_base added to every row
// end, enqueued on the engine's stream.  sync = false leaves the stream running.  The batch's
// own refusals (merged list, stale tables) hold as in tvm_match_order_into.
int order_into(tvm_engine* e, tvm_batch* b, void* csr_adv_dev, void* row_end_dev, uint64_t cap, uint64_t n,
               uint32_t row_base, bool sync, char* err, size_t errlen);
// hipMemcpy[Peer]Async of `bytes` from src (on e's device) to dst on device dst_device, on e's
// stream, behind whatever e has enqueued.
int copy_from_engine(tvm_engine* e, void* dst, int dst_device, const void* src, size_t bytes, char* err,
                     size_t errlen);
// What the batch's last device-resident pass may hand out: 0, or TVM_EINVAL when its list is
// the merged one (tvm_match_redhat_merge) or n exceeds its match capacity.
int order_refusal(const tvm_batch* b, uint64_t n);

// Releases the batch's prepared pipeline, if any (a group prepare that failed on another member).
void pipeline_drop(tvm_batch* b);

// Joins the worker threads of every live engine group (tvm_shutdown; group.cpp).
void shutdown_groups();

}  // namespace capi_hooks
}  // namespace tvm
