// libvdf_nova.so, part 2a: the walk window (trace_walks.hpp) -- the job, its buffers, the spare and the side queue behind the device
// traces of vdf_circuits and vdf_custom_chain.
#include "nova_internal.hpp"

namespace vdfnova {
void walk_slice(uint64_t every, uint64_t launch_rounds, uint64_t done, uint64_t budget, uint64_t* rounds, uint64_t* top, int* last) {
  uint64_t now = std::min(every - done, launch_rounds ? launch_rounds : 1024);   // 1,024 rounds hold a queue for about a millisecond
  if (budget) now = std::min(now, budget);
  *rounds = now;
  *top = every - done;
  *last = done + now == every;
}

bool TraceWalks::covers(size_t first, size_t count) const {
  if (!job) return false;
  const auto it = std::lower_bound(job->steps.begin(), job->steps.end(), first);
  return it != job->steps.end() && *it - first < count;
}
void TraceWalks::scratch_free() {
  if (s.d_walk) vdf_dev_free(side, s.d_walk);
  if (s.d_expect) vdf_dev_free(side, s.d_expect);
  if (s.h_ok) vdf_host_free(side, s.h_ok);
  s = WalkScratch();
}
int TraceWalks::scratch_ensure(size_t walks, size_t entry_bytes) {
  if (s.walks >= walks) return VDF_OK;
  scratch_free();
  if (vdf_dev_alloc(side, walks * entry_bytes, &s.d_walk) != VDF_OK || vdf_dev_alloc(side, walks * entry_bytes, &s.d_expect) != VDF_OK ||
      vdf_host_alloc(side, walks * sizeof(int32_t), (void**)&s.h_ok) != VDF_OK) {
    const int rc = fail(VDF_ERR_OOM, std::string("walk buffers: ") + vdf_last_error(side));
    scratch_free();
    return rc;
  }
  s.walks = walks;
  return VDF_OK;
}
void TraceWalks::release(size_t first, size_t count, bool park) {
  for (size_t k = first; k < first + count; ++k) {
    TraceSlot& t = owner->slot(k);
    if (!t.block) continue;
    if (park && t.block.use_count() == 1) spare = std::move(t.block);
    t = TraceSlot();
  }
}
int TraceWalks::enqueue(uint64_t budget) {
  WalkJob* j = job.get();
  while (j->done < j->every) {
    uint64_t now, top;
    int last;
    walk_slice(j->every, j->launch_rounds, j->done, budget, &now, &top, &last);
    { int rc = owner->launch(side, *j, s, now, top, last); if (rc != VDF_OK) return rc; }
    j->done += now;
    if (budget && (budget -= now) == 0) break;
  }
  return VDF_OK;
}
int TraceWalks::resolve(int* bad, size_t bad_first, size_t bad_count) {
  WalkJob* j = job.get();
  if (!j) return VDF_OK;
  int rc = enqueue(0);
  if (rc == VDF_OK) rc = owner->finish(side, *j, s);
  if (rc == VDF_OK && (rc = vdf_ctx_sync(side)) != VDF_OK) fail(rc, std::string("vdf_ctx_sync: ") + vdf_last_error(side));
  if (rc != VDF_OK) vdf_ctx_sync(side);
  owner->unstage();                                                     // the uploads have run
  if (rc != VDF_OK) {                                                   // a device failure: none of these traces can be trusted
    for (size_t k : j->steps) lose(k);
    job.reset();
    return rc;
  }
  size_t first_bad = (size_t)-1, bad_walk = 0;
  for (size_t li = 0; li < j->steps.size(); ++li) {
    size_t miss = (size_t)-1;                                           // the step's first walk that missed
    for (size_t m = j->step_walks; m-- > 0;)
      if (s.h_ok[li * j->step_walks + m] != 1) miss = m;
    if (miss == (size_t)-1) continue;
    const size_t k = j->steps[li];
    lose(k);
    if (first_bad == (size_t)-1) { first_bad = k; bad_walk = miss; }
    if (bad && k >= bad_first && k - bad_first < bad_count) bad[k - bad_first] = 1;
  }
  job.reset();                                                          // (its buffers stay: scratch_free)
  if (first_bad != (size_t)-1) return fail(VDF_ERR_BAD_ARG, owner->missed(first_bad, bad_walk));
  return VDF_OK;
}
int TraceWalks::pump(size_t k, size_t lead) {
  const WalkJob* j = job.get();
  if (!j || j->done >= j->every) return VDF_OK;
  const size_t wanted_at = j->steps[0] - std::min(lead, j->steps[0]);
  const uint64_t calls = wanted_at > k ? wanted_at - k : 1, left = j->every - j->done;
  return enqueue((left + calls - 1) / calls);
}
int TraceWalks::begin(vdf_ctx* ctx, std::vector<size_t> steps, int wait, uint64_t launch_rounds, int pending, int* bad, size_t bad_first,
                      size_t bad_count) {
  if (home && vdf_ctx_device(home) != vdf_ctx_device(ctx)) return fail(VDF_ERR_BAD_ARG, std::string("the ") + owner->whose + " traces live on another device");
  home = ctx;
  if (steps.empty()) return pending;
  if (!side) {
    const int dev = vdf_ctx_device(ctx);
    if (vdf_ctx_create_pooled(&dev, 1, VDF_QUEUE_SIDE, &side) != VDF_OK) return fail(VDF_ERR_DEVICE, std::string("walk context: ") + vdf_last_error(nullptr));
    HIPCALL(side, vdf_ctx_set_async(side, 1));
  }
  std::unique_ptr<WalkJob> j(new WalkJob());
  j->steps = std::move(steps);
  j->launch_rounds = launch_rounds;
  owner->shape(j->steps[0], j.get());
  const size_t n = j->steps.size();
  j->walks = n * j->step_walks;
  if (n > (~(uint64_t)0 >> 1) / j->trace_bytes) return fail(VDF_ERR_OOM, "the traces do not fit");
  // a windowed prover's spare allocation, when it is exactly this size; anything else is asked of the device
  if (spare && spare.use_count() == 1 && spare->ctx == ctx && spare->bytes == n * j->trace_bytes) j->block = std::move(spare);
  spare.reset();
  if (!j->block) {
    j->block = std::shared_ptr<TraceBlock>(new TraceBlock{ctx, n * j->trace_bytes});
    const std::string what = "the traces of " + std::to_string(n) + " " + owner->noun;
    size_t free_bytes = 0;                         // asked first: an allocation beyond the free memory may be granted and fail later
    HIPCALL(ctx, vdf_dev_mem_info(ctx, &free_bytes, nullptr));
    if (j->block->bytes + j->walks * 2 * j->entry_bytes > free_bytes)
      return fail(VDF_ERR_OOM, what + " (" + std::to_string(j->block->bytes) + " bytes) do not fit the device's free memory (" + std::to_string(free_bytes) + " bytes)");
    if (vdf_dev_alloc(ctx, j->block->bytes, &j->block->d) != VDF_OK) {
      j->block->d = nullptr;
      return fail(VDF_ERR_OOM, what + " do not fit: " + vdf_last_error(ctx));
    }
  }
  { int rc = scratch_ensure(j->walks, j->entry_bytes); if (rc != VDF_OK) return rc; }
  {
    int rc = VDF_OK;
    if (j->walks) {                                  // (a job of no walks -- traces its owner uploads in setup -- stages nothing)
      const void* starts, *expects;
      owner->stage_walks(*j, &starts, &expects);
      memset(s.h_ok, 0, j->walks * sizeof(int32_t));
      rc = vdf_dev_memcpy(side, s.d_walk, starts, j->walks * j->entry_bytes);
      if (rc == VDF_OK) rc = vdf_dev_memcpy(side, s.d_expect, expects, j->walks * j->entry_bytes);
    }
    if (rc == VDF_OK) rc = owner->setup(side, *j, s);
    if (rc != VDF_OK) return fail(rc, std::string("walk set-up: ") + vdf_last_error(side));
  }
  job = std::move(j);
  for (size_t li = 0; li < n; ++li) {                                   // resident from now on; a walk that misses takes it away again
    TraceSlot& t = owner->slot(job->steps[li]);
    t.d_trace = (char*)job->block->d + li * job->trace_bytes;
    t.block = job->block;
  }
  int rc;
  if (wait) rc = resolve(bad, bad_first, bad_count);
  else {
    uint64_t now, top;
    int last;
    walk_slice(job->every, job->launch_rounds, 0, 0, &now, &top, &last);
    rc = enqueue(now);
  }
  return rc != VDF_OK ? rc : pending;
}
void TraceWalks::memory(size_t slots, size_t* resident_steps, uint64_t* device_bytes) const {
  size_t n = 0;
  uint64_t bytes = spare ? spare->bytes : 0;                            // (held by a windowed prover between two windows)
  std::vector<const TraceBlock*> seen;
  for (size_t k = 0; k < slots; ++k) {
    const TraceSlot& t = owner->slot(k);
    if (!t.d_trace) continue;
    ++n;
    if (std::find(seen.begin(), seen.end(), t.block.get()) != seen.end()) continue;   // a block counts once
    seen.push_back(t.block.get());
    bytes += t.block->bytes;
  }
  if (resident_steps) *resident_steps = n;
  if (device_bytes) *device_bytes = bytes;
}
void TraceWalks::teardown(size_t slots) {
  if (job) { vdf_ctx_sync(side); job.reset(); }
  spare.reset();
  if (side) scratch_free();
  for (size_t k = 0; k < slots; ++k) lose(k);     // every trace's allocation goes with the last step that points into it
  if (side) vdf_ctx_destroy(side);
  side = nullptr;
}
}  // namespace vdfnova
