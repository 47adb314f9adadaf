// libvdf_nova.so, part 2c: the chain of a custom step circuit (vdf_custom_chain, include/vdf_nova.h) -- what circuits_host.cpp is
// to the built-in kinds: the checkpoints of a chain on the host, and per step a device trace rebuilt by the chain's walk tape
// (vdf_round_tape_walk; vdf_round_tape_walk_lanes for a chain of several lanes) on a side queue, a window ahead of the prover.
#include "nova_internal.hpp"

using namespace vdfnova;

// Traces being rebuilt: one walk per checkpoint interval of steps [first, first + count), all in one launch per slice of rounds;
// `done` rounds of `every` are enqueued so far.
struct ChainJob {
  size_t first = 0, count = 0;
  std::shared_ptr<TraceBlock> block;       // count traces of lanes * (t + 1) entries
  uint64_t done = 0, launch_rounds = 0;
};
struct ChainStep {
  void* d_trace = nullptr;                 // null, or inside `block`
  std::shared_ptr<TraceBlock> block;
};
struct vdf_custom_chain {
  int field = VDF_FIELD_FQ;
  uint64_t t = 0, every = 0;
  size_t lanes = 1;                        // chains side by side in every step (vdf_cs_repeat_lanes)
  std::vector<uint64_t> j_base;            // per lane
  size_t per = 0, na = 0;                  // walks per step AND LANE, elements per entry
  std::vector<vdf_tape_op> ops;
  std::vector<Fe> consts, inv, cp;         // inv: lanes * n_inv; cp: per lane (steps * per + 1) entries, forward order, lane-major
  std::vector<Fe> stage;                   // lanes > 1, while a job is pending: the walks' starts, then their targets, gathered
                                           // step-major, lane-minor (freed when the job resolves)
  size_t lane_entries() const { return v.size() * per + 1; }
  std::vector<ChainStep> v;
  vdf_round_tape tape;                     // into ops / consts
  vdf_ctx* ctx = nullptr;                  // where the traces live
  // the walks (WalkState of nova_internal.hpp, for entries of n_adv elements): a side queue of the device, a job enqueued with
  // wait = 0 being finished by the next call that needs its result, buffers kept from one job to the next, and the allocation of
  // a released window kept for the window after next
  vdf_ctx* side = nullptr;
  std::unique_ptr<ChainJob> job;
  void* d_walk = nullptr, *d_expect = nullptr;
  int32_t* h_ok = nullptr;                 // pinned: 1 per walk that landed on its checkpoint
  size_t scratch_walks = 0;
  std::shared_ptr<TraceBlock> spare;
  bool job_covers(size_t first, size_t count = 1) const {
    return job && count && first < job->first + job->count && job->first < first + count;
  }
};

namespace {
constexpr uint64_t DEFAULT_LAUNCH_ROUNDS = 1024;   // the built-in walks' default (circuits_host.cpp walk_launch_rounds)

void slice(uint64_t every, uint64_t launch_rounds, uint64_t done, uint64_t budget, uint64_t* rounds, uint64_t* top, int* last) {
  uint64_t now = std::min(every - done, launch_rounds ? launch_rounds : DEFAULT_LAUNCH_ROUNDS);
  if (budget) now = std::min(now, budget);
  *rounds = now;
  *top = every - done;
  *last = done + now == every;
}
void scratch_free(vdf_custom_chain* c) {
  if (c->d_walk) vdf_dev_free(c->side, c->d_walk);
  if (c->d_expect) vdf_dev_free(c->side, c->d_expect);
  if (c->h_ok) vdf_host_free(c->side, c->h_ok);
  c->d_walk = c->d_expect = nullptr; c->h_ok = nullptr;
  c->scratch_walks = 0;
}
int scratch_ensure(vdf_custom_chain* c, size_t walks) {
  if (c->scratch_walks >= walks) return VDF_OK;
  scratch_free(c);
  vdf_ctx* q = c->side;
  if (vdf_dev_alloc(q, walks * c->na * 32, &c->d_walk) != VDF_OK || vdf_dev_alloc(q, walks * c->na * 32, &c->d_expect) != VDF_OK ||
      vdf_host_alloc(q, walks * sizeof(int32_t), (void**)&c->h_ok) != VDF_OK) {
    const int rc = fail(VDF_ERR_OOM, std::string("walk buffers: ") + vdf_last_error(q));
    scratch_free(c);
    return rc;
  }
  c->scratch_walks = walks;
  return VDF_OK;
}
void lose(vdf_custom_chain* c, size_t k) { c->v[k].d_trace = nullptr; c->v[k].block.reset(); }
void release_range(vdf_custom_chain* c, size_t first, size_t count, bool park) {
  for (size_t k = first; k < first + count; ++k) {
    ChainStep& s = c->v[k];
    if (!s.block) continue;
    s.d_trace = nullptr;
    if (park && s.block.use_count() == 1) c->spare = std::move(s.block);
    s.block.reset();
  }
}
// enqueue up to `budget` more rounds of the pending walks (0: all that are left), in launches of the job's bounded length
int job_enqueue(vdf_custom_chain* c, uint64_t budget) {
  ChainJob* j = c->job.get();
  const size_t walks = j->count * c->lanes * c->per;
  uint64_t jb[VDF_TAPE_MAX_LANES];
  for (size_t l = 0; l < c->lanes; ++l) jb[l] = c->j_base[l] + (uint64_t)j->first * c->t;
  while (j->done < c->every) {
    uint64_t now, top;
    int last;
    slice(c->every, j->launch_rounds, j->done, budget, &now, &top, &last);
    if (c->lanes == 1)
      HIPCALL(c->side, vdf_round_tape_walk(c->side, c->field, &c->tape, (const vdf_fe*)c->inv.data(), (vdf_fe*)c->d_walk, walks, now,
                                           (vdf_fe*)j->block->d, (size_t)c->every, (size_t)top, c->per, (size_t)(c->t + 1), jb[0], c->t, last,
                                           last ? (const vdf_fe*)c->d_expect : nullptr, last ? c->h_ok : nullptr));
    else                                             // every lane of every step of the window in ONE launch: group G = step * lanes + lane
      HIPCALL(c->side, vdf_round_tape_walk_lanes(c->side, c->field, &c->tape, c->lanes, (const vdf_fe*)c->inv.data(), (vdf_fe*)c->d_walk, walks,
                                                 now, (vdf_fe*)j->block->d, (size_t)c->every, (size_t)top, c->per, (size_t)(c->t + 1), jb, c->t,
                                                 last, last ? (const vdf_fe*)c->d_expect : nullptr, last ? c->h_ok : nullptr));
    j->done += now;
    if (budget && (budget -= now) == 0) break;
  }
  return VDF_OK;
}
// finish the pending walks: the rest of their rounds with the comparison on the device, and the verdict per step
int job_resolve(vdf_custom_chain* c, int* bad, size_t bad_first, size_t bad_count) {
  ChainJob* j = c->job.get();
  if (!j) return VDF_OK;
  int rc = job_enqueue(c, 0);
  if (rc == VDF_OK && (rc = vdf_ctx_sync(c->side)) != VDF_OK) fail(rc, std::string("vdf_ctx_sync: ") + vdf_last_error(c->side));
  if (rc != VDF_OK) vdf_ctx_sync(c->side);
  std::vector<Fe>().swap(c->stage);                                     // the uploads have run: the staging copy goes with the job
  if (rc != VDF_OK) {                                                   // a device failure: none of these traces can be trusted
    for (size_t k = j->first; k < j->first + j->count; ++k) lose(c, k);
    c->job.reset();
    return rc;
  }
  size_t first_bad = (size_t)-1, bad_lane = 0;
  for (size_t li = 0; li < j->count; ++li) {
    size_t miss = (size_t)-1;                                           // the first lane of the step with a walk that missed
    for (size_t m = c->lanes * c->per; m-- > 0;)
      if (c->h_ok[li * c->lanes * c->per + m] != 1) miss = m / c->per;
    if (miss == (size_t)-1) continue;
    const size_t k = j->first + li;
    lose(c, k);
    if (first_bad == (size_t)-1) { first_bad = k; bad_lane = miss; }
    if (bad && k >= bad_first && k - bad_first < bad_count) bad[k - bad_first] = 1;
  }
  c->job.reset();                                                       // (its buffers stay: scratch_free)
  if (first_bad != (size_t)-1)
    return fail(VDF_ERR_BAD_ARG, "step " + std::to_string(first_bad) + (c->lanes > 1 ? ", lane " + std::to_string(bad_lane) : std::string()) +
                                     ": a walk did not land on the checkpoint below it");
  return VDF_OK;
}
}  // namespace

namespace vdfnova {
ChainInfo chain_info(const vdf_custom_chain* c) { return ChainInfo{c->field, c->t, c->na, c->v.size(), c->ctx, c->lanes}; }
int chain_need(vdf_custom_chain* c, size_t k, const vdf_fe** d_trace) {
  if (c->job_covers(k)) { int rc = job_resolve(c, nullptr, 0, 0); if (rc != VDF_OK) return rc; }
  if (!c->v[k].d_trace) return fail(VDF_ERR_BAD_ARG, "advice of step " + std::to_string(k) + " not materialised");
  *d_trace = (const vdf_fe*)c->v[k].d_trace;
  return VDF_OK;
}
// Called by the step that proves k: the pending walks are wanted by the step that proves job->first, so the calls from here to
// there share the remaining rounds evenly.
int chain_pump(vdf_custom_chain* c, size_t k) {
  ChainJob* j = c->job.get();
  if (!j || j->done >= c->every) return VDF_OK;
  const uint64_t calls = j->first > k ? j->first - k : 1, left = c->every - j->done;
  return job_enqueue(c, (left + calls - 1) / calls);
}
int chain_settle(vdf_custom_chain* c) { return job_resolve(c, nullptr, 0, 0); }
bool chain_resident(const vdf_custom_chain* c, size_t k) { return c->v[k].d_trace != nullptr; }
const vdf_fe* chain_ready(const vdf_custom_chain* c, size_t k) {
  return k < c->v.size() && !c->job_covers(k) ? (const vdf_fe*)c->v[k].d_trace : nullptr;
}
void chain_park(vdf_custom_chain* c, size_t k) { release_range(c, k, 1, true); }
void chain_drop_spare(vdf_custom_chain* c) { c->spare.reset(); }
}  // namespace vdfnova

extern "C" {
int vdf_nova_custom_chain_slice(uint64_t every, uint64_t launch_rounds, uint64_t done, uint64_t budget, uint64_t* rounds, uint64_t* top,
                                int* last) {
  if (!rounds || !top || !last) return fail(VDF_ERR_BAD_ARG, "null argument");
  if (every == 0 || done >= every) return fail(VDF_ERR_BAD_ARG, "`every` must be positive and `done` below it");
  slice(every, launch_rounds, done, budget, rounds, top, last);
  return VDF_OK;
}
int vdf_nova_custom_chain_from_checkpoints(int fid, const vdf_round_tape* walk_tape, const vdf_fe* inv, uint64_t t, uint64_t every,
                                           size_t num_steps, const vdf_fe* checkpoints, uint64_t j_base, vdf_custom_chain** out) {
  const size_t stride = every && t && num_steps <= ((size_t)1 << 40) ? num_steps * (size_t)(t / every) + 1 : 1;      // (refused below otherwise)
  return vdf_nova_custom_chain_lanes_from_checkpoints(fid, walk_tape, inv, t, every, num_steps, 1, checkpoints, stride, &j_base, out);
}
int vdf_nova_custom_chain_lanes_from_checkpoints(int fid, const vdf_round_tape* walk_tape, const vdf_fe* inv, uint64_t t, uint64_t every,
                                                 size_t num_steps, size_t lanes, const vdf_fe* checkpoints, size_t lane_stride,
                                                 const uint64_t* j_base, vdf_custom_chain** out) {
  return nova_guard([&]() -> int {
    if (!out) return fail(VDF_ERR_BAD_ARG, "null out");
    *out = nullptr;
    if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
    if (!walk_tape || !checkpoints || !j_base) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (num_steps == 0) return fail(VDF_ERR_BAD_ARG, "num_steps must be > 0");
    if (t == 0 || t >= (1ull << 31)) return fail(VDF_ERR_BAD_ARG, "t out of range (1 <= t < 2^31, vdf_cs_repeat)");
    if (every == 0 || t % every != 0) return fail(VDF_ERR_BAD_ARG, "`every` must be positive and divide t");
    if (lanes == 0 || lanes > VDF_TAPE_MAX_LANES) return fail(VDF_ERR_BAD_ARG, "lanes must be 1 .. VDF_TAPE_MAX_LANES");
    // the check the walk's launcher applies, by its host restatement with nothing to walk (a null `inv` the tape reads included):
    // vdf_round_tape_walk's for one lane, vdf_round_tape_walk_lanes' (lanes * n_inv, n_inv more slots) for more
    {
      const int rc = lanes == 1 ? eval_walk_tape(fid, walk_tape, (const Fe*)inv, nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0, nullptr, nullptr)
                                : eval_walk_tape_lanes(fid, walk_tape, lanes, (const Fe*)inv, nullptr, 0, 0, nullptr, 0, 0, 0, 0, j_base, 0, 0, nullptr, nullptr);
      if (rc != VDF_OK) return rc;
    }
    const size_t per = (size_t)(t / every), na = walk_tape->n_adv;
    if (num_steps > ((size_t)1 << 40) / per) return fail(VDF_ERR_BAD_LENGTH, "too many checkpoints");
    const size_t entries = num_steps * per + 1;
    if (lane_stride < entries || lane_stride > ((size_t)1 << 44)) return fail(VDF_ERR_BAD_ARG, "lane_stride must be at least num_steps * (t / every) + 1");
    std::unique_ptr<vdf_custom_chain> c(new vdf_custom_chain());
    c->field = fid; c->t = t; c->every = every; c->lanes = lanes; c->per = per; c->na = na;
    c->j_base.assign(j_base, j_base + lanes);
    c->ops.assign(walk_tape->ops, walk_tape->ops + walk_tape->n_ops);
    c->consts.assign((const Fe*)walk_tape->consts, (const Fe*)walk_tape->consts + walk_tape->n_consts);
    if (walk_tape->n_inv) c->inv.assign((const Fe*)inv, (const Fe*)inv + lanes * walk_tape->n_inv);
    c->tape = *walk_tape;
    c->tape.ops = c->ops.data();
    c->tape.consts = (const vdf_fe*)c->consts.data();
    c->cp.resize(lanes * entries * na);
    const bool device = vdf_ptr_is_device(checkpoints);
    for (size_t l = 0; l < lanes; ++l) {
      const Fe* src = (const Fe*)checkpoints + l * lane_stride * na;
      if (device) {
        // (a copy only, after every refusal: the runtime finds the pointer's device, nothing is allocated there)
        const int rc = vdf_ptr_download(c->cp.data() + l * entries * na, src, entries * na * 32);
        if (rc != VDF_OK) return fail(rc, std::string("checkpoints: ") + vdf_last_error(nullptr));
      } else memcpy(c->cp.data() + l * entries * na, src, entries * na * 32);
    }
    c->v.resize(num_steps);
    *out = c.release();
    return VDF_OK;
  });
}
int vdf_nova_custom_chain_materialize(vdf_ctx* ctx, vdf_custom_chain* c, size_t first, size_t count, int wait, uint64_t launch_rounds,
                                      int* bad) {
  return nova_guard([&]() -> int {
    if (!ctx || !c) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (first > c->v.size() || count > c->v.size() - first) return fail(VDF_ERR_BAD_LENGTH, "step range out of bounds");
    if (bad) for (size_t k = 0; k < count; ++k) bad[k] = 0;
    const int pending = job_resolve(c, bad, first, count);              // one job at a time; its verdict is this call's too
    if (pending != VDF_OK && pending != VDF_ERR_BAD_ARG) return pending;
    if (c->ctx && vdf_ctx_device(c->ctx) != vdf_ctx_device(ctx)) return fail(VDF_ERR_BAD_ARG, "the chain's traces live on another device");
    c->ctx = ctx;
    // the steps of the range without a trace, from the first to the last of them (a resident step between two of them is walked again)
    size_t lo = first + count, hi = first;
    for (size_t k = first; k < first + count; ++k) if (!c->v[k].d_trace) { lo = std::min(lo, k); hi = k + 1; }
    if (lo >= hi) return pending;
    if (!c->side) {
      const int dev = vdf_ctx_device(ctx);
      if (vdf_ctx_create_pooled(&dev, 1, VDF_QUEUE_SIDE, &c->side) != VDF_OK)
        return fail(VDF_ERR_DEVICE, std::string("walk context: ") + vdf_last_error(nullptr));
      HIPCALL(c->side, vdf_ctx_set_async(c->side, 1));
    }
    vdf_ctx* q = c->side;
    std::unique_ptr<ChainJob> j(new ChainJob());
    j->first = lo; j->count = hi - lo; j->launch_rounds = launch_rounds;
    const uint64_t trace_bytes = c->lanes * (c->t + 1) * c->na * 32;
    const size_t walks = j->count * c->lanes * c->per;
    if (j->count > (~(uint64_t)0 >> 1) / trace_bytes) return fail(VDF_ERR_OOM, "the traces do not fit");
    if (walks > ((size_t)1 << 31)) return fail(VDF_ERR_BAD_LENGTH, "more than 2^31 walks in a window");
    // the windowed prover's spare allocation, when it is exactly this size; anything else is asked of the device
    if (c->spare && c->spare.use_count() == 1 && c->spare->ctx == ctx && c->spare->bytes == j->count * trace_bytes) j->block = std::move(c->spare);
    c->spare.reset();
    if (!j->block) {
      j->block = std::shared_ptr<TraceBlock>(new TraceBlock{ctx, j->count * trace_bytes});
      size_t free_bytes = 0;                       // asked first: an allocation beyond the free memory may be granted and fail later
      HIPCALL(ctx, vdf_dev_mem_info(ctx, &free_bytes, nullptr));
      if (j->block->bytes + walks * c->na * 64 > free_bytes)
        return fail(VDF_ERR_OOM, "the traces of " + std::to_string(j->count) + " steps (" + std::to_string(j->block->bytes) +
                                     " bytes) do not fit the device's free memory (" + std::to_string(free_bytes) + " bytes)");
      if (vdf_dev_alloc(ctx, j->block->bytes, &j->block->d) != VDF_OK) {
        j->block->d = nullptr;
        return fail(VDF_ERR_OOM, "the traces of " + std::to_string(j->count) + " steps do not fit: " + vdf_last_error(ctx));
      }
    }
    { int rc = scratch_ensure(c, walks); if (rc != VDF_OK) return rc; }
    {
      // walk li * per + m stands on the checkpoint above interval m of step lo + li and must land on the one below it: both runs
      // are contiguous in the lane's checkpoints; with more lanes than one they are gathered step-major, lane-minor (the walks'
      // order), into a staging vector that lives until the job resolves
      const Fe* cp = c->cp.data() + lo * c->per * c->na;
      const Fe* starts = cp + c->na;
      if (c->lanes > 1) {
        const size_t run = c->per * c->na;
        c->stage.resize(2 * walks * c->na);
        for (size_t li = 0; li < j->count; ++li)
          for (size_t l = 0; l < c->lanes; ++l) {
            const Fe* src = c->cp.data() + (l * c->lane_entries() + (lo + li) * c->per) * c->na;
            memcpy(c->stage.data() + (li * c->lanes + l) * run, src + c->na, run * 32);
            memcpy(c->stage.data() + walks * c->na + (li * c->lanes + l) * run, src, run * 32);
          }
        starts = c->stage.data();
        cp = c->stage.data() + walks * c->na;
      }
      memset(c->h_ok, 0, walks * sizeof(int32_t));
      int rc = vdf_dev_memcpy(q, c->d_walk, starts, walks * c->na * 32);
      if (rc == VDF_OK) rc = vdf_dev_memcpy(q, c->d_expect, cp, walks * c->na * 32);
      if (rc != VDF_OK) return fail(rc, std::string("walk set-up: ") + vdf_last_error(q));
    }
    c->job = std::move(j);
    ChainJob* job = c->job.get();
    for (size_t li = 0; li < job->count; ++li) {                        // resident from now on; a walk that misses takes it away again
      ChainStep& s = c->v[job->first + li];
      s.d_trace = (char*)job->block->d + li * trace_bytes;
      s.block = job->block;
    }
    if (!wait) {
      uint64_t now, top;
      int last;
      slice(c->every, job->launch_rounds, 0, 0, &now, &top, &last);
      const int rc = job_enqueue(c, now);
      return rc != VDF_OK ? rc : pending;
    }
    const int rc = job_resolve(c, bad, first, count);
    return rc != VDF_OK ? rc : pending;
  });
}
int vdf_nova_custom_chain_release(vdf_custom_chain* c, size_t first, size_t count) {
  return nova_guard([&]() -> int {
    if (!c) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (first > c->v.size() || count > c->v.size() - first) return fail(VDF_ERR_BAD_LENGTH, "step range out of bounds");
    const int pending = c->job_covers(first, count) ? job_resolve(c, nullptr, 0, 0) : VDF_OK;
    release_range(c, first, count, false);
    return pending;
  });
}
int vdf_nova_custom_chain_memory(const vdf_custom_chain* c, size_t* resident_steps, uint64_t* device_bytes) {
  if (!c) return fail(VDF_ERR_BAD_ARG, "null argument");
  size_t n = 0;
  uint64_t bytes = 0;
  std::vector<const TraceBlock*> seen;
  for (const ChainStep& s : c->v) {
    if (!s.d_trace) continue;
    ++n;
    if (std::find(seen.begin(), seen.end(), s.block.get()) != seen.end()) continue;   // a block counts once
    seen.push_back(s.block.get());
    bytes += s.block->bytes;
  }
  if (c->spare) bytes += c->spare->bytes;                              // (held by a windowed prover between two windows)
  if (resident_steps) *resident_steps = n;
  if (device_bytes) *device_bytes = bytes;
  return VDF_OK;
}
int vdf_nova_custom_chain_host_bytes(const vdf_custom_chain* c, uint64_t* bytes) {
  if (!c || !bytes) return fail(VDF_ERR_BAD_ARG, "null argument");
  *bytes = c->ops.size() * sizeof(vdf_tape_op) + (c->consts.size() + c->inv.size() + c->cp.size() + c->stage.size()) * 32;
  return VDF_OK;
}
size_t vdf_nova_custom_chain_len(const vdf_custom_chain* c) { return c ? c->v.size() : 0; }
int vdf_nova_custom_chain_advice(vdf_custom_chain* c, size_t k, const vdf_fe** d_advice) {
  return nova_guard([&]() -> int {
    if (!c || !d_advice) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (k >= c->v.size()) return fail(VDF_ERR_BAD_LENGTH, "step index out of range");
    *d_advice = nullptr;
    if (c->job_covers(k)) { int rc = job_resolve(c, nullptr, 0, 0); if (rc != VDF_OK && rc != VDF_ERR_BAD_ARG) return rc; }
    *d_advice = (const vdf_fe*)c->v[k].d_trace;
    return VDF_OK;
  });
}
void vdf_nova_custom_chain_free(vdf_custom_chain* c) {
  if (!c) return;
  if (c->job) { vdf_ctx_sync(c->side); c->job.reset(); }
  c->spare.reset();
  if (c->side) scratch_free(c);
  c->v.clear();                                   // every trace's allocation goes with the last step that points into it
  if (c->side) vdf_ctx_destroy(c->side);
  delete c;
}
}  // extern "C"
