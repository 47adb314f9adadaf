// libvdf_nova.so, part 2b: the circuits handle of the Nova surface (vdf_circuits; src/nova/proof.rs:57-66, :268-294) -- the steps
// of a chain as prove_step reads them, made from an evaluation, from a chain's checkpoints or pushed while the chain grows, and
// the device traces behind them: copied from the host, or rebuilt from checkpoints by inverse walks on a side queue.
#include "nova_internal.hpp"

using namespace vdfnova;

namespace {
// states[1 .. n] count on from states[0], whose i is `from`, in steps of `every`
int check_counters(int fid, const vdf_state* states, size_t n, Fe from, uint64_t every) {
  const Field& F = field(fid);
  const Fe step = from_u64(every, F);
  for (size_t k = 1; k <= n; ++k) {
    from = add(from, step, F);
    if (memcmp(&states[k].i, &from, 32) != 0)
      return fail(VDF_ERR_BAD_ARG, "checkpoint " + std::to_string(k) + ": i is not states[0].i + " + std::to_string(k) + " * every");
  }
  return VDF_OK;
}
// the step whose states every `every` rounds are states[0 .. per]
Circuit checkpoint_circuit(uint64_t t, uint64_t every, const vdf_state* states, size_t per) {
  Circuit c;
  c.t = t; c.every = every;
  c.cp.resize(per + 1);
  for (size_t m = 0; m <= per; ++m) c.cp[m] = load_state(&states[m]);
  c.input = c.cp.front(); c.result = c.cp.back();
  return c;
}
// ---- forward chains: a step pushed for all `lanes` lanes of the chain (a single chain: one) ----------------------------------
// a refusal about lane l: "lane 2: ... the lane's current end" in a chain of lanes, "... the chain's current end" in a single one
std::string lane_tag(const vdf_circuits* c, size_t l) { return c->lanes > 1 ? "lane " + std::to_string(l) + ": " : std::string(); }
const char* lane_owner(const vdf_circuits* c) { return c->lanes > 1 ? "lane's" : "chain's"; }
// the step every lane ends: appended, and the chain stands where it ends
void push_step(vdf_circuits* c, Circuit&& cc) {
  cc.input = cc.lane_input[0]; cc.result = cc.lane_result[0];
  c->lane_end = cc.lane_result;
  c->end = cc.result;
  c->v.push_back(std::move(cc));
}
int push_traces(vdf_circuits* c, const vdf_fe* trace_xy, size_t lane_stride) {
  const uint64_t t = c->forward_t;
  const size_t L = c->lanes;
  if (lane_stride < t + 1) return fail(VDF_ERR_BAD_ARG, "lane_stride must be at least t + 1");
  const Field& F = field(c->field);
  Circuit cc;
  cc.t = t;
  cc.lane_input = c->lane_end;
  cc.lane_result.resize(L);
  for (size_t l = 0; l < L; ++l) {                                   // every lane checked before anything is appended
    const vdf_fe* tr = trace_xy + 2 * l * lane_stride;
    if (memcmp(&tr[0], &c->lane_end[l].x, 32) != 0 || memcmp(&tr[1], &c->lane_end[l].y, 32) != 0)
      return fail(VDF_ERR_BAD_ARG, lane_tag(c, l) + "the trace does not start at the " + lane_owner(c) + " current end");
    memcpy(&cc.lane_result[l].x, &tr[2 * t], 32);
    memcpy(&cc.lane_result[l].y, &tr[2 * t + 1], 32);
    cc.lane_result[l].i = add(c->lane_end[l].i, from_u64(t, F), F);
  }
  cc.trace_xy.reserve(L * 2 * (t + 1));
  for (size_t l = 0; l < L; ++l) {
    const Fe* tr = (const Fe*)trace_xy + 2 * l * lane_stride;
    cc.trace_xy.insert(cc.trace_xy.end(), tr, tr + 2 * (t + 1));
  }
  push_step(c, std::move(cc));
  return VDF_OK;
}
int push_checkpoints(vdf_circuits* c, uint64_t every, const vdf_state* states, size_t lane_stride) {
  const uint64_t t = c->forward_t;
  const size_t L = c->lanes;
  if (every == 0 || t % every != 0) return fail(VDF_ERR_BAD_ARG, "`every` must be positive and divide t");
  const size_t per = (size_t)(t / every);
  if (lane_stride < per + 1) return fail(VDF_ERR_BAD_ARG, "lane_stride must be at least t / every + 1");
  if (c->checkpoints)
    for (const Circuit& k : c->v) if (k.every && k.every != every) return fail(VDF_ERR_BAD_ARG, "`every` differs from the chain's earlier checkpoint steps");
  for (size_t l = 0; l < L; ++l) {                                   // every lane checked before anything is appended
    const vdf_state* st = states + l * lane_stride;
    if (memcmp(&st[0], &c->lane_end[l], 96) != 0) return fail(VDF_ERR_BAD_ARG, lane_tag(c, l) + "states[0] is not the " + lane_owner(c) + " current end");
    if (check_counters(c->field, st, per, c->lane_end[l].i, every) != VDF_OK) return fail(VDF_ERR_BAD_ARG, lane_tag(c, l) + vdf_nova_last_error());
  }
  Circuit cc;
  cc.t = t; cc.every = every;
  cc.lane_input = c->lane_end;
  cc.cp.reserve(L * (per + 1));
  for (size_t l = 0; l < L; ++l)
    for (size_t m = 0; m <= per; ++m) cc.cp.push_back(load_state(&states[l * lane_stride + m]));
  for (size_t l = 0; l < L; ++l) cc.lane_result.push_back(cc.cp[l * (per + 1) + per]);
  push_step(c, std::move(cc));
  c->checkpoints = true;
  return VDF_OK;
}
// ---- checkpoint circuits: traces by inverse walks ----------------------------------------------------------------
// rounds per launch of the walks: a launch of 1,024 rounds holds a queue for about a millisecond
uint64_t walk_launch_rounds() {
  static const uint64_t v = [] {
    const char* e = getenv("VDF_NOVA_WALK_LAUNCH");
    const long n = e && *e ? atol(e) : 0;
    return (uint64_t)(n >= 1 && n <= (1 << 22) ? n : 1024);
  }();
  return v;
}
// the one cast (CircuitWalks, nova_internal.hpp): walks resolved, begun or parked under a const handle write d_trace and block of v[k]
vdf_circuits* written(const vdf_circuits* c) { return const_cast<vdf_circuits*>(c); }
}  // namespace

// ---- what TraceWalks asks of the circuits: walk (li L + l) per_lane + m is lane l's interval m of step steps[li] -------------------
TraceSlot& CircuitWalks::slot(size_t k) { return written(c)->v[k]; }
void CircuitWalks::shape(size_t first_step, WalkJob* j) {
  const Circuit& c0 = c->v[first_step];
  j->every = c0.every;
  j->trace_bytes = c->lanes * (c0.t + 1) * 64;                          // a step's trace: its lanes' traces back to back
  j->step_walks = c->lanes * (size_t)(c0.t / c0.every);
  j->entry_bytes = 96;
}
void CircuitWalks::stage_walks(const WalkJob& j, const void** starts, const void** expects) {
  const size_t L = c->lanes, per = j.step_walks / L;
  from.resize(j.walks); to.resize(j.walks);
  for (size_t li = 0; li < j.steps.size(); ++li) {
    const Circuit& k = c->v[j.steps[li]];
    for (size_t l = 0; l < L; ++l)
      for (size_t m = 0; m < per; ++m) {
        const size_t wk = (li * L + l) * per + m, at = l * (per + 1) + m;
        from[wk] = k.cp[at + 1]; to[wk] = k.cp[at];
      }
  }
  *starts = from.data(); *expects = to.data();
}
void CircuitWalks::unstage() { std::vector<St>().swap(from); std::vector<St>().swap(to); }
int CircuitWalks::setup(vdf_ctx* q, const WalkJob& j, const WalkScratch& s) {
  const size_t per = j.step_walks / c->lanes;
  return vdf_minroot_trace_heads(q, (const vdf_state*)s.d_expect, j.steps.size() * c->lanes, per, (vdf_fe*)j.block->d, (size_t)(c->v[j.steps[0]].t + 1));
}
int CircuitWalks::launch(vdf_ctx* q, const WalkJob& j, const WalkScratch& s, uint64_t rounds, uint64_t top, int) {
  HIPCALL(q, vdf_minroot_inverse_walk(q, c->field, (vdf_state*)s.d_walk, j.walks, rounds, (vdf_fe*)j.block->d, (size_t)j.every, (size_t)top,
                                      j.step_walks / c->lanes, (size_t)(c->v[j.steps[0]].t + 1)));
  return VDF_OK;
}
int CircuitWalks::finish(vdf_ctx* q, const WalkJob& j, const WalkScratch& s) {   // the comparison on the device
  const int rc = vdf_minroot_check_batch(q, c->field, (const vdf_state*)s.d_walk, (const vdf_state*)s.d_expect, j.walks, 0, s.h_ok);
  return rc == VDF_OK ? rc : fail(rc, std::string("vdf_minroot_check_batch: ") + vdf_last_error(q));
}
std::string CircuitWalks::missed(size_t k, size_t) { return "circuit " + std::to_string(k) + ": an inverse walk did not land on the checkpoint before it"; }

namespace vdfnova {
int circuits_need(const vdf_circuits* c, size_t k) {
  if (c->walk.covers(k)) { int rc = c->walk.resolve(nullptr, 0, 0); if (rc != VDF_OK) return rc; }
  const Circuit& cc = c->v[k];
  if (!cc.d_trace && cc.trace_xy.empty()) return fail(VDF_ERR_BAD_ARG, "trace of circuit " + std::to_string(k) + " not materialised");
  return VDF_OK;
}
// prove_step(k) needs circuits k and k + 1: the pending walks are wanted by the prove_step one before their first step
int circuits_pump(const vdf_circuits* c, size_t k) { return c->walk.pump(k, 1); }
int circuits_materialize(vdf_ctx* ctx, const vdf_circuits* c, size_t first, size_t count, int wait, int* bad) {
  return vdf_nova_circuits_materialize(ctx, written(c), first, count, wait, bad);
}
}  // namespace vdfnova

extern "C" {
int vdf_nova_eval_and_make_circuits(int mode, uint64_t t, size_t num_steps, const vdf_state* initial_state,
                                    vdf_fe z0_primary[3], vdf_circuits** out) {
  return vdf_nova_eval_and_make_circuits_field(VDF_FIELD_FQ, mode, t, num_steps, initial_state, z0_primary, out);
}
int vdf_nova_eval_and_make_circuits_field(int fid, int mode, uint64_t t, size_t num_steps, const vdf_state* initial_state,
                                          vdf_fe z0_primary[3], vdf_circuits** out) {
  return nova_guard([&]() -> int {
    if (!valid_field(fid) || !valid_mode(mode) || !initial_state || !z0_primary || !out || t == 0) return fail(VDF_ERR_BAD_ARG, "bad argument");
    if (num_steps == 0) return fail(VDF_ERR_BAD_ARG, "num_steps must be > 0 (assert!, src/nova/proof.rs:268)");
    vdf_circuits* cs = new vdf_circuits();
    cs->field = fid;
    St state = load_state(initial_state);
    for (size_t s = 0; s < num_steps; ++s) {                          // :274-279
      Circuit c;
      c.t = t;
      c.input = state;                                                 // previous_state, :285-291
      c.trace_xy.resize(2 * (t + 1));
      eval_step(fid, mode, t, &state, c.trace_xy.data());
      c.result = state;
      cs->v.push_back(std::move(c));
    }
    memcpy(z0_primary, &state, 96);                                    // z0 = final state, :278-281
    std::reverse(cs->v.begin(), cs->v.end());                          // circuits.reverse(), :294
    *out = cs;
    return VDF_OK;
  });
}
int vdf_nova_circuits_from_checkpoints(uint64_t t, uint64_t every, size_t num_steps, const vdf_state* states,
                                       vdf_fe z0_primary[3], vdf_circuits** out) {
  return vdf_nova_circuits_from_checkpoints_field(VDF_FIELD_FQ, t, every, num_steps, states, z0_primary, out);
}
int vdf_nova_circuits_from_checkpoints_field(int fid, uint64_t t, uint64_t every, size_t num_steps, const vdf_state* states,
                                             vdf_fe z0_primary[3], vdf_circuits** out) {
  return nova_guard([&]() -> int {
    if (!valid_field(fid) || !states || !z0_primary || !out || t == 0) return fail(VDF_ERR_BAD_ARG, "bad argument");
    if (num_steps == 0) return fail(VDF_ERR_BAD_ARG, "num_steps must be > 0 (assert!, src/nova/proof.rs:268)");
    if (every == 0 || t % every != 0) return fail(VDF_ERR_BAD_ARG, "`every` must be positive and divide t");
    const size_t per = (size_t)(t / every), total = num_steps * per + 1;
    { int rc = check_counters(fid, states, total - 1, load_state(&states[0]).i, every); if (rc != VDF_OK) return rc; }
    std::unique_ptr<vdf_circuits> cs(new vdf_circuits());
    cs->field = fid;
    cs->checkpoints = true;
    cs->v.resize(num_steps);
    for (size_t s = 0; s < num_steps; ++s) cs->v[num_steps - 1 - s] = checkpoint_circuit(t, every, states + s * per, per);   // circuits.reverse(), :294
    memcpy(z0_primary, &states[total - 1], 96);                        // z0 = final state, :278-281
    *out = cs.release();
    return VDF_OK;
  });
}

// ---- forward chains: circuits in the order of evaluation, appended to while the chain grows.  A step advances `lanes`
// evaluations, and its trace is their traces back to back; a single chain is the chain of one lane, whose lane_stride is implied.
int vdf_nova_circuits_forward_begin(uint64_t t, const vdf_state* initial_state, vdf_fe z0_primary[3], vdf_circuits** out) {
  return vdf_nova_circuits_lanes_begin_field(VDF_FIELD_FQ, t, 1, initial_state, z0_primary, out);
}
int vdf_nova_circuits_forward_begin_field(int fid, uint64_t t, const vdf_state* initial_state, vdf_fe z0_primary[3], vdf_circuits** out) {
  return vdf_nova_circuits_lanes_begin_field(fid, t, 1, initial_state, z0_primary, out);
}
int vdf_nova_circuits_lanes_begin(uint64_t t, size_t lanes, const vdf_state* initial, vdf_fe* z0_primary, vdf_circuits** out) {
  return vdf_nova_circuits_lanes_begin_field(VDF_FIELD_FQ, t, lanes, initial, z0_primary, out);
}
int vdf_nova_circuits_lanes_begin_field(int fid, uint64_t t, size_t lanes, const vdf_state* initial, vdf_fe* z0_primary, vdf_circuits** out) {
  return nova_guard([&]() -> int {
    if (!valid_field(fid) || !initial || !z0_primary || !out || t == 0 || t > (1ull << 24)) return fail(VDF_ERR_BAD_ARG, "bad argument");
    if (lanes == 0 || lanes > VDF_NOVA_MAX_LANES) return fail(VDF_ERR_BAD_ARG, "lanes must be 1 .. VDF_NOVA_MAX_LANES");
    std::unique_ptr<vdf_circuits> cs(new vdf_circuits());
    cs->field = fid;
    cs->forward = true;
    cs->forward_t = t;
    cs->lanes = lanes;
    for (size_t l = 0; l < lanes; ++l) cs->lane_end.push_back(load_state(&initial[l]));
    cs->end = cs->lane_end[0];
    memcpy(z0_primary, initial, 96 * lanes);                           // z0 = the lanes' initial states, flattened
    *out = cs.release();
    return VDF_OK;
  });
}
int vdf_nova_circuits_push_trace(vdf_circuits* c, const vdf_fe* trace_xy) {
  return nova_guard([&]() -> int {
    if (!c || !trace_xy) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (!c->forward) return fail(VDF_ERR_BAD_ARG, "not a forward chain (vdf_nova_circuits_forward_begin)");
    if (c->lanes > 1) return fail(VDF_ERR_BAD_ARG, "a chain of more than one lane: vdf_nova_circuits_push_traces");
    return push_traces(c, trace_xy, (size_t)c->forward_t + 1);
  });
}
int vdf_nova_circuits_push_traces(vdf_circuits* c, const vdf_fe* trace_xy, size_t lane_stride) {
  return nova_guard([&]() -> int {
    if (!c || !trace_xy) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (!c->forward) return fail(VDF_ERR_BAD_ARG, "not a forward chain (vdf_nova_circuits_lanes_begin)");
    return push_traces(c, trace_xy, lane_stride);
  });
}
int vdf_nova_circuits_push_checkpoints(vdf_circuits* c, uint64_t every, const vdf_state* states) {
  return nova_guard([&]() -> int {
    if (!c || !states) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (!c->forward) return fail(VDF_ERR_BAD_ARG, "not a forward chain (vdf_nova_circuits_forward_begin)");
    if (c->lanes > 1) return fail(VDF_ERR_BAD_ARG, "a chain of more than one lane: vdf_nova_circuits_push_checkpoints_lanes");
    return push_checkpoints(c, every, states, (size_t)(every ? c->forward_t / every : 0) + 1);   // (a bad `every` is refused there)
  });
}
int vdf_nova_circuits_push_checkpoints_lanes(vdf_circuits* c, uint64_t every, const vdf_state* states, size_t lane_stride) {
  return nova_guard([&]() -> int {
    if (!c || !states) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (!c->forward) return fail(VDF_ERR_BAD_ARG, "not a forward chain (vdf_nova_circuits_lanes_begin)");
    return push_checkpoints(c, every, states, lane_stride);
  });
}
size_t vdf_nova_circuits_lanes(const vdf_circuits* c) { return c ? c->lanes : 0; }
int vdf_nova_circuits_field(const vdf_circuits* c) { return c ? c->field : -1; }
int vdf_nova_circuit_lane_states(const vdf_circuits* c, size_t k, size_t lane, vdf_state* result, vdf_state* input) {
  if (!c || k >= c->v.size()) return fail(VDF_ERR_BAD_LENGTH, "circuit index out of range");
  if (lane >= c->lanes) return fail(VDF_ERR_BAD_LENGTH, "lane out of range");
  const Circuit& cc = c->v[k];
  const bool per_lane = !cc.lane_result.empty();                       // a forward chain's step; any other circuit is its own lane 0
  if (result) store_state(result, per_lane ? cc.lane_result[lane] : cc.result);
  if (input) store_state(input, per_lane ? cc.lane_input[lane] : cc.input);
  return VDF_OK;
}
// ---- traces on the device ---------------------------------------------------------------------------------------
int vdf_nova_circuits_materialize(vdf_ctx* ctx, vdf_circuits* c, size_t first, size_t count, int wait, int* bad) {
  return nova_guard([&]() -> int {
    if (!ctx || !c) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (!c->checkpoints) return fail(VDF_ERR_BAD_ARG, "these circuits carry their traces: vdf_nova_circuits_upload");
    if (first > c->v.size() || count > c->v.size() - first) return fail(VDF_ERR_BAD_LENGTH, "circuit range out of bounds");
    if (bad) for (size_t k = 0; k < count; ++k) bad[k] = 0;
    const int pending = c->walk.resolve(bad, first, count);            // one job at a time; its verdict is this call's too
    if (pending != VDF_OK && pending != VDF_ERR_BAD_ARG) return pending;
    // (a forward chain may mix steps pushed as traces with steps pushed as checkpoints: only the latter are walked)
    std::vector<size_t> steps;
    for (size_t k = first; k < first + count; ++k) if (needs_walk(c->v[k])) steps.push_back(k);
    return c->walk.begin(ctx, std::move(steps), wait, walk_launch_rounds(), pending, bad, first, count);
  });
}
int vdf_nova_circuits_release(vdf_circuits* c, size_t first, size_t count) {
  return nova_guard([&]() -> int {
    if (!c) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (first > c->v.size() || count > c->v.size() - first) return fail(VDF_ERR_BAD_LENGTH, "circuit range out of bounds");
    const int pending = c->walk.covers(first, count) ? c->walk.resolve(nullptr, 0, 0) : VDF_OK;
    for (size_t k = first; k < first + count; ++k) {
      if (!c->v[k].cp.empty()) c->walk.release(k, 1, false);            // a walked trace (one copied from the host stays)
      // a forward chain is a stream: a step that has been proved lets go of its pushed host trace too
      if (c->forward) std::vector<Fe>().swap(c->v[k].trace_xy);
    }
    return pending;
  });
}
int vdf_nova_circuits_memory(const vdf_circuits* c, size_t* resident_steps, uint64_t* device_bytes) {
  if (!c) return fail(VDF_ERR_BAD_ARG, "null argument");
  c->walk.memory(c->v.size(), resident_steps, device_bytes);
  return VDF_OK;
}
int vdf_nova_circuit_trace(const vdf_circuits* c, size_t k, const void** d_trace) {
  return nova_guard([&]() -> int {
    if (!c || !d_trace) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (k >= c->v.size()) return fail(VDF_ERR_BAD_LENGTH, "circuit index out of range");
    *d_trace = nullptr;
    if (c->walk.covers(k)) { int rc = c->walk.resolve(nullptr, 0, 0); if (rc != VDF_OK && rc != VDF_ERR_BAD_ARG) return rc; }
    *d_trace = c->v[k].d_trace;
    return VDF_OK;
  });
}
int vdf_nova_circuits_upload(vdf_ctx* ctx, vdf_circuits* c) {
  if (ctx && c && c->checkpoints) return vdf_nova_circuits_materialize(ctx, c, 0, c->v.size(), 1, nullptr);
  return nova_guard([&]() -> int {
    if (!ctx || !c) return fail(VDF_ERR_BAD_ARG, "null argument");
    c->walk.home = ctx;
    for (auto& k : c->v) {                          // a block per circuit
      if (k.d_trace) continue;
      std::shared_ptr<TraceBlock> b(new TraceBlock{ctx, k.trace_xy.size() * 32});
      HIPCALL(ctx, vdf_dev_alloc(ctx, b->bytes, &b->d));
      k.d_trace = b->d; k.block = std::move(b);
      HIPCALL(ctx, vdf_dev_memcpy(ctx, k.d_trace, k.trace_xy.data(), k.trace_xy.size() * 32));
    }
    return VDF_OK;
  });
}
size_t vdf_nova_circuits_len(const vdf_circuits* c) { return c ? c->v.size() : 0; }
int vdf_nova_circuit_states(const vdf_circuits* c, size_t k, vdf_state* result, vdf_state* input) {
  if (!c || k >= c->v.size()) return fail(VDF_ERR_BAD_LENGTH, "circuit index out of range");
  if (result) store_state(result, c->v[k].result);
  if (input) store_state(input, c->v[k].input);
  return VDF_OK;
}
int vdf_nova_circuits_host_bytes(const vdf_circuits* c, uint64_t* bytes) {
  if (!c || !bytes) return fail(VDF_ERR_BAD_ARG, "null argument");
  uint64_t n = 0;
  for (const Circuit& k : c->v) n += k.trace_xy.size() * 32 + k.cp.size() * 96;
  *bytes = n;
  return VDF_OK;
}
void vdf_nova_circuits_free(vdf_circuits* c) {
  if (!c) return;
  c->walk.teardown(c->v.size());
  delete c;
}
}  // extern "C"
