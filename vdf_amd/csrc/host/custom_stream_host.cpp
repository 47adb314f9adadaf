// libvdf_nova.so, part 2d: a custom chain proved while it is evaluated (vdf_nova_eval_and_prove_custom, include/vdf_nova.h) -- what
// vdf_nova_eval_and_prove is to the built-in forward circuit.  ChainEvaluator (custom_stream.hpp) evaluates on threads of its own,
// the calling thread grows a vdf_custom_chain (custom_chain_host.cpp) by what they finish, proves and releases.
#include "nova_internal.hpp"
#include "../tape_launch.h"
#include "custom_stream.hpp"

using namespace vdfnova;

namespace vdfnova {
ChainEvaluator::ChainEvaluator(const Spec& sp, const vdf_fe* init) : spec(sp), initial(init, init + sp.lanes * sp.tape->n_adv) {}
ChainEvaluator::~ChainEvaluator() { stop(); join(); }

void ChainEvaluator::start() {
  {
    std::lock_guard<std::mutex> lk(mu);
    if (started) return;
    started = true;
    t_begin = now_ms();
  }
  for (size_t l = 0; l < spec.lanes; ++l) threads.emplace_back([this, l] { lane_main(l); });
}
void ChainEvaluator::stop() {
  { std::lock_guard<std::mutex> lk(mu); stopped = true; }
  cv.notify_all();
}
void ChainEvaluator::join() {
  for (std::thread& th : threads) if (th.joinable()) th.join();
}
void ChainEvaluator::eval_times(double* eval_ms, double* eval_end) {
  std::lock_guard<std::mutex> lk(mu);
  if (eval_ms) *eval_ms = t_end ? t_end - t_begin : 0;
  if (eval_end) *eval_end = t_end;
}

// Lane l, step by step: t rounds from where it stands, in slices one launch of the tape may run (the restatement keeps the device
// path's work cap), into a trace of its own; what is handed over is copied into the step's slot once the queue has room for it.
void ChainEvaluator::lane_main(size_t l) {
  const size_t na = spec.tape->n_adv, n = entries(), stride = spec.every ? (size_t)spec.every : 1;
  const uint64_t bound = std::max<uint64_t>(1, vdflaunch::forward_launch_bound(spec.tape));
  const Fe* inv = spec.tape->n_inv ? (const Fe*)spec.inv + l * spec.tape->n_inv : nullptr;
  std::vector<Fe> trace(((size_t)spec.t + 1) * na), stand((const Fe*)initial.data() + l * na, (const Fe*)initial.data() + (l + 1) * na);
  auto failed = [&](int rc, const std::string& msg) {
    { std::lock_guard<std::mutex> lk(mu); if (!err) { err = rc; err_msg = "lane " + std::to_string(l) + ": " + msg; } stopped = true; }
    cv.notify_all();
  };
  try {
    for (size_t k = 0; k < spec.num_steps; ++k) {
      std::copy(stand.begin(), stand.end(), trace.begin());
      for (uint64_t done = 0; done < spec.t;) {
        { std::lock_guard<std::mutex> lk(mu); if (stopped) return; }
        const uint64_t now = std::min(bound, spec.t - done);
        const int rc = eval_forward_tape(spec.field, spec.tape, inv, stand.data(), 1, now, nullptr, 0, 0, trace.data(), 0, done,
                                         spec.j_base[l] + (uint64_t)k * spec.t, 0);
        if (rc != VDF_OK) return failed(rc, vdf_nova_last_error());
        done += now;
      }
      std::unique_lock<std::mutex> lk(mu);
      if (k + 1 == spec.num_steps && ++last_done == spec.lanes) t_end = now_ms();      // the chain's output exists from here
      cv.wait(lk, [&] { return stopped || k < taken + spec.queue_steps; });
      if (stopped) return;
      while (ready.size() <= k - taken) ready.emplace_back();
      Slot& s = ready[k - taken];
      if (s.data.empty()) s.data.resize(spec.lanes * n * na);
      for (size_t e = 0; e < n; ++e) memcpy(&s.data[(l * n + e) * na], &trace[e * stride * na], na * 32);
      ++s.lanes_done;
      lk.unlock();
      cv.notify_all();
    }
  } catch (const std::exception& ex) { failed(VDF_ERR_OOM, ex.what()); }
}

int ChainEvaluator::take(std::vector<Step>* out, bool wait, std::string* why) {
  std::unique_lock<std::mutex> lk(mu);
  auto front_done = [&] { return !ready.empty() && ready.front().lanes_done == spec.lanes; };
  if (wait) cv.wait(lk, [&] { return front_done() || stopped || err || taken == spec.num_steps; });
  if (err) { if (why) *why = err_msg; return err; }
  while (front_done()) {
    out->push_back(std::move(ready.front().data));
    ready.pop_front();
    ++taken;
  }
  lk.unlock();
  cv.notify_all();
  return VDF_OK;
}
}  // namespace vdfnova

extern "C" int vdf_nova_eval_and_prove_custom(vdf_pp* pp, const vdf_step_circuit* primary, const vdf_nova_custom_stream* s, const vdf_fe* initial,
                                              size_t num_steps, const vdf_fe* z0, vdf_fe* final_entries, vdf_proof** out,
                                              vdf_nova_stream_stats* stats) {
  return nova_guard([&]() -> int {
    if (!out) return fail(VDF_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (!pp || !primary || !primary->synthesize || !s || !s->forward_tape || !initial || !z0 || !s->j_base) return fail(VDF_ERR_BAD_ARG, "null argument");
    if (num_steps == 0) return fail(VDF_ERR_BAD_ARG, "num_steps must be > 0");
    if (pp->circuit_kind != VDF_CIRCUIT_CUSTOM) return fail(VDF_ERR_BAD_ARG, "these parameters are not for a custom step circuit");
    if (s->every && (s->t == 0 || s->t % s->every != 0)) return fail(VDF_ERR_BAD_ARG, "`every` must divide t (0: whole traces are handed over)");
    if (s->walk_tape && s->walk_tape->n_adv != s->forward_tape->n_adv) return fail(VDF_ERR_BAD_ARG, "the walk tape's n_adv differs from the forward tape's");
    // the chain first: its refusals (field, t, lanes, the tape that rebuilds, a table's rows) come before any thread exists
    const vdf_round_tape* rebuild = s->walk_tape ? s->walk_tape : s->forward_tape;
    vdf_custom_chain* chain = nullptr;
    int rc = vdf_nova_custom_chain_begin(pp->field, rebuild, s->walk_tape ? VDF_CHAIN_DESCENDING : VDF_CHAIN_ASCENDING,
                                         s->walk_tape ? s->walk_inv : s->inv, s->t, s->lanes, initial, s->j_base, &chain);
    if (rc != VDF_OK) return rc;
    struct FreeChain { vdf_custom_chain* c; ~FreeChain() { vdf_nova_custom_chain_free(c); } } free_chain{chain};
    // ... and the evaluator's tape by the evaluator's own rules, with nothing to walk
    rc = eval_forward_tape(pp->field, s->forward_tape, (const Fe*)s->inv, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0, 0, 0, 0);
    if (rc != VDF_OK) return rc;
    // the evaluator's J is chain-global like the walks' (vdf_nova_custom_chain_begin)
    const std::string tab = tape_table_rows_fit_chain(s->forward_tape, s->t, s->lanes, s->j_base, "forward", "evaluator's");
    if (!tab.empty()) return fail(VDF_ERR_BAD_ARG, tab);
    constexpr size_t EVAL_QUEUE = 4;
    const size_t na = s->forward_tape->n_adv;
    // declared after the chain: whatever way this call ends, the lanes are told and joined first (no thread outlives the call)
    ChainEvaluator ev(ChainEvaluator::Spec{pp->field, s->forward_tape, s->inv, s->t, s->every, s->lanes, s->j_base, num_steps, EVAL_QUEUE}, initial);
    const size_t n = ev.entries();
    std::vector<vdf_fe> last(initial, initial + s->lanes * na);
    vdf_proof* p = nullptr;
    size_t pushed = 0, max_backlog = 0;
    ev.start();
    for (size_t k = 0; rc == VDF_OK && k < num_steps; ++k) {
      // everything the evaluator has finished goes into the chain (the step after this one then rides in this step's lookahead)
      std::vector<ChainEvaluator::Step> got;
      std::string why;
      rc = ev.take(&got, pushed <= k, &why);
      if (rc != VDF_OK) { fail(rc, "evaluator, " + why); break; }
      const size_t first = pushed;
      for (size_t g = 0; rc == VDF_OK && g < got.size(); ++g) {
        rc = s->every ? vdf_nova_custom_chain_push_checkpoints(chain, s->every, got[g].data(), n)
                      : vdf_nova_custom_chain_push_advice(chain, got[g].data(), n);
        if (rc != VDF_OK) break;
        ++pushed;
        for (size_t l = 0; l < s->lanes; ++l) memcpy(&last[l * na], &got[g][(l * n + n - 1) * na], na * 32);
      }
      got.clear();
      if (rc == VDF_OK && pushed <= k) rc = fail(VDF_ERR_DEVICE, "the evaluator ended before step " + std::to_string(k));
      max_backlog = std::max(max_backlog, pushed - std::min(pushed, k));
      if (rc == VDF_OK && pushed > first) rc = vdf_nova_custom_chain_materialize(pp->ctx, chain, first, pushed - first, 0, 0, nullptr);
      if (rc == VDF_OK) rc = vdf_nova_prove_step_custom_chain(pp, &p, primary, chain, k, z0);
      if (rc == VDF_OK) rc = vdf_nova_custom_chain_release(chain, k, 1);
    }
    if (rc == VDF_OK) rc = finalize_l2(p);
    const double t_done = now_ms();
    if (rc != VDF_OK) {
      const std::string why = vdf_nova_last_error();           // (freeing synchronises the lookahead's queues: before the chain goes)
      if (p) vdf_nova_proof_free(p);
      return fail(rc, why);
    }
    if (final_entries) memcpy(final_entries, last.data(), last.size() * sizeof(vdf_fe));
    if (stats) {
      double eval_ms = 0, eval_end = 0;
      ev.eval_times(&eval_ms, &eval_end);
      stats->eval_ms = eval_ms;
      stats->after_eval_ms = t_done - eval_end;
      stats->max_backlog = max_backlog;
      stats->steps = num_steps;
    }
    *out = p;
    return VDF_OK;
  });
}
