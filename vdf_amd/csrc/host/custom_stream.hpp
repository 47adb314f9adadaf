// The evaluator of vdf_nova_eval_and_prove_custom (custom_stream_host.cpp): one thread per lane runs the host restatement of the
// chain's forward tape step by step, and finished steps wait in a bounded queue for the thread that proves them.  It knows no
// vdf_pp and touches no device, so tools/host_custom_stream_check.cpp drives it alone under the sanitizers.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../../include/vdf_nova.h"

namespace vdfnova {
class ChainEvaluator {
 public:
  // tape, inv and j_base are the caller's and outlive the evaluator; inv: lanes * tape->n_inv (NULL for n_inv = 0).
  // every = 0: a step is handed over as lanes traces of t + 1 entries; else as lanes runs of t / every + 1 checkpoints.
  struct Spec {
    int field;
    const vdf_round_tape* tape;
    const vdf_fe* inv;
    uint64_t t, every;
    size_t lanes;
    const uint64_t* j_base;
    size_t num_steps;
    size_t queue_steps;                    // at most this many finished steps wait (a lane runs no further ahead of the taker)
  };
  // One finished step: lanes runs of entries() entries of n_adv elements, lane-major, each starting on the entry the step before ended on.
  typedef std::vector<vdf_fe> Step;

  ChainEvaluator(const Spec& spec, const vdf_fe* initial);          // initial: lanes * n_adv, copied; no thread yet
  ~ChainEvaluator();                                                 // stop() and join: no thread outlives the object
  ChainEvaluator(const ChainEvaluator&) = delete;
  ChainEvaluator& operator=(const ChainEvaluator&) = delete;

  size_t entries() const { return spec.every ? (size_t)(spec.t / spec.every) + 1 : (size_t)spec.t + 1; }
  void start();                                                      // the lanes' threads begin (once)
  // Moves every finished step, in order, to the end of *out.  wait: blocks until there is at least one, unless all num_steps have been
  // taken, the evaluator was stopped or a lane failed.  A lane's failure is this call's return value from then on (its message in
  // *why); VDF_OK otherwise.
  int take(std::vector<Step>* out, bool wait, std::string* why);
  void stop();                                                       // the lanes end after the round slice they are in; idempotent
  void join();
  // from start() to the last lane's last round, and that instant on now_ms()'s clock; 0 until then
  void eval_times(double* eval_ms, double* eval_end);

 private:
  struct Slot { Step data; size_t lanes_done = 0; };
  void lane_main(size_t l);
  const Spec spec;
  std::vector<vdf_fe> initial;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Slot> ready;                  // ready[i]: step taken + i
  size_t taken = 0, last_done = 0;
  bool stopped = false, started = false;
  int err = 0;
  std::string err_msg;
  double t_begin = 0, t_end = 0;
  std::vector<std::thread> threads;
};
}  // namespace vdfnova
