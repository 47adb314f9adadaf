// The walk window of libvdf_nova.so: device traces rebuilt from checkpoints on a side queue, one window ahead of the prover.  ONE
// implementation (trace_walks.cpp) of everything that does not depend on what is walked; the two owners -- vdf_circuits
// (circuits_host.cpp: inverse MinRoot walks) and vdf_custom_chain (custom_chain_host.cpp: a chain's walk tape) -- say what differs
// through WalkOwner.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>
#include "../../../include/vdf_nova.h"

// the one owner of a device trace: the traces one materialize call built, or the one vdf_nova_circuits_upload copied; freed when
// the last step that points into it lets go
struct TraceBlock {
  vdf_ctx* ctx;
  uint64_t bytes;
  void* d = nullptr;
  ~TraceBlock() { if (d) vdf_dev_free(ctx, d); }
};
// a step's trace in HBM: null, or inside `block` (what Circuit and a custom chain's step both are to the walks)
struct TraceSlot {
  void* d_trace = nullptr;
  std::shared_ptr<TraceBlock> block;
};

namespace vdfnova {
// THE slicing rule: the next launch of walks that have `done` of `every` rounds behind them runs min(every - done, launch_rounds
// (0: 1,024), budget (0: no bound)) rounds from entry top = every - done; last: it reaches the checkpoint (vdf_nova_custom_chain_slice)
void walk_slice(uint64_t every, uint64_t launch_rounds, uint64_t done, uint64_t budget, uint64_t* rounds, uint64_t* top, int* last);

// Traces being rebuilt: one walk per checkpoint interval (and lane) of every step in `steps`, all in one launch per slice of
// rounds; `done` rounds of `every` are enqueued so far.  Trace li of `block` is step steps[li]'s.
struct WalkJob {
  std::vector<size_t> steps;               // step indices, ascending
  std::shared_ptr<TraceBlock> block;       // steps.size() traces of trace_bytes
  size_t walks = 0;                        // steps.size() * step_walks; 0 (and every = 0): traces the owner's setup uploads, nothing walked
  uint64_t done = 0, launch_rounds = 0;    // launch_rounds: the bound of walk_slice
  // what the owner says of a job (WalkOwner::shape)
  uint64_t every = 0, trace_bytes = 0;     // rounds per walk; bytes of a step's trace
  size_t step_walks = 0, entry_bytes = 0;  // walks per step (lanes * t / every); bytes of a walk's state: 96 (vdf_state), n_adv * 32
};
// where each walk stands, the checkpoint it must land on, and (pinned) 1 per walk that landed on it
struct WalkScratch {
  void* d_walk = nullptr, *d_expect = nullptr;
  int32_t* h_ok = nullptr;
  size_t walks = 0;                        // the walks these three have room for
};
// What differs between the two owners.  Every device call of a hook goes to the side queue `q` it is handed.
struct WalkOwner {
  const char* whose;                       // "circuits'" / "chain's": "the ... traces live on another device"
  const char* noun;                        // "circuits" / "steps": "the traces of 3 ... do not fit"
  virtual TraceSlot& slot(size_t k) = 0;
  virtual void shape(size_t first_step, WalkJob* j) = 0;     // every, trace_bytes, step_walks, entry_bytes of a job that begins there
  // two host runs of walks * entry_bytes, in the walks' order: where they start and where they must land.  They stay as they are
  // until unstage(), which follows the synchronisation that resolves the job.
  virtual void stage_walks(const WalkJob& j, const void** starts, const void** expects) = 0;
  virtual void unstage() {}
  virtual int setup(vdf_ctx* q, const WalkJob& j, const WalkScratch& s) { return VDF_OK; }    // once per job, behind the uploads
  virtual int launch(vdf_ctx* q, const WalkJob& j, const WalkScratch& s, uint64_t rounds, uint64_t top, int last) = 0;
  virtual int finish(vdf_ctx* q, const WalkJob& j, const WalkScratch& s) { return VDF_OK; }   // once per job, behind its last launch
  virtual std::string missed(size_t k, size_t walk) = 0;     // the message: walk `walk` of step k (the step's first that missed)
 protected:
  WalkOwner(const char* whose, const char* noun) : whose(whose), noun(noun) {}
  ~WalkOwner() {}
};

// The walks of one owner: on a side queue of the device (made by the first job), a job begun with wait = 0 being finished by the next
// call that needs its result.  Their buffers are kept from one job to the next, and a windowed prover keeps the allocation of the
// window it releases for the window after next (`spare`): a device free is a synchronisation of the whole device, and two per
// window showed in the prover's rate.
class TraceWalks {
 public:
  explicit TraceWalks(WalkOwner* owner) : owner(owner) {}
  vdf_ctx* home = nullptr;                 // where the traces live
  bool covers(size_t first, size_t count = 1) const;        // the pending job builds a trace of steps [first, first + count)
  bool resident(size_t k) const { return owner->slot(k).d_trace != nullptr; }
  // A materialize call after its argument checks and resolve(): `pending` is that verdict, carried when it is VDF_ERR_BAD_ARG and
  // returned once the new job is begun.  The job covers `steps` (ascending; none: nothing to do); its traces come from the spare when
  // that is exactly their size, else from the device after a look at its free memory.  wait = 0 enqueues one slice, else resolves.
  int begin(vdf_ctx* ctx, std::vector<size_t> steps, int wait, uint64_t launch_rounds, int pending, int* bad, size_t bad_first, size_t bad_count);
  // up to `budget` more rounds of the pending walks (0: all that are left), in launches cut by walk_slice
  int enqueue(uint64_t budget);
  // finish the pending walks: the rest of their rounds, the comparison, one synchronisation, the verdict per step.  A step whose
  // walk missed loses its trace (bad[k - bad_first] = 1 inside the caller's range); after a device failure every step of the job does.
  int resolve(int* bad, size_t bad_first, size_t bad_count);
  // Called by the step that proves k, when the pending walks are wanted by the step that proves their first step less `lead`: the
  // calls from here to there share the remaining rounds evenly.
  int pump(size_t k, size_t lead);
  // steps [first, first + count) let go of their traces; park: an allocation left to nobody becomes the spare
  void release(size_t first, size_t count, bool park);
  void drop_spare() { spare.reset(); }
  // of the owner's first `slots` steps: those with a trace, and the bytes behind them -- each block once, plus the spare
  void memory(size_t slots, size_t* resident_steps, uint64_t* device_bytes) const;
  // the end of the owner: the queue drained if a job is pending, the spare and the buffers freed, the slots let go, the queue destroyed
  void teardown(size_t slots);

 private:
  WalkOwner* const owner;
  vdf_ctx* side = nullptr;
  std::unique_ptr<WalkJob> job;
  WalkScratch s;
  std::shared_ptr<TraceBlock> spare;
  void scratch_free();
  int scratch_ensure(size_t walks, size_t entry_bytes);
  void lose(size_t k) { owner->slot(k) = TraceSlot(); }      // left without a trace
};
}  // namespace vdfnova
