// libvdf_nova.so: uniform rounds of a custom step circuit (include/vdf_nova.h vdf_cs_repeat) -- the extension point of the
// reference's StepCircuit trait (/root/reference/src/nova/proof.rs:79-153) for rounds the GPU can run.  A body is recorded once
// (record_round_body), replayed over a constraint system with real calls (replay_round: the shape, and the witness from host
// advice), and compiled into the slot program libvdf_hip.so runs one repetition per thread (RoundRecord::ops; vdf_round_tape_run).
#include "nova_internal.hpp"
#include "rounds.hpp"
#include "../minroot_chain.h"
#include "../tape_launch.h"
#include "../periodic_rules.h"

using namespace vdfnova;
using namespace vdflaunch;

static_assert(VDF_POW_ACC == vdf::MR_ACC && VDF_POW_NONE == vdf::MR_NONE && sizeof(vdf_pow_step) == sizeof(vdf::MinrootChainStep),
              "vdf_pow_step is minroot_chain.h's step format made public");

namespace {
constexpr uint32_t REC_TAG = 0x80000000u;        // handles of a recording vdf_cs: REC_TAG | node -- no handle of another vdf_cs looks like one
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

// node of a handle the body owns, or -1 (and the failure flag)
long rec_node(vdf_cs* c, vdf_num h) {
  const uint32_t k = h & ~REC_TAG;
  // (a walk body is handed one entry: `next`, or the inputs a round body calls cur when it walks forward; the other is not its own)
  const uint32_t other = c->forward ? c->rec->in_next(0) : c->rec->in_cur(0);
  if ((h & REC_TAG) && k < c->rec->nodes.size() && !(c->walk && k >= other && k < other + c->rec->n_adv)) return (long)k;
  c->bad = true;
  return -1;
}
vdf_num rec_push(vdf_cs* c, uint8_t op, bool value_only, uint32_t a, uint32_t b, uint32_t cc) {
  if (++c->rec_calls > VDF_ROUND_MAX_OPS) { c->bad = true; return 0; }
  RecNode n;
  n.op = op; n.value_only = value_only; n.a = a; n.b = b; n.c = cc;
  c->rec->nodes.push_back(n);
  return REC_TAG | (uint32_t)(c->rec->nodes.size() - 1);
}
uint32_t rec_const(vdf_cs* c, const vdf_fe* k) {
  Fe v;
  memcpy(&v, k, 32);
  c->rec->consts.push_back(v);
  if (c->rec->consts.size() > VDF_ROUND_MAX_CONSTS) c->bad = true;
  return (uint32_t)(c->rec->consts.size() - 1);
}

// Inputs are loaded where they are first used, every value keeps its slot until its last use, and an operand that dies at an op
// gives its slot up before the result takes one (the kernel reads both operands before it writes).  A value that no variable
// depends on gets neither an op nor a slot.  alloc_from makes no value of its own: the variable is its source's slot, written out.
// outs (a walk body): what is written out is not the products but the nodes outs[c], column c, at the end of the tape -- a product
// is a value like any other, an output stays alive to the end, and an input that is passed straight through is loaded there.
int compile_round(RoundRecord& r, const std::vector<uint32_t>* outs = nullptr) {
  const size_t n = r.nodes.size(), nin = r.n_inputs();
  std::vector<uint32_t> root(n);
  for (size_t i = 0; i < n; ++i) root[i] = r.nodes[i].op == R_ALLOC_FROM ? root[r.nodes[i].a] : (uint32_t)i;
  auto operands = [&](const RecNode& x, uint32_t out[2]) -> int {
    switch (x.op) {
      case R_ADD: case R_SUB: case R_MUL: out[0] = root[x.a]; out[1] = root[x.b]; return 2;
      case R_SCALE: case R_ALLOC_FROM: case R_POW: case R_POWC: out[0] = root[x.a]; return 1;
      default: return 0;                            // inputs, constants; enforce costs the device nothing
    }
  };
  std::vector<char> needed(n, 0);
  std::vector<long> last_use(n, -1);
  if (outs) for (uint32_t o : *outs) { needed[o] = 1; last_use[o] = (long)n; }
  for (size_t i = n; i-- > nin;) {
    const RecNode& x = r.nodes[i];
    if (!outs && (x.op == R_MUL || x.op == R_ALLOC_FROM)) needed[i] = 1;
    if (!needed[i] || x.op == R_ENFORCE) continue;
    uint32_t o[2];
    const int k = operands(x, o);
    for (int q = 0; q < k; ++q) { needed[o[q]] = 1; if (last_use[o[q]] < (long)i) last_use[o[q]] = (long)i; }
  }
  std::vector<uint32_t> slot(n, NO_SLOT);
  std::vector<char> busy;
  auto take = [&]() -> uint32_t {
    for (size_t s = 0; s < busy.size(); ++s) if (!busy[s]) { busy[s] = 1; return (uint32_t)s; }
    busy.push_back(1);
    return (uint32_t)busy.size() - 1;
  };
  auto emit = [&](int op, uint32_t dst, uint32_t a, uint32_t b) {
    vdf_tape_op o;
    o.op = (uint8_t)op; o.dst = (uint8_t)dst; o.a = (uint8_t)a; o.b = (uint8_t)b;
    r.ops.push_back(o);
  };
  r.ops.clear();
  r.chain_tmp = 0;
  uint32_t var = 0;
  auto load_input = [&](uint32_t in) {
    if (in >= nin || slot[in] != NO_SLOT) return;
    slot[in] = take();
    if (in == r.in_j()) emit(VDF_TAPE_J, slot[in], 0, 0);
    else if (in < r.in_carry(0)) emit(VDF_TAPE_INV, slot[in], in - r.in_inv(0), 0);
    else if (in < r.in_cur(0)) emit(VDF_TAPE_ADV, slot[in], in - r.in_carry(0), 0);      // carry c IS advice entry j, column c
    else if (in < r.in_next(0)) emit(VDF_TAPE_ADV, slot[in], in - r.in_cur(0), 0);
    else emit(VDF_TAPE_ADV, slot[in], in - r.in_next(0), 1);
  };
  for (size_t i = nin; i < n; ++i) {
    const RecNode& x = r.nodes[i];
    if (x.op == R_ENFORCE || !needed[i]) continue;
    uint32_t o[2];
    const int k = operands(x, o);
    for (int q = 0; q < k; ++q) load_input(o[q]);      // inputs at their first use
    const uint32_t sa = k > 0 ? slot[o[0]] : 0, sb = k > 1 ? slot[o[1]] : 0;
    for (int q = 0; q < k; ++q)
      if (last_use[o[q]] == (long)i && !(q == 1 && o[1] == o[0])) busy[slot[o[q]]] = 0;
    switch (x.op) {
      case R_CONST: slot[i] = take(); emit(VDF_TAPE_CONST, slot[i], x.a, 0); break;
      case R_ADD: slot[i] = take(); emit(VDF_TAPE_ADD, slot[i], sa, sb); break;
      case R_SUB: slot[i] = take(); emit(VDF_TAPE_SUB, slot[i], sa, sb); break;
      case R_SCALE: slot[i] = take(); emit(VDF_TAPE_SCALE, slot[i], sa, x.b); break;
      case R_POW: slot[i] = take(); emit(VDF_TAPE_POW, slot[i], sa, x.b); break;
      case R_POWC: slot[i] = take(); emit(VDF_TAPE_POWC, slot[i], sa, x.b); if (x.c > r.chain_tmp) r.chain_tmp = x.c; break;
      case R_TAB: slot[i] = take(); emit(VDF_TAPE_TAB, slot[i], x.a, 0); break;
      case R_MUL: slot[i] = take(); emit(VDF_TAPE_MUL, slot[i], sa, sb); if (!outs) emit(VDF_TAPE_OUT, 0, slot[i], var++); break;
      default: emit(VDF_TAPE_OUT, 0, sa, var++); break;      // R_ALLOC_FROM
    }
    if (x.op != R_ALLOC_FROM && last_use[i] < 0) busy[slot[i]] = 0;      // a product nothing reads again
  }
  if (outs)
    for (uint32_t o : *outs) { load_input(o); emit(VDF_TAPE_OUT, 0, slot[o], var++); }
  r.n_slots = (uint32_t)busy.size();
  if (var != r.n_vars) return fail(VDF_ERR_DEVICE, "round tape: variable count drifted");
  if (r.n_slots > VDF_ROUND_MAX_LIVE) return fail(VDF_ERR_BAD_ARG, "the round body keeps more than VDF_ROUND_MAX_LIVE values alive at once");
  if (r.ops.size() > VDF_TAPE_MAX_OPS) return fail(VDF_ERR_BAD_ARG, "the round body compiles to more than VDF_TAPE_MAX_OPS device ops");
  return VDF_OK;
}
}  // namespace

static_assert(VDF_ROUND_MAX_LIVE == VDF_TAPE_MAX_SLOTS && VDF_ROUND_MAX_VARS == VDF_TAPE_MAX_VARS && VDF_ROUND_MAX_INV == VDF_TAPE_MAX_INV &&
              VDF_ROUND_MAX_ADV == VDF_TAPE_MAX_ADV && VDF_ROUND_MAX_CONSTS == VDF_TAPE_MAX_CONSTS, "the seam's caps are the kernel's");
static_assert(2 * VDF_ROUND_MAX_OPS + 1 + VDF_ROUND_MAX_INV + VDF_ROUND_MAX_CARRY + 2 * VDF_ROUND_MAX_ADV <= VDF_TAPE_MAX_OPS,
              "every body within the seam's caps fits the kernel's tape");

namespace vdfnova {

int record_round_body(CS* cs, const vdf_round_body* b, RoundRecord* out) {
  if (!b || !b->body) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: null body");
  if (b->n_inv > VDF_ROUND_MAX_INV || b->n_carry > VDF_ROUND_MAX_CARRY || b->n_adv > VDF_ROUND_MAX_ADV || b->n_adv == 0)
    return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: n_inv, n_carry or n_adv beyond its cap (VDF_ROUND_MAX_*), or no advice column");
  if (b->n_carry > b->n_adv) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: n_carry > n_adv (a carry's value is an advice column)");
  RoundRecord r;
  r.n_inv = (uint32_t)b->n_inv; r.n_carry = (uint32_t)b->n_carry; r.n_adv = (uint32_t)b->n_adv;
  r.nodes.resize(r.n_inputs());
  for (uint32_t k = 0; k < r.n_adv; ++k) r.nodes[r.in_cur(k)].value_only = r.nodes[r.in_next(k)].value_only = true;
  vdf_cs h;
  h.cs = cs;
  h.rec = &r;
  std::vector<vdf_num> hin(r.n_inputs()), hout(r.n_carry ? r.n_carry : 1, 0);
  for (uint32_t k = 0; k < r.n_inputs(); ++k) hin[k] = REC_TAG | k;
  const int rc = b->body(b->self, &h, hin[r.in_j()], hin.data() + r.in_inv(0), hin.data() + r.in_carry(0), hin.data() + r.in_cur(0),
                         hin.data() + r.in_next(0), hout.data());
  if (rc != 0) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: the round body failed");
  if (h.rec_calls > VDF_ROUND_MAX_OPS) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: more than VDF_ROUND_MAX_OPS calls in the round body");
  if (r.consts.size() > VDF_ROUND_MAX_CONSTS) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: more than VDF_ROUND_MAX_CONSTS constants in the round body");
  if (h.bad) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: the round body used a handle it does not own, a value-only handle in a constraint, or a call that is not recordable (a second table of vdf_cs_tab included)");
  for (uint32_t k = 0; k < r.n_carry; ++k) {
    const long nd = rec_node(&h, hout[k]);
    if (nd < 0 || r.nodes[nd].value_only) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: carry_out holds a foreign or value-only handle");
    r.carry_out.push_back((uint32_t)nd);
  }
  for (const RecNode& x : r.nodes) {
    if (x.op == R_MUL || x.op == R_ALLOC_FROM) ++r.n_vars;
    if (x.op == R_MUL || x.op == R_ENFORCE) ++r.n_cons;
  }
  if (r.n_vars == 0) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: the round body makes no variable");
  if (r.n_vars > VDF_ROUND_MAX_VARS) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: more than VDF_ROUND_MAX_VARS variables per repetition");
  const int crc = compile_round(r);
  if (crc != VDF_OK) return crc;
  *out = std::move(r);
  return VDF_OK;
}

void replay_round(CS& cs, const RoundRecord& r, uint64_t j, const std::vector<Num>& inv, std::vector<Num>& carry, const Fe* cur, const Fe* next,
                  std::vector<Num>& v) {
  v.resize(r.nodes.size());
  v[r.in_j()] = cs.constant(from_u64(j, cs.F));
  for (uint32_t k = 0; k < r.n_inv; ++k) v[r.in_inv(k)] = inv[k];
  for (uint32_t k = 0; k < r.n_carry; ++k) {
    v[r.in_carry(k)] = std::move(carry[k]);
    if (cur) v[r.in_carry(k)].v = cur[k];
  }
  for (uint32_t k = 0; k < r.n_adv; ++k) {
    v[r.in_cur(k)] = cs.zero_num();
    v[r.in_next(k)] = cs.zero_num();
    if (cur) { v[r.in_cur(k)].v = cur[k]; v[r.in_next(k)].v = next[k]; }
  }
  for (size_t i = r.n_inputs(); i < r.nodes.size(); ++i) {
    const RecNode& x = r.nodes[i];
    switch (x.op) {
      case R_CONST: v[i] = cs.constant(r.consts[x.a]); break;
      case R_TAB: v[i] = cs.constant(r.tab_data()[(size_t)(j % r.tab_rows) * r.tab_cols + x.a]); break;      // what vdf_cs_const of that entry would make
      case R_ADD: v[i] = cs.add(v[x.a], v[x.b]); break;
      case R_SUB: v[i] = cs.sub(v[x.a], v[x.b]); break;
      case R_SCALE: v[i] = cs.scale(v[x.a], r.consts[x.b]); break;
      case R_MUL: v[i] = cs.mul(v[x.a], v[x.b]); break;
      case R_ALLOC_FROM: v[i] = cs.alloc(v[x.a].v); break;
      default: cs.enforce(v[x.a], v[x.b], v[x.c]); break;
    }
  }
  for (uint32_t k = 0; k < r.n_carry; ++k) carry[k] = v[r.carry_out[k]];
}

// ---- the host interpreter of round tapes: a restatement of rounds.hip's tape_round that shares no text with it (the GPU tests
// compare the device's bytes with this), only the rules: a call is checked ONCE by tape_launch.h (the tape by tape_rules.h behind
// it) -- what the launcher of its kind refuses, in the launcher's order, code and words -- then run without looking again.
static int refused(const Verdict& v) { return v.refused() ? fail(v.code, v.why) : VDF_OK; }

// x ^ e, e a plain integer: left to right from the top set bit, as the kernel does it (any order gives the same canonical value)
static Fe pow_plain(const Fe& x, const Fe& e, const Field& F) {
  int q = 3;
  while (q >= 0 && e.l[q] == 0) --q;
  if (q < 0) return one(F);
  Fe acc = x;
  for (int bit = 62 - __builtin_clzll(e.l[q]); q >= 0; --q, bit = 63)
    for (; bit >= 0; --bit) {
      acc = sqr(acc, F);
      if ((e.l[q] >> bit) & 1) acc = mul(acc, x, F);
    }
  return acc;
}

// x ^ E(chain): the chain's steps with the host's canonical sqr / mul -- the byte-for-byte reference of k_tape_forward_walk_chain,
// whose lazy values are these modulo m.  consts[b ..]: a packed chain tape_rules.h has accepted.
static Fe pow_chain_run(const Fe& x, const Fe* consts, size_t b, const Field& F) {
  const uint8_t* p = (const uint8_t*)(consts + b);
  const vdf_pow_step* st = (const vdf_pow_step*)(p + 4);
  Fe T[VDF_POW_CHAIN_MAX_TMP], v = x;
  T[0] = x;
  for (size_t k = 0; k < p[0]; ++k) {
    if (st[k].src != VDF_POW_ACC) v = T[st[k].src];
    for (unsigned q = st[k].squarings; q; --q) v = sqr(v, F);
    if (st[k].mul != VDF_POW_NONE) v = mul(v, T[st[k].mul], F);
    if (st[k].dst != VDF_POW_NONE) T[st[k].dst] = v;
  }
  return v;
}

// One round of a checked tape over the slot file s.  adv[b]: the advice entry an ADV with that b reads (the rules admit one b only
// in a walk: the entry stood on); out: where OUT writes (the repetition's variables, or the entry a walk's round produces).
static void run_tape_round(const vdf_round_tape* tp, const Field& F, uint64_t j, const Fe* inv, const Fe* const adv[2], Fe* s, Fe* out) {
  const Fe* consts = (const Fe*)tp->consts;
  for (size_t i = 0; i < tp->n_ops; ++i) {
    const vdf_tape_op& o = tp->ops[i];
    switch (o.op) {
      case VDF_TAPE_ADV: s[o.dst] = adv[o.b][o.a]; break;
      case VDF_TAPE_INV: s[o.dst] = inv[o.a]; break;
      case VDF_TAPE_J: s[o.dst] = from_u64(j, F); break;
      case VDF_TAPE_CONST: s[o.dst] = consts[o.a]; break;
      case VDF_TAPE_ADD: s[o.dst] = add(s[o.a], s[o.b], F); break;
      case VDF_TAPE_SUB: s[o.dst] = sub(s[o.a], s[o.b], F); break;
      case VDF_TAPE_MUL: s[o.dst] = mul(s[o.a], s[o.b], F); break;
      case VDF_TAPE_SCALE: s[o.dst] = mul(s[o.a], consts[o.b], F); break;
      case VDF_TAPE_POW: s[o.dst] = pow_plain(s[o.a], consts[o.b], F); break;
      case VDF_TAPE_POWC: s[o.dst] = pow_chain_run(s[o.a], consts, o.b, F); break;
      case VDF_TAPE_TAB: s[o.dst] = ((const Fe*)tp->table)[(size_t)(j % tp->tab_rows) * tp->tab_cols + o.a]; break;
      default: out[o.b] = s[o.a]; break;      // VDF_TAPE_OUT
    }
  }
}

// both round restatements: vdf_round_tape_run (kind RUN) is lanes = 1, its lane_stride unread; lane after lane
static int round_tape_lanes(int fid, Kind kind, const vdf_round_tape* tp, uint64_t t, size_t lanes, const Fe* inv, const Fe* advice,
                            size_t lane_stride, Fe* out) {
  if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
  if (!out || !advice) return fail(VDF_ERR_BAD_ARG, "null argument");
  const int rc = refused(round_launch(kind, tp, t, lanes, (const vdf_fe*)inv, lane_stride));
  if (rc != VDF_OK) return rc;
  const Field& F = field(fid);
  Fe s[VDF_TAPE_MAX_SLOTS];
  for (size_t l = 0; l < lanes; ++l)
    for (uint64_t j = 0; j < t; ++j) {
      const Fe* const adv[2] = {advice + (l * lane_stride + j) * tp->n_adv, advice + (l * lane_stride + j + 1) * tp->n_adv};
      run_tape_round(tp, F, j, inv + l * tp->n_inv, adv, s, out + (l * t + j) * tp->n_vars);
    }
  return VDF_OK;
}

int eval_round_tape(int fid, const vdf_round_tape* tp, uint64_t t, const Fe* inv, const Fe* advice, Fe* out) {
  return round_tape_lanes(fid, RUN, tp, t, 1, inv, advice, 0, out);
}

int eval_round_tape_lanes(int fid, const vdf_round_tape* tp, uint64_t t, size_t lanes, const Fe* inv, const Fe* advice, size_t lane_stride,
                          Fe* out) {
  return round_tape_lanes(fid, RUN_LANES, tp, t, lanes, inv, advice, lane_stride, out);
}

int record_walk_body(CS* cs, const vdf_walk_body* b, RoundRecord* out, bool forward) {
  if (!b || !b->body) return fail(VDF_ERR_BAD_ARG, "walk body: null body");
  if (b->n_inv > VDF_ROUND_MAX_INV || b->n_adv > VDF_ROUND_MAX_ADV || b->n_adv == 0)
    return fail(VDF_ERR_BAD_ARG, "walk body: n_inv or n_adv beyond its cap (VDF_ROUND_MAX_*), or no advice column");
  RoundRecord r;
  r.n_inv = (uint32_t)b->n_inv; r.n_adv = (uint32_t)b->n_adv;
  r.nodes.resize(r.n_inputs());
  vdf_cs h;
  h.cs = cs;
  h.rec = &r;
  h.walk = true;
  h.forward = forward;
  std::vector<vdf_num> hin(r.n_inputs()), hout(r.n_adv, 0);
  for (uint32_t k = 0; k < r.n_inputs(); ++k) hin[k] = REC_TAG | k;
  // (the entry stood on: entry j + 1 descending, entry j ascending -- the inputs compile_round loads with ADV b = 1 and b = 0)
  const int rc = b->body(b->self, &h, hin[r.in_j()], hin.data() + r.in_inv(0), hin.data() + (forward ? r.in_cur(0) : r.in_next(0)), hout.data());
  if (rc != 0) return fail(VDF_ERR_BAD_ARG, "walk body: the body failed");
  if (h.rec_calls > VDF_ROUND_MAX_OPS) return fail(VDF_ERR_BAD_ARG, "walk body: more than VDF_ROUND_MAX_OPS calls");
  if (r.consts.size() > VDF_ROUND_MAX_CONSTS) return fail(VDF_ERR_BAD_ARG, "walk body: more than VDF_ROUND_MAX_CONSTS constants");
  if (h.bad) return fail(VDF_ERR_BAD_ARG, "walk body: a handle the body does not own, or a call that is not value arithmetic (alloc, alloc_from, enforce, value, repeat; pow or pow_chain outside a forward body, an invalid chain, a second table of vdf_cs_tab)");
  std::vector<uint32_t> outs;
  for (uint32_t k = 0; k < r.n_adv; ++k) {
    const long nd = rec_node(&h, hout[k]);
    if (nd < 0) return fail(VDF_ERR_BAD_ARG, "walk body: cur_out holds a handle the body does not own");
    outs.push_back((uint32_t)nd);
  }
  r.n_vars = r.n_adv;
  const int crc = compile_round(r, &outs);
  if (crc != VDF_OK) return crc;
  if (r.n_slots + 2 * r.n_adv + r.chain_tmp > VDF_WALK_MAX_SLOTS)
    return fail(VDF_ERR_BAD_ARG, "walk body: live values + 2 * n_adv + the chains' temporaries > VDF_WALK_MAX_SLOTS");
  *out = std::move(r);
  return VDF_OK;
}

// both descending walks: vdf_round_tape_walk (kind WALK) is lanes = 1 under its own slot cap; group G = w / group is lane
// G % lanes of step G / lanes, with that lane's j_base and inv
static int walk_tape_lanes(int fid, Kind kind, const vdf_round_tape* tp, size_t lanes, const Fe* inv, Fe* entries, size_t n,
                           uint64_t rounds, Fe* trace, size_t walk_stride, size_t top, uint64_t group, uint64_t group_stride, const uint64_t* j_base,
                           uint64_t j_group_step, int heads, const Fe* expect, int32_t* ok) {
  if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
  const Verdict v = walk_launch({kind, tp, lanes, (const vdf_fe*)inv, j_base, n, rounds, entries, trace, walk_stride, top, group, heads, expect, ok, nullptr, 0});
  if (v.refused() || v.nothing) return refused(v);
  groups(n, &group, &group_stride);
  const Field& F = field(fid);
  const size_t na = tp->n_adv;
  Fe s[VDF_TAPE_MAX_SLOTS], stand[VDF_TAPE_MAX_ADV], prod[VDF_TAPE_MAX_ADV];
  const Fe* const adv[2] = {nullptr, stand};      // a descending walk stands on entry j + 1
  for (size_t w = 0; w < n; ++w) {
    const uint64_t G = w / group, first = (w % group) * walk_stride + top;
    const uint64_t g = G / lanes;
    const Fe* lane_inv = inv + (G % lanes) * tp->n_inv;
    Fe* tr = trace ? trace + (G * group_stride + first) * na : nullptr;
    uint64_t j = j_base[G % lanes] + g * j_group_step + first - 1;
    for (size_t c = 0; c < na; ++c) stand[c] = entries[w * na + c];
    for (uint64_t r = 0; r < rounds; ++r, --j) {
      if (tr) {
        for (size_t c = 0; c < na; ++c) tr[c] = stand[c];
        tr -= na;
      }
      run_tape_round(tp, F, j, lane_inv, adv, s, prod);
      for (size_t c = 0; c < na; ++c) stand[c] = prod[c];
    }
    for (size_t c = 0; c < na; ++c) entries[w * na + c] = stand[c];
    if (tr && heads && w % group == 0)
      for (size_t c = 0; c < na; ++c) tr[c] = stand[c];
    if (expect) ok[w] = memcmp(stand, expect + w * na, na * sizeof(Fe)) == 0;
  }
  return VDF_OK;
}

int eval_walk_tape(int fid, const vdf_round_tape* tp, const Fe* inv, Fe* entries, size_t n, uint64_t rounds, Fe* trace, size_t walk_stride,
                   size_t top, size_t group, size_t group_stride, uint64_t j_base, uint64_t j_group_step, int heads, const Fe* expect, int32_t* ok) {
  return walk_tape_lanes(fid, WALK, tp, 1, inv, entries, n, rounds, trace, walk_stride, top, group, group_stride, &j_base, j_group_step, heads,
                         expect, ok);
}

int eval_walk_tape_lanes(int fid, const vdf_round_tape* tp, size_t lanes, const Fe* inv, Fe* entries, size_t n, uint64_t rounds, Fe* trace,
                         size_t walk_stride, size_t top, size_t group, size_t group_stride, const uint64_t* j_base, uint64_t j_group_step,
                         int heads, const Fe* expect, int32_t* ok) {
  return walk_tape_lanes(fid, WALK_LANES, tp, lanes, inv, entries, n, rounds, trace, walk_stride, top, group, group_stride, j_base, j_group_step, heads,
                         expect, ok);
}

int eval_forward_tape(int fid, const vdf_round_tape* tp, const Fe* inv, Fe* entries, size_t n, uint64_t rounds, Fe* checkpoints, uint64_t every,
                      size_t cp_stride, Fe* trace, size_t walk_stride, uint64_t base, uint64_t j_base, uint64_t j_walk_step) {
  if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
  const Verdict v = walk_launch({FORWARD, tp, 1, (const vdf_fe*)inv, nullptr, n, rounds, entries, trace, walk_stride, base, 0, 0, nullptr, nullptr, checkpoints, every});
  if (v.refused() || v.nothing) return refused(v);
  const Field& F = field(fid);
  const size_t na = tp->n_adv;
  Fe s[VDF_TAPE_MAX_SLOTS], stand[VDF_TAPE_MAX_ADV], prod[VDF_TAPE_MAX_ADV];
  const Fe* const adv[2] = {stand, nullptr};      // a forward walk stands on entry j
  for (size_t w = 0; w < n; ++w) {
    uint64_t j = j_base + w * j_walk_step + base;
    for (size_t c = 0; c < na; ++c) stand[c] = entries[w * na + c];
    for (uint64_t r = 0; r < rounds; ++r, ++j) {
      run_tape_round(tp, F, j, inv, adv, s, prod);
      for (size_t c = 0; c < na; ++c) stand[c] = prod[c];
      const uint64_t g = base + r + 1;
      if (trace)
        for (size_t c = 0; c < na; ++c) trace[(w * walk_stride + g) * na + c] = stand[c];
      if (checkpoints && g % every == 0)
        for (size_t c = 0; c < na; ++c) checkpoints[(w * cp_stride + g / every) * na + c] = stand[c];
    }
    for (size_t c = 0; c < na; ++c) entries[w * na + c] = stand[c];
  }
  return VDF_OK;
}

// vdf_round_tape_rebuild_lanes on the host: the refusals and the whole of the index arithmetic are tape_launch.h's -- the statement
// the launcher and its kernel read
int eval_forward_tape_rebuild_lanes(int fid, const vdf_round_tape* tp, size_t lanes, const Fe* inv, Fe* entries, size_t n, uint64_t rounds,
                                    Fe* trace, size_t walk_stride, uint64_t base, size_t group, size_t group_stride, const uint64_t* j_base,
                                    uint64_t j_group_step, int heads, const Fe* expect, int32_t* ok) {
  if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
  const Verdict v = walk_launch({REBUILD, tp, lanes, (const vdf_fe*)inv, j_base, n, rounds, entries, trace, walk_stride, base, group, heads, expect, ok, nullptr, 0});
  if (v.refused() || v.nothing) return refused(v);
  uint64_t grp = group, gstride = group_stride;
  groups(n, &grp, &gstride);
  const Field& F = field(fid);
  const size_t na = tp->n_adv;
  Fe s[VDF_TAPE_MAX_SLOTS], stand[VDF_TAPE_MAX_ADV], prod[VDF_TAPE_MAX_ADV];
  const Fe* const adv[2] = {stand, nullptr};      // an ascending walk stands on entry j
  for (size_t w = 0; w < n; ++w) {
    const Place p = place(w, grp, walk_stride, base, (uint32_t)lanes);
    const Fe* lane_inv = inv + p.l * tp->n_inv;
    uint64_t j = counter(p, j_base[p.l], j_group_step);
    for (size_t c = 0; c < na; ++c) stand[c] = entries[w * na + c];
    if (trace && heads && p.first)
      for (size_t c = 0; c < na; ++c) trace[trace_entry(p, gstride, p.k) * na + c] = stand[c];
    for (uint64_t r = 0; r < rounds; ++r, ++j) {
      run_tape_round(tp, F, j, lane_inv, adv, s, prod);
      for (size_t c = 0; c < na; ++c) stand[c] = prod[c];
      if (trace)
        for (size_t c = 0; c < na; ++c) trace[trace_entry(p, gstride, p.k + r + 1) * na + c] = stand[c];
    }
    for (size_t c = 0; c < na; ++c) entries[w * na + c] = stand[c];
    if (expect) ok[w] = memcmp(stand, expect + w * na, na * sizeof(Fe)) == 0;
  }
  return VDF_OK;
}

}  // namespace vdfnova

// ---- periodic rows (rounds.hpp) ---------------------------------------------------------------------------------------------
namespace vdfnova {

bool detect_periodic_rows(const Coo m[3], const Field& F, size_t seg_begin, size_t n_vars, size_t row_begin, size_t n_cons, uint64_t t,
                          PeriodicRows* out) {
  if (n_cons == 0 || n_cons > VDF_PERIODIC_MAX_ROWS || n_vars == 0 || n_vars > UINT32_MAX || t < 2 || t > ((uint64_t)1 << 31) / n_cons) return false;
  typedef std::vector<std::pair<uint32_t, Fe>> Row;
  const size_t total = (size_t)t * n_cons;
  const uint64_t run_end = (uint64_t)seg_begin + t * (uint64_t)n_vars;
  std::vector<Row> got[3];
  for (int k = 0; k < 3; ++k) {
    got[k].resize(total);
    for (size_t e = 0; e < m[k].rows.size(); ++e)
      if (m[k].rows[e] >= row_begin && m[k].rows[e] - row_begin < total) got[k][m[k].rows[e] - row_begin].push_back({m[k].cols[e], canon(m[k].vals[e], F)});
    for (Row& g : got[k]) {
      std::sort(g.begin(), g.end(), [](const std::pair<uint32_t, Fe>& a, const std::pair<uint32_t, Fe>& b) { return a.first < b.first; });
      size_t w = 0;                                  // a column named twice counts once, with the sum
      for (size_t e = 0; e < g.size(); ++e)
        if (w && g[w - 1].first == g[e].first) g[w - 1].second = add(g[w - 1].second, g[e].second, F); else g[w++] = g[e];
      g.resize(w);
    }
  }
  for (uint64_t j0 = 0; j0 <= 4 && j0 + 2 <= t; ++j0) {
    PeriodicRows pr;
    pr.lead = j0; pr.n_cons = (uint32_t)n_cons; pr.n_vars = (uint32_t)n_vars;
    pr.row_begin = row_begin + (size_t)j0 * n_cons; pr.row_count = (size_t)(t - j0) * n_cons;
    pr.row_start.push_back(0);
    bool ok = true;
    auto konst = [&](const Fe& v) -> int {
      for (size_t q = 0; q < pr.consts.size(); ++q) if (pr.consts[q] == v) return (int)q;
      if (pr.consts.size() == VDF_PERIODIC_MAX_CONSTS) return -1;
      pr.consts.push_back(v);
      return (int)pr.consts.size() - 1;
    };
    const int64_t base0 = (int64_t)(seg_begin + j0 * n_vars);
    for (size_t c = 0; c < n_cons && ok; ++c)
      for (int k = 0; k < 3 && ok; ++k) {
        const Row& ra = got[k][j0 * n_cons + c];
        const Row& rb = got[k][(j0 + 1) * n_cons + c];
        if (ra.size() > VDF_PERIODIC_MAX_ROW_TERMS || pr.terms.size() + ra.size() > VDF_PERIODIC_MAX_TERMS) { ok = false; break; }
        for (const auto& e : ra) {
          vdf_periodic_term tm;
          tm.pad = 0; tm.c1 = VDF_TERM_NO_SLOPE;
          const int k0 = konst(e.second);
          if (k0 < 0) { ok = false; break; }
          tm.c0 = (uint8_t)k0;
          if (e.first >= seg_begin && e.first < run_end) {
            const int64_t rel = (int64_t)e.first - base0;
            if (rel < INT32_MIN || rel > INT32_MAX) { ok = false; break; }
            tm.kind = VDF_TERM_SEG; tm.col = (uint32_t)(int32_t)rel;
          } else {
            tm.kind = VDF_TERM_ABS; tm.col = e.first;
            const auto it = std::lower_bound(rb.begin(), rb.end(), e.first, [](const std::pair<uint32_t, Fe>& a, uint32_t col) { return a.first < col; });
            if (it == rb.end() || it->first != e.first) { ok = false; break; }
            const Fe slope = sub(it->second, e.second, F);
            if (!slope.is_zero()) {
              const int k1 = konst(slope);
              if (k1 < 0) { ok = false; break; }
              tm.c1 = (uint8_t)k1;
            }
          }
          pr.terms.push_back(tm);
        }
        pr.row_start.push_back((uint16_t)pr.terms.size());
      }
    if (!ok) continue;
    // every triple of every repetition j0 .. t - 1 against the pattern
    std::vector<Fe> coef(pr.terms.size());
    for (size_t e = 0; e < pr.terms.size(); ++e) coef[e] = pr.consts[pr.terms[e].c0];
    Row want;
    for (uint64_t j = j0; j < t && ok; ++j) {
      const int64_t base = (int64_t)(seg_begin + j * n_vars);
      for (size_t c = 0; c < n_cons && ok; ++c)
        for (int k = 0; k < 3 && ok; ++k) {
          const Row& g = got[k][j * n_cons + c];
          const size_t b = pr.row_start[3 * c + k], e = pr.row_start[3 * c + k + 1];
          if (g.size() != e - b) { ok = false; break; }
          want.clear();
          for (size_t q = b; q < e; ++q) {
            const vdf_periodic_term& tm = pr.terms[q];
            const int64_t col = tm.kind == VDF_TERM_SEG ? base + (int32_t)tm.col : (int64_t)tm.col;
            if (col < 0 || col > (int64_t)UINT32_MAX) { ok = false; break; }
            want.push_back({(uint32_t)col, coef[q]});
          }
          if (!ok) break;
          std::sort(want.begin(), want.end(), [](const std::pair<uint32_t, Fe>& x, const std::pair<uint32_t, Fe>& y) { return x.first < y.first; });
          for (size_t q = 0; q < g.size(); ++q)
            if (g[q].first != want[q].first || g[q].second != want[q].second) { ok = false; break; }
        }
      for (size_t e = 0; e < pr.terms.size(); ++e)
        if (pr.terms[e].c1 != VDF_TERM_NO_SLOPE) coef[e] = add(coef[e], pr.consts[pr.terms[e].c1], F);
    }
    if (!ok) continue;
    pr.valid = true;
    *out = std::move(pr);
    return true;
  }
  return false;
}

int eval_periodic_rows(int fid, const vdf_periodic_rows* pr, uint64_t j_first, uint64_t reps, size_t seg_begin, size_t row_begin,
                       size_t num_cols, size_t num_cons, const Fe* z2, const Fe* az1, const Fe* bz1, const Fe* cz1, const Fe* u1, Fe* az2,
                       Fe* bz2, Fe* cz2, Fe* T) {
  if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
  if (!z2 || !az1 || !bz1 || !cz1 || !u1 || !az2 || !bz2 || !cz2 || !T) return fail(VDF_ERR_BAD_ARG, "null argument");
  bool nothing = false;
  const std::string why = vdfperiodic::refuse(pr, j_first, reps, seg_begin, row_begin, num_cols, num_cons, &nothing);
  if (!why.empty()) return fail(VDF_ERR_BAD_ARG, why);
  if (nothing) return VDF_OK;
  const uint64_t rows = reps * pr->n_cons;
  const Field& F = field(fid);
  const Fe* consts = (const Fe*)pr->consts;
  for (uint64_t i = 0; i < rows; ++i) {
    const uint64_t j = j_first + i / pr->n_cons;
    const uint32_t c = (uint32_t)(i % pr->n_cons);
    const size_t r = row_begin + i;
    Fe acc[3];
    for (int k = 0; k < 3; ++k) {
      acc[k] = zero();
      for (uint32_t q = pr->row_start[3 * c + k]; q < pr->row_start[3 * c + k + 1]; ++q) {
        const vdf_periodic_term& t = pr->terms[q];
        const size_t col = t.kind == VDF_TERM_SEG ? (size_t)((int64_t)(seg_begin + j * pr->n_vars) + (int32_t)t.col) : (size_t)t.col;
        Fe coef = consts[t.c0];
        if (t.c1 != VDF_TERM_NO_SLOPE) coef = add(coef, mul(from_u64(j - pr->j0, F), consts[t.c1], F), F);
        acc[k] = add(acc[k], mul(coef, z2[col], F), F);
      }
    }
    az2[r] = acc[0]; bz2[r] = acc[1]; cz2[r] = acc[2];
    Fe tt = add(mul(az1[r], acc[1], F), mul(acc[0], bz1[r], F), F);
    tt = sub(tt, mul(*u1, acc[2], F), F);
    T[r] = sub(tt, cz1[r], F);
  }
  return VDF_OK;
}

}  // namespace vdfnova

// ---- the recording side of the vdf_cs_* calls (nova_host.cpp hands a call over when the handle records) ------------------
namespace vdfnova {
vdf_num rec_cs_const(vdf_cs* c, const vdf_fe* k) {
  if (!k) { c->bad = true; return 0; }
  return rec_push(c, R_CONST, false, rec_const(c, k), 0, 0);
}
vdf_num rec_cs_bin(vdf_cs* c, int op, vdf_num a, vdf_num b) {
  const long x = rec_node(c, a), y = rec_node(c, b);
  if (x < 0 || y < 0) return 0;
  const bool vo = c->rec->nodes[x].value_only || c->rec->nodes[y].value_only;      // (never set in a walk body: a product there is a value)
  if (op == R_MUL && vo) { c->bad = true; return 0; }      // a constraint over a value without a linear combination
  return rec_push(c, (uint8_t)op, vo, (uint32_t)x, (uint32_t)y, 0);
}
vdf_num rec_cs_scale(vdf_cs* c, vdf_num a, const vdf_fe* k) {
  const long x = rec_node(c, a);
  if (x < 0 || !k) { c->bad = true; return 0; }
  return rec_push(c, R_SCALE, c->rec->nodes[x].value_only, (uint32_t)x, rec_const(c, k), 0);
}
vdf_num rec_cs_pow(vdf_cs* c, vdf_num a, const uint64_t e[4]) {
  if (!c->forward || !e) { c->bad = true; return 0; }      // a power inside a circuit would need constraints: the circuit author's business
  const long x = rec_node(c, a);
  if (x < 0) return 0;
  vdf_fe k;
  memcpy(&k, e, 32);
  return rec_push(c, R_POW, false, (uint32_t)x, rec_const(c, &k), 0);
}
// the chain goes into the constants as vdf_hip.h lays it out: pow_chain.h packs it, and checks it first
vdf_num rec_cs_pow_chain(vdf_cs* c, vdf_num a, const vdf_pow_step* steps, size_t n_steps) {
  if (!c->forward) { c->bad = true; return 0; }
  vdfpow::ChainInfo ci;
  if (!vdfpow::check(steps, n_steps, 0, &ci).empty()) { c->bad = true; return 0; }
  const long x = rec_node(c, a);
  if (x < 0) return 0;
  vdf_fe k[(4 + 4 * VDF_POW_CHAIN_MAX_STEPS + 31) / 32];
  vdfpow::pack(steps, n_steps, ci.n_tmp, (uint8_t*)k);
  const size_t nk = vdfpow::packed_consts(n_steps);
  const uint32_t first = rec_const(c, &k[0]);
  for (size_t q = 1; q < nk; ++q) rec_const(c, &k[q]);
  return rec_push(c, R_POWC, false, (uint32_t)x, first, ci.n_tmp);
}
// one table per body: the first call names it (nothing is copied); every later call must name the same (pointer, rows, cols)
vdf_num rec_cs_tab(vdf_cs* c, const vdf_fe* table, size_t rows, size_t cols, size_t col) {
  RoundRecord& r = *c->rec;
  if (!table || rows == 0 || rows > VDF_TAPE_MAX_TAB_ROWS || cols == 0 || cols > VDF_TAPE_MAX_TAB_COLS || col >= cols) { c->bad = true; return 0; }
  if (r.tab_rows == 0) {
    r.tab_src = table; r.tab_rows = (uint32_t)rows; r.tab_cols = (uint32_t)cols;
  } else if (r.tab_src != table || r.tab_rows != rows || r.tab_cols != cols) { c->bad = true; return 0; }
  return rec_push(c, R_TAB, false, (uint32_t)col, 0, 0);
}
int rec_cs_enforce(vdf_cs* c, vdf_num a, vdf_num b, vdf_num cc) {
  if (c->walk) { c->bad = true; return VDF_ERR_BAD_ARG; }      // a walk body computes values: it has nothing to constrain
  const long x = rec_node(c, a), y = rec_node(c, b), z = rec_node(c, cc);
  if (x < 0 || y < 0 || z < 0) return VDF_ERR_BAD_ARG;
  const std::vector<RecNode>& nd = c->rec->nodes;
  if (nd[x].value_only || nd[y].value_only || nd[z].value_only) { c->bad = true; return VDF_ERR_BAD_ARG; }
  rec_push(c, R_ENFORCE, false, (uint32_t)x, (uint32_t)y, (uint32_t)z);
  return c->bad ? VDF_ERR_BAD_ARG : VDF_OK;
}
}  // namespace vdfnova

namespace vdfnova {
void periodic_rows_export(const PeriodicRows& pr, uint16_t* row_start, vdf_periodic_term* terms, vdf_fe* consts, vdf_periodic_rows* out,
                          uint64_t* lead, uint64_t* first_row, uint64_t* row_count) {
  memcpy(row_start, pr.row_start.data(), pr.row_start.size() * sizeof(uint16_t));
  if (!pr.terms.empty()) memcpy(terms, pr.terms.data(), pr.terms.size() * sizeof(vdf_periodic_term));
  if (!pr.consts.empty()) memcpy(consts, pr.consts.data(), pr.consts.size() * 32);
  *out = pr.view();
  out->row_start = row_start; out->terms = terms; out->consts = consts;
  if (lead) *lead = pr.lead;
  if (first_row) *first_row = pr.row_begin;
  if (row_count) *row_count = pr.row_count;
}
}  // namespace vdfnova

extern "C" {

vdf_num vdf_cs_alloc_from(vdf_cs* c, vdf_num src) {
  if (!c) return 0;
  if (c->rec) {
    if (c->walk) { c->bad = true; return 0; }          // a walk body makes no variable
    const long x = rec_node(c, src);
    return x < 0 ? 0 : rec_push(c, R_ALLOC_FROM, false, (uint32_t)x, 0, 0);
  }
  if (src >= c->pool.size()) { c->bad = true; return 0; }
  const Fe v = c->pool[src].v;
  c->pool.push_back(c->cs->alloc(c->cs->shape ? zero() : v));
  return (vdf_num)(c->pool.size() - 1);
}

vdf_num vdf_cs_pow(vdf_cs* c, vdf_num a, const uint64_t e[4]) {
  if (!c) return 0;
  if (c->rec) return rec_cs_pow(c, a, e);
  c->bad = true;                                       // value arithmetic of a forward body only
  return 0;
}

vdf_num vdf_cs_tab(vdf_cs* c, const vdf_fe* table, size_t rows, size_t cols, size_t col) {
  if (!c) return 0;
  if (c->rec) return rec_cs_tab(c, table, rows, cols, col);
  c->bad = true;                                       // the round constant of round j: only a body has a j
  return 0;
}

vdf_num vdf_cs_pow_chain(vdf_cs* c, vdf_num a, const vdf_pow_step* steps, size_t n_steps) {
  if (!c) return 0;
  if (c->rec) return rec_cs_pow_chain(c, a, steps, n_steps);
  c->bad = true;                                       // value arithmetic of a forward body only
  return 0;
}

int vdf_nova_pow_chain_exponent(const vdf_pow_step* steps, size_t n_steps, uint64_t e[4], uint32_t* n_tmp, uint64_t* products) {
  return nova_guard([&]() -> int {
    vdfpow::ChainInfo ci;
    const std::string why = vdfpow::check(steps, n_steps, 0, &ci);
    if (!why.empty()) return fail(VDF_ERR_BAD_ARG, "vdf_nova_pow_chain_exponent: " + why);
    if (e) memcpy(e, ci.e.l, 32);
    if (n_tmp) *n_tmp = ci.n_tmp;
    if (products) *products = ci.products();
    return VDF_OK;
  });
}

// Left to right, sliding windows of at most `window` bits that begin and end in a one.  The table first: T[1] = x^2, then T[1 + k]
// = x^(2k + 1) = T[k] * T[1] for k = 1 .. 2^(window - 1) - 1 (T[0] = x), whether the exponent uses every entry or not -- one squaring
// and 2^(window - 1) - 1 products.  Then one step per window: the squarings since the window before, and the product by the window's
// odd value; the first window only names the temporary the accumulator starts from, and zeros at the bottom are a last step of
// squarings alone.
int vdf_nova_pow_chain_window(const uint64_t e[4], unsigned window, vdf_pow_step* steps, size_t cap, size_t* n_steps) {
  return nova_guard([&]() -> int {
    if (!e || !steps || !n_steps) return fail(VDF_ERR_BAD_ARG, "vdf_nova_pow_chain_window: null argument");
    if (window < 2 || window > 4) return fail(VDF_ERR_BAD_ARG, "vdf_nova_pow_chain_window: window must be 2 .. 4");
    vdfpow::U256 E;
    memcpy(E.l, e, 32);
    const int bits = (int)vdfpow::bitlen(E);
    if (bits == 0) return fail(VDF_ERR_BAD_ARG, "vdf_nova_pow_chain_window: e = 0 has no chain");
    auto bit = [&](int i) { return (unsigned)((E.l[i / 64] >> (i % 64)) & 1); };
    std::vector<vdf_pow_step> out;
    out.push_back(vdf_pow_step{0, 1, VDF_POW_NONE, 1});
    for (unsigned k = 1; k < (1u << (window - 1)); ++k) out.push_back(vdf_pow_step{VDF_POW_ACC, 0, (uint8_t)(k == 1 ? 0 : 1), (uint8_t)(1 + k)});
    auto slot_of = [](unsigned odd) { return (uint8_t)(odd == 1 ? 0 : (odd + 1) / 2); };
    uint8_t src = VDF_POW_ACC;                         // the first window: where the accumulator starts
    unsigned pending = 0;
    bool first = true;
    for (int i = bits - 1; i >= 0;) {
      if (!bit(i)) { ++pending; --i; continue; }
      int lo = i - (int)window + 1 > 0 ? i - (int)window + 1 : 0;
      while (!bit(lo)) ++lo;
      unsigned val = 0;
      for (int q = i; q >= lo; --q) val = 2 * val + bit(q);
      if (first) { src = slot_of(val); first = false; }
      else {
        out.push_back(vdf_pow_step{src, (uint8_t)(pending + (unsigned)(i - lo + 1)), slot_of(val), VDF_POW_NONE});
        src = VDF_POW_ACC; pending = 0;
      }
      i = lo - 1;
    }
    if (pending || src != VDF_POW_ACC) out.push_back(vdf_pow_step{src, (uint8_t)pending, VDF_POW_NONE, VDF_POW_NONE});
    if (out.size() > cap || out.size() > VDF_POW_CHAIN_MAX_STEPS)
      return fail(VDF_ERR_BAD_LENGTH, "vdf_nova_pow_chain_window: the chain has " + std::to_string(out.size()) + " steps: more than cap or VDF_POW_CHAIN_MAX_STEPS");
    memcpy(steps, out.data(), out.size() * sizeof(vdf_pow_step));
    *n_steps = out.size();
    return VDF_OK;
  });
}

int vdf_minroot_pow_chain(int fid, vdf_pow_step* steps, size_t cap, size_t* n_steps) {
  return nova_guard([&]() -> int {
    if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
    if (!steps || !n_steps) return fail(VDF_ERR_BAD_ARG, "vdf_minroot_pow_chain: null argument");
    const vdf::MinrootChainProgram& p = fid == VDF_FIELD_FQ ? vdf::MINROOT_CHAIN_FQ : vdf::MINROOT_CHAIN_FP;
    if (cap < vdf::MINROOT_CHAIN_MAX_STEPS) return fail(VDF_ERR_BAD_LENGTH, "vdf_minroot_pow_chain: the programs have 32 steps");
    memcpy(steps, p.step, sizeof(p.step));             // (padded to 32 with steps that do nothing)
    *n_steps = vdf::MINROOT_CHAIN_MAX_STEPS;
    return VDF_OK;
  });
}

int vdf_cs_repeat(vdf_cs* c, const vdf_round_body* b, uint64_t t, const vdf_num* inv, const vdf_num* carry_in, const vdf_fe* advice,
                  vdf_num* carry_out) {
  return vdf_cs_repeat_lanes(c, b, t, 1, inv, carry_in, advice, (size_t)t + 1, carry_out);
}

// `lanes` chains through ONE recorded body: lane after lane, repetition after repetition, what the plain double loop would call
int vdf_cs_repeat_lanes(vdf_cs* c, const vdf_round_body* b, uint64_t t, size_t lanes, const vdf_num* inv, const vdf_num* carry_in,
                        const vdf_fe* advice, size_t lane_stride, vdf_num* carry_out) {
  if (!c) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: null vdf_cs");
  // every refusal below happens before the first variable is made
  auto refuse = [&](const std::string& why) { c->bad = true; return fail(VDF_ERR_BAD_ARG, why); };
  if (c->rec) return refuse("vdf_cs_repeat: not inside a round body");
  if (!c->rep) return refuse("vdf_cs_repeat: this constraint system takes no repeated rounds");
  if (c->rep->used) return refuse("vdf_cs_repeat: one vdf_cs_repeat per circuit");
  if (!b || (b->n_inv && !inv) || (b->n_carry && (!carry_in || !carry_out))) return refuse("vdf_cs_repeat: null argument");
  if (t == 0 || t >= (1ull << 31)) return refuse("vdf_cs_repeat: t out of range");
  if (lanes == 0 || lanes > VDF_TAPE_MAX_LANES) return refuse("vdf_cs_repeat_lanes: lanes must be 1 .. VDF_TAPE_MAX_LANES");
  if (lanes * b->n_inv > VDF_TAPE_MAX_INV && b->n_inv <= VDF_ROUND_MAX_INV) return refuse("vdf_cs_repeat_lanes: lanes * n_inv > VDF_TAPE_MAX_INV");
  if (lane_stride < t + 1 || lane_stride > ((size_t)1 << 40)) return refuse("vdf_cs_repeat_lanes: lane_stride must be at least t + 1");
  CS& cs = *c->cs;
  if (!cs.shape && !advice) return refuse("vdf_cs_repeat: a witness needs advice");
  RoundRecord rec;
  if (record_round_body(&cs, b, &rec) != VDF_OK) { c->bad = true; return VDF_ERR_BAD_ARG; }
  std::vector<Num> invn(lanes * rec.n_inv), carry_all(lanes * rec.n_carry);
  for (size_t k = 0; k < invn.size(); ++k) {
    if (inv[k] >= c->pool.size()) return refuse("vdf_cs_repeat: bad handle in inv");
    invn[k] = c->pool[inv[k]];
  }
  for (size_t k = 0; k < carry_all.size(); ++k) {
    if (carry_in[k] >= c->pool.size()) return refuse("vdf_cs_repeat: bad handle in carry_in");
    carry_all[k] = c->pool[carry_in[k]];
  }
  // (a probe looks at no advice, not even at where it lives: no device call is made on its behalf)
  const bool probe = c->probe && !cs.shape;
  const bool device = !cs.shape && !probe && vdf_ptr_is_device(advice);
  if (device && (!c->ctx || cs.dev_len != 0)) return refuse("vdf_cs_repeat: advice in device memory outside vdf_nova_prove_step_custom");
  if ((device || probe) && c->step_advice && c->step_advice_elems) {
    // advice inside the trace a chain built for this step: the library owns that buffer and knows its length -- lanes * (t + 1)
    // entries -- so nothing may be read behind it, by the copies of entry t below or by the kernel
    const uintptr_t lo = (uintptr_t)c->step_advice, hi = lo + c->step_advice_elems * 32, at = (uintptr_t)advice;
    if (at >= lo && at < hi && ((lanes - 1) * lane_stride + t + 1) * rec.n_adv * 32 > hi - at)
      return refuse("vdf_cs_repeat_lanes: the repeat reads past the step's trace of lanes * (t + 1) entries (vdf_cs_step_advice): over a "
                    "chain's trace lane_stride must be t + 1, and t, lanes and n_adv the chain's");
  }
  RepeatState& rep = *c->rep;
  rep.used = true;
  rep.t = t;
  rep.lanes = lanes;
  rep.lane_stride = lane_stride;
  rep.var_begin = cs.num_vars();
  rep.row_begin = cs.rows;
  rep.d_advice = nullptr;
  const size_t na = rec.n_adv;
  if (probe) {
    // the body and the values of inv are what a lookahead needs; entry t is not copied (that would wait for the device), so the
    // carries leave with the value 0, and neither variables nor rows are made
    for (Num& n : carry_all) n = cs.zero_num();
    rep.d_advice = advice;
    rep.inv.resize(invn.size());
    for (size_t k = 0; k < invn.size(); ++k) rep.inv[k] = invn[k].v;
  } else if (device) {
    std::vector<Fe> last(na);
    for (size_t l = 0; l < lanes; ++l) {                                 // entry t of every lane: the values of its carry_out
      const int rc = vdf_dev_memcpy(c->ctx, last.data(), (const char*)advice + (l * lane_stride + t) * na * 32, na * 32);
      if (rc != VDF_OK) { c->bad = true; return fail(rc, std::string("vdf_cs_repeat: advice entry t: ") + vdf_last_error(c->ctx)); }
      for (uint32_t k = 0; k < rec.n_carry; ++k) { carry_all[l * rec.n_carry + k] = cs.zero_num(); carry_all[l * rec.n_carry + k].v = last[k]; }
    }
    cs.skip(lanes * t * rec.n_vars, lanes * t * rec.n_cons);
    rep.d_advice = advice;
    rep.inv.resize(invn.size());
    for (size_t k = 0; k < invn.size(); ++k) rep.inv[k] = invn[k].v;
  } else {
    std::vector<Num> scratch, lane_inv(rec.n_inv), carry(rec.n_carry);
    for (size_t l = 0; l < lanes; ++l) {
      for (uint32_t k = 0; k < rec.n_inv; ++k) lane_inv[k] = invn[l * rec.n_inv + k];
      for (uint32_t k = 0; k < rec.n_carry; ++k) carry[k] = std::move(carry_all[l * rec.n_carry + k]);
      const Fe* adv = cs.shape ? nullptr : (const Fe*)advice + l * lane_stride * na;
      for (uint64_t j = 0; j < t; ++j) replay_round(cs, rec, j, lane_inv, carry, adv ? adv + j * na : nullptr, adv ? adv + (j + 1) * na : nullptr, scratch);
      for (uint32_t k = 0; k < rec.n_carry; ++k) {
        if (adv) carry[k].v = adv[t * na + k];
        carry_all[l * rec.n_carry + k] = std::move(carry[k]);
      }
    }
  }
  rep.rec = std::move(rec);
  for (size_t k = 0; k < carry_all.size(); ++k) {
    c->pool.push_back(std::move(carry_all[k]));
    carry_out[k] = (vdf_num)(c->pool.size() - 1);
  }
  return VDF_OK;
}

int vdf_nova_round_body_record(int fid, const vdf_round_body* b, vdf_tape_op ops[VDF_TAPE_MAX_OPS], vdf_fe consts[VDF_TAPE_MAX_CONSTS],
                               vdf_round_tape* out) {
  return nova_guard([&]() -> int {
    if (!valid_field(fid) || !ops || !consts || !out) return fail(VDF_ERR_BAD_ARG, "bad argument");
    CS cs(fid, true);
    RoundRecord rec;
    const int rc = record_round_body(&cs, b, &rec);
    if (rc != VDF_OK) return rc;
    *out = rec.view();
    memcpy(ops, rec.ops.data(), rec.ops.size() * sizeof(vdf_tape_op));
    if (!rec.consts.empty()) memcpy(consts, rec.consts.data(), rec.consts.size() * 32);      // (a body may have no constant)
    out->ops = ops;
    out->consts = consts;
    out->table = rec.tab_src;                          // the caller's own array, which the caller keeps alive
    return VDF_OK;
  });
}

int vdf_nova_round_tape_eval(int fid, const vdf_round_tape* tape, uint64_t t, const vdf_fe* inv, const vdf_fe* advice, vdf_fe* out) {
  return nova_guard([&]() -> int { return eval_round_tape(fid, tape, t, (const Fe*)inv, (const Fe*)advice, (Fe*)out); });
}

static int walk_body_record(int fid, const vdf_walk_body* b, vdf_tape_op* ops, vdf_fe* consts, vdf_round_tape* out, bool forward) {
  return nova_guard([&]() -> int {
    if (!valid_field(fid) || !ops || !consts || !out) return fail(VDF_ERR_BAD_ARG, "bad argument");
    CS cs(fid, true);
    RoundRecord rec;
    const int rc = record_walk_body(&cs, b, &rec, forward);
    if (rc != VDF_OK) return rc;
    *out = rec.view();
    memcpy(ops, rec.ops.data(), rec.ops.size() * sizeof(vdf_tape_op));
    if (!rec.consts.empty()) memcpy(consts, rec.consts.data(), rec.consts.size() * 32);      // (a body may have no constant)
    out->ops = ops;
    out->consts = consts;
    out->table = rec.tab_src;                          // the caller's own array, which the caller keeps alive
    return VDF_OK;
  });
}

int vdf_nova_walk_body_record(int fid, const vdf_walk_body* b, vdf_tape_op ops[VDF_TAPE_MAX_OPS], vdf_fe consts[VDF_TAPE_MAX_CONSTS],
                              vdf_round_tape* out) {
  return walk_body_record(fid, b, ops, consts, out, false);
}

int vdf_nova_forward_body_record(int fid, const vdf_walk_body* b, vdf_tape_op ops[VDF_TAPE_MAX_OPS], vdf_fe consts[VDF_TAPE_MAX_CONSTS],
                                 vdf_round_tape* out) {
  return walk_body_record(fid, b, ops, consts, out, true);
}

int vdf_nova_forward_tape_eval(int fid, const vdf_round_tape* tape, const vdf_fe* inv, vdf_fe* entries, size_t n, uint64_t rounds,
                               vdf_fe* checkpoints, uint64_t every, size_t cp_stride, vdf_fe* trace, size_t walk_stride, uint64_t base,
                               uint64_t j_base, uint64_t j_walk_step) {
  return nova_guard([&]() -> int {
    return eval_forward_tape(fid, tape, (const Fe*)inv, (Fe*)entries, n, rounds, (Fe*)checkpoints, every, cp_stride, (Fe*)trace, walk_stride,
                             base, j_base, j_walk_step);
  });
}
int vdf_nova_forward_tape_rebuild_eval_lanes(int fid, const vdf_round_tape* forward_tape, size_t lanes, const vdf_fe* inv, vdf_fe* entries, size_t n,
                                             uint64_t rounds, vdf_fe* trace, size_t walk_stride, uint64_t base, size_t group, size_t group_stride,
                                             const uint64_t* j_base, uint64_t j_group_step, int heads, const vdf_fe* expect, int32_t* ok) {
  return nova_guard([&]() -> int {
    return eval_forward_tape_rebuild_lanes(fid, forward_tape, lanes, (const Fe*)inv, (Fe*)entries, n, rounds, (Fe*)trace, walk_stride, base, group,
                                           group_stride, j_base, j_group_step, heads, (const Fe*)expect, ok);
  });
}

int vdf_nova_periodic_rows_detect(int fid, const uint64_t nnz[3], const uint32_t* const rows[3], const uint32_t* const cols[3],
                                  const vdf_fe* const vals[3], size_t seg_begin, size_t n_vars, size_t row_begin, size_t n_cons, uint64_t t,
                                  uint16_t row_start[VDF_PERIODIC_MAX_STARTS], vdf_periodic_term terms[VDF_PERIODIC_MAX_TERMS],
                                  vdf_fe consts[VDF_PERIODIC_MAX_CONSTS], vdf_periodic_rows* out, uint64_t* lead, uint64_t* first_row,
                                  uint64_t* row_count) {
  const int rc = nova_guard([&]() -> int {
    if (!valid_field(fid) || !nnz || !rows || !cols || !vals || !row_start || !terms || !consts || !out) return -fail(VDF_ERR_BAD_ARG, "bad argument");
    Coo m[3];
    for (int k = 0; k < 3; ++k) {
      if (nnz[k] && (!rows[k] || !cols[k] || !vals[k])) return -fail(VDF_ERR_BAD_ARG, "null triple array");
      m[k].rows.assign(rows[k], rows[k] + nnz[k]);
      m[k].cols.assign(cols[k], cols[k] + nnz[k]);
      m[k].vals.assign((const Fe*)vals[k], (const Fe*)vals[k] + nnz[k]);
    }
    PeriodicRows pr;
    if (!detect_periodic_rows(m, field(fid), seg_begin, n_vars, row_begin, n_cons, t, &pr)) return 0;
    periodic_rows_export(pr, row_start, terms, consts, out, lead, first_row, row_count);
    return 1;
  });
  return rc > 1 ? -rc : rc;                          // (nova_guard's own failures are positive codes)
}

int vdf_nova_periodic_rows_eval(int fid, const vdf_periodic_rows* rows, uint64_t j_first, uint64_t reps, size_t seg_begin, size_t row_begin,
                                size_t num_cols, size_t num_cons, const vdf_fe* z2, const vdf_fe* Az1, const vdf_fe* Bz1, const vdf_fe* Cz1,
                                const vdf_fe* u1, vdf_fe* Az2, vdf_fe* Bz2, vdf_fe* Cz2, vdf_fe* T) {
  return nova_guard([&]() -> int {
    return eval_periodic_rows(fid, rows, j_first, reps, seg_begin, row_begin, num_cols, num_cons, (const Fe*)z2, (const Fe*)Az1, (const Fe*)Bz1,
                              (const Fe*)Cz1, (const Fe*)u1, (Fe*)Az2, (Fe*)Bz2, (Fe*)Cz2, (Fe*)T);
  });
}

int vdf_nova_round_tape_eval_lanes(int fid, const vdf_round_tape* tape, uint64_t t, size_t lanes, const vdf_fe* inv, const vdf_fe* advice,
                                   size_t lane_stride, vdf_fe* out) {
  return nova_guard([&]() -> int { return eval_round_tape_lanes(fid, tape, t, lanes, (const Fe*)inv, (const Fe*)advice, lane_stride, (Fe*)out); });
}

int vdf_nova_walk_tape_eval_lanes(int fid, const vdf_round_tape* tape, size_t lanes, const vdf_fe* inv, vdf_fe* entries, size_t n, uint64_t rounds,
                                  vdf_fe* trace, size_t walk_stride, size_t top, size_t group, size_t group_stride, const uint64_t* j_base,
                                  uint64_t j_group_step, int heads, const vdf_fe* expect, int32_t* ok) {
  return nova_guard([&]() -> int {
    return eval_walk_tape_lanes(fid, tape, lanes, (const Fe*)inv, (Fe*)entries, n, rounds, (Fe*)trace, walk_stride, top, group, group_stride,
                                j_base, j_group_step, heads, (const Fe*)expect, ok);
  });
}

int vdf_nova_walk_tape_eval(int fid, const vdf_round_tape* tape, const vdf_fe* inv, vdf_fe* entries, size_t n, uint64_t rounds, vdf_fe* trace,
                            size_t walk_stride, size_t top, size_t group, size_t group_stride, uint64_t j_base, uint64_t j_group_step, int heads,
                            const vdf_fe* expect, int32_t* ok) {
  return nova_guard([&]() -> int {
    return eval_walk_tape(fid, tape, (const Fe*)inv, (Fe*)entries, n, rounds, (Fe*)trace, walk_stride, top, group, group_stride, j_base,
                          j_group_step, heads, (const Fe*)expect, ok);
  });
}

}  // extern "C"
