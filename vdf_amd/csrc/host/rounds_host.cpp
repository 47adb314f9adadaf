// libvdf_nova.so: uniform rounds of a custom step circuit (include/vdf_nova.h vdf_cs_repeat) -- the extension point of the
// reference's StepCircuit trait (/root/reference/src/nova/proof.rs:79-153) for rounds the GPU can run.  A body is recorded once
// (record_round_body), replayed over a constraint system with real calls (replay_round: the shape, and the witness from host
// advice), and compiled into the slot program libvdf_hip.so runs one repetition per thread (RoundRecord::ops; vdf_round_tape_run).
#include "nova_internal.hpp"
#include "rounds.hpp"

using namespace vdfnova;

namespace {
constexpr uint32_t REC_TAG = 0x80000000u;        // handles of a recording vdf_cs: REC_TAG | node -- no handle of another vdf_cs looks like one
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

// node of a handle the body owns, or -1 (and the failure flag)
long rec_node(vdf_cs* c, vdf_num h) {
  if ((h & REC_TAG) && (h & ~REC_TAG) < c->rec->nodes.size()) return (long)(h & ~REC_TAG);
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
int compile_round(RoundRecord& r) {
  const size_t n = r.nodes.size(), nin = r.n_inputs();
  std::vector<uint32_t> root(n);
  for (size_t i = 0; i < n; ++i) root[i] = r.nodes[i].op == R_ALLOC_FROM ? root[r.nodes[i].a] : (uint32_t)i;
  auto operands = [&](const RecNode& x, uint32_t out[2]) -> int {
    switch (x.op) {
      case R_ADD: case R_SUB: case R_MUL: out[0] = root[x.a]; out[1] = root[x.b]; return 2;
      case R_SCALE: case R_ALLOC_FROM: out[0] = root[x.a]; return 1;
      default: return 0;                            // inputs, constants; enforce costs the device nothing
    }
  };
  std::vector<char> needed(n, 0);
  std::vector<long> last_use(n, -1);
  for (size_t i = n; i-- > nin;) {
    const RecNode& x = r.nodes[i];
    if (x.op == R_MUL || x.op == R_ALLOC_FROM) needed[i] = 1;
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
  uint32_t var = 0;
  for (size_t i = nin; i < n; ++i) {
    const RecNode& x = r.nodes[i];
    if (x.op == R_ENFORCE || !needed[i]) continue;
    uint32_t o[2];
    const int k = operands(x, o);
    for (int q = 0; q < k; ++q) {                   // inputs at their first use
      const uint32_t in = o[q];
      if (in >= nin || slot[in] != NO_SLOT) continue;
      slot[in] = take();
      if (in == r.in_j()) emit(VDF_TAPE_J, slot[in], 0, 0);
      else if (in < r.in_carry(0)) emit(VDF_TAPE_INV, slot[in], in - r.in_inv(0), 0);
      else if (in < r.in_cur(0)) emit(VDF_TAPE_ADV, slot[in], in - r.in_carry(0), 0);      // carry c IS advice entry j, column c
      else if (in < r.in_next(0)) emit(VDF_TAPE_ADV, slot[in], in - r.in_cur(0), 0);
      else emit(VDF_TAPE_ADV, slot[in], in - r.in_next(0), 1);
    }
    const uint32_t sa = k > 0 ? slot[o[0]] : 0, sb = k > 1 ? slot[o[1]] : 0;
    for (int q = 0; q < k; ++q)
      if (last_use[o[q]] == (long)i && !(q == 1 && o[1] == o[0])) busy[slot[o[q]]] = 0;
    switch (x.op) {
      case R_CONST: slot[i] = take(); emit(VDF_TAPE_CONST, slot[i], x.a, 0); break;
      case R_ADD: slot[i] = take(); emit(VDF_TAPE_ADD, slot[i], sa, sb); break;
      case R_SUB: slot[i] = take(); emit(VDF_TAPE_SUB, slot[i], sa, sb); break;
      case R_SCALE: slot[i] = take(); emit(VDF_TAPE_SCALE, slot[i], sa, x.b); break;
      case R_MUL: slot[i] = take(); emit(VDF_TAPE_MUL, slot[i], sa, sb); emit(VDF_TAPE_OUT, 0, slot[i], var++); break;
      default: emit(VDF_TAPE_OUT, 0, sa, var++); break;      // R_ALLOC_FROM
    }
    if (x.op != R_ALLOC_FROM && last_use[i] < 0) busy[slot[i]] = 0;      // a product nothing reads again
  }
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
  if (h.bad) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: the round body used a handle it does not own, a value-only handle in a constraint, or a call that is not recordable");
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

int eval_round_tape(int fid, const vdf_round_tape* tp, uint64_t t, const Fe* inv, const Fe* advice, Fe* out) {
  if (!valid_field(fid)) return fail(VDF_ERR_BAD_ARG, "unknown field");
  if (!tp || !out || !advice || (tp->n_ops && !tp->ops) || (tp->n_consts && !tp->consts) || (tp->n_inv && !inv)) return fail(VDF_ERR_BAD_ARG, "null argument");
  if (t == 0 || t >= (1ull << 31)) return fail(VDF_ERR_BAD_LENGTH, "t out of range");
  if (tp->n_ops > VDF_TAPE_MAX_OPS || tp->n_consts > VDF_TAPE_MAX_CONSTS || tp->n_slots > VDF_TAPE_MAX_SLOTS || tp->n_vars > VDF_TAPE_MAX_VARS ||
      tp->n_inv > VDF_TAPE_MAX_INV || tp->n_adv > VDF_TAPE_MAX_ADV || tp->n_vars == 0 || tp->n_adv == 0 || tp->n_slots == 0)
    return fail(VDF_ERR_BAD_ARG, "tape exceeds a published cap (VDF_TAPE_MAX_*), or has no variable, slot or advice column");
  const Field& F = field(fid);
  const Fe* consts = (const Fe*)tp->consts;
  Fe s[VDF_TAPE_MAX_SLOTS];
  for (uint64_t j = 0; j < t; ++j) {
    bool written[VDF_TAPE_MAX_SLOTS] = {}, var_out[VDF_TAPE_MAX_VARS] = {};
    const Fe* adv = advice + j * tp->n_adv;
    for (size_t i = 0; i < tp->n_ops; ++i) {
      const vdf_tape_op& o = tp->ops[i];
      auto rd = [&](uint8_t x) { return x < tp->n_slots && written[x]; };
      bool ok = false;
      Fe r = zero();
      switch (o.op) {
        case VDF_TAPE_ADV: ok = o.a < tp->n_adv && o.b <= 1; if (ok) r = adv[o.b * tp->n_adv + o.a]; break;
        case VDF_TAPE_INV: ok = o.a < tp->n_inv; if (ok) r = inv[o.a]; break;
        case VDF_TAPE_J: ok = true; r = from_u64(j, F); break;
        case VDF_TAPE_CONST: ok = o.a < tp->n_consts; if (ok) r = consts[o.a]; break;
        case VDF_TAPE_ADD: ok = rd(o.a) && rd(o.b); if (ok) r = add(s[o.a], s[o.b], F); break;
        case VDF_TAPE_SUB: ok = rd(o.a) && rd(o.b); if (ok) r = sub(s[o.a], s[o.b], F); break;
        case VDF_TAPE_MUL: ok = rd(o.a) && rd(o.b); if (ok) r = mul(s[o.a], s[o.b], F); break;
        case VDF_TAPE_SCALE: ok = rd(o.a) && o.b < tp->n_consts; if (ok) r = mul(s[o.a], consts[o.b], F); break;
        case VDF_TAPE_OUT:
          ok = rd(o.a) && o.b < tp->n_vars && !var_out[o.b];
          if (ok) { var_out[o.b] = true; out[j * tp->n_vars + o.b] = s[o.a]; }
          break;
        default: break;
      }
      if (ok && o.op != VDF_TAPE_OUT) { ok = o.dst < tp->n_slots; if (ok) { s[o.dst] = r; written[o.dst] = true; } }
      if (!ok) return fail(VDF_ERR_BAD_ARG, "tape op " + std::to_string(i) + " is malformed (opcode, index out of range, or a slot read before it is written)");
    }
    for (uint32_t k = 0; k < tp->n_vars; ++k)
      if (!var_out[k]) return fail(VDF_ERR_BAD_ARG, "tape leaves variable " + std::to_string(k) + " unwritten");
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
  const bool vo = c->rec->nodes[x].value_only || c->rec->nodes[y].value_only;
  if (op == R_MUL && vo) { c->bad = true; return 0; }      // a constraint over a value without a linear combination
  return rec_push(c, (uint8_t)op, vo, (uint32_t)x, (uint32_t)y, 0);
}
vdf_num rec_cs_scale(vdf_cs* c, vdf_num a, const vdf_fe* k) {
  const long x = rec_node(c, a);
  if (x < 0 || !k) { c->bad = true; return 0; }
  return rec_push(c, R_SCALE, c->rec->nodes[x].value_only, (uint32_t)x, rec_const(c, k), 0);
}
int rec_cs_enforce(vdf_cs* c, vdf_num a, vdf_num b, vdf_num cc) {
  const long x = rec_node(c, a), y = rec_node(c, b), z = rec_node(c, cc);
  if (x < 0 || y < 0 || z < 0) return VDF_ERR_BAD_ARG;
  const std::vector<RecNode>& nd = c->rec->nodes;
  if (nd[x].value_only || nd[y].value_only || nd[z].value_only) { c->bad = true; return VDF_ERR_BAD_ARG; }
  rec_push(c, R_ENFORCE, false, (uint32_t)x, (uint32_t)y, (uint32_t)z);
  return c->bad ? VDF_ERR_BAD_ARG : VDF_OK;
}
}  // namespace vdfnova

extern "C" {

vdf_num vdf_cs_alloc_from(vdf_cs* c, vdf_num src) {
  if (!c) return 0;
  if (c->rec) {
    const long x = rec_node(c, src);
    return x < 0 ? 0 : rec_push(c, R_ALLOC_FROM, false, (uint32_t)x, 0, 0);
  }
  if (src >= c->pool.size()) { c->bad = true; return 0; }
  const Fe v = c->pool[src].v;
  c->pool.push_back(c->cs->alloc(c->cs->shape ? zero() : v));
  return (vdf_num)(c->pool.size() - 1);
}

int vdf_cs_repeat(vdf_cs* c, const vdf_round_body* b, uint64_t t, const vdf_num* inv, const vdf_num* carry_in, const vdf_fe* advice,
                  vdf_num* carry_out) {
  if (!c) return fail(VDF_ERR_BAD_ARG, "vdf_cs_repeat: null vdf_cs");
  // every refusal below happens before the first variable is made
  auto refuse = [&](const std::string& why) { c->bad = true; return fail(VDF_ERR_BAD_ARG, why); };
  if (c->rec) return refuse("vdf_cs_repeat: not inside a round body");
  if (!c->rep) return refuse("vdf_cs_repeat: this constraint system takes no repeated rounds");
  if (c->rep->used) return refuse("vdf_cs_repeat: one vdf_cs_repeat per circuit");
  if (!b || (b->n_inv && !inv) || (b->n_carry && (!carry_in || !carry_out))) return refuse("vdf_cs_repeat: null argument");
  if (t == 0 || t >= (1ull << 31)) return refuse("vdf_cs_repeat: t out of range");
  CS& cs = *c->cs;
  if (!cs.shape && !advice) return refuse("vdf_cs_repeat: a witness needs advice");
  RoundRecord rec;
  if (record_round_body(&cs, b, &rec) != VDF_OK) { c->bad = true; return VDF_ERR_BAD_ARG; }
  std::vector<Num> invn(rec.n_inv), carry(rec.n_carry);
  for (uint32_t k = 0; k < rec.n_inv; ++k) {
    if (inv[k] >= c->pool.size()) return refuse("vdf_cs_repeat: bad handle in inv");
    invn[k] = c->pool[inv[k]];
  }
  for (uint32_t k = 0; k < rec.n_carry; ++k) {
    if (carry_in[k] >= c->pool.size()) return refuse("vdf_cs_repeat: bad handle in carry_in");
    carry[k] = c->pool[carry_in[k]];
  }
  const bool device = !cs.shape && vdf_ptr_is_device(advice);
  if (device && (!c->ctx || cs.dev_len != 0)) return refuse("vdf_cs_repeat: advice in device memory outside vdf_nova_prove_step_custom");
  RepeatState& rep = *c->rep;
  rep.used = true;
  rep.t = t;
  rep.var_begin = cs.num_vars();
  rep.d_advice = nullptr;
  const size_t na = rec.n_adv;
  if (cs.shape) {
    std::vector<Num> scratch;
    for (uint64_t j = 0; j < t; ++j) replay_round(cs, rec, j, invn, carry, nullptr, nullptr, scratch);
  } else if (!device) {
    const Fe* adv = (const Fe*)advice;
    std::vector<Num> scratch;
    for (uint64_t j = 0; j < t; ++j) replay_round(cs, rec, j, invn, carry, adv + j * na, adv + (j + 1) * na, scratch);
    for (uint32_t k = 0; k < rec.n_carry; ++k) carry[k].v = adv[t * na + k];
  } else {
    std::vector<Fe> last(na);
    const int rc = vdf_dev_memcpy(c->ctx, last.data(), (const char*)advice + t * na * 32, na * 32);
    if (rc != VDF_OK) { c->bad = true; return fail(rc, std::string("vdf_cs_repeat: advice entry t: ") + vdf_last_error(c->ctx)); }
    cs.skip(t * rec.n_vars, t * rec.n_cons);
    rep.d_advice = advice;
    rep.inv.resize(rec.n_inv);
    for (uint32_t k = 0; k < rec.n_inv; ++k) rep.inv[k] = invn[k].v;
    for (uint32_t k = 0; k < rec.n_carry; ++k) { carry[k] = cs.zero_num(); carry[k].v = last[k]; }
  }
  rep.rec = std::move(rec);
  for (uint32_t k = 0; k < rep.rec.n_carry; ++k) {
    c->pool.push_back(std::move(carry[k]));
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
    memcpy(consts, rec.consts.data(), rec.consts.size() * 32);
    out->ops = ops;
    out->consts = consts;
    return VDF_OK;
  });
}

int vdf_nova_round_tape_eval(int fid, const vdf_round_tape* tape, uint64_t t, const vdf_fe* inv, const vdf_fe* advice, vdf_fe* out) {
  return nova_guard([&]() -> int { return eval_round_tape(fid, tape, t, (const Fe*)inv, (const Fe*)advice, (Fe*)out); });
}

}  // extern "C"
