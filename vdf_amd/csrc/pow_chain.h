// Caller-supplied addition chains (include/vdf_hip.h vdf_pow_step, VDF_TAPE_POWC): what makes a chain valid, its exponent, its
// cost, and how it lies in a tape's constants -- stated ONCE, header-only, for both libraries: libvdf_hip.so's launchers
// (rounds.hip pack_tape) and libvdf_nova.so's recorder, host evaluator and entry points (host/rounds_host.cpp) include this file,
// since neither library can call the other's internals.  Host code only: no kernel reads this.
//
// A chain is minroot_chain.h's step format made public: a straight-line program over an accumulator v and n_tmp temporaries,
// T[0] = the base on entry,
//   v = T[src] (src != ACC);  v = v^(2^squarings);  v = v * T[mul] (mul != NONE);  T[dst] = v (dst != NONE)
// and the exponent follows from the steps: e(T[0]) = 1, e = e(src) * 2^squarings + e(mul).
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/vdf_hip.h"

namespace vdfpow {

struct U256 {
  uint64_t l[4];
};
inline unsigned bitlen(const U256& a) {
  for (int q = 3; q >= 0; --q)
    if (a.l[q]) return 64 * q + 64 - __builtin_clzll(a.l[q]);
  return 0;
}
// a * 2^k; false when the product reaches 2^256
inline bool shl(const U256& a, unsigned k, U256* out) {
  if (bitlen(a) + k > 256) return false;
  U256 r = {{0, 0, 0, 0}};
  const unsigned w = k / 64, s = k % 64;
  for (int q = 3; q >= (int)w; --q) {
    r.l[q] = a.l[q - w] << s;
    if (s && q - (int)w - 1 >= 0) r.l[q] |= a.l[q - w - 1] >> (64 - s);
  }
  *out = r;
  return true;
}
// a + b; false when the sum reaches 2^256
inline bool add(const U256& a, const U256& b, U256* out) {
  U256 r;
  unsigned carry = 0;
  for (int q = 0; q < 4; ++q) {
    const unsigned __int128 t = (unsigned __int128)a.l[q] + b.l[q] + carry;
    r.l[q] = (uint64_t)t;
    carry = (unsigned)(t >> 64);
  }
  *out = r;
  return carry == 0;
}

struct ChainInfo {
  U256 e;                  // the chain's exponent
  uint32_t n_tmp;          // the temporaries it uses: its largest index + 1 (or the count the caller declared)
  uint64_t squarings;      // the sum over the steps
  uint64_t muls;           // steps with a product
  uint64_t products() const { return squarings + muls ? squarings + muls : 1; }      // what the work caps count
};

// "" for a valid chain (vdf_hip.h), else what is wrong, naming the step.  n_tmp_declared = 0: the count follows from the steps.
inline std::string check(const vdf_pow_step* st, size_t n_steps, uint32_t n_tmp_declared, ChainInfo* out) {
  if (!st) return "null steps";
  if (n_steps == 0 || n_steps > VDF_POW_CHAIN_MAX_STEPS) return "a chain has 1 .. VDF_POW_CHAIN_MAX_STEPS steps";
  if (n_tmp_declared > VDF_POW_CHAIN_MAX_TMP) return "a chain has 1 .. VDF_POW_CHAIN_MAX_TMP temporaries";
  const uint32_t cap = n_tmp_declared ? n_tmp_declared : VDF_POW_CHAIN_MAX_TMP;
  U256 e[VDF_POW_CHAIN_MAX_TMP], acc = {{0, 0, 0, 0}};
  bool written[VDF_POW_CHAIN_MAX_TMP] = {};
  e[0] = U256{{1, 0, 0, 0}};
  written[0] = true;                                   // the base
  ChainInfo info;
  info.n_tmp = 1; info.squarings = 0; info.muls = 0;
  for (size_t k = 0; k < n_steps; ++k) {
    const vdf_pow_step& s = st[k];
    const std::string at = "step " + std::to_string(k) + ": ";
    if (s.src == VDF_POW_ACC) {
      if (k == 0) return at + "the first step cannot go on from the accumulator";
    } else {
      if (s.src >= cap) return at + "src is not a temporary of the chain (index >= n_tmp)";
      if (!written[s.src]) return at + "src reads a temporary no step has written";
      acc = e[s.src];
      if (s.src + 1u > info.n_tmp) info.n_tmp = s.src + 1u;
    }
    if (!shl(acc, s.squarings, &acc)) return at + "the exponent reaches 2^256";
    info.squarings += s.squarings;
    if (s.mul != VDF_POW_NONE) {
      if (s.mul >= cap) return at + "mul is not a temporary of the chain (index >= n_tmp)";
      if (!written[s.mul]) return at + "mul reads a temporary no step has written";
      if (!add(acc, e[s.mul], &acc)) return at + "the exponent reaches 2^256";
      ++info.muls;
      if (s.mul + 1u > info.n_tmp) info.n_tmp = s.mul + 1u;
    }
    if (s.dst != VDF_POW_NONE) {
      if (s.dst >= cap) return at + "dst is not a temporary of the chain (index >= n_tmp)";
      e[s.dst] = acc;
      written[s.dst] = true;
      if (s.dst + 1u > info.n_tmp) info.n_tmp = s.dst + 1u;
    }
  }
  if (n_tmp_declared) info.n_tmp = n_tmp_declared;
  info.e = acc;
  if (out) *out = info;
  return "";
}

// the constants a chain of n_steps steps takes in a tape: ceil((4 + 4 n_steps) / 32)
inline size_t packed_consts(size_t n_steps) { return (4 + 4 * n_steps + 31) / 32; }

// The chain in `bytes` (packed_consts(n_steps) * 32 of them): n_steps, n_tmp, two zero bytes, the steps, zeros to the end
inline void pack(const vdf_pow_step* st, size_t n_steps, uint32_t n_tmp, uint8_t* bytes) {
  memset(bytes, 0, packed_consts(n_steps) * 32);
  bytes[0] = (uint8_t)n_steps;
  bytes[1] = (uint8_t)n_tmp;
  memcpy(bytes + 4, st, 4 * n_steps);
}

// The chain that lies in a tape's constants from consts[b] on: "" when it is valid, ends inside n_consts and is padded with
// zeros; *steps then points at its n_steps steps (into consts).
inline std::string check_packed(const vdf_fe* consts, size_t n_consts, size_t b, ChainInfo* out, const vdf_pow_step** steps,
                                size_t* n_steps) {
  static_assert(sizeof(vdf_pow_step) == 4, "a step is four bytes");
  if (b >= n_consts) return "the chain's constant is not one of the tape's";
  const uint8_t* p = (const uint8_t*)(consts + b);
  const size_t n = p[0], n_tmp = p[1];
  if (p[2] || p[3]) return "bytes 2 and 3 of a chain's first constant are zero";
  if (n == 0 || n > VDF_POW_CHAIN_MAX_STEPS) return "a chain has 1 .. VDF_POW_CHAIN_MAX_STEPS steps";
  if (n_tmp == 0 || n_tmp > VDF_POW_CHAIN_MAX_TMP) return "a chain has 1 .. VDF_POW_CHAIN_MAX_TMP temporaries";
  const size_t need = packed_consts(n);
  if (need > n_consts - b) return "the chain runs past the tape's constants";
  for (size_t q = 4 + 4 * n; q < need * 32; ++q)
    if (p[q]) return "the bytes behind a chain's last step are zero";
  const vdf_pow_step* st = (const vdf_pow_step*)(p + 4);
  const std::string why = check(st, n, (uint32_t)n_tmp, out);
  if (!why.empty()) return why;
  if (steps) *steps = st;
  if (n_steps) *n_steps = n;
  return "";
}

}  // namespace vdfpow
