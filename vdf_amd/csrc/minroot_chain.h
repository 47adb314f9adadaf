// The forward MinRoot round's fifth root x -> x^e, e = 1/5 mod (m - 1), as DATA: the two exponents and the two addition chains
// of the reference (src/minroot.rs:88-127 PallasVDF::forward_step_ltr_addition_chain over Fq, :223-261 VestaVDF::forward_step
// over Fp), stated once.  The host evaluator (host/minroot_host.cpp) and the device's forward walk (minroot.hip k_forward_walk)
// both run THIS program; neither restates a step of it.  253 squarings for either field, 30 products over Fq and 29 over Fp.
//
// A chain is a straight-line program over an accumulator v and nine slots of one field element each.  One step is
//   v = slot[src] (src != ACC);  v = v^(2^squarings);  v = v * slot[mul] (mul != NONE);  slot[dst] = v (dst != NONE)
// with slot[S1] = x on entry and v = x^e after the last step.  Every step is wave-uniform on the device (the program does not
// depend on the data), so a lane-private slot array may live in LDS and be indexed by a scalar.
//
// The head (13 steps, the same for both fields) builds the eight multiplicands the tails use, x^1, x^0b11, x^0b101, x^0b111,
// x^0b1001, x^0b1111 and, of the runs of 0x33 bytes both exponents begin with (r2 = x^0x33, r4 = x^0x3333, r8, r16, r32), r4 and
// r8; a tail step is the reference's sqr_mul(v, squarings, multiplicand) (:89-92): (squarings, multiplicand index).
// Slots are reused where a value is dead: x^0b10 and r4 share one, x^0b110, r2 and r8 another, r16 has the ninth.
#pragma once
#include <stdint.h>

namespace vdf {

constexpr uint64_t FP_RESCUE_INVALPHA[4] = {0xe0f0f3f0cccccccdull, 0x4e9ee0c9a10a60e2ull, 0x3333333333333333ull,
                                            0x3333333333333333ull};   // src/minroot.rs:273-278
constexpr uint64_t FQ_RESCUE_INVALPHA[4] = {0xd69f2280cccccccdull, 0x4e9ee0c9a143ba4aull, 0x3333333333333333ull,
                                            0x3333333333333333ull};   // src/minroot.rs:280-285

enum : uint8_t {
  MR_S1 = 0, MR_S11 = 1, MR_S101 = 2, MR_S111 = 3, MR_S1001 = 4, MR_S1111 = 5, MR_SR4 = 6, MR_SR8 = 7,   // the tails' multiplicands
  MR_ST = 8,                                                                                             // r16
  MR_S10 = MR_SR4, MR_S110 = MR_SR8, MR_SR2 = MR_SR8,                                                    // dead before their slot is reused
  MR_SLOTS = 9,
  MR_ACC = 0xFE,       // src: go on from the accumulator
  MR_NONE = 0xFF       // mul: no product; dst: nothing kept
};

struct MinrootChainStep { uint8_t src, squarings, mul, dst; };

// src/minroot.rs:93-112 (= :228-247): the multiplicands, the runs r2 .. r32 and the first tail-shaped step
constexpr MinrootChainStep MINROOT_CHAIN_HEAD[] = {
    {MR_S1, 1, MR_NONE, MR_S10},        // 10    = 1^2
    {MR_ACC, 0, MR_S1, MR_S11},         // 11    = 10 * 1
    {MR_ACC, 0, MR_S10, MR_S101},       // 101   = 10 * 11
    {MR_S11, 1, MR_NONE, MR_S110},      // 110   = 11^2
    {MR_ACC, 0, MR_S1, MR_S111},        // 111   = 110 * 1
    {MR_ACC, 0, MR_S10, MR_S1001},      // 1001  = 111 * 10
    {MR_ACC, 0, MR_S110, MR_S1111},     // 1111  = 1001 * 110
    {MR_S110, 3, MR_S11, MR_SR2},       // r2    = sqr_mul(110, 3, 11)
    {MR_ACC, 8, MR_SR2, MR_SR4},        // r4    = sqr_mul(r2, 8, r2)
    {MR_ACC, 16, MR_SR4, MR_SR8},       // r8    = sqr_mul(r4, 16, r4)
    {MR_ACC, 32, MR_SR8, MR_ST},        // r16   = sqr_mul(r8, 32, r8)
    {MR_ACC, 64, MR_ST, MR_NONE},       // r32   = sqr_mul(r16, 64, r16)
    {MR_ACC, 5, MR_S1001, MR_NONE},     // sqr_mul(r32, 5, 1001)
};
#define VDF_MR_T(n, m) {MR_ACC, n, m, MR_NONE}
// src/minroot.rs:107-126 (PallasVDF, Fq): (squarings, multiplicand)
constexpr MinrootChainStep MINROOT_CHAIN_TAIL_FQ[] = {
    VDF_MR_T(8, MR_S111), VDF_MR_T(4, MR_S1), VDF_MR_T(2, MR_SR4), VDF_MR_T(7, MR_S11), VDF_MR_T(6, MR_S1001),
    VDF_MR_T(3, MR_S101), VDF_MR_T(7, MR_S101), VDF_MR_T(7, MR_S111), VDF_MR_T(4, MR_S111), VDF_MR_T(5, MR_S1001),
    VDF_MR_T(5, MR_S101), VDF_MR_T(3, MR_S11), VDF_MR_T(4, MR_S101), VDF_MR_T(3, MR_S101), VDF_MR_T(6, MR_S1111),
    VDF_MR_T(4, MR_S1001), VDF_MR_T(6, MR_S101), VDF_MR_T(37, MR_SR8), VDF_MR_T(2, MR_S1)};
// src/minroot.rs:242-260 (VestaVDF, Fp)
constexpr MinrootChainStep MINROOT_CHAIN_TAIL_FP[] = {
    VDF_MR_T(8, MR_S111), VDF_MR_T(4, MR_S1), VDF_MR_T(2, MR_SR4), VDF_MR_T(7, MR_S11), VDF_MR_T(6, MR_S1001),
    VDF_MR_T(3, MR_S101), VDF_MR_T(5, MR_S1), VDF_MR_T(7, MR_S101), VDF_MR_T(4, MR_S11), VDF_MR_T(8, MR_S111),
    VDF_MR_T(4, MR_S1), VDF_MR_T(4, MR_S111), VDF_MR_T(9, MR_S1111), VDF_MR_T(8, MR_S1111), VDF_MR_T(6, MR_S1111),
    VDF_MR_T(2, MR_S11), VDF_MR_T(34, MR_SR8), VDF_MR_T(2, MR_S1)};
#undef VDF_MR_T

// head + tail as one program (what both interpreters loop over)
constexpr int MINROOT_CHAIN_MAX_STEPS = 32;
struct MinrootChainProgram {
  uint32_t len;
  MinrootChainStep step[MINROOT_CHAIN_MAX_STEPS];
};
template <int NT> constexpr MinrootChainProgram minroot_chain_program(const MinrootChainStep (&tail)[NT]) {
  constexpr int NH = (int)(sizeof(MINROOT_CHAIN_HEAD) / sizeof(MINROOT_CHAIN_HEAD[0]));
  static_assert(NH + NT <= MINROOT_CHAIN_MAX_STEPS, "program too long");
  MinrootChainProgram p{};
  p.len = NH + NT;
  for (int k = 0; k < NH; ++k) p.step[k] = MINROOT_CHAIN_HEAD[k];
  for (int k = 0; k < NT; ++k) p.step[NH + k] = tail[k];
  for (int k = NH + NT; k < MINROOT_CHAIN_MAX_STEPS; ++k) p.step[k] = MinrootChainStep{MR_ACC, 0, MR_NONE, MR_NONE};
  return p;
}
constexpr MinrootChainProgram MINROOT_CHAIN_FQ = minroot_chain_program(MINROOT_CHAIN_TAIL_FQ);
constexpr MinrootChainProgram MINROOT_CHAIN_FP = minroot_chain_program(MINROOT_CHAIN_TAIL_FP);

// squarings / products of a program: 253 and 30 (Fq), 253 and 29 (Fp) -- the cost model of DESIGN.md 4.8
constexpr int minroot_chain_squarings(const MinrootChainProgram& p) {
  int n = 0;
  for (uint32_t k = 0; k < p.len; ++k) n += p.step[k].squarings;
  return n;
}
constexpr int minroot_chain_products(const MinrootChainProgram& p) {
  int n = 0;
  for (uint32_t k = 0; k < p.len; ++k) n += p.step[k].mul != MR_NONE;
  return n;
}
static_assert(minroot_chain_squarings(MINROOT_CHAIN_FQ) == 253 && minroot_chain_products(MINROOT_CHAIN_FQ) == 30, "Fq chain");
static_assert(minroot_chain_squarings(MINROOT_CHAIN_FP) == 253 && minroot_chain_products(MINROOT_CHAIN_FP) == 29, "Fp chain");

}  // namespace vdf
