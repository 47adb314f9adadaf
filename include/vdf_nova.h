/* vdf_nova.h -- host layer above the kernel ABI (include/vdf_hip.h): the reference crate's public
 * surface for the MinRoot VDF and its Nova proof, restated as a C ABI (libvdf_nova.so).
 *
 * The reference is Rust (/root/reference/src/minroot.rs, src/nova/proof.rs); no Rust toolchain
 * exists in the build image, so the host side is C++ and mirrors the reference's names, argument
 * meaning and error behaviour.  Every pass over a vector is a call through include/vdf_hip.h; this
 * library contains no kernel and no CPU fallback for one.  What stays on the host is what the
 * reference also keeps sequential or O(1): the forward MinRoot evaluation (src/minroot.rs:329-359,
 * the "delay" itself), and the synthesis of the ~10^4 variables of an augmented circuit that are not
 * MinRoot rounds (hashes, in-circuit group arithmetic: strictly sequential field work).
 *
 * What a proof is: Nova IVC on the Pallas / Vesta cycle (src/nova/proof.rs:26-43), protocol
 * "vdf-nova-ivc-v1", specified in oracle/nova.py.  prove_step (:342-349) folds the previous secondary
 * instance, synthesises the PRIMARY augmented circuit (in-circuit check of the previous output hash,
 * in-circuit NIFS verifier for the secondary curve, the MinRoot step circuit, the next output hash)
 * commits and folds it, then does the same for the SECONDARY augmented circuit around
 * TrivialTestCircuit (:258-260).  A proof has constant size in the number of steps and verify
 * (:370-392) recomputes two hashes and checks three satisfiability claims, `zi_secondary == [0]`
 * included.  nova-snark 0.8.0's own constants (Poseidon parameters, allocation order, transcript,
 * generator derivation) are not in /root/reference and pinned by none of its tests:
 * proofs are self-consistent and bit-exact against oracle/nova.py, not interchangeable with
 * nova-snark's -- parity unpinned.
 *
 * Threading.  The evaluator functions and vdf_nova_ro_hash / shape_digest / aug_synthesize are pure (any thread, any time).
 * A parameter set (vdf_pp) owns the device queue its proofs enqueue on: ONE call at a time per parameter set and per
 * handle made under it (prove_step, verify, compress, the wire functions that touch the device); calls under different
 * parameter sets are independent and may run on different threads at once (two chains = two sets: bench.py's
 * aggregate_over_concurrent_chains).  Concurrent vdf_nova_compress calls under one set are serialised by the library at the
 * point where they share its second queue; nothing else is.  The library has threads of its own: up to a few sets of three
 * detached synthesis helpers, made when a prover first wants them and parked between calls (they never touch a handle
 * outside the call that handed them work), and one thread per vdf_nova_compress for the secondary side's argument, joined
 * before the call returns; vdf_nova_eval_and_prove runs the forward evaluation on a thread of its own, joined before it returns.
 */
#ifndef VDF_NOVA_H
#define VDF_NOVA_H

#include "vdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src/minroot.rs:14-20 */
enum { VDF_MODE_LTR_SEQUENTIAL = 0, VDF_MODE_LTR_ADDCHAIN_SEQUENTIAL = 1, VDF_MODE_RTL_SEQUENTIAL = 2,
       VDF_MODE_RTL_ADDCHAIN_SEQUENTIAL = 3 };

/* State<T> { x, y, i } (src/minroot.rs:267-272) is vdf_state of vdf_hip.h: the device's inverse walks take it too */

/* ---- MinRoot evaluator (trait MinRootVDF, src/minroot.rs:287-374); field = VDF_FIELD_FQ is
 * PallasVDF (:40-197), VDF_FIELD_FP is VestaVDF (:201-262, ignores the mode, :203-205) -------- */
int vdf_minroot_forward_step(int field, int mode, const vdf_fe* x, vdf_fe* out);      /* :77-84, :223 */
int vdf_minroot_inverse_step(int field, const vdf_fe* x, vdf_fe* out);                /* :73-75 */
int vdf_minroot_round(int field, int mode, const vdf_state* s, vdf_state* out);       /* :329-335 */
int vdf_minroot_inverse_round(int field, const vdf_state* s, vdf_state* out);         /* :338-344 */
/* eval / simple_eval (:348-359).  trace_xy (optional, 2*(t+1) elements) receives (x, y) of every
 * state 0..t -- the reference discards it (:352-359); the witness kernel consumes it. */
int vdf_minroot_eval(int field, int mode, const vdf_state* s, uint64_t t, vdf_state* out, vdf_fe* trace_xy);
/* simple_eval that keeps every `every`-th state instead of all or none: out_states[k] = the state after k * every rounds,
 * k = 0 .. rounds_total / every (the first and the last included).  `every` must divide rounds_total (VDF_ERR_BAD_ARG; 0 too).
 * The producer side of vdf_nova_circuits_from_checkpoints.  Pure, any thread. */
int vdf_minroot_eval_checkpoints(int field, int mode, const vdf_state* s, uint64_t rounds_total, uint64_t every, vdf_state* out_states);
int vdf_minroot_inverse_eval(int field, const vdf_state* s, uint64_t t, vdf_state* out);   /* :363-365 */
int vdf_minroot_check(int field, const vdf_state* result, uint64_t t, const vdf_state* original); /* :369-371; 1 = ok */
int vdf_minroot_element(int field, uint64_t n, vdf_fe* out);                           /* V::element, :60, :207 */

/* ---- Nova proof API (src/nova/proof.rs:232-392) ------------------------------------------------ */
typedef struct vdf_pp vdf_pp;             /* NovaVDFPublicParams, :38-43 */
typedef struct vdf_circuits vdf_circuits; /* Vec<InverseMinRootCircuit<G1>>, :57-66 (reversed, :294) */
typedef struct vdf_proof vdf_proof;       /* NovaVDFProof::Recursive, :51-55 */
typedef struct vdf_snark vdf_snark;       /* NovaVDFProof::Compressed, :54 */

/* The primary step circuit (the seam of :79-153).  REFERENCE (the default: what vdf_nova_public_params builds, what
 * the bench measures and the parity tests check first): the circuit exactly as the reference writes it -- 4 variables
 * per round, new_x allocated at :167-173 and used by no constraint (:219-227 takes y - i + 1 directly), 4t + 1 step
 * variables, 3t + 1 constraints; 2^19 generators at t = 2^16.  Because nothing binds new_x a prover may set it freely, so
 * a proof over this circuit does not attest the VDF (tests/test_oracle_nova.py builds the forgery): a weakness of the
 * work-in-progress reference that a drop-in reproduces.  BOUND: the sound variant, offered as an option -- new_x carried
 * as the linear combination y - i + 1 instead of a variable, 3 variables and the same 3 constraints per round.
 * The witness of the reference's circuit is committed WITHOUT a term per new_x: new_x_j is an affine image of new_y_(j-1),
 * so its share folds into derived generators (vdf_hip.h vdf_minroot_step_segment_packed) -- same commitment, 3t + 4 terms.
 * FORWARD: the step in the direction of evaluation (src/minroot.rs:329-335), arity 3, z_in = (x_0, y_0, i_in): per round the
 * fifth root x_(j+1) is allocated (the hint comes from the forward trace), tmp1 = x_(j+1)^2, tmp2 = tmp1^2 and
 * tmp2 * x_(j+1) = x_j + y_j is enforced; y_(j+1) = x_j + i_in + j is a linear combination; then final_i = i_in + t.
 * 3 variables and 3 constraints per round, the size of BOUND.  Sound by construction: the fifth root is the only free variable
 * of a round and x -> x^5 is a bijection on Fq.  A proof of this kind states z0 = the chain's INITIAL state and zi = its final
 * state, and its steps are proved in the order they are evaluated (vdf_nova_circuits_forward_begin, vdf_nova_eval_and_prove);
 * verify, compress, the batch calls and both wire formats work on it unchanged.  packed_commit does not apply; fold_fused
 * falls back to the unfused fold.
 * FORWARD_LANES: L forward circuits side by side in ONE step circuit of arity 3L, z = (x_0, y_0, i_0, x_1, y_1, i_1, ...): every
 * lane carries its own round counter, so any L evaluations of equal length share one running proof, one compress, one verify
 * and one blob on the wire.  Lane l's 3t + 1 variables sit at seg_begin + l (3t + 1) (x', tmp1, tmp2 per round, then final_i),
 * its constraints at row_begin + l (3t + 1), and the 3L inputs in the variables right in front of seg_begin, lane l at
 * seg_begin - 3L + 3l.  Made by vdf_nova_public_params_lanes only; outside the rounds a lane costs about 1,059 constraints (the
 * longer z0 / zi the two state hashes absorb), host-synthesised.  packed_commit does not apply; fold_fused falls back. */
enum { VDF_CIRCUIT_MINROOT_BOUND = 0, VDF_CIRCUIT_MINROOT_REFERENCE = 1, VDF_CIRCUIT_CUSTOM = 2 /* vdf_step_circuit, below */,
       VDF_CIRCUIT_MINROOT_FORWARD = 3, VDF_CIRCUIT_MINROOT_FORWARD_LANES = 4 };
#define VDF_NOVA_MAX_LANES 16             /* arity 48, under the seam's cap of 64 */
enum { VDF_SIDE_PRIMARY = 0, VDF_SIDE_SECONDARY = 1 };

/* public_params(num_iters_per_step), :232-237: both augmented circuits synthesised once for their R1CS shapes,
 * Pedersen generators per curve (next_pow2(max(vars, cons)) of them, seeded try-and-increment -- unknown discrete
 * logarithms; nova-snark's own label -> hash derivation is unpinned) with their fixed-base tables, and the digest of
 * all of it that every hash of the protocol absorbs.  One-time; outside every timed region (benches/nova.rs:51-58). */
int  vdf_nova_public_params(vdf_ctx* ctx, uint64_t num_iters_per_step, vdf_pp** out);      /* the reference's circuit */
/* The same with the step circuit and the generator family chosen.  gens_family = VDF_GENS_KNOWN_DLOG is for tests only
 * (commitments checkable by the discrete-log identity at full size; such commitments are not binding);
 * VDF_GENS_LABEL_SHAKE derives the generators from the label "vdf-nova-ivc-v1 gens" through SHAKE256, the way nova-snark
 * derives its CommitGens (vdf_bases_generate_label): parameters reproducible from a string. */
int  vdf_nova_public_params_ex(vdf_ctx* ctx, uint64_t num_iters_per_step, int circuit_kind, int gens_family, vdf_pp** out);
/* HBM a parameter set holds, and how to bound the optional part.  Beside the shapes and the generators with their
 * fixed-base tables (2^19 Pallas generators x 16 windows x 64 B = 512 MiB for the reference's circuit at t = 2^16, plus the
 * derived generators of the packed commitment), public_params builds a DIGIT TABLE per side for the generators of the
 * small commitments a step waits on (vdf_bases_precompute_digits: 0.85 MB per generator at a 10-bit window, 2.9 MB at 12):
 * all 10,049 generators of the secondary side and the ~12.5 k of the primary side outside the MinRoot rounds and the early
 * rows.  It is an accelerator only (results are the same group elements without it) and it is BUDGETED: the tables of both
 * sides together take at most vdf_nova_tuning.digit_budget_bytes -- 20 GiB by default, which buys the 10-bit tables
 * (19 GB at t = 2^16); 72 GiB buys the 12-bit ones (65 GB) for ~2.5 % of a step -- and never more than the free HBM less a
 * reserve for what is allocated afterwards (proof buffers, MSM workspaces).  A table that does not fit is skipped
 * (vdf_nova_pp_memory reports it; tuning.verbose logs it).  Flags:
 *   VDF_PP_NO_DIGIT_TABLES  no digit tables: every commitment takes the bucket method (about +0.5 ms per step at t = 2^16)
 *   VDF_PP_NO_EARLY_ROWS    the cross term T of a step is made and committed in one piece instead of ahead of the step
 *                           for the rows that read only the MinRoot rounds (one MSM workspace and one queue fewer) */
enum { VDF_PP_NO_DIGIT_TABLES = 1u, VDF_PP_NO_EARLY_ROWS = 2u };
int  vdf_nova_public_params_flags(vdf_ctx* ctx, uint64_t num_iters_per_step, int circuit_kind, int gens_family, uint32_t flags,
                                  vdf_pp** out);
/* The random oracle as a PARAMETER BLOCK, covered by the parameters' digest.  The reference reaches
 * its RO through nova-snark 0.8.0 -> neptune 7.2.0 (Cargo.toml:14-15), neither of which is in the reference tree: nothing
 * pins their constants here, so this library's default is its own permutation -- and everything the RO is made of is data:
 *   family 0 (VDF_RO_POSEIDON2): Poseidon2-style, width 4, 8 + 56 rounds, constants from SHAKE256 (the default; the only
 *            block of this family the build supports);
 *   family 1 (VDF_RO_POSEIDON):  the original Poseidon permutation -- dense Cauchy MDS matrix 1 / (i + t + j), round
 *            constants from the paper's Grain LFSR, any width 2..25 (a sponge of rate width - 1), even full_rounds <= 16,
 *            partial_rounds <= 128.  vdf_nova_ro_preset(1) is the shape [UPSTREAM-RECALL] neptune gives nova-snark: width 25,
 *            8 + 57 rounds.  Recalled, unpinned, NOT claimed interoperable: it shows that adopting the upstream constants
 *            is a change of this block, not of code.
 * alpha must be 5, challenge_bits 128, hash_bits 250 (what the circuits of this build are written for); any other value is
 * refused.  A block other than the default changes both R1CS shapes and the digest. */
enum { VDF_RO_POSEIDON2 = 0, VDF_RO_POSEIDON = 1 };
typedef struct vdf_nova_ro_params {
  uint32_t struct_size;          /* sizeof(vdf_nova_ro_params) as the caller compiled it */
  int32_t  family, width, full_rounds, partial_rounds, alpha, challenge_bits, hash_bits;
} vdf_nova_ro_params;
int  vdf_nova_ro_preset(int which, vdf_nova_ro_params* out);        /* 0 = this build's default, 1 = the neptune-shaped block */
int  vdf_nova_pp_ro(const vdf_pp* pp, vdf_nova_ro_params* out);     /* the block a parameter set was made under */
/* Everything tunable about a parameter set and the prover that runs over it, in one struct (DESIGN.md says what each
 * choice measured).  vdf_nova_tuning_default fills in the defaults; the environment variables of earlier rounds
 * (VDF_NOVA_*) are read once, by that function's first call, as overrides of those defaults.  A parameter set keeps its
 * copy: two sets in one process may differ. */
typedef struct vdf_nova_tuning {
  uint32_t struct_size;          /* sizeof(vdf_nova_tuning) as the caller compiled it */
  uint32_t flags;                /* VDF_PP_* */
  uint64_t digit_budget_bytes;   /* HBM for the digit tables of both sides together (20 GiB) */
  int32_t  digit_window;         /* 0 = the widest window of 12 .. 8 whose tables fit the budget; 6..12 = exactly this one
                                    (still subject to the free HBM); -1 = none */
  int32_t  early_rows;           /* 2 = the early rows of T start with the step (default), 1 = after the secondary NIFS, 0 = none */
  int32_t  stencil;              /* 1 = the built-in circuits' early rows without the sparse matrices (vdf_nova_pp_stencil) */
  int32_t  small_window;         /* fixed-base window of a side with fewer than 2^17 generators, 6..16 (15) */
  int32_t  big_window;           /* ... with 2^17 and more, 12..20 (16) */
  int32_t  packed_commit;        /* 1 = the reference circuit's rounds committed over derived generators (3t + 4 terms) */
  int32_t  lookahead_early;      /* 1 = the next step's rounds are launched under the primary side's wait */
  int32_t  gate_accumulate;      /* 1 = the lookahead's bucket accumulation is held behind the primary side's direct sum */
  int32_t  fold_on_rows;         /* 1 = the primary fold runs on the early rows' queue */
  int32_t  nifs_ahead;           /* 1 = a step launches the next step's first device phases on its way out */
  int32_t  early_row_parts;      /* 1..3: the early rows as an MSM job of that many parts (1) */
  int32_t  lookahead_priority;   /* wave priority of the lookahead's sort and bucket reduction, 0..3 (1) */
  int32_t  side_accumulate_fill; /* accumulation workgroups per CU the two side queues' MSMs fill, 1..3 (3) */
  int32_t  verbose;              /* 1 = decisions (skipped tables, the window chosen) on stderr */
  int32_t  compress_queues;      /* 1: vdf_nova_compress runs the primary side's two openings on two queues half a round apart (one
                                    opening's sort and bucket reduction under the other's accumulation); 0: in lockstep on one (1) */
  int32_t  rows_at_challenge;    /* 1: the primary fold and the next step's early rows are launched the moment the secondary circuit's
                                    synthesis has derived the fold challenge (a call-back from inside it); 0: after the synthesis (1) */
  int32_t  fold_fused;           /* 1: the stencil kernel of the next step's early rows applies the primary fold to ITS rows of A z, B z,
                                    C z and E on the way (vdf_nifs_cross_term_minroot_fold) and only z and the other rows are folded by a
                                    launch of their own, beside it; 0: one fold over whole vectors in front of the rows (0: measured; needs stencil) */
  int32_t  periodic_rows;        /* 1: a custom circuit whose vdf_cs_repeat rows are periodic (vdf_nova_pp_periodic_rows) gets their share of the
                                    cross term from the description, without the sparse matrices (vdf_nova_pp_stencil == 7); 0: the generic
                                    kernel over every row (0 until measured).  The proofs are the same bytes either way */
  int32_t  custom_ahead;         /* a custom circuit with a vdf_cs_repeat, in the steps a chain drives (vdf_nova_prove_step_custom_chain,
                                    vdf_nova_prove_recursively_custom): 0 = the repeat's rounds, their commitment and all of T inside the step
                                    (default); 1 = the NEXT step's rounds and their commitment on the lookahead queue, as for a built-in kind;
                                    2 = that, and the rows of T that read only those rounds and z_in on the early-rows queue
                                    (vdf_nova_pp_early_rows).  Costs one more `synthesize` per step (the probe, vdf_cs_is_probe).  The proofs
                                    are the same bytes in all three; every other circuit and driver ignores it */
} vdf_nova_tuning;
void vdf_nova_tuning_default(vdf_nova_tuning* out);
/* Host only.  The tuning a constructor would run with when handed `tuning` (NULL = the defaults): a struct_size smaller than this
 * build's, down to the struct as it was before `custom_ahead`, is a caller compiled against an older header -- the fields it does
 * not have read as 0; VDF_ERR_BAD_ARG for any other struct_size and for a field out of range.  out->struct_size = this build's. */
int  vdf_nova_tuning_read(const vdf_nova_tuning* tuning, vdf_nova_tuning* out);
/* public_params with the tuning given (NULL = the defaults); VDF_ERR_BAD_ARG for a field out of range */
int  vdf_nova_public_params_tuned(vdf_ctx* ctx, uint64_t num_iters_per_step, int circuit_kind, int gens_family,
                                  const vdf_nova_tuning* tuning, vdf_pp** out);
int  vdf_nova_pp_tuning(const vdf_pp* pp, vdf_nova_tuning* out);            /* the copy this parameter set runs with */
/* public_params under the given random-oracle block (NULL = the default) and tuning (NULL = the defaults) */
int  vdf_nova_public_params_ro(vdf_ctx* ctx, uint64_t num_iters_per_step, int circuit_kind, int gens_family,
                               const vdf_nova_ro_params* ro, const vdf_nova_tuning* tuning, vdf_pp** out);
/* wall-clock milliseconds of the stages of the call that made `pp`: [0] both shapes + digest (host), [1] shapes to the
 * device, [2] generators, [3] fixed-base tables (the packed commitment's included), [4] digit tables, [5] the rest, [6] total */
/* Parameters of the forward circuit in `lanes` lanes (VDF_CIRCUIT_MINROOT_FORWARD_LANES), t rounds per lane and step.
 * lanes == 1 returns exactly the parameters of VDF_CIRCUIT_MINROOT_FORWARD (same kind, same digest); lanes of 0 or above
 * VDF_NOVA_MAX_LANES is VDF_ERR_BAD_ARG.  ro / tuning: NULL = the defaults.  The digest is the oracle's `params` for
 * tests/lanes_spec.py's LanesForwardCircuit with digest_shapes(t, ...) as for the forward circuit.  tuning.stencil = 0 keeps
 * the generic rows kernel (the same bytes); vdf_nova_eval_and_prove refuses such parameters (its evaluator is one chain). */
int  vdf_nova_public_params_lanes(vdf_ctx* ctx, uint64_t num_iters_per_step, size_t lanes, int gens_family, const vdf_nova_ro_params* ro,
                                  const vdf_nova_tuning* tuning, vdf_pp** out);
size_t vdf_nova_pp_lanes(const vdf_pp* pp);     /* 1 for every kind but VDF_CIRCUIT_MINROOT_FORWARD_LANES */
/* ---- the cycle in either ORIENTATION ---------------------------------------------------------------------------------
 * The orientation of a parameter set is the field of its primary circuit, which is the VDF's field.  VDF_FIELD_FQ (G1 = Pallas,
 * G2 = Vesta: PallasVDF chains) is what every constructor above makes.  VDF_FIELD_FP is the reverse (G1 = Vesta, G2 = Pallas:
 * VestaVDF chains, what vdf_minroot_eval*(VDF_FIELD_FP) and vdf_minroot_eval_batch(VDF_FIELD_FP) produce).  Nothing else about
 * the protocol changes: the digest formula (no orientation byte: the matrices differ), the wire magics, the random-oracle blocks
 * and the generator families (seed / label per curve) are the same, and the secondary circuit is still TrivialTestCircuit.  A
 * proof attests a chain over ONE field.  Everything that takes a pp -- prove_step, prove_recursively[_windowed], eval_and_prove
 * (its evaluator thread runs the pp's field), verify, compress[_batch], verify_compressed[_batch], verify_batch, both
 * (de)serialisers, the _custom trio, introspection -- follows the pp's orientation; "primary" then reads "the Fp side, committed
 * on Vesta".  Refused with VDF_ERR_BAD_ARG and nothing done: a pp of one orientation with circuits of the other; a blob made
 * under the other orientation (its digest differs).  Canonicity of imported scalars is checked against each side's own modulus.
 *
 * The general constructor: every built-in kind; lanes is meaningful for VDF_CIRCUIT_MINROOT_FORWARD_LANES (1 gives the forward
 * circuit itself, as vdf_nova_public_params_lanes does) and must be 1 otherwise.  ro / tuning: NULL = the defaults.  The
 * constructors above are field = VDF_FIELD_FQ through the same code. */
int  vdf_nova_public_params_field(vdf_ctx* ctx, int field, uint64_t num_iters_per_step, int circuit_kind, size_t lanes, int gens_family,
                                  const vdf_nova_ro_params* ro, const vdf_nova_tuning* tuning, vdf_pp** out);
int  vdf_nova_pp_field(const vdf_pp* pp);       /* the orientation: VDF_FIELD_FQ / VDF_FIELD_FP (-1 for NULL) */
int  vdf_nova_pp_setup_ms(const vdf_pp* pp, double ms[7]);
/* bytes of HBM held per side: generators, their fixed-base table, the digit table (0 = none; *skipped bit s set when
 * side s wanted one and it did not fit).  The primary side's figures include the derived generators of the packed
 * commitment and their table.  (Not in these figures: after the first vdf_nova_compress / vdf_nova_verify_compressed a set also
 * keeps that call's scratch vectors, 0.18 GB for the reference's circuit at t = 2^16, until it is freed.) */
int  vdf_nova_pp_memory(const vdf_pp* pp, uint64_t gens_bytes[2], uint64_t table_bytes[2], uint64_t digit_bytes[2], uint32_t* skipped);
void vdf_nova_pp_free(vdf_pp* pp);
int  vdf_nova_pp_sizes(const vdf_pp* pp, int side, uint64_t* num_cons, uint64_t* num_vars, uint64_t* num_io, uint64_t* nnz3,
                       uint64_t* num_gens);
/* the 250-bit digest of the parameters (little-endian), and the run of primary variables the GPU fills (MinRoot rounds; for a
 * custom circuit the variables of its vdf_cs_repeat, filled by the GPU in the steps whose advice is in device memory; 0, 0 without one) */
int  vdf_nova_pp_digest(const vdf_pp* pp, uint8_t out[32]);
int  vdf_nova_pp_segment(const vdf_pp* pp, uint64_t* begin, uint64_t* len);
/* the run of primary constraints whose share of a step's cross term T and of comm_T prove_step makes ahead of the rest of
 * the step (they read only that segment, the step's input and the constant); len = 0: none, T is committed in one piece.
 * A custom circuit: the run when tuning.custom_ahead = 2 (the same rule: the longest run, no row of more than 8 entries per
 * matrix, at least 64 rows), else 0, 0 */
int  vdf_nova_pp_early_rows(const vdf_pp* pp, uint64_t* begin, uint64_t* len);
/* 4 / 3: the early rows are the built-in MinRoot stencil (the reference's rounds / the bound form), verified against the
 * shape's triples when the parameters were made -- their cross term runs without the sparse matrices
 * (vdf_hip.h vdf_nifs_cross_term_minroot); 5 (VDF_STENCIL_FORWARD): the forward circuit's stencil
 * (vdf_nifs_cross_term_minroot_forward) -- a CODE, not a count of variables per round (that circuit has 3; 3 and 4 were
 * taken); 0: they run through the generic sparse kernel (a custom circuit, or no early rows);
 * 6 (VDF_STENCIL_FORWARD_LANES): the forward circuit in lanes, all L (3t + 1) early rows as one run
 * (vdf_nifs_cross_term_minroot_forward_lanes) -- a code like 5;
 * 7 (VDF_STENCIL_PERIODIC): a custom circuit whose vdf_cs_repeat rows are periodic, with tuning.periodic_rows = 1: those rows run
 * from their description (vdf_hip.h vdf_nifs_cross_term_periodic), every other row through the generic kernel -- on the
 * early-rows queue when the step has early rows (tuning.custom_ahead = 2), on the step's own otherwise */
enum { VDF_STENCIL_FORWARD = 5, VDF_STENCIL_FORWARD_LANES = 6, VDF_STENCIL_PERIODIC = 7 };
int  vdf_nova_pp_stencil(const vdf_pp* pp);
/* 1 when the parameters of a custom circuit carry a periodic description of its vdf_cs_repeat rows (whatever the tuning says about
 * using it), else 0 and zeros: the rows [row_begin, row_begin + row_count) it covers (repetitions lead .. t - 1), the lead, and the
 * terms of one repetition in all three matrices.  Outputs may be NULL. */
int  vdf_nova_pp_periodic_rows(const vdf_pp* pp, uint64_t* row_begin, uint64_t* row_count, uint64_t* lead, uint64_t* terms_per_rep);
/* The same answer without a device (host only): builds the shape of the built-in step circuit at t, finds the early rows
 * and compares them with the stencil; returns 5 / 4 / 3 / 0 (negative: an error code).  Outputs may be NULL. */
int  vdf_nova_shape_stencil(uint64_t t, int circuit_kind, uint64_t* early_begin, uint64_t* early_len, uint64_t* seg_begin);

/* InverseMinRootCircuit::eval_and_make_circuits, :262-299: num_steps forward evaluations of
 * num_iters_per_step rounds each from initial_state (host, sequential), one circuit per step
 * holding (result, input) and -- beyond the reference -- the step's forward trace; circuits are
 * returned REVERSED (:294).  z0_primary = the final state (:278-281). */
int  vdf_nova_eval_and_make_circuits(int mode, uint64_t num_iters_per_step, size_t num_steps,
                                     const vdf_state* initial_state, vdf_fe z0_primary[3], vdf_circuits** out);
/* Moves every circuit's forward trace into HBM (outside the timed region: the trace is an input of
 * proving, produced by the untimed forward evaluation).  On checkpoint circuits: vdf_nova_circuits_materialize of all of
 * them with wait = 1, so that eval -> upload -> prove works with either kind. */
int  vdf_nova_circuits_upload(vdf_ctx* ctx, vdf_circuits* c);
/* The constructors of circuits with the chain's FIELD given: a handle remembers it (vdf_nova_circuits_field), and its evaluator,
 * its round counters (.i arithmetic), its push checks and the inverse walks / landing checks of vdf_nova_circuits_materialize
 * run over it.  The constructors without the argument are field = VDF_FIELD_FQ.  VDF_FIELD_FP ignores `mode`, as VestaVDF does. */
int  vdf_nova_eval_and_make_circuits_field(int field, int mode, uint64_t num_iters_per_step, size_t num_steps,
                                           const vdf_state* initial_state, vdf_fe z0_primary[3], vdf_circuits** out);
int  vdf_nova_circuits_from_checkpoints_field(int field, uint64_t t, uint64_t every, size_t num_steps, const vdf_state* states,
                                              vdf_fe z0_primary[3], vdf_circuits** out);
int  vdf_nova_circuits_forward_begin_field(int field, uint64_t t, const vdf_state* initial_state, vdf_fe z0_primary[3], vdf_circuits** out);
int  vdf_nova_circuits_lanes_begin_field(int field, uint64_t t, size_t lanes, const vdf_state* initial, vdf_fe* z0_primary, vdf_circuits** out);
int  vdf_nova_circuits_field(const vdf_circuits* c);      /* VDF_FIELD_FQ / VDF_FIELD_FP (-1 for NULL) */
/* The circuits of a chain evaluated ELSEWHERE.  states: the chain's states every `every` rounds in forward order,
 * num_steps * (t / every) + 1 of them, states[0] the initial state; `every` divides t (every = t: one state per step
 * boundary, exactly what the reference's circuits hold, :57-66).  Host only; holds the states and NO trace (96 bytes per
 * checkpoint instead of 64 (t + 1) per step).  Checked here: states[k].i == states[0].i + k * every (VDF_ERR_BAD_ARG,
 * vdf_nova_last_error names k).  Returned reversed like eval_and_make_circuits (:294); z0_primary = the final state. */
int  vdf_nova_circuits_from_checkpoints(uint64_t t, uint64_t every, size_t num_steps, const vdf_state* states,
                                        vdf_fe z0_primary[3], vdf_circuits** out);
/* Build the device-resident traces of circuits [first, first + count) (indices as prove_step's k) by inverse walks
 * (vdf_hip.h vdf_minroot_inverse_walk), one per checkpoint interval, on a side queue of `ctx`'s device; entry 0 of a step's
 * trace is its input state.  Steps that have a trace already are left alone (a second call is a no-op).  Every walk's landing
 * state is compared ON THE DEVICE with the checkpoint before it; bad (optional, count ints) gets 1 for a step with a walk that
 * missed, else 0.  Returns VDF_ERR_BAD_ARG (vdf_nova_last_error names the first such step) if any missed -- such a step is left
 * without a trace -- and VDF_ERR_OOM, nothing built, if the traces do not fit.  The traces of one call are ONE device
 * allocation, returned to the device when the last of them is released.
 * wait = 0 enqueues the first slice of the walks and returns (bad is not written); each prove_step over these circuits then
 * enqueues the share of the remaining rounds that finishes them by the step that needs them -- launches of a bounded number of
 * rounds (1,024; environment VDF_NOVA_WALK_LAUNCH) so that a queue shared with a prover is never held for long -- and the next
 * materialize / release / prove_step that needs the result enqueues what is left and waits for it; a walk that missed is
 * reported by that call.  On circuits that carry host traces: VDF_ERR_BAD_ARG (they have vdf_nova_circuits_upload). */
int  vdf_nova_circuits_materialize(vdf_ctx* ctx, vdf_circuits* c, size_t first, size_t count, int wait, int* bad);
/* frees those traces (steps without one are skipped: releasing a range never materialised is a no-op); not while a
 * prove_step over the circuits is running.  prove_step's guarantee -- nothing in flight reads the circuits' memory when it
 * returns -- makes a release between two steps safe. */
int  vdf_nova_circuits_release(vdf_circuits* c, size_t first, size_t count);
/* how many circuits have a device trace now, and the device memory the traces hold: resident x (t + 1) x 64 bytes, plus the
 * traces already released out of an allocation that others still use, plus the allocation a windowed prove_recursively keeps
 * between two windows (it exists only inside that call, so a single-threaded caller never sees it; vdf_nova_custom_chain_memory
 * counts it the same way).  Pending walks are not waited for.  Outputs may be NULL. */
int  vdf_nova_circuits_memory(const vdf_circuits* c, size_t* resident_steps, uint64_t* device_bytes);
/* the device trace of circuit k, 2 (t + 1) elements, NULL when it has none (pending walks over it are finished first): for
 * tests and tools */
int  vdf_nova_circuit_trace(const vdf_circuits* c, size_t k, const void** d_trace);
/* host memory the circuits hold in traces and checkpoints (bytes) */
int  vdf_nova_circuits_host_bytes(const vdf_circuits* c, uint64_t* bytes);

/* ---- forward chains: circuits that GROW (for parameters of VDF_CIRCUIT_MINROOT_FORWARD) -------------------------------
 * An empty chain of steps of t rounds that starts at initial_state; z0_primary = that state.  Steps are appended in the
 * order of evaluation and circuit k is the k-th one pushed, so a prover may run while the chain is still being evaluated.
 * There is NO lock: a push or a release must not overlap a vdf_nova_prove_step over the same circuits (between two steps
 * both are safe).  prove_step's lookahead stops at the end of the vector: the last step pushed so far runs without it.
 * prove_step with forward parameters over other circuits, or the other way round, is VDF_ERR_BAD_ARG.
 * vdf_nova_prove_recursively[_windowed] over a complete forward chain work as over any other circuits. */
int  vdf_nova_circuits_forward_begin(uint64_t t, const vdf_state* initial_state, vdf_fe z0_primary[3], vdf_circuits** out);
/* Appends one step from its host trace, 2 (t + 1) elements as vdf_minroot_eval writes them.  Entry 0 must be (x, y) of the
 * chain's current end (VDF_ERR_BAD_ARG otherwise, nothing appended); the step's result is entry t with i advanced by t.  The
 * trace is copied and reaches the device through the proof's staging buffer when the step (or its lookahead) runs. */
int  vdf_nova_circuits_push_trace(vdf_circuits* c, const vdf_fe* trace_xy);
/* Appends one step from its t / every + 1 states every `every` rounds (states[0] = the chain's current end, compared whole;
 * .i checked as vdf_nova_circuits_from_checkpoints checks it; `every` divides t and is the same for every such step of a
 * chain).  The step holds no trace until vdf_nova_circuits_materialize rebuilds it by inverse walks, each checked against
 * the checkpoint before it: the entry for an evaluator elsewhere that sends 96-byte states instead of 64 (t + 1) bytes a step.
 * vdf_nova_circuits_release on a forward chain also drops the host trace of a step pushed by vdf_nova_circuits_push_trace:
 * a long stream holds a bounded number of steps. */
int  vdf_nova_circuits_push_checkpoints(vdf_circuits* c, uint64_t every, const vdf_state* states);
/* ---- forward chains in LANES (for parameters of vdf_nova_public_params_lanes) -------------------------------------------
 * An empty chain of steps that advance `lanes` evaluations by t rounds each; z0_primary (3 lanes elements) = the initial states,
 * flattened.  A lanes chain of ONE lane is a forward chain (every call above works on it); on a chain of more lanes the
 * single-lane push calls return VDF_ERR_BAD_ARG.  Everything else -- materialize / release / memory / prove_step /
 * prove_recursively[_windowed] -- works as on a forward chain, a step's trace being `lanes` traces back to back, t + 1 entries each. */
int  vdf_nova_circuits_lanes_begin(uint64_t t, size_t lanes, const vdf_state* initial, vdf_fe* z0_primary, vdf_circuits** out);
/* Appends one step from `lanes` host traces, lane l's at trace_xy + 2 l lane_stride (lane_stride >= t + 1 entries of 64 B), each
 * checked as vdf_nova_circuits_push_trace checks one; a bad lane appends nothing and vdf_nova_last_error names it. */
int  vdf_nova_circuits_push_traces(vdf_circuits* c, const vdf_fe* trace_xy, size_t lane_stride);
/* Appends one step from every lane's t / every + 1 states: lane l's are states[l lane_stride + k], k = 0 .. t / every, each lane
 * checked as vdf_nova_circuits_push_checkpoints checks one (a bad lane appends nothing, vdf_nova_last_error names it).  With
 * lane_stride = rounds_total / every + 1 and the pointer advanced by step * t / every, the output of vdf_minroot_eval_batch
 * feeds in unchanged. */
int  vdf_nova_circuits_push_checkpoints_lanes(vdf_circuits* c, uint64_t every, const vdf_state* states, size_t lane_stride);
size_t vdf_nova_circuits_lanes(const vdf_circuits* c);
/* result / input of lane `lane` of circuit k (vdf_nova_circuit_states gives lane 0) */
int  vdf_nova_circuit_lane_states(const vdf_circuits* c, size_t k, size_t lane, vdf_state* result, vdf_state* input);
size_t vdf_nova_circuits_len(const vdf_circuits* c);
/* result / input of circuit k (k = 0 is proved first): InverseMinRootCircuit.result / .input */
int  vdf_nova_circuit_states(const vdf_circuits* c, size_t k, vdf_state* result, vdf_state* input);
void vdf_nova_circuits_free(vdf_circuits* c);

/* NovaVDFProof::prove_recursively(pp, circuits, num_iters_per_step, z0), :302-358: one prove_step
 * per circuit.  Returns VDF_ERR_* (the reference asserts success, :353). */
int  vdf_nova_prove_recursively(vdf_pp* pp, const vdf_circuits* circuits, uint64_t num_iters_per_step,
                                const vdf_fe z0[3], vdf_proof** out);
/* The same with the window chosen.  Over checkpoint circuits whose traces are not all resident, prove_recursively builds them
 * in windows of window_steps circuits: window 0 up front, then while window w is proved window w + 1 is walked on the side
 * queue and window w - 1 released -- never more than two windows of traces in HBM, whatever the chain's length.
 * window_steps = 0: as many steps as fit 1 GiB, at least 2 (255 at t = 2^16) -- what the plain call uses.  Circuits that carry
 * traces, or whose traces the caller has made resident, are proved exactly as before and nothing of theirs is released. */
int  vdf_nova_prove_recursively_windowed(vdf_pp* pp, const vdf_circuits* circuits, uint64_t num_iters_per_step,
                                         const vdf_fe z0[3], size_t window_steps, vdf_proof** out);
/* One RecursiveSNARK::prove_step (:342-349): *proof == NULL starts a new proof (the `None` case).  z0_secondary is
 * [0] (:310, :389-391).  What a step computes that does not depend on the chain -- the MinRoot rounds of circuit k and
 * their share of the commitment -- is enqueued one call early, for circuit k + 1 of the same `circuits`, on a second
 * context the proof owns; a call for any other step finds no such work waiting and does it then.  The results are
 * those of a prover without lookahead, and no call returns while anything in flight still reads the circuits' memory.
 * Over checkpoint circuits the traces of circuit k AND of circuit k + 1 (when there is one) must be resident
 * (vdf_nova_circuits_materialize): VDF_ERR_BAD_ARG "trace of circuit k not materialised" otherwise, nothing done. */
int  vdf_nova_prove_step(vdf_pp* pp, vdf_proof** proof, const vdf_circuits* circuits, size_t k, const vdf_fe z0[3]);
/* Evaluate a chain and prove it WHILE it is evaluated (forward parameters only).  A thread of this call runs
 * vdf_minroot_eval step by step from initial_state (num_steps steps of pp's t rounds) and hands each finished trace over
 * through a queue of at most 4; the calling thread pushes, proves and releases.  *out: the running proof of
 * z0 = initial_state, zi = *final_state (optional output), ready for verify / compress.  stats (optional): eval_ms = the
 * evaluator's time to its last round; after_eval_ms = from that moment to the return (the last step and the last secondary
 * commitment); max_backlog = the most steps evaluated and not yet proved at the start of a step (1: the prover kept up). */
typedef struct vdf_nova_stream_stats { double eval_ms, after_eval_ms; uint64_t max_backlog, steps; } vdf_nova_stream_stats;
int  vdf_nova_eval_and_prove(vdf_pp* pp, int mode, const vdf_state* initial_state, size_t num_steps, vdf_state* final_state,
                             vdf_proof** out, vdf_nova_stream_stats* stats);
/* NovaVDFProof::verify(pp, num_steps, z0, zi), :370-387: *ok = 1 iff the proof is valid for num_steps steps from z0
 * (two output hashes, three satisfiability claims), the verified zi_primary equals zi, and zi_secondary == [0]
 * (the Ok(bool) of :386). */
int  vdf_nova_verify(const vdf_proof* proof, vdf_pp* pp, size_t num_steps, const vdf_fe z0[3], const vdf_fe zi[3], int* ok);
void vdf_nova_proof_free(vdf_proof* proof);
size_t vdf_nova_proof_num_steps(const vdf_proof* proof);
/* Introspection for the parity tests.  Instances: commitments as affine points, u and X[2] in Montgomery form of the
 * instance's own scalar field (the parameters' field on the primary side, the other one on the secondary).  Witness pointers: device memory,
 * z = [W | u | X] (W = the first num_vars elements) and E (NULL for the fresh instance). */
enum { VDF_INST_RUNNING_PRIMARY = 0, VDF_INST_RUNNING_SECONDARY = 1, VDF_INST_FRESH_SECONDARY = 2,
       /* witness pointer only: z of the fresh primary instance the LAST prove_step folded (its instance: vdf_nova_proof_last_step);
        * valid until the next step */
       VDF_INST_FRESH_PRIMARY_LAST = 3 };
int  vdf_nova_proof_instance(const vdf_proof* proof, int which, vdf_affine* comm_W, vdf_affine* comm_E, vdf_fe* u, vdf_fe X[2]);
int  vdf_nova_proof_witness_ptrs(const vdf_proof* proof, int which, const void** d_z, const void** d_E);
int  vdf_nova_proof_zi(const vdf_proof* proof, vdf_fe zi_primary[3], vdf_fe zi_secondary[1]);
/* by-products of the last prove_step: the fresh primary instance, both cross-term commitments (identity in the base
 * step) and both fold challenges (canonical 128-bit integers, little-endian limbs) */
typedef struct { vdf_affine comm_W1; vdf_fe X1[2]; vdf_affine comm_T1, comm_T2; uint64_t r1[4], r2[4]; } vdf_nova_step_info;
int  vdf_nova_proof_last_step(const vdf_proof* proof, vdf_nova_step_info* out);
/* host wall-clock of the last prove_step, milliseconds: [0] enqueue + wait of the secondary cross term and commitments,
 * [1] synthesis of the primary augmented circuit, [2] upload + enqueue of the primary cross term and commitments,
 * [3] wait for them, [4] synthesis of the secondary augmented circuit, [5] upload + fold launches, [6] lookahead
 * launch, [7] total. */
int  vdf_nova_last_step_ms(const vdf_proof* proof, double ms[8]);
/* Per-launch timing of everything a prover enqueues (vdf_hip.h vdf_ctx_kernel_events) over its three queues -- queue[i] =
 * 0 the step's chain (the parameters' context), 1 the lookahead (MinRoot rounds of the next step and their commitment),
 * 2 the early rows of the cross term -- on one time line.  For bench.py's prove_step.roofline; measure rates with it off. */
int  vdf_nova_proof_set_kernel_timing(vdf_proof* proof, int enable);
int  vdf_nova_proof_kernel_events(vdf_proof* proof, vdf_kernel_event* out, int* queue, size_t cap, size_t* n);

/* ---- the step-circuit seam (src/nova/proof.rs:79-153: `impl StepCircuit for InverseMinRootCircuit` -- arity, synthesize,
 * output) ---------------------------------------------------------------------------------------------------------
 * A step circuit written by the host: `synthesize` receives the constraint system and the arity handles of z_in, makes
 * its variables and constraints through the vdf_cs_* calls below, and stores the handles of z_out.  The same function
 * runs in two modes, as a bellperson circuit does: when the parameters are made the constraints are recorded (values
 * are ignored); in every prove_step only the values are computed (vdf_cs_is_witness).  `output` of the trait is the
 * value of z_out after a witness synthesis.  The library's own circuits (both MinRoot forms, TrivialTestCircuit) sit
 * behind the same C++ interface (host/r1cs.hpp StepCircuit); a custom circuit's variables are made on the host, except those of
 * the uniform rounds it hands to vdf_cs_repeat (below) with their advice in device memory. */
typedef struct vdf_cs vdf_cs;
typedef uint32_t vdf_num;                 /* a linear combination with its value, owned by the vdf_cs */
typedef struct {
  size_t arity;
  int (*synthesize)(void* self, vdf_cs* cs, const vdf_num* z_in, vdf_num* z_out);       /* 0 = ok */
  void* self;
} vdf_step_circuit;
int     vdf_cs_is_witness(const vdf_cs* cs);                          /* 1: values are live; 0: the shape is being recorded */
int     vdf_cs_is_probe(const vdf_cs* cs);                            /* 1: the extra witness synthesis of tuning.custom_ahead (below) */
vdf_num vdf_cs_const(vdf_cs* cs, const vdf_fe* k);                    /* the constant k (Montgomery form) */
vdf_num vdf_cs_add(vdf_cs* cs, vdf_num a, vdf_num b);
vdf_num vdf_cs_sub(vdf_cs* cs, vdf_num a, vdf_num b);
vdf_num vdf_cs_scale(vdf_cs* cs, vdf_num a, const vdf_fe* k);
vdf_num vdf_cs_alloc(vdf_cs* cs, const vdf_fe* value);                /* a new variable (AllocatedNum::alloc) */
vdf_num vdf_cs_mul(vdf_cs* cs, vdf_num a, vdf_num b);                 /* a new variable a * b and its constraint */
int     vdf_cs_enforce(vdf_cs* cs, vdf_num a, vdf_num b, vdf_num c);  /* a * b = c */
int     vdf_cs_value(const vdf_cs* cs, vdf_num a, vdf_fe* out);       /* witness mode */
/* ---- uniform rounds of a custom circuit: vdf_cs_repeat ---------------------------------------------------------------------
 * t repetitions of one round, written once as a callback over the calls above and run, in a prove_step, by ONE GPU thread per
 * repetition (libvdf_hip.so vdf_round_tape_run) instead of t host callbacks.
 *
 * TRACING.  vdf_cs_repeat calls `body` exactly once, on a recording vdf_cs, and keeps what it did as a tape: a straight-line
 * program of add, sub, scale, const, mul (a variable and its constraint), alloc_from (a variable) and enforce.  Inside the body
 * only the handles it was given or made itself exist: any other handle, vdf_cs_alloc, vdf_cs_value and a nested vdf_cs_repeat set
 * the circuit's failure flag (as a bad handle does anywhere) and vdf_cs_repeat returns VDF_ERR_BAD_ARG with nothing allocated.
 * A body must not branch on values or on vdf_cs_is_witness: it is not run again.
 *
 * INPUTS of repetition j = 0 .. t - 1.  `j`: the constant j.  `inv`: n_inv loop-invariant numbers of the caller.  `carry`:
 * n_carry numbers -- carry_in for j = 0, the previous repetition's carry_out (as linear combinations) after that.  `cur` / `next`:
 * the n_adv columns of advice entries j and j + 1 as VALUE-ONLY handles: they, and sums / differences / multiples made of them,
 * feed vdf_cs_alloc_from and further value arithmetic; in vdf_cs_mul, vdf_cs_enforce or carry_out they are an error.
 *
 * ADVICE AND VALUES.  advice: (t + 1) entries of n_adv elements, entry-major, Montgomery form (a vdf_minroot_eval trace is
 * n_adv = 2), in host or device memory; NULL while the shape is recorded.  THE VALUE OF CARRY c IN REPETITION j IS ADVICE ENTRY j,
 * COLUMN c -- on the host path and on the device path alike, and the values of the returned carry_out are entry t (copied back
 * when the advice is in device memory).  That rule is what makes repetitions independent.  Advice that disagrees with what the
 * body computes (a wrong root, the trace of another step) therefore does not fail here: the witness is unsatisfiable,
 * vdf_nova_prove_step_custom returns VDF_OK and vdf_nova_verify_custom answers 0.  Nothing faults.
 *
 * MODES.  Shape: the tape is replayed t times on the host; variables and constraints are repetition-major in the order of the
 * body's calls, so the same circuit written as a plain loop has the same shape and the same digest.  Witness, host advice: the
 * tape is interpreted on the host (the fallback, and the reference of the device path).  Witness, device advice (inside
 * vdf_nova_prove_step_custom): the t n_vars variables are left out of the host's witness and a kernel writes them straight into
 * the fresh witness before it is committed; vdf_nova_pp_segment names the run.
 *
 * LIMITS, each VDF_ERR_BAD_ARG: one vdf_cs_repeat per circuit; 1 <= t < 2^31; n_carry <= n_adv; the caps below.  The parameters
 * keep the tape: a prove_step whose body records another one is VDF_ERR_BAD_ARG.
 *
 * THE CROSS TERM.  The rows of the repetitions come from replaying one tape, so from some repetition on they are periodic: the
 * parameters read that off the shape's triples, compare it with every triple of every repetition, and keep the description
 * (vdf_nova_pp_periodic_rows).  With tuning.periodic_rows = 1 a step's cross term then takes those rows from the description
 * (vdf_hip.h vdf_nifs_cross_term_periodic) and only the others through the sparse matrices; a circuit whose rows are not periodic
 * (a carry that accumulates: its rows grow with j) keeps the generic kernel.  Lookahead and early rows of the cross term: for
 * the steps a chain drives, tuning.custom_ahead (THE PROBE, below).  Out of scope for custom circuits: a second repeat. */
#define VDF_ROUND_MAX_INV 16
#define VDF_ROUND_MAX_CARRY 8
#define VDF_ROUND_MAX_ADV 8
#define VDF_ROUND_MAX_OPS 128      /* vdf_cs_* calls of one body */
#define VDF_ROUND_MAX_CONSTS 24    /* of them vdf_cs_const and vdf_cs_scale (one stored constant each) */
#define VDF_ROUND_MAX_VARS 64      /* variables per repetition (vdf_cs_mul, vdf_cs_alloc_from) */
#define VDF_ROUND_MAX_LIVE 24      /* values alive at once: an input counts from its first use, every value until its last;
                                      a value that no variable depends on does not count */
typedef struct {
  size_t n_inv, n_carry, n_adv;
  int (*body)(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* carry, const vdf_num* cur, const vdf_num* next,
              vdf_num* carry_out);                                      /* 0 = ok */
  void* self;
} vdf_round_body;
int     vdf_cs_repeat(vdf_cs* cs, const vdf_round_body* b, uint64_t t, const vdf_num* inv, const vdf_num* carry_in, const vdf_fe* advice,
                      vdf_num* carry_out);
/* CHAINS IN LANES.  vdf_cs_repeat_lanes runs `lanes` chains through ONE recorded body -- the custom circuit's counterpart of
 * VDF_CIRCUIT_MINROOT_FORWARD_LANES: one proof, one compress, one verify for all of them.  inv and the carries are lane-major
 * (lanes * n_inv and lanes * n_carry handles); lane l's advice starts lane_stride ENTRIES after lane l - 1's (lane_stride >= t + 1).
 * The value of carry c of lane l in repetition j is column c of entry j of lane l's advice.  Variables and constraints are
 * lane-major, then repetition-major: the circuit written as a plain `for l: for j:` loop has the same shape and digest, and
 * repetition j, constraint c of lane l is row row_begin + (l * t + j) * n_cons + c (vdf_nova_pp_repeat_rows / _lanes).  It still
 * counts as the circuit's one repeat, and the parameters keep `lanes`.  With device advice a prove_step writes all lanes' variables
 * by ONE launch (vdf_hip.h vdf_round_tape_run_lanes); with host advice the tape is interpreted on the host.  VDF_ERR_BAD_ARG besides
 * vdf_cs_repeat's refusals: lanes outside 1 .. VDF_TAPE_MAX_LANES, lanes * n_inv > VDF_TAPE_MAX_INV, lane_stride < t + 1, and -- when
 * the advice lies in the trace a chain built for the step (vdf_cs_step_advice below: lanes * (t + 1) entries, owned by the library)
 * -- a repeat that would read past that trace: there lane_stride must be t + 1 and t, lanes and n_adv the chain's (the stride of
 * vdf_nova_custom_chain_lanes_from_checkpoints is that of the CHECKPOINTS and is not this one).  Periodic
 * rows are out of scope for more than one lane: the parameters keep no description and tuning.periodic_rows = 1 gives the generic
 * kernel.  vdf_cs_repeat is this call with lanes = 1 and lane_stride = t + 1, through the same code. */
int     vdf_cs_repeat_lanes(vdf_cs* cs, const vdf_round_body* b, uint64_t t, size_t lanes, const vdf_num* inv, const vdf_num* carry_in,
                            const vdf_fe* advice, size_t lane_stride, vdf_num* carry_out);
vdf_num vdf_cs_alloc_from(vdf_cs* cs, vdf_num src);                    /* a new variable with src's value, no constraint */
/* THE ROUND CONSTANT OF ROUND j FROM A TABLE (vdf_hip.h VDF_TAPE_TAB).  vdf_cs_tab(cs, table, rows, cols, col) = table[(j mod rows)
 * * cols + col], j the counter the body was handed: a short fixed list cycled over the rounds, as VeeDo / MiMC-style roots and
 * Rescue- or Poseidon-shaped rounds add one; a 0 / 1 column switches a term on and off by round.  table: rows x cols elements,
 * row-major, canonical Montgomery form, HOST memory, 1 <= rows <= VDF_TAPE_MAX_TAB_ROWS, 1 <= cols <= VDF_TAPE_MAX_TAB_COLS, col <
 * cols.  Legal ONLY while a body is recorded -- a round, walk or forward body; on a live vdf_cs it sets the failure flag, as
 * vdf_cs_pow does.  ONE table per body: a second call with another (pointer, rows, cols) sets the failure flag, as do a null
 * table and dimensions outside the caps.  A recording copies nothing: the caller keeps the table alive and unchanged for as long
 * as the circuit or the tape is in use.  The tape that vdf_nova_round_body_record, _walk_body_record and _forward_body_record hand
 * out names the CALLER'S pointer (out->table, tab_rows, tab_cols) -- host memory, so the tape goes to the host evaluators below as it is, and to a launcher of vdf_hip.h with `table`
 * replaced by a device-readable copy.
 * In a ROUND body the result is a constant handle, like j: usable in linear combinations, vdf_cs_mul, vdf_cs_enforce and carry_out;
 * in repetition j it contributes table[j mod rows][col] on the constant's column, so the same circuit written as a plain loop
 * with vdf_cs_const(&table[(j % rows) * cols + col]) has the same shape and the same digest.  In walk and forward bodies it is a
 * value.  It costs one call of VDF_ROUND_MAX_OPS and no stored constant.
 * The parameters of a custom circuit keep a copy of the table with the tape and ONE device copy, freed with them; a step whose
 * recorded body has another table -- one element is enough -- is "differs from the one these parameters were made with" (the
 * comparison is one pass over the table per step on the host, and one more for a probe of tuning.custom_ahead).  Rows
 * that read a table are periodic only with the table's period: the detection compares every triple of every repetition and
 * keeps the generic kernel for them (tuning.periodic_rows = 1 included).
 * CHAINS.  A chain's walks see the chain-global J (step g: j_base + g * t + ...), the round body's j is step-local; the two name
 * the same row only when tab_rows divides t and every j_base, and vdf_nova_custom_chain_[lanes_]from_checkpoints refuse anything
 * else (VDF_ERR_BAD_ARG naming the check).  There the walk tape's table is HOST memory; the chain copies it, makes one device copy
 * with its first walks, and counts both in _host_bytes and _memory. */
vdf_num vdf_cs_tab(vdf_cs* cs, const vdf_fe* table, size_t rows, size_t cols, size_t col);
/* Host only.  Records a body and hands out its tape for vdf_round_tape_run (ops / consts: caller's arrays of the two caps, which
 * out->ops / out->consts then point into); out->n_cons = the constraints per repetition.  field: the body's field. */
int  vdf_nova_round_body_record(int field, const vdf_round_body* b, vdf_tape_op ops[VDF_TAPE_MAX_OPS], vdf_fe consts[VDF_TAPE_MAX_CONSTS],
                                vdf_round_tape* out);
/* Host only.  What vdf_round_tape_run computes, on the host: out = the t n_vars variables (inv, advice, out: host memory). */
int  vdf_nova_round_tape_eval(int field, const vdf_round_tape* tape, uint64_t t, const vdf_fe* inv, const vdf_fe* advice, vdf_fe* out);
/* ---- walk bodies: the advice of such rounds, rebuilt on the GPU from checkpoints (vdf_hip.h vdf_round_tape_walk) -------------
 * The fast direction of the round, written once: `next` holds the n_adv columns of advice entry j + 1, `j` the index of the entry
 * to produce (the j of the round body whose repetition j relates entries j and j + 1), `inv` n_inv loop-invariant values; the body
 * stores the handle of every column of entry j in cur_out.  It is called once, on a recording vdf_cs, where vdf_cs_add, _sub,
 * _scale, _const and _mul are VALUE arithmetic: _mul makes no variable and no constraint.  vdf_cs_alloc, _alloc_from, _enforce,
 * _value, _repeat and handles the body was not given or did not make set the failure flag: VDF_ERR_BAD_ARG.  cur_out[c] may be
 * any handle the body owns: an input passed straight through, or one handle in two columns.  Slots are allocated as for a round
 * body (inputs loaded at first use, live ranges, a linear scan).  The caps are VDF_ROUND_MAX_INV / _ADV / _OPS / _CONSTS / _LIVE,
 * and live values + 2 * n_adv <= VDF_WALK_MAX_SLOTS; one beyond is VDF_ERR_BAD_ARG.  The slow direction of a delay function, an
 * exponentiation by a 254-bit number, is recorded as a forward body (vdf_nova_forward_body_record below, vdf_cs_pow).
 *
 * The chain's checkpoints (vdf_round_tape_eval_batch, vdf_minroot_eval_checkpoints, or the caller's own evaluator) are then all a prover needs: one
 * vdf_round_tape_walk per window of steps leaves the traces where vdf_cs_repeat reads its advice, and checks every landing
 * against the checkpoint below it.  examples/prove_custom_checkpoints.c. */
typedef struct {
  size_t n_inv, n_adv;
  int (*body)(void* self, vdf_cs* cs, vdf_num j, const vdf_num* inv, const vdf_num* next, vdf_num* cur_out);      /* 0 = ok */
  void* self;
} vdf_walk_body;
/* Host only.  Records a walk body and hands out its walk tape (ops / consts as vdf_nova_round_body_record); n_vars = n_adv, n_cons = 0. */
int  vdf_nova_walk_body_record(int field, const vdf_walk_body* b, vdf_tape_op ops[VDF_TAPE_MAX_OPS], vdf_fe consts[VDF_TAPE_MAX_CONSTS],
                               vdf_round_tape* out);
/* Host only.  vdf_round_tape_walk restated on the host: the same arguments, the same refusals, every pointer host memory -- the
 * reference of the device path, byte for byte.  The refusals of this and of every restatement below are not written twice: both
 * libraries read them from one header (csrc/tape_launch.h; the periodic rows' from csrc/periodic_rules.h), so a call is refused
 * here for what its launcher refuses it for, in the same order, with the same code and the same words. */
int  vdf_nova_walk_tape_eval(int field, const vdf_round_tape* tape, const vdf_fe* inv, vdf_fe* entries, size_t n, uint64_t rounds,
                             vdf_fe* trace, size_t walk_stride, size_t top, size_t group, size_t group_stride, uint64_t j_base,
                             uint64_t j_group_step, int heads, const vdf_fe* expect, int32_t* ok);
/* Host only.  vdf_round_tape_run_lanes and vdf_round_tape_walk_lanes (vdf_hip.h) restated on the host: the same arguments, the same
 * refusals (the caps on lanes and lanes * n_inv, lane_stride < t + 1, the slot cap with n_inv counted), every pointer host memory
 * -- the references of the device paths, byte for byte.  With lanes = 1 they write what vdf_nova_round_tape_eval and
 * vdf_nova_walk_tape_eval write. */
int  vdf_nova_round_tape_eval_lanes(int field, const vdf_round_tape* tape, uint64_t t, size_t lanes, const vdf_fe* inv, const vdf_fe* advice,
                                    size_t lane_stride, vdf_fe* out);
int  vdf_nova_walk_tape_eval_lanes(int field, const vdf_round_tape* tape, size_t lanes, const vdf_fe* inv, vdf_fe* entries, size_t n,
                                   uint64_t rounds, vdf_fe* trace, size_t walk_stride, size_t top, size_t group, size_t group_stride,
                                   const uint64_t* j_base, uint64_t j_group_step, int heads, const vdf_fe* expect, int32_t* ok);
/* ---- forward bodies: the chain itself evaluated on the GPU (vdf_hip.h vdf_round_tape_forward_walk / vdf_round_tape_eval_batch) --
 * The slow direction of the round, written once, in the same struct: the `next` argument holds the n_adv columns of the entry the
 * walk STANDS ON (entry j), `j` is that entry's index (the j of the round body whose repetition j relates entries j and j + 1),
 * and the body stores the handle of every column of entry j + 1 in cur_out.  Everything else is as for a walk body -- value
 * arithmetic only, the same refusals, the same caps, each refused one beyond -- with two more calls:
 *   vdf_cs_pow(cs, a, e) = a ^ e, e a PLAIN 256-bit little-endian integer (e = 0 gives 1, also for a = 0).  One call, one result
 *   slot, the exponent one stored constant under VDF_ROUND_MAX_CONSTS.  It is legal ONLY while a forward body is recorded: on a
 *   live vdf_cs, in a round body and in a descending walk body it sets the failure flag, as a bad handle does.  A power inside
 *   a circuit would need constraints and is the circuit author's business.
 * With the three bodies of one round (forward, walk, round) a delay function the library did not write runs the whole pipeline
 * on the device: vdf_round_tape_eval_batch -> checkpoints -> vdf_round_tape_walk -> vdf_nova_prove_step_custom.
 * examples/prove_custom_pipeline.c.  A throughput feature for many chains, not a faster single chain (vdf_hip.h). */
vdf_num vdf_cs_pow(vdf_cs* cs, vdf_num a, const uint64_t e[4]);
/*   vdf_cs_pow_chain(cs, a, steps, n_steps) = a ^ E, E the exponent of the caller's ADDITION CHAIN (vdf_hip.h vdf_pow_step: a
 *   straight-line program over an accumulator and a few temporaries; every real delay function of this family is a power by a huge
 *   fixed exponent, and its authors have such a chain).  Recorded as ONE VDF_TAPE_POWC: one call, one result slot; the chain takes
 *   ceil((4 + 4 n_steps) / 32) packed constants under VDF_ROUND_MAX_CONSTS, and its temporaries count against the slot cap: live
 *   values + 2 * n_adv + (the largest n_tmp of the body's chains) <= VDF_WALK_MAX_SLOTS.  The value is byte for byte vdf_cs_pow(cs,
 *   a, E)'s; on the device the chain's products stay in the lazy domain and only the result is made canonical.  Legal ONLY while a
 *   forward body is recorded, as vdf_cs_pow; there and for an invalid chain it sets the failure flag. */
vdf_num vdf_cs_pow_chain(vdf_cs* cs, vdf_num a, const vdf_pow_step* steps, size_t n_steps);
/* Host only.  Validates a chain (vdf_hip.h: VDF_ERR_BAD_ARG, vdf_nova_last_error names the step) and returns its exponent e (a plain
 * 256-bit little-endian integer), the temporaries it needs (its largest index + 1) and its product count, max(1, squarings + steps
 * with a product) -- what VDF_FORWARD_TAPE_MAX_WORK counts.  Each output may be NULL. */
int  vdf_nova_pow_chain_exponent(const vdf_pow_step* steps, size_t n_steps, uint64_t e[4], uint32_t* n_tmp, uint64_t* products);
/* Host only.  A chain for ANY exponent e >= 1: left to right, sliding windows of at most `window` bits (2 .. 4).  The table comes
 * first, always whole: T[1] = x^2 and the odd powers T[1 + k] = x^(2k + 1) up to 2^window - 1 (2^(window - 1) + 1 temporaries, one
 * squaring and 2^(window - 1) - 1 products); then one step per window.  For both MinRoot root exponents window 4 gives 316 products
 * (252 squarings, 56 products, 8 for the table) against 377 of VDF_TAPE_POW's square-and-multiply and 283 / 282 of the hand-made
 * chains.  steps: `cap` steps of room; *n_steps: the steps written.  VDF_ERR_BAD_LENGTH when the chain does not fit cap or
 * VDF_POW_CHAIN_MAX_STEPS (window 2 over a dense exponent), VDF_ERR_BAD_ARG for e = 0 or a window outside 2 .. 4. */
int  vdf_nova_pow_chain_window(const uint64_t e[4], unsigned window, vdf_pow_step* steps, size_t cap, size_t* n_steps);
/* Host only.  The library's own two chains for the MinRoot fifth root x -> x^(1/5 mod (m - 1)) (src/minroot.rs:88-127 over Fq,
 * :223-261 over Fp), as the host evaluator and vdf_minroot_forward_walk run them: 32 steps (padded with steps that do nothing), 9
 * temporaries, 253 squarings, 30 products over Fq and 29 over Fp.  cap < 32: VDF_ERR_BAD_LENGTH. */
int  vdf_minroot_pow_chain(int field, vdf_pow_step* steps, size_t cap, size_t* n_steps);
/* Host only.  Records a forward body and hands out its forward walk tape (ops / consts as vdf_nova_round_body_record); n_vars = n_adv, n_cons = 0. */
int  vdf_nova_forward_body_record(int field, const vdf_walk_body* b, vdf_tape_op ops[VDF_TAPE_MAX_OPS], vdf_fe consts[VDF_TAPE_MAX_CONSTS],
                                  vdf_round_tape* out);
/* Host only.  vdf_round_tape_forward_walk restated on the host: the same arguments, the same refusals, every pointer host memory --
 * the reference of the device path, byte for byte. */
int  vdf_nova_forward_tape_eval(int field, const vdf_round_tape* tape, const vdf_fe* inv, vdf_fe* entries, size_t n, uint64_t rounds,
                                vdf_fe* checkpoints, uint64_t every, size_t cp_stride, vdf_fe* trace, size_t walk_stride, uint64_t base,
                                uint64_t j_base, uint64_t j_walk_step);
/* Host only.  vdf_round_tape_rebuild_lanes (vdf_hip.h) restated on the host: the same arguments, the same refusals (the rules of a
 * forward walk tape, the caps on lanes and lanes * n_inv, a null j_base, expect without ok, base + rounds > walk_stride, the slot cap
 * with n_inv and the chains' n_tmp counted, the work cap), every pointer host memory -- the reference of the device path, byte for
 * byte.  The index arithmetic is the launcher's own statement (csrc/tape_launch.h), the interpreter the host's. */
int  vdf_nova_forward_tape_rebuild_eval_lanes(int field, const vdf_round_tape* forward_tape, size_t lanes, const vdf_fe* inv, vdf_fe* entries,
                                              size_t n, uint64_t rounds, vdf_fe* trace, size_t walk_stride, uint64_t base, size_t group,
                                              size_t group_stride, const uint64_t* j_base, uint64_t j_group_step, int heads,
                                              const vdf_fe* expect, int32_t* ok);

/* public_params / prove_step / verify for a custom primary step circuit (the secondary stays TrivialTestCircuit).
 * z0, zi: `arity` elements.  compress, verify_compressed and the wire formats work on such proofs unchanged. */
int  vdf_nova_public_params_custom(vdf_ctx* ctx, const vdf_step_circuit* primary, int gens_family, vdf_pp** out);
int  vdf_nova_prove_step_custom(vdf_pp* pp, vdf_proof** proof, const vdf_step_circuit* primary, const vdf_fe* z0);
int  vdf_nova_verify_custom(const vdf_proof* proof, vdf_pp* pp, size_t num_steps, const vdf_fe* z0, const vdf_fe* zi, int* ok);
/* the same parameters in the orientation `field`: the custom circuit is synthesised over that field (vdf_cs_* values are its elements) */
int  vdf_nova_public_params_custom_field(vdf_ctx* ctx, int field, const vdf_step_circuit* primary, int gens_family, vdf_pp** out);
/* ... with the tuning given (NULL = the defaults, what the two constructors above use); VDF_ERR_BAD_ARG for a field out of range */
int  vdf_nova_public_params_custom_tuned(vdf_ctx* ctx, int field, const vdf_step_circuit* primary, int gens_family,
                                         const vdf_nova_tuning* tuning, vdf_pp** out);

/* ---- a custom circuit's chain: proved from its checkpoints, the walks a window ahead of the prover ---------------------------
 * What vdf_circuits is to the built-in kinds, for a circuit whose rounds are a vdf_cs_repeat and whose advice a walk tape rebuilds:
 * the chain's checkpoints on the host, and per step a device trace of t + 1 advice entries that exists only while the step's
 * window is proved.  The walks run on a side queue of the prover's device, all walks of a window in one vdf_round_tape_walk per
 * slice of rounds, and are finished by the call that needs their result.
 *
 * vdf_nova_custom_chain_from_checkpoints: `checkpoints` = num_steps * (t / every) + 1 entries of walk_tape->n_adv elements,
 * entry-major, Montgomery form, forward order, entry 0 the chain's start; host or device memory (vdf_ptr_is_device; a device array
 * -- one chain's slice of vdf_round_tape_eval_batch's output -- is downloaded once).  The chain keeps host copies of the tape,
 * of `inv` (walk_tape->n_inv elements, host memory) and of the checkpoints, and no trace.  j_base: the VDF_TAPE_J that the walk
 * producing entry 1 sees, minus 0 (the rule of vdf_round_tape_walk); step g's group of walks gets j_base + g * t.  Refused with
 * VDF_ERR_BAD_ARG on the host, nothing allocated on a device, vdf_nova_last_error naming the check: a walk tape that
 * vdf_round_tape_walk would refuse (a malformed op, n_vars != n_adv, an ADV with b = 0, a POW, the slot cap), `every` = 0 or not
 * dividing t, t = 0 or t >= 2^31, num_steps = 0, a null pointer, an unknown field.
 *
 * vdf_nova_custom_chain_materialize has the semantics of vdf_nova_circuits_materialize.  The traces of the steps of [first, first
 * + count) that are not resident are ONE device allocation (of the whole range when none is: count * (t + 1) * n_adv elements,
 * step g's trace at (g - first) * (t + 1) * n_adv, entries 0 .. t -- what vdf_cs_repeat reads as advice).  One walk per checkpoint
 * interval of every step; a slice with `done` rounds behind it is vdf_round_tape_walk(rounds = now, top = every - done,
 * walk_stride = every, group = t / every, group_stride = t + 1, j_base = the chain's + first * t, j_group_step = t), now = min(every
 * - done, launch_rounds) (vdf_nova_custom_chain_slice; launch_rounds = 0: 1,024); heads = 1, expect and ok only in the slice that
 * finishes the walks.  wait = 0 enqueues the first slice and returns; later calls pump and resolve.  A step with a walk that missed
 * its checkpoint is left without a trace, bad[k - first] = 1 (bad: count ints or NULL), and the call that resolves returns
 * VDF_ERR_BAD_ARG "step k: a walk did not land on the checkpoint below it" for the first such step.
 * _release / _memory / _host_bytes / _len / _free: as their vdf_nova_circuits_* counterparts.  _advice: the device trace of step k,
 * NULL when none is resident; pending walks over the step are finished first (for tests and tools).
 *
 * vdf_cs_step_advice: inside a synthesize driven by vdf_nova_prove_step_custom_chain or vdf_nova_prove_recursively_custom, in
 * witness mode, the device trace of the step being proved; NULL in every other case (a shape being recorded, a round or walk
 * body, plain vdf_nova_prove_step_custom).  A circuit writes vdf_cs_repeat(cs, &body, t, inv, carry_in, vdf_cs_is_witness(cs) ?
 * vdf_cs_step_advice(cs) : NULL, out) and needs no per-step state of its own; its shape and digest do not depend on the call.
 *
 * vdf_nova_prove_step_custom_chain: vdf_nova_prove_step_custom for step k of the chain, k = the steps the proof has (0 for *proof
 * = NULL).  Pending walks are finished if they cover k; VDF_ERR_BAD_ARG "advice of step k not materialised" when the trace is
 * absent (nothing else is done); the other pending walks get their share of rounds; then the step runs.  Also VDF_ERR_BAD_ARG: a
 * chain over the other field than the parameters' orientation, k beyond the chain or out of order, a chain whose t or n_adv is
 * not the parameters' vdf_cs_repeat's.
 * vdf_nova_prove_recursively_custom: the loop of vdf_nova_prove_recursively_windowed -- window 0 materialised and waited for,
 * window 1 enqueued, then step by step; after the last step of window w, window w is released and window w + 2 begun: never more
 * than two windows of traces in HBM (and one spare allocation).  window_steps = 0: as many steps as fit 1 GiB, at least 2; 1 is
 * raised to 2.  On an error nothing stays in flight, what the call built is released and *proof = NULL; the chain is left as it
 * was found.  The proof is byte for byte the one vdf_nova_prove_step_custom makes step by step from the same advice.
 * flags & VDF_CUSTOM_CHECK_STEPS: after every step vdf_nova_proof_last_unsat runs, and a non-zero count ends the call with
 * VDF_ERR_BAD_ARG "step k: N unsatisfied rows, first row r (repetition j, constraint c of the repeat)" (the parenthesis for a
 * row of the repeat; "lane l, repetition j, ..." when the repeat has more than one lane).  Without the flag wrong advice is not an error, as in vdf_cs_repeat above.
 *
 * CHAINS IN LANES (vdf_cs_repeat_lanes).  vdf_nova_custom_chain_lanes_from_checkpoints takes `lanes` chains of equal length: lane l's
 * num_steps * (t / every) + 1 checkpoints start lane_stride ENTRIES after lane l - 1's -- with lane_stride = rounds_total / every + 1
 * that is `lanes` consecutive chains of vdf_round_tape_eval_batch's output unchanged, from host or device memory.  inv: lanes *
 * n_inv elements, lane-major; j_base: `lanes` counters (host memory).  A step's trace is then lanes * (t + 1) entries, lane l's t + 1
 * at l * (t + 1): what vdf_cs_repeat_lanes reads at lane_stride = t + 1.  materialize makes lanes * (t / every) walks per step and ONE
 * vdf_round_tape_walk_lanes per slice for the whole window (group = t / every, group_stride = t + 1, j_base[l] = the lane's +
 * first * t, j_group_step = t); a walk that misses is reported as "step k, lane l: a walk did not land on the checkpoint below it".
 * Refused with VDF_ERR_BAD_ARG besides the above: lanes outside 1 .. VDF_TAPE_MAX_LANES, lanes * n_inv > VDF_TAPE_MAX_INV,
 * lane_stride < num_steps * (t / every) + 1, a null j_base, and for lanes > 1 the slot cap of vdf_round_tape_walk_lanes (n_inv more
 * slots).  vdf_nova_custom_chain_host_bytes counts, besides the tape, inv and the checkpoints, the staging copy of a window's starts
 * and targets (2 * walks entries, lanes > 1 only) while that window's walks are pending; it is freed when they resolve.
 * vdf_nova_custom_chain_from_checkpoints is this call with lanes = 1.  The two provers work unchanged above it and refuse a
 * chain whose lanes are not the parameters' ("the chain has L lanes, the parameters' vdf_cs_repeat has M").
 *
 * LOOKAHEAD AND EARLY ROWS (tuning.custom_ahead = 1 / 2; 0, the default, is the schedule above launch for launch).  A chain knows
 * step k + 1's advice while step k runs, so the rounds of step k + 1's repeat and their commitment can be made on the lookahead
 * queue during step k, and (mode 2) the rows of T that read nothing but those rounds, z_in and the constant on the early-rows queue,
 * as for a built-in kind.  What the library does not know is the repeat's `inv` of step k + 1: linear combinations of variables
 * only `synthesize` makes.  THE PROBE: once step k's primary circuit has produced z_(k+1), `synthesize` is called ONE EXTRA TIME per
 * step on a throw-away witness-mode vdf_cs whose z_in holds z_(k+1) and whose vdf_cs_step_advice is step k + 1's trace.
 * vdf_cs_is_probe answers 1 there (0 everywhere else), so a circuit may skip host work it does not need; in that call
 * vdf_cs_repeat[_lanes] records the body and keeps the values of `inv`, reads nothing of the advice (the carry_out it returns have
 * the value 0), and makes no variable and no row; everything else the circuit does works on values nobody keeps.  THE CONTRACT:
 * `synthesize` must be a function of z_in and the step's advice -- a circuit that counts its calls, or computes `inv` from anything
 * else, is not broken by the probe but gets nothing from it.  The real step compares what its own vdf_cs_repeat sees with what the
 * lookahead used: the bytes of `inv`, the advice pointer, t, lanes and lane_stride, the chain object and k.  Equal: a HIT, the
 * rounds are not made again.  Anything else: a MISS -- the side queues are drained, what they made is discarded, and the step runs
 * as under custom_ahead = 0.  No lookahead is attempted (the step is SKIPPED) over a trace whose walks are still pending or not
 * checked against their checkpoints, or beyond the chain.  A miss or a skip costs time, never correctness: the proof is byte for
 * byte the same in every case.  vdf_nova_proof_ahead_stats counts the three.  A repeat whose rows read some other variable of the
 * circuit has no early rows, and mode 2 is mode 1 for it.
 * Out of scope for custom chains: custom_ahead for steps not driven by a chain (plain vdf_nova_prove_step_custom keeps the schedule
 * of custom_ahead = 0: the library does not know its next advice), a second vdf_cs_repeat, lanes of different length.
 *
 * ASCENDING CHAINS: rounds without a cheap inverse.  A walk tape may hold no power, so the constructors above serve rounds whose
 * inverse direction is a handful of products.  A Rescue-shaped round (a root layer and a power layer: a 254-bit exponentiation in
 * BOTH directions) or a round with a lossy mix (no inverse at all) has no such tape.  vdf_nova_custom_chain_from_checkpoints_forward
 * and vdf_nova_custom_chain_lanes_from_checkpoints_forward build the same object from the chain's own FORWARD tape (the one
 * vdf_round_tape_eval_batch evaluated it with; POW, POWC and TAB admitted): one walk per checkpoint interval starts on the
 * checkpoint BELOW it, walks up, and is compared with the checkpoint ABOVE.  Checkpoints, lane_stride, inv, the copy of the table
 * and the rule that tab_rows divides t and every j_base are as above.  j_base means the same number in both directions -- the
 * VDF_TAPE_J of the round between entries 0 and 1 -- so one chain's two tapes take the same argument.  A slice with `done` rounds
 * behind it is vdf_round_tape_rebuild_lanes(rounds = now, base = done, walk_stride = every, group = t / every, group_stride = t + 1,
 * j_base[l] = the lane's + first * t, j_group_step = t, heads = 1), expect and ok only in the slice that finishes; lanes = 1 is the
 * same call.  launch_rounds = 0 means min(1,024, VDF_FORWARD_TAPE_MAX_WORK / the tape's products per round), and a larger value of
 * the caller's is LOWERED to that bound, not refused (a launch of a power tape may not hold a queue longer):
 * vdf_nova_custom_chain_launch_rounds says what a value becomes.  A walk that misses reads "step k[, lane l]: a walk did not land on
 * the checkpoint above it".  Refused with VDF_ERR_BAD_ARG: what vdf_round_tape_rebuild_lanes refuses of the tape, and the list above.
 * Everything above the constructors -- materialize, release, memory, host_bytes, advice, vdf_cs_step_advice, both provers,
 * VDF_CUSTOM_CHECK_STEPS, custom_ahead, both orientations -- works unchanged above an ascending chain.  A capability and a matter of
 * resident memory (checkpoints, not traces), NOT of speed: a lane spends about 0.1 ms per round of a fifth root, so an ascending
 * chain wants dense checkpoints, and a round WITH a cheap inverse keeps its descending tape.
 *
 * CHAINS THAT GROW: proved while they are evaluated.  vdf_nova_custom_chain_begin makes an EMPTY chain that stands on `initial`
 * (lanes * n_adv elements, lane-major: entry 0 of every lane; host memory).  tape: the walk tape (direction = VDF_CHAIN_DESCENDING)
 * or the chain's forward tape (VDF_CHAIN_ASCENDING); inv, t, lanes and j_base as the four constructors take them, and every refusal
 * of theirs that does not concern checkpoints applies (the tape's rules, t, lanes, a table's tab_rows dividing t and every j_base),
 * besides a direction that is neither.  Each push appends ONE step, step k being the k-th pushed, and _len grows by one:
 * - vdf_nova_custom_chain_push_checkpoints: every lane's t / every + 1 checkpoints of the step, lane l's at checkpoints + l *
 *   lane_stride * n_adv (host or device memory; lane_stride in entries, at least t / every + 1, not read for one lane);
 * - vdf_nova_custom_chain_push_advice: every lane's whole trace, t + 1 entries, lane l's at advice + l * lane_stride * n_adv (host
 *   memory; lane_stride at least t + 1).  The chain keeps a host copy until the step is released.
 * THE JOINT IS CHECKED: entry 0 of every lane of a pushed step must equal, byte for byte, the chain's end -- `initial` before the
 * first push, then the last entry of the last push, per lane.  Otherwise VDF_ERR_BAD_ARG "lane l: the step does not start on the
 * chain's end" and nothing is appended (as vdf_nova_circuits_push_trace).  ONE HAND-OVER PER CHAIN: the first push decides between
 * checkpoints and advice, and the other call on the same chain is VDF_ERR_BAD_ARG from then on; for checkpoints it also decides
 * `every` (it must divide t), and a push with another is refused -- a walk job is a contiguous run of steps with one shape.  Both
 * calls return VDF_ERR_BAD_ARG on a chain made by a from_checkpoints constructor.
 * Everything above the constructors works unchanged over the steps pushed so far: materialize, release, memory, advice, direction,
 * [set_]launch_rounds, vdf_nova_prove_step_custom_chain (a k not yet pushed is "step k is beyond the chain", and the proof object
 * goes on after the push), vdf_nova_prove_recursively_custom over a chain that has been pushed completely, VDF_CUSTOM_CHECK_STEPS,
 * lanes, both orientations, and tuning.custom_ahead, whose lookahead stops at the end of the chain and counts a skip: push step k +
 * 1 before step k is proved and it rides in step k's lookahead.  materialize over steps pushed as ADVICE uploads their host copies
 * into one allocation on the side queue where it would otherwise launch walks, with no walk and no comparison; wait = 0 means what
 * it means for walks (the next call that needs the trace synchronises), and the circuit and both provers see a device trace exactly
 * as over a walked step.  release also drops the host copy of a released step pushed as advice -- a long stream holds a bounded
 * number of traces, and such a step cannot be materialised again (VDF_ERR_BAD_ARG) -- while checkpoints (n_adv * 32 bytes per
 * interval) are kept; vdf_nova_custom_chain_host_bytes counts both.
 * CONCURRENCY: no lock, as for forward circuits.  A push or a release must not overlap a vdf_nova_prove_step_custom_chain (or any
 * other call) over the same chain; both are safe between two steps.
 *
 * vdf_nova_eval_and_prove_custom: vdf_nova_eval_and_prove for a custom chain.  One library thread per lane evaluates the chain step
 * by step with the host restatement of forward_tape (vdf_nova_forward_tape_eval; lane l's rounds see VDF_TAPE_J = j_base[l] + the
 * rounds behind them) and hands finished steps over through a queue of at most 4: whole traces (every = 0, push_advice) or the
 * entries every `every` rounds (push_checkpoints), which the chain rebuilds on the device by walk_tape (descending), or, walk_tape =
 * NULL, by forward_tape itself (ascending).  The CALLING thread pushes everything that is ready, materialises it with wait = 0,
 * proves step k, releases it, and finalises the proof as the built-in call does; `synthesize` is called on the calling thread only
 * (a circuit written in another language is never entered from a library thread).  However the call ends -- a refused push, a step
 * that fails, a `synthesize` that returns an error -- the evaluators are told to stop and are joined before it returns.
 * initial: lanes * n_adv elements; final_entries (optional): the lanes' last entries; stats as for vdf_nova_eval_and_prove: eval_ms
 * to the last lane's last round, after_eval_ms from there to the return.  pp: parameters of the custom circuit `primary`, whose
 * repeat has t rounds and `lanes` lanes and reads vdf_cs_step_advice.  The proof is byte for byte the one
 * vdf_nova_prove_step_custom makes from the same traces. */
typedef struct vdf_custom_chain vdf_custom_chain;
enum { VDF_CHAIN_DESCENDING = 0, VDF_CHAIN_ASCENDING = 1 };
#define VDF_CUSTOM_CHECK_STEPS 1u
int  vdf_nova_custom_chain_from_checkpoints(int field, const vdf_round_tape* walk_tape, const vdf_fe* inv, uint64_t t, uint64_t every,
                                            size_t num_steps, const vdf_fe* checkpoints, uint64_t j_base, vdf_custom_chain** out);
int  vdf_nova_custom_chain_lanes_from_checkpoints(int field, const vdf_round_tape* walk_tape, const vdf_fe* inv, uint64_t t, uint64_t every,
                                                  size_t num_steps, size_t lanes, const vdf_fe* checkpoints, size_t lane_stride,
                                                  const uint64_t* j_base, vdf_custom_chain** out);
int  vdf_nova_custom_chain_from_checkpoints_forward(int field, const vdf_round_tape* forward_tape, const vdf_fe* inv, uint64_t t,
                                                    uint64_t every, size_t num_steps, const vdf_fe* checkpoints, uint64_t j_base,
                                                    vdf_custom_chain** out);
int  vdf_nova_custom_chain_lanes_from_checkpoints_forward(int field, const vdf_round_tape* forward_tape, const vdf_fe* inv, uint64_t t,
                                                          uint64_t every, size_t num_steps, size_t lanes, const vdf_fe* checkpoints,
                                                          size_t lane_stride, const uint64_t* j_base, vdf_custom_chain** out);
int  vdf_nova_custom_chain_begin(int field, const vdf_round_tape* tape, int direction, const vdf_fe* inv, uint64_t t, size_t lanes,
                                 const vdf_fe* initial, const uint64_t* j_base, vdf_custom_chain** out);
int  vdf_nova_custom_chain_push_checkpoints(vdf_custom_chain* chain, uint64_t every, const vdf_fe* checkpoints, size_t lane_stride);
int  vdf_nova_custom_chain_push_advice(vdf_custom_chain* chain, const vdf_fe* advice, size_t lane_stride);
/* VDF_CHAIN_DESCENDING or VDF_CHAIN_ASCENDING; -1 for NULL */
int  vdf_nova_custom_chain_direction(const vdf_custom_chain* chain);
/* the launch_rounds a job of this chain runs with when the caller asks for `launch_rounds`: 0 is first replaced by the chain's own
 * default (_set_launch_rounds; 0 until set); then the value itself for a descending chain (0 stays 0: walk_slice's 1,024), the
 * bound of an ascending chain for 0 or anything above it */
int  vdf_nova_custom_chain_launch_rounds(const vdf_custom_chain* chain, uint64_t launch_rounds, uint64_t* out);
/* the rounds per launch of the jobs whose caller asks for 0 -- vdf_nova_prove_recursively_custom always does: how a caller of the
 * prover cuts the walks of its windows finer than 1,024 rounds (0: back to the default).  Either direction. */
int  vdf_nova_custom_chain_set_launch_rounds(vdf_custom_chain* chain, uint64_t launch_rounds);
int  vdf_nova_custom_chain_materialize(vdf_ctx* ctx, vdf_custom_chain* chain, size_t first, size_t count, int wait, uint64_t launch_rounds,
                                       int* bad);
int  vdf_nova_custom_chain_release(vdf_custom_chain* chain, size_t first, size_t count);
int  vdf_nova_custom_chain_memory(const vdf_custom_chain* chain, size_t* resident_steps, uint64_t* device_bytes);
int  vdf_nova_custom_chain_host_bytes(const vdf_custom_chain* chain, uint64_t* bytes);
size_t vdf_nova_custom_chain_len(const vdf_custom_chain* chain);
int  vdf_nova_custom_chain_advice(vdf_custom_chain* chain, size_t k, const vdf_fe** d_advice);
void vdf_nova_custom_chain_free(vdf_custom_chain* chain);
/* Host only, pure: the slice of the walks that follows `done` rounds of `every`: *rounds = min(every - done, launch_rounds, budget)
 * (launch_rounds = 0: 1,024; budget = 0: no limit), *top = every - done, *last = 1 when the slice finishes the walks.  What
 * materialize and the pumps cut their launches by.  VDF_ERR_BAD_ARG: every = 0, done >= every, a null pointer. */
int  vdf_nova_custom_chain_slice(uint64_t every, uint64_t launch_rounds, uint64_t done, uint64_t budget, uint64_t* rounds, uint64_t* top,
                                 int* last);
const vdf_fe* vdf_cs_step_advice(const vdf_cs* cs);
int  vdf_nova_prove_step_custom_chain(vdf_pp* pp, vdf_proof** proof, const vdf_step_circuit* primary, vdf_custom_chain* chain, size_t k,
                                      const vdf_fe* z0);
int  vdf_nova_prove_recursively_custom(vdf_pp* pp, const vdf_step_circuit* primary, vdf_custom_chain* chain, const vdf_fe* z0,
                                       size_t window_steps, uint32_t flags, vdf_proof** proof);
typedef struct vdf_nova_custom_stream {
  const vdf_round_tape* forward_tape;  /* evaluates the chain; required */
  const vdf_fe* inv;                   /* lanes * forward_tape->n_inv */
  const vdf_round_tape* walk_tape;     /* NULL: steps handed over as checkpoints are rebuilt by forward_tape (ascending) */
  const vdf_fe* walk_inv;              /* lanes * walk_tape->n_inv */
  uint64_t t, every;                   /* every = 0: whole traces are handed over (push_advice); else it divides t (push_checkpoints) */
  size_t lanes; const uint64_t* j_base;
} vdf_nova_custom_stream;
int  vdf_nova_eval_and_prove_custom(vdf_pp* pp, const vdf_step_circuit* primary, const vdf_nova_custom_stream* s, const vdf_fe* initial,
                                    size_t num_steps, const vdf_fe* z0, vdf_fe* final_entries /* lanes * n_adv, optional */,
                                    vdf_proof** out, vdf_nova_stream_stats* stats /* optional */);
/* Which constraint of the LAST step is unsatisfied: *count = the rows r of the fresh primary instance with (A z)[r] (B z)[r] !=
 * (C z)[r], *first_row = the smallest (UINT64_MAX: none); vdf_hip.h vdf_unsat_rows.  For proofs of every circuit kind.  The step's
 * own A z, B z, C z do not outlive it on every path (the base step folds nothing and never makes them apart from the running
 * instance's; the next step's early rows -- a built-in kind's, or a custom chain's under tuning.custom_ahead = 2 -- overwrite
 * theirs on the way out of the step; a verifier uses the vectors as
 * scratch), so they are made again from the fresh z, which stays in its ring slot until the next step: one sparse product into
 * three vectors the first request allocates.  VDF_ERR_BAD_ARG before this object's first prove_step (a deserialised proof too). */
int  vdf_nova_proof_last_unsat(const vdf_proof* proof, uint64_t* count, uint64_t* first_row);
/* Of the steps after the first that this proof object proved: in how many a lookahead of a custom chain (tuning.custom_ahead) was
 * used (*hits), discarded (*misses), or not attempted (*skipped).  All three are 0 for every other kind of proof, for
 * custom_ahead = 0 and for steps of plain vdf_nova_prove_step_custom.  Outputs may be NULL. */
int  vdf_nova_proof_ahead_stats(const vdf_proof* proof, uint64_t* hits, uint64_t* misses, uint64_t* skipped);
/* The rows of a custom circuit's vdf_cs_repeat: repetition j, constraint c is row *row_begin + j * *n_cons + c, j < *t.  Returns 1,
 * or 0 for parameters without a repeat (outputs 0); does not depend on the rows being periodic. */
int  vdf_nova_pp_repeat_rows(const vdf_pp* pp, uint64_t* row_begin, uint64_t* n_cons, uint64_t* t);
/* ... and the lanes of the repeat (vdf_cs_repeat_lanes; 1 for vdf_cs_repeat): lane l, repetition j, constraint c is row *row_begin +
 * (l * *t + j) * *n_cons + c.  Returns 1, or 0 for parameters without a repeat (*lanes = 0). */
int  vdf_nova_pp_repeat_lanes(const vdf_pp* pp, uint64_t* lanes);

/* ---- host-only entry points (no device): what the CPU tests pin against oracle/nova.py ------------------------- */
/* the random oracle: lane 1 of the sponge after absorbing xs under `tag` (a full field element, Montgomery in and out) */
int  vdf_nova_ro_hash(int field, uint64_t tag, const vdf_fe* xs, size_t n, vdf_fe* out);
/* the default block's VDF_RO_CONSTANTS (88) round constants of `field` in Montgomery form, in the order vdf_ro_hash_batch
 * (vdf_hip.h) reads them: ext[r][lane] for r = 0..7, lane-minor, then in[0..55].  Pure: callable without a GPU. */
int  vdf_nova_ro_constants(int field, vdf_fe out[VDF_RO_CONSTANTS]);
/* the host restatement of vdf_ro_hash_batch, and the reference its tests compare with byte for byte: out[i] =
 * vdf_nova_ro_hash(field, tag, xs + i * len, len) for bits = 0, the low `bits` bits of its canonical integer as a plain
 * little-endian integer for bits in 1..255.  The same refusals: an unknown field, any other `bits`, len > VDF_RO_HASH_MAX_LEN,
 * a null pointer with n > 0 (xs may be null when len = 0): VDF_ERR_BAD_ARG.  n = 0 is VDF_OK and touches nothing. */
int  vdf_nova_ro_hash_batch_eval(int field, uint64_t tag, const vdf_fe* xs, size_t len, size_t n, int bits, vdf_fe* out);
/* digest of the parameters public_params would make (both shapes synthesised on the host), and the sizes per side:
 * sizes[side] = {num_cons, num_vars, nnz(A) + nnz(B) + nnz(C)} */
int  vdf_nova_shape_digest(uint64_t num_iters_per_step, int circuit_kind, int gens_family, uint8_t out[32], uint64_t sizes[2][3]);
/* the same shape as COO triples per matrix (A, B, C), in the order the constraints were made, values in Montgomery form of the
 * side's scalar field: call once with rows = cols = vals = NULL for nnz[3], then with arrays of those lengths. */
int  vdf_nova_shape_export(uint64_t num_iters_per_step, int circuit_kind, int side, uint64_t nnz[3], uint32_t* const rows[3],
                           uint32_t* const cols[3], vdf_fe* const vals[3]);
int  vdf_nova_shape_digest_custom(const vdf_step_circuit* primary, int gens_family, uint8_t out[32], uint64_t sizes[2][3]);
/* vdf_nova_shape_export for a custom primary circuit synthesised over `field` (side 1: the secondary shape of that orientation) */
int  vdf_nova_shape_export_custom(int field, const vdf_step_circuit* primary, int side, uint64_t nnz[3], uint32_t* const rows[3],
                                  uint32_t* const cols[3], vdf_fe* const vals[3]);
/* ---- periodic rows (vdf_hip.h vdf_periodic_rows), host only ---------------------------------------------------------------
 * Detection over COO triples: are the rows row_begin + j * n_cons + c (j < t, c < n_cons; the variables of repetition j at
 * seg_begin + j * n_vars) periodic from some lead j0 in 0 .. 4 on?  The pattern is taken from repetition j0, the slopes of the
 * affine coefficients from j0 + 1, and then EVERY triple of EVERY repetition j0 .. t - 1 in all three matrices is compared with
 * it: the same set of terms, SEG coefficients equal, ABS coefficients equal to c0 + (j - j0) c1 in the field.  Returns 1 and the
 * description (row_start / terms / consts: caller's arrays of the caps, which *out then points into; *lead = j0; the rows covered
 * are [*first_row, *first_row + *row_count)), or 0 for none -- a mismatch anywhere, fewer than two periodic repetitions, a row of
 * more than VDF_PERIODIC_MAX_ROW_TERMS terms, a cap exceeded: not an error, such rows keep the generic kernel -- or a NEGATIVE
 * error code.  lead, first_row, row_count may be NULL. */
int  vdf_nova_periodic_rows_detect(int field, const uint64_t nnz[3], const uint32_t* const rows[3], const uint32_t* const cols[3],
                                   const vdf_fe* const vals[3], size_t seg_begin, size_t n_vars, size_t row_begin, size_t n_cons, uint64_t t,
                                   uint16_t row_start[VDF_PERIODIC_MAX_STARTS], vdf_periodic_term terms[VDF_PERIODIC_MAX_TERMS],
                                   vdf_fe consts[VDF_PERIODIC_MAX_CONSTS], vdf_periodic_rows* out, uint64_t* lead, uint64_t* first_row,
                                   uint64_t* row_count);
/* vdf_nifs_cross_term_periodic restated on the host: the same arguments, the same refusals, every pointer host memory -- the
 * reference of the device path, byte for byte. */
int  vdf_nova_periodic_rows_eval(int field, const vdf_periodic_rows* rows, uint64_t j_first, uint64_t reps, size_t seg_begin,
                                 size_t row_begin, size_t num_cols, size_t num_cons, const vdf_fe* z2, const vdf_fe* Az1, const vdf_fe* Bz1,
                                 const vdf_fe* Cz1, const vdf_fe* u1, vdf_fe* Az2, vdf_fe* Bz2, vdf_fe* Cz2, vdf_fe* T);
/* The detection public_params_custom would make, without a device: the primary shape of `primary` over `field` and its
 * vdf_cs_repeat; returns as vdf_nova_periodic_rows_detect (0 also for a circuit without a repeat).  *seg_begin = the first variable
 * of repetition 0, *num_cons / *num_cols = the primary shape's (num_cols = variables + 1 + public IO), filled either way. */
int  vdf_nova_shape_periodic_custom(int field, const vdf_step_circuit* primary, uint16_t row_start[VDF_PERIODIC_MAX_STARTS],
                                    vdf_periodic_term terms[VDF_PERIODIC_MAX_TERMS], vdf_fe consts[VDF_PERIODIC_MAX_CONSTS],
                                    vdf_periodic_rows* out, uint64_t* seg_begin, uint64_t* lead, uint64_t* first_row, uint64_t* row_count,
                                    uint64_t* num_cons, uint64_t* num_cols);
/* The early rows public_params_custom would find under tuning.custom_ahead = 2, without a device: the longest run of primary
 * constraints that read nothing of a witness but the variables of the circuit's vdf_cs_repeat, the constant and the `arity`
 * variables of z_in where the augmented circuit allocates them, none of more than 8 entries in any matrix; *rows = 0 (and
 * *row_begin = 0) when the run is shorter than 64 rows or the circuit has no repeat.  *zin_begin = the column of z_in[0],
 * *seg_begin = the first variable of repetition 0 (0 without a repeat).  Outputs may be NULL. */
int  vdf_nova_shape_early_rows_custom(int field, const vdf_step_circuit* primary, uint64_t* row_begin, uint64_t* rows,
                                      uint64_t* zin_begin, uint64_t* seg_begin);
/* One augmented circuit synthesised on the host with every variable computed there (small t only).  The inputs that
 * belong to the folded side (U_u, U_X, u_X) are in Montgomery form of THAT side's scalar field, everything else in the
 * circuit's own field.  result / input: the MinRoot step's states (side 0; ignored for side 1).  arity = 3 / 1. */
typedef struct {
  vdf_fe params, i, z0[3], zi[3];
  vdf_affine U_comm_W, U_comm_E; vdf_fe U_u, U_X[2];
  vdf_affine u_comm_W; vdf_fe u_X[2];
  vdf_affine T;
} vdf_nova_aug_inputs;
int  vdf_nova_aug_synthesize(int side, uint64_t num_iters_per_step, int circuit_kind, const vdf_nova_aug_inputs* in,
                             const vdf_state* result, const vdf_state* input, vdf_fe* W, size_t w_cap, size_t* num_vars,
                             size_t* num_cons, vdf_fe X[2], vdf_fe z_next[3]);
/* the host-only entry points under another random-oracle block (NULL = the default): sponge, shape digest, synthesis */
int  vdf_nova_ro_hash_ro(const vdf_nova_ro_params* ro, int field, uint64_t tag, const vdf_fe* xs, size_t n, vdf_fe* out);
/* a family-1 block's constants of `field` in Montgomery form, in the layout vdf_ro_hash_batch_block (vdf_hip.h) reads: rc, the
 * (full_rounds + partial_rounds) * width round constants, round-major and lane-minor; mds, the width * width matrix, row-major.
 * counts (optional) receives {(full_rounds + partial_rounds) * width, width * width}; with rc = mds = NULL only the counts are
 * written (either pointer alone may be NULL too).  ro = NULL, the default block (family 0 has vdf_nova_ro_constants), a block
 * this build does not support or an unknown field: VDF_ERR_BAD_ARG.  Pure: callable without a GPU. */
int  vdf_nova_ro_block_constants(const vdf_nova_ro_params* ro, int field, vdf_fe* rc, vdf_fe* mds, size_t counts[2]);
/* the host restatement of vdf_ro_hash_batch_block, and the reference its tests compare with byte for byte: out[i] =
 * vdf_nova_ro_hash_ro(ro, field, tag, xs + i * len, len) under the `bits` rule of vdf_nova_ro_hash_batch_eval.  ro = NULL
 * behaves as vdf_nova_ro_hash_batch_eval.  Refusals as the device call's, in its order, each VDF_ERR_BAD_ARG: an unknown field;
 * a block this build does not support (a width, full_rounds or partial_rounds out of range among them); bits outside 0..255;
 * len > VDF_RO_HASH_MAX_LEN; then n = 0 is VDF_OK and touches nothing; a null out, or a null xs with len > 0. */
int  vdf_nova_ro_hash_batch_eval_ro(const vdf_nova_ro_params* ro, int field, uint64_t tag, const vdf_fe* xs, size_t len, size_t n,
                                    int bits, vdf_fe* out);
int  vdf_nova_shape_digest_ro(const vdf_nova_ro_params* ro, uint64_t num_iters_per_step, int circuit_kind, int gens_family, uint8_t out[32],
                              uint64_t sizes[2][3]);
int  vdf_nova_aug_synthesize_ro(const vdf_nova_ro_params* ro, int side, uint64_t num_iters_per_step, int circuit_kind,
                                const vdf_nova_aug_inputs* in, const vdf_state* result, const vdf_state* input, vdf_fe* W, size_t w_cap,
                                size_t* num_vars, size_t* num_cons, vdf_fe X[2], vdf_fe z_next[3]);

/* the host-only entry points for the forward circuit in lanes (lanes = 1: the forward circuit itself).  shape_stencil_lanes
 * returns 6 (5 for one lane) when the L (3t + 1) early rows are one run and match the stencil.  aug_synthesize_lanes is the
 * PRIMARY circuit only: z0 / zi of `in` are ignored and read from the arrays z0 / zi (3 lanes elements each); results / inputs:
 * one state per lane; z_next: 3 lanes elements. */
int  vdf_nova_shape_digest_lanes(const vdf_nova_ro_params* ro, uint64_t num_iters_per_step, size_t lanes, int gens_family, uint8_t out[32],
                                 uint64_t sizes[2][3]);
int  vdf_nova_shape_stencil_lanes(uint64_t t, size_t lanes, uint64_t* early_begin, uint64_t* early_len, uint64_t* seg_begin);
int  vdf_nova_shape_export_lanes(uint64_t num_iters_per_step, size_t lanes, int side, uint64_t nnz[3], uint32_t* const rows[3],
                                 uint32_t* const cols[3], vdf_fe* const vals[3]);
int  vdf_nova_aug_synthesize_lanes(const vdf_nova_ro_params* ro, uint64_t num_iters_per_step, size_t lanes, const vdf_nova_aug_inputs* in,
                                   const vdf_fe* z0, const vdf_fe* zi, const vdf_state* results, const vdf_state* inputs, vdf_fe* W,
                                   size_t w_cap, size_t* num_vars, size_t* num_cons, vdf_fe X[2], vdf_fe* z_next);

/* The host-only entry points in the orientation `field` (the primary circuit's field), one general form each: circuit_kind is
 * any built-in kind, lanes is meaningful for VDF_CIRCUIT_MINROOT_FORWARD_LANES (1 = the forward circuit) and must be 1 otherwise;
 * ro: NULL = the default block.  aug_synthesize_field: side 1 ignores the step's arguments; on side 0, z0 / zi (3 lanes elements)
 * replace those of `in` when given (required for more than one lane), results / inputs hold one state per lane and z_next gets
 * 3 lanes elements. */
int  vdf_nova_shape_digest_field(int field, const vdf_nova_ro_params* ro, uint64_t num_iters_per_step, int circuit_kind, size_t lanes,
                                 int gens_family, uint8_t out[32], uint64_t sizes[2][3]);
int  vdf_nova_shape_export_field(int field, uint64_t num_iters_per_step, int circuit_kind, size_t lanes, int side, uint64_t nnz[3],
                                 uint32_t* const rows[3], uint32_t* const cols[3], vdf_fe* const vals[3]);
int  vdf_nova_shape_stencil_field(int field, uint64_t t, int circuit_kind, size_t lanes, uint64_t* early_begin, uint64_t* early_len,
                                  uint64_t* seg_begin);
int  vdf_nova_aug_synthesize_field(int field, const vdf_nova_ro_params* ro, int side, uint64_t num_iters_per_step, int circuit_kind,
                                   size_t lanes, const vdf_nova_aug_inputs* in, const vdf_fe* z0, const vdf_fe* zi, const vdf_state* results,
                                   const vdf_state* inputs, vdf_fe* W, size_t w_cap, size_t* num_vars, size_t* num_cons, vdf_fe X[2],
                                   vdf_fe* z_next);

/* of the calling thread's last augmented-circuit synthesis: how many slope inverses the native pre-pass queued (batched
 * inversion) and how many of them were wrong or unused (0 for well-formed inputs: the queue is only an accelerator) */
int  vdf_nova_synthesis_stats(uint64_t* queued, uint64_t* misses);

/* ---- compression (src/nova/proof.rs:360-368, :383) ---------------------------------------------------------
 * NovaVDFProof::compress -> nova-snark CompressedSNARK::prove: the last secondary instance is folded into the running
 * one, then one succinct argument PER SIDE (SS1 / SS2 of :32-33) that the running primary instance and the folded
 * secondary instance are satisfiable, instead of their witnesses.  Protocol "vdf-spartan-v3" (oracle/spartan.py): a
 * Spartan-style sum-check argument with inner-product-argument openings under the side's own Pedersen generators; the
 * extra generator of the openings is generator number num_gens of the same family.  Self-consistent, bit-exact against
 * the oracle, not interchangeable with nova-snark (unpinned).  Every pass over a vector runs on the GPU. */
int  vdf_nova_compress(const vdf_proof* proof, vdf_pp* pp, vdf_snark** out);
/* vdf_nova_compress for many proofs under one parameter set: out[q] serialises to exactly what
 * vdf_nova_compress(proofs[q], pp) gives, and is freed on its own with vdf_nova_snark_free.  Groups of up to 8 distinct
 * proofs (fewer when the free device memory does not hold their scratch) move through both sides' arguments in lockstep:
 * every sum-check round is one reduction and one fold for the whole group, the M-vectors one transposed product, and the
 * rounds of the openings are spread over the set's compression queues, one proof's MSM sort and host turn under another's
 * bucket accumulation.  Each proof keeps its own transcript.  A proof named more than once is compressed once; every slot
 * that names it gets its own copy.  The proofs are left as vdf_nova_compress leaves them.  A null pp or out: VDF_ERR_BAD_ARG;
 * a null proof, one made under other parameters (VDF_ERR_BAD_ARG) or one with no steps (VDF_ERR_BAD_LENGTH) fails the whole
 * call before any device work, every out[q] NULL and vdf_nova_last_error naming the entry; count = 0 does nothing. */
int  vdf_nova_compress_batch(vdf_pp* pp, size_t count, const vdf_proof* const proofs[], vdf_snark* out[]);
/* NovaVDFProof::verify for the Compressed variant (:383): *ok = 1 iff the two output hashes match the carried
 * instances for num_steps steps from z0, both arguments verify (the secondary one for the instance the verifier
 * folds itself), the carried zi_primary equals zi and zi_secondary == [0]. */
int  vdf_nova_verify_compressed(const vdf_snark* snark, vdf_pp* pp, size_t num_steps, const vdf_fe z0[3], const vdf_fe zi[3],
                                int* ok);
/* Many compressed proofs under one parameter set: ok[q] = what vdf_nova_verify_compressed returns for entry q (up to a
 * soundness error of about 2^-128), *all_ok = 1 iff every entry verifies; z0, zi: count x arity elements.  Each proof's
 * exact checks and transcript replay run on their own; the group checks of all its inner-product openings are combined,
 * with independent 128-bit weights drawn from a transcript of the whole batch, into one MSM over each side's generators
 * and one over the small points.  When a combined check fails, every remaining entry is verified on its own.  A null
 * proof or one made under other parameters fails the call with VDF_ERR_BAD_ARG (vdf_nova_last_error names the entry);
 * count = 0 gives *all_ok = 1. */
int  vdf_nova_verify_compressed_batch(vdf_pp* pp, size_t count, const vdf_snark* const snarks[], const size_t num_steps[],
                                      const vdf_fe* z0, const vdf_fe* zi, int ok[], int* all_ok);
/* How vdf_nova_verify_compressed_batch evaluates the shape's polynomial at every proof's point, M(r_x, r_y) -- the one value a
 * replay needs the device for.  The transcript does not absorb it, so the batch replays every proof on the host without a
 * device wait and evaluates all of a side's points afterwards by passes over the shape's rows (vdf_hip.h
 * vdf_sparse_eval_multi); an entry whose comparison fails leaves the batch before the combined group check.  Verdicts, *all_ok
 * and error codes do not depend on the setting, and no proof's bytes do.  A switch of the parameter set, not of vdf_nova_tuning:
 *   n = 0      every replay evaluates its own point, as vdf_nova_verify_compressed does (eq table, transposed product, dot, a wait);
 *   n = 1..64  at most n points per pass.  A point holds 32 (M + Z) bytes of tables meanwhile (M, Z: the padded numbers of
 *              constraints and of columns; 24 MB on the primary side at t = 2^16); a pass takes fewer points when the free
 *              device memory less 2 GiB does not hold n of them.  The tables live in the side's scratch block, which the set keeps
 *              at its largest size until it is freed.  A verifier short of memory lowers n.
 * Anything else is VDF_ERR_BAD_ARG.  The initial value is the environment variable VDF_NOVA_VERIFY_MULTI (0..64) when it is
 * set, else 16 (measured: DESIGN.md 4.4, profiles/r21_verify_multi.txt; tools/gpu_verify_multi_time.py).
 * vdf_nova_pp_verify_multi reads the value back (0 for a null pp).  vdf_nova_pp_verify_multi_stats: out[0] = passes launched,
 * out[1] = points evaluated, out[2] = points whose comparison failed, since the set was made. */
int  vdf_nova_pp_set_verify_multi(vdf_pp* pp, int n);
int  vdf_nova_pp_verify_multi(const vdf_pp* pp);
int  vdf_nova_pp_verify_multi_stats(const vdf_pp* pp, uint64_t out[3]);
/* Many running proofs under one parameter set: ok[q] = what vdf_nova_verify_custom returns for entry q (up to a soundness
 * error of about 2^-128), *all_ok = 1 iff every entry verifies; z0, zi: count x arity elements.  Each entry's exact checks
 * (step count, z0, output hashes, the last secondary instance's u and comm_E, zi, every instance's z tail) run on their own;
 * then per side all live entries' commitments are opened in one MSM over the generators (and one over the commitments), and
 * their R1CS residuals are summed in one pass over the shape and tested for zero.  The weights are 128 bits each from the
 * operating system, fresh for every call.  When a combined check fails, every live entry is verified on its own.  The proofs
 * are left as they were: a chain verified between two steps goes on to the same bytes.  A null pp, all_ok or array:
 * VDF_ERR_BAD_ARG; a null proof or one made under other parameters fails the call with VDF_ERR_BAD_ARG, a half-folded one
 * with VDF_ERR_DEVICE, before any device work and with vdf_nova_last_error naming the entry; count = 0 gives *all_ok = 1. */
int  vdf_nova_verify_batch(vdf_pp* pp, size_t count, const vdf_proof* const proofs[], const size_t num_steps[], const vdf_fe* z0,
                           const vdf_fe* zi, int ok[], int* all_ok);
void vdf_nova_snark_free(vdf_snark* snark);
/* Flat canonical encoding of the two arguments, primary then secondary (little-endian, non-Montgomery, 64-byte points;
 * layout in the implementation and in oracle/wire.py): size, export, and import -- which replaces the arguments of
 * `snark` and returns VDF_ERR_NONCANONICAL for an out-of-range field element or a point off its curve. */
size_t vdf_nova_snark_size(const vdf_snark* snark);
int  vdf_nova_snark_bytes(const vdf_snark* snark, uint8_t* out, size_t cap);
int  vdf_nova_snark_set_bytes(vdf_snark* snark, const uint8_t* in, size_t len);

/* ---- wire formats ---------------------------------------------------------------------
 * The reference keeps its proofs in memory only (src/nova/proof.rs:52-55 derives no serialisation); these encodings
 * are this library's own, versioned by their magic.  Field elements: 32 bytes, canonical, little-endian.  Points:
 * 32 bytes, canonical little-endian x with the parity of y in bit 255, the identity as 32 zero bytes.
 *
 *   relaxed instance = comm_W [32] | comm_E [32] | u [32] | X [2 x 32];   strict instance = comm_W [32] | X [2 x 32]
 *   "VDFSNK03" compressed proof = magic[8] | t u64 | digest of the public parameters [32]
 *        | running primary instance | running secondary instance | last secondary instance (strict)
 *        | cross-term commitment of the last fold [32] | z_i primary [96] | z_i secondary [32]
 *        | argument of the primary side | argument of the secondary side   (as vdf_nova_snark_bytes, 32-byte points)
 *   "VDFRSK02" running proof    = magic[8] | t u64 | steps u64 | digest [32] | z_0 [96] | z_i primary [96] | z_i secondary [32]
 *        | the same three instances | W1 | E1 | W2 | E2 | w2
 *
 * Both are constant-size in the number of steps.  Deserialisation fails with VDF_ERR_BAD_ARG for a foreign magic or
 * other public parameters, VDF_ERR_BAD_LENGTH for a length that does not fit the shapes, and VDF_ERR_NONCANONICAL for
 * an out-of-range field element or bytes that decode to no curve point.  The running proof is a checkpoint:
 * vdf_nova_proof_deserialize rebuilds the device-resident state (including A z, B z, C z of the running instances),
 * refuses witnesses that do not open their commitments, and vdf_nova_prove_step continues from it. */
/* The 32-byte point encoding by itself (host arithmetic only, no device); curve = VDF_CURVE_PALLAS / VDF_CURVE_VESTA,
 * coordinates in Montgomery form like everywhere in this ABI.  decompress: VDF_ERR_NONCANONICAL unless the bytes are
 * exactly what compress writes for some point. */
int  vdf_nova_point_compress(int curve, const vdf_affine* p, uint8_t out[32]);
int  vdf_nova_point_decompress(int curve, const uint8_t in[32], vdf_affine* out);
size_t vdf_nova_snark_serialized_size(const vdf_snark* snark);
int  vdf_nova_snark_serialize(const vdf_snark* snark, uint8_t* out, size_t cap);
int  vdf_nova_snark_deserialize(vdf_pp* pp, const uint8_t* in, size_t len, vdf_snark** out);
/* Many compressed proofs from their wire bytes under one parameter set, their points decoded on the device.  status[q] is exactly
 * the code vdf_nova_snark_deserialize(pp, in[q], len[q], ..) returns for that entry alone (a null in[q]: VDF_ERR_BAD_ARG);
 * out[q] is NULL unless status[q] == VDF_OK, and is then the object the single call makes (vdf_nova_snark_bytes and
 * vdf_nova_snark_serialize give the same bytes; the caller frees it with vdf_nova_snark_free).  The host walks every encoding
 * once -- magic, t, digest, length, the range of every field element -- and notes its point encodings; one
 * vdf_points_decompress (vdf_hip.h) per curve then decodes the points of all entries that passed, and one wait follows.  An entry
 * that failed a host check sends no point to the device, and no entry changes another's result.  The call returns VDF_OK when it
 * ran, whatever the entries' codes; VDF_ERR_BAD_ARG for a null pp or (count > 0) a null array; a device failure is the call's
 * own error and leaves every out[q] NULL.  count = 0 does nothing.  The single call decodes on the host, one square root per
 * point: use it for one proof where no device wait is wanted, this one for many. */
int  vdf_nova_snark_deserialize_batch(vdf_pp* pp, size_t count, const uint8_t* const in[], const size_t len[], vdf_snark* out[],
                                      int status[]);
/* A verifier that holds bytes only: vdf_nova_snark_deserialize_batch, then vdf_nova_verify_compressed_batch over the entries
 * that decoded.  An entry that does not decode has ok[q] = 0 and its code in status[q] (VDF_OK for every entry that decoded,
 * verified or not), and the others are verified as if it were absent: their verdicts are those of
 * vdf_nova_verify_compressed_batch over handles made by vdf_nova_snark_deserialize.  num_steps: count values; z0, zi: count x
 * arity elements, entry-major (those of an undecodable entry are not read).  *all_ok = 1 iff every entry decoded and verified;
 * count = 0 gives *all_ok = 1.  A null pp, all_ok or (count > 0) array: VDF_ERR_BAD_ARG. */
int  vdf_nova_verify_wire_batch(vdf_pp* pp, size_t count, const uint8_t* const in[], const size_t len[], const size_t num_steps[],
                                const vdf_fe* z0, const vdf_fe* zi, int ok[], int status[], int* all_ok);
/* ---- aggregation: many running proofs as ONE compressed proof ("vdf-aggregate-v1") ----------------------------------------
 * vdf_nova_compress_batch makes K proofs of 11 KB each and its verifiers pay K arguments; lanes put many chains into one proof,
 * but only up to 16 of equal length, fixed before the first step and proved by one prover.  Aggregation is for proofs made
 * independently -- other provers' step counts, other times, any circuit kind, either orientation -- under one parameter set:
 * Nova's folding scheme for two RELAXED instances folds the K running primary instances into one and the K folded secondary
 * instances into one, and one argument per side is made for the two accumulators.
 *
 *   per proof k   as vdf_nova_compress begins: R1_k = the running primary instance; F2_k = the running secondary instance
 *                 folded with the last secondary one (cross-term commitment T2_k, the Poseidon challenge the circuits
 *                 recompute).  Statement k = what "VDFSNK03" carries: r_U1, r_U2, l_u2, T2, z_i primary, z_i secondary.
 *   per side s    (0: the R1_k, 1: the F2_k) a transcript of oracle/spartan.py, label "aggregate": absorb("count", K u64 LE |
 *                 s u64 LE), then EVERY instance as the compression argument absorbs one (digest, comm_W, comm_E, u, X), in
 *                 order, before the first challenge: each challenge binds all K statements.  acc = instance 1; for k = 2..K
 *                 (index 1: acc, index 2: instance k)
 *                     TT_k = A z1 o B z2 + A z2 o B z1 - u1 C z2 - u2 C z1,   absorb_pt("T", commit(TT_k)),   r = challenge("r")
 *                     W <- W1 + r W2,   E <- E1 + r TT_k + r^2 E2,   u <- u1 + r u2,   X <- X1 + r X2
 *                     comm_W <- comm_W1 + r comm_W2,   comm_E <- comm_E1 + r commit(TT_k) + r^2 comm_E2       (r: 128 bits)
 *   arguments     one "vdf-spartan-v3" argument per side for acc, on its own transcript "compress" as always.  For K = 1
 *                 nothing is folded and the two arguments are byte for byte those of vdf_nova_compress.
 *   verifier      K >= 1 and every num_steps[k] >= 1; per k the two output hashes, z_i and z_i secondary == [0] exactly as
 *                 vdf_nova_verify_compressed checks them; its own secondary fold with T2_k; the transcripts and folds above
 *                 on instances only (host point arithmetic); then both arguments.
 * SOUNDNESS: knowledge soundness of Nova's folding of two relaxed instances, applied K - 1 times per side with 128-bit
 * Fiat-Shamir challenges: a valid aggregate attests all K statements.  Nothing about zero knowledge is claimed.  The verdict
 * is ONE bit for the whole aggregate (there is one argument); only the exact per-entry checks can name an entry.
 *
 *   "VDFAGG01" = magic[8] | t u64 | count u64 | digest [32] | count x statement (r_U1 | r_U2 | l_u2 | T2 | z_i primary |
 *        z_i secondary, as in "VDFSNK03") | (count - 1) x commit(TT) primary [32] | (count - 1) x commit(TT) secondary [32]
 *        | argument of the primary side | argument of the secondary side
 *
 * vdf_nova_compress_aggregate: count = 1 .. VDF_NOVA_AGGREGATE_MAX.  Entries are folded one at a time: the device scratch is
 * one accumulator per side and one incoming instance, whatever the count.  Each incoming instance costs one sparse product
 * (vdf_spmv3), one vdf_cross_term_relaxed, one commitment and one vdf_fold_relaxed per side; the accumulator's A z, B z, C z
 * are folded along.  The proofs are left as vdf_nova_compress leaves them and can go on proving; a proof named twice is
 * folded twice.  Refused before any device work, with *out = NULL and vdf_nova_last_error naming the entry: a null pp or out,
 * count 0 or above the cap, a null proof or one made under other parameters (VDF_ERR_BAD_ARG); a proof with no steps
 * (VDF_ERR_BAD_LENGTH).
 * vdf_nova_verify_aggregate: z0, zi: count x arity elements, entry-major.  *ok = 1 iff every check above holds.  *bad_entry
 * (may be NULL) = the first entry whose exact checks fail, -1 when they all pass: a failing argument gives *ok = 0,
 * *bad_entry = -1.  A count other than the aggregate's gives *ok = 0 and VDF_OK; other parameters: VDF_ERR_BAD_ARG.
 * vdf_nova_aggregate_deserialize: the codes of vdf_nova_snark_deserialize (VDF_ERR_BAD_ARG: foreign magic, another t or
 * digest; VDF_ERR_BAD_LENGTH: a length that does not fit count and the shapes; VDF_ERR_NONCANONICAL: an element out of range
 * or bytes that decode to no point). */
#define VDF_NOVA_AGGREGATE_MAX 1024
typedef struct vdf_aggregate vdf_aggregate;
int  vdf_nova_compress_aggregate(vdf_pp* pp, size_t count, const vdf_proof* const proofs[], vdf_aggregate** out);
int  vdf_nova_verify_aggregate(const vdf_aggregate* agg, vdf_pp* pp, size_t count, const size_t num_steps[], const vdf_fe* z0,
                               const vdf_fe* zi, int* ok, int64_t* bad_entry);
void vdf_nova_aggregate_free(vdf_aggregate* agg);
size_t vdf_nova_aggregate_count(const vdf_aggregate* agg);
size_t vdf_nova_aggregate_serialized_size(const vdf_aggregate* agg);
int  vdf_nova_aggregate_serialize(const vdf_aggregate* agg, uint8_t* out, size_t cap);
int  vdf_nova_aggregate_deserialize(vdf_pp* pp, const uint8_t* in, size_t len, vdf_aggregate** out);
/* Host only, no context: the verifier's transcript and folds of ONE side over plain arrays (vdf_nova_verify_aggregate runs the
 * same code on its decoded instances).  A relaxed instance as the wire encodes it: */
typedef struct vdf_wire_instance { uint8_t comm_W[32], comm_E[32], u[32], X[2][32]; } vdf_wire_instance;
/* field_of_primary: the orientation (VDF_FIELD_FQ: the parameters' default); side 0 / 1: instances over that field / the other
 * one, commitments on the curve whose scalars it is; digest: the parameters'.  inst: count instances, comm_TT: count - 1 points
 * (may be NULL for count = 1).  *acc = the folded instance; r_out (may be NULL): the count - 1 challenges, Montgomery form of
 * the side's field.  VDF_ERR_BAD_ARG: a null pointer, an unknown field or side, count outside 1 .. VDF_NOVA_AGGREGATE_MAX;
 * VDF_ERR_NONCANONICAL: an element out of range or bytes that decode to no point. */
int  vdf_nova_aggregate_fold_instances(int field_of_primary, int side, const uint8_t digest[32], size_t count,
                                       const vdf_wire_instance inst[], const uint8_t comm_TT[][32], vdf_wire_instance* acc,
                                       vdf_fe r_out[]);
/* ---- the aggregate's verifier with its per-entry group arithmetic on the device ---------------------------------------------
 * vdf_nova_verify_aggregate spends, per entry, eight point decodings (in vdf_nova_aggregate_deserialize) and eight scalar
 * multiplications on the host; the two arguments that are the point of aggregation do not grow with the count.  In
 * "vdf-aggregate-v1" every instance is absorbed before the first challenge and only commit(TT_k) after it, so no challenge
 * depends on a folded accumulator and a side's sequential folds are two sums,
 *     comm_W = W_1 + sum_{k>=2} r_k W_k        comm_E = E_1 + sum_{k>=2} (r_k^2 E_k + r_k commit(TT_k)),
 * one vdf_msm_batch over the 3 count - 1 uploaded points; the count secondary folds F2_k = r_U2_k + rho_k l_u2_k are one
 * vdf_points_axpy (vdf_hip.h) of 2 count entries.  Transcripts, challenges, the exact per-entry checks and the folds of u and X
 * stay on the host, and so do the Poseidon hashes unless vdf_nova_pp_set_verify_ro_device moves them (below).  The three calls below are held, byte for byte and code for code, to the host calls
 * above, which stay the statement; they run on the parameter set's context and leave its asynchronous flag and stream as they
 * found them, whatever they return.
 *
 * vdf_nova_aggregate_fold_instances_device: vdf_nova_aggregate_fold_instances with the orientation and the digest taken from
 *   pp; the points are decoded by one vdf_points_decompress and go to the sums as they lie.  *acc and r_out: the host call's
 *   bytes.  The same refusals with the same codes (a null pp: VDF_ERR_BAD_ARG).
 * vdf_nova_verify_aggregate_device: vdf_nova_verify_aggregate's contract -- the same checks in the same order, the same *ok,
 *   *bad_entry and return codes.
 * vdf_nova_verify_aggregate_wire: bytes in, verdict out (the aggregate's vdf_nova_verify_wire_batch).  Every point of "VDFAGG01"
 *   -- the statements', the commit(TT), the arguments' L and R -- is decoded by one vdf_points_decompress per curve, then the
 *   device verifier runs.  *decode_code = exactly what vdf_nova_aggregate_deserialize(pp, bytes, len, ..) returns for these
 *   bytes; unless it is VDF_OK nothing is verified and *ok = 0, *bad_entry = -1, and the call itself returns VDF_OK.  With
 *   *decode_code == VDF_OK the return code, *ok and *bad_entry are vdf_nova_verify_aggregate's for the decoded object.  A null
 *   pp, bytes, ok or decode_code: VDF_ERR_BAD_ARG.
 * vdf_nova_aggregate_verify_times: what the last of the two verifiers above spent on this thread, host wall time in ms:
 *   [0] the exact checks (three Poseidon hashes per entry), [1] the secondary folds, [2] both accumulators, [3] both arguments,
 *   [4] the decoding (the wire call only).  For tools/gpu_aggregate_verify.py.  [0] means "exact checks and hashes" whoever
 *   computed the hashes (see below).
 * vdf_nova_pp_set_verify_ro_device: where vdf_nova_verify_aggregate_device (and with it vdf_nova_verify_aggregate_wire) makes the
 *   three Poseidon hashes of every entry -- both state hashes and the fold challenge.  min_count = 0 (the default): on the host,
 *   one entry after the other.  min_count > 0: for an aggregate of at least min_count entries a host pass packs the messages,
 *   three vdf_ro_hash_batch launches (vdf_hip.h; bits = 250, 250, 128) and one wait follow, and the comparisons run on the host
 *   in entry order.  *ok and *bad_entry are the same for EVERY input: the first failing entry is named, whichever check it
 *   fails.  A negative value: VDF_ERR_BAD_ARG.  This switch is family 0 only: a parameter set made under another RO
 *   parameter block accepts it and keeps the host hashes (vdf_nova_pp_set_verify_ro_block_device below is that set's switch).  The set keeps one device copy of each field's 88 round
 *   constants, made on first use and freed with it.  vdf_nova_verify_aggregate, the maker and the batch verifiers do not read
 *   the switch.  vdf_nova_pp_verify_ro_device reads it back (0 for a null pp); vdf_nova_pp_verify_ro_stats: out[0] = hashes made
 *   on the device under this set, out[1] = launches.
 * vdf_nova_pp_set_verify_ro_block_device: the same choice for a parameter set made under ANOTHER RO parameter block (family 1),
 *   a separate switch that leaves the one above as it is.  It is read only for such a set; a default-block set accepts it and
 *   ignores it.  min_count = 0 (the default): the host hashes.  min_count > 0: for an aggregate of at least min_count entries
 *   the same host pass packs the messages and three vdf_ro_hash_batch_block launches (vdf_hip.h) and one wait make the hashes;
 *   *ok, *bad_entry and the decode code are the same for every input.  A negative value: VDF_ERR_BAD_ARG.  The set keeps one
 *   device copy of the block's round constants and matrix per field, made on first use and freed with it.
 *   vdf_nova_pp_verify_ro_block_device reads it back (0 for a null pp); vdf_nova_pp_verify_ro_stats counts these hashes and
 *   launches in the same two counters. */
int  vdf_nova_aggregate_fold_instances_device(vdf_pp* pp, int side, size_t count, const vdf_wire_instance inst[],
                                              const uint8_t comm_TT[][32], vdf_wire_instance* acc, vdf_fe r_out[]);
int  vdf_nova_verify_aggregate_device(const vdf_aggregate* agg, vdf_pp* pp, size_t count, const size_t num_steps[],
                                      const vdf_fe* z0, const vdf_fe* zi, int* ok, int64_t* bad_entry);
int  vdf_nova_verify_aggregate_wire(vdf_pp* pp, const uint8_t* bytes, size_t len, size_t count, const size_t num_steps[],
                                    const vdf_fe* z0, const vdf_fe* zi, int* ok, int64_t* bad_entry, int* decode_code);
int  vdf_nova_aggregate_verify_times(double ms[5]);
int  vdf_nova_pp_set_verify_ro_device(vdf_pp* pp, int min_count);
int  vdf_nova_pp_verify_ro_device(const vdf_pp* pp);
int  vdf_nova_pp_verify_ro_stats(const vdf_pp* pp, uint64_t out[2]);
int  vdf_nova_pp_set_verify_ro_block_device(vdf_pp* pp, int min_count);
int  vdf_nova_pp_verify_ro_block_device(const vdf_pp* pp);
size_t vdf_nova_proof_serialized_size(const vdf_proof* proof);
int  vdf_nova_proof_serialize(const vdf_proof* proof, uint8_t* out, size_t cap);
int  vdf_nova_proof_deserialize(vdf_pp* pp, const uint8_t* in, size_t len, vdf_proof** out);
const char* vdf_nova_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* VDF_NOVA_H */
