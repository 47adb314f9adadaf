/* vdf_hip.h -- C ABI of the MI355X-native Nova/MinRoot hot path (libvdf_hip.so).
 *
 * This is the drop-in boundary (seam B2).  Each entry point
 * names the reference interface it replaces.  The reference is Rust; the third-party
 * crates it calls through (pasta-msm 0.1.1, nova-snark 0.8.0, pasta_curves 0.4.0,
 * Cargo.toml:15-18) are where these operations live today, reached from
 * `RecursiveSNARK::prove_step` at /root/reference/src/nova/proof.rs:342-349.
 *
 * Conventions
 *   - All integers little-endian.  A field element is 4 x u64 limbs of x*2^256 mod m
 *     (Montgomery form), the in-memory form of pasta_curves with `repr-c`
 *     (Cargo.toml:17).  Inputs must be canonical (< m); the hot path does not check
 *     (like pasta-msm); vdf_bases_validate checks a generator table once (VDF_ERR_NONCANONICAL).
 *   - affine = {x, y}, identity = (0, 0).  jac = {x, y, z} Jacobian, identity z = 0.
 *     Jacobian outputs are not unique; parity is defined on the affine normalisation.
 *   - Every data pointer may be a HOST pointer or a DEVICE (hipMalloc / torch) pointer;
 *     the library classifies each one with hipPointerGetAttributes.  Host buffers are
 *     staged through device memory (PCIe-inclusive); device buffers are used in place.
 *   - Caller owns every buffer.  The library keeps no caller pointer past a call; only the
 *     opaque handles (vdf_ctx, vdf_bases, vdf_shape) own device memory.
 *   - Calls are blocking unless the context is in async mode AND every buffer of the call
 *     is device-resident; then work is enqueued on the context's HIP stream.
 *   - Re-entrant across threads on one context (per-context mutex); no global mutable state
 *     except the lazily created default context of the two `mult_pippenger_*` shims and, when switched on,
 *     their generator cache (vdf_shim_set_cache).
 *   - No C++ exception or abort crosses this boundary: int status + vdf_last_error().
 *   - There is NO CPU back-end: vdf_ctx_create fails with VDF_ERR_NO_DEVICE without a GPU.
 */
#ifndef VDF_HIP_H
#define VDF_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } vdf_fe;            /* pasta_curves Fp / Fq, repr-c */
typedef struct { vdf_fe x, y; } vdf_affine;          /* pallas::Affine / vesta::Affine */
typedef struct { vdf_fe x, y, z; } vdf_jac;          /* pallas::Point / vesta::Point */
typedef struct { vdf_fe x, y, i; } vdf_state;        /* src/minroot.rs:267-272: State<T> { x, y, i }, three Montgomery elements */

typedef struct vdf_ctx vdf_ctx;
typedef struct vdf_bases vdf_bases;
typedef struct vdf_shape vdf_shape;

enum {
  VDF_OK = 0,
  VDF_ERR_BAD_ARG = 1,
  VDF_ERR_BAD_LENGTH = 2,
  VDF_ERR_NONCANONICAL = 3,
  VDF_ERR_DEVICE = 4,
  VDF_ERR_OOM = 5,
  VDF_ERR_NO_DEVICE = 6
};

enum { VDF_CURVE_PALLAS = 0, VDF_CURVE_VESTA = 1 };   /* G1 / G2, src/nova/proof.rs:26-27 */
enum { VDF_FIELD_FP = 0, VDF_FIELD_FQ = 1 };          /* S2 = Fp, S1 = Fq, src/nova/proof.rs:29-30 */

/* ---- context ------------------------------------------------------------------------ */
/* One context drives one GPU.  device_ids/n_devices: n_devices must be 1 (one process per
 * GPU; multi-GPU jobs create one context per rank, or one per device in a single process, and
 * combine them with vdf_msm_sharded / vdf_msm_multi).  No reference counterpart (the
 * reference is CPU-only); this is the handle the FFI shim would keep in a OnceCell. */
int  vdf_ctx_create(const int* device_ids, int n_devices, vdf_ctx** out);
void vdf_ctx_destroy(vdf_ctx* ctx);
/* The budget of hardware queues.  The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (this
 * library asks for 16 when it makes the process's first HIP call and the variable is unset; the runtime's default is 4); with
 * more streams than queues, kernels of one stream wait behind another's (measured with 8: two provers and a compression -- 11
 * streams -- ran slower than one prover; with 16 they run at the two-prover rate).  A context made HERE takes
 * its stream from a per-device pool instead of opening one: a new stream while the device's streams known to this library
 * (vdf_ctx_create contexts + pooled ones) number less than the budget minus one (left to the host's own streams: torch's,
 * a caller's copies), otherwise it SHARES the least used pooled stream of its role -- VDF_QUEUE_SIDE contexts (work with a
 * step's slack: a prover's look-ahead, a compression's second and third queue) with each other before they share with a
 * VDF_QUEUE_CRITICAL one (a prover's early rows).  Sharing serialises the sharers' work and nothing else: results do not
 * change.  libvdf_nova.so makes all of its internal contexts this way, so a host may run any number of provers and
 * compressions in one process; contexts from vdf_ctx_create always own their stream (the host decides how many it opens). */
#define VDF_QUEUE_CRITICAL 1
#define VDF_QUEUE_SIDE 2
int  vdf_ctx_create_pooled(const int* device_ids, int n_devices, int role, vdf_ctx** out);
/* ... and a queue that works HAND IN HAND with `parent`'s (a prover's look-ahead and early rows beside its chain).  The
 * hardware takes queues onto its pipes in the order they were created, and which pipes a prover's three queues sit on is worth
 * 10-14 % of its rate (measured: 1,114-1,125 prove_step/s when they were created back to back, 979-1,034 with one or two
 * foreign streams opened in between; profiles/r05_single_chain_vs_padding.txt).  vdf_ctx_create therefore opens two more
 * streams right behind the context's own and keeps them; this call hands them out (VDF_QUEUE_SIDE the first, VDF_QUEUE_CRITICAL
 * the second), whatever the host has opened since.  When they are taken (a second prover on the same context), or `parent`
 * runs on a foreign stream (vdf_ctx_set_stream), the context comes from the pool as above.  The streams live as long as any
 * context that uses them. */
int  vdf_ctx_create_pooled_near(vdf_ctx* parent, int role, vdf_ctx** out);
/* *pooled = 1 for a pooled context, *sharers = contexts on its stream (1 = its own), *device_streams = streams this library
 * holds on the context's device.  Any output may be NULL. */
int  vdf_ctx_queue_info(vdf_ctx* ctx, int* pooled, int* sharers, int* device_streams);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the context's own; NULL = back to the context's own
 * (whose neighbours vdf_ctx_create_pooled_near hands out: a prover on a foreign stream takes its queues from the pool). */
int  vdf_ctx_set_stream(vdf_ctx* ctx, void* hip_stream);
void* vdf_ctx_get_stream(vdf_ctx* ctx);
/* async != 0: calls whose buffers are all device-resident return after enqueueing. */
int  vdf_ctx_set_async(vdf_ctx* ctx, int async);
int  vdf_ctx_get_async(vdf_ctx* ctx, int* async);
int  vdf_ctx_sync(vdf_ctx* ctx);
int  vdf_ctx_device(vdf_ctx* ctx);                      /* the HIP device ordinal this context drives */
const char* vdf_last_error(vdf_ctx* ctx);              /* ctx may be NULL: last create error */

/* ---- commitment generators (Pedersen bases) ------------------------------------------ */
/* Replaces nova-snark's CommitGens (built in PublicParams::setup, src/nova/proof.rs:236):
 * the generator table lives in HBM for the life of the public parameters. */
int  vdf_bases_upload(vdf_ctx* ctx, int curve, const vdf_affine* bases, size_t n, vdf_bases** out);
/* Setup-time check of a generator table (upload itself does not look at the points, like pasta-msm): every
 * coordinate a canonical residue (else VDF_ERR_NONCANONICAL) and every point the identity (0, 0) or on
 * y^2 = x^3 + 5 (else VDF_ERR_BAD_ARG); *first_bad (optional) = smallest offending index. */
int  vdf_bases_validate(vdf_ctx* ctx, const vdf_bases* bases, size_t* first_bad);
/* Synthetic generators P_i = [k_i]G, G = (-1, 2), k_i = splitmix64-derived 64-bit (see
 * oracle/pasta.py base_dlog); stands in for nova-snark's label -> hash-to-curve derivation,
 * which is implementation-defined and unpinned. */
int  vdf_bases_generate(vdf_ctx* ctx, int curve, uint64_t seed, size_t n, vdf_bases** out);
/* Same, for the index range [start, start + n): the shard a rank owns in a multi-GPU MSM. */
int  vdf_bases_generate_range(vdf_ctx* ctx, int curve, uint64_t seed, size_t start, size_t n, vdf_bases** out);
/* Generator families.  KNOWN_DLOG is the one above (it makes full-size results checkable in O(n) through
 * sum s_i P_i = [sum s_i k_i] G).  TRY_AND_INCREMENT has no known discrete logarithms, like generators derived
 * from a hash: per index a xoshiro256** stream seeded by splitmix64(seed, index) yields candidates
 * x = 256 bits mod p; the first x with x^3 + 5 a square is taken, y = the even root (SURVEY.md 8d, config 2;
 * restated in oracle/pasta.py tai_base).  Setup-time only. */
enum { VDF_GENS_KNOWN_DLOG = 0, VDF_GENS_TRY_AND_INCREMENT = 1, VDF_GENS_LABEL_SHAKE = 2 /* vdf_bases_generate_label; a family id for the proof layer */ };
int  vdf_bases_generate_family(vdf_ctx* ctx, int curve, int family, uint64_t seed, size_t start, size_t n, vdf_bases** out);
/* Generators derived from a LABEL, as nova-snark derives its CommitGens (label -> SHAKE256 -> curve points;
 * PublicParams::setup, src/nova/proof.rs:236).  nova-snark's own encoding is not in /root/reference, so
 * this one is the build's own (restated in oracle/pasta.py label_base): for index i and counter c = 0, 1, ... one SHAKE256
 * block "vdf-gens-v1" | curve u8 | len u8 | label | i LE64 | c LE32 yields 64 bytes = x mod p; the first x != 0 with
 * x^3 + 5 a square is taken, y = the even root.  Unknown discrete logarithms; reproducible from the string alone; index-
 * addressed like the other families (a rank generates its own range).  label_len <= 64. */
int  vdf_bases_generate_label(vdf_ctx* ctx, int curve, const uint8_t* label, size_t label_len, size_t start, size_t n, vdf_bases** out);
/* Build the fixed-base table  2^(window_bits*sets*j) * P_i, j = 0..tables-1, so that an MSM
 * needs only `sets` bucket sets (sets == 0: library default; sets == windows: no table).  window_bits == 0: the
 * recommended window for this many generators (16 below 2^19 generators, 17 from there on).  A table serves MSMs over
 * any sub-range of its generators; for MSMs much shorter than the table choose the window by their length. */
int  vdf_bases_precompute(vdf_ctx* ctx, vdf_bases* bases, int window_bits, int sets);
int  vdf_bases_window(const vdf_bases* bases);            /* window of the current table, 0 without one */
/* Digit table for the SMALL commitments a prover waits on (the ~10^4-term witnesses and cross-term rows of
 * RecursiveSNARK::prove_step, src/nova/proof.rs:342-349): every multiple d * 2^(window_bits * j) * P_i, d = 1 .. 2^(window_bits-1),
 * of the generators in up to 4 disjoint index ranges.  vdf_msm / vdf_msm_batch calls whose vectors all lie inside those
 * ranges (at most 2^17 scalars per call) then skip the bucket method: signed digits select table entries and the MSM is
 * a plain sum of gathered points -- two launches, ~20 dependent additions instead of a sort and ~80.  Same group element;
 * its Jacobian representative differs from the bucket method's.  HBM: count * W * 2^(window_bits-1) * 64 bytes, W =
 * ceil(256 / window_bits) (+1 when the top digit could overflow): 852 KB per generator at window_bits = 10 (0 = that).
 * ranges = 0 drops the table.  VDF_MSM_DIRECT=0 in the environment disables the path (tuning). */
int  vdf_bases_precompute_digits(vdf_ctx* ctx, vdf_bases* bases, int window_bits, int ranges, const size_t begin[], const size_t count[]);
/* HBM a digit table at window c over `generators` generators takes (64 B x windows(c) x 2^(c-1) each), 0 for a window the
 * library refuses; and what the fixed-base table of `bases` holds (0 without one).  No device work. */
size_t vdf_digit_table_bytes(int window_bits, size_t generators);
size_t vdf_bases_table_bytes(const vdf_bases* bases);
int  vdf_bases_digit_window(const vdf_bases* bases);      /* window of the digit table, 0 without one */
size_t vdf_bases_digit_table_bytes(const vdf_bases* bases); /* HBM held by the digit table, 0 without one */
int  vdf_bases_download(vdf_ctx* ctx, const vdf_bases* bases, size_t offset, size_t n, vdf_affine* out);
size_t vdf_bases_len(const vdf_bases* bases);
const void* vdf_bases_device_ptr(const vdf_bases* bases);
void vdf_bases_free(vdf_bases* bases);

/* ---- multi-scalar multiplication ------------------------------------------------------ */
/* out = sum_{i<n} scalars[i] * bases[offset + i].
 * Replaces nova-snark `Group::vartime_multiscalar_mul` -> pasta_msm::pallas/vesta
 * (the Pedersen commit of W and T inside prove_step, src/nova/proof.rs:342-349; K1/K2).
 * is_mont: scalars are in Montgomery form (as pasta-msm's `is_mont = true`). */
int  vdf_msm(vdf_ctx* ctx, const vdf_bases* bases, size_t offset, const vdf_fe* scalars, size_t n,
             int is_mont, vdf_jac* out);
/* k <= 4 MSMs over the same generator table in one pipeline: out[i] = sum_j scalars[i][j] * bases[offset[i] + j],
 * j < n[i].  The results equal k vdf_msm calls bit for bit; the batch shares every launch -- one sort, one
 * bucket-accumulation grid balanced over all entries, one latency-bound tail -- which is what a fold needs when it
 * commits to the fresh witness and to the cross term under the same generators (nova-snark commit_W / commit_T).
 * `out` holds k points, host or device. */
int  vdf_msm_batch(vdf_ctx* ctx, const vdf_bases* bases, int k, const size_t offset[], const vdf_fe* const scalars[],
                   const size_t n[], int is_mont, vdf_jac out[]);
/* The same batch with the vectors arriving one at a time -- an MSM *job*.  vdf_msm_job_push(g) starts the sort and
 * bucket accumulation of vector g on a stream of its own, ordered after the work already enqueued on the context
 * (the kernel that produces the vector) and leaving the context's stream free: a fold pushes the fresh witness,
 * enqueues the cross-term kernel, pushes T -- and T's production and sort run under the witness's ALU-bound
 * accumulation.  vdf_msm_job_finish waits for all vectors, runs the one shared bucket reduction and delivers the k
 * points (host, pinned or device memory) like vdf_msm_batch; it ends the job in every case.  Needs a fixed-base
 * table with one bucket set; scalars in device memory; one job per context at a time, and no other MSM on the
 * context while it is open.  Results equal vdf_msm / vdf_msm_batch bit for bit (as affine points). */
typedef struct vdf_msm_job vdf_msm_job;
int  vdf_msm_job_begin(vdf_ctx* ctx, const vdf_bases* bases, int k, const size_t offset[], const size_t n[], int is_mont,
                       vdf_msm_job** out);
int  vdf_msm_job_push(vdf_msm_job* job, int g, const vdf_fe* scalars);
int  vdf_msm_job_finish(vdf_msm_job* job, vdf_jac out[]);
/* Window size override for tuning (0 = automatic).  It applies to calls without a fixed-base table (a table fixes its own
 * window); a batch too wide for the requested window -- bucket sets x 2^(window - 11) sort partitions, at most 8192 --
 * runs at the largest window that fits. */
int  vdf_ctx_set_msm_window(vdf_ctx* ctx, int window_bits);
/* out = sum of n Jacobian points (the combine step of a point-chunk-sharded MSM: each GPU
 * contributes one 96-byte partial, exchanged with an RCCL all-gather). */
int  vdf_point_sum(vdf_ctx* ctx, int curve, const vdf_jac* points, size_t n, vdf_jac* out);
/* ---- one MSM across the GPUs of a node (no reference counterpart: the reference is one process) ----------
 * Point-chunk sharding: a rank owns generators [start, start + count) for good (with their fixed-base table) and gets
 * the matching slice of scalars; it contributes ONE 96-byte partial; elliptic-curve addition is no RCCL reduction
 * operator, so the exchange is an all-gather of the partials (latency-bound over xGMI) and every rank sums them itself.
 *
 * One process per GPU: the host supplies the collective.  `gather` receives device pointers -- `send` (bytes) and `recv`
 * (world * bytes, rank-major) -- and the hipStream_t the partial was produced on, on which it must order the
 * collective: RCCL `ncclAllGather(send, recv, bytes, ncclChar, comm, (hipStream_t)stream)`; returns 0 on success.
 * partial / gathered: device buffers of 1 / `world` points the caller owns (they stay valid through the collective).
 * flags: VDF_SHARDED_ALWAYS_GATHER takes the collective path for world == 1 too (rehearsal on one GPU). */
typedef int (*vdf_allgather_fn)(void* user, const void* send, void* recv, size_t bytes, void* stream);
enum { VDF_SHARDED_ALWAYS_GATHER = 1 };
int  vdf_msm_sharded(vdf_ctx* ctx, const vdf_bases* shard_bases, size_t offset, const vdf_fe* shard_scalars, size_t n, int is_mont,
                     int rank, int world, vdf_allgather_fn gather, void* user, int flags, vdf_jac* partial, vdf_jac* gathered,
                     vdf_jac* out);
/* One process driving k GPUs (k <= 64): ctxs[i] / bases[i] / scalars[i] / n[i] are device i's context, generator shard
 * and scalar slice (device or host memory); all partials are computed concurrently, land in pinned host memory and are
 * summed on ctxs[0]'s device.  Blocking. */
int  vdf_msm_multi(vdf_ctx* const ctxs[], const vdf_bases* const bases[], const size_t offsets[], const vdf_fe* const scalars[],
                   const size_t n[], int k, int is_mont, vdf_jac* out);
/* Stage timing of MSM calls (HIP events on the context's stream; for bench.py's roofline leg).
 * enable != 0 records events around the stages of every following vdf_msm.  vdf_msm_timing
 * synchronises and returns, summed over the calls since the last query:
 * ms[0] = sort (digits, histogram, scans, scatter), ms[1] = bucket accumulation kernel,
 * ms[2] = tail (fix-up, bucket reduction, final), ms[3] = whole pipeline; *calls = number of MSMs. */
int  vdf_ctx_set_timing(vdf_ctx* ctx, int enable);
int  vdf_msm_timing(vdf_ctx* ctx, float ms[4], int* calls);
/* Per-launch timing of EVERY kernel a context enqueues (bench.py's per-kernel roofline of prove_step).  While enabled,
 * each launch is bracketed by two HIP events on the stream it runs on.  vdf_ctx_kernel_events synchronises the context's
 * stream and drains the launches recorded since the last call: kernel name, the ALGORITHMIC bytes the launch is priced at
 * (96 B per (base, scalar) pair on an MSM's accumulation kernel, 96 B per folded element, 64 + 32 * vars B
 * per MinRoot round, the CSR + vector bytes of a cross term; 0 for the helper kernels of a pipeline) and start / end in
 * milliseconds since a per-device origin shared by all contexts -- so the launches of several contexts (a prover's three
 * queues) can be laid on one time line.  out == NULL: *n = launches waiting, nothing drained.  Costs two event records
 * per launch while on: measure throughput with it off. */
typedef struct { char name[24]; double bytes; double start_ms, end_ms; } vdf_kernel_event;
int  vdf_ctx_set_kernel_timing(vdf_ctx* ctx, int enable);
int  vdf_ctx_kernel_events(vdf_ctx* ctx, vdf_kernel_event* out, size_t cap, size_t* n);

/* Drop-in shims with the upstream pasta-msm 0.1.1 shape (upload-on-call, default context on device 0).  The
 * signature returns nothing and an all-zero `out` is the identity -- a valid-looking commitment -- so a call that
 * cannot compute (no device, out of memory, a failed launch) prints the reason on stderr and abort()s instead of
 * returning; a caller that wants a status code uses vdf_bases_upload + vdf_msm. */
void mult_pippenger_pallas(vdf_jac* out, const vdf_affine* points, size_t npoints, const vdf_fe* scalars, bool is_mont);
void mult_pippenger_vesta(vdf_jac* out, const vdf_affine* points, size_t npoints, const vdf_fe* scalars, bool is_mont);
/* Generator cache of the shims: keep up to `entries` (0..64; 0 = off, the default; the environment variable
 * VDF_SHIM_CACHE sets the initial value) generator arrays resident, recognised by (curve, address, length) and a
 * content hash of ALL their points (one pass over the array per call, on up to 8 host threads: ~0.3 ms at 2^19
 * points); from the second call on a set also gets its fixed-base table.  For callers whose generators do not change
 * -- nova-snark's CommitGens -- the unmodified pasta-msm call then costs a hash, a scalar upload and a table MSM instead
 * of a 64-byte-per-point upload and a table-less MSM.  An array rewritten in place, anywhere, hashes differently and is
 * uploaded again.  The address is used as a key only and never dereferenced outside the call that passes it. */
int  vdf_shim_set_cache(int entries);

/* ---- R1CS shape + sparse mat-vec ------------------------------------------------------- */
/* Replaces nova-snark R1CSShape{A,B,C} (COO triples over z = (W, u, X)) and
 * `R1CSShape::multiply_vec` (K4).  rows/cols/vals[k] describe matrix k = A, B, C; values in
 * Montgomery form.  The shape is converted to CSR with a coefficient dictionary and kept in HBM. */
int  vdf_shape_create(vdf_ctx* ctx, int field, size_t num_cons, size_t num_cols,
                      const uint32_t* const rows[3], const uint32_t* const cols[3],
                      const vdf_fe* const vals[3], const size_t nnz[3], vdf_shape** out);
void vdf_shape_free(vdf_shape* shape);
int  vdf_spmv3(vdf_ctx* ctx, const vdf_shape* shape, const vdf_fe* z, vdf_fe* Az, vdf_fe* Bz, vdf_fe* Cz);

/* ---- folding vector ops ---------------------------------------------------------------- */
/* T = Az1 o Bz2 + Az2 o Bz1 - u1*Cz2 - Cz1   (nova-snark `commit_T`, K5; u2 = 1). */
int  vdf_cross_term(vdf_ctx* ctx, int field, const vdf_fe* Az1, const vdf_fe* Bz1, const vdf_fe* Cz1,
                    const vdf_fe* Az2, const vdf_fe* Bz2, const vdf_fe* Cz2, const vdf_fe* u1,
                    size_t n, vdf_fe* T);
/* is_zero = 1 iff all n elements are zero, decided on the device (a verifier's residual A z o B z - u C z - E is checked
 * where it lies instead of being copied out); synchronises. */
int  vdf_vec_is_zero(vdf_ctx* ctx, const vdf_fe* v, size_t n, int* is_zero);
/* Which rows of an instance are unsatisfied: out[0] = the number of rows r < n with Az[r] * Bz[r] != Cz[r] (canonical Montgomery
 * elements of `field`, the product as every kernel makes it), out[1] = the smallest such r, UINT64_MAX when there is none.  One
 * pass over the three vectors (96 bytes per row), which must be device memory (VDF_ERR_BAD_ARG otherwise); out: host memory or
 * vdf_host_alloc memory, written when the call returns (an asynchronous context and vdf_host_alloc memory: after vdf_ctx_sync).
 * n = 0 writes {0, UINT64_MAX} and launches nothing.  A diagnostic for a strict instance (u = 1, E = 0): the fresh instance of a
 * step whose advice or round body is wrong (vdf_nova.h vdf_nova_proof_last_unsat). */
int  vdf_unsat_rows(vdf_ctx* ctx, int field, const vdf_fe* Az, const vdf_fe* Bz, const vdf_fe* Cz, size_t n, uint64_t out[2]);
/* out = a + r*b   (nova-snark RelaxedR1CSWitness::fold: W1 + r*W2, E1 + r*T; K6).
 * `r` is one field element (host or device).  out may alias a. */
int  vdf_axpy(vdf_ctx* ctx, int field, const vdf_fe* a, const vdf_fe* r, const vdf_fe* b, size_t n, vdf_fe* out);
/* Folding two RELAXED instances (Nova's folding scheme in its general form; vdf_nova.h vdf_nova_compress_aggregate).
 * vdf_cross_term_relaxed: T = Az1 o Bz2 + Az2 o Bz1 - u1*Cz2 - u2*Cz1, canonical; with u2 = 1 byte for byte vdf_cross_term's T.
 * vdf_fold_relaxed: in ONE pass over the n rows and in place on the index-1 vectors,
 *   Az1 += r*Az2, Bz1 += r*Bz2, Cz1 += r*Cz2, E1 += r*T + r^2*E2
 * (A z, B z, C z are linear in z: the accumulator's products stay current and no sparse product runs on it; z itself is folded
 * with vdf_axpy).  r^2 is formed once on the host.  With E2 = 0 the result is byte for byte four vdf_axpy calls.
 * u1, u2, r: canonical Montgomery elements in HOST memory (they travel in the kernel arguments).  Every vector: n elements of
 * device memory (vdf_ptr_is_device); the vectors a call writes may not overlap any other operand.  Refused with VDF_ERR_BAD_ARG:
 * a null pointer with n > 0, a host pointer where a vector is read or written, a device pointer for u1, u2 or r, an unknown
 * field.  n = 0 launches nothing and touches no pointer.  Asynchronous on an asynchronous context, like their neighbours. */
int  vdf_cross_term_relaxed(vdf_ctx* ctx, int field, const vdf_fe* Az1, const vdf_fe* Bz1, const vdf_fe* Cz1, const vdf_fe* u1,
                            const vdf_fe* Az2, const vdf_fe* Bz2, const vdf_fe* Cz2, const vdf_fe* u2, size_t n, vdf_fe* T);
int  vdf_fold_relaxed(vdf_ctx* ctx, int field, const vdf_fe* r, size_t n, vdf_fe* Az1, vdf_fe* Bz1, vdf_fe* Cz1, vdf_fe* E1,
                      const vdf_fe* Az2, const vdf_fe* Bz2, const vdf_fe* Cz2, const vdf_fe* E2, const vdf_fe* T);

/* ---- MinRoot step-circuit witness ------------------------------------------------------- */
/* Fills the 4t+1 auxiliary values `InverseMinRootCircuit::synthesize` allocates
 * (src/nova/proof.rs:107-126), in allocation order per round new_x, tmp1, tmp2, new_y
 * (src/nova/proof.rs:167, 176, 178, 181) then final_i (:122), from the forward trace
 * trace_xy[k] = (x_k, y_k), k = 0..t (trace_xy[t] is the step's `result`, trace_xy[0] its
 * `input`); i0 = the `i` of trace_xy[0].  Round-parallel. */
int  vdf_minroot_witness(vdf_ctx* ctx, int field, const vdf_fe* trace_xy, const vdf_fe* i0, uint64_t t,
                         vdf_fe* W_segment);

/* ---- MinRoot inverse walks: a step's forward trace rebuilt from the state it ends in ------------------------
 * The inverse round (src/minroot.rs:338-344) (x, y, i) -> (y - (i - 1), x^5 - (y - (i - 1)), i - 1) is three products where
 * the forward round is ~285, and lands exactly on the state the forward round started from.  One lane per walk.
 *
 * n independent walks of `rounds` inverse rounds (at most 2^22 per call).  states: n states in DEVICE memory, read as where
 * each walk stands and overwritten with where it stands afterwards (so a long walk may be cut into several calls).
 * trace_xy (device, or NULL for no trace): walk w writes (x, y) of the state it stands on BEFORE round r to
 *   trace_xy[2 * ((w / group) * group_stride + (w % group) * walk_stride + top - r)],   r = 0 .. rounds - 1
 * (elements of 32 bytes; walk_stride, group_stride and top in states; group = 0: all walks are one group and group_stride is
 * ignored), so a walk cut into calls passes top, top - rounds, ...; top >= rounds - 1.  The state a walk lands on is NOT
 * written (it is the next call's first, or the caller's to compare and store).  With walk_stride = top = rounds the walks of
 * one step's checkpoint intervals tile entries 1 .. t of that step's trace, each entry written once; group = walks per step
 * and group_stride = t + 1 then lay the steps of a window out trace after trace, in one launch.  The caller sizes trace_xy.
 * Exact: byte-identical to the host's rounds (vdf_nova.h vdf_minroot_inverse_round). */
int  vdf_minroot_inverse_walk(vdf_ctx* ctx, int field, vdf_state* states, size_t n, uint64_t rounds, vdf_fe* trace_xy,
                              size_t walk_stride, size_t top, size_t group, size_t group_stride);
/* ok[w] = 1 iff `rounds` inverse rounds from results[w] land on originals[w] (x, y and i): the reference's check
 * (src/minroot.rs:369-371), n at a time; rounds = 0 compares the states as they are.  results / originals / ok: host or device
 * (device inputs are left as they were).  Walks longer than 2^22 rounds are cut into launches by the call. */
int  vdf_minroot_check_batch(vdf_ctx* ctx, int field, const vdf_state* results, const vdf_state* originals, size_t n,
                             uint64_t rounds, int* ok);
/* trace_xy[2 * k * trace_stride] = (x, y) of states[k * state_stride], k < n (device memory; strides in states): entry 0 of
 * the traces of a window of steps from their input states. */
int  vdf_minroot_trace_heads(vdf_ctx* ctx, const vdf_state* states, size_t n, size_t state_stride, vdf_fe* trace_xy,
                             size_t trace_stride);

/* ---- MinRoot forward walks: many chains evaluated at once ---------------------------------------------------------------
 * The forward round (src/minroot.rs:329-335) (x, y, i) -> ((x + y)^e, x + i, i + 1) is 253 squarings and 30 products (Fp: 29) that
 * each wait for the one before.  A chain is sequential; chains are independent: one lane per chain.  This is a THROUGHPUT feature for
 * many chains (beacon lanes, sequential-work farms, test and benchmark corpora), NOT a faster VDF: a single chain on a lane is
 * far slower than vdf_minroot_eval on a host core (README.md has the measured ratio).
 *
 * n independent walks of `rounds` forward rounds, at most VDF_MINROOT_FORWARD_MAX_ROUNDS per call (VDF_ERR_BAD_ARG above it: a
 * round takes tens of microseconds and a launch must not hold a queue for seconds).  states: n states in DEVICE memory, read as
 * where each walk stands and overwritten with where it stands afterwards, so a long walk is cut into calls.  `base` = the rounds
 * the walks have behind them; with g = base + r + 1 the count after round r (r = 0 .. rounds - 1), walk w writes
 *   trace_xy[2 * (w * walk_stride + g)] = (x, y) after the round              (device, or NULL; walk_stride in entries of 64 B),
 *   checkpoints[w * cp_stride + g / every] = the state, when `every` divides g  (device, or NULL; cp_stride in states)
 * -- the ascending counterpart of vdf_minroot_inverse_walk's layout.  Entry 0 / checkpoint 0 (the state a walk starts from) is
 * the caller's to write.  The caller sizes both arrays.  The trace (64 B per round and chain) serves short walks and tests;
 * checkpoints are the interface to the prover (vdf_nova.h vdf_nova_circuits_push_checkpoints / _from_checkpoints, which rebuild
 * a step's trace by inverse walks at ~2 % of the evaluation's cost).  n = 0 or rounds = 0 do nothing.
 * Exact: states, checkpoints and trace entries are byte for byte what vdf_minroot_round gives (vdf_nova.h), in any mode. */
#define VDF_MINROOT_FORWARD_MAX_ROUNDS 2048
int  vdf_minroot_forward_walk(vdf_ctx* ctx, int field, vdf_state* states, size_t n, uint64_t rounds, vdf_state* checkpoints,
                              uint64_t every, size_t cp_stride, vdf_fe* trace_xy, size_t walk_stride, uint64_t base);
/* vdf_minroot_eval_checkpoints (vdf_nova.h) for n chains at once: rounds_total forward rounds from initial[w], cut into launches
 * of launch_rounds (0 = 1,024; at most VDF_MINROOT_FORWARD_MAX_ROUNDS) enqueued on the context's stream.  every = 0:
 * out_states[w] = the final state of chain w (n states).  every > 0 (it must divide rounds_total, VDF_ERR_BAD_ARG otherwise):
 * out_states[w * (rounds_total / every + 1) + k] = chain w after k * every rounds, k = 0 (the initial state) .. rounds_total /
 * every -- per chain exactly the array vdf_minroot_eval_checkpoints writes, and what vdf_nova_circuits_push_checkpoints /
 * _from_checkpoints take.  initial / out_states: host or device (a device `initial` is left as it was; they may not overlap). */
int  vdf_minroot_eval_batch(vdf_ctx* ctx, int field, const vdf_state* initial, size_t n, uint64_t rounds_total, uint64_t every,
                            uint64_t launch_rounds, vdf_state* out_states);

/* ---- fused step operations (one kernel launch each) --------------------------------------- */
/* The three entry points below do what a sequence of the calls above does, in a single launch and with
 * every single-field-element operand read from HOST memory and passed as a kernel argument: no staging
 * copy, no stream synchronisation.  They exist because one NIFS fold at 2^16 iterations is ~1 ms of GPU
 * work, so a dozen launches and half a dozen 32-byte uploads per step are a measurable share of it.
 * Vector operands must already be in device memory (VDF_ERR_BAD_ARG otherwise); results are identical,
 * bit for bit, to the unfused calls. */

/* The whole fresh column vector z = (W, u, X) of the exposed-IO MinRoot step circuit:
 *   z = [ z_in[0..3) | new_x, tmp1, tmp2, new_y per round (4t, as vdf_minroot_witness) | i0 | u | X[0..6) ]
 * i.e. vdf_minroot_witness plus the seven scalar stores around it.  z has 3 + 4t + 1 + 1 + 6 elements.
 * z_in, i0, u, X: host memory. */
int  vdf_minroot_step_z(vdf_ctx* ctx, int field, const vdf_fe* trace_xy, uint64_t t, const vdf_fe z_in[3],
                        const vdf_fe* i0, const vdf_fe* u, const vdf_fe X[6], vdf_fe* z);
/* The same, and also the witness without its new_x values:
 *   w_packed = [ z_in[0..3) | tmp1, tmp2, new_y per round (3t) | i0 ],  3t + 4 elements.
 * new_x of round j equals y_j - (i_j - 1), where y_j is z_in[1] (j = 0) or the previous round's new_y and i_j = z_in[2] - j
 * (src/nova/proof.rs:162-173): an affine image of another witness value.  A Pedersen commitment to W therefore needs
 * no term for it -- sum_j new_x_j G_j folds into the generators of the y_j and a point that depends on z_in[2] only --
 * and is an MSM over 3t + 4 instead of 4t + 4 points, with the same value (libvdf_nova.so uses this). */
int  vdf_minroot_step_z_packed(vdf_ctx* ctx, int field, const vdf_fe* trace_xy, uint64_t t, const vdf_fe z_in[3],
                               const vdf_fe* i0, const vdf_fe* u, const vdf_fe X[6], vdf_fe* z, vdf_fe* w_packed);
/* Only the variables `InverseMinRootCircuit::synthesize` allocates (src/nova/proof.rs:107-126), for a step circuit that
 * sits inside an augmented circuit: vars_per_round = 4: new_x, tmp1, tmp2, new_y per round (the reference's allocation,
 * as vdf_minroot_witness) ; vars_per_round = 3: tmp1, tmp2, new_y (the bound form, where new_x is the linear
 * combination y - i + 1 and no variable); then final_i = i0.  out has vars_per_round * t + 1 elements.  i0: host memory. */
int  vdf_minroot_step_segment(vdf_ctx* ctx, int field, const vdf_fe* trace_xy, uint64_t t, const vdf_fe* i0, int vars_per_round,
                              vdf_fe* out);
/* The reference's allocation (vars_per_round = 4) and, in the same pass, the scalars of its commitment WITHOUT the new_x
 * terms:   packed = [ tmp1, tmp2, new_y per round (3t) | final_i | y_0 | i_in | 1 ],  3t + 4 elements,
 * y_0 the y the first round reads and i_in the i it reads (= i0 + t; host memory, like i0).  new_x of round j is
 * y_j - (i_in - (j + 1)) with y_j = new_y of round j - 1 (src/nova/proof.rs:162-173), so over the generators G of `out`
 *   sum_j new_x_j G[4j]  =  y_0 G[0] + sum_(j>=1) new_y_(j-1) G[4j] - i_in S1 + S2,   S1 = sum_j G[4j],  S2 = sum_j (j + 1) G[4j]
 * and the commitment to `out` equals the MSM of `packed` over the derived generators
 *   [ G[4j+1], G[4j+2], G[4j+3] + G[4j+4] (last round: G[4t-1]) per round | G[4t] | G[0] | -S1 | S2 ]
 * -- the same group element from 3t + 4 instead of 4t + 1 terms (libvdf_nova.so commits the reference's circuit this way). */
int  vdf_minroot_step_segment_packed(vdf_ctx* ctx, int field, const vdf_fe* trace_xy, uint64_t t, const vdf_fe* i0, const vdf_fe* i_in,
                                     vdf_fe* out, vdf_fe* packed);
/* The variables of the FORWARD MinRoot step circuit (vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD), which proves a step in the
 * direction it was evaluated: per round j the fifth root x_(j+1) = trace_xy[j + 1].x, its square and its fourth power, then
 * final_i = i_end (the step's last round counter; host memory).  out has 3t + 1 elements; trace_xy as everywhere
 * (trace_xy[k] = (x_k, y_k), k = 0..t, device memory).  This is vdf_minroot_forward_segment_lanes with lanes = 1 and
 * lane_stride = t + 1: the same checks, the same launch. */
int  vdf_minroot_forward_segment(vdf_ctx* ctx, int field, const vdf_fe* trace_xy, uint64_t t, const vdf_fe* i_end, vdf_fe* out);
/* The same for `lanes` chains at once (vdf_nova.h VDF_CIRCUIT_MINROOT_FORWARD_LANES), ONE launch: lane l's trace starts
 * lane_stride entries of 64 B after lane l - 1's (lane_stride >= t + 1: the layout vdf_minroot_inverse_walk's groups and
 * vdf_minroot_forward_walk's walk_stride write) and its 3t + 1 variables follow lane l - 1's in out (lanes x (3t + 1) elements).
 * i_end: `lanes` elements in HOST memory, handed to the kernel as arguments (no staging copy, no synchronisation).
 * 1 <= lanes <= VDF_MINROOT_MAX_LANES.  Byte for byte what `lanes` calls of vdf_minroot_forward_segment write. */
#define VDF_MINROOT_MAX_LANES 16
int  vdf_minroot_forward_segment_lanes(vdf_ctx* ctx, int field, const vdf_fe* trace_xy, size_t lane_stride, uint64_t t, size_t lanes,
                                       const vdf_fe* i_end, vdf_fe* out);
/* ---- round tapes: the variables of t uniform repetitions of a round somebody else wrote (libvdf_nova.so's vdf_cs_repeat) --
 * A tape is a short straight-line program over a file of n_slots field values, run once per repetition j = 0 .. t - 1 by one
 * GPU thread each.  Every op is four bytes {op, dst, a, b}; dst and the operands of the arithmetic ops are slot numbers:
 *   VDF_TAPE_ADV    slot[dst] = advice entry j + b (b = 0 or 1), column a (a < n_adv)
 *   VDF_TAPE_INV    slot[dst] = inv[a]                  (loop-invariant values, a < n_inv)
 *   VDF_TAPE_J      slot[dst] = the constant j          (Montgomery form)
 *   VDF_TAPE_CONST  slot[dst] = consts[a]
 *   VDF_TAPE_ADD / _SUB / _MUL   slot[dst] = slot[a] (+ - *) slot[b]   (a = b under _MUL is a squaring)
 *   VDF_TAPE_SCALE  slot[dst] = slot[a] * consts[b]
 *   VDF_TAPE_OUT    variable b of this repetition = slot[a]: out[j * n_vars + b]   (dst unused; b < n_vars)
 *   VDF_TAPE_POW    slot[dst] = slot[a] ^ E, E = consts[b] read as a PLAIN 256-bit little-endian integer (no field element, no
 *                   Montgomery form).  Forward walk tapes only (below): anywhere else it is a malformed op
 *   VDF_TAPE_POWC   slot[dst] = slot[a] ^ E(chain), the chain a caller-supplied addition chain that lies in the constants from
 *                   consts[b] on (vdf_pow_step below).  Forward walk tapes only, like VDF_TAPE_POW
 *   VDF_TAPE_TAB    slot[dst] = table[(J mod tab_rows) * tab_cols + a]: the round constant of round J from the tape's TABLE, a
 *                   short list cycled over the rounds.  J is the 64-bit value VDF_TAPE_J has in that round (already reduced
 *                   modulo 2^64 by the call's J rule), so the row is exactly J mod tab_rows for any tab_rows, a power of two
 *                   or not, also where a walk's J crosses 2^64.  a < tab_cols, b = 0.  Valid in round, walk and forward walk
 *                   tapes alike; it counts no product.  In a tape with tab_rows = 0 it is a malformed op
 * THE TABLE: one per tape, tab_rows x tab_cols elements (at most VDF_TAPE_MAX_TAB_ROWS x VDF_TAPE_MAX_TAB_COLS: 1 MiB), row-major,
 * canonical Montgomery form; tab_rows = tab_cols = 0 and table = NULL for a tape without one.  Unlike ops and consts it does NOT
 * travel in the kernel arguments (it would not fit, and a lane's row is a per-lane value: arguments indexed by one would go to
 * scratch): for the seven launchers of this header `table` is memory a kernel may read in place, as advice and entries are --
 * vdf_dev_alloc or vdf_host_alloc, checked with vdf_ptr_is_device; for the host evaluators of vdf_nova.h it is host memory.  A TAB
 * is a per-lane 32-byte load from it.  Nothing on the device can index out of range: the row is below tab_rows by construction
 * and the column is checked before the launch.  A tape that holds a TAB launches kernels of its own (k_round_tape_tab,
 * k_round_tape_lanes_tab, k_tape_walk_tab, k_tape_walk_lanes_tab, k_tape_forward_walk_tab, k_tape_rebuild_lanes_tab); every other tape launches the kernels
 * it always did.  Refused with VDF_ERR_BAD_ARG naming the op: a TAB with tab_rows = 0, a >= tab_cols or b != 0; and naming the
 * table: one dimension 0 beside a non-zero one, a cap exceeded, a null table with tab_rows > 0.
 * THE STRUCT GREW at its end by table, tab_rows, tab_cols (vdf_version r2): callers are rebuilt, and one that fills the struct
 * field by field sets the three to 0.
 * advice: (t + 1) entries of n_adv elements, entry-major (a MinRoot trace is n_adv = 2).  A slot is read only after an op of
 * the same tape wrote it (refused otherwise) and every variable is written exactly once.  n_cons, the constraints per
 * repetition, is carried for the caller (constraints cost nothing here).  The caps below are refused with VDF_ERR_BAD_ARG. */
enum { VDF_TAPE_ADV = 0, VDF_TAPE_INV = 1, VDF_TAPE_J = 2, VDF_TAPE_CONST = 3, VDF_TAPE_ADD = 4, VDF_TAPE_SUB = 5, VDF_TAPE_MUL = 6,
       VDF_TAPE_SCALE = 7, VDF_TAPE_OUT = 8, VDF_TAPE_POW = 9, VDF_TAPE_POWC = 10, VDF_TAPE_TAB = 11 };
#define VDF_TAPE_MAX_OPS 320      /* ops of a tape (loads and stores included) */
#define VDF_TAPE_MAX_CONSTS 24
#define VDF_TAPE_MAX_SLOTS 24     /* live values: 2 KiB of LDS each per 64 repetitions */
#define VDF_TAPE_MAX_VARS 64      /* variables per repetition */
#define VDF_TAPE_MAX_INV 16
#define VDF_TAPE_MAX_ADV 8
#define VDF_TAPE_MAX_TAB_ROWS 4096
#define VDF_TAPE_MAX_TAB_COLS 8
typedef struct vdf_tape_op { uint8_t op, dst, a, b; } vdf_tape_op;
typedef struct vdf_round_tape {
  const vdf_tape_op* ops;  size_t n_ops;       /* host memory */
  const vdf_fe* consts;    size_t n_consts;    /* host memory, Montgomery form */
  uint32_t n_slots, n_vars, n_cons, n_inv, n_adv;
  const vdf_fe* table;                         /* VDF_TAPE_TAB's table (above): device-readable for the launchers, host for vdf_nova.h's evaluators */
  uint32_t tab_rows, tab_cols;
} vdf_round_tape;
/* Runs the tape over repetitions 0 .. t - 1: out (device, t * n_vars elements) gets the variables, repetition-major.  inv: n_inv
 * elements in HOST memory; tape: host memory -- both travel as kernel arguments (no staging copy, no synchronisation).  advice:
 * device memory; tape->table (if any): device-readable memory, "a device pointer where host memory is read or the reverse"
 * otherwise, in all seven launchers.  Values are whatever the ops make of the advice: nothing is checked against a constraint. */
int  vdf_round_tape_run(vdf_ctx* ctx, int field, const vdf_round_tape* tape, uint64_t t, const vdf_fe* inv, const vdf_fe* advice,
                        vdf_fe* out);
/* The same for `lanes` advice arrays at once, ONE launch (kernel k_round_tape_lanes, the lane in the grid's second dimension):
 * lane l reads its advice lane_stride ENTRIES after lane l - 1's (lane_stride >= t + 1: with rounds_total / every + 1 the layout
 * vdf_round_tape_eval_batch writes per chain, with t + 1 the traces of vdf_round_tape_walk_lanes' groups back to back), writes its
 * t * n_vars variables at out + l * t * n_vars, and sees VDF_TAPE_J = j and its own inv[l * n_inv .. l * n_inv + n_inv).  inv: lanes *
 * n_inv elements in HOST memory, lane-major; all of them travel in the kernel arguments' block of VDF_TAPE_MAX_INV elements (no
 * staging copy, no synchronisation), hence the second cap.  Refused with VDF_ERR_BAD_ARG: lanes outside 1 .. VDF_TAPE_MAX_LANES,
 * lanes * n_inv > VDF_TAPE_MAX_INV, lane_stride < t + 1, and what vdf_round_tape_run refuses.
 * Byte for byte what `lanes` calls of vdf_round_tape_run write; vdf_nova.h vdf_nova_round_tape_eval_lanes restates it on the host
 * (what a launch of a tape is refused for is stated once for both libraries, in csrc/tape_launch.h). */
#define VDF_TAPE_MAX_LANES 16
int  vdf_round_tape_run_lanes(vdf_ctx* ctx, int field, const vdf_round_tape* tape, uint64_t t, size_t lanes, const vdf_fe* inv,
                              const vdf_fe* advice, size_t lane_stride, vdf_fe* out);
/* 1 when a kernel of this library may read p in place (device memory, or host memory of vdf_host_alloc), else 0 */
int  vdf_ptr_is_device(const void* p);
/* ---- walk tapes: the ADVICE of such rounds rebuilt on the device from checkpoints ---------------------------------------------
 * The same seam in the other direction.  Every delay function of this family is slow one way (a root) and a handful of products
 * per round the other way; a walk tape is that fast round, one advice entry computed from the one after it, and a walk is
 * `rounds` of them, sequential, one GPU lane per walk -- vdf_minroot_inverse_walk for a round the library did not write, with an
 * entry of n_adv elements where that call has a 64-byte (x, y).  This call walks in the DESCENDING direction; the slow direction,
 * a 254-bit exponentiation per round, is a forward walk tape (vdf_round_tape_forward_walk below, with VDF_TAPE_POW).
 *
 * A walk tape is a vdf_round_tape (same struct, same ops, same transport in the kernel arguments) read under these rules:
 *   n_vars == n_adv          what a round writes is one advice entry
 *   VDF_TAPE_ADV  b must be 1: slot[dst] = column a of the entry the walk stands on (entry j + 1); b = 0 would be the entry being
 *                 produced and is refused
 *   VDF_TAPE_OUT  column b of the produced entry (entry j) = slot[a]; every column exactly once.  An OUT does not disturb a later
 *                 ADV of the same column in the same round
 *   VDF_TAPE_J    j, the index of the produced entry -- the meaning j has in the round body, whose repetition j relates entries j
 *                 and j + 1
 * everything else as above.  vdf_nova.h vdf_nova_walk_body_record makes one from a callback.
 *
 * entries (device, n x n_adv elements): entries[w] is where walk w stands; it is overwritten with where it lands, so a long walk
 * is cut into calls.  Strides are in ENTRIES.  With g = w / group and the local index k = (w % group) * walk_stride + top - r,
 * r = 0 .. rounds - 1 (group = 0: all walks are one group and group_stride is ignored), walk w
 *   writes the entry it stands on before round r to trace[(g * group_stride + k) * n_adv]      (trace: device, or NULL)
 *   and sees VDF_TAPE_J = j_base + g * j_group_step + k - 1 in that round (arithmetic modulo 2^64),
 * so a window of steps laid out trace after trace sees a chain-global counter under one host `inv`.  top >= rounds - 1.
 * heads != 0: the first walk of each group also writes the entry it lands on, at local index top - rounds (then top >= rounds):
 * with walk_stride = top = rounds one launch leaves complete traces 0 .. t, one per group, each entry written once -- what
 * vdf_cs_repeat reads as advice.  expect (device, n x n_adv, or NULL): ok[w] (device, required with expect) = 1 iff the landing
 * equals expect[w] in every column -- the checkpoint check, so that nothing comes back to the host but n ints.
 *
 * Refused with VDF_ERR_BAD_ARG before anything is launched: a malformed tape (opcode, slot, column, constant, a read before a
 * write, a column written twice or never), n_vars != n_adv, an ADV with b = 0, top < rounds - 1 (heads: top < rounds) with a
 * trace, expect without ok, a device pointer where host memory is read or the reverse, n_slots + 2 * n_adv > VDF_WALK_MAX_SLOTS
 * (the value file and the two entries are 2 KiB of LDS each per wavefront: 64 KiB, the most a launch gets without asking), and
 * rounds * max(1, products per round) > VDF_WALK_MAX_WORK (products: the tape's MUL and SCALE ops) -- the order of the built-in
 * walk's own cap of 2^22 rounds of three products, so that one launch holds a queue no longer than the built-in one may; callers
 * cut longer walks into calls.  n = 0 or rounds = 0 do nothing.
 * Exact: every value is canonical after every op; entries and trace are byte for byte vdf_nova_walk_tape_eval's (vdf_nova.h). */
#define VDF_WALK_MAX_SLOTS 32
#define VDF_WALK_MAX_WORK (1ull << 23)
int  vdf_round_tape_walk(vdf_ctx* ctx, int field, const vdf_round_tape* tape, const vdf_fe* inv, vdf_fe* entries, size_t n,
                         uint64_t rounds, vdf_fe* trace, size_t walk_stride, size_t top, size_t group, size_t group_stride,
                         uint64_t j_base, uint64_t j_group_step, int heads, const vdf_fe* expect, int32_t* ok);
/* vdf_round_tape_walk for the chains of `lanes` lanes in ONE launch (kernel k_tape_walk_lanes), with the groups numbered step-major,
 * lane-minor: group G = w / group = g * lanes + l is lane l of step g.  Everything is vdf_round_tape_walk's with G in the place of
 * its g, except what a lane owns: the trace of G lies at G * group_stride (with group_stride = t + 1 a step's trace is its lanes'
 * traces back to back -- vdf_round_tape_run_lanes' advice at lane_stride = t + 1), and a walk of G sees
 *   VDF_TAPE_J = j_base[l] + g * j_group_step + k - 1 (modulo 2^64) and inv[l * n_inv .. l * n_inv + n_inv).
 * inv: lanes * n_inv elements, j_base: `lanes` counters, both HOST memory, carried in the kernel arguments.  group = 0: all walks
 * are group 0, lane 0 of step 0.  heads, expect and ok as there.  A thread keeps its lane's inv in n_inv more slots of LDS, so the
 * cap on slots is n_slots + 2 * n_adv + n_inv <= VDF_WALK_MAX_SLOTS here (also with lanes = 1); VDF_WALK_MAX_WORK holds as there.
 * Refused with VDF_ERR_BAD_ARG besides: lanes outside 1 .. VDF_TAPE_MAX_LANES, lanes * n_inv > VDF_TAPE_MAX_INV, a null j_base.
 * With lanes = 1 entries, trace and ok are byte for byte vdf_round_tape_walk's; for any lanes vdf_nova_walk_tape_eval_lanes'. */
int  vdf_round_tape_walk_lanes(vdf_ctx* ctx, int field, const vdf_round_tape* tape, size_t lanes, const vdf_fe* inv, vdf_fe* entries,
                               size_t n, uint64_t rounds, vdf_fe* trace, size_t walk_stride, size_t top, size_t group,
                               size_t group_stride, const uint64_t* j_base, uint64_t j_group_step, int heads, const vdf_fe* expect,
                               int32_t* ok);
/* ---- forward walk tapes: the chain itself evaluated on the device, many chains at once --------------------------------------
 * The ascending counterpart: the SLOW direction of the round, advice entry j + 1 computed from entry j, one GPU lane per chain --
 * vdf_minroot_forward_walk for a round the library did not write, in that call's layout with an entry of n_adv elements in
 * place of (x, y).  Like that call it is a THROUGHPUT feature for many chains (beacon lanes, sequential-work farms, test and
 * benchmark corpora), NOT a faster VDF: a single chain on a lane is far slower than a host core.
 *
 * A forward walk tape is a vdf_round_tape read under these rules:
 *   n_vars == n_adv          what a round writes is one advice entry
 *   VDF_TAPE_ADV  b must be 0: slot[dst] = column a of the entry the walk stands on (entry j); b = 1 would be the entry being
 *                 produced and is refused
 *   VDF_TAPE_OUT  column b of the produced entry (entry j + 1) = slot[a]; every column exactly once.  An OUT does not disturb a
 *                 later ADV of the same column in the same round
 *   VDF_TAPE_J    j, the index of the entry the walk stands on -- the j of the round body whose repetition j relates entries j
 *                 and j + 1
 *   VDF_TAPE_POW  slot[dst] = slot[a] ^ E, E = the 256 bits of consts[b] as a plain little-endian integer.  E = 0 gives 1 (also
 *                 for base 0), E = 1 copies, any E < 2^256 is accepted; the result is canonical like every other op's.  Left to
 *                 right square-and-multiply from the top set bit: bitlen(E) - 1 squarings and popcount(E) - 1 products
 *   VDF_TAPE_POWC slot[dst] = slot[a] ^ E, E the exponent of the addition chain in consts[b ..] (below).  The result is canonical:
 *                 byte for byte what VDF_TAPE_POW with exponent E gives.  POW and POWC may stand in one tape
 * everything else as above.  vdf_nova.h vdf_nova_forward_body_record makes one from a callback (vdf_cs_pow, vdf_cs_pow_chain).
 *
 * An addition chain (vdf_pow_step) is a straight-line program over an accumulator v and n_tmp temporaries T[0 .. n_tmp), T[0] the
 * base on entry.  One step is
 *   v = T[src] unless src == VDF_POW_ACC;  v = v^(2^squarings);  v = v * T[mul] unless mul == VDF_POW_NONE;
 *   T[dst] = v unless dst == VDF_POW_NONE
 * and the result is v after the last step.  Its exponent E follows from the steps: e(T[0]) = 1, and a step gives e = e(src) *
 * 2^squarings + e(mul).  A chain is VALID when it has 1 .. VDF_POW_CHAIN_MAX_STEPS steps, n_tmp is 1 .. VDF_POW_CHAIN_MAX_TMP and
 * every index is below n_tmp, step 0 does not start from VDF_POW_ACC, no temporary is read before a step wrote it (T[0] counts as
 * written) and every intermediate exponent is below 2^256.  A step of 0 squarings, no product and no dst is legal (padding).
 * In a tape the chain is read as plain BYTES, as VDF_TAPE_POW reads its exponent as a plain integer: byte 0 of consts[b] is n_steps,
 * byte 1 n_tmp, bytes 2 and 3 zero; the steps follow at four bytes each and run on into consts[b + 1] and further, ceil((4 + 4
 * n_steps) / 32) constants in all (at most 12); the bytes behind the last step up to the end of the last constant are zero.
 * The kernel (k_tape_forward_walk_chain, launched only for a tape that holds a POWC; any other tape launches k_tape_forward_walk as
 * before) keeps the accumulator in registers and the temporaries in n_tmp more slots of LDS, all products in the lazy domain and
 * the result made canonical once.  A POWC counts max(1, sum of squarings + steps with a product) products.
 * Refused with VDF_ERR_BAD_ARG on top of the list below: an invalid chain, one that runs past n_consts, non-zero padding, and
 * n_slots + 2 * n_adv + (the largest n_tmp of the tape's chains) > VDF_WALK_MAX_SLOTS.
 *
 * entries (device, n x n_adv elements): entries[w] is where walk w stands; it is overwritten with where it stands afterwards, so
 * long chains are cut into calls.  Strides are in ENTRIES.  `base` = the rounds the walks have behind them; with g = base + r + 1
 * the count after round r (r = 0 .. rounds - 1), walk w
 *   writes the entry it produced to trace[(w * walk_stride + g) * n_adv]                        (trace: device, or NULL),
 *   and to checkpoints[(w * cp_stride + g / every) * n_adv] when `every` divides g              (checkpoints: device, or NULL),
 *   and sees VDF_TAPE_J = j_base + w * j_walk_step + base + r in that round (arithmetic modulo 2^64).
 * Entry 0 and checkpoint 0 (where a walk starts) are the caller's to write; the caller sizes both arrays.
 *
 * Refused with VDF_ERR_BAD_ARG before anything is launched: a malformed tape (opcode, slot, column, constant, a read before a
 * write, a column written twice or never), n_vars != n_adv, an ADV with b = 1, checkpoints without `every`, a device pointer where
 * host memory is read or the reverse, n_slots + 2 * n_adv > VDF_WALK_MAX_SLOTS, and rounds * max(1, products per round) >
 * VDF_FORWARD_TAPE_MAX_WORK, where MUL and SCALE count one product each and a POW of exponent E counts max(1, bitlen(E) - 1 +
 * popcount(E) - 1): 2^20 is within a factor two of what the built-in forward walk allows one launch (2,048 rounds of 283
 * products), so that one launch holds a queue no longer than that one may.  n = 0 or rounds = 0 do nothing.
 * Exact: entries, checkpoints and trace are byte for byte vdf_nova_forward_tape_eval's (vdf_nova.h). */
#define VDF_FORWARD_TAPE_MAX_WORK (1ull << 20)
typedef struct vdf_pow_step { uint8_t src, squarings, mul, dst; } vdf_pow_step;
#define VDF_POW_ACC  0xFE   /* src: go on from the accumulator */
#define VDF_POW_NONE 0xFF   /* mul: no product; dst: nothing kept */
#define VDF_POW_CHAIN_MAX_STEPS 95
#define VDF_POW_CHAIN_MAX_TMP   12
int  vdf_round_tape_forward_walk(vdf_ctx* ctx, int field, const vdf_round_tape* tape, const vdf_fe* inv, vdf_fe* entries, size_t n,
                                 uint64_t rounds, vdf_fe* checkpoints, uint64_t every, size_t cp_stride, vdf_fe* trace,
                                 size_t walk_stride, uint64_t base, uint64_t j_base, uint64_t j_walk_step);
/* ---- traces rebuilt by forward tapes: vdf_round_tape_walk_lanes ascending -----------------------------------------------------
 * For a round with no cheap inverse (a Rescue-shaped round has a root layer AND a power layer; a lossy mix has no inverse at all):
 * one lane per checkpoint interval walks UP from the checkpoint below with the chain's own forward tape, writes the entries it
 * produces where vdf_cs_repeat reads its advice, and is compared with the checkpoint above.  The tape is read under the rules of a
 * forward walk tape (ADV with b = 0 only; POW, POWC and TAB admitted).  The groups are vdf_round_tape_walk_lanes': group G =
 * w / group = g * lanes + l is lane l of step g; group = 0: everything is group 0 and group_stride is ignored.  Strides are in ENTRIES.
 * `base` = the rounds the walks have behind them.  Before round r (r = 0 .. rounds - 1) walk w stands on local index
 * k = (w % group) * walk_stride + base + r, and in that round it
 *   sees VDF_TAPE_J = j_base[l] + g * j_group_step + k (modulo 2^64): the index of the entry it stands on, the j of the round body's
 *   repetition j -- the value the descending walk sees when it PRODUCES that entry, so one chain's two tapes take the same j_base;
 *   writes the entry it produced to trace[(G * group_stride + k + 1) * n_adv]                  (trace: device, or NULL).
 * heads != 0: the first walk of each group also writes the entry it stands on before round 0 of the call, at local index `base`.
 * With walk_stride = every and slices that add up to `every`, one window's launches leave complete traces 0 .. t per group; the
 * interior boundaries are written once each, by the walk below -- its landing, not the checkpoint (the two are compared).
 * expect / ok as in the descending call: ok[w] = 1 iff the entry the walk stands on after the call equals expect[w] in every column.
 * entries[w] is overwritten with where the walk stands afterwards.  inv (lanes * n_inv elements, lane-major) and j_base (`lanes`
 * counters) are HOST memory and travel in the kernel arguments; a thread keeps its lane's inv in n_inv more slots of LDS.
 * Kernels: k_tape_rebuild_lanes, and k_tape_rebuild_lanes_tab for a tape that holds a TAB; lanes = 1 is the same kernel.
 * Refused with VDF_ERR_BAD_ARG before anything is launched: everything vdf_round_tape_forward_walk refuses of a tape; lanes outside
 * 1 .. VDF_TAPE_MAX_LANES, lanes * n_inv > VDF_TAPE_MAX_INV, a null j_base; expect without ok; with a trace and more than one walk
 * per group, base + rounds > walk_stride; n_slots + 2 * n_adv + n_inv + (the largest n_tmp of the tape's chains) >
 * VDF_WALK_MAX_SLOTS; rounds * max(1, products per round) > VDF_FORWARD_TAPE_MAX_WORK; a device pointer where host memory is read
 * or the reverse.  n = 0 or rounds = 0 do nothing.
 * Exact: entries, trace and ok are byte for byte vdf_nova_forward_tape_rebuild_eval_lanes' (vdf_nova.h). */
int  vdf_round_tape_rebuild_lanes(vdf_ctx* ctx, int field, const vdf_round_tape* forward_tape, size_t lanes, const vdf_fe* inv,
                                  vdf_fe* entries, size_t n, uint64_t rounds, vdf_fe* trace, size_t walk_stride, uint64_t base,
                                  size_t group, size_t group_stride, const uint64_t* j_base, uint64_t j_group_step, int heads,
                                  const vdf_fe* expect, int32_t* ok);
/* vdf_minroot_eval_batch for a forward walk tape: rounds_total rounds from initial[w] (n x n_adv elements), cut into launches of
 * launch_rounds (0 = the largest count VDF_FORWARD_TAPE_MAX_WORK allows the tape, at most 1,024) enqueued on the context's stream.
 * every = 0: out_entries[w * n_adv] = the final entry of chain w (n entries).  every > 0 (it must divide rounds_total,
 * VDF_ERR_BAD_ARG otherwise): out_entries[(w * (rounds_total / every + 1) + k) * n_adv] = chain w after k * every rounds, k = 0
 * (the initial entry) .. rounds_total / every -- per chain the checkpoint array vdf_round_tape_walk's `expect` is cut from.
 * Chain w sees VDF_TAPE_J = j_base + w * j_walk_step + (rounds behind it).  initial / out_entries: host or device (a device
 * `initial` is left as it was; they may not overlap).  tape, inv: host memory. */
int  vdf_round_tape_eval_batch(vdf_ctx* ctx, int field, const vdf_round_tape* tape, const vdf_fe* inv, const vdf_fe* initial, size_t n,
                               uint64_t rounds_total, uint64_t every, uint64_t launch_rounds, uint64_t j_base, uint64_t j_walk_step,
                               vdf_fe* out_entries);
/* vdf_spmv3(shape, z2) followed by vdf_cross_term(Az1, Bz1, Cz1, Az2, Bz2, Cz2, u1): writes Az2, Bz2, Cz2
 * (num_cons each) and T.  u1: host memory.  (nova-snark NIFS::prove -> commit_T, K4 + K5.) */
int  vdf_nifs_cross_term(vdf_ctx* ctx, const vdf_shape* shape, const vdf_fe* z2, const vdf_fe* Az1, const vdf_fe* Bz1,
                         const vdf_fe* Cz1, const vdf_fe* u1, vdf_fe* Az2, vdf_fe* Bz2, vdf_fe* Cz2, vdf_fe* T);
/* The same over part of the rows: VDF_ROWS_INSIDE = the rows [row_begin, row_begin + row_count) only, VDF_ROWS_OUTSIDE =
 * every row but those.  The vectors are full-length either way (num_cons); only the selected rows are read and written.
 * A prover that knows part of the fresh witness early (the step circuit's own variables, made ahead of the step) runs
 * the rows that read nothing else on another context before the rest of the witness exists; the range must not hold a
 * row of more than 8 entries (those are summed by a wavefront in the OUTSIDE / ALL call). */
#define VDF_ROWS_ALL 0
#define VDF_ROWS_INSIDE 1
#define VDF_ROWS_OUTSIDE 2
int  vdf_nifs_cross_term_rows(vdf_ctx* ctx, const vdf_shape* shape, size_t row_begin, size_t row_count, int part, const vdf_fe* z2,
                              const vdf_fe* Az1, const vdf_fe* Bz1, const vdf_fe* Cz1, const vdf_fe* u1, vdf_fe* Az2, vdf_fe* Bz2,
                              vdf_fe* Cz2, vdf_fe* T);
/* The same rows for the built-in MinRoot step circuits WITHOUT the sparse matrices: the 3t + 1 constraints of
 * InverseMinRootCircuit::synthesize (src/nova/proof.rs:107-133, :219-227) are a fixed stencil over the rounds' own
 * variables -- A z2, B z2, C z2 of a row are copies of witness values and one four-term sum -- so rows
 * [row_begin, row_begin + 3t + 1) are computed from coalesced streams only (no row pointers, columns, coefficients or
 * gathers).  seg_begin: index of the first round variable in z2 (the step circuit's input x, y, i occupies the three
 * variables before it); vars_per_round: 4 = the reference's rounds (new_x, tmp1, tmp2, new_y), 3 = the bound form;
 * one_col: the constant's column (num_vars).  Exact for any z2.  The caller is responsible for the rows being that
 * stencil (libvdf_nova.so compares it with the shape's triples once, at public_params).  Vectors: device memory,
 * full length (num_cons / num_cols); u1: host memory. */
int  vdf_nifs_cross_term_minroot(vdf_ctx* ctx, int field, int vars_per_round, uint64_t t, size_t seg_begin, size_t one_col, size_t row_begin,
                                 const vdf_fe* z2, const vdf_fe* Az1, const vdf_fe* Bz1, const vdf_fe* Cz1, const vdf_fe* u1, vdf_fe* Az2,
                                 vdf_fe* Bz2, vdf_fe* Cz2, vdf_fe* T);
/* The stencil of the FORWARD step circuit, rows [row_begin, row_begin + 3t + 1), with x' = x_(j+1), tmp1, tmp2 of round j at
 * seg_begin + 3j .. + 2, final_i at seg_begin + 3t and z_in = (x_0, y_0, i) in the three variables before seg_begin:
 *   row 3j      x' * x' = tmp1;    row 3j + 1   tmp1 * tmp1 = tmp2;
 *   row 3j + 2  tmp2 * x' = x_j + y_j   (j = 0: z_in.x + z_in.y; j >= 1: x_j + x_(j-1) + i + (j - 1) * one);
 *   row 3t      final_i * one = i + t * one.
 * Operands and guarantees as vdf_nifs_cross_term_minroot (exact for any z2; the caller answers for the rows being this
 * stencil).  libvdf_nova.so reports this stencil as code 5 (vdf_nova_pp_stencil).  This is
 * vdf_nifs_cross_term_minroot_forward_lanes with lanes = 1: the same checks, the same launch. */
int  vdf_nifs_cross_term_minroot_forward(vdf_ctx* ctx, int field, uint64_t t, size_t seg_begin, size_t one_col, size_t row_begin,
                                         const vdf_fe* z2, const vdf_fe* Az1, const vdf_fe* Bz1, const vdf_fe* Cz1, const vdf_fe* u1,
                                         vdf_fe* Az2, vdf_fe* Bz2, vdf_fe* Cz2, vdf_fe* T);
/* The forward stencil over `lanes` lanes, ONE launch, rows [row_begin, row_begin + lanes (3t + 1)): lane l's variables are
 * seg_begin + l (3t + 1) .. + 3t (x', tmp1, tmp2 per round, then final_i), its rows row_begin + l (3t + 1) .., and ITS
 * z_in = (x_0, y_0, i) sits at seg_begin - 3 lanes + 3 l .. + 2, where the single-lane stencil reads seg_begin - 3 .. - 1.
 * Operands and guarantees as vdf_nifs_cross_term_minroot_forward (exact for any z2, a `one` that is not 1 included).
 * libvdf_nova.so reports this stencil as code 6 (vdf_nova_pp_stencil), and as code 5 when it runs one lane. */
int  vdf_nifs_cross_term_minroot_forward_lanes(vdf_ctx* ctx, int field, uint64_t t, size_t lanes, size_t seg_begin, size_t one_col,
                                               size_t row_begin, const vdf_fe* z2, const vdf_fe* Az1, const vdf_fe* Bz1,
                                               const vdf_fe* Cz1, const vdf_fe* u1, vdf_fe* Az2, vdf_fe* Bz2, vdf_fe* Cz2, vdf_fe* T);
/* ---- periodic rows: the cross term of the rows of t replays of ONE recorded round, WITHOUT the sparse matrices ------------------
 * What the stencils above are for the built-in circuits, for a round the library did not write (libvdf_nova.so vdf_cs_repeat).
 * Rows that come from replaying one tape are periodic: from some repetition on, row c of repetition j + 1 is row c of repetition
 * j with every column inside the repeat's run of variables moved by n_vars, every other column fixed, and every coefficient equal
 * but those that are affine in j.  A vdf_periodic_rows describes the rows of ONE repetition; the kernel evaluates them from
 * coalesced streams and a description of a few hundred bytes that travels in its arguments (no row pointers, no column or
 * coefficient loads, no staging copy, no synchronisation).  libvdf_nova.so finds the description in a shape's triples and checks
 * it against every repetition (vdf_nova.h vdf_nova_periodic_rows_detect).
 *
 * Row c (c < n_cons), matrix k (0 = A, 1 = B, 2 = C) holds the terms terms[row_start[3 c + k]] .. terms[row_start[3 c + k + 1] - 1];
 * row_start has 3 n_cons + 1 entries, ascending from 0 to n_terms.  In repetition j a term contributes coefficient * z2[column]:
 *   VDF_TERM_SEG  column = seg_begin + j * n_vars + col, col read as a SIGNED 32-bit offset (negative: a look-back into earlier
 *                 repetitions); coefficient = consts[c0]
 *   VDF_TERM_ABS  column = col (the circuit's inputs, an inv, the constant's column); coefficient = consts[c0], or, with
 *                 c1 != VDF_TERM_NO_SLOPE, consts[c0] + (j - j0) * consts[c1]
 * consts: host memory, Montgomery form.  Coefficients 1 and -1 cost an addition or a subtraction, anything else a product.
 * The caps, each refused one beyond with VDF_ERR_BAD_ARG; with them the whole description is 2 KiB of kernel arguments (1,024 B of terms, 768 B of constants, 200 B of row starts). */
enum { VDF_TERM_SEG = 0, VDF_TERM_ABS = 1 };
#define VDF_TERM_NO_SLOPE 0xFF
#define VDF_PERIODIC_MAX_ROW_TERMS 8   /* terms of one row in one matrix: vdf_nifs_cross_term_rows' bound on a row inside a range */
#define VDF_PERIODIC_MAX_ROWS 32       /* rows (constraints) per repetition */
#define VDF_PERIODIC_MAX_STARTS 97     /* ... and the entries of row_start they take: 3 VDF_PERIODIC_MAX_ROWS + 1 */
#define VDF_PERIODIC_MAX_TERMS 128     /* terms per repetition, all rows and matrices together */
#define VDF_PERIODIC_MAX_CONSTS 24
typedef struct vdf_periodic_term { uint8_t kind, c0, c1, pad; uint32_t col; } vdf_periodic_term;
typedef struct vdf_periodic_rows {
  uint32_t n_cons, n_vars;                          /* rows and variables per repetition */
  uint64_t j0;                                      /* the repetition the pattern was taken from: slopes count from it */
  const uint16_t* row_start;                        /* host memory, 3 n_cons + 1 entries */
  const vdf_periodic_term* terms;  size_t n_terms;  /* host memory */
  const vdf_fe* consts;            size_t n_consts; /* host memory, Montgomery form */
} vdf_periodic_rows;
/* Az2, Bz2, Cz2 and T of the rows row_begin + (j - j_first) * n_cons + c, j = j_first .. j_first + reps - 1, c < n_cons, with the
 * operands of vdf_nifs_cross_term_minroot_forward (vectors: device memory, full length num_cons / num_cols; u1: host memory).
 * Nothing else is touched.  Exact for any z2, a `one` that is not 1 included: byte for byte what vdf_nifs_cross_term writes into
 * the same rows for a shape whose rows are those terms (and vdf_nova_periodic_rows_eval on the host).  The caller answers for
 * the rows being those terms.  Checked before anything is launched, each VDF_ERR_BAD_ARG and never an access out of bounds: the
 * caps, term kinds, constant indices, row_start, j_first < j0, every column a term reaches for the first and the last j against
 * [0, num_cols), the row range against num_cons, more than 2^31 rows, a device pointer where host memory is read or the
 * reverse.  reps = 0 does nothing. */
int  vdf_nifs_cross_term_periodic(vdf_ctx* ctx, int field, const vdf_periodic_rows* rows, uint64_t j_first, uint64_t reps,
                                  size_t seg_begin, size_t row_begin, size_t num_cols, size_t num_cons, const vdf_fe* z2,
                                  const vdf_fe* Az1, const vdf_fe* Bz1, const vdf_fe* Cz1, const vdf_fe* u1, vdf_fe* Az2,
                                  vdf_fe* Bz2, vdf_fe* Cz2, vdf_fe* T);
/* The same rows with the PREVIOUS fold of those rows applied on the way.  A prover that keeps A z, B z, C z of the running
 * instance folds them after every step (X1 <- X1 + r X2); for the stencil rows the fresh vectors X2 of the previous step are
 * exactly what this call is about to overwrite in Az2 / Bz2 / Cz2.  So, per row: Az1 += r Az2, Bz1 += r Bz2, Cz1 += r Cz2
 * (and E1 += r T_prev when E1 is not NULL; T_prev may be T itself) with the vectors' CURRENT contents, stored in place; then
 * Az2, Bz2, Cz2 and T of z2 as vdf_nifs_cross_term_minroot computes them, crossed with the FOLDED running rows and u1 (the
 * caller passes the folded u).  One pass over the rows instead of a fold over whole vectors in front of it; the caller folds
 * z, and every vector outside [row_begin, row_begin + 3t + 1), with vdf_fold_many.  r, u1: host memory. */
int  vdf_nifs_cross_term_minroot_fold(vdf_ctx* ctx, int field, int vars_per_round, uint64_t t, size_t seg_begin, size_t one_col,
                                      size_t row_begin, const vdf_fe* z2, const vdf_fe* r, vdf_fe* Az1, vdf_fe* Bz1, vdf_fe* Cz1,
                                      vdf_fe* E1, const vdf_fe* T_prev, const vdf_fe* u1, vdf_fe* Az2, vdf_fe* Bz2, vdf_fe* Cz2,
                                      vdf_fe* T);
/* acc[i] <- acc[i] + r * add[i], i < k <= 8, n[i] elements each: k vdf_axpy calls with a common r (host
 * memory).  The fold of a relaxed witness is k = 2 (W, E); a prover that keeps A z, B z, C z of the running
 * instance folds them too (they are linear in z), k = 5, instead of recomputing three sparse products. */
int  vdf_fold_many(vdf_ctx* ctx, int field, const vdf_fe* r, int k, vdf_fe* const acc[], const vdf_fe* const add[],
                   const size_t n[]);
/* Stream order across contexts of one device: work enqueued on `ctx` after this call starts only after
 * everything enqueued on `other` so far has finished (an event; the host does not wait). */
int  vdf_ctx_wait(vdf_ctx* ctx, vdf_ctx* other);
/* Marks: vdf_ctx_mark remembers the current end of the context's queue under `slot` (0 .. VDF_MARK_SLOTS-1: 0..3 are the
 * caller's on ANY context; 4..15 are used by libvdf_nova.so on the contexts it is given -- prove_step 4..7, compress 8 --
 * and never 0..3 there); vdf_ctx_sync_mark
 * blocks the host until everything enqueued before that mark has finished, while later work keeps running.  A
 * prover that looks one step ahead waits for this step's commitment without waiting for the next step's. */
#define VDF_MARK_SLOTS 16
int  vdf_ctx_mark(vdf_ctx* ctx, int slot);
int  vdf_ctx_sync_mark(vdf_ctx* ctx, int slot);
/* ... and vdf_ctx_wait_mark makes work enqueued on `ctx` from now on start only after `other`'s mark `slot` has been
 * reached -- not after whatever `other` was given since (vdf_ctx_wait would wait for that too). */
int  vdf_ctx_wait_mark(vdf_ctx* ctx, vdf_ctx* other, int slot);
/* One-shot scheduling hint for the NEXT bucket-method MSM enqueued on `ctx`: its sort runs as usual, its bucket
 * accumulation -- the one kernel of the pipeline that fills every SIMD -- starts only after `other`'s mark `slot` has
 * been reached.  A prover that commits ahead on a side queue keeps that accumulation out of the way of a short,
 * latency-critical kernel on its main queue (measured: a 10^4-term direct sum takes 190 us beside an accumulation and
 * 110 us alone).  Results are unchanged; an MSM that takes the direct-sum path ignores the hint. */
int  vdf_ctx_gate_accumulate(vdf_ctx* ctx, vdf_ctx* other, int slot);
/* Wave priority (0..3, default 3) of the latency-bound kernels of this context's bucket-method MSMs -- the sort and the
 * bucket reduction; the bucket accumulation always runs at 0 and a direct sum at 2.  A prover that commits on several
 * queues gives the queue whose result it needs LAST a lower priority than the one on its longest dependent path
 * (libvdf_nova.so: the lookahead's MSM at 1, the early rows' at 3).  Scheduling only: results are unchanged. */
int  vdf_ctx_set_light_priority(vdf_ctx* ctx, int priority);

/* ---- compression SNARK building blocks ------------------------------------------------------ */
/* The passes behind `NovaVDFProof::compress` and the verification of a compressed proof
 * (/root/reference/src/nova/proof.rs:360-368, :383 -> nova-snark 0.8.0 CompressedSNARK: sum-checks over the relaxed
 * R1CS and inner-product-argument openings).  Protocol and padding are restated in
 * oracle/spartan.py.  Vectors live in device memory, single field elements in host memory (passed as kernel
 * arguments); multilinear tables are MSB-first: index i = sum x_j 2^(k-j), binding a variable folds the upper half
 * of a table onto the lower half. */
/* out[i] = prod_j (bit_j(i) ? hi[j] : lo[j]), i < 2^k, k <= 24: eq(r, .) with lo = 1 - r, hi = r; the inner-product
 * argument's generator coefficients with lo = x^-1, hi = x. */
int  vdf_pair_table(vdf_ctx* ctx, int field, const vdf_fe* lo, const vdf_fe* hi, int k, vdf_fe* out);
/* out[i] = (prod_j (bit_j(i >> log_m) ? hi[j] : lo[j])) * pattern[i mod 2^log_m], i < 2^(k + log_m), log_m <= 4: the table over
 * the top k index bits times a vector of 2^log_m values over the low bits (host memory) -- the generator coefficients of an
 * inner-product argument that stopped at a vector of 2^log_m elements instead of halving down to one. */
int  vdf_pair_table_pattern(vdf_ctx* ctx, int field, const vdf_fe* lo, const vdf_fe* hi, int k, const vdf_fe* pattern, int log_m,
                            vdf_fe* out);
/* One opening of an inner-product argument as its verifier's final check sees it: a weight, the k round factors
 * (lo = x^-1, hi = x of round j) and the final vector of 2^log_m elements; every element host memory, Montgomery form;
 * k + log_m <= 24, log_m <= 4. */
typedef struct vdf_ipa_opening {
  vdf_fe weight;
  int k, log_m;
  const vdf_fe* lo;
  const vdf_fe* hi;
  const vdf_fe* pattern;
} vdf_ipa_opening;
/* out[i] = sum over the openings q with i < 2^(k_q + log_m_q) of
 *            weight_q * pattern_q[i mod 2^log_m_q] * prod_j (bit (k_q-1-j) of (i >> log_m_q) ? hi_q[j] : lo_q[j]),   i < n,
 * zero past every opening: the generator coefficients of a random linear combination of many openings' checks (one MSM over
 * the generators for all of them); count = 1 with weight 1 is vdf_pair_table_pattern.  The openings' factors travel to the
 * device in one copy per call; out (device, n elements) is ready for vdf_msm(..., is_mont = 1). */
int  vdf_ipa_coefficients(vdf_ctx* ctx, int field, const vdf_ipa_opening* ops, int count, size_t n, vdf_fe* out);
/* v[t][i] <- c_lo[t] * v[t][i] + c_hi[t] * v[t][i + n/2], i < n/2, for t < k <= 8 vectors of length n (power of two)
 * in one launch: a sum-check binding (1 - r, r); the argument's folds (x, x^-1) / (x^-1, x). */
int  vdf_fold_halves(vdf_ctx* ctx, int field, int k, vdf_fe* const v[], const vdf_fe c_lo[], const vdf_fe c_hi[], size_t n);
/* Sums over a vector pair / the five tables of the R1CS sum-check; `out` host, pinned or device:
 *   kind 0  out[0] = sum_i a[i] b[i], i < n                                    tables = {a, b}
 *   kind 1  g(0), g(2) of g(t) = sum_{i < n/2} p_t[i] q_t[i]                    tables = {p, q}
 *   kind 2  g(0), g(2), g(3) of g(t) = sum eq_t (a_t b_t - u c_t - e_t)        tables = {eq, a, b, c, e}, u: host
 *   kind 3  sum a[i] b[n/2 + i],  sum a[n/2 + i] b[i]                          tables = {a, b}
 * with f_t[i] = f[i] + t (f[n/2 + i] - f[i]). */
enum { VDF_REDUCE_DOT = 0, VDF_REDUCE_QUADRATIC_ROUND = 1, VDF_REDUCE_R1CS_ROUND = 2, VDF_REDUCE_IPA_CROSS = 3 };
int  vdf_reduce(vdf_ctx* ctx, int field, int kind, const vdf_fe* const tables[], const vdf_fe* u, size_t n, vdf_fe* out);
/* out[y] = sum_x eq[x] (A + rho B + rho^2 C)[x, y] for the num_cols columns of the shape (eq: num_cons elements). */
int  vdf_spmv3_t(vdf_ctx* ctx, const vdf_shape* shape, const vdf_fe* eq, const vdf_fe* rho, vdf_fe* out);
/* The same passes for many instances of one length at once (the lockstep rounds of vdf_nova_compress_batch); the
 * instances' pointers and factors travel to the device in one copy per call.  Field sums are exact, so every result equals
 * that of the single call bit for bit.
 * vdf_reduce_batch: `count` (<= 512) reductions of one kind over tables of length n; tables = count x (5 for kind 2, else
 * 2) device pointers, instance by instance; u = count host elements for kind 2 (else ignored, may be NULL); out = count x
 * nout elements (host, pinned or device), nout = 1, 2, 3, 2 for kinds 0..3.  Two launches in all. */
int  vdf_reduce_batch(vdf_ctx* ctx, int field, int kind, size_t count, const vdf_fe* const tables[], const vdf_fe* u, size_t n,
                      vdf_fe* out);
/* vdf_fold_halves for up to 320 vectors of one length n, each with its own c_lo[t], c_hi[t] (host); one launch. */
int  vdf_fold_halves_batch(vdf_ctx* ctx, int field, int k, vdf_fe* const v[], const vdf_fe c_lo[], const vdf_fe c_hi[], size_t n);
/* vdf_spmv3_t for `count` instances (eq[q], rho[q] -> out[q]) over one shape: the column structure is read once per
 * launch of up to four instances. */
int  vdf_spmv3_t_batch(vdf_ctx* ctx, const vdf_shape* shape, size_t count, const vdf_fe* const eq[], const vdf_fe rho[],
                       vdf_fe* const out[]);
/* Random linear combinations of many instances (vdf_nova_verify_batch), one pass each.
 * out[i] = sum_j w[j] * v[j][i] for i < n_out, v[j][i] = 0 for i >= n[j] (n[j] <= n_out); w[j] canonical integers below 2^128
 * (limbs 2 and 3 zero, else VDF_ERR_BAD_ARG); v, out device memory (out may be one of the v[j]); count 1..64.  v Montgomery
 * gives out Montgomery, ready for vdf_msm(..., is_mont = 1). */
int  vdf_lincomb_u128(vdf_ctx* ctx, int field, int count, const vdf_fe* const v[], const size_t n[], const vdf_fe w[],
                      size_t n_out, vdf_fe* out);
/* out[r] = sum_q rho[q] * ((A z_q)[r] * (B z_q)[r] - u[q] * (C z_q)[r] - E_q[r]) for every row r of `shape`; E[q] == NULL is
 * the zero vector (E == NULL: all are); u Montgomery (host), rho canonical below 2^128 (host; limbs 2 and 3 zero, else
 * VDF_ERR_BAD_ARG); z, E, out device memory; count 1..64.  The rows are read once for all instances. */
int  vdf_relaxed_residual_batch(vdf_ctx* ctx, const vdf_shape* shape, int count, const vdf_fe* const z[], const vdf_fe* const E[],
                                const vdf_fe u[], const vdf_fe rho[], vdf_fe* out);
/* Many points of the shape's polynomial in one pass over its rows (vdf_nova_verify_compressed_batch: every proof's M(r_x, r_y)):
 * out[q] = sum over the entries (x, y, v) of A, B, C of  eq_x[q][x] * w_q(matrix) * v * eq_y[q][ycol(y)],
 * w_q = 1, rho[q], rho[q]^2;  ycol(y) = y for y < col_split, else col_hi_base + (y - col_split).
 * eq_x[q]: nx >= num_cons elements, eq_y[q]: ny elements (device, Montgomery); rho Montgomery (host);
 * out: count elements in HOST memory (Montgomery); count 0..VDF_SPARSE_EVAL_MAX (64).  The rows are read
 * once per launch for all instances of that launch.  Synchronises once, whether the context is asynchronous or not.
 * The vectors need not be eq tables: they are arbitrary field vectors to the kernel.  With eq_x[q] = eq(r_x, .) and
 * eq_y[q] = eq(r_y, .) the result equals vdf_pair_table -> vdf_spmv3_t -> vdf_reduce(VDF_REDUCE_DOT) for the same point,
 * limb for limb, without the transposed product and without the M vector.
 * VDF_ERR_BAD_ARG, before anything is launched: a null pointer with count > 0, count above the cap, nx < num_cons,
 * col_split > num_cols, col_split > ny, col_hi_base + (num_cols - col_split) > ny.  count == 0 is VDF_OK and writes nothing. */
#define VDF_SPARSE_EVAL_MAX 64
int  vdf_sparse_eval_multi(vdf_ctx* ctx, const vdf_shape* shape, int count, const vdf_fe* const eq_x[], size_t nx,
                           const vdf_fe* const eq_y[], size_t ny, const vdf_fe rho[], size_t col_split, size_t col_hi_base,
                           vdf_fe* out);
/* One round of the inner-product argument without materialising folded generators: with n_j the current length of
 * a, s[t] the coefficient of original generator t in its folded generator, h = n_j / 2 and r = t mod n_j,
 *   sL[t] = r >= h ? s[t] a[r - h] : 0,   sR[t] = r < h ? s[t] a[r + h] : 0,   t < n,
 * so that L = MSM(sL) and R = MSM(sR) over the original generators. */
int  vdf_ipa_scalars(vdf_ctx* ctx, int field, const vdf_fe* a, const vdf_fe* s, size_t n, size_t nj, vdf_fe* sL, vdf_fe* sR);
/* s[t] *= (t mod n_j) >= n_j / 2 ? x_hi : x_lo, t < n. */
int  vdf_scale_pattern(vdf_ctx* ctx, int field, vdf_fe* s, size_t n, size_t nj, const vdf_fe* x_lo, const vdf_fe* x_hi);

/* ---- utilities the host layer and the tests need ---------------------------------------- */
/* Element-wise Montgomery product / conversions, n elements (test + host plumbing). */
int  vdf_fe_mul(vdf_ctx* ctx, int field, const vdf_fe* a, const vdf_fe* b, size_t n, vdf_fe* out);
int  vdf_fe_to_mont(vdf_ctx* ctx, int field, const vdf_fe* a, size_t n, vdf_fe* out);
int  vdf_fe_from_mont(vdf_ctx* ctx, int field, const vdf_fe* a, size_t n, vdf_fe* out);
/* Element-wise square root, n elements (Montgomery in and out): out[i] is the root of a[i] whose canonical value is even
 * (the convention of the generator families) and ok[i] = 1; for a non-residue ok[i] = 0 and out[i] = 0.  a = 0 has the
 * root 0.  Tonelli-Shanks with every trip count fixed (both fields have 2-adicity 32): every lane runs the same number of
 * products whatever its element.  Each array in host or device memory.  The root of vdf_points_decompress as a primitive of
 * its own, so that every 2-adic depth can be tested: a random element reaches depth k with probability 2^(k-32). */
int  vdf_fe_sqrt(vdf_ctx* ctx, int field, const vdf_fe* a, size_t n, vdf_fe* out, uint8_t* ok);
/* n points from the wire's 32-byte encoding (vdf_nova.h: x little-endian, the parity of y in bit 255, 32 zero bytes the
 * identity), one lane per point: ok[i] = 1 and out[i] = the point in Montgomery form, byte for byte what
 * vdf_nova_point_decompress writes, exactly when that call returns VDF_OK for the 32 bytes; otherwise (x >= m after masking
 * bit 255, zero bytes with the parity bit set, x^3 + 5 a non-residue) ok[i] = 0 and out[i] is zeroed.  The 32 zero bytes give
 * the identity (0, 0) with ok[i] = 1.  enc: n x 32 bytes, no alignment asked; out: n points; ok: n bytes; each of the three in
 * host or device memory (vdf_ptr_is_device).  The bytes are a peer's: no loop of the kernel depends on them.  n = 0 is VDF_OK
 * and touches nothing. */
int  vdf_points_decompress(vdf_ctx* ctx, int curve, const uint8_t* enc, size_t n, vdf_affine* out, uint8_t* ok);
/* out[i] = a[i] + s[i] * b[i] on `curve`, one lane per entry: the per-entry folds of a verifier that holds many statements
 * (vdf_nova_verify_aggregate_device).  a, b, out: affine points in Montgomery form, the identity (0, 0); s[i]: a PLAIN
 * little-endian integer (not Montgomery form).  bits = 128 or 255 (anything else: VDF_ERR_BAD_ARG) is how many of its low bits
 * count: bits of s[i] at and above `bits` are MASKED -- never read -- so the call computes a[i] + (s[i] mod 2^bits) * b[i]; a
 * scalar at or above the group order is not reduced first (the result is the same point).  out[i] is canonical affine
 * Montgomery form, byte for byte the host's pt_to_aff(pt_add(a, pt_mul(b, s, bits))); every exceptional case of the group law
 * is handled (either operand the identity, a = -s b, a = s b, a = b).  The points are not checked to lie on the curve
 * (vdf_bases_validate, vdf_points_decompress do that).  The operands are a peer's: every lane runs `bits` doublings and
 * `bits` additions, a scalar's bit only selects.  Each array in host or device memory (vdf_ptr_is_device), device arrays
 * 16-byte aligned, `out` not overlapping an input.  n = 0 is VDF_OK and touches nothing; a null pointer with n > 0 is
 * VDF_ERR_BAD_ARG. */
int  vdf_points_axpy(vdf_ctx* ctx, int curve, const vdf_affine* a, const vdf_affine* b, const vdf_fe* s, int bits, size_t n,
                     vdf_affine* out);
/* The random oracle of the folding layer on the device (family 0, the default block of vdf_nova.h: Poseidon2 of width 4,
 * rate 3, x^5, 8 external and 56 internal rounds), one lane per message: the per-entry hashes of a verifier that holds many
 * statements (vdf_nova_verify_aggregate_device under vdf_nova_pp_set_verify_ro_device).  n messages of `len` elements each,
 * message-major (xs[i * len + j]), canonical Montgomery form.  rc: the field's VDF_RO_CONSTANTS round constants in Montgomery
 * form, ext[r][lane] for r = 0..7 (lane-minor) and then in[0..55] -- what vdf_nova_ro_constants writes.  out[i] is
 * vdf_nova_ro_hash(field, tag, xs + i * len, len): the state starts as (tag + (len << 32), 0, 0, 0), each block of three
 * elements (the last one possibly short) is added into lanes 1..3 and followed by one permutation, the result is lane 1;
 * len = 0 permutes nothing and gives 0.  bits = 0 writes that element in Montgomery form; bits in 1..255 writes the low `bits`
 * bits of its canonical integer as a PLAIN little-endian 256-bit integer (the state hash at 250, the fold challenge at 128);
 * any other value is VDF_ERR_BAD_ARG, as are an unknown field and len > VDF_RO_HASH_MAX_LEN.  The messages are a peer's: no
 * loop, branch or address of the kernel depends on them.  Each array in host or device memory (vdf_ptr_is_device), device
 * arrays 16-byte aligned (otherwise VDF_ERR_BAD_ARG), `out` not overlapping an input.  n = 0 is VDF_OK and touches nothing; a
 * null pointer with n > 0 is VDF_ERR_BAD_ARG (xs may be null when len = 0).  This call is family 0 only; a family-1 block
 * (the dense matrix of width up to 25) runs through vdf_ro_hash_batch_block below.  vdf_nova_ro_hash_batch_eval is the host
 * restatement. */
#define VDF_RO_CONSTANTS  88          /* 8 external rounds x 4 lanes, then 56 internal */
#define VDF_RO_HASH_MAX_LEN 1024
int  vdf_ro_hash_batch(vdf_ctx* ctx, int field, uint64_t tag, const vdf_fe* rc, const vdf_fe* xs, size_t len, size_t n, int bits,
                       vdf_fe* out);
/* The same oracle under a family-1 block of vdf_nova.h (the original Poseidon permutation: `width` elements, x^5 on every
 * element in the first and last full_rounds / 2 rounds and on element 0 in the partial_rounds between, a dense width x width
 * matrix after every round; the sponge's rate is width - 1), one message per 32 lanes: lane i of a group holds state element
 * i, and the matrix product goes through LDS.  rc: (full_rounds + partial_rounds) * width round constants, round-major and
 * lane-minor; mds: width * width elements, row-major; both in Montgomery form -- what vdf_nova_ro_block_constants writes.
 * out[i] is vdf_nova_ro_hash_ro(block, field, tag, xs + i * len, len): the state starts as (tag + (len << 32), 0, ..), each
 * block of width - 1 elements (the last one possibly short) is added into elements 1..width - 1 and followed by one
 * permutation, the result is element 1; len = 0 permutes nothing and gives 0.  xs, len, n, bits and out as above, and every
 * rule above carries over.  Refusals, in this order, each VDF_ERR_BAD_ARG: an unknown field; width outside
 * 2..VDF_RO_BLOCK_MAX_WIDTH; full_rounds odd or outside 2..VDF_RO_BLOCK_MAX_FULL; partial_rounds outside
 * 0..VDF_RO_BLOCK_MAX_PARTIAL; bits outside 0..255; len > VDF_RO_HASH_MAX_LEN; then n = 0 is VDF_OK and touches nothing; a null
 * rc, mds or out, or a null xs with len > 0; a device array that is not 16-byte aligned.  No loop, branch or address of the
 * kernel depends on a message.  vdf_nova_ro_hash_batch_eval_ro is the host restatement. */
#define VDF_RO_BLOCK_MAX_WIDTH   25
#define VDF_RO_BLOCK_MAX_FULL    16
#define VDF_RO_BLOCK_MAX_PARTIAL 128
int  vdf_ro_hash_batch_block(vdf_ctx* ctx, int field, uint64_t tag, int width, int full_rounds, int partial_rounds,
                             const vdf_fe* rc, const vdf_fe* mds, const vdf_fe* xs, size_t len, size_t n, int bits, vdf_fe* out);
/* Throughput probe: each of n lanes runs `iters` dependent Montgomery multiplications
 * (roofline / issue-rate calibration for DESIGN.md; not on the prove path). */
int  vdf_fe_mul_chain(vdf_ctx* ctx, int field, const vdf_fe* a, size_t n, int iters, vdf_fe* out);
/* Process-wide tuning of the kernels (every field has a measured default; DESIGN.md says what each was worth).  The
 * environment variables of earlier rounds (VDF_MSM_*, VDF_NIFS_LANES, VDF_SHIM_CACHE) are read ONCE, the first time the
 * library needs a value, as overrides of these defaults; a host sets them here instead.  Values are read at launch time.
 * Thread-safe: a set publishes a new immutable snapshot; a call running on another thread meanwhile sees the old values or
 * the new ones at each of its launches, never a mixture within one read (set before a call for a defined outcome). */
typedef struct vdf_hip_tuning {
  uint32_t struct_size;        /* sizeof(vdf_hip_tuning) as the caller compiled it */
  int32_t msm_direct;          /* 1: MSMs inside a digit table's ranges are direct sums (msm_direct.hip); 0: bucket method only */
  int32_t direct_priority;     /* wave priority of the direct sum, 0..3 (2) */
  int32_t direct_fused;        /* 1: the direct sum's last workgroup adds the workgroup points; 0: a second launch does */
  int32_t light_priority;      /* ceiling of the wave priority of sort / fix-up / bucket-reduction kernels, 0..3 (3);
                                  a context lowers its own with vdf_ctx_set_light_priority */
  int32_t accumulate_fill;     /* resident bucket-accumulation workgroups per CU one launch is sized for, 1..3; 0 (the default) =
                                  automatic: three for a single MSM of 2^22 (scalar, window) entries or more, two below and for batches; a context overrides it with
                                  vdf_ctx_set_accumulate_fill */
  int32_t accumulate_lds;      /* bytes of unused LDS per accumulation workgroup: caps its occupancy per CU (0) */
  int32_t slice_len;           /* fixed slice length of the bucket accumulation, 1..65536; 0 = from the entry count */
  int32_t part_bits;           /* high bucket bits of the sort's first pass; -1 = about one partition per CU */
  int32_t reduction;           /* 1: bucket reduction as a matrix (k_red_sums / weights / combine); 0: segments */
  int32_t reduction_quads;     /* quads of the segment reduction, 64..65536; 0 = 8192 */
  int32_t heavy_min;           /* a bucket spanning more slices than max(this, 2 x average + 4) goes to a wavefront; 0 = 6 */
  int32_t giant_span;          /* ... and more than this to several wavefronts; 0 = 64 */
  int32_t nifs_lanes;          /* lanes per row of the fused cross term: 1, 4, 8; 0 = 8 up to 2^15 rows, else 1 */
  int32_t shim_cache;          /* generator arrays the mult_pippenger shims keep resident, 0..64 (0; vdf_shim_set_cache) */
  int32_t nifs_fused;          /* 1: rows of more than 8 entries are summed inside the cross term's launch (k_nifs_cross_f) when it
                                  runs eight lanes per row; 0: by a launch of their own before it (1) */
  int32_t fold_u128;           /* 1: vdf_fold_many with a scalar below 2^128 (every NIFS fold challenge) multiplies by its plain value
                                  without a Montgomery reduction (fe_mul_u128); 0: the general multiplication (1) */
  int32_t fixup_serial;        /* 1: the slice heads of a bucket are added by ONE lane (k_fixup_serial: 2.4 x fewer instructions per
                                  addition, a longer dependent chain; 1); 0: by a quad of lanes (k_fixup) */
  int32_t sort_staged;         /* 1: the sort's second pass lays a tile of entries out bucket by bucket in LDS and writes whole
                                  runs (k_fine_staged); 0: every entry written on its own (k_fine) */
  int32_t glv;                 /* 1: a table-less MSM over a whole generator set of 2^12 points or more uses the curve's endomorphism
                                  (2n points, 129-bit half-scalars: half the Horner chain); 0: never */
} vdf_hip_tuning;
int  vdf_hip_tuning_get(vdf_hip_tuning* out);            /* the values in force (struct_size filled in) */
int  vdf_hip_tuning_set(const vdf_hip_tuning* in);       /* VDF_ERR_BAD_ARG (nothing changed) if a field is out of range */
/* Per context: how many resident accumulation workgroups per CU its bucket-method MSMs fill (1..3; 0 = the process-wide
 * value).  A prover's side queues fill all three (their launches share the device with other queues' kernels, and a
 * grid sized for two is packed three-and-one by the dispatcher); independent MSMs in flight do better with two. */
int  vdf_ctx_set_accumulate_fill(vdf_ctx* ctx, int workgroups_per_cu);
/* Box fingerprint: every SIMD runs `iters` dependent Montgomery products (two wavefronts per SIMD, ~0.85 us per
 * iteration: 6000 iterations = 5 ms); *shader_mhz = shader clocks / 100 MHz reference ticks summed over the wavefronts
 * (the clock the device sustained under the MSM's kind of load), *kernel_ms = the launch's duration (HIP events).
 * Synchronises the context's stream.  Either output may be NULL. */
int  vdf_ctx_clock_probe(vdf_ctx* ctx, int iters, double* shader_mhz, double* kernel_ms);
/* Device memory helpers so a non-torch host (the C++ Nova layer) can keep state resident. */
int  vdf_dev_alloc(vdf_ctx* ctx, size_t bytes, void** out);
int  vdf_dev_free(vdf_ctx* ctx, void* p);
int  vdf_dev_mem_info(vdf_ctx* ctx, size_t* free_bytes, size_t* total_bytes);   /* HBM of the context's device; either may be NULL */
int  vdf_dev_memcpy(vdf_ctx* ctx, void* dst, const void* src, size_t bytes);   /* any direction */
/* A blocking copy to host memory without a context, for a holder of a device pointer that has none (the runtime finds the
 * pointer's device).  src must be complete: what a context's queue is still writing needs that context's vdf_ctx_sync first.
 * An error's text is vdf_last_error(NULL). */
int  vdf_ptr_download(void* dst, const void* src, size_t bytes);
/* Pinned host memory mapped into the device's address space.  Calls treat such a pointer like device memory
 * (used in place, no staging, no implicit synchronisation): a kernel's small result -- an MSM's point -- lands
 * in host memory by itself and is readable after vdf_ctx_sync, with no device-to-host copy. */
int  vdf_host_alloc(vdf_ctx* ctx, size_t bytes, void** out);
int  vdf_host_free(vdf_ctx* ctx, void* p);
int  vdf_dev_memset(vdf_ctx* ctx, void* dst, int value, size_t bytes);
/* Library build identification ("vdf_hip gfx950 <date>"). */
const char* vdf_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VDF_HIP_H */
