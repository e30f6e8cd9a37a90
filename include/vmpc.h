/* vmpc.h - C-ABI of the MI355X-native AC20 hot path (libvmpc_hip.so).
 *
 * The reference (toonsegers/verifiable_mpc) is pure Python and has NO FFI of its own:
 * its seam is the Python functions of verifiable_mpc/ac20/pivot.py and
 * compressed_pivot.py and the MPyC group-element operators they use.
 * Each entry point below names the reference call site whose work it takes over; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and implemented in
 * verifiable_mpc_amd/_native.py.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / Python types;
 *  - scalars: 32 bytes little-endian, canonical residue < l (l = Ed25519 group order);
 *  - affine points: 64 bytes x||y little-endian, canonical residues < p = 2^255-19;
 *  - projective points: 96 bytes X||Y||Z (representative preserved, see ge25519.h);
 *  - extended points: 128 bytes X||Y||Z||T;
 *  - every function returns 0 on success or a negative VMPC_E_* code; the library never
 *    retains host pointers past a call and never draws randomness (the reference draws
 *    r, rho and generator exponents in Python: compressed_pivot.py:105-106,
 *    circuit_sat_r1cs.py:64,81);
 *  - *_dev functions take DEVICE pointers, enqueue on the context's stream and return
 *    without synchronising unless stated; buffers may come from vmpc_malloc or from any
 *    other HIP allocator (e.g. torch tensors' data_ptr()).
 *  - one context per host thread / GPU; no global mutable state besides the HIP runtime.
 */
#ifndef VMPC_H
#define VMPC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VMPC_OK 0
#define VMPC_E_INVAL (-22)      /* bad length / null pointer / bad flag */
#define VMPC_E_NONCANON (-34)   /* scalar >= l or coordinate >= p */
#define VMPC_E_NOTONCURVE (-33) /* affine point does not satisfy the curve equation */
#define VMPC_E_NOMEM (-12)
#define VMPC_E_HIP (-5)         /* HIP runtime error, see vmpc_last_error() */
#define VMPC_E_NODEV (-19)      /* no GPU visible */
#define VMPC_E_RANGE (-75)      /* a length above what the entry supports (it states its cap); nothing was written */
#define VMPC_E_AGAIN (-11)      /* vmpc_ctx_sync: a commitment took the fused short path (16-row table of <= 2^17 columns)
                                 * and its scalars were skewed beyond that path's fixed capacities (e.g. a witness of
                                 * mostly small values: > ~24 K non-zero digits in one bin); nothing of the call's
                                 * output is valid - switch the path off (vmpc_ctx_set_short_path) and repeat the call.
                                 * The context then skips the short path for its next 64 eligible calls by itself. */

#define VMPC_SCALAR_BYTES 32
#define VMPC_AFFINE_BYTES 64
#define VMPC_PROJ_BYTES 96
#define VMPC_EXT_BYTES 128

typedef struct vmpc_ctx vmpc_ctx;

/* ---- runtime ------------------------------------------------------------------- */
/* number of visible GPUs (or VMPC_E_*); writes "gfx950 MI355X ..." style text */
int vmpc_backend_info(char *buf, size_t buflen);
const char *vmpc_last_error(void);
int vmpc_ctx_create(int device, vmpc_ctx **out);
int vmpc_ctx_destroy(vmpc_ctx *ctx);
/* run on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int vmpc_ctx_set_stream(vmpc_ctx *ctx, void *hip_stream);
int vmpc_ctx_sync(vmpc_ctx *ctx);
/* Commitments over a 16-row fixed-base table of at most 2^17 columns (BASELINE config 2, every prover round after the
 * fold jump) take a fused three-launch path (csrc/msm_short.hip) with fixed capacities; on: the default.  A call whose
 * scalars overflow them is reported by vmpc_ctx_sync as VMPC_E_AGAIN: switch the path off, repeat, switch it on.
 * on = 2: on, and the 64-call back-off that follows an overflow is cleared. */
int vmpc_ctx_set_short_path(vmpc_ctx *ctx, int on);
int vmpc_ctx_get_short_path(vmpc_ctx *ctx, int *on);       /* the current setting (callers that switch it off for a call restore THIS) */
/* test hook: mark the context as holding a queued stream wait (vmpc_p4_run_compact's state between two rounds) -
 * every call that would have to grow the workspace or the pinned block must then fail with VMPC_E_INVAL instead of
 * synchronising a stream that waits on the calling thread */
int vmpc_ctx_debug_hold_wait(vmpc_ctx *ctx, int on);
/* test hooks: enqueue a kernel that keeps a stream busy for about `microseconds` and touches no memory (one 64-lane
 * workgroup, one lane polling the 100-MHz constant-rate counter with s_sleep between polls, and a bound on the number
 * of polls - 4 per requested microsecond + 64, each under 2048 shader clocks - that ends it even if the counter
 * stands still).  Work enqueued behind it stays pending while the host enqueues its consumer on another stream: the
 * cross-stream ordering tests (tests/stream_order_cases.py) delay a producer or a consumer with it.  The first form
 * delays the context's stream, the second any stream of `device` (a vmpc_stream_create bucket stream).
 * microseconds > 20000: VMPC_E_RANGE, nothing is launched; 0: VMPC_OK, nothing is launched.  Not for production
 * paths: nothing in the library calls them. */
int vmpc_ctx_debug_delay(vmpc_ctx *ctx, unsigned microseconds);
int vmpc_stream_debug_delay(void *hip_stream, int device, unsigned microseconds);
/* test hooks for the rule that a call's result is a function of its arguments, never of what the scratch arena held
 * (tests/arena_cases.py, DESIGN.md "Arena independence").  Not for production paths: nothing in the library calls them.
 * vmpc_ctx_debug_arena_fill: enqueue a fill of the whole arena with the 32-bit `word` on the context's stream, and of the
 *   prover's pool kept between proofs when no vmpc_p4 holds it.  No arena yet: VMPC_OK, nothing enqueued.  word > 0xFFFF:
 *   VMPC_E_RANGE, nothing enqueued - the values are small on purpose, so that a kernel which trusts a stale count or
 *   index computes a wrong answer and not an address far outside its buffers.  While the context holds a queued stream
 *   wait (vmpc_ctx_debug_hold_wait, a prover round between begin and end): VMPC_E_INVAL, nothing enqueued.
 * vmpc_ctx_debug_arena_info: the arena's size, the bytes the last call that reserved it took from it (0: it reserved and
 *   took nothing), and how many times the arena has been (re)allocated so far (any of the three may be NULL).
 * vmpc_ctx_debug_rearmed: synchronises the stream; *ok = 1 when every cursor word of the fused short path is zero (what
 *   the path's last kernel leaves, csrc/common.h) or when the path was never set up on this context, else 0. */
#define VMPC_DEBUG_ARENA_FILL_MAX 0xFFFFu
int vmpc_ctx_debug_arena_fill(vmpc_ctx *ctx, uint32_t word);
int vmpc_ctx_debug_arena_info(vmpc_ctx *ctx, size_t *bytes, size_t *used, uint64_t *generation);
int vmpc_ctx_debug_rearmed(vmpc_ctx *ctx, int *ok);
/* non-blocking: *done = 1 when everything enqueued on the context's stream has completed (a driver that keeps
 * several commitments in flight refills whichever context finishes first) */
int vmpc_ctx_query(vmpc_ctx *ctx, int *done);
/* make `waiter`'s stream wait (on the device, no host block) for everything enqueued so far on
 * `other`'s stream: lets two contexts run independent MSMs (A_i and B_i of one Protocol-4
 * round, compressed_pivot.py:41-42) concurrently */
int vmpc_ctx_wait_for(vmpc_ctx *waiter, vmpc_ctx *other);
int vmpc_malloc(vmpc_ctx *ctx, size_t bytes, void **dptr);
int vmpc_free(vmpc_ctx *ctx, void *dptr);
int vmpc_memcpy_h2d(vmpc_ctx *ctx, void *dst, const void *src, size_t bytes); /* synchronous */
int vmpc_memcpy_d2h(vmpc_ctx *ctx, void *dst, const void *src, size_t bytes); /* synchronous */
int vmpc_memcpy_d2d(vmpc_ctx *ctx, void *dst, const void *src, size_t bytes); /* async */
/* per-stage HIP-event timing of the MSM pipeline (bench.py roofline leg) */
int vmpc_ctx_profile(vmpc_ctx *ctx, int enable);
/* sums since the last reset; names is a ';'-separated list matching ms[] */
int vmpc_ctx_profile_read(vmpc_ctx *ctx, char *names, size_t names_len, double *ms,
                          uint64_t *launches, int max_stages, int reset);
/* Phase pipelining of a stream of commitments (pivot.py:139-145 called proof after proof): the contexts of a pipeline
 * share ONE bucket stream (vmpc_stream_create; priority < 0 = lowest).  Every commitment's bucket stage is then
 * enqueued there - bucket kernels run one at a time, back to back, as persistent launches of `wgs_per_cu` 256-lane
 * workgroups per CU (0 = the whole grid) that leave register-file room on every SIMD - while the sort of the next
 * commitment and the reduction / recombination of the previous one run beside it on the contexts' own streams.
 * Ordering is by events on the device; results and vmpc_ctx_sync behave as before.  NULL = off. */
int vmpc_stream_create(int device, int priority, void **out_hip_stream);
int vmpc_stream_destroy(void *hip_stream);
int vmpc_ctx_set_bucket_stream(vmpc_ctx *ctx, void *hip_stream, int wgs_per_cu);
/* Pippenger window width override (0 = automatic); for tuning / tests */
int vmpc_ctx_set_window(vmpc_ctx *ctx, int c_bits);
/* the window width and window count the planner uses for an n-term Ed25519 MSM */
int vmpc_ed25519_msm_plan(vmpc_ctx *ctx, size_t n, int *c_bits, int *windows);
/* Read-only view of the sort front end (csrc/msm_sort.hip) of the LAST MSM call on this context, for tests: the plan
 * and the device addresses of the arrays the sort and the segment planning left in the context's workspace.  The
 * workspace is reset at the start of every call that uses it, so the arrays are valid from the moment the MSM call
 * has completed (the caller synchronises first) until the next such call; nothing after the sort writes them (the
 * bucket, finish, reduce and recombination kernels read them only).  A batched BN-256 table MSM leaves the view of its
 * one shared pass.  VMPC_E_INVAL when no sort has run since the workspace was last reset - in particular when the
 * last call took the fused short path, which does not use this stage.  Host side only: no launch, no device access.
 * Element types: digits int16 (int32 when `wide`) [W][n_pad]; tasks uint32[4] records, ctrl[1] of them (<= t_max);
 * every other array uint32: hist1[hist1_n + 1], counts / starts / nseg / seg_starts / heavy_list [W * nb1],
 * sorted[hist1[hist1_n]], ctrl[16 + 64 * W]. */
typedef struct vmpc_sort_view {
    uint64_t n_total, n_pad, row_stride, hist1_n, t_max;
    uint32_t top_max_b;
    int32_t c, W, nb, nb1, period, top_row, LB, LB_top, NC, J, idx_bits, fine_in_entry, fine_cap, seg_shift, balanced,
        wide, chunks_per_row;
    const void *digits, *hist1, *counts, *starts, *sorted, *nseg, *seg_starts, *heavy_list, *tasks, *ctrl;
} vmpc_sort_view;
int vmpc_msm_sort_view(vmpc_ctx *ctx, vmpc_sort_view *out);
/* Integer-ALU ceiling of the bucket stage (bench.py roofline leg): mixed additions per second of
 * a register-resident chain on every lane of the chip - the bucket kernel without memory. */
int vmpc_ed25519_madd_rate(vmpc_ctx *ctx, int iters, double *madds_per_second);

/* Calibration probe for the HBM-traffic counters (profiles/, bench.py roofline.traffic): n_gathers reads of one
 * 128-byte line each from a device table of table_lines lines, in the bucket stage's access pattern (one lane per
 * line, eight 16-byte loads).  mode 0: lines at random (hash of the gather index and seed); 1: consecutive lanes
 * read consecutive lines; 2: the same bytes as a wide coalesced stream (16 B per lane).  Known bytes read:
 * 128 * n_gathers.  ms (may be NULL): duration of the launch (synchronises). */
int vmpc_gather_probe_dev(vmpc_ctx *ctx, const void *table, size_t table_lines, size_t n_gathers, int mode,
                          uint32_t seed, double *ms);

/* ---- host-buffer one-shots (SURVEY.md 8b proposal) -------------------------------- */
/* h^gamma-less MSM: out = sum scalars[i] * points[i].
 * Replaces the list comprehension + reduce of pivot.vector_commitment,
 * verifiable_mpc/ac20/pivot.py:143-144 (called from circuit_sat_cb.py:103 and
 * compressed_pivot.py:41,42,110,193). */
int vmpc_ed25519_msm(const uint8_t *scalars, const uint8_t *points, size_t n, uint8_t out[64]);
/* out[i] = c * pts_l[i] + pts_r[i]: the generator fold of
 * verifiable_mpc/ac20/compressed_pivot.py:64 (prover) and :178 (verifier). */
int vmpc_ed25519_fold(const uint8_t *pts_l, const uint8_t *pts_r, const uint8_t c[32],
                      size_t half, uint8_t *out);
/* out[i] = scalars[i] * base: generator setup g_i = h ** r_i,
 * verifiable_mpc/ac20/circuit_sat_r1cs.py:64-70,81. */
int vmpc_ed25519_fixed_base_batch(const uint8_t base[64], const uint8_t *scalars, size_t n,
                                  uint8_t *out);
/* out[i] = c * x[i] + y[i] mod l: z' = z_l + c z_r and L' = c L_l + L_r,
 * verifiable_mpc/ac20/compressed_pivot.py:70-76; z = c0 x + r, :134. */
int vmpc_fr_axpy(const uint8_t c[32], const uint8_t *x, const uint8_t *y, size_t n, uint8_t *out);
/* out = sum a[i] * b[i] mod l: LinearForm evaluation, verifiable_mpc/ac20/pivot.py:84-92. */
int vmpc_fr_dot(const uint8_t *a, const uint8_t *b, size_t n, uint8_t out[32]);

/* ---- device-resident entry points ---------------------------------------------------- */
/* canonical-encoding + on-curve check of n affine points; *n_bad = number of offenders (sync) */
int vmpc_points_validate_dev(vmpc_ctx *ctx, const void *affine, size_t n, uint64_t *n_bad);

/* Pedersen vector commitment as one MSM over n + n_extra terms
 * (pivot.py:139-145: the extra term is h ** gamma).  Any of out_ext / out_affine may be
 * NULL.  Scalars must be canonical (checked on device, reported at the next sync point
 * through vmpc_ctx_sync -> VMPC_E_NONCANON). */
int vmpc_msm_dev(vmpc_ctx *ctx, const void *scalars, const void *affine_points, size_t n,
                 const void *extra_scalars, const void *extra_affine_points, size_t n_extra,
                 void *out_ext, void *out_affine);

/* Fixed-base tables for a generator vector that serves many commitments: the CRS of
 * pivot.py:139-145 (g, h, k are fixed between proofs: circuit_sat_r1cs.py:47-93 creates them once).
 * The table holds rows 2^(256 rho / rows) * P_i, rho = 0..rows-1, rows in {1, 2, 4, 8, 16}, for the n
 * points followed by the n_extra extra points (rows * 128 bytes per point, rows padded to a multiple
 * of 8 points: vmpc_msm_table_bytes).  A commitment over a table needs no point preparation and only
 * (16/rows - 1) * 16 doublings of window recombination (none for rows = 16); its result equals
 * vmpc_msm_dev's on the same points and scalars (as a group element; compared after normalisation).
 * rows = 13 is the WIDE-WINDOW table (round 6): rows 2^(20 rho) * P_i, rho = 0..12, row stride a multiple of 8192
 * points (n + n_extra <= 2^22 - 8192).  A commitment over it is 13 mixed additions per term - the scalar's thirteen signed
 * 20-bit digits, one set of 2^19 buckets - instead of 16, with no recombination at all: the fastest form for the
 * commitments of pivot.py:139-145 from 2^19 generators up (0.98 ms alone at 2^20; 1.66 GB).  Accepted by
 * vmpc_msm_table_dev / _batch_dev and vmpc_p4_set_commit_table; the fold entry points and vmpc_p4_create need one of the
 * other row counts (their kernels read rows spaced 256 / rows bits). */
int vmpc_msm_table_bytes(size_t n, size_t n_extra, int rows, size_t *bytes);
int vmpc_msm_table_build_dev(vmpc_ctx *ctx, const void *affine_points, size_t n,
                             const void *extra_affine_points, size_t n_extra, int rows, void *table);
/* out = sum_{i<m} scalars[i] * P_i + sum_{e<table_extra} extra_scalars[e] * E_e over the table built
 * from (P_0..P_{table_n-1}, E_0..E_{table_extra-1}); m <= table_n; extra_scalars may be NULL (zeros). */
int vmpc_msm_table_dev(vmpc_ctx *ctx, const void *table, size_t table_n, size_t table_extra, int rows,
                       const void *scalars, size_t m, const void *extra_scalars, void *out_ext,
                       void *out_affine);
/* `batch` commitments over the same table in one pass (A_i and B_i of a round, compressed_pivot.py:41-42; or
 * independent commitments a prover has queued): scalars[k] / extra_scalars[k] are DEVICE pointers held in HOST
 * arrays of `batch` entries (extra_scalars may be NULL, or hold NULL entries); outputs are consecutive
 * (128 bytes / 64 bytes per commitment).  Same results as `batch` calls of vmpc_msm_table_dev; the bucket
 * reduction and the window recombination - latency chains - run once for the whole batch.  batch <= 16. */
int vmpc_msm_table_batch_dev(vmpc_ctx *ctx, const void *table, size_t table_n, size_t table_extra, int rows,
                             const void *const *scalars, size_t m, const void *const *extra_scalars, int batch,
                             void *out_ext, void *out_affine);

/* sum of m extended points in index order, normalised (multi-GPU combine of the per-rank
 * partial commitments; also A * Q^c * B^(c^2) style products once the powers are points) */
int vmpc_points_sum_dev(vmpc_ctx *ctx, const void *ext_points, size_t m, void *out_ext,
                        void *out_affine);
/* k such sums at once: point i of sum j at ext_points + 128 * (i * k + j) - the layout an all-gather of
 * k partial points per rank produces (A_i and B_i of a round: k = 2); outputs consecutive */
int vmpc_points_sum_many_dev(vmpc_ctx *ctx, const void *ext_points, size_t m, size_t k, void *out_ext,
                             void *out_affine);

/* ---- the multi-GPU exchange step (kernel row "allgather_add_points") ------------------------------
 * One process per GPU.  A commitment over generators that are sharded over G ranks (pivot.py:143-144 is a sum of
 * independent terms) is G partial sums plus ONE exchange: an all-gather of the 128-byte partial points and, on
 * every rank, their sum in rank order - the same bits on all ranks, so Fiat-Shamir challenges need no broadcast.
 * Transports: RCCL (ncclAllGather on the context's stream, xGMI inside a node; librccl is dlopen'ed on first use,
 * there is no link-time dependency), or a caller-supplied callback (host-staged gloo in the tests, any other
 * fabric), or none for world = 1. */
typedef struct vmpc_comm vmpc_comm;
#define VMPC_COMM_ID_BYTES 128
/* rank 0 draws the id (ncclGetUniqueId) and hands it to every rank over any side channel */
int vmpc_comm_unique_id(uint8_t out[VMPC_COMM_ID_BYTES]);
/* collective: every rank calls it with the same id (ncclCommInitRank on ctx's device) */
int vmpc_comm_create_rccl(vmpc_ctx *ctx, const uint8_t unique_id[VMPC_COMM_ID_BYTES], int world, int rank,
                          vmpc_comm **out);
/* the caller moves the bytes: fn(user, mine, gathered, bytes_per_rank) is called with DEVICE pointers after the
 * context's stream has been synchronised, must fill gathered[r * bytes_per_rank ..] with rank r's `mine` for every r
 * and return 0.  fn = NULL is allowed for world = 1 (the gather is a device copy). */
typedef int (*vmpc_exchange_fn)(void *user, const void *mine, void *gathered, size_t bytes_per_rank);
int vmpc_comm_create_callback(int world, int rank, vmpc_exchange_fn fn, void *user, vmpc_comm **out);
int vmpc_comm_destroy(vmpc_comm *comm);
/* kind: 0 = self (world 1), 1 = RCCL, 2 = callback.  For an RCCL communicator world / rank are what RCCL itself
 * reports (ncclCommCount / ncclCommUserRank), not the values passed at creation. */
int vmpc_comm_info(const vmpc_comm *comm, int *world, int *rank, int *kind);
/* gathered (world x bytes_per_rank, device) = every rank's `mine`, in rank order; enqueued on ctx's stream */
int vmpc_comm_allgather_dev(vmpc_comm *comm, vmpc_ctx *ctx, const void *mine, void *gathered, size_t bytes_per_rank);
/* k commitments at once: mine_ext = this rank's k partial points (128 B each, device); gathered_scratch = world x k x
 * 128 bytes of device scratch; out_ext / out_affine (either may be NULL) = the k rank-ordered sums, as
 * vmpc_points_sum_many_dev writes them.  No host synchronisation with the RCCL transport. */
int vmpc_comm_points_allsum_dev(vmpc_comm *comm, vmpc_ctx *ctx, const void *mine_ext, size_t k,
                                void *gathered_scratch, void *out_ext, void *out_affine);

/* element-wise `base_i ** n_i` replaying the reference's operation sequence (ge25519.h):
 * bases are projective (96 B) or, with bases_affine != 0, affine (64 B, Z = 1); a single
 * base is broadcast when n_bases == 1.  signed_scalars = 1 applies the reference's
 * pivot._int convention (pivot.py:119-128): residues above l/2 act as negative exponents;
 * signed_scalars = 2 takes exponents in sign-magnitude form (|n| < 2^255, bit 255 = sign) for
 * callers that hold the reference's Python ints, which need not be residues (pivot.py:143).
 * Outputs: projective representatives (may be NULL) and/or affine (may be NULL). */
int vmpc_repeat_dev(vmpc_ctx *ctx, const void *bases, size_t n_bases, int bases_affine,
                    const void *scalars, size_t n, int signed_scalars, void *out_proj,
                    void *out_affine);

/* out_i = scalars[i] * base as AFFINE points (64 B each), for callers that need the group elements of
 * `h ** r_i` (circuit_sat_r1cs.py:64-70,81) but not the reference's projective representatives: a
 * comb table of the one base replaces the per-element ladder (6x less work than vmpc_repeat_dev).
 * Scalars canonical (< l; checked on device, reported at the next sync point). */
int vmpc_fixed_base_dev(vmpc_ctx *ctx, const void *base_affine, const void *scalars, size_t n,
                        void *out_affine);

/* g'_i = (g_l[i] ** c) * g_r[i], compressed_pivot.py:64/:178, replayed exactly.
 * in_affine != 0: inputs are 64-byte affine points (Z = 1), else 96-byte projective. */
int vmpc_fold_dev(vmpc_ctx *ctx, const void *g_l, const void *g_r, int in_affine,
                  const uint8_t c[32], size_t half, void *out_proj, void *out_affine);

/* pivot.list_mul (pivot.py:26-28): balanced pairwise product tree of n projective points
 * in the reference's order, optional identity appended at the end; `points` is clobbered. */
int vmpc_tree_reduce_dev(vmpc_ctx *ctx, void *proj_points, size_t n, int append_identity,
                         void *out_proj);

/* .normalize() for a whole vector (compressed_pivot.py:52,118): projective -> affine */
int vmpc_normalize_dev(vmpc_ctx *ctx, const void *proj, size_t n, void *out_affine);
/* affine (x, y) -> projective (x, y, 1) */
int vmpc_affine_to_proj_dev(vmpc_ctx *ctx, const void *affine, size_t n, void *out_proj);

/* The GF(l) vector entries from here to vmpc_fr_dot_to_dev (csrc/frvec.hip): out = c * x + y, c * x, <a, b>, the
 * challenge products and the tail scalars.  Every element of a VECTOR operand (x, y, a, b, z, and `products` from the
 * second round on) must be a canonical residue < l.  Unlike the host constants (c, tail, the challenges: checked,
 * VMPC_E_NONCANON) the vectors are NOT checked, and unlike the Pi_Nullity entries below they are not reduced on the way
 * in: an element is loaded as it is, and a sum is corrected by one subtraction of l only.  With a non-canonical element
 * the result is unspecified (no fault, no error code, possibly a non-canonical or a wrong residue).  Results of
 * canonical operands are canonical. */
int vmpc_fr_axpy_dev(vmpc_ctx *ctx, const uint8_t c[32], const void *x, const void *y, size_t n,
                     void *out);
int vmpc_fr_scale_dev(vmpc_ctx *ctx, const uint8_t c[32], const void *x, size_t n, void *out);
/* out[0..n) = c * x + y (y == NULL: c * x), out[n] = tail: z_hat = (c0 * x + r) || phi and L~ = c1 * (L || 0)
 * (compressed_pivot.py:134-141) in one pass each, without a copy to append the scalar.  c, tail: canonical
 * residues (VMPC_E_NONCANON otherwise); out: n + 1 elements. */
int vmpc_fr_axpy_tail_dev(vmpc_ctx *ctx, const uint8_t c[32], const void *x, const void *y, size_t n,
                          const uint8_t tail[32], void *out);
/* out[j] = z[j mod 2^low_bits] * prod_{i < rounds} (c_i if bit (low_bits+rounds-1-i) of j is 0
 * else 1), n = 2^(rounds+low_bits) <= 2^40, rounds <= 20; challenges = rounds x 32 bytes (host).
 * These are the coefficients of `rounds` applications of the fold of compressed_pivot.py:64
 * written as one linear map, so that the verifier's final check (compressed_pivot.py:193) becomes
 * a single N-term MSM over the original generators (used by the compact transcript only). */
int vmpc_fr_challenge_products_dev(vmpc_ctx *ctx, const uint8_t *challenges, int rounds, int low_bits,
                                   const void *z, size_t n, void *out);
/* Scalars of A_i / B_i (compressed_pivot.py:41-42) expressed over a base vector of 2^log2_m0
 * generators to which the last t folds (challenges c_0..c_{t-1}, host, 32 B each) have not been
 * applied; z is the current witness of 2^(log2_m0 - t) scalars.  out_a / out_b: 2^log2_m0 scalars. */
int vmpc_fr_tail_scalars_dev(vmpc_ctx *ctx, const uint8_t *challenges, int t, int log2_m0,
                             const void *z, void *out_a, void *out_b);
/* The same scalars round by round: `products` (2^log2_m0 scalars) carries the challenge products from
 * the call with t - 1 to the call with t (t = 0 initialises it) and only the newest challenge
 * c_{t-1} is passed: two products per element and round instead of up to t + 1. */
int vmpc_fr_tail_scalars_inc_dev(vmpc_ctx *ctx, const uint8_t newest_challenge[32], int t, int log2_m0,
                                 const void *z, void *products, void *out_a, void *out_b);
/* the same for positions j0 .. j0 + count - 1 only; products / out_a / out_b hold `count` elements (one rank's
 * block of g_hat in the sharded prover: scalar work proportional to the block, not to N) */
int vmpc_fr_tail_scalars_block_dev(vmpc_ctx *ctx, const uint8_t newest_challenge[32], int t, int log2_m0,
                                   const void *z, size_t j0, size_t count, void *products, void *out_a,
                                   void *out_b);
/* synchronous: result copied to host */
int vmpc_fr_dot_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, uint8_t out[32]);
/* the same, result left in device memory (32 bytes at out_dev, asynchronous) */
int vmpc_fr_dot_to_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, void *out_dev);

/* How the reference's str(input_list) prints a curve point is recalled from MPyC, not observed:
 * the bracket pair ('[' ']' or '(' ')') and whether a coordinate c > (p - 1) / 2 prints as -(p - c).  Process-wide,
 * effective for every later formatting call, no rebuild (scripts/check_against_mpyc.py names the call to make when
 * real MPyC prints otherwise).  Scalar signedness travels with each call (is_signed below).  Defaults: '[' ']' 0. */
int vmpc_set_reference_format(char point_open, char point_close, int coord_signed);
int vmpc_get_reference_format(char *point_open, char *point_close, int *coord_signed);
/* Text of the Fiat-Shamir pre-image (pivot.py:134 str(input_list)) produced on device:
 * "item0, item1, ..., item{n-1}, " (every item followed by ", ").  Synchronous; *len gets
 * the number of bytes written, VMPC_E_NOMEM if cap is too small. */
int vmpc_format_points_dev(vmpc_ctx *ctx, const void *proj, size_t n, void *out_text, size_t cap,
                           uint64_t *len);
int vmpc_format_scalars_dev(vmpc_ctx *ctx, const void *scalars, size_t n, int is_signed,
                            void *out_text, size_t cap, uint64_t *len);
/* Asynchronous forms: text is produced into `dev_text` (cap >= n * 245 for points, n * 81 for
 * scalars) and copied, with its length, into PINNED host memory (vmpc_host_alloc) on the context's
 * stream; nothing is valid until that stream has been synchronised (vmpc_ctx_sync). */
int vmpc_format_points_async_dev(vmpc_ctx *ctx, const void *proj, size_t n, void *dev_text, size_t cap,
                                 void *host_text, uint64_t *host_len);
int vmpc_format_scalars_async_dev(vmpc_ctx *ctx, const void *scalars, size_t n, int is_signed,
                                  void *dev_text, size_t cap, void *host_text, uint64_t *host_len);
/* The same with the text delivered in pieces of chunk_bytes (>= 4096): host_len is a pinned block of >= 16 bytes -
 * [0, 8) the text's length, [8, 12) the number of pieces that have landed (0 when the call is made, advanced on the
 * stream) - so that the caller can hash piece k while piece k + 1 is in flight (pivot.py:131-136 hashes ~1 GB of such
 * text per proof at N = 2^20). */
int vmpc_format_points_chunked_dev(vmpc_ctx *ctx, const void *proj, size_t n, void *dev_text, size_t cap,
                                   void *host_text, uint64_t *host_len, size_t chunk_bytes);
int vmpc_format_scalars_chunked_dev(vmpc_ctx *ctx, const void *scalars, size_t n, int is_signed, void *dev_text,
                                    size_t cap, void *host_text, uint64_t *host_len, size_t chunk_bytes);
/* page-locked host memory for the asynchronous copies above */
int vmpc_host_alloc(size_t bytes, void **out);
int vmpc_host_free(void *p);

/* out = A + c * Q + c^2 * B on the HOST, affine x || y (64 bytes) in and out, c a canonical residue: the commitment
 * fold Q' = A * Q**c * B**(c**2) of compressed_pivot.py:66 / :180, whose normalised value the reference transcript
 * hashes every round (no device, no context). */
int vmpc_ed25519_fold_commitment_host(const uint8_t A[64], const uint8_t Q[64], const uint8_t B[64],
                                      const uint8_t c[32], uint8_t out[64]);

/* out = sum_i scalars[i] * points[i] on the HOST (n <= 8; affine 64-byte points, canonical 32-byte residues): the
 * commitment Q = A * P**c0 * k**(c1 (c0 y + t)) of compressed_pivot.py:140 / :233, whose normalised value the first
 * round's pre-image contains (no device, no context). */
int vmpc_ed25519_lincomb_host(const uint8_t *points, const uint8_t *scalars, size_t n, uint8_t out[64]);

/* ---- BN-256 G1 / G2 (Pinocchio prover MSMs) ----------------------------------
 * The eight sums of verifiable_mpc/trinocchio/pynocchio.py:229-246
 *     apply_to_list(point_add, [int(c[i]) * evalkey[...] for i in qap.indices_mid])
 * on the curve of verifiable_mpc/ac20/pairing.py:44-51 (y^2 = x^3 + 3 over F_p; sextic twist over
 * F_p[i]/(i^2+1)).  Scalars: 32 B little-endian, canonical < n (the 256-bit group order).
 * G1 points: 64 B x||y canonical; G2 points: 128 B x.re||x.im||y.re||y.im; the point at infinity
 * is the all-zero encoding.  Outputs are affine. */
int vmpc_bn256_g1_msm(const uint8_t *scalars, const uint8_t *points, size_t n, uint8_t out[64]);
int vmpc_bn256_g2_msm(const uint8_t *scalars, const uint8_t *points, size_t n, uint8_t out[128]);
int vmpc_bn256_g1_msm_dev(vmpc_ctx *ctx, const void *scalars, const void *points, size_t n,
                          void *out_affine);
int vmpc_bn256_g2_msm_dev(vmpc_ctx *ctx, const void *scalars, const void *points, size_t n,
                          void *out_affine);
/* group = 1 (G1) or 2 (G2): canonical encodings and curve equation; *n_bad = offenders (sync) */
/* out_i = scalars[i] * base for one base point (group 1: 64-byte points, group 2: 128-byte): the key generation
 * of the Pinocchio prover is n such products of the two generators (pynocchio.py:101-200).  Scalars: 32-byte
 * little-endian integers below 2^256 (not reduced); affine outputs, all-zero bytes = infinity. */
int vmpc_bn256_fixed_base_dev(vmpc_ctx *ctx, int group, const void *base_affine, const void *scalars, size_t n,
                              void *out_affine);

int vmpc_bn256_validate_dev(vmpc_ctx *ctx, int group, const void *points, size_t n, uint64_t *n_bad);
/* Integer-ALU ceiling of the BN-256 bucket stage (bench.py, `alu` block of the bn256 line): Jacobian mixed
 * additions (madd-2007-bl on the Montgomery-form field; group 2: over F_p^2) per second of a register-resident
 * chain on every lane of the chip - the bucket kernel without memory. */
int vmpc_bn256_madd_rate(vmpc_ctx *ctx, int group, int iters, double *madds_per_second);
/* Fixed-base tables over an evaluation-key vector (fixed per circuit; pynocchio.py:228-246 reads the
 * same evalkey entries for every proof): 17 rows 2^(16 w) * P_i.  vmpc_bn256_table_msm_dev computes
 * sum_{i<m} scalars[i] * P_i, equal to vmpc_bn256_g{1,2}_msm_dev on the first m points. */
int vmpc_bn256_table_bytes(int group, size_t n, size_t *bytes);
int vmpc_bn256_table_build_dev(vmpc_ctx *ctx, int group, const void *points, size_t n, void *table);
/* out_affine (64 / 128 B) and / or out_jacobian (canonical X || Y || Z, 96 / 192 B; Z = 0 is the
 * point at infinity) - the Jacobian form skips the inversion chain that one lane would run */
int vmpc_bn256_table_msm_dev(vmpc_ctx *ctx, int group, const void *table, size_t table_n,
                             const void *scalars, size_t m, void *out_affine, void *out_jacobian);
/* n_tables (<= 16) prepared keys of the SAME length table_n, ONE scalar vector: out_jacobian[k] (96 / 192 B each,
 * consecutive) = sum_{i<m} scalars[i] * P_k[i].  The shape of trinocchio/pynocchio.py:229-246, where the sums
 * r_v*v_mid*g1, r_y*y_mid*g1, r_v*alpha_v*v_mid*g1, ... all run over c_mid: recoding, bucket sort and plan happen once,
 * every table gets its own bucket launch over the one sorted index list, the bucket sets are reduced and finished
 * together.  A column that holds the point at infinity (all-zero entry) in table k contributes nothing to sum k, so
 * sums that differ in a few trailing terms (the zero-knowledge deltas) still share every scalar. */
int vmpc_bn256_table_msm_multi_dev(vmpc_ctx *ctx, int group, const void *const *tables, int n_tables, size_t table_n,
                                   const void *scalars, size_t m, void *out_jacobian);
/* ONE prepared key, `rows` scalar vectors: out_affine[r] (64 / 128 B each, consecutive; all-zero bytes = infinity) =
 * sum_{i<m} scalars[r * row_stride + i] * P_i.  The shape of a batch of knowledge-of-exponent verifications
 * (ac20/knowledge_of_exponent.py:136-153: R = sum_j L[n-1-j] pp_rhs[j], one linear form per proof over one pp).
 * Scalars are read as vmpc_bn256_table_msm_dev reads them; row_stride is counted in scalars and is >= m.  Rows go in
 * groups of at most 16: each row has its own recoding and sort, a group shares one launch of the bucket stage (the row on
 * the grid's y axis), one bucket reduction and one recombination launch.  No arena: `scratch` is the caller's device
 * memory of at least vmpc_bn256_table_msm_rows_scratch_bytes(group, table_n, rows) bytes (sized for one group, so the
 * same for every rows >= 16; 0: an argument out of range), not read, and free again when the stream has passed the
 * call.  m == 0: every output is infinity; rows == 0: nothing is written.  m > table_n, row_stride < m, a NULL pointer
 * or too small a scratch_bytes: VMPC_E_INVAL before any launch.  Asynchronous. */
size_t vmpc_bn256_table_msm_rows_scratch_bytes(int group, size_t table_n, size_t rows);
int vmpc_bn256_table_msm_rows_dev(vmpc_ctx *ctx, int group, const void *table, size_t table_n, const void *scalars,
                                  size_t row_stride, size_t m, size_t rows, void *scratch, size_t scratch_bytes,
                                  void *out_affine);

/* ---- BN-256 optimal-ate pairing (verifiable_mpc/ac20/pairing.py:614-643; the Pinocchio verifier, trinocchio/
 * pynocchio.py:276-325) -------------------------------------------------------------------------------------------
 * g1: G1 affine points, 64 B each; g2: twist affine points, 128 B each (x.re, x.im, y.re, y.im); canonical LE, the
 * all-zero encoding is the point at infinity - the formats of vmpc_bn256_*_msm.  Points are NOT validated here
 * (vmpc_bn256_validate_dev does that); a point at infinity on either side gives 1.
 * GT element: 12 canonical 32-byte LE residues, 384 B, in the order of the reference's tower
 *     f = x w + y in Fp6[w]/(w^2 - tau), x = x.x tau^2 + x.y tau + x.z in Fp2[tau]/(tau^3 - xi), xi = i + 3:
 *     x.x.re, x.x.im, x.y.re, x.y.im, x.z.re, x.z.im, y.x.re, y.x.im, y.y.re, y.y.im, y.z.re, y.z.im
 * (1 is y.z.re = 1, every other residue 0).  The value is the reference's pynocchio.pairing(a, b) = optimal_ate(b, a)
 * coefficient for coefficient. */
/* gt_out[j] = e(g1[j], g2[j]), j < n */
int vmpc_bn256_pairing_dev(vmpc_ctx *ctx, const void *g1, const void *g2, size_t n, void *gt_out);
/* for k < n_products: prod_{offsets[k] <= j < offsets[k+1]} e(g1[j], g2[j]) over n_pairs pairs, ONE final
 * exponentiation per product; is_one[k] = (product == 1) (1 / 0), gt_out[k] the product (either may be NULL, not
 * both).  offsets: n_products + 1 device words; an empty range is the product 1; a range outside [0, n_pairs] is
 * not computed and reports is_one 0 and an all-zero gt_out entry.  Device buffers; nothing is synchronised. */
int vmpc_bn256_pairing_product_dev(vmpc_ctx *ctx, const void *g1, const void *g2, size_t n_pairs,
                                   const uint32_t *offsets, size_t n_products, uint8_t *is_one, void *gt_out);
/* out[b] = s (sum_{i < n_bases} scalars[b][i] bases[i] + sum_{j < n_row_points} row_points[b][j]) for b < batch,
 * s = -1 if negate else 1: the verifier's IO sums (few bases, many rows), with the proof's own points added as
 * terms of coefficient 1.  group 1 (64-byte points) or 2 (128-byte); scalars: batch x n_bases 32-byte LE integers
 * (< 2^256, not reduced); row_points: batch x n_row_points points; out: batch affine points.  Points are not
 * validated (vmpc_bn256_validate_dev). */
int vmpc_bn256_lincomb_batch_dev(vmpc_ctx *ctx, int group, const void *bases, size_t n_bases, const void *scalars,
                                 const void *row_points, size_t n_row_points, size_t batch, int negate, void *out);
/* host-buffer one-shots of the three above (own context; lincomb validates its points: VMPC_E_NOTONCURVE) */
int vmpc_bn256_pairing(const uint8_t *g1, const uint8_t *g2, size_t n, uint8_t *gt_out);
int vmpc_bn256_pairing_product(const uint8_t *g1, const uint8_t *g2, size_t n_pairs, const uint32_t *offsets,
                               size_t n_products, uint8_t *is_one, uint8_t *gt_out);
int vmpc_bn256_lincomb_batch(int group, const uint8_t *bases, size_t n_bases, const uint8_t *scalars,
                             const uint8_t *row_points, size_t n_row_points, size_t batch, int negate, uint8_t *out);

/* ---- GF(n) for the BN-256 group order n: the scalar side of the knowledge-of-exponent pivot (AC20 section 9,
 * verifiable_mpc/ac20/knowledge_of_exponent.py) ------------------------------------------------------------------
 * Scalars: 32 bytes little-endian.  INPUTS may be any 32-byte value (they are reduced mod n when they are loaded);
 * outputs are canonical residues < n. */
/* out[k] = sum_{i + j = k} a[i] * b[j] mod n for k < na + nb - 1: the product of two coefficient vectors, the
 * prover's c_poly = c_poly_lhs * c_poly_rhs of knowledge_of_exponent.py:121-123 (verifiable_mpc/tools/qap_creator.py
 * Poly.__mul__, O(n^2) Python).  na, nb >= 1.  Cap: na and nb at most VMPC_BN256_FR_POLY_MAX each; above it the
 * entry answers VMPC_E_RANGE before it looks at any pointer and writes nothing.  `out` must not overlap a or b.
 * Uses the context arena (partial sums of a large product).  It is vmpc_bn256_fr_poly_mul_batch_dev's window
 * [0, na + nb - 1) of one product: one kernel, one planner (csrc/bn256_koe.hip). */
#define VMPC_BN256_FR_POLY_MAX ((size_t)1 << 20)
int vmpc_bn256_fr_poly_mul_dev(vmpc_ctx *ctx, const void *a, size_t na, const void *b, size_t nb, void *out);
/* host-buffer form of the above (own context, synchronous) */
int vmpc_bn256_fr_poly_mul(const uint8_t *a, size_t na, const uint8_t *b, size_t nb, uint8_t *out);
/* n_wit products of one shape in one launch sequence: out_w[k - k_lo] = (a_w * b_w)[k] for k in the WINDOW
 * [k_lo, k_lo + k_cnt) (k_lo + k_cnt <= na + nb - 1), row w of a / b / out at a_stride / b_stride / out_stride scalars
 * (a_stride >= na, out_stride >= k_cnt; b_stride >= nb, or 0: ONE b for all products).  Only the tiles of 256 outputs that
 * meet the window are launched and only the window's k_cnt scalars of a row are written - the batched h asks for the
 * halves P[0 .. d-2] and Q[d-1 .. 2d-2] of its two d x d products.  The segment length is chosen with n_wit counted (a
 * large batch: fewer, longer segments); canonical residues, so the bits do not depend on the segmentation.
 * n_wit <= VMPC_BN256_QAP_MAX_WIT (the product index is a grid dimension), na and nb within the cap
 * above, strides <= 2^31, else VMPC_E_RANGE before any pointer is looked at; n_wit = 0 or k_cnt = 0: VMPC_OK, no launch.
 * Arena: vmpc_bn256_fr_poly_mul_batch_bytes(...), reserved before the first launch (0: the product needs none). */
#define VMPC_BN256_QAP_MAX_WIT ((size_t)65535)
int vmpc_bn256_fr_poly_mul_batch_dev(vmpc_ctx *ctx, const void *a, size_t a_stride, size_t na, const void *b,
                                     size_t b_stride, size_t nb, size_t k_lo, size_t k_cnt, void *out, size_t out_stride,
                                     size_t n_wit);
size_t vmpc_bn256_fr_poly_mul_batch_bytes(size_t na, size_t nb, size_t k_lo, size_t k_cnt, size_t n_wit);
/* The same products in O(d log d), by an NTT over the INTEGERS (csrc/bn256_ntt.hip; GF(n) itself has none): the
 * coefficients - any 32-byte values, not reduced first - are convolved modulo 18 primes c 2^22 + 1 < 2^31, the exact
 * integer coefficient (< 2^20 2^512 < the primes' product) is rebuilt by Garner's digits and reduced mod n.  The three
 * entries take the arguments, caps and answers of the three above and write the same canonical residues, bit for bit;
 * only the window's scalars of a row are written, the transforms are whole (length: the power of two >= na + nb - 1).
 * Arena: the residues of b and of a group of a rows; n_wit is cut into groups so that it stays below 1 GiB
 * (vmpc_ctx_set_ntt_arena_cap lowers the cap: what the tests of the group boundary do; 0 restores it). */
int vmpc_bn256_fr_poly_mul_ntt_dev(vmpc_ctx *ctx, const void *a, size_t na, const void *b, size_t nb, void *out);
int vmpc_bn256_fr_poly_mul_ntt_batch_dev(vmpc_ctx *ctx, const void *a, size_t a_stride, size_t na, const void *b,
                                         size_t b_stride, size_t nb, size_t k_lo, size_t k_cnt, void *out,
                                         size_t out_stride, size_t n_wit);
size_t vmpc_bn256_fr_poly_mul_ntt_batch_bytes(size_t na, size_t nb, size_t k_lo, size_t k_cnt, size_t n_wit);
int vmpc_ctx_set_ntt_arena_cap(vmpc_ctx *ctx, size_t bytes);
/* Which product vmpc_bn256_fr_poly_mul_dev / _batch_dev - and with them every caller: h, t's coefficients, the
 * knowledge-of-exponent prover - compute with.  SCHOOLBOOK: a new context starts here.  AUTO: the NTT when
 * min(na, nb) >= VMPC_BN256_FR_NTT_MIN.  NTT: always.  Any other mode: VMPC_E_INVAL, the mode stays. */
#define VMPC_POLY_PRODUCT_SCHOOLBOOK 0
#define VMPC_POLY_PRODUCT_AUTO 1
#define VMPC_POLY_PRODUCT_NTT 2
/* the smallest power of two at which the NTT's median was below the schoolbook's for a square product (DESIGN.md
 * section 25) */
#define VMPC_BN256_FR_NTT_MIN ((size_t)2)
/* transforms of up to this many points run in one workgroup's LDS; longer ones in two or three passes */
#define VMPC_BN256_FR_NTT_LDS_LEN 2048
int vmpc_ctx_set_poly_product(vmpc_ctx *ctx, int mode);
int vmpc_ctx_get_poly_product(vmpc_ctx *ctx, int *mode);
/* out[i] = scale * z^(i+1) mod n for i < count (z, scale: one 32-byte device scalar each): the exponents of the
 * trusted setup, which knowledge_of_exponent.py:52-66 reaches by 2n sequential `g1_base ** z` / `g2_base ** z` on the
 * points themselves; here the 2n points are vmpc_bn256_fixed_base_dev of these exponents. */
int vmpc_bn256_fr_powers_dev(vmpc_ctx *ctx, const void *z, const void *scale, size_t count, void *out);
/* out = c * x + y (y NULL: c * x) and <a, b> left in device memory, mod n: vmpc_fr_axpy_dev and vmpc_fr_dot_to_dev over
 * this field, the same kernels (csrc/frvec.hip).  c: a canonical residue, else VMPC_E_NONCANON; the vectors any 32-byte
 * values.  The dot product's partial sums go to `scratch`, the caller's device memory of
 * vmpc_bn256_fr_dot_scratch_bytes(n) bytes, not to the arena.  n = 0: out_dev = 0. */
int vmpc_bn256_fr_axpy_dev(vmpc_ctx *ctx, const uint8_t c[32], const void *x, const void *y, size_t n, void *out);
size_t vmpc_bn256_fr_dot_scratch_bytes(size_t n);
int vmpc_bn256_fr_dot_to_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, void *out_dev, void *scratch);
/* The operands of the opening's product from device memory (knowledge_of_exponent.py:116-123):
 * lhs = (gamma, x_0, .., x_{n-1}) (n + 1 scalars) and rhs = (L_{n-1}, .., L_0) (n scalars).  lhs or rhs may be NULL
 * (the verifier reverses L only; gamma and x are then not read).  gamma >= n: VMPC_E_NONCANON.
 * n < VMPC_BN256_FR_POLY_MAX, else VMPC_E_RANGE.  No arena. */
int vmpc_bn256_koe_stage_dev(vmpc_ctx *ctx, const void *x, const uint8_t gamma[32], const void *L, size_t n, void *lhs,
                             void *rhs);
/* After the product c (2n scalars): u_out (one device scalar) = c[n] = <L, x>, and c[n] = 0, so that c is the scalar
 * vector of Q's MSM over the 2n generators (knowledge_of_exponent.py:124-130).  n >= 1.  No arena. */
int vmpc_bn256_koe_split_dev(vmpc_ctx *ctx, void *c, size_t n, void *u_out);
/* vmpc_bn256_koe_stage_dev for n_wit openings of one length n in ONE launch (the witness on the grid's y): for every p,
 * lhs_p = (gammas[p], x_p[0..n-1]) and rhs_p = (L_p[n-1], .., L_p[0]), row p of x, L, lhs, rhs being p times its stride
 * (in scalars) past the pointer.  gammas: n_wit device scalars, uploaded as canonical residues.  x NULL: no lhs is
 * written (gammas and lhs are not read); L NULL: no rhs; both NULL: VMPC_E_INVAL.  n < VMPC_BN256_FR_POLY_MAX,
 * n_wit <= VMPC_BN256_QAP_MAX_WIT, every stride <= 2^31 and, for n_wit > 0, lhs_stride >= n + 1 and the others >= n - of
 * all four, whichever sides are asked for - else VMPC_E_RANGE before any pointer is looked at.  n_wit = 0: VMPC_OK, no
 * launch.  The bits are those of n_wit single calls.  No arena. */
int vmpc_bn256_koe_stage_batch_dev(vmpc_ctx *ctx, const void *x, size_t x_stride, const void *gammas, const void *L,
                                   size_t L_stride, size_t n, size_t n_wit, void *lhs, size_t lhs_stride, void *rhs,
                                   size_t rhs_stride);
/* vmpc_bn256_koe_split_dev for n_wit products, rows of 2n scalars c_stride >= 2n scalars apart, in one launch with a
 * lane per row: u_out[p] = c_p[n] (n_wit device scalars), then c_p[n] = 0; nothing else is written.  n >= 1; caps as
 * above, else VMPC_E_RANGE; n_wit = 0: VMPC_OK, no launch.  No arena. */
int vmpc_bn256_koe_split_batch_dev(vmpc_ctx *ctx, void *c, size_t c_stride, size_t n, size_t n_wit, void *u_out);

/* ---- Pinocchio key generation (verifiable_mpc/trinocchio/pynocchio.py:101-200): the exponents of the key points,
 * same scalar conventions.  Every key entry is (exponent) * g1 or g2, made by vmpc_bn256_fixed_base_dev. */
/* ell_out[j-1] = l_j(s) for j = 1..d, the Lagrange basis of the points 1..d at s (the reference's QAP interpolates
 * constraint j at x = j, qap_creator.r1cs_to_qap_ff), and t_out = t(s) = prod_{j=1..d} (s - j).  Exact for every s,
 * s in {1..d} (l_j = [j = s], t = 0) and s = 0 included.  d >= 1; cap VMPC_BN256_QAP_MAX_D: above it the entry answers
 * VMPC_E_RANGE before it looks at any pointer.  Uses the context arena (3 (d + 1) scalars). */
#define VMPC_BN256_QAP_MAX_D ((size_t)1 << 22)
int vmpc_bn256_qap_lagrange_dev(vmpc_ctx *ctx, const void *s, size_t d, void *ell_out, void *t_out);
/* out[c] = sum over the entries e of column c of vals[e] * basis[rows[e]]: the values v_i(s), w_i(s), y_i(s) of a
 * sparse R1CS (basis = l(s)) or of dense QAP polynomials (basis = 1, s, .., s^d).  The entries are in column order;
 * `items` holds n_items triples (start, end, dst) of uint32 that cover them: entries [start, end) sum to out[dst], or,
 * when bit 31 of dst is set, to partial sum (dst & 0x7fffffff) < n_partial.  `long_cols` holds n_long triples
 * (col, first, count): out[col] = the sum of partial sums first .. first + count - 1.  Rows >= n_basis add nothing;
 * destinations out of range are not written.  Deterministic (no atomics).  Uses the context arena (the partials).
 * One implementation with vmpc_fr_cs_colsum_dev (csrc/fr_colsum.h). */
int vmpc_bn256_qap_colsum_dev(vmpc_ctx *ctx, const void *basis, size_t n_basis, const uint32_t *rows, const void *vals,
                              size_t nnz, const uint32_t *items, size_t n_items, const uint32_t *long_cols,
                              size_t n_long, size_t n_partial, void *out, size_t n_out);
/* The exponents of the evaluation key's per-wire entries (pynocchio.py:106-154) for the wires idx[0 .. n_idx): seven
 * vectors of n_idx + 3 scalars each, consecutive in `out`, with coef = 9 scalars (r_v, r_w, r_y, alpha_v r_v,
 * alpha_w r_w, alpha_y r_y, beta r_v, beta r_w, beta r_y), vwy = v(s) || w(s) || y(s) (n_wires each) and t = t(s):
 *   r_v v_i, r_w w_i, r_y y_i, alpha_v r_v v_i, alpha_w r_w w_i, alpha_y r_y y_i, beta (r_v v_i + r_w w_i + r_y y_i).
 * The three trailing rows of each vector belong to the deltas (v, w, y): the vector's coefficient of that delta times
 * t(s) where the proof element uses it, 0 where it does not. */
int vmpc_bn256_keygen_exps_dev(vmpc_ctx *ctx, const void *coef, const void *vwy, size_t n_wires, const void *t,
                               const uint32_t *idx, size_t n_idx, void *out);

/* ---- The Pinocchio prover's h = (V W - Y) / t (verifiable_mpc/trinocchio/pynocchio.py:203-225: compute_p_poly,
 * p / qap.t, compute_h_zk_terms - quadratic Python over the dense QAP) from the row values a = V c, b = W c, y = Y c of
 * the R1CS (a_j = V(j): constraint j sits at x = j), same scalar conventions (csrc/bn256_qap_h.hip, DESIGN.md section
 * 14).  With w_j = t'(j) = (-1)^(d-j) (j-1)! (d-j)!, u_j = a_j / w_j and the moments A_k = sum_j u_j j^(k-1) (B_k from b),
 *     C_k = sum_{i=1..k-1} A_i B_(k-i) + delta_v B_k + delta_w A_k,   h_e = sum_{i=e+1..d} t_i C_(i-e) + delta_v delta_w t_e
 *                                                                            - [e = 0] delta_y      (e = 0..d).
 * Cap for all seven entries: d + 1 <= VMPC_BN256_FR_POLY_MAX; above it they answer VMPC_E_RANGE before they look at any
 * pointer.  d >= 1. */
/* out0[k] = sum_{j=1..d} u0[j-1] j^k mod n for k < n_out (n_out <= VMPC_BN256_FR_POLY_MAX), and the same for u1 -> out1
 * when u1 is not NULL (the two share the powers of j).  Replaces nothing the reference has: it stands in for the
 * interpolation of V and W (qap_creator.r1cs_to_qap_ff) and the product of pynocchio.py:203-211.  Deterministic (no
 * atomics).  Uses the context arena: at most 2 x 32 x n_out scalars (the partial sums of the ranges of j). */
int vmpc_bn256_qap_moments_dev(vmpc_ctx *ctx, const void *u0, const void *u1, size_t d, size_t n_out, void *out0,
                               void *out1);
/* ua[j-1] = a[j-1] / w_j and, when b is not NULL, ub[j-1] = b[j-1] / w_j for j = 1..d: factorial prefix products and
 * one inversion.  Uses the context arena (d + d / 64 + 4 scalars). */
int vmpc_bn256_qap_h_weights_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t d, void *ua, void *ub);
/* *first_bad (a device uint32) = the smallest i < d with a[i] * b[i] != y[i] mod n, 0xffffffff if there is none: the
 * check that the reference's demo makes on the remainder of p / qap.t.  No arena. */
int vmpc_bn256_qap_check_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t d, uint32_t *first_bad);
/* *out (ONE device scalar) = sum_{j<d} rho^j (a[j] b[j] - y[j]) mod n: the share-side replacement of the check above
 * (demos/demo_zkp_trinocchio.py:70-72 divides p by qap.t in the clear and drops the remainder; a party that holds only
 * Shamir shares of the witness has rows that never satisfy a_j b_j = y_j).  On degree-t shares of a satisfying witness
 * the M parties' results are a degree-2t sharing of 0 for every rho; a violated row makes it nonzero for all but d of
 * the rho.  rho: a canonical residue in HOST memory (VMPC_E_NONCANON otherwise).  Each lane sums its rows' unreduced
 * products, workgroup partials go through the arena (at most 64 scalars) and are added in a fixed order:
 * deterministic, no atomics. */
int vmpc_bn256_qap_residual_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t d,
                                const uint8_t rho[32], void *out);
/* out[0..d] = the coefficients of t(x) = prod_{j=1..d} (x - j), lowest first (qap_creator.r1cs_to_qap_ff builds qap.t by
 * d Poly.__mul__): leaves of 128 factors and a product tree over vmpc_bn256_fr_poly_mul_dev.  scratch: device memory
 * of 2 (d + (d + 127) / 128) scalars (not read when d <= 128).  Uses the context arena as the products do. */
int vmpc_bn256_qap_t_coeffs_dev(vmpc_ctx *ctx, size_t d, void *scratch, void *out);
/* out[p d + i] = sum_k coeffs[p n_coeffs + k] (i + 1)^k for i < d, p < n_polys (<= 65535): the values V(j), W(j), Y(j)
 * of a dense QAP's V = sum_i c_i v_i (pynocchio.py:203-209), Horner with small multipliers.  No arena. */
int vmpc_bn256_qap_horner_dev(vmpc_ctx *ctx, const void *coeffs, size_t n_coeffs, size_t n_polys, size_t d, void *out);
/* out[0..d] = h_0 .. h_d as above (pynocchio.py:212-225: p / qap.t plus compute_h_zk_terms) from the moments
 * A[i] = A_(i+1), B[i] = B_(i+1) (i < d), t's d + 1 coefficients and deltas = (delta_v, delta_w, delta_y) (NULL: all
 * zero).  scratch: device memory of 5 d scalars, of which 3 d are used.  It is vmpc_bn256_qap_h_combine_batch_dev for one
 * witness: the halves P[0 .. d-2] and Q[d-1 .. 2d-2] of two d x d products, and that entry's arena. */
int vmpc_bn256_qap_h_combine_dev(vmpc_ctx *ctx, const void *A, const void *B, const void *t, size_t d,
                                 const void *deltas, void *scratch, void *out);

/* The same stages for n_wit witnesses of ONE QAP (the batch prover): the witness is a grid dimension,
 * row w of every per-witness vector lies `stride` scalars after row w - 1 (a stride is at least the row's length and at
 * most 2^31; scalars of a row beyond its length are never written).  Each single entry above is its batch entry with
 * n_wit = 1 - one kernel and one host implementation per stage - so the bits are those of n_wit single calls.
 * n_wit <= VMPC_BN256_QAP_MAX_WIT and the cap on d as above, else VMPC_E_RANGE before any pointer is looked at; n_wit = 0:
 * VMPC_OK, no launch.  Deterministic (integer sums in a fixed order, no atomics on field values).  Where an entry uses
 * the arena it reserves it before its first launch: a batch too large for it does nothing. */
/* first_bad[w] (n_wit device words) = witness w's smallest bad row, 0xffffffff if none; a, b, y share the stride */
int vmpc_bn256_qap_check_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t stride, size_t d,
                                   uint32_t *first_bad, size_t n_wit);
/* out[w] (n_wit consecutive device scalars) = sum_{j<d} rho^j (a_w[j] b_w[j] - y_w[j]) mod n: vmpc_bn256_qap_residual_dev
 * for n_wit share vectors under ONE rho (a canonical residue in HOST memory, VMPC_E_NONCANON otherwise); a, b, y share
 * the stride.  A batch with a violated row passes for at most n_wit d of the rho.  Arena:
 * n_wit x at most 64 partials. */
int vmpc_bn256_qap_residual_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, const void *y, size_t stride, size_t d,
                                      const uint8_t rho[32], void *out, size_t n_wit);
/* the scan of the factorial prefix products and the inversion ONCE, then one launch for the n_wit rows of ua (and ub) */
int vmpc_bn256_qap_h_weights_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t d, void *ua,
                                       void *ub, size_t u_stride, size_t n_wit);
/* The moments on a grid (k segments, ranges of j, witnesses).  The number of ranges counts the witnesses:
 * 2048 / (k segments x n_wit), at most 32 and at most one per 1024 j - a large batch ends
 * at one range (one partial per k and witness).  Arena: vmpc_bn256_qap_moments_batch_bytes(d, n_out, n_wit) (0 where the
 * call would answer VMPC_E_RANGE or do nothing). */
int vmpc_bn256_qap_moments_batch_dev(vmpc_ctx *ctx, const void *u0, const void *u1, size_t u_stride, size_t d,
                                     size_t n_out, void *out0, void *out1, size_t out_stride, size_t n_wit);
size_t vmpc_bn256_qap_moments_batch_bytes(size_t d, size_t n_out, size_t n_wit);

/* ---- The same moments in O(d log^2 d): a subproduct tree over the points 1 .. d with its products through the NTT over
 * the integers, whatever the context's product mode (csrc/bn256_qap_mtree.hip).  With
 * N(x) = sum_j u_j prod_{i != j} (x - i), T(x) = prod_j (x - j), R and D their coefficients reversed (D(0) = 1),
 *     sum_{k>=0} A_(k+1) z^k = sum_j u_j / (1 - j z) = R(z) / D(z):   out[k] = (R D^-1 mod z^n_out)[k],
 * the canonical residues vmpc_bn256_qap_moments_batch_dev writes, bit for bit.
 * Geometry (csrc/qap_mtree_plan.h): L is the smallest number of levels with s = ceil(d / 2^L) <= 128 and the tree is the
 * full binary tree of 2^L leaves of s points over 1 .. d' = s 2^L; the points beyond d carry u_j = 0 and change N and T
 * by the same factor.  At the cap d <= 2^20 - 1: L <= 13 (ceil((2^20 - 1) / 2^13) = 128), so d' <= 128 x 2^13 = 2^20; a
 * level's products have at most d' + 1 <= 2^20 + 1 coefficients, a Newton step's and the final product's operands at
 * most n_max <= 2^20 each: every transform length is at most 2^21.
 * The PLAN depends on (d, n_max) alone - the T of every node, level by level, and D^-1 mod z^n_max (Newton doubling) -
 * and is built once: vmpc_bn256_qap_mtree_bytes(d, n_max) device bytes, (L + 1) d' + 2^(L+1) - 1 + 3 n_max scalars (2 n_max
 * of them the build's own; 0 where the build would answer VMPC_E_RANGE or d = 0).  126 MB at d = n_max = 2^18, 570 MB
 * at the cap.
 * A call: u1 NULL means one vector; rows as in the batch entries above (strides at least the row's length and at most
 * 2^31, scalars of a row beyond its length never written); u holds any 32-byte values; 1 <= d, n_out <= n_max with the
 * (d, n_max) the plan was built for.  VMPC_E_RANGE before any pointer is looked at when d + 1 or n_max exceeds
 * VMPC_BN256_FR_POLY_MAX, n_out > n_max (so n_out > VMPC_BN256_FR_POLY_MAX too), n_wit > VMPC_BN256_QAP_MAX_WIT or a
 * stride is out of range; n_out = 0 or n_wit = 0: VMPC_OK, no launch.  scratch: the caller's device memory of
 * vmpc_bn256_qap_moments_tree_scratch_bytes(d, n_wit) (4 d' scalars a witness).  Arena:
 * vmpc_bn256_qap_moments_tree_batch_bytes(d, n_out, n_wit), reserved before the first launch; the witnesses are cut
 * into groups that keep a level's residues within the NTT's arena cap (vmpc_ctx_set_ntt_arena_cap), which changes no
 * value.  The launches of a call depend on L and on the number of groups, not on d / s or n_wit.  Deterministic. */
size_t vmpc_bn256_qap_mtree_bytes(size_t d, size_t n_max);
int vmpc_bn256_qap_mtree_build_dev(vmpc_ctx *ctx, size_t d, size_t n_max, void *plan);
size_t vmpc_bn256_qap_moments_tree_batch_bytes(size_t d, size_t n_out, size_t n_wit);
size_t vmpc_bn256_qap_moments_tree_scratch_bytes(size_t d, size_t n_wit);
int vmpc_bn256_qap_moments_tree_batch_dev(vmpc_ctx *ctx, const void *plan, size_t d, size_t n_max, const void *u0,
                                          const void *u1, size_t u_stride, size_t n_out, void *out0, void *out1,
                                          size_t out_stride, void *scratch, size_t n_wit);
/* compute_h's threshold under device.moment_transform("auto"): the tree from this d on.  The smallest power of two at
 * which the tree's median (plan cached, two vectors, one witness) is below the direct kernel's in the same run and stays
 * below at every larger power of two measured: 0.594 ms against 1.637 ms at d = 2^10, the smallest size of the grid
 * 2^10, 2^12 .. 2^18 of profiles/moments_tree_probe.jsonl (8.57 against 673.8 at 2^18); below 2^10 nothing was
 * measured. */
#define VMPC_BN256_QAP_MTREE_MIN ((size_t)1 << 10)
/* out rows (d + 1 scalars, out_stride apart) from the moments' rows A, B (ab_stride apart), t's d + 1 coefficients (the
 * QAP's, shared) and deltas = n_wit x 3 consecutive scalars (NULL: all zero).  scratch: 3 d scalars per witness.  The two
 * products go through vmpc_bn256_fr_poly_mul_batch_dev and are asked only for what is read: P[0 .. d-2] of A * B and
 * Q[d-1 .. 2d-2] of (t_1 .. t_d) * crev, t passed as the shared b.  Arena: the larger of the two products'. */
int vmpc_bn256_qap_h_combine_batch_dev(vmpc_ctx *ctx, const void *A, const void *B, size_t ab_stride, const void *t,
                                       size_t d, const void *deltas, void *scratch, void *out, size_t out_stride,
                                       size_t n_wit);

/* ---- Pinocchio witnesses from the R1CS (the reference's QAP.calculate_witness / code_to_r1cs.assign_variables walk flat
 * code), scalars mod n ----
 * n_wit witnesses of ONE "program-shaped" R1CS from their inputs.  The plan (pynocchio.SolvePlan, all arrays in DEVICE
 * memory except level_ptr) lists the d rows in LEVEL order - the rows of level k are level_ptr[k] .. level_ptr[k+1]-1
 * and read only wires that the inputs or earlier levels define: one CSR per matrix (row_ptr of d + 1 words, col, 32-byte
 * canonical vals; the new wire's own entry left out), and per row its kind (0: a check row, a b = y; 1: the new wire
 * stands in Y, c_s = (a b - y) inv; 2: in V, c_s = (y / b - a) inv; 3: in W, c_s = (y / a - b) inv), the new wire
 * (0xffffffff for a check row) and inv, the inverse of the new wire's coefficient (32 bytes).  level_ptr_dev is the
 * device copy of level_ptr (n_levels + 1 words), which the call reads on the HOST to plan its launches.
 * c: n_wit rows of m + 1 slots, c_stride scalars apart; the caller has put the inputs into slots 1..n_in (any 32-byte
 * values).  On return slot 0 is 1 and every slot 0..m a canonical residue, the inputs' included; nothing beyond slot m
 * of a row is written.  first_bad (n_wit device words, all set to 0xffffffff by the call): the smallest level-order
 * position of a row of the witness that FAILED - a zero divisor (kinds 2, 3) or a check row with a b != y; that row is
 * the root cause, everything before it was sound.  A failed row faults nothing: it stores 0 or nothing, the call
 * completes and the witness's later slots are unspecified.  An integer minimum on that word is the only atomic; field
 * values never go through one and the result does not depend on scheduling.
 * Launches: a level of at least wide_rows rows gets a launch of its own (rows on x, witnesses on y); a maximal run of
 * consecutive narrower levels is ONE launch (a workgroup per witness walks the levels, a workgroup barrier between
 * them; nothing is synchronised between workgroups).  The call's first launch also prepares slot 0 and the inputs and
 * therefore always has the run's shape, a wide level 0 included.  wide_rows = 0: the library's rule (257 rows,
 * whatever n_wit: a level that a run's 256 lanes cannot take in one step); 1: one launch per level; SIZE_MAX: one launch.  The bits of the result are the same for every
 * wide_rows.  n_wit > VMPC_BN256_R1CS_MAX_WIT, c_stride < m + 1 or > 2^31, n_in > m: VMPC_E_RANGE before any pointer is
 * looked at; n_wit = 0 or n_levels = 0: VMPC_OK, no launch.  Runs on the context's stream, synchronises nothing.  No
 * arena. */
#define VMPC_BN256_R1CS_MAX_WIT ((size_t)65535)
int vmpc_bn256_r1cs_solve_batch_dev(vmpc_ctx *ctx, const uint32_t *v_row_ptr, const uint32_t *v_col, const void *v_vals,
                                    const uint32_t *w_row_ptr, const uint32_t *w_col, const void *w_vals,
                                    const uint32_t *y_row_ptr, const uint32_t *y_col, const void *y_vals,
                                    const uint32_t *kind, const uint32_t *wire, const void *inv,
                                    const uint32_t *level_ptr_dev, const uint32_t *level_ptr /* HOST */, size_t n_levels,
                                    size_t n_in, size_t m, void *c, size_t c_stride, size_t n_wit, size_t wide_rows,
                                    uint32_t *first_bad);
/* the number of kernel launches that call makes (host arithmetic on the level table, by the function the call itself
 * schedules with; 0 where it launches nothing) */
size_t vmpc_bn256_r1cs_solve_launches(const uint32_t *level_ptr, size_t n_levels, size_t n_wit, size_t wide_rows);

/* ---- Protocol 8 from a sparse circuit (verifiable_mpc/ac20/circuit_sat_cb.py:59-252), scalars mod l as above ------
 * m multiplication gates, M = m + 1, z = (x, f(0), g(0), h(0), h(1), .., h(2m)); f runs through (j, a_j) for j = 1..m
 * and (m + 1, r_a), g alike (circuit_sat_r1cs.py:380-388).  m <= VMPC_FR_CS_MAX_M: above it the entries answer
 * VMPC_E_RANGE before they look at any pointer.  All deterministic (integer sums in a fixed order, no atomics on
 * field values). */
#define VMPC_FR_CS_MAX_M ((size_t)1 << 20)
/* For the n_gates gates `gates[t]` (NULL: gates 0 .. n_gates-1) of one depth level: a_out[i], b_out[i] = the affine
 * forms of the left / right wire (CSR rows i of A / B: row_ptr, col, 32-byte vals, one 32-byte constant per row) at
 * (x, gamma), where column c < n_x reads z[c] and column c >= n_x reads z[gamma_offset + c - n_x]; then
 * z[gamma_offset + i] = a_i b_i (circuit_builder.py:133-151).  The caller launches the levels in order and has
 * checked that every column index is in range.  check = 1: z's gammas are the caller's, nothing is written to z, and
 * *first_bad (a device uint32) = the smallest i with a_i b_i != z[gamma_offset + i], 0xffffffff if none.  check = 2:
 * a_out, b_out only (the values of output rows: pass them as A and as B).  No arena. */
int vmpc_fr_cs_triples_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_vals,
                           const void *a_const, const uint32_t *b_row_ptr, const uint32_t *b_col, const void *b_vals,
                           const void *b_const, const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset,
                           void *z, void *a_out, void *b_out, int check, uint32_t *first_bad);
/* vmpc_fr_cs_triples_dev for n_wit witnesses of ONE circuit in one launch (the witness on the grid's y; the single entry
 * is this one with n_wit = 1).  The forms and
 * the gate list are shared; witness w reads and writes z + 32 w z_stride, a_out + 32 w ab_stride and b_out alike (strides
 * in scalars: z_stride >= the length of z, ab_stride >= the rows' count), and with check = 1 first_bad[w] (n_wit device
 * words, all set to 0xffffffff by the call) is ITS smallest bad gate.  check = 2: the values of the rows for every
 * witness, a_out and b_out may be one buffer.  n_wit <= VMPC_FR_CS_MAX_WIT, the strides <= 2^31 and not below what the
 * call itself addresses (gamma_offset + n_gates, n_gates), else VMPC_E_RANGE; n_wit = 0 or n_gates = 0: VMPC_OK and no
 * launch.  The bits are those of n_wit single calls.  No arena. */
#define VMPC_FR_CS_MAX_WIT ((size_t)65535)
int vmpc_fr_cs_triples_batch_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_vals,
                                 const void *a_const, const uint32_t *b_row_ptr, const uint32_t *b_col,
                                 const void *b_vals, const void *b_const, const uint32_t *gates, size_t n_gates,
                                 size_t n_x, size_t gamma_offset, void *z, size_t z_stride, void *a_out, void *b_out,
                                 size_t ab_stride, size_t n_wit, int check, uint32_t *first_bad);
/* fact[k] = k!, ifact[k] = 1 / k! for k = 0..K (K >= 1): two product scans and one inversion.  Arena: 2 K scalars. */
int vmpc_fr_cs_tables_dev(vmpc_ctx *ctx, size_t K, void *fact, void *ifact);
/* a, b: M scalars (a_1..a_m, r_a).  Writes z_tail[0] = f(0), [1] = g(0), [2] = h(0), [2 + m + 1] = r_a r_b and
 * [2 + x] = f(x) g(x) for x = m+2 .. 2m; z_tail[3 .. 2 + m] (the gammas) are left alone.  fact / ifact: the tables with
 * K >= 2m + 1.  Two m x m correlations with 1 / k, schoolbook with lazy reduction (circuit_sat_r1cs.py:384-386 and
 * circuit_sat_cb.py:89-90 interpolate, multiply and evaluate coefficient lists).  Arena: about (4 + 2 s) m scalars
 * for s segments of j. */
int vmpc_fr_cs_extend_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact, const void *ifact,
                          void *z_tail);
/* vmpc_fr_cs_extend_dev for n_wit witnesses in one launch sequence (the single entry is this one with n_wit = 1):
 * a, b are n_wit rows of M scalars, ab_stride >= M scalars apart, z_tail n_wit rows z_stride >= 2m + 3 scalars apart
 * (strides <= 2^31, n_wit <= VMPC_FR_CS_MAX_WIT, else
 * VMPC_E_RANGE; n_wit = 0: VMPC_OK, no launch).  The table 1 / k and the weights are computed once, the correlation runs
 * on a grid (tiles, segments, witnesses), and the segment length is chosen with n_wit counted, so a large batch uses
 * fewer, longer segments.  Canonical residues: the bits are those of n_wit single calls whatever the segmentation.
 * Arena: vmpc_fr_cs_extend_batch_bytes(m, n_wit); when it cannot be reserved the error is returned and nothing is
 * launched. */
int vmpc_fr_cs_extend_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t m, const void *fact,
                                const void *ifact, void *z_tail, size_t z_stride, size_t n_wit);
/* the arena bytes vmpc_fr_cs_extend_batch_dev reserves (0 where the call would answer VMPC_E_RANGE or do nothing) on a
 * context in the DIRECT mode below; _ctx: on THIS context, by the route its mode gives this m and under its NTT arena
 * cap (ctx NULL: the direct figure) */
size_t vmpc_fr_cs_extend_batch_bytes(size_t m, size_t n_wit);
size_t vmpc_fr_cs_extend_batch_bytes_ctx(const vmpc_ctx *ctx, size_t m, size_t n_wit);
/* The batch entries over GF(n), the BN-256 order: the same templates at the other field (the batch prover of the
 * knowledge-of-exponent variant).  Arguments, range checks, caps (VMPC_FR_CS_MAX_WIT, VMPC_FR_CS_MAX_M), return codes and
 * both extension routes are their GF(l) namesakes'; the arena figures are the same numbers. */
int vmpc_bn256_fr_cs_triples_batch_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col,
                                       const void *a_vals, const void *a_const, const uint32_t *b_row_ptr,
                                       const uint32_t *b_col, const void *b_vals, const void *b_const,
                                       const uint32_t *gates, size_t n_gates, size_t n_x, size_t gamma_offset, void *z,
                                       size_t z_stride, void *a_out, void *b_out, size_t ab_stride, size_t n_wit, int check,
                                       uint32_t *first_bad);
int vmpc_bn256_fr_cs_extend_batch_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t ab_stride, size_t m,
                                      const void *fact, const void *ifact, void *z_tail, size_t z_stride, size_t n_wit);
size_t vmpc_bn256_fr_cs_extend_batch_bytes(size_t m, size_t n_wit);
size_t vmpc_bn256_fr_cs_extend_batch_bytes_ctx(const vmpc_ctx *ctx, size_t m, size_t n_wit);
/* How the three extension entries - and with them circuit_sat_prover, its batch and the M-party prover - compute the
 * sums over j for x = m+2 .. 2m.  DIRECT: the correlation kernel, 2 m^2 multiply-accumulates; a new context starts
 * here.  NTT: the cyclic product of the 2 n_wit rows u_f, u_g with the table 1 / k by the multi-prime NTT over the
 * integers (csrc/bn256_ntt.hip) at L = vmpc_fr_cs_extend_ntt_len(m) points, the window's exact integer coefficients
 * (< 2^20 l^2) reduced mod l: the same canonical residues, so z is the direct kernel's bit for bit.  AUTO: the NTT from
 * VMPC_FR_CS_EXT_NTT_MIN gates on.  Any other mode: VMPC_E_INVAL, the mode stays.  A mode of its own:
 * vmpc_ctx_set_poly_product does not touch it.  The arena then also holds the residues of the table and of a group of the
 * rows (vmpc_ctx_set_ntt_arena_cap applies), still ONE reservation before the first launch.
 * vmpc_fr_cs_extend_ntt_len: L, the smallest power of two >= 2m + 2 (alias-free for the window m+1 .. 2m-1 although
 * the whole product has 3m + 2 coefficients), or 0 where the direct kernel is taken WHATEVER the mode: m < 2 (no
 * correlation) and m = 2^20 = VMPC_FR_CS_MAX_M, where 2m + 2 exceeds the longest transform, 2^21 points. */
#define VMPC_CS_EXTENSION_DIRECT 0
#define VMPC_CS_EXTENSION_AUTO 1
#define VMPC_CS_EXTENSION_NTT 2
/* the smallest power of two on the grid of scripts/cs_extension_probe.py at which the NTT's median was below the direct
 * kernel's and stayed below at every larger grid size (the table of DESIGN.md section 28) */
#define VMPC_FR_CS_EXT_NTT_MIN ((size_t)64)
int vmpc_ctx_set_cs_extension(vmpc_ctx *ctx, int mode);
int vmpc_ctx_get_cs_extension(vmpc_ctx *ctx, int *mode);
size_t vmpc_fr_cs_extend_ntt_len(size_t m);
/* The same extension with f and g kept apart, nothing multiplied and no z: f_out[0] = f(0), f_out[1 + o] = f(m + 2 + o)
 * for o < m - 1, g_out alike; max(m, 1) scalars each.  Linear in a and b, so on Shamir shares of them it gives shares
 * of f and g at those points (mpc_ac20_cb.py:66-85 interpolates and evaluates share polynomials).  Arena as above. */
int vmpc_fr_cs_extend_fg_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact, const void *ifact,
                             void *f_out, void *g_out);
/* out[j] = the Lagrange basis polynomial of node j among 0..K at c, j = 0..K (ac20/recombine.py:5-32 as called by
 * circuit_builder.py:548-549); ifact: the table with at least K + 1 entries.  No inversion: exact for every c, a
 * node included (the unit vector).  Arena: 3 K scalars. */
int vmpc_fr_cs_lagrange_dev(vmpc_ctx *ctx, const uint8_t c[32], size_t K, const void *ifact, void *out);
/* Transposed sparse mat-vec: out is zeroed (n_out scalars), then out[dst] = sum over the entries e of a column of
 * vals[e] * weights[rows[e]] (circuit_builder.py:517-545).  Entries in column order and the plan (items, long_cols,
 * n_partial) as vmpc_bn256_qap_colsum_dev takes them, over this field: an item's dst is the column's position in out,
 * so positions that no column maps to stay zero.  Rows >= n_rows add nothing, positions >= n_out are not written.
 * n_rows <= 2^31 and the plan's bounds as there, else VMPC_E_RANGE.  Arena: n_partial scalars. */
int vmpc_fr_cs_colsum_dev(vmpc_ctx *ctx, const void *weights, size_t n_rows, const uint32_t *rows, const void *vals,
                          size_t nnz, const uint32_t *items, size_t n_items, const uint32_t *long_cols, size_t n_long,
                          size_t n_partial, void *out, size_t n_out);
/* *first_diff (a device uint32) = the smallest i < n with a[i] != b[i], 0xffffffff if none.  No arena. */
int vmpc_fr_cs_first_diff_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, uint32_t *first_diff);

/* ---- The same over GF(n), n the BN-256 group order: Protocol 8 for the knowledge-of-exponent pivot (DESIGN.md section
 * 29).  One template per kernel and host body with the GF(l) entries above (csrc/circuit_sat.hip), instantiated at
 * csrc/fr_bn.h; arguments, caps (VMPC_FR_CS_MAX_M) and answers are those of the namesake above, VMPC_E_NONCANON for a
 * scalar ARGUMENT >= n.  Scalars in device memory may be any 32-byte value (reduced mod n when loaded); outputs are
 * canonical residues.  vmpc_ctx_set_cs_extension governs vmpc_bn256_fr_cs_extend_dev as it governs the GF(l) entry: on
 * the NTT route a window coefficient is below 2^20 n^2 < 2^532, inside the 551 bits of the 18 primes, and is reduced mod
 * n - the same canonical residues as the direct kernel's.  Arena: the extension and the column sum reserve as above;
 * tables and lagrange do NOT use the arena - `scratch` is the caller's device memory of
 * vmpc_bn256_fr_cs_tables_scratch_bytes(K) / vmpc_bn256_fr_cs_lagrange_scratch_bytes(K) bytes (0: K out of range), not
 * read, and free again when the stream has passed the call.  The share form (_fg) exists over both fields
 * (vmpc_bn256_fr_cs_extend_fg_dev below: the M-party KoE prover); the batch form exists over GF(l)
 * only. */
int vmpc_bn256_fr_cs_triples_dev(vmpc_ctx *ctx, const uint32_t *a_row_ptr, const uint32_t *a_col, const void *a_vals,
                                 const void *a_const, const uint32_t *b_row_ptr, const uint32_t *b_col,
                                 const void *b_vals, const void *b_const, const uint32_t *gates, size_t n_gates,
                                 size_t n_x, size_t gamma_offset, void *z, void *a_out, void *b_out, int check,
                                 uint32_t *first_bad);
size_t vmpc_bn256_fr_cs_tables_scratch_bytes(size_t K);
int vmpc_bn256_fr_cs_tables_dev(vmpc_ctx *ctx, size_t K, void *fact, void *ifact, void *scratch);
int vmpc_bn256_fr_cs_extend_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact,
                                const void *ifact, void *z_tail);
/* vmpc_fr_cs_extend_fg_dev over GF(n): f and g kept apart for a witness of Shamir shares mod n (mpc_ac20_cb.py:66-85),
 * max(m, 1) canonical residues each; arguments, caps, answers and arena as there, the route by
 * vmpc_ctx_set_cs_extension. */
int vmpc_bn256_fr_cs_extend_fg_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t m, const void *fact,
                                   const void *ifact, void *f_out, void *g_out);
size_t vmpc_bn256_fr_cs_lagrange_scratch_bytes(size_t K);
int vmpc_bn256_fr_cs_lagrange_dev(vmpc_ctx *ctx, const uint8_t c[32], size_t K, const void *ifact, void *out,
                                  void *scratch);
int vmpc_bn256_fr_cs_colsum_dev(vmpc_ctx *ctx, const void *weights, size_t n_rows, const uint32_t *rows,
                                const void *vals, size_t nnz, const uint32_t *items, size_t n_items,
                                const uint32_t *long_cols, size_t n_long, size_t n_partial, void *out, size_t n_out);
/* two encodings of one residue (v and v + n, where that fits 256 bits) compare equal */
int vmpc_bn256_fr_cs_first_diff_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, uint32_t *first_diff);

/* ---- Shamir sharings of vectors mod l (csrc/mpc_share.hip; verifiable_mpc/ac20/mpc_ac20_cb.py:39-189 through
 * mpc.schur_prod and mpc._random).  Party q < parties holds the value at node q + 1.  Matrices are row-major in device
 * memory, row r at base + 32 r stride.  parties <= VMPC_SHARE_MAX_PARTIES, n and the strides <= 2^31: above them the
 * entries answer VMPC_E_RANGE before they look at any pointer.  Deterministic (no atomics on field values),
 * asynchronous on the context's stream, no arena. */
#define VMPC_SHARE_MAX_PARTIES 64
/* d_i = a_i b_i (b == NULL: a_i); out[q][i] = d_i + sum_{k=1..t} coeffs[k-1][i] (q + 1)^k for q < parties: a fresh
 * degree-t sharing of every d_i (coeffs: t rows of n scalars, stride n; t = 0 copies d to every row).  The Shamir
 * dealer, and the local half of a product of shares.  t < parties, out_stride >= n, else VMPC_E_INVAL.  The vector
 * operands are canonical residues and are not checked (as for vmpc_fr_axpy_dev). */
int vmpc_fr_share_mul_deal_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, const void *coeffs, size_t t,
                               size_t parties, void *out, size_t out_stride);
/* out[dst ? dst[i] : i] = sum_{p < parties} weights[p] parts[p][i] for i < n.  weights: parties x 32 bytes in HOST
 * memory; dst: n uint32 in device memory or NULL - the caller keeps every dst[i] inside out, positions that no dst[i]
 * names are left alone.  The products are summed unreduced and reduced once, which is why every operand must be a
 * canonical residue: a weight >= l is VMPC_E_NONCANON at once; an element of parts >= l leaves its output unwritten
 * and the next vmpc_ctx_sync answers VMPC_E_NONCANON.  part_stride >= n, else VMPC_E_INVAL. */
int vmpc_fr_share_combine_dev(vmpc_ctx *ctx, const void *parts, size_t parties, size_t n, size_t part_stride,
                              const uint8_t *weights, const uint32_t *dst, void *out);

/* ---- The same sharings mod n, BN-256's group order, for Pinocchio proofs from a shared witness
 * (demos/demo_zkp_trinocchio.py:76-93: mpc.gather of the witness and h shares, compute_proof on them, recombination of
 * the proof elements).  Conventions, caps and VMPC_SHARE_MAX_PARTIES as above. */
/* vmpc_fr_share_mul_deal_dev over GF(n); the vector operands may be any 32-byte values and are taken mod n.  With
 * b == NULL the Shamir dealer; with a all zeros and t = 2 t' the dealer of degree-2t' sharings of zero. */
int vmpc_bn256_fr_share_mul_deal_dev(vmpc_ctx *ctx, const void *a, const void *b, size_t n, const void *coeffs,
                                     size_t t, size_t parties, void *out, size_t out_stride);
/* out[dst ? dst[i] : i] = addend[i] + sum_{p < parties} weights[p] parts[p][i] for i < n; addend: n scalars in device
 * memory (any 32-byte values, taken mod n) or NULL.  n^2 fills 512 bits - three products of n - 1 still fit 512 bits,
 * four need 513 - so the products are summed in the wide accumulator of csrc/fr256.h (f256_acc) and reduced once.
 * Canonicity as for vmpc_fr_share_combine_dev: a weight >= n is VMPC_E_NONCANON at once; an element of parts >= n
 * leaves its output unwritten and the next vmpc_ctx_sync answers VMPC_E_NONCANON.  part_stride >= n, else
 * VMPC_E_INVAL. */
int vmpc_bn256_fr_share_combine_dev(vmpc_ctx *ctx, const void *parts, size_t parties, size_t n, size_t part_stride,
                                    const uint8_t *weights, const uint32_t *dst, const void *addend, void *out);

/* out[e] = sum_{p < parties} weights[p] parts[p][e] for e < n, a sum of group elements: the recombination of the proof
 * shares in the exponent (demos/demo_zkp_trinocchio.py:86-93; csrc/bn256_recombine.hip).  group 1
 * (64-byte affine points) or 2 (128-byte); parts: `parties` rows of points in device memory, row p at
 * parts + width p part_stride (part_stride in POINTS); all-zero bytes are the point at infinity, in and out; out: n
 * canonical affine points, so the bytes do not depend on how the sum is organised.  weights: parties x 32 bytes in HOST
 * memory, canonical residues mod n, passed to the kernel as arguments (a weight above n / 2 as its negative and a
 * negated point).  Points are not validated (vmpc_bn256_validate_dev).  parties > VMPC_SHARE_MAX_PARTIES, n or
 * part_stride above 2^31: VMPC_E_RANGE before any pointer is looked at; a weight >= n: VMPC_E_NONCANON at once;
 * part_stride < n, another group, parties = 0 with n > 0, a null pointer where there is work: VMPC_E_INVAL; n = 0:
 * VMPC_OK, no launch.  One lane per (party, element), the partial sums of a workgroup's wavefronts added through LDS in
 * a fixed order; asynchronous on the context's stream, no arena, no atomics. */
int vmpc_bn256_recombine_dev(vmpc_ctx *ctx, int group, const void *parts, size_t parties, size_t n, size_t part_stride,
                             const uint8_t *weights /* HOST */, void *out);

/* out[i] = scalars[i] * points[i] for i < n, every point with a scalar of its own: one party's pass over a jointly made
 * pp of the knowledge-of-exponent pivot (csrc/bn256_scale.hip; the role of the loop of
 * verifiable_mpc/ac20/mpc_ac20.py:54-84).  group 1 (64-byte affine points) or 2 (128-byte); points, scalars and out in
 * device memory; all-zero bytes are the point at infinity, in and out; out: n canonical affine points, so the bytes do
 * not depend on how the chain is organised.  A scalar is the 256-bit little-endian integer as it stands, NOT reduced
 * mod n (for a point of order n the result is the same either way); 0 gives infinity.  Points are not validated
 * (vmpc_bn256_validate_dev).  n above 2^31: VMPC_E_RANGE before any pointer is looked at; another group, a null pointer
 * with n > 0: VMPC_E_INVAL; n = 0: VMPC_OK, no launch.  One lane per element, a branch-free 256-bit double-and-add
 * (csrc/scale_chain.h) and one inversion; asynchronous on the context's stream, no arena, no atomics. */
int vmpc_bn256_scale_points_dev(vmpc_ctx *ctx, int group, const void *points, const void *scalars, size_t n, void *out);

/* ---- The R1CS solve on shares mod n (demos/demo_zkp_trinocchio.py:70: qap.calculate_witness on secure values, one
 * MPyC multiplication per `*` line of the flat code, tools/code_to_r1cs.py:253-274; csrc/bn256_r1cs_share.hip, DESIGN.md
 * section 23).  One party's two halves of a ROUND: the product rows r0 .. r1-1 of a plan in the layout of
 * vmpc_bn256_r1cs_solve_batch_dev (pynocchio.ShareSolvePlan; all plan arrays in DEVICE memory) on n_wit share vectors c,
 * c_stride scalars apart, slot 0 = 1 and every slot that the rows read a canonical residue.  With n_r = r1 - r0 the
 * element of row i and witness w is e = w n_r + (i - r0), n_e = n_wit n_r.  The rows that need no exchange run through
 * vmpc_bn256_r1cs_solve_batch_dev itself, which computes a party's share of a linear row's wire unchanged.
 * parties > VMPC_SHARE_MAX_PARTIES, n_wit > VMPC_BN256_R1CS_MAX_WIT, a stride or n_e above 2^31, c_stride < m + 1:
 * VMPC_E_RANGE before any pointer is looked at; t >= parties, a table stride below n_e, r1 < r0, a null pointer where
 * there is work: VMPC_E_INVAL; an empty range or n_wit = 0: VMPC_OK, no launch.  One lane per (row, witness),
 * deterministic (no atomics on field values), asynchronous on the context's stream, no arena. */
/* d = (V_i . c_w)(W_i . c_w), this party's degree-2t share of the product, and a fresh degree-t sharing of it:
 * out[q][e] = d + sum_{k=1..t} coeffs[k-1][e] (q + 1)^k for q < parties (coeffs: t rows of n_e scalars, stride n_e;
 * out: `parties` rows, out_stride apart; t = 0 copies d to every row).  d itself is written nowhere. */
int vmpc_bn256_r1cs_share_mul_deal_dev(vmpc_ctx *ctx, const uint32_t *v_row_ptr, const uint32_t *v_col,
                                       const void *v_vals, const uint32_t *w_row_ptr, const uint32_t *w_col,
                                       const void *w_vals, size_t r0, size_t r1, size_t m, const void *c, size_t c_stride,
                                       size_t n_wit, const void *coeffs, size_t t, size_t parties, void *out,
                                       size_t out_stride);
/* After the exchange: c_w[wire_i] = (sum_{p < parties} weights[p] parts[p][e] - Y_i . c_w) inv_i, the sum in the wide
 * accumulator of csrc/fr256.h, reduced once; an inverse of 1 is not multiplied.  weights: parties x 32 bytes in HOST
 * memory.  Canonicity as for vmpc_bn256_fr_share_combine_dev: a weight >= n is VMPC_E_NONCANON at once; an element of
 * parts >= n leaves its wire unwritten and the next vmpc_ctx_sync answers VMPC_E_NONCANON. */
int vmpc_bn256_r1cs_share_finish_dev(vmpc_ctx *ctx, const uint32_t *y_row_ptr, const uint32_t *y_col, const void *y_vals,
                                     const uint32_t *wire, const void *inv, size_t r0, size_t r1, size_t m,
                                     const void *parts, size_t parties, size_t part_stride,
                                     const uint8_t *weights /* HOST */, void *c, size_t c_stride, size_t n_wit);

/* ---- Pi_Nullity (AC20 p. 17-18, verifiable_mpc/ac20/nullity.py:21-40): s dense linear forms over n variables as a
 * row-major matrix in device memory, row i at rows + 32 i row_stride, 32-byte little-endian elements.  ANY 256-bit
 * element is accepted and taken mod l (the arithmetic reduces it on the way in); results are canonical.  Caps:
 * s <= VMPC_FR_ROWS_MAX_S, n and row_stride <= VMPC_FR_ROWS_MAX_N; above them the entries answer VMPC_E_RANGE before
 * they look at any pointer and write nothing.  row_stride >= n (not read when s <= 1).  Deterministic: integer sums in
 * a fixed order, no atomics on field values. */
#define VMPC_FR_ROWS_MAX_S ((size_t)1 << 16)
#define VMPC_FR_ROWS_MAX_N ((size_t)1 << 30)
/* out[j] = sum_{i<s} rho^i rows[i][j] for j < n (nullity.py:25 and :32, L = sum_i linform_i * rho**i): one pass over
 * the matrix, Horner from the last row down; few columns under many rows (n < 65536, s >= 32) are cut into row
 * segments whose partial rows are combined with rho^(segment length).  rho: a canonical residue (VMPC_E_NONCANON
 * otherwise).  s = 0: zeros; s = 1: the reduced row.  `out` must not overlap `rows`.  Arena: the partial rows (below
 * 2^17 scalars). */
int vmpc_fr_rows_combine_dev(vmpc_ctx *ctx, const void *rows, size_t s, size_t n, size_t row_stride,
                             const uint8_t rho[32], void *out);
/* out[i] = sum_{j<n} rows[i][j] x[j] for i < s (device memory, s scalars): every L_i(x) of pivot.py:84-92 in one launch
 * sequence.  *first_nonzero (a device uint32; may be NULL) = the smallest i with out[i] != 0, 0xffffffff if there is
 * none.  Arena: at most max(s, 2048) scalars. */
int vmpc_fr_rows_dot_dev(vmpc_ctx *ctx, const void *rows, size_t s, size_t n, size_t row_stride, const void *x, void *out,
                         uint32_t *first_nonzero);

/* ---- Batch verification of compact Protocol-4/5 proofs over one CRS (csrc/batch_verify.hip).
 * Proof p < K has `rounds` challenges c_{p,i}, a final response z'_p of 2^low_bits elements and a weight w_p; with
 * N = 2^(rounds + low_bits) and v_p[j] as vmpc_fr_challenge_products_dev defines it for (c_p, z'_p):
 *     u_out[j]    = sum_p w_p v_p[j]                          N residues
 *     dots_out[p] = sum_{j < form_len} w_p v_p[j] forms[p][j]  K residues   (elements from form_len on count as zero)
 * so that the K final checks (compressed_pivot.py:193-197) become ONE N-term MSM with scalars u.  Everything is in
 * device memory: challenges_dev K x rounds, zprime_dev K x 2^low_bits, weights_dev K canonical residues (not checked,
 * as for the vector operands above); forms_dev: K device pointers held in device memory, each to form_len residues
 * (may be NULL when form_len == 0).  No v_p is written anywhere; results are canonical and bit-reproducible (integer
 * sums in a fixed order, no atomics).  Caps: K <= VMPC_FR_BATCH_MAX_K, rounds <= VMPC_FR_BATCH_MAX_ROUNDS,
 * rounds + low_bits <= VMPC_FR_BATCH_MAX_BITS; above them the entry answers VMPC_E_RANGE before it looks at any pointer.
 * K < 1, a negative count, a missing pointer or form_len > N: VMPC_E_INVAL.  Nothing is launched or written after
 * either.  Asynchronous on the context's stream.  Arena: K (2^(a+1) + 2^b) + K * segments scalars, a = min(rounds,
 * (rounds + low_bits) / 2), b = rounds + low_bits - a. */
#define VMPC_FR_BATCH_MAX_K 4096
#define VMPC_FR_BATCH_MAX_ROUNDS 20
#define VMPC_FR_BATCH_MAX_BITS 30
int vmpc_fr_batch_products_dev(vmpc_ctx *ctx, int K, int rounds, int low_bits, const void *challenges_dev,
                               const void *zprime_dev, const void *weights_dev, const void *const *forms_dev,
                               size_t form_len, void *u_out, void *dots_out);

/* SHA-256 of every `chunk_bytes`-sized piece of a device buffer (last piece may be short):
 * out_digests[i] = SHA256(data[i*chunk : (i+1)*chunk]), 32 bytes each.  Leaves of the compact
 * transcript's two-level digests; not used by the reference transcript. */
int vmpc_sha256_chunks_dev(vmpc_ctx *ctx, const void *data, size_t nbytes, size_t chunk_bytes,
                           void *out_digests);

/* k halving folds of a tabulated generator vector in one pass (compressed_pivot.py:64 applied k times):
 *   out[j] = sum_{b < 2^k} scalars[b] * P[j + b * (n_cols >> k)],   j < n_cols >> k,
 * over the first n_cols columns of `table` (generators, then extras), n_cols a power of two, 1 <= k <= 6.
 * `scalars`: 2^k canonical 32-byte residues in HOST memory (the challenge products); out: affine x||y.
 * 64 mixed additions per column instead of a 253-bit scalar multiplication per generator and round. */
int vmpc_msm_table_fold_dev(vmpc_ctx *ctx, const void *table, size_t table_n, size_t table_extra, int rows,
                            size_t n_cols, int k, const uint8_t *scalars, void *out_affine);

/* The plan vmpc_msm_table_fold_dev / _table_dev make for (rows, n_cols, k, scalars) on this context, for tests
 * (csrc/fold_jump_plan.h; the calls above go through the same code).  Digit position p of a scalar - n_digits signed
 * digits of digit_bits bits, 8 or, for 16 rows or under VMPC_FOLD_JUMP_DIGITS=4, 4 - uses table row p / O at offset
 * p % O; the walk is launched as grid_x x grid_y workgroups of 256 lanes, n_blocks of the grid_x with work, grid_y = S
 * lanes sharing the schedule of one (output, offset).  sched_out: NULL, or room for sched_capacity_words >= sched_words
 * = O * e1 words: per offset the number of entries, the entries by |digit| descending (bits 0..7 = scalar index,
 * 8..12 = row, 15 = negate, 16..23 = |digit|) and a closing 0.  VMPC_E_NONCANON for a scalar >= l.  Host side only:
 * no launch, no device access, nothing taken from the workspace. */
typedef struct vmpc_fold_plan {
    int32_t digit_bits, n_digits, O, e1, S;
    uint32_t n_blocks, grid_x, grid_y;
    uint64_t m_out, sched_words;
} vmpc_fold_plan;
int vmpc_msm_table_fold_plan(vmpc_ctx *ctx, int rows, size_t n_cols, int k, const uint8_t *scalars,
                             vmpc_fold_plan *out, uint32_t *sched_out, size_t sched_capacity_words);

/* the same fold, leaving the folded vector's own fixed-base table (out_rows rows, the n_extra device points
 * extra_affine_points as its extras; size: vmpc_msm_table_bytes(n_cols >> k, n_extra, out_rows)) instead of the
 * vector - what a prover that keeps committing to the folded generators wants (vmpc_p4_round uses it) */
int vmpc_msm_table_fold_table_dev(vmpc_ctx *ctx, const void *table, size_t table_n, size_t table_extra, int rows,
                                  size_t n_cols, int k, const uint8_t *scalars, const void *extra_affine_points,
                                  size_t n_extra, int out_rows, void *out_table);

/* ---- device-resident Protocol-4 prover rounds (SURVEY.md 8b "vmpc_ctx_round") -----------------------------------
 * One halving round of compressed_pivot.py:29-86 per call: z_hat, L~ and the per-generator challenge products stay in
 * HBM for all log N rounds; a round folds z_hat and L~ with the previous challenge (:70-76), computes the two
 * inner products that are the exponents of k (:41-42), and A_i, B_i as one batched pass over the tabulated CRS
 * (the generators are not folded: the pending challenge products multiply the scalars).  The Fiat-Shamir hash
 * stays with the caller.  `table`: vmpc_msm_table_build_dev over table_n generators g followed by table_extra
 * extras; extras 0 .. h_slots-1 are the tail of g_hat (h), extra k_slot is k (k_affine: the same point, x||y,
 * host memory).  z_hat / L_tilde: N = table_n + h_slots device scalars each, N a power of two.
 * On a CRS of 2^18 generators or more the context folds the generators once, after 5 rounds, with
 * vmpc_msm_table_fold_dev and continues on a table of the 32-times shorter vector (VMPC_P4_JUMP=0: never). */
typedef struct vmpc_p4 vmpc_p4;
int vmpc_p4_create(vmpc_ctx *ctx, const void *table, size_t table_n, size_t table_extra, int rows, int h_slots,
                   int k_slot, const uint8_t k_affine[64], const void *z_hat, const void *L_tilde, vmpc_p4 **out);
/* vmpc_p4_create with the number of rounds before the generators are folded chosen by the caller (jump_k = 0: never,
 * < 0: the default of 5) and, with lazy_fold != 0, a fold that waits for vmpc_p4_prefold: the round that is given the
 * jump_k-th challenge still commits over the unfolded table, and the fold is enqueued - on the context's stream,
 * nothing waited for - when the caller asks (not between vmpc_p4_round_begin and _end), at the latest at the start of
 * the round after.  vmpc_p4_prefold without a fold that is due does nothing.  vmpc_p4_run_compact refuses a lazy
 * context. */
int vmpc_p4_create_opts(vmpc_ctx *ctx, const void *table, size_t table_n, size_t table_extra, int rows, int h_slots,
                        int k_slot, const uint8_t k_affine[64], const void *z_hat, const void *L_tilde, int jump_k,
                        int lazy_fold, vmpc_p4 **out);
int vmpc_p4_prefold(vmpc_p4 *p4);
/* A second table over the SAME generators and extras (same n, same extras in the same order) for the A_i, B_i
 * commitments of the rounds BEFORE the generators are folded - the 13-row wide-window table (vmpc_msm_table_build_dev
 * with rows = 13): 13 mixed additions per term instead of 16.  The fold itself reads the table given to
 * vmpc_p4_create (rows spaced 256 / rows bits).  NULL: none.  The caller keeps it alive as long as the context. */
int vmpc_p4_set_commit_table(vmpc_p4 *p4, const void *table, int rows);
/* The same rounds with g_hat cut into `world` CONTIGUOUS blocks, one per rank of `comm` (one process
 * per GPU): block_table = vmpc_msm_table_build_dev over THIS rank's block_n = N / world generators (h is the last
 * generator of the last block) with k among its extras (k_slot); z_hat / L_tilde: all N scalars, the same on every
 * rank.  A round computes the partial A_i, B_i over the block and exchanges them once (vmpc_comm_points_allsum_dev);
 * every rank returns the same A_i, B_i.  The k term is added by rank 0.  The fold of the generators after 5 rounds
 * stays local: a rank folds the strides its block holds (needs 2^5 >= 2 world and a block of >= 2^18 generators)
 * and later rounds commit to the rank's partial vector.  world must be a power of two.  All ranks must make the
 * same calls in the same order. */
int vmpc_p4_create_sharded(vmpc_ctx *ctx, vmpc_comm *comm, const void *block_table, size_t block_n, size_t table_extra,
                           int rows, int k_slot, const uint8_t k_affine[64], const void *z_hat, const void *L_tilde,
                           vmpc_p4 **out);
/* prev_challenge: derived from the previous call's A, B; NULL on the first call.  out_A / out_B: affine x||y.
 * Valid log2(N) - 1 times.  If a call fails after the witness fold was enqueued the context is unusable: every
 * further call returns VMPC_E_INVAL, destroy it (vmpc_ctx_destroy refuses while a round context is alive). */
int vmpc_p4_round(vmpc_p4 *p4, const uint8_t prev_challenge[32], uint8_t out_A[64], uint8_t out_B[64]);
/* vmpc_p4_round in two halves, for a caller with host work of its own to do while the pair is computed (the reference
 * transcript's prover enqueues the round's exact generator fold on another stream meanwhile): _begin folds the witness
 * with prev_challenge and enqueues the commitments without waiting, _end waits and returns A_i, B_i.  Until _end every
 * other vmpc_p4_* call on this context except vmpc_p4_destroy returns VMPC_E_INVAL. */
int vmpc_p4_round_begin(vmpc_p4 *p4, const uint8_t prev_challenge[32]);
int vmpc_p4_round_end(vmpc_p4 *p4, uint8_t out_A[64], uint8_t out_B[64]);
/* after the last round: fold with its challenge and return z' (two 32-byte residues, compressed_pivot.py:77-79) */
int vmpc_p4_finish(vmpc_p4 *p4, const uint8_t last_challenge[32], uint8_t out_z_prime[64]);
/* every round and the finish behind one call, with the COMPACT transcript's challenge chain (verifiable_mpc_amd/
 * compressed_pivot.py, _Transcript): state_i = SHA-256(state_{i-1} || round index, 4 bytes LE || A_i || B_i),
 * c_i = state_i (little-endian integer) mod l.  state: in = the chain value before the first round, out = after the
 * last.  out_AB: (log2(N) - 1) x 128 bytes, A_i || B_i affine.  The context must not have run a round yet. */
int vmpc_p4_run_compact(vmpc_p4 *p4, uint8_t state[32], int first_round_index, uint8_t *out_AB, uint8_t out_z_prime[64]);
int vmpc_p4_destroy(vmpc_p4 *p4);

#ifdef __cplusplus
}
#endif
#endif
