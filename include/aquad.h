/*
 * aquad.h -- C ABI of the MI355X-native adaptive-quadrature engine (libaquad.so).
 *
 * The reference (/root/reference/aquadPartA.c) has no plugin or FFI layer: its boundary is
 * the macro quartet F/A/B/EPSILON (:45-48) plus the farmer/worker message protocol
 * (farmer() :125-173, worker() :175-208) that main() (:78-123) drives. Each entry point below
 * names the reference interface it replaces. Plain C types only: no HIP, RCCL or torch types cross
 * this boundary; every host buffer is caller-owned; device memory, streams, events and RCCL
 * communicators are owned by opaque handles (aq_ctx: one GPU; aq_group: GPUs that combine results
 * over RCCL). No global state; a handle is not re-entrant; calls block unless the name says _async.
 * Errors: 0 on success, a negative AQ_E* code otherwise (the reference's only error is
 * numprocs < 2 -> stderr + exit(1), :86-90; the CLI maps codes to that behaviour).
 *
 * Deviation from SURVEY.md §8b's sketch: every call takes its aq_ctx / aq_group first (the sketch's
 * own "no global state" rule); aq_integrate_batch also returns per-integral task counts.
 */
#ifndef AQUAD_H
#define AQUAD_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AQ_OK 0
#define AQ_EINVAL (-1)     /* bad argument (non-finite bounds, b < a, eps < 0, bad shard, outside the integrand's domain;
                            every integrand: each bound 0 or 2^-900 <= |x| <= 2^900) */
#define AQ_EHIP (-2)       /* a HIP runtime call failed */
#define AQ_ETIMEOUT (-3)   /* an on-device wait saw no progress for the stall bound (aq_set_stall_timeout) */
#define AQ_EOVERFLOW (-4)  /* a frontier / work-queue capacity was exceeded */
#define AQ_EDEPTH (-5)     /* refinement reached max_depth (the reference would not terminate) */
#define AQ_ENOMEM (-6)     /* device or host allocation failed */
#define AQ_ENODEV (-7)     /* no HIP device */
#define AQ_ERCCL (-8)      /* an RCCL call failed (aq_group_*) */
#define AQ_ERESIDENT (-9)  /* the persistent grid cannot be co-resident on the device (its workgroups wait
                            on each other): refused before launch, never a stall */
#define AQ_ENOCONV (-10)   /* some integral missed its tolerance within max_rounds (outputs are still all written) */

#define AQ_DEFAULT_MAX_DEPTH 96
#define AQ_MAX_LEVELS 128     /* length of the per-level histograms */
#define AQ_CU_SLOTS 2048      /* hardware CU slot space: xcc*256 + (se*2+sh)*16 + cu */
#define AQ_XS_LIMBS 68        /* exact area accumulator: int64 limbs (aq_fetch_exact / aq_exact_round) */
#define AQ_EXACT_ROW (AQ_XS_LIMBS + 4)   /* limbs, tasks, accepted, spilled, levels | error << 32 */
#define AQ_MAX_PARAMS 4       /* most parameters per integral of the AQ_F_PARAM family (aq_param_count()) */

/* Integrand = the reference's F(arg) macro (aquadPartA.c:46) as a compile-time kernel variant. */
typedef enum {
    AQ_F_COSH4 = 0,     /* cosh(x)*cosh(x)*cosh(x)*cosh(x), glibc-2.35-exact cosh (the reference), |x| <= 170 */
    AQ_F_SIN_RECIP = 1, /* sin(1/x) (SURVEY config 4), glibc-exact for |x| > 9.5e-9 */
    AQ_F_USER = 2,      /* the plug-in compiled in from AQ_USER_F_HEADER (aq_user_integrand_name()) */
    AQ_F_PARAM = 3      /* the parametrised plug-in F(x; theta) compiled in from AQ_PARAM_F_HEADER
                           (aq_param_integrand_name()): one parameter row per integral, through the
                           aq_*_params entry points only -- every other entry point refuses it */
} aq_integrand;

/* Replaces the compile-time macros EPSILON / F / A / B (aquadPartA.c:45-48) and mpirun -n (:83). */
typedef struct {
    int32_t integrand;  /* aq_integrand */
    int32_t max_depth;  /* refinement cap; 0 -> AQ_DEFAULT_MAX_DEPTH (<= AQ_MAX_LEVELS - 1) */
    double a;           /* A (:47) */
    double b;           /* B (:48) */
    double eps;         /* EPSILON (:45): absolute, strict '>' test (:191) */
    int32_t n_gpus;     /* GPUs the integral is sharded over: 0 or 1 for aq_integrate, the group size
                           (or 0) for aq_integrate_group */
    int32_t reserved;
} aq_problem;

/* Replaces farmer()'s return value and the global tasks_per_process[] (:72, :101, :162). */
typedef struct {
    double area;        /* Σ accepted larea+rarea (:199 sent, :149 summed): the exact sum of the workers'
                           partials (per-lane double sums in the persistent kernel), rounded once -- within
                           a few ulp of the exact leaf sum, last bits schedule-dependent */
    uint64_t tasks;     /* intervals evaluated = Σ tasks_per_process (:162) */
    uint64_t accepted;  /* accepted subintervals (tag-1 area messages, :201) */
    uint32_t levels;    /* 1 + deepest refinement level reached */
    uint32_t n_cu;      /* CUs that evaluated at least one task. Per-CU counts (n_cu, tasks_per_cu) are kept
                           for the synchronous calls and for launches of fewer than 12 integrals into slots
                           below 16384; other launches report n_cu = 0 and zero rows (their per-CU work is
                           still counted by aq_cu_task_counters, which sees every launch) */
    uint64_t spilled;   /* interval pairs moved through the HBM work queue (load balance) */
    uint32_t n_gpus;    /* GPUs that contributed (entries written to tasks_per_gpu) */
    uint32_t reserved;
    uint64_t *tasks_per_gpu;  /* [n_gpus] caller-owned or NULL: tasks per GPU (the workers of :162) */
    uint64_t *tasks_per_cu;   /* [n_gpus * aq_ctx_num_cus()] caller-owned or NULL: tasks per CU, each
                                 GPU's CUs in hardware-slot order (0 where not kept) */
} aq_result;

typedef struct aq_ctx aq_ctx;

/* ---- lifecycle (replaces MPI_Init / MPI_Comm_size / MPI_Finalize, :82-84, :121) ------------- */
int aq_device_count(int *count);
int aq_ctx_create(int device, aq_ctx **out);
void aq_ctx_destroy(aq_ctx *ctx);
const char *aq_strerror(int code);
/* Compute units of the context's device (one persistent workgroup each). */
int aq_ctx_num_cus(const aq_ctx *ctx);
/* Wavefront workers of the on-device farmer (workgroups x 12 waves per workgroup): the partition of
 * sharded and multi-integral launches (aq_integrate_shard documents it). An unsharded launch of ONE
 * integral runs 8 waves per workgroup (its set-up and seeding are issue-bound at three waves per SIMD);
 * launches of 2 or more integrals run 12. */
int aq_ctx_num_workers(const aq_ctx *ctx);
/* Device memory the context holds, bytes. */
int aq_ctx_device_bytes(const aq_ctx *ctx, uint64_t *bytes);
/* Per-level task/accepted histograms on the persistent path (default on; a diagnostic the
 * reference does not produce -- pipelined callers switch it off). */
int aq_set_level_histograms(aq_ctx *ctx, int enable);
/* The persistent kernel's grid is one workgroup per CU (AQ_GRID=<n> in the environment at create time
 * overrides it, e.g. to leave CUs to other work). Its workgroups hand work to each other, so every
 * launch checks -- for the exact kernel instance, block size and LDS -- that the device can hold the
 * whole grid at once, and refuses with AQ_ERESIDENT otherwise. AQ_COOP=1 at create time launches it
 * as a cooperative kernel (the runtime's own co-residency guarantee) instead of a plain launch. */
/* How long a waiting workgroup tolerates NO PROGRESS of the on-device work queue before the launch
 * fails with AQ_ETIMEOUT (default 10 s, or the AQ_STALL_MS environment variable at create time). A
 * bound on stalls, not on run time: launches of any length that keep progressing never time out. */
int aq_set_stall_timeout(aq_ctx *ctx, double ms);
/* Name of the AQ_F_USER plug-in compiled into this library. */
const char *aq_user_integrand_name(void);

/* ---- the hot path ----------------------------------------------------------------------------
 * aq_integrate: farmer(numprocs) + every worker() of one run (:125-208) as ONE persistent HIP
 * launch: wavefronts expand sibling-pair frontiers in LDS (task body :183-202), accumulate accepted
 * areas, and rebalance through an HBM work queue (the bag of tasks, :152-165).
 * Bit-identical interval tree: `tasks` and `accepted` equal the reference's counts exactly.
 * The synchronous calls (aq_integrate, aq_integrate_shard) use an internal result slot, never the
 * caller's async slots, and read it back with one small kernel into pinned host memory.
 */
int aq_integrate(aq_ctx *ctx, const aq_problem *p, aq_result *res);

/* This process's share of a multi-GPU run: the depth-D positions (D = floor(log2(V)) + 2) are
 * dealt in snake order over V = nshards * aq_ctx_num_workers() virtual workers; shard `shard`
 * evaluates its positions' subtrees plus the tasks at depth <= D it owns (each counted by the
 * owner of its leftmost descendant position, so by exactly one shard). Summing
 * area/tasks/accepted over all shards (the caller's all-reduce, or aq_integrate_group) gives
 * exactly the single-GPU result. */
int aq_integrate_shard(aq_ctx *ctx, const aq_problem *p, int shard, int nshards, aq_result *res);
/* The same shard, returned as its exact row (int64[AQ_EXACT_ROW], the layout of aq_fetch_exact): the
 * input of a caller's int64 all-reduce (ppls_amd/dist.py). Blocking, internal slot like
 * aq_integrate_shard; the return code carries the row's error bits (the row is written either way). */
int aq_integrate_shard_exact(aq_ctx *ctx, const aq_problem *p, int shard, int nshards, int64_t *row);

/* ---- multi-GPU over RCCL (replaces the MPI layer, :145-171, and `result += buff[0]`, :149) ----
 * A group is a set of contexts, one per GPU, joined by RCCL communicators over xGMI. Either one
 * process drives n GPUs (aq_group_create: ncclCommInitAll), or every process drives one GPU
 * (the MPI layout: rank 0 makes an id with aq_group_unique_id, the caller broadcasts it -- e.g.
 * MPI_Bcast -- and every rank calls aq_group_join). aq_integrate_group runs rank r's shard r of N
 * on each member, then ONE grouped RCCL exchange: an int64 all-reduce of the exact area limbs and
 * counts (so the area is the correctly rounded exact sum, whatever N) and an all-gather of each
 * rank's task / per-CU counts (tasks_per_gpu, tasks_per_cu). Every member gets the whole result. */
typedef struct aq_group aq_group;
#define AQ_GROUP_ID_BYTES 128
int aq_group_create(aq_ctx *const *ctxs, int n, aq_group **out);
int aq_group_unique_id(void *id /* AQ_GROUP_ID_BYTES */);
int aq_group_join(aq_ctx *ctx, int nranks, int rank, const void *id, aq_group **out);
void aq_group_destroy(aq_group *g);
int aq_group_size(const aq_group *g);
int aq_integrate_group(aq_group *g, const aq_problem *p, aq_result *res);

/* Asynchronous form for pipelined callers (bench): enqueue one integral on the context's stream,
 * results land in device slot `slot` (0 <= slot < aq_async_slots()); aq_fetch blocks for it. */
int aq_async_slots(void);
int aq_integrate_async(aq_ctx *ctx, const aq_problem *p, int shard, int nshards, int slot);
/* K integrals of one integrand / eps / max_depth in ONE persistent launch (K <=
 * aq_max_integrals_per_launch()): integral i has bounds [a[i], b[i]] and lands in slot first_slot+i
 * (first_slot + k <= aq_async_slots()). The integrals share the machine: a wave that runs out of
 * work on one integral seeds its share of the next, so the tail of each overlaps the next. */
int aq_max_integrals_per_launch(void);
int aq_integrate_many_async(aq_ctx *ctx, int integrand, int k, const double *a, const double *b, double eps,
                            int max_depth, int shard, int nshards, int first_slot);
/* Like aq_integrate_many_async with a per-integral shard: integral i is shard shard[i] of nshards
 * (the partition of aq_integrate_shard; every launch of one nshards uses the same partition, so any
 * rank may run any shard of any integral -- the rebalanced multi-GPU batch, ppls_amd/dist.py).
 * nshards == 1 (every shard[i] 0: whole integrals) is an unsharded launch, as aq_integrate_many_async. */
int aq_integrate_mixed_async(aq_ctx *ctx, int integrand, int k, const double *a, const double *b,
                             const int32_t *shard, int nshards, double eps, int max_depth, int first_slot);
int aq_fetch(aq_ctx *ctx, int slot, aq_result *res);
/* The slot's exact row: int64[AQ_EXACT_ROW] = area limbs, tasks, accepted, spilled,
 * levels | error bits << 32 -- summed limb-wise across shards (an int64 all-reduce), the rounded
 * area is the same whatever the partition. */
int aq_fetch_exact(aq_ctx *ctx, int slot, int64_t *row);
/* Correctly rounded double of AQ_XS_LIMBS exact-accumulator limbs (host function). */
double aq_exact_round(const int64_t *limbs);
int aq_synchronize(aq_ctx *ctx);
/* Enqueue (on the context's stream) a copy of n consecutive slots' totals, starting at first_slot
 * (mod aq_async_slots()), into the DEVICE buffer d_out as n rows of 4 doubles
 * {area, tasks, accepted, error bits}: the input of one all-reduce for n pipelined integrals. */
int aq_gather_results(aq_ctx *ctx, int first_slot, int n, void *d_out);
/* The same slots as exact int64 rows (AQ_EXACT_ROW each) into the DEVICE buffer d_out. */
int aq_gather_exact(aq_ctx *ctx, int first_slot, int n, void *d_out);

/* Level-synchronous breadth-first path (one kernel per tree level, host loop): the debug /
 * cross-check schedule. Fills per-level histograms (caller arrays of length maxlev or NULL). */
int aq_integrate_levels(aq_ctx *ctx, const aq_problem *p, aq_result *res, uint64_t *tasks_per_level,
                        uint64_t *leaves_per_level, int maxlev);

/* Frontier engine over caller-owned device buffers (the level-synchronous multi-GPU schedule of
 * ppls_amd/frontier.py). A frontier is n records {l, r, F(l), F(r)} (4 doubles each, row-major) of
 * one tree depth. aq_frontier_root writes the root record of [a, b] to d_out[0].
 * aq_level_step enqueues one task step (aquadPartA.c:183-202) on every record of d_in: refining
 * records append their two children to d_out (at most cap_out records; the number written lands in
 * the device counter *d_n_out, which the call zeroes first), accepted ones add into the device
 * accumulator d_acc[8] = {area hi, area lo (double-double), tasks, accepted, error bits, deepest
 * level, 0, 0}; the caller zeroes d_acc once per integral. Both calls are asynchronous on the
 * context's stream and never read device memory from the host.
 * The area is exact to the double-double's own rounding: with n accepted records of areas t_i (each the
 * reference's double larea + rarea), |d_acc[0] + d_acc[1] - sum t_i| <= n * 2^-100 * sum |t_i|, whatever the
 * order the lanes, blocks and folds add them in (the bound of aq_integrate_mesh's cum; aq_level_narrow too).
 * A step runs min(ceil(n_in / 1024), 8192) workgroups, each striding over the level in chunks of 1024 records;
 * AQ_LEVEL_GRID=<n> in the environment (read at aq_ctx_create, clamped to 1..8192) puts n in place of the 8192,
 * so that a small level runs several chunks per workgroup -- for tests; the results do not depend on it. */
int aq_frontier_root(aq_ctx *ctx, int integrand, double a, double b, double *d_out);
int aq_level_step(aq_ctx *ctx, int integrand, const double *d_in, uint32_t n_in, double *d_out, uint32_t cap_out,
                  double eps, int depth, int max_depth, uint32_t *d_n_out, double *d_acc);
/* The same step with the input count read on the DEVICE from *d_n_in (a counter a previous step
 * wrote), so levels chain on the stream with no host round trip (ppls_amd/frontier.py syncs only
 * every few levels, or at rebalancing levels). n_in_max bounds *d_n_in (it sizes the grid; blocks
 * past the real count exit at once). *d_n_out is NOT zeroed: the caller zeroes the counters once
 * (one array of per-level counts: level d reads counts[d] and appends to counts[d + 1]). */
int aq_level_step_chained(aq_ctx *ctx, int integrand, const double *d_in, const uint32_t *d_n_in, uint32_t n_in_max,
                          double *d_out, uint32_t cap_out, double eps, int depth, int max_depth, uint32_t *d_n_out,
                          double *d_acc);

/* Deferred folds: while enabled, the level steps leave their per-block partial rows pending and ONE
 * fold adds them into the accumulator later -- at aq_synchronize, at a step with another d_acc, or
 * when disabling (the chained engine's levels between two host looks then cost one launch each, not
 * two). d_acc is complete once aq_synchronize returns. */
int aq_level_defer_fold(aq_ctx *ctx, int enable);
/* `levels` consecutive levels in ONE single-workgroup launch (the narrow top of the tree, where a
 * launch per level is launch- and latency-bound): level depth + k reads d_counts[depth + k] records
 * from d_buf{k & 1} and appends its children to d_buf{(k + 1) & 1} (at most cap records), writing
 * their number to d_counts[depth + k + 1]; the accepted areas and counts add into d_acc as
 * aq_level_step's do. The last level's children are in d_buf{levels & 1}. Asynchronous. */
int aq_level_narrow(aq_ctx *ctx, int integrand, double *d_buf0, double *d_buf1, uint32_t cap, uint32_t *d_counts,
                    int depth, int levels, double eps, int max_depth, double *d_acc);

/* The frontier engine on ONE GPU with its host loop in C (ppls_amd/frontier.py's single-rank path):
 * the root, the narrow top (aq_level_narrow), then chained level steps with deferred folds, the
 * frontier size read every sync_every levels. Frontier buffers of cap records each are context-owned
 * (grown on demand). Fills res and the per-level histograms (arrays of maxlev, or NULL). */
int aq_frontier_integrate(aq_ctx *ctx, const aq_problem *p, uint32_t cap, int sync_every, aq_result *res,
                          uint64_t *tasks_per_level, uint64_t *leaves_per_level, int maxlev);

/* Per-level task / accepted histograms of the last aq_integrate* call (levels 0..maxlev-1). */
int aq_level_histogram(aq_ctx *ctx, uint64_t *tasks_per_level, uint64_t *leaves_per_level, int maxlev);

/* Per-CU task counters of the last call (tasks_per_process[] mapped to compute units).
 * out[AQ_CU_SLOTS] indexed by hardware slot; returns the number of non-zero slots. */
int aq_tasks_per_cu(aq_ctx *ctx, uint64_t *out, int cap);
/* Per-CU task counters of EVERY persistent launch (any shape: lone integrals, batches, shards),
 * summed since the context was created or last reset: each workgroup adds its tasks to its hardware
 * CU slot once at exit. out[AQ_CU_SLOTS] by hardware slot (cap entries written); reset != 0 zeroes
 * the counters after the read. Waits for the context's stream. Returns the number of non-zero slots.
 * Σ out == Σ tasks of the launches since the reset (every task is counted by the CU that ran it). */
int aq_cu_task_counters(aq_ctx *ctx, uint64_t *out, int cap, int reset);

/* Batch front end (SURVEY config 3): n independent integrals [a[i], b[i]] of one integrand.
 * Per-integral area / accepted / tasks (any may be NULL). NOTE the output order: accepted BEFORE
 * tasks (round 1's header had a single `accepted` output; both are uint64_t*, so a caller written
 * against another order compiles and gets the arrays swapped). The integrals run in launches of up
 * to aq_max_integrals_per_launch(); each launch's bounds are validated just before it is enqueued,
 * so a bad bound in a later launch returns AQ_EINVAL after the earlier launches ran: the outputs
 * are then unspecified (not all-or-nothing). Each launch runs its integrals largest-first (a device
 * pre-pass estimates every tree's size; only the order changes, never a result); the host checks,
 * stages and unpacks on up to 8 threads (a pool the context keeps, created by its first batch call).
 * Environment: AQ_BATCH_SORT=0 keeps the input order, AQ_HOST_THREADS=<n> bounds the host threads
 * (read when the pool is created), AQ_BATCH_FIRST / AQ_BATCH_LAST set the first / last launch's size
 * (defaults 131072 / no split), AQ_BATCH_TRACE=1 prints the call's host phase times on stderr. */
int aq_integrate_batch(aq_ctx *ctx, size_t n, const double *a, const double *b, double eps, int integrand,
                       double *area, uint64_t *accepted, uint64_t *tasks);

/* Device evaluation of the integrand / of cosh (libm parity checks). */
int aq_eval_integrand(aq_ctx *ctx, int integrand, size_t n, const double *x, double *out);
int aq_eval_cosh(aq_ctx *ctx, size_t n, const double *x, double *out);

/* ---- per-integral parameters: F(x; theta_i) ----------------------------------------------------
 * The reference's F(arg) macro is one function; AQ_F_PARAM is a FAMILY compiled in from a plug-in
 * header (default: the Gaussian exp(-((x - mu) * s)^2), theta = {mu, s}; at {0, 1} bit for bit the
 * AQ_F_USER Gaussian). Every integral carries its own row of aq_param_count() doubles, theta is
 * row-major [integrals][aq_param_count()]. The calls mirror aq_eval_integrand, aq_integrate,
 * aq_integrate_many_async and aq_integrate_batch (same slots, same readers: aq_fetch, aq_fetch_exact,
 * aq_gather_*; same chunking, size order and AQ_BATCH_* environment) and return AQ_EINVAL for a null
 * theta, a non-finite entry, or a row outside the family's domain. aq_integrate_params wants
 * p->integrand == AQ_F_PARAM. The device theta buffers are allocated by the first of these calls.
 * Not covered: aq_integrate_levels, the frontier engine (aq_level_*, aq_frontier_*) and
 * aq_integrate_group take no theta and return AQ_EINVAL for AQ_F_PARAM. */
int aq_param_count(void);                       /* nparams of the compiled-in family */
const char *aq_param_integrand_name(void);
int aq_eval_integrand_params(aq_ctx *ctx, size_t n, const double *x, const double *theta /* [n*np] */, double *out);
int aq_integrate_params(aq_ctx *ctx, const aq_problem *p, const double *theta /* [np] */, aq_result *res);
int aq_integrate_many_params_async(aq_ctx *ctx, int k, const double *a, const double *b,
                                   const double *theta /* [k*np] */, double eps, int max_depth, int shard,
                                   int nshards, int first_slot);
int aq_integrate_batch_params(aq_ctx *ctx, size_t n, const double *a, const double *b,
                              const double *theta /* [n*np] */, double eps, double *area, uint64_t *accepted,
                              uint64_t *tasks);

/* ---- error estimate and extrapolated area ------------------------------------------------------
 * EPSILON bounds each accepted interval's difference d = (larea + rarea) - lrarea (:191), not the
 * result. The _err calls run the same interval tree (area, tasks, accepted and levels as the plain
 * calls give them) and also sum d over the accepted tasks, at no extra F evaluation:
 *   err_abs    = Σ|d|  an estimate of the area's error (what QUADPACK calls abserr);
 *   err_signed = Σd    one Richardson (Simpson) step: area + err_signed / 3 (aq_err_extrapolate).
 * Each term is the reference's own value; the sums are plain double sums in a schedule-dependent order
 * (within accepted * 2^-52 * err_abs of the exact sums). They have no exact-row form; an integral's
 * shards' sums add up to the whole integral's.
 * theta is the AQ_F_PARAM row(s) ([np] / [k*np] / [n*np]) and must be non-NULL exactly when the
 * integrand is AQ_F_PARAM (validated as the _params calls do), else AQ_EINVAL. The calls mirror
 * aq_integrate, aq_integrate_many_async and aq_integrate_batch (same slots; aq_fetch, aq_fetch_exact and
 * aq_gather_* read an ERR slot as any other; same chunking, size order and AQ_BATCH_* environment; either
 * of the batch's two error outputs may be NULL as its other outputs may). aq_fetch_err waits for the
 * slot like aq_fetch and returns AQ_EINVAL unless the slot's last launch was an _err launch; any launch
 * into a slot zeroes its sums first. An _err launch runs 8 waves per workgroup whatever its shape (every
 * _err launch of one nshards deals one partition), keeps no level histograms or diagnostics (levels is
 * reported) and leaves per-CU counts as the plain calls do. The device buffers are allocated by the
 * first of these calls.
 * Not covered: aq_integrate_mixed_async, aq_integrate_group, aq_integrate_levels and the frontier
 * engine (aq_level_*, aq_frontier_*) have no _err form. */
typedef struct { double err_abs, err_signed; } aq_err;   /* Σ|d|, Σd over accepted tasks, d = (larea+rarea)-lrarea (:191) */
double aq_err_extrapolate(double area, const aq_err *e);  /* host: area + err_signed / 3 (one Richardson step) */
int aq_integrate_err(aq_ctx *ctx, const aq_problem *p, const double *theta, aq_result *res, aq_err *err);
int aq_integrate_many_err_async(aq_ctx *ctx, int integrand, int k, const double *a, const double *b,
                                const double *theta, double eps, int max_depth, int shard, int nshards,
                                int first_slot);
int aq_fetch_err(aq_ctx *ctx, int slot, aq_err *err);
int aq_integrate_batch_err(aq_ctx *ctx, size_t n, const double *a, const double *b, const double *theta, double eps,
                           int integrand, double *area, uint64_t *accepted, uint64_t *tasks, double *err_abs,
                           double *err_signed);

/* ---- tolerance-driven batch: epsabs / epsrel on the result ---------------------------------------
 * aq_integrate_batch_tol integrates n integrals of one integrand until each one's error estimate meets the
 * caller's tolerance: rounds of ERR launches at a shrinking EPSILON, every round over the integrals that
 * have not retired yet. Round r runs at eps_r (eps_1 = eps0, eps_{r+1} = eps_r / shrink: one division per
 * round, so a caller reproduces the schedule bit for bit); one EPSILON per round because EPSILON is an
 * argument of the launch. After a round an integral is CONVERGED when, evaluated in double exactly so,
 *     err_abs <= fmax(epsabs, epsrel * fabs(area))
 * (a tie converges; a NaN in err_abs or area does not). An integral retires when it converges, when its row
 * carries error bits (it is not relaunched), or in round max_rounds. The test, the retiring rows' records
 * and the stable compaction of the survivors' bounds and parameters run on the device between two launches;
 * the host reads one count per round. err_abs is the device's sum, schedule-dependent within
 * accepted * 2^-52 * err_abs (above): a decision nearer to its target than that may go either way from
 * run to run.
 * Outputs (any may be NULL; accepted BEFORE tasks, as aq_integrate_batch_err): every integral reports the
 * area, counts and sums of the round in which it retired, eps_used[i] that round's EPSILON, and
 * rounds[i] = r (1-based) when it converged in round r, -r when it retired in round r without converging
 * (r == max_rounds, or its row carried error bits).
 * Returns the code of the rows' error bits if any row had some (AQ_ETIMEOUT, AQ_EOVERFLOW, AQ_EDEPTH), else
 * AQ_ENOCONV if an integral did not converge -- the outputs are all written in both cases -- else AQ_OK.
 * AQ_EINVAL: a bad aq_tol (below; also when the last round's EPSILON would no longer be a normal double), a
 * theta that does not go with the integrand (as the _err calls), a bad bound or parameter row (checked block
 * by block as the batch front end checks chunk by chunk: the outputs are then unspecified).
 * The call blocks. The integrals run in blocks of up to aq_max_integrals_per_launch() (AQ_TOL_BLOCK=<n> in
 * the environment, read per call, sets a smaller block), every round's launch into slots 0 .. k-1, which the
 * call leaves clean; rows run in compacted input order (no size order). Its device buffers are allocated by
 * the first of these calls.
 * Not covered: shards, aq_group, aq_integrate_mixed_async, aq_integrate_levels and the frontier engine. */
typedef struct {
    double epsabs, epsrel;  /* converged when err_abs <= fmax(epsabs, epsrel * fabs(area)); both >= 0, finite, not both 0 */
    double eps0;            /* EPSILON of round 1; finite, > 0 */
    double shrink;          /* eps of round r+1 = eps of round r / shrink (one division per round); 0 -> 8; else in [2, 1024] */
    int32_t max_rounds;     /* 0 -> 12; else 1..64 */
    int32_t max_depth;      /* as aq_problem.max_depth */
} aq_tol;
int aq_integrate_batch_tol(aq_ctx *ctx, size_t n, const double *a, const double *b, const double *theta,
                           int integrand, const aq_tol *tol,
                           double *area, uint64_t *accepted, uint64_t *tasks,
                           double *err_abs, double *err_signed,
                           double *eps_used, int32_t *rounds);

/* ---- device-resident batch: device arrays in and out, ordered on a stream ---------------------------
 * aq_integrate_batch_device is the _err batch (and, with both error outputs NULL, the plain and _params
 * batch) for a caller whose bounds and parameter rows are already on the GPU and whose results stay there:
 * every pointer of aq_device_io is DEVICE memory of the context's device. The call only ENQUEUES: it reads no
 * bound on the host, copies nothing to or from the host and waits for no stream or event, whatever n (its
 * only blocking work is the allocation of its device rings, by the first such call of a context -- and, for
 * AQ_F_PARAM, of their theta part by the first such AQ_F_PARAM call; aq_ctx_device_bytes does not move before).
 * Ordering. `stream` points to the caller's hipStream_t (the pointer's target may be the null stream): the
 * context's stream first waits for everything enqueued on that stream so far, and before the call returns
 * that stream has been made to wait for the last output write -- work the caller enqueues on it afterwards
 * sees complete outputs, and may free or overwrite the inputs. stream == NULL: no caller's stream; the inputs
 * must be complete when the call is made, and aq_synchronize or aq_device_batch_check orders the outputs.
 * Results. The same trees, counts, areas and error sums as aq_integrate_batch_err gives for the same rows
 * (the sums within the bound stated there), in input order; ERR launches (8 waves per workgroup) run iff
 * err_abs or err_signed is non-NULL, plain launches otherwise. Any output may be NULL.
 * Per-row status in place of an all-or-nothing AQ_EINVAL: a row outside the domain (the rule of AQ_EINVAL
 * above, checked on the device by the same predicate the host calls use) gets status AQ_ROW_INVALID, area and
 * error sums NaN and accepted = tasks = 0, and disturbs no other row (inside the launch it runs as the empty
 * interval [0, 0], one task, which aq_cu_task_counters does count). A row whose slot carries error bits gets
 * them in status, and the outputs the host batch would give for it: AQ_ROW_DEPTH on the rows whose own tree
 * reached max_depth, AQ_ROW_TIMEOUT and AQ_ROW_OVERFLOW -- the launch's, which no row can be blamed for -- on
 * every row of the chunk. Other rows get status 0.
 * AQ_EINVAL from the host: a NULL ctx or io, NULL a or b with n > 0, a theta that does not go with the
 * integrand (the rule of the _err calls), a bad eps, max_depth or integrand. n == 0 returns AQ_OK and enqueues
 * nothing. Device pointers are NOT otherwise validated (a host pointer or a short array is undefined
 * behaviour), and inputs that overlap outputs are undefined.
 * aq_device_batch_check waits for the context's stream, stores in *invalid_rows (may be NULL) the number of
 * AQ_ROW_INVALID rows since the last check, and returns AQ_EINVAL if there were any, else the code of the OR of
 * the rows' error bits since the last check (AQ_ETIMEOUT, AQ_EOVERFLOW, AQ_EDEPTH), else AQ_OK; it then resets
 * both. Before the first device batch of a context it reports 0 and AQ_OK.
 * The rows run in chunks of up to aq_max_integrals_per_launch() (AQ_DEVBATCH_CHUNK=<n> in the environment,
 * read per call and clamped to [1, that], sets a smaller chunk), each in size order (AQ_BATCH_SORT=0: input
 * order); the next chunk is checked and sized on a side stream while one runs. The launches use slots
 * 0 .. chunk-1 -- a chunk of fewer than 12 rows slots from 16384 -- and leave them clean; the call has
 * device rings and events of its own, so the other calls of the context may follow it without waiting.
 * Not covered: a device form of aq_integrate_batch_tol (it needs one host look per round by design), shards
 * and aq_group, the frontier engine, the CLI. */
#define AQ_ROW_TIMEOUT  1u   /* the slot error bits, as in a gathered row's 4th field ... */
#define AQ_ROW_OVERFLOW 2u
#define AQ_ROW_DEPTH    4u
#define AQ_ROW_INVALID  8u   /* ... and: the row failed the domain check and was not integrated */
typedef struct {
    const double *a, *b;          /* DEVICE, [n] */
    const double *theta;          /* DEVICE, [n * aq_param_count()] row-major; non-NULL exactly for AQ_F_PARAM */
    double   *area;               /* DEVICE [n] or NULL */
    uint64_t *accepted, *tasks;   /* DEVICE [n] or NULL */
    double   *err_abs, *err_signed; /* DEVICE [n] or NULL; ERR launches run iff one of them is non-NULL */
    uint32_t *status;             /* DEVICE [n] or NULL: 0, or AQ_ROW_* bits */
    int32_t   max_depth;          /* as aq_problem.max_depth */
    int32_t   reserved;
} aq_device_io;
int aq_integrate_batch_device(aq_ctx *ctx, size_t n, const aq_device_io *io, double eps, int integrand,
                              void *const *stream);
int aq_device_batch_check(aq_ctx *ctx, uint64_t *invalid_rows);

/* ---- the accepted mesh: the tree's leaves in x order, and the running integral ----------------------
 * aq_integrate_mesh builds the tree aq_frontier_integrate(ctx, p, frontier_cap, sync_every, ...) builds -- res is
 * filled exactly as that call fills it -- and keeps what that call throws away: the partition of [a, b] into
 * accepted subintervals. The call blocks. Every pointer of aq_mesh_io is DEVICE memory of the context's device.
 * Nodes. An accepted task [l, r] with mid = (l + r) / 2 (aquadPartA.c:187) contributes the panels [l, mid] and
 * [mid, r]; the nodes are all leaf bounds and midpoints in increasing order, m + 1 = 2 * accepted + 1 of them:
 * x[2j] = l_j, x[2j+1] = mid_j, x[m] = b. f holds the very values the task steps computed (F(l), F(mid), F(r):
 * nothing is evaluated again), level[k] the depth of the accepted task that owns panel [x_k, x_k+1].
 * Running integral. With P_j = Σ_{i<j} (larea_i + rarea_i), each term the reference's own double (:189-190,
 * :199): cum[2j] is P_j and cum[2j+1] is P_j + larea_j, each rounded to double once; cum[0] = 0 and cum[m] =
 * P_accepted. The prefix is carried in double-double, its error <= accepted * 2^-100 * Σ|larea_i + rarea_i|, so
 * every cum value is the correctly rounded exact prefix or its neighbour; cum[m] and res->area are two roundings
 * of the same sum.
 * Determinism. For given inputs x, f, cum and level are bit-identical from run to run and for every sync_every
 * (the leaves leave the level kernels in schedule order, are sorted by their unique left bounds, and the scan's
 * tree depends on the leaf count alone).
 * *n_nodes receives 2 * accepted + 1. If that exceeds cap_nodes the tree is still walked to its end -- leaves
 * past the capacity are counted, not stored -- res and *n_nodes are written, the return is AQ_EOVERFLOW and the
 * arrays are unspecified: retry with the size reported. AQ_EOVERFLOW from the frontier capacity and AQ_EDEPTH
 * are aq_frontier_integrate's; the mesh would have gaps, so the arrays are unspecified and *n_nodes = 0.
 * AQ_EINVAL: a NULL ctx, p, io, n_nodes, x, f or cum; cap_nodes < 3 or > 2^31; the argument errors of
 * aq_frontier_integrate; AQ_F_PARAM (the frontier engine takes no theta).
 * Device memory: leaf records (48 bytes per leaf of cap_nodes / 2), sort keys, indices and scratch, and scan
 * partials are context-owned, allocated by the first mesh call, grown on demand and freed with the context;
 * aq_ctx_device_bytes does not move before that first call.
 * aq_mesh_eval gives the integral from x_0 to each q of d_q[nq] from a mesh (device arrays of n_nodes): for
 * x_0 <= q <= x_m, with k the largest index <= m - 1 such that x_k <= q, one IEEE operation each:
 *   h = q - x_k;  w = x_k+1 - x_k;  fq = f_k + (f_k+1 - f_k) * (h / w);  out = cum_k + (f_k + fq) * h / 2
 * -- the trapezoid rule on the partial panel: continuous across nodes up to rounding, monotone where F >= 0,
 * equal to cum_k at every node x_k, k < m (at x_m: cum_m-1 plus the last panel's trapezoid), its error on a full leaf the leaf's accepted |d| <= EPSILON. A q outside
 * [x_0, x_m], or NaN, gives NaN. The call only enqueues on the context's stream and reads nothing on the host
 * (aq_synchronize orders the output). AQ_EINVAL: a NULL ctx, a NULL array with nq > 0, n_nodes < 3.
 * aq_mesh_invert answers the reverse question, for each y of d_y[nq] the x at which the integral from x_0 reaches
 * y: quantiles, equal-mass partitions, inverse-CDF samples. For a mesh whose cum is non-decreasing (F >= 0, or
 * any F whose trapezoids are all >= 0) and cum_0 <= y <= cum_m, with k the largest index <= m - 1 such that
 * cum_k <= y, one IEEE double operation each, nothing contracted, sqrt correctly rounded:
 *   w = x_k+1 - x_k;  r = y - cum_k;  s = (f_k+1 - f_k) / w;
 *   disc = fmax(f_k * f_k + (2 * s) * r, 0);  den = f_k + sqrt(disc);
 *   h = (r == 0) ? 0 : (2 * r) / den;  h = fmin(h, w);  out = x_k + h
 * -- the stable root of r = f_k h + s h^2 / 2, which inverts aq_mesh_eval's trapezoid on the partial panel. So:
 * out lies in [x_k, x_k+1]; out is non-decreasing in y; out == x_k exactly when y == cum_k (for k < m, where cum
 * increases strictly); across a run of equal cum values (panels of zero area) the answer is the right end of the
 * run; at y == cum_m the answer is the last panel's root (b up to the conditioning ulp(y) / F), or x_m-1 if that
 * panel has zero area. A y outside [cum_0, cum_m], or NaN, gives NaN. If the panel the search ends in does not
 * satisfy cum_k <= y <= cum_k+1 the output is NaN: that happens only when cum is not non-decreasing -- F changes
 * sign, as sin(1/x) does -- and on such a mesh every output is NaN or a point of [x_0, x_m] and nothing more is
 * promised (every index stays in bounds). The call only enqueues on the context's stream, reads nothing on the
 * host and owns no device memory (aq_synchronize orders the output). AQ_EINVAL as for aq_mesh_eval: a NULL ctx,
 * a NULL array with nq > 0, n_nodes < 3; nq == 0 enqueues nothing. Few queries take a binary search over cum, one
 * query per lane; many (2^21 and more) a kernel that first searches every 2^sh-th value of cum in a 2048-entry
 * table in LDS; both return the same k, and AQ_MESH_INVERT=0 / 1 in the environment, read per call, forces the
 * first / the second.
 * Not covered: meshes from the persistent kernel (aq_integrate*, shards, aq_group, the batches, the
 * tolerance-driven batch), inversion of non-monotone meshes, host-memory outputs (callers copy), the CLI.
 * AQ_F_PARAM and several meshes per call are aq_integrate_mesh_batch's, with aq_mesh_eval_batch and
 * aq_mesh_invert_batch (below). */
typedef struct {
    double  *x;      /* DEVICE [cap_nodes]: x_0 = a < x_1 < ... < x_m = b, m = 2 * accepted */
    double  *f;      /* DEVICE [cap_nodes]: F(x_k), the values the tree evaluated */
    double  *cum;    /* DEVICE [cap_nodes]: running integral, cum_0 = 0 */
    uint8_t *level;  /* DEVICE [cap_nodes - 1] or NULL: depth of the accepted task that owns panel k */
} aq_mesh_io;
int aq_integrate_mesh(aq_ctx *ctx, const aq_problem *p, uint32_t frontier_cap, int sync_every,
                      uint64_t cap_nodes, const aq_mesh_io *io, aq_result *res, uint64_t *n_nodes);
int aq_mesh_eval(aq_ctx *ctx, uint64_t n_nodes, const double *d_x, const double *d_f, const double *d_cum,
                 size_t nq, const double *d_q, double *d_out);
int aq_mesh_invert(aq_ctx *ctx, uint64_t n_nodes, const double *d_x, const double *d_f, const double *d_cum,
                   size_t nq, const double *d_y, double *d_out);

/* ---- batched meshes: many integrals' leaves, cum and queries in one call ---------------------------
 * aq_integrate_mesh_batch builds the meshes of n integrals of one integrand -- AQ_F_PARAM included, row i under
 * theta[i * aq_param_count() ..] -- in ONE level-synchronous run: the records of every row's depth d share one
 * frontier, so a level is one launch whatever n. Every pointer of aq_mesh_batch_io is DEVICE memory of the
 * context's device. The call blocks, as aq_integrate_mesh does; the inputs must be complete when it is made.
 * Per-row mesh. Row i with a valid domain gets exactly the mesh aq_integrate_mesh defines for [a[i], b[i]] at eps:
 * 2 * accepted_i + 1 nodes at x / f / cum [offsets[i], offsets[i+1]), x, f and level the values the task steps
 * computed, cum restarting at 0 with the row; tasks_i = 2 * accepted_i - 1. level[k] is the depth of the task that
 * owns panel k -> k+1; at a row's last node it is unspecified.
 * Invalid rows. The domain rule of AQ_EINVAL above, checked on the device by the predicate the host calls use (as
 * aq_integrate_batch_device does). A row that fails gets AQ_ROW_INVALID in status, no nodes (offsets[i+1] ==
 * offsets[i]), area NaN, accepted = tasks = 0 and no record in the frontier; it disturbs no other row.
 * Running integral. Each row's prefix is carried in double-double and adds that row's terms alone (a segmented
 * scan: no global prefix, nothing subtracted), so it errs by at most accepted_i * 2^-100 * Σ|terms of row i| and
 * every cum value is the correctly rounded exact prefix of its own row or that value's neighbour, whatever the
 * magnitudes of the rows before it. area[i] is the row's last cum.
 * Determinism. For given inputs every output is bit-identical from run to run and for every sync_every (the
 * leaves are sorted by (row, l), unique; the scan's tree depends on the rows' leaf counts alone).
 * Capacity. info->n_nodes = 2 * leaves + valid rows, written even when it exceeds cap_nodes: the trees are then
 * still walked to their end -- leaves past the capacity are counted, not stored -- the return is AQ_EOVERFLOW,
 * offsets, the node arrays and the per-row outputs but status are unspecified and nothing is written at or past
 * cap_nodes: retry with the size reported.
 * Frontier overflow. A level of all rows together that exceeds frontier_cap records: AQ_EOVERFLOW with
 * info->n_nodes = 0. info->widest_level of a successful run, the largest level, is the frontier_cap that suffices.
 * AQ_EDEPTH when any row refines at max_depth: info->n_nodes = 0, the node arrays are unspecified, and status
 * carries AQ_ROW_DEPTH on exactly the rows whose unbounded tree has more than max_depth levels. status (the
 * AQ_ROW_INVALID and AQ_ROW_DEPTH bits) is written whatever the return, once the arguments were accepted.
 * AQ_EINVAL: a NULL ctx, io, a, b, offsets, x, f, cum or info; a theta that does not go with the integrand (the
 * rule of the _err calls); a bad eps, max_depth or sync_every; frontier_cap < max(n, 2); cap_nodes < 3 or > 2^31.
 * n == 0: AQ_OK, info zeroed, nothing enqueued. info->invalid_rows, leaves, tasks and levels describe the run.
 * Device memory. The batch frontier (32 + 4 bytes a record of frontier_cap, twice; the records are the frontier
 * engine's buffers), leaf records (48 bytes per leaf of cap_nodes / 2; aq_integrate_mesh's), sort arrays and
 * scratch, row tables and scan partials are context-owned, allocated by the first such call, grown on demand and
 * freed with the context; aq_ctx_device_bytes does not move before that call, nor at a second call of the same
 * sizes.
 * aq_mesh_eval_batch / aq_mesh_invert_batch answer nq_per_row queries for each of the n rows of such a mesh: row
 * i's query j, d_q[i * nq_per_row + j], is bit for bit what aq_mesh_eval / aq_mesh_invert (its plain search) return
 * for it on the slice [offsets[i], offsets[i+1]) -- the NaN cases included -- and a row of fewer than 3 nodes
 * answers NaN. One query per lane, a binary search inside the row's slice. The calls only enqueue on the
 * context's stream, own no device memory and read nothing on the host (aq_synchronize orders the output).
 * AQ_EINVAL: a NULL ctx, or a NULL array with n * nq_per_row > 0.
 * Not covered: shards and aq_group, meshes from the persistent kernel, the CLI, a device-side retry when a
 * capacity is missed, a staged-table search for very many queries per row. A finer mesh from this one, and with it
 * a per-row eps, are aq_mesh_refine_batch's (below). */
typedef struct {
    const double *a, *b;        /* DEVICE [n] */
    const double *theta;        /* DEVICE [n * aq_param_count()] row-major; non-NULL exactly for AQ_F_PARAM */
    uint64_t *offsets;          /* DEVICE [n + 1]: row i's nodes are [offsets[i], offsets[i+1]) of x / f / cum */
    double   *x, *f, *cum;      /* DEVICE [cap_nodes] */
    uint8_t  *level;            /* DEVICE [cap_nodes] or NULL */
    double   *area;             /* DEVICE [n] or NULL: the row's last cum (NaN for an invalid row) */
    uint64_t *accepted, *tasks; /* DEVICE [n] or NULL */
    uint32_t *status;           /* DEVICE [n] or NULL: 0, or AQ_ROW_* bits */
    int32_t   max_depth;        /* as aq_problem.max_depth */
    int32_t   reserved;
} aq_mesh_batch_io;
typedef struct {
    uint64_t n_nodes, leaves, tasks, invalid_rows;
    uint32_t levels, widest_level;
} aq_mesh_batch_info;
int aq_integrate_mesh_batch(aq_ctx *ctx, size_t n, const aq_mesh_batch_io *io, double eps, int integrand,
                            uint32_t frontier_cap, int sync_every, uint64_t cap_nodes, aq_mesh_batch_info *info);
int aq_mesh_eval_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_x, const double *d_f,
                       const double *d_cum, size_t nq_per_row, const double *d_q, double *d_out);
int aq_mesh_invert_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_x, const double *d_f,
                         const double *d_cum, size_t nq_per_row, const double *d_y, double *d_out);

/* ---- mesh refinement: a batch mesh continued to a smaller eps ---------------------------------------
 * aq_mesh_refine_batch takes the meshes aq_integrate_mesh_batch (or an earlier refinement) returned for n rows --
 * d_offsets [n + 1], d_x, d_f, d_level [offsets[n]]; cum is not read -- and returns in `out` the meshes of the same
 * rows at eps, without evaluating F again where the input already holds it. A mesh stores, bit for bit, what the
 * task step computed for every accepted task (l, mid, r, F(l), F(mid), F(r), its depth), and the tree at eps' <= eps
 * is a super-tree of the tree at eps, so:
 * Retest. Every input leaf of an active row (d_active[i] != 0; d_active NULL: every row) is retested with the three
 * area expressions of the task step and fabs((larea + rarea) - lrarea) > eps, one IEEE operation each. A leaf that
 * passes stays a leaf. A leaf at depth d that fails contributes its two children {l, mid, F(l), F(mid)} and
 * {mid, r, F(mid), F(r)} to the frontier of depth d + 1, and the tree goes on exactly as aq_integrate_mesh_batch
 * walks it. Rows that are not active keep all their leaves. A row without nodes stays without nodes: AQ_ROW_INVALID
 * in status, area NaN, accepted = tasks = 0.
 * Result. For active rows and eps no larger than the eps the input was built with, `out` is the mesh
 * aq_integrate_mesh_batch defines at eps: offsets, x, f and level bit for bit, every cum value within that call's
 * bound, and cum bit for bit as well whenever that call would hold the same leaves in every row (every row active).
 * With eps at or above the input's nothing fails: the output is the input and info->evaluated == 0.
 * out->a, out->b and out->theta are ignored; d_theta (DEVICE [n * aq_param_count()]) is non-NULL exactly for
 * AQ_F_PARAM. The inputs must not overlap the outputs and are not validated (as the query calls do not validate
 * theirs). Every mesh pointer is DEVICE memory of the context's device; the call blocks.
 * info: n_nodes, leaves and tasks (= 2 * leaves - rows with nodes) of the OUTPUT meshes; evaluated = the task steps
 * this call ran = evaluations of F = (tasks of the output trees) - (tasks of the input trees), whatever the mask;
 * reseeded = the input leaves that failed; levels = the deepest level + 1 of the output trees; widest_level = the
 * largest level of THIS run, the frontier_cap that suffices (roots never enter the frontier: it has no relation to n).
 * Capacity and errors, as aq_integrate_mesh_batch: past cap_nodes the trees are walked to their end, info->n_nodes is
 * reported and the return is AQ_EOVERFLOW; a level past frontier_cap is AQ_EOVERFLOW with n_nodes = 0; AQ_EDEPTH
 * when a failing leaf or a later task would refine at max_depth, with AQ_ROW_DEPTH on those rows. AQ_EINVAL: a NULL
 * ctx, info, out, offsets / x / f / cum of out, or input array (d_level among them: the depths come from it); a
 * theta that does not go with the integrand; a bad eps, max_depth or sync_every; frontier_cap < 2; cap_nodes < 3 or
 * > 2^31. n == 0: AQ_OK, info zeroed, nothing enqueued.
 * Device memory. The seed buffer (36 bytes per child of a failing leaf) and the depth table are context-owned,
 * allocated by the first such call and grown on demand; aq_ctx_device_bytes does not move before that call.
 * aq_mesh_err_batch gives, per row of a batch mesh, Σ|d| and Σd over its leaves, d = (larea + rarea) - lrarea
 * recomputed from the nodes, so every term is the reference's own double (:191) -- the error estimate of the _err
 * calls, from the mesh alone. The sums are carried in double-double and rounded once: each lies within accepted_i *
 * 2^-100 * Σ|d| of the exact sum before that rounding. The reduction's shape is fixed by the row's own leaf count
 * (no float atomics), so a row's sums are bit-identical from run to run and in whatever batch the row sits. A row
 * without nodes gives NaN. Either output may be NULL. The call only enqueues on the context's stream; its scratch
 * is context-owned. AQ_EINVAL: a NULL ctx, or a NULL input with n > 0.
 * Not covered: the single-mesh form (a batch of one row serves), shards and groups, the CLI, a C form
 * of the tolerance loop (Context.integrate_mesh_batch_tol drives these two calls round by round). */
typedef struct {
    uint64_t n_nodes, leaves, tasks;   /* of the OUTPUT meshes; tasks = 2 * leaves - rows with nodes */
    uint64_t evaluated;                /* task steps this call ran (= evaluations of F) */
    uint64_t reseeded;                 /* input leaves that failed the new test */
    uint32_t levels, widest_level;     /* deepest level + 1 of the output trees; the largest level of THIS run */
} aq_mesh_refine_info;
int aq_mesh_refine_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_x, const double *d_f,
                         const uint8_t *d_level, const double *d_theta, const uint8_t *d_active, double eps,
                         int integrand, const aq_mesh_batch_io *out, uint32_t frontier_cap, int sync_every,
                         uint64_t cap_nodes, aq_mesh_refine_info *info);
int aq_mesh_err_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_x, const double *d_f,
                      double *d_err_abs, double *d_err_signed);

/* ---- mesh coarsening: any coarser mesh, or a leaf budget, from a fine mesh ----------------------------
 * The converse of refinement: the tree at eps' >= eps is a sub-tree of the tree at eps, and everything its tasks
 * computed is stored in the fine mesh as node values, so every coarser mesh of a batch mesh (d_offsets [n + 1], d_x,
 * d_f, d_level [offsets[n]]; cum is not read) follows from the node arrays alone: no integrand, no theta, whatever
 * eps each row was built with. All pointers are DEVICE memory of the context's device. The three calls block; the
 * inputs are not validated (as the query calls do not validate theirs), but every index a kernel forms stays inside
 * its row's slice whatever bytes d_level holds.
 * Thresholds. An interior even node k of a row is the midpoint of exactly one internal node T of the row's tree;
 * thr[k] is the minimum over T and its ancestors of |d| = fabs((larea + rarea) - lrarea), the task step's three
 * expressions on the stored values, one IEEE operation each. aq_mesh_thresholds_batch writes, for k a node of row i
 * (local index, m_i the last): +inf at k == 0 and k == m_i, 0 at odd k, the threshold at even interior k. So x[k]
 * is a leaf bound of the row's mesh at eps' iff thr[k] > eps', for every eps' >= 0 (the strict > of the task step).
 * Budget. aq_mesh_budget_batch writes eps[i] = -1.0 when row i has at most max_leaves leaves (or no nodes), else
 * the max_leaves-th largest (1-based) threshold among its even interior nodes: coarsened at that eps the row has the
 * largest leaf count <= max_leaves that any eps gives -- exactly max_leaves unless thresholds tie there.
 * max_leaves >= 1, else AQ_EINVAL.
 * Coarsening. aq_mesh_coarsen_batch coarsens row i at e_i = d_eps ? d_eps[i] : eps; a row whose e_i is negative or
 * NaN is copied unchanged (the mask, and the -1 the budget call writes); a scalar eps that is negative or NaN with
 * d_eps == NULL is AQ_EINVAL. d_thr: the thresholds call's output, or NULL (computed into context scratch).
 * For e_i no smaller than the eps the row was built with, row i of `out` is the mesh aq_integrate_mesh_batch defines
 * at e_i: offsets, x, f, level, accepted, tasks and status bit for bit, every cum value within that call's bound
 * (restarting per row), and cum bit for bit that call's whenever every row holds the leaves one build would give (one
 * eps for all rows). For a smaller e_i nothing merges: the output row is the input row. A row without nodes stays
 * without nodes: AQ_ROW_INVALID, area NaN, accepted = tasks = 0. out->a, out->b, out->theta and out->max_depth are
 * ignored; the inputs must not overlap the outputs.
 * info: n_nodes, leaves and tasks (= 2 * leaves - rows with nodes) of the OUTPUT; merged = input leaves - output
 * leaves; levels = the deepest output level + 1.
 * Capacity. n_nodes > cap_nodes: AQ_EOVERFLOW with info->n_nodes reported and nothing written at or past cap_nodes
 * (offsets and the node arrays are then unspecified). The input's node count always suffices.
 * AQ_EINVAL: a NULL ctx, out, info, out->offsets, out->x, out->f or out->cum; a NULL input array with n > 0 (d_thr of
 * the thresholds and budget calls and d_eps of the budget call among them); cap_nodes < 3 or > 2^31; an input of more
 * than 2^31 nodes; n > 0x7fffffff. n == 0: AQ_OK, info zeroed, nothing enqueued.
 * Determinism. Every output of the three calls is bit-identical from run to run: the positions are an integer scan
 * without atomics, the thresholds a minimum, and the leaves are sorted by (row, l) before they are laid out.
 * Host looks. Each call reads the input's node count, offsets[n], first; the coarsen call also reads its output's
 * leaf count before the layout.
 * Device memory. 16 bytes of position per leaf, with its row, |d| and parent index (16 bytes more), the threshold
 * scratch when d_thr is NULL, and for the budget the mesh's sort arrays over the nodes; the coarsen call borrows the
 * leaf buffer and sort arrays of aq_integrate_mesh_batch. All of it is context-owned, allocated by the first of
 * these calls and grown on demand; aq_ctx_device_bytes does not move before that call, nor at a second call of the
 * same sizes.
 * Not covered: meshes from the persistent kernel, shards and groups, the CLI, a per-row max_leaves, enqueue-only
 * forms; a batch of few, huge rows -- the position scan runs one workgroup per row (a row's leaves / 256 steps in
 * turn) and the head of a merged leaf walks the leaves merged into it alone, so such a batch serialises; the calls are
 * for batches of many rows (the largest row measured has 15 573 leaves). */
typedef struct {
    uint64_t n_nodes, leaves, tasks;   /* of the OUTPUT meshes; tasks = 2 * leaves - rows with nodes */
    uint64_t merged;                   /* input leaves - output leaves */
    uint32_t levels, reserved;         /* deepest level + 1 of the output trees */
} aq_mesh_coarsen_info;
int aq_mesh_thresholds_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_x, const double *d_f,
                             const uint8_t *d_level, double *d_thr);
int aq_mesh_budget_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_thr, uint64_t max_leaves,
                         double *d_eps);
int aq_mesh_coarsen_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_x, const double *d_f,
                          const uint8_t *d_level, const double *d_thr, const double *d_eps, double eps,
                          const aq_mesh_batch_io *out, uint64_t cap_nodes, aq_mesh_coarsen_info *info);

/* ---- mesh moments: per row the integral of (x - c)^k F over any sub-range, from the mesh ----------------
 * M_k(i) = the integral over [lo_i, hi_i] of (x - c_i)^k fhat_i(x) dx, k = 0 .. order, where fhat_i is the
 * piecewise-linear function through row i's nodes (d_offsets [n + 1], d_x, d_f; cum and level are not read) -- the
 * function whose integral aq_mesh_eval returns. No evaluation of F: one pass over x and f. d_center, d_lo and d_hi
 * are DEVICE [n] or NULL (c_i = 0.0, lo_i = the row's x_0, hi_i = the row's x_m); d_out is DEVICE [n * (order + 1)],
 * row-major: M_0 .. M_order of row i.
 * The term of one panel with ends x0 < x1 and values g0, g1 (after clipping, below), every line one IEEE double
 * operation in this order (the library is built with -ffp-contract=off):
 *     u0 = x0 - c;  u1 = x1 - c;  w = x1 - x0;
 *     p0[0] = p1[0] = 1;  p0[i] = p0[i-1] * u0;  p1[i] = p1[i-1] * u1;
 *     s0 = s1 = 0.0;  for j = 0 .. k in increasing order:
 *         a = p0[k-j] * p1[j];  s0 = s0 + (double)(k+1-j) * a;  s1 = s1 + (double)(j+1) * a;
 *     t_k = (g0 * s0 + g1 * s1) * w / (double)((k+1)*(k+2));      (a true division)
 * For k = 0 this is (g0 + g1) * w / 2, the reference's larea and rarea (:189-190). The closed form is exact for a
 * linear g; the computed t_k lies within (3k + 8) * 2^-53 * T_k of it to first order, T_k = w (|g0| + |g1|)
 * max(|u0|, |u1|)^k / 2 (DESIGN 2.14 derives it).
 * Range. A row's range is valid when x_0 <= lo_i <= hi_i <= x_m. An invalid range (NaN included) or a row of fewer
 * than 3 nodes writes NaN to all order + 1 outputs of that row and disturbs no other row. lo_i == hi_i writes +0.0 to
 * all of them and touches no panel (a zero-width row such as [1, 1] is safe). Otherwise the panel that holds q (lo or
 * hi) is aq_mesh_eval's: the largest k <= m - 1 with x_k <= q, and the value there is aq_mesh_eval's expression
 * fq = f_k + (f_k+1 - f_k) * ((q - x_k) / (x_k+1 - x_k)), always from the full panel's two nodes; a q equal to a node
 * takes that node's stored f (hi at node x_k, k < m, ends the panel before it: no zero-width panel is added). A panel
 * wholly inside the range is never interpolated, panels outside contribute nothing, and lo and hi in one panel give
 * one clipped panel with both ends interpolated.
 * Sum. Each M_k is carried in double-double and rounded once: before that rounding it lies within P_i * 2^-100 *
 * sum |t_k| of the exact sum of the terms, P_i the panels in range. No float atomics: the reduction's shape depends
 * on the row's own panel count and on the indices of the panels that hold lo_i and hi_i, on nothing else, so a row's
 * outputs are bit-identical from run to run, in any batch, at any offset; and the outputs of an order = K call are,
 * bit for bit, the first K + 1 outputs of an order = 4 call.
 * The call only enqueues on the context's stream and reads nothing on the host; the inputs are not validated (every
 * index a kernel forms stays inside its row's slice). AQ_EINVAL: a NULL ctx; order outside 0 .. AQ_MESH_MAX_MOMENT
 * (whatever n); a NULL d_offsets, d_x, d_f or d_out with n > 0; an n that aq_mesh_err_batch refuses (n * 8 >= 2^31).
 * n == 0: AQ_OK, nothing enqueued.
 * Device memory. The block partials (8 * (order + 1) * 16 bytes per row) are context-owned and apart from
 * aq_mesh_err_batch's, so the two calls may follow each other without waiting; allocated by the first call and grown
 * on demand: aq_ctx_device_bytes does not move before that call, nor at a second call of the same n and order.
 * Not covered: orders above 4; weights other than powers; meshes from the persistent kernel; shards and groups; the
 * CLI; a single-mesh form (a batch of one row serves); a better deal of blocks for batches of few huge rows (eight
 * workgroups per row whatever its size, as aq_mesh_err_batch). */
#define AQ_MESH_MAX_MOMENT 4
int aq_mesh_moments_batch(aq_ctx *ctx, size_t n, const uint64_t *d_offsets, const double *d_x, const double *d_f,
                          int order,                   /* K, 0 .. AQ_MESH_MAX_MOMENT */
                          const double *d_center,      /* DEVICE [n] or NULL: c_i (NULL: 0.0) */
                          const double *d_lo,          /* DEVICE [n] or NULL: lo_i (NULL: the row's x_0) */
                          const double *d_hi,          /* DEVICE [n] or NULL: hi_i (NULL: the row's x_m) */
                          double *d_out);              /* DEVICE [n * (K + 1)] row-major: M_0 .. M_K of row i */

/* ---- measurement ----------------------------------------------------------------------------
 * When enabled, HIP events bracket every launch of the persistent kernel, and of aq_mesh_invert's kernel, on
 * the context's stream; aq_kernel_time returns the summed milliseconds and launch count since the last reset. */
int aq_kernel_timing(aq_ctx *ctx, int enable);
int aq_kernel_time(aq_ctx *ctx, double *total_ms, uint64_t *launches);
/* Per-workgroup timeline of the persistent kernel (48 uint64 words per workgroup: realtime stamps
 * in 100 MHz ticks -- entry, init, first seed, seeded, last round, first idle, termination seen,
 * loop exit, flushed, fold, exit -- rounds, tasks, chunks and records moved through the HBM queue,
 * seeds, max ring size, CU slot, active lanes summed over rounds, shader-clock cycles per round
 * phase and per seeding phase, records moved through the wave cellars; field names in
 * ppls_amd.Context.DIAG_FIELDS).
 * Runs an instrumented kernel variant. aq_diagnostics returns the number of workgroup records. */
int aq_set_diagnostics(aq_ctx *ctx, int enable);
int aq_diagnostics(aq_ctx *ctx, uint64_t *out, int cap_words);

/* ---- observable surface ----------------------------------------------------------------------
 * aq_print_reference prints exactly main()'s output (:107-117) for a result: "Area=%lf\n\nTasks Per
 * Process\n", then the index row and the count row, each entry followed by a tab. Entry 0 is the
 * farmer (always 0), entries 1..n_gpus the GPUs' tasks (res->tasks_per_gpu; one worker when NULL).
 * aq_print_reference_procs prints the same for any tasks_per_process[nprocs] (e.g. CUs dealt over
 * P-1 worker columns, the CLI's `-n P`). */
void aq_print_reference(FILE *f, const aq_result *res);
void aq_print_reference_procs(FILE *f, double area, const uint64_t *tasks_per_process, int nprocs);

#ifdef __cplusplus
}
#endif
#endif /* AQUAD_H */
