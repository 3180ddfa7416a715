// ================================================================================================
// Host side: the C ABI of include/aquad.h (included by aquad.hip after the kernels).
// ================================================================================================
#include "aq_host_args.h"   // the argument rules and the chunk schedule (no HIP: tests/test_host_args.py)
#include "aq_batch_plan.h"  // the batch pipelines, host and device-resident: steps, streams, events (no HIP:
                            // tests/test_batch_plan.py, tests/test_device_batch_plan.py)
#include "aq_frontier_walk.h"   // the frontier engine's host loop (no HIP: tests/test_frontier_walk.py)
#include "aq_host_mem.h"    // owning device / pinned buffers, events, streams

using namespace aq;

namespace {

#ifndef AQ_SYNC_SPIN
#define AQ_SYNC_SPIN 1   // synchronous calls wait on k_fetch_sync's sequence word, not the stream
#endif
constexpr int NSLOTS_ALL = NSLOTS + 1;
constexpr int NSTAGE = 4;          // pinned bounds staging buffers
constexpr unsigned QCAP = 16384;
constexpr double DEFAULT_STALL_MS = 10000.0;
constexpr int GROUP_SUM = XS_LIMBS + 3 + 2 * AQ_MAX_LEVELS;   // int64 words all-reduced per group run
static_assert(MAXK <= NSLOTS, "a launch's integrals need distinct slots");
static_assert(XS_LIMBS == AQ_XS_LIMBS, "aquad.h and aq_xsum.h disagree on the accumulator size");

#define AQ_HIP(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "aquad: HIP error %s at %s:%d\n", hipGetErrorString(e_),   \
                    __FILE__, __LINE__);                                              \
            return AQ_EHIP;                                                           \
        }                                                                             \
    } while (0)

#define AQ_NCCL(call)                                                                 \
    do {                                                                              \
        ncclResult_t r_ = (call);                                                     \
        if (r_ != ncclSuccess) {                                                      \
            fprintf(stderr, "aquad: RCCL error %s at %s:%d\n", ncclGetErrorString(r_), \
                    __FILE__, __LINE__);                                              \
            return AQ_ERCCL;                                                          \
        }                                                                             \
    } while (0)

static_assert(HB_TIMEOUT == ERRB_TIMEOUT && HB_OVERFLOW == ERRB_OVERFLOW && HB_DEPTH == ERRB_DEPTH,
              "aq_host_args.h and aq_device.h disagree on the error bits");

bool integrand_ok(int f) { return f == AQ_F_COSH4 || f == AQ_F_SIN_RECIP || f == AQ_F_USER; }

// (The supported domain -- bounds_ok, params_ok -- is aq_domain.h's: one predicate for these host checks and
// the device-resident batch's check kernel.)

int validate(const aq_problem* p) {
    if (!p) return AQ_EINVAL;
    if (!integrand_ok(p->integrand)) return AQ_EINVAL;
    if (!bounds_ok(p->integrand, p->a, p->b)) return AQ_EINVAL;
    if (!(p->eps >= 0.0)) return AQ_EINVAL;
    if (p->max_depth < 0 || p->max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    if (p->n_gpus < 0) return AQ_EINVAL;
    return AQ_OK;
}

// Host view of one finished integral, whichever path produced it.
struct HostOut {
    double area = 0.0;
    unsigned long long tasks = 0, leaves = 0, spilled = 0;
    unsigned levels = 0, error = 0;
    unsigned long long hist[2 * AQ_MAX_LEVELS] = {};
    unsigned long long cu[AQ_CU_SLOTS] = {};
};

// The device rings both batch pipelines keep, each its own set (a call of the host batch may follow a
// device-resident one still in flight without waiting): two chunks, indexed by chunk parity and `R` rows apart
// -- bounds, theta, size order and its permutation -- and one chunk's size keys. Who may touch which parity
// when: aq_batch_plan.h.
struct BatchRings {
    DevBuf<double2> bounds;     // [2][R]
    DevBuf<double2> sorted;     // [2][R] the chunk's bounds in size order (k_batch_scatter)
    DevBuf<unsigned> key;       // [R] size class per integral (k_batch_estimate)
    DevBuf<unsigned> perm;      // [2][R] sorted position -> integral
    DevBuf<unsigned> cnt;       // [2] x (EST_KEYS counts + EST_KEYS cursors)
    DevBuf<double> est;         // [2] the chunk's sum of size estimates
    DevBuf<double> theta;       // [2][R][nparams] (the first AQ_F_PARAM call)
    DevBuf<double> thsorted;    // [2][R][nparams] (k_batch_scatter_theta)
    size_t R = 0;               // the current call's rows per parity
    bool par = false;           // ... and whether theta rows travel in it
    explicit BatchRings(unsigned long long* bytes)
        : bounds{bytes}, sorted{bytes}, key{bytes}, perm{bytes}, cnt{bytes}, est{bytes}, theta{bytes}, thsorted{bytes} {}

    // for a call with chunks of at most `rows` (grow-only: nothing happens once they hold as much)
    int grow(size_t rows, bool par_) {
        constexpr size_t NP = (size_t)param::nparams;
        R = rows, par = par_;
        AQ_HIP(bounds.grow(2 * R));
        AQ_HIP(sorted.grow(2 * R));
        AQ_HIP(key.grow(R));
        AQ_HIP(perm.grow(2 * R));
        AQ_HIP(cnt.grow(4 * EST_KEYS));
        AQ_HIP(est.grow(2));
        if (par) {
            AQ_HIP(theta.grow(NP * 2 * R));
            AQ_HIP(thsorted.grow(NP * 2 * R));
        }
        return AQ_OK;
    }

    // chunk c's places in the rings (null where the call has none: theta)
    struct View {
        double2 *bounds, *sorted;
        unsigned *perm, *cnt, *cnt_next;   // (cnt_next, est_next: the other parity's, which the scatter zeroes)
        double *est, *est_next, *theta, *thsorted;
    };
    View at(size_t c) const {
        constexpr size_t NP = (size_t)param::nparams;
        const size_t p = c & 1u;
        return View{bounds + p * R, sorted + p * R, perm + p * R, cnt + 2 * EST_KEYS * p, cnt + 2 * EST_KEYS * (p ^ 1u),
                    est + p, est + (p ^ 1u), par ? theta + p * R * NP : nullptr, par ? thsorted + p * R * NP : nullptr};
    }
};

// The host batch's buffers (aq_integrate_batch, _params, _err): the rings for the largest chunk so far (grow-only
// up to MAXK rows, whatever n: ADVICE r5 -- they had been sized to the whole batch, 72 B per integral), with rings
// of rows {area, tasks, accepted, error} and error sums beside them; the pinned host copies cover the whole call
// (grow-only).
struct HostBatch : BatchRings {
    DevBuf<double> rows;        // [2][R][4]
    DevBuf<double> errrows;     // [2][R][2] {err_abs, err_signed} (the first aq_integrate_batch_err)
    PinBuf<double> h_rows;      // [n][4]
    PinBuf<double2> h_bounds;   // [n]
    PinBuf<double> h_theta;     // [n][nparams]
    PinBuf<double> h_errrows;   // [n][2]
    bool err = false;           // error rows travel in the current call
    explicit HostBatch(unsigned long long* bytes) : BatchRings{bytes}, rows{bytes}, errrows{bytes} {}

    // for a call of n integrals in chunks of at most `chunk_rows`, with theta rows (par_) and error rows (err_)
    int grow(size_t chunk_rows, size_t n, bool par_, bool err_) {
        constexpr size_t NP = (size_t)param::nparams;
        if (int rc = BatchRings::grow(chunk_rows, par_)) return rc;
        err = err_;
        AQ_HIP(rows.grow(8 * R));
        AQ_HIP(h_rows.grow(4 * n));
        AQ_HIP(h_bounds.grow(n));
        if (par) AQ_HIP(h_theta.grow(NP * n));
        if (err) {
            AQ_HIP(errrows.grow(4 * R));
            AQ_HIP(h_errrows.grow(2 * n));
        }
        return AQ_OK;
    }
    double* rows_at(size_t c) const { return rows + 4 * (c & 1u) * R; }
    double* errrows_at(size_t c) const { return err ? errrows + 2 * (c & 1u) * R : nullptr; }
};

// The device-resident batch's buffers (aq_integrate_batch_device): the rings, the check kernel's flag ring, what
// aq_device_batch_check reads, and the events its plan names -- the context's, reused from call to call, because
// the call returns while they are pending. The rings hold two chunks of MAXK rows whatever the call's size: they
// are allocated once, by the context's first such call (theta and its size-ordered copy by the first AQ_F_PARAM
// one), and no later call allocates, frees or waits.
struct DevBatch : BatchRings {
    DevBuf<unsigned> flag;            // [2][R]
    DevBuf<DevBatchStat> stat;        // one: invalid rows and error bits since the last aq_device_batch_check
    PinBuf<DevBatchStat> h_stat;      // its pinned copy
    std::vector<Event> ev;            // by the plan's event numbers (grow-only)
    explicit DevBatch(unsigned long long* bytes) : BatchRings{bytes}, flag{bytes}, stat{bytes} {}

    int ensure(bool par_, size_t n_events) {
        if (int rc = BatchRings::grow((size_t)MAXK, par_)) return rc;
        AQ_HIP(flag.grow(2 * R));
        if (!stat) {
            AQ_HIP(h_stat.alloc(1, true));
            AQ_HIP(stat.alloc(1, true));
        }
        while (ev.size() < n_events) {
            ev.emplace_back();
            AQ_HIP(ev.back().create(hipEventDisableTiming));
        }
        return AQ_OK;
    }
    unsigned* flags(size_t c) const { return flag + (c & 1u) * R; }
};

// aq_integrate_batch_tol's buffers, for its largest block so far (grow-only up to MAXK rows): the live rows'
// bounds, theta and original indices in two ping-pong halves (a round's survivors are compacted from one into
// the other), a round's gathered rows, its survivor flags and per-workgroup counts, and the block's retired
// records; pinned: the staging of a block's bounds and theta, its records' copy, and the survivors' count and
// first indices.
struct TolBufs {
    DevBuf<double2> bounds;      // [2][rows]
    DevBuf<double> theta;        // [2][rows][nparams] (AQ_F_PARAM calls only)
    DevBuf<unsigned> idx;        // [2][rows]
    DevBuf<double> rows;         // [rows][4] (k_gather_reset)
    DevBuf<double> err;          // [rows][2] (k_gather_err)
    DevBuf<unsigned char> flag;  // [rows]
    DevBuf<unsigned> cnt;        // [ceil(rows / TOL_T)] survivors per workgroup
    DevBuf<double> tsum;         // [ceil(rows / TOL_T)] ... and their tasks
    DevBuf<double> res;          // [rows][TOL_REC]
    PinBuf<double2> h_bounds;    // [rows]
    PinBuf<double> h_theta;      // [rows][nparams]
    PinBuf<double> h_res;        // [rows][TOL_REC]
    PinBuf<TolSurv> h_surv;      // coherent: k_tol_compact's target
    TolSurv* d_surv = nullptr;   // its device address
    explicit TolBufs(unsigned long long* bytes)
        : bounds{bytes}, theta{bytes}, idx{bytes}, rows{bytes}, err{bytes}, flag{bytes}, cnt{bytes}, tsum{bytes},
          res{bytes} {}

    // for blocks of `n` rows, on the first such call (a context that never made one holds none of these:
    // aq_ctx_device_bytes does not move until then)
    int ensure(size_t n, bool par) {
        constexpr size_t NP = (size_t)param::nparams;
        AQ_HIP(bounds.grow(2 * n));
        AQ_HIP(idx.grow(2 * n));
        AQ_HIP(rows.grow(4 * n));
        AQ_HIP(err.grow(2 * n));
        AQ_HIP(flag.grow(n));
        AQ_HIP(cnt.grow((n + TOL_T - 1) / TOL_T));
        AQ_HIP(tsum.grow((n + TOL_T - 1) / TOL_T));
        AQ_HIP(res.grow(TOL_REC * n));
        AQ_HIP(h_bounds.grow(n));
        AQ_HIP(h_res.grow(TOL_REC * n));
        if (par) {
            AQ_HIP(theta.grow(2 * NP * n));
            AQ_HIP(h_theta.grow(NP * n));
        }
        if (!h_surv) {
            AQ_HIP(h_surv.alloc(1, true, hipHostMallocCoherent | hipHostMallocMapped));
            AQ_HIP(hipHostGetDevicePointer((void**)&d_surv, h_surv, 0));
        }
        return AQ_OK;
    }
};

// The frontier engine's buffers: the two frontier buffers a level step reads and writes in turn, the records per
// depth (allocated at create: aq_integrate_levels counts there too), and a walk's accumulator (walk_run), with the
// pinned copies of the last two.
struct FrontBufs {
    unsigned long long* const bytes;   // the counter the device buffers count in (aq_ctx::dev_bytes)
    DevBuf<Rec> d_rec[2] = {DevBuf<Rec>{bytes}, DevBuf<Rec>{bytes}};   // both of one size, or neither
    DevBuf<unsigned> d_count{bytes};   // [AQ_MAX_LEVELS + 2]
    PinBuf<unsigned> h_count;
    DevBuf<double> d_acc{bytes};       // 8 doubles (k_level_fold's layout)
    PinBuf<double> h_acc;

    // The two frontier buffers hold at least cap records each. They only grow; a failed allocation leaves
    // neither, so the two always hold the same count and no caller launches on half a pair.
    int ensure_front(size_t cap) {
        if (d_rec[0].grow(cap) == hipSuccess && d_rec[1].grow(cap) == hipSuccess) return AQ_OK;
        d_rec[0].reset();
        d_rec[1].reset();
        fprintf(stderr, "aquad: no device memory for two frontier buffers of %zu records\n", cap);
        return AQ_EHIP;
    }
    // ... and what a walk over them needs beside
    int ensure_walk(size_t cap) {
        if (int rc = ensure_front(cap)) return rc;
        AQ_HIP(d_acc.grow(8));
        AQ_HIP(h_count.grow(AQ_MAX_LEVELS + 2));
        AQ_HIP(h_acc.grow(8));
        return AQ_OK;
    }
};

// The accepted mesh's buffers, each allocated by the first call that needs it and grown on demand (a context that
// made no such call holds none: aq_ctx_device_bytes does not move until then). The batch of meshes runs in the
// single mesh's leaf, sort and partial arrays and adds its own; refinement runs in the batch's and adds its own.
struct MeshBufs {
    unsigned long long* const bytes;   // the counter the device buffers count in (aq_ctx::dev_bytes)
    // the single mesh (aq_integrate_mesh)
    DevBuf<Leaf> d_leaf{bytes};                    // leaf records in schedule order
    DevBuf<unsigned long long> d_leafcnt{bytes};   // accepted tasks counted by the emitting kernels (one word)
    DevBuf<double> d_mkey[2] = {DevBuf<double>{bytes}, DevBuf<double>{bytes}};       // sort keys in / out
    DevBuf<unsigned> d_midx[2] = {DevBuf<unsigned>{bytes}, DevBuf<unsigned>{bytes}}; // leaf indices in / out
    DevBuf<unsigned char> d_msort{bytes};          // the sort's scratch
    DevBuf<double2> d_mparts{bytes};               // the scan's block partials
    // the batch of meshes (aq_integrate_mesh_batch)
    DevBuf<unsigned> d_brow[2] = {DevBuf<unsigned>{bytes}, DevBuf<unsigned>{bytes}};   // the frontier records' rows
    DevBuf<unsigned> d_bkey[2] = {DevBuf<unsigned>{bytes}, DevBuf<unsigned>{bytes}};   // the second sort's keys in / out
    DevBuf<unsigned> d_bfirst{bytes};              // [n + 1] every row's first sorted leaf
    DevBuf<unsigned> d_bnode{bytes};               // a sorted leaf's first node | its row's head bit
    DevBuf<unsigned> d_bpflag{bytes};              // the segmented scan's "block has a head"
    DevBuf<unsigned> d_bstatus{bytes};             // [n] the rows' status when the caller wants none
    DevBuf<unsigned long long> d_binvalid{bytes};  // rows that failed the check (one word)
    PinBuf<unsigned long long> h_bwords;           // pinned: the leaf count and the invalid rows
    // mesh refinement (aq_mesh_refine_batch)
    DevBuf<Rec> d_rseed{bytes};                    // the failing leaves' children, one segment per depth
    DevBuf<unsigned> d_rseedrow{bytes};            // ... and their rows
    DevBuf<unsigned> d_rtab{bytes};                // the depth table (aquad.hip REFINE_TAB_*)
    PinBuf<unsigned> h_rtab;                       // pinned copy
    PinBuf<unsigned long long> h_rnodes;           // pinned: the input's node count (one word)
    DevBuf<double4> d_eparts{bytes};               // aq_mesh_err_batch's block partials (its first call)
    DevBuf<double2> d_momparts{bytes};             // aq_mesh_moments_batch's block partials (its first call)
    // mesh coarsening (aq_mesh_thresholds_batch, aq_mesh_budget_batch, aq_mesh_coarsen_batch)
    DevBuf<ulonglong2> d_cpos{bytes};              // a leaf's 128-bit position, at slot (its first node) >> 1
    DevBuf<unsigned> d_crow{bytes};                // ... its row (0xffffffff: no leaf's slot)
    DevBuf<double> d_cdabs{bytes};                 // ... |d| of the internal node whose midpoint the leaf starts at
    DevBuf<unsigned> d_cpar{bytes};                // ... and the leaf at that node's parent's midpoint (0: none)
    DevBuf<double> d_cthr{bytes};                  // the thresholds, when the caller passes none

    // the leaf buffer of a run that may emit cap_leaves, and its count
    int ensure_leaves(size_t cap_leaves) {
        AQ_HIP(d_leaf.grow(cap_leaves));
        AQ_HIP(d_leafcnt.grow(1));
        return AQ_OK;
    }
    // the sort of nl leaves by l and the scan over `grid` blocks of them; for a batch of `rows` > 0 also the
    // segmented scan's arrays and, with more than one row, the second pass by row
    int ensure_sort(size_t nl, size_t sort_bytes, size_t grid, size_t rows = 0) {
        for (int k = 0; k < 2; ++k) {
            AQ_HIP(d_mkey[k].grow(nl));
            AQ_HIP(d_midx[k].grow(nl));
            if (rows > 1) AQ_HIP(d_bkey[k].grow(nl));
        }
        AQ_HIP(d_msort.grow(std::max<size_t>(sort_bytes, 1)));
        AQ_HIP(d_mparts.grow(grid));
        if (rows > 0) {
            AQ_HIP(d_bpflag.grow(grid));
            AQ_HIP(d_bnode.grow(nl));
        }
        return AQ_OK;
    }
    // a walk of n rows over a frontier of cap records (own_status: the caller gave no status array; refine: with
    // refinement's depth table)
    int ensure_batch(size_t n, size_t cap, size_t cap_leaves, bool own_status, bool refine) {
        for (int k = 0; k < 2; ++k) AQ_HIP(d_brow[k].grow(cap));
        if (int rc = ensure_leaves(cap_leaves)) return rc;
        AQ_HIP(d_binvalid.grow(1));
        AQ_HIP(d_bfirst.grow(n + 1));
        if (own_status) AQ_HIP(d_bstatus.grow(n));
        AQ_HIP(h_bwords.grow(2));
        if (refine) {
            AQ_HIP(d_rtab.grow(REFINE_TAB_WORDS));
            AQ_HIP(h_rtab.grow(REFINE_TAB_WORDS));
            AQ_HIP(h_rnodes.grow(1));
        }
        return AQ_OK;
    }
    // the thresholds of a mesh of m nodes (own_thr: into d_cthr)
    int ensure_coarsen(size_t m, bool own_thr) {
        const size_t slots = (m + 1) / 2;
        AQ_HIP(h_rnodes.grow(1));
        AQ_HIP(d_cpos.grow(slots));
        AQ_HIP(d_crow.grow(slots));
        AQ_HIP(d_cdabs.grow(slots));
        AQ_HIP(d_cpar.grow(slots));
        if (own_thr) AQ_HIP(d_cthr.grow(m));
        return AQ_OK;
    }
};

}  // namespace

struct aq_ctx {
    int device = 0;
    int num_cus = 0;
    int grid = 0;                      // persistent workgroups per launch (one per CU, or AQ_GRID)
    std::unique_ptr<HostPool> pool;    // the batch front end's host threads (created on first use)
    int occ[4][2][6] = {};             // k_stream<FID,HIST> by Variant: resident workgroups per CU (0: not asked yet)
    bool coop = false;                 // AQ_COOP=1: cooperative launches
    bool histograms = true;
    double stall_ms = DEFAULT_STALL_MS;
    // Every buffer, event and stream below frees itself (aq_host_mem.h); the streams come first, so they are
    // destroyed last. DevBuf<T> x{&dev_bytes} counts in aq_ctx_device_bytes, DevBuf<T> x{} does not.
    unsigned long long dev_bytes = 0;  // device memory held
    Stream stream;
    Stream s_h2d, s_d2h, s_pre;        // the batch front end's copy and pre-pass streams (created on first use)
    DevBuf<ExpPair> d_tab{&dev_bytes};
    DevBuf<Ctl> d_ctl{&dev_bytes};     // NSLOTS control blocks (totals, exact area, histograms)
    DevBuf<QCtl> d_q{&dev_bytes};      // two queue / termination blocks, used by launches in turn
    int qsel = 0;                      // the block the next launch uses
    DevBuf<unsigned long long> d_parts{&dev_bytes};   // (NPARTS + 1) x grid per-workgroup pack_cu words (per-CU
                                                      // launches into slots < NPARTS, and the sync slot: parts_row)
    DevBuf<double> d_parea{&dev_bytes};               // ... and their area words (PCU_AREA: a double-double per workgroup)
    bool dirty[NSLOTS_ALL] = {};       // slot's sums / area used since they were last reset
    bool parts_dirty[NSLOTS_ALL] = {}; // slot's per-workgroup words written (per-CU launches)
    bool slot_hist[NSLOTS_ALL] = {};
    DevBuf<double2> d_bounds{&dev_bytes};   // NSLOTS {a, b}
    DevBuf<int> d_shard{&dev_bytes};   // NSLOTS per-integral shard (mixed launches)
    PinBuf<double2> h_bounds;          // pinned staging ring, NSTAGE x NSLOTS (a launch's copy may still be
                                       // pending when the host queues the next launch)
    PinBuf<int> h_shard;               // pinned staging ring, NSTAGE x NSLOTS
    Event stage_ev[NSTAGE];            // recorded after each staging copy
    int stage = 0;
    DevBuf<Chunk> d_chunks{&dev_bytes};
    DevBuf<Cellar> d_cellar{&dev_bytes};   // grid * NW per-wave HBM overflow stacks
    DevBuf<unsigned> d_ready{&dev_bytes};
    unsigned epoch = 0;
    DevBuf<LaunchHint> d_hint{&dev_bytes};   // job-size hint carried from launch to launch
    HintState hint;                    // the workload the hint was measured on (aq_launch_plan.h)
    int gsplit_env = 0;                // AQ_GSPLIT: waves per job of a multi-integral launch (0 = default)
    // level path
    DevBuf<DevResults> d_lres{&dev_bytes};
    FrontBufs front{&dev_bytes};       // the frontier pair, its per-depth counts and a walk's accumulator
    DevBuf<LevelPart> d_lparts{&dev_bytes};   // frontier engine: per-block partials of one level step
    bool defer_fold = false;           // aq_level_defer_fold: level steps leave their rows for one later fold
    int level_grid = 0;                // aq_level_step's grid cap (MAXB, or AQ_LEVEL_GRID), set at create
    int lp_pending = 0;                // level-step rows written and not yet folded
    double* lp_acc = nullptr;          // ... into this accumulator (the caller's)
    MeshBufs mesh{&dev_bytes};         // the accepted mesh, single, batched and refined (grown by those calls)
    HostBatch batch{&dev_bytes};       // the batch front end's rings and pinned copies (grown by its calls)
    // per-integral parameters (AQ_F_PARAM), allocated by the first parametrised call (ensure_params): NSLOTS + 1
    // rows on the device beside d_bounds, and their pinned staging ring
    DevBuf<double> d_theta{&dev_bytes};      // [NSLOTS_ALL][nparams]
    PinBuf<double> h_theta;                  // pinned staging ring, NSTAGE x NSLOTS x nparams
    // error estimate (the ERR launches, aq_*_err), allocated by the first ERR call (ensure_err): the slots' two sums
    DevBuf<double> d_err{&dev_bytes};  // [NSLOTS_ALL][2] = Σ|d|, Σd over the slot's accepted tasks
    PinBuf<double> h_err;              // one pair (aq_fetch_err)
    bool err_dirty[NSLOTS_ALL] = {};   // slot's pair written since it was last zeroed
    bool slot_err[NSLOTS_ALL] = {};    // slot's last launch was an ERR launch (beside slot_hist)
    int occ_err[4][6] = {};            // the ERR instances' resident workgroups per CU, by Variant (as occ)
    TolBufs tol{&dev_bytes};           // aq_integrate_batch_tol's buffers (allocated by its first call)
    DevBatch devbatch{&dev_bytes};     // aq_integrate_batch_device's rings and events (allocated by its first call)
    // eval buffers (not counted)
    DevBuf<double> d_x, d_y;
    // host staging
    PinBuf<unsigned long long> h_parts;   // grid words
    PinBuf<SlotSums> h_sums;           // one
    PinBuf<XSum> h_area;               // one
    PinBuf<unsigned long long> h_hist; // 2 * AQ_MAX_LEVELS
    PinBuf<DevResults> h_lres;
    PinBuf<SyncOut> h_sync;            // coherent: k_fetch_sync's target (the synchronous path)
    SyncOut* d_sync = nullptr;         // its device address
    unsigned long long sync_seq = 0;   // the last synchronous call's sequence number (SyncOut::seq)
    HostOut last;
    bool last_valid = false;
    // diagnostics
    DevBuf<unsigned long long> d_diag;                // (not counted)
    DevBuf<unsigned long long> d_cu_acc{&dev_bytes};  // [AQ_CU_SLOTS] tasks per CU slot since the last reset (every launch)
    // timing
    bool timing = false;
    std::vector<std::pair<Event, Event>> ev_pending;
    std::vector<std::pair<Event, Event>> ev_free;
    double timed_ms = 0.0;
    unsigned long long timed_launches = 0;
};

namespace {

// Return slots [s, s+k) to the all-zero state if any was used since it was last reset (k_reset:
// sums, exact area, queue words; histograms when written). Per-workgroup words (per-CU launches only)
// need no clearing: readers use them only while the slot's `pcu` flag is set (k_reset clears it), and
// the per-CU launch that sets it stores every workgroup's words (r03: the memset that cleared them
// had put a fill kernel before every lone launch on a reused slot).
int ensure_clean(aq_ctx* c, int s, int k) {
    // (byte flags scanned and set with memchr / memset: a 262144-slot launch's flag loops had cost the
    // host ~0.1 ms in front of the launch)
    if (memchr(c->dirty + s, 1, (size_t)k)) {
        bool hist = false;
        for (int i = s; i < s + k; ++i) hist |= c->dirty[i] && c->slot_hist[i];
        hipLaunchKernelGGL(k_reset, dim3(k), dim3(128), 0, c->stream, c->d_ctl, s, hist ? 1 : 0);
        AQ_HIP(hipGetLastError());
        memset(c->dirty + s, 0, (size_t)k);
    }
    memset(c->parts_dirty + s, 0, (size_t)k);
    // the slots' error sums (ERR launches): zero again before any launch into them
    if (c->d_err && memchr(c->err_dirty + s, 1, (size_t)k)) {
        AQ_HIP(hipMemsetAsync(c->d_err + 2 * (size_t)s, 0, 2 * sizeof(double) * (size_t)k, c->stream));
        memset(c->err_dirty + s, 0, (size_t)k);
    }
    return AQ_OK;
}

// f(std::integral_constant<int, F_...>{}) for an AQ_F_* integrand: the one place where the run-time
// integrand becomes the kernels' FID template argument (`decltype(F)::value` in a generic lambda).
template <typename Fn>
auto with_fid(int integrand, Fn&& f) {
    switch (integrand) {
        case AQ_F_COSH4: return f(std::integral_constant<int, F_COSH4>{});
        case AQ_F_SIN_RECIP: return f(std::integral_constant<int, F_SIN_RECIP>{});
        default: return f(std::integral_constant<int, F_USER>{});
    }
}

// The k_stream instance of a plan's variant. The lone instance exists only where plan_launch picks it: not
// for the skewed integrand, and not when AQ_LONE_NW is NW (there LONE names the per-CU instance itself).
template <int FID, bool HIST>
const void* stream_kernel(Variant v) {
    constexpr bool lone_ok = FID != F_SIN_RECIP && AQ_LONE_NW != NW;
    switch (v) {
        case Variant::DIAG_PCU: return (const void*)k_stream<FID, HIST, true, true>;
        case Variant::DIAG: return (const void*)k_stream<FID, HIST, true, false>;
        case Variant::PCU: return (const void*)k_stream<FID, HIST, false, true>;
        case Variant::PLAIN: return (const void*)k_stream<FID, HIST, false, false>;
        case Variant::LONE: return (const void*)k_stream<FID, HIST, false, true, lone_ok ? AQ_LONE_NW : NW>;
        case Variant::HEAP: return (const void*)k_stream<FID, HIST, false, false, NW, true>;
    }
    return nullptr;
}

// ... and of an ERR launch's plan: three instances per integrand, all without histograms and diagnostics at
// ERR_NW waves per workgroup -- per-CU (the plan's PCU and LONE), plain, heap.
template <int FID>
const void* stream_kernel_err(Variant v) {
    switch (v) {
        case Variant::PCU:
        case Variant::LONE: return (const void*)k_stream<FID, false, false, true, ERR_NW, false, true>;
        case Variant::PLAIN: return (const void*)k_stream<FID, false, false, false, ERR_NW, false, true>;
        case Variant::HEAP: return (const void*)k_stream<FID, false, false, false, ERR_NW, true, true>;
        default: return nullptr;   // (an ERR plan names no DIAG variant)
    }
}

// Kernel timing (aq_kernel_timing / aq_kernel_time): a launch's event pair, reused from the free list, its
// first event recorded ahead of the launch and its second after it; aq_kernel_time reads the pending pairs.
using EventPair = std::pair<Event, Event>;
int timing_begin(aq_ctx* ctx, EventPair& ev) {
    if (!ctx->timing) return AQ_OK;
    if (!ctx->ev_free.empty()) {
        ev = std::move(ctx->ev_free.back());
        ctx->ev_free.pop_back();
    } else {
        AQ_HIP(ev.first.create());
        AQ_HIP(ev.second.create());
    }
    AQ_HIP(hipEventRecord(ev.first, ctx->stream));
    return AQ_OK;
}
int timing_end(aq_ctx* ctx, EventPair& ev) {
    if (!ctx->timing) return AQ_OK;
    AQ_HIP(hipEventRecord(ev.second, ctx->stream));
    ctx->ev_pending.push_back(std::move(ev));
    return AQ_OK;
}

// One persistent launch: k integrals of one integrand into slots first_slot ...
struct LaunchArgs {
    int integrand = AQ_F_COSH4;          // AQ_F_*
    int k = 0;
    const double* a = nullptr;           // the k bounds on the host
    const double* b = nullptr;
    const int32_t* shard_of = nullptr;   // per-integral shard of nshards (nullptr: every integral is shard `shard`)
    double eps = 0.0;
    int max_depth = 0, shard = 0, nshards = 1, first_slot = 0;
    const double2* dev_bounds = nullptr; // the k {a, b} already on the device (the batch front end copies them ahead
                                         // on its own stream), else they are staged and copied by the launch
    const double* theta = nullptr;       // AQ_F_PARAM: the k parameter rows on the host (staged and copied by the
                                         // launch, per-CU launches too: theta is not a kernel argument), or
    const double* dev_theta = nullptr;   // ... already on the device in the launch's order (the batch front end)
    bool err = false;                    // an ERR launch (its instances keep no histograms, whatever `hist`)
    bool hist = false;                   // per-level histograms (the callers pass ctx->histograms; the batch none)
    bool heap = false;                   // the batch front end's launches: the heap-seeding instance (HEAPS)
    bool sync_fold = false;              // a per-CU launch's reader folds its area words itself (k_fetch_sync,
                                         // k_pack_group): no k_fold_parts after it
};

// The launch's shape -- instance, waves, shares, seed depth, tail, job mode -- is plan_launch's
// (aq_launch_plan.h); this enqueues it.
template <int FID, bool HIST>
int launch_stream(aq_ctx* ctx, const LaunchArgs& g) {
    static_assert(FID >= 0 && FID < 4, "aq_ctx::occ holds one row per integrand");
    const int k = g.k, max_depth = g.max_depth, shard = g.shard, nshards = g.nshards, first_slot = g.first_slot;
    const double eps = g.eps, *a = g.a, *b = g.b, *theta = g.theta, *dev_theta = g.dev_theta;
    const int32_t* shard_of = g.shard_of;
    const double2* dev_bounds = g.dev_bounds;
    const bool err = g.err;
    // an ERR launch's instances keep no histograms (launch passes HIST = false); ctx->d_err exists
    if (err && (HIST || !ctx->d_err)) return AQ_EINVAL;
    constexpr int NP = param::nparams;
    const bool stage_theta = FID == F_PARAM && !dev_theta;
    if (FID == F_PARAM && !theta && !dev_theta) return AQ_EINVAL;
    const int G = ctx->grid;
    const LaunchRequest rq{FID, G, k, shard_of != nullptr, nshards, first_slot, ctx->d_diag != nullptr,
                           g.heap, ctx->gsplit_env, eps, err};
    const LaunchPlan plan = plan_launch(rq, ctx->hint);
    if (plan.rc) return plan.rc;   // refused before anything is enqueued
    // per-CU launches pass their bounds as kernel arguments: no staging copy
    const bool pcu = plan.per_cu != 0;
    const void* kfn = plan.err ? stream_kernel_err<FID>(plan.variant) : stream_kernel<FID, HIST>(plan.variant);
    if (!kfn) return AQ_EINVAL;
    // Co-residency (VERDICT r3 #6): idle workgroups wait on the HBM queue for busy ones, so the whole
    // grid must be resident at once. The device's answer for this exact instance (its VGPRs, its
    // static LDS, PT threads) times the CUs must cover the grid -- checked before anything is
    // enqueued, refused with a code instead of a stall. (Other kernels sharing the device, e.g. RCCL's,
    // can still delay some workgroups' start; the no-progress stall bound then ends the launch.)
    int& occ = plan.err ? ctx->occ_err[FID][(int)plan.variant] : ctx->occ[FID][HIST][(int)plan.variant];
    if (occ == 0) {
        AQ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, plan.nwt * 64, 0));
        if (occ < 1) occ = -1;
    }
    if (occ < 1 || (long long)occ * ctx->num_cus < (long long)G) return AQ_ERESIDENT;
    int rc = ensure_clean(ctx, first_slot, k);
    if (rc) return rc;
    if ((!pcu && !dev_bounds) || shard_of || stage_theta) {
        const int st = ctx->stage;
        ctx->stage = (st + 1) % NSTAGE;
        AQ_HIP(hipEventSynchronize(ctx->stage_ev[st]));   // the copy that last used this buffer is done
        if (!pcu && !dev_bounds) {
            double2* hb = ctx->h_bounds + (size_t)st * NSLOTS;
            for (int i = 0; i < k; ++i) hb[i] = make_double2(a[i], b[i]);
            AQ_HIP(hipMemcpyAsync(ctx->d_bounds + first_slot, hb, sizeof(double2) * (size_t)k,
                                  hipMemcpyHostToDevice, ctx->stream));
        }
        if (shard_of) {
            int* hs = ctx->h_shard + (size_t)st * NSLOTS;
            for (int i = 0; i < k; ++i) hs[i] = shard_of[i];
            AQ_HIP(hipMemcpyAsync(ctx->d_shard + first_slot, hs, sizeof(int) * (size_t)k, hipMemcpyHostToDevice,
                                  ctx->stream));
        }
        if (stage_theta) {
            double* ht = ctx->h_theta + (size_t)st * NSLOTS * NP;
            memcpy(ht, theta, sizeof(double) * (size_t)k * NP);
            AQ_HIP(hipMemcpyAsync(ctx->d_theta + (size_t)first_slot * NP, ht, sizeof(double) * (size_t)k * NP,
                                  hipMemcpyHostToDevice, ctx->stream));
        }
        AQ_HIP(hipEventRecord(ctx->stage_ev[st], ctx->stream));
    }
    StreamParams P{};
    P.bounds = dev_bounds ? dev_bounds : ctx->d_bounds + first_slot;
    P.shard_of = shard_of ? ctx->d_shard + first_slot : nullptr;
    P.nprob = k;
    P.first_slot = first_slot;
    P.eps = eps;
    P.max_depth = max_depth ? max_depth : AQ_DEFAULT_MAX_DEPTH;
    P.shard = shard;
    P.nshards = nshards;
    P.shares = plan.shares;
    P.D = plan.D;
    P.tail_from = plan.tail_from;
    P.tail_mult = plan.tail_mult;
    P.epoch = ++ctx->epoch;
    if (P.epoch == 0) P.epoch = ++ctx->epoch;
    P.qcap = QCAP;
    P.stall_ticks = (unsigned long long)(ctx->stall_ms * 1e5);   // 100 MHz realtime clock
    P.ctls = ctx->d_ctl;
    P.q = ctx->d_q + ctx->qsel;
    P.q_next = ctx->d_q + (ctx->qsel ^ 1);
    P.parts = ctx->d_parts + 2 * parts_row(first_slot) * ctx->grid;
    P.parea = ctx->d_parea + 2 * parts_row(first_slot) * ctx->grid;
    if (plan.err) P.err = ctx->d_err;   // (shares diag's word: an ERR launch runs no DIAG instance)
    else P.diag = ctx->d_diag;
    P.cu_acc = ctx->d_cu_acc;
    P.chunks = ctx->d_chunks;
    P.cellar = ctx->d_cellar;
    P.ready = ctx->d_ready;
    P.hint = ctx->d_hint;
    P.per_cu = plan.per_cu;
    P.static_jobs = plan.static_jobs;
    if (pcu)
        for (int i = 0; i < k; ++i) P.kbounds[i] = make_double2(a[i], b[i]);
    P.adaptive = plan.adaptive;
    if (FID == F_PARAM) P.theta = dev_theta ? dev_theta : ctx->d_theta + (size_t)first_slot * NP;
    ctx->hint = plan.hint;   // (committed before the launch: a failing launch leaves the new state)
    EventPair ev;
    if ((rc = timing_begin(ctx, ev))) return rc;
    void* args[] = {&P};
    if (ctx->coop)
        AQ_HIP(hipLaunchCooperativeKernel(kfn, dim3(G), dim3(plan.nwt * 64), args, 0, ctx->stream));
    else
        AQ_HIP(hipLaunchKernel(kfn, dim3(G), dim3(plan.nwt * 64), args, 0, ctx->stream));
    ctx->qsel ^= 1;   // the launch zeroes the other block for the next one
    if ((rc = timing_end(ctx, ev))) return rc;
    // a per-CU launch leaves its area in per-workgroup words (PCU_AREA): folded into the slots here, for
    // every reader, unless the synchronous path's own read-back folds them (k_fetch_sync, k_pack_group)
    if (pcu && !g.sync_fold) {
        hipLaunchKernelGGL(k_fold_parts, dim3(k), dim3(256), 0, ctx->stream, ctx->d_ctl, (const double*)P.parea,
                           ctx->grid, first_slot);
        AQ_HIP(hipGetLastError());
    }
    memset(ctx->dirty + first_slot, 1, (size_t)k);
    if (pcu) memset(ctx->parts_dirty + first_slot, 1, (size_t)k);
    memset(ctx->slot_hist + first_slot, HIST ? 1 : 0, (size_t)k);
    memset(ctx->slot_err + first_slot, plan.err ? 1 : 0, (size_t)k);
    if (plan.err) memset(ctx->err_dirty + first_slot, 1, (size_t)k);
    return AQ_OK;
}

// The parametrised family's buffers, on the first parametrised call (a fresh context holds none of them:
// aq_ctx_device_bytes does not move until then).
int ensure_params(aq_ctx* ctx) {
    if (ctx->d_theta) return AQ_OK;
    constexpr size_t NP = (size_t)param::nparams;
    AQ_HIP(ctx->h_theta.grow(NP * NSLOTS * NSTAGE));
    AQ_HIP(ctx->d_theta.alloc(NP * NSLOTS_ALL, false));
    return AQ_OK;
}

// The error estimate's slot sums, on the first ERR call (a fresh context and the plain calls hold none of
// them: aq_ctx_device_bytes does not move until then). Zeroed once; ensure_clean and the readers keep the
// slots zero between launches.
int ensure_err(aq_ctx* ctx) {
    if (ctx->d_err) return AQ_OK;
    AQ_HIP(ctx->h_err.grow(2));
    AQ_HIP(ctx->d_err.alloc(2 * (size_t)NSLOTS_ALL, true));
    return AQ_OK;
}

// with_fid for the stream launches and the batch of meshes: AQ_F_PARAM too (with_fid stays the three fixed
// integrands': the only level kernel instantiated for id 3 is the batch form, k_level_step<F_PARAM, BatchSink>)
template <typename Fn>
auto with_stream_fid(int integrand, Fn&& f) {
    if (integrand == AQ_F_PARAM) return f(std::integral_constant<int, F_PARAM>{});
    return with_fid(integrand, f);
}

// Enqueue one launch, with the buffers its family needs.
int launch(aq_ctx* ctx, const LaunchArgs& g) {
    int rc;
    if (g.err && (rc = ensure_err(ctx))) return rc;
    if (g.integrand == AQ_F_PARAM && (rc = ensure_params(ctx))) return rc;
    return with_stream_fid(g.integrand, [&](auto F) {
        constexpr int FID = decltype(F)::value;
        return g.hist && !g.err ? launch_stream<FID, true>(ctx, g) : launch_stream<FID, false>(ctx, g);
    });
}

// Per-CU counts of one GPU in hardware-slot order (the aq_result.tasks_per_cu row).
void cu_row(const unsigned long long* cu, uint64_t* row, int n) {
    int k = 0;
    for (int s = 0; s < AQ_CU_SLOTS && k < n; ++s)
        if (cu[s]) row[k++] = cu[s];
    for (; k < n; ++k) row[k] = 0;
}

void fill_result(const aq_ctx* ctx, const HostOut& h, aq_result* out) {
    if (!out) return;
    out->area = h.area;
    out->tasks = h.tasks;
    out->accepted = h.leaves;
    out->levels = h.levels;
    out->spilled = h.spilled;
    unsigned n = 0;
    for (int i = 0; i < AQ_CU_SLOTS; ++i) n += h.cu[i] ? 1u : 0u;
    out->n_cu = n;
    out->n_gpus = 1;
    if (out->tasks_per_gpu) out->tasks_per_gpu[0] = h.tasks;
    if (out->tasks_per_cu) cu_row(h.cu, out->tasks_per_cu, ctx->num_cus);
}

// A slot's result from host copies of its sums, exact limbs, per-workgroup words (per-CU launches,
// else nullptr) and histograms (else nullptr): ctx->last (the "last call" of aq_tasks_per_cu /
// aq_level_histogram) and *out.
static int finish_fetch(aq_ctx* ctx, SlotSums sm, const XSum& area, const unsigned long long* parts,
                        const unsigned long long* hist, aq_result* out) {
    HostOut& h = ctx->last;
    h = HostOut();
    h.area = xs_round(area);
    if (!parts) sm.pcu = 0;
    const Counts k = slot_counts(sm, parts, ctx->grid);
    h.tasks = k.tasks;
    h.leaves = k.leaves;
    h.spilled = sm.spilled;
    h.levels = k.levels;
    h.error = sm.error;
    if (parts) {   // per-CU counts: lone-integral launches keep per-workgroup words
        for (int i = 0; i < ctx->grid; ++i) {
            const unsigned long long w = parts[2 * i];
            h.cu[w & ((1u << CU_BITS) - 1u)] += w >> CU_BITS;
        }
    }
    if (hist) memcpy(h.hist, hist, sizeof(h.hist));
    ctx->last_valid = true;
    fill_result(ctx, h, out);
    return err_from_bits(h.error);
}

// Copy a slot's words into the pinned staging and wait for them: its sums and exact area, its per-workgroup
// words if a per-CU launch wrote them, its histograms if asked for and kept. *sm: the sums, their `pcu` flag
// cleared unless the per-workgroup words came along.
int read_slot(aq_ctx* ctx, int slot, bool hist, SlotSums* sm) {
    if (ctx->parts_dirty[slot])
        AQ_HIP(hipMemcpyAsync(ctx->h_parts, ctx->d_parts + 2 * parts_row(slot) * ctx->grid,
                              2 * sizeof(unsigned long long) * (size_t)ctx->grid, hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(ctx->h_sums, &ctx->d_ctl[slot].sums, sizeof(SlotSums), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(ctx->h_area, &ctx->d_ctl[slot].area, sizeof(XSum), hipMemcpyDeviceToHost, ctx->stream));
    if (hist && ctx->slot_hist[slot])
        AQ_HIP(hipMemcpyAsync(ctx->h_hist, ctx->d_ctl[slot].hist, sizeof(unsigned long long) * 2 * AQ_MAX_LEVELS,
                              hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    *sm = *ctx->h_sums;
    if (!ctx->parts_dirty[slot]) sm->pcu = 0;
    return AQ_OK;
}

int fetch_slot(aq_ctx* ctx, int slot, aq_result* out) {
    SlotSums sm;
    const int rc = read_slot(ctx, slot, true, &sm);
    if (rc) return rc;
    return finish_fetch(ctx, sm, *ctx->h_area, ctx->parts_dirty[slot] ? ctx->h_parts.get() : nullptr,
                        ctx->slot_hist[slot] ? ctx->h_hist.get() : nullptr, out);
}

// a slot's exact row (aq_fetch_exact): limbs, tasks, accepted, spilled, levels | error bits << 32
int fetch_exact_slot(aq_ctx* ctx, int slot, int64_t* row) {
    SlotSums s;
    const int rc = read_slot(ctx, slot, false, &s);
    if (rc) return rc;
    for (int i = 0; i < XS_LIMBS; ++i) row[i] = ctx->h_area->limb[i];
    const Counts k = slot_counts(s, ctx->h_parts, ctx->grid);
    row[XS_LIMBS] = (int64_t)k.tasks;
    row[XS_LIMBS + 1] = (int64_t)k.leaves;
    row[XS_LIMBS + 2] = (int64_t)s.spilled;
    row[XS_LIMBS + 3] = (int64_t)k.levels | ((int64_t)s.error << 32);
    return err_from_bits(s.error);
}

// Wait for k_fetch_sync's sequence number in pinned host memory: a spin on one coherent word, with a
// stream query every 256 spins so that a failed launch is reported instead of waited on; past 2 ms (a
// long launch: the spin would only hold a host core) the stream synchronisation takes over.
static bool wait_sync_seq(aq_ctx* ctx, unsigned long long want) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned n = 1;; ++n) {
        if (__atomic_load_n(&ctx->h_sync->seq, __ATOMIC_ACQUIRE) == want) return true;
        if ((n & 255u) == 0u) {
            const hipError_t e = hipStreamQuery(ctx->stream);
            if (e == hipSuccess) return __atomic_load_n(&ctx->h_sync->seq, __ATOMIC_ACQUIRE) == want;
            if (e != hipErrorNotReady) return false;
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
                if (hipStreamSynchronize(ctx->stream) != hipSuccess) return false;
                return __atomic_load_n(&ctx->h_sync->seq, __ATOMIC_ACQUIRE) == want;
            }
        }
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
    }
}

// The synchronous calls' read-back of SYNC_SLOT: one k_fetch_sync launch writes the result into
// pinned host memory and zeroes the slot; the host waits for its sequence number there
// (AQ_SYNC_SPIN; 0: a stream synchronisation).
// err: the call was an ERR launch -- its two sums come back in the same pinned result (SyncOut::err, written by
// k_fetch_sync_err just ahead) and are zeroed too.
static int fetch_sync(aq_ctx* ctx, aq_result* out, aq_err* err = nullptr) {
    const bool wp = ctx->parts_dirty[SYNC_SLOT], wh = ctx->slot_hist[SYNC_SLOT];
    const unsigned long long seq = ++ctx->sync_seq;
    if (err)   // the two sums first: in the pinned result before k_fetch_sync releases the sequence number
        hipLaunchKernelGGL(k_fetch_sync_err, dim3(1), dim3(64), 0, ctx->stream, ctx->d_err + 2 * (size_t)SYNC_SLOT,
                           ctx->d_sync);
    hipLaunchKernelGGL(k_fetch_sync, dim3(1), dim3(256), 0, ctx->stream, ctx->d_ctl + SYNC_SLOT,
                       ctx->d_parts + 2 * parts_row(SYNC_SLOT) * ctx->grid,
                       (const double*)(ctx->d_parea + 2 * parts_row(SYNC_SLOT) * ctx->grid), ctx->grid, wp ? 1 : 0,
                       wh ? 1 : 0, ctx->d_sync, seq);
    AQ_HIP(hipGetLastError());
    if (AQ_SYNC_SPIN) {
        if (!wait_sync_seq(ctx, seq)) {
            (void)hipStreamSynchronize(ctx->stream);
            return AQ_EHIP;
        }
    } else {
        AQ_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->dirty[SYNC_SLOT] = ctx->parts_dirty[SYNC_SLOT] = ctx->slot_hist[SYNC_SLOT] = false;
    const SyncOut& o = *ctx->h_sync;
    if (err) {
        ctx->err_dirty[SYNC_SLOT] = ctx->slot_err[SYNC_SLOT] = false;
        err->err_abs = o.err[0];
        err->err_signed = o.err[1];
    }
    return finish_fetch(ctx, o.sums, o.area, wp ? o.parts : nullptr, wh ? o.hist : nullptr, out);
}

}  // namespace

// The RCCL group (aq_integrate_group). The vectors hold one entry per member driven by this process.
struct aq_group {
    int nranks = 0;
    int grid = 0;
    std::vector<aq_ctx*> ctx;
    std::vector<int> rank;                // their ranks
    std::vector<ncclComm_t> comm;         // (null until the communicator exists)
    std::vector<DevBuf<long long>> d_sum;            // GROUP_SUM int64 (all-reduced in place)
    std::vector<DevBuf<unsigned long long>> d_mine;  // 3 + grid words (this rank's contribution)
    std::vector<DevBuf<unsigned long long>> d_all;   // nranks * (3 + grid) words (all-gathered)
    PinBuf<long long> h_sum;              // pinned copies of member 0's results
    PinBuf<unsigned long long> h_all;

    aq_group(int nranks_, int members) : nranks(nranks_), comm(members, nullptr), d_sum(members), d_mine(members),
                                         d_all(members) {}
};

namespace {

int group_alloc(aq_group* g) {
    const size_t info = 3 + (size_t)g->grid;
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        AQ_HIP(hipSetDevice(g->ctx[m]->device));
        AQ_HIP(g->d_sum[m].alloc(GROUP_SUM, false));
        AQ_HIP(g->d_mine[m].alloc(info, false));
        AQ_HIP(g->d_all[m].alloc(info * g->nranks, false));
    }
    AQ_HIP(g->h_sum.alloc(GROUP_SUM, false));
    AQ_HIP(g->h_all.alloc(info * g->nranks, false));
    return AQ_OK;
}

// The end of aq_group_create / aq_group_join, after the communicator's `init` call returned r: the group's
// buffers, and the group published -- or destroyed.
int group_finish(aq_group* g, ncclResult_t r, const char* init, aq_group** out) {
    int rc = AQ_OK;
    if (r != ncclSuccess) {
        fprintf(stderr, "aquad: %s: %s\n", init, ncclGetErrorString(r));
        g->comm.assign(g->comm.size(), nullptr);
        rc = AQ_ERCCL;
    } else {
        rc = group_alloc(g);
    }
    if (rc) {
        aq_group_destroy(g);
        return rc;
    }
    *out = g;
    return AQ_OK;
}

}  // namespace

extern "C" {

#if AQ_STAMPS
// diagnostic builds only (AQ_STAMPS=1): the per-wave timelines of the last plain launch
// (ST_STRIDE words per wave, waves in workgroup-major order; tools/stamps_single.py)
int aq_debug_stamps(uint64_t* out, size_t words) {
    if (words > sizeof(g_aq_stamps) / 8) return AQ_EINVAL;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_aq_stamps), words * 8, 0, hipMemcpyDeviceToHost) != hipSuccess) return AQ_EHIP;
    return AQ_OK;
}
#endif

// test support (not in include/aquad.h): the seed depth of a job of V = shares x shards virtual
// workers (aq_stream.h seed_depth_job), so the CPU tests can pin the oracle partition's restatement
// of it (tests/conftest.py device_seed_S) without a GPU
int aq_seed_depth(unsigned long long V) { return V ? seed_depth_job(V) : -1; }

const char* aq_strerror(int code) {
    switch (code) {
        case AQ_OK: return "ok";
        case AQ_EINVAL: return "invalid argument";
        case AQ_EHIP: return "HIP runtime error";
        case AQ_ETIMEOUT: return "on-device wait made no progress within the stall bound";
        case AQ_EOVERFLOW: return "frontier / work-queue capacity exceeded";
        case AQ_EDEPTH: return "maximum refinement depth reached";
        case AQ_ENOMEM: return "out of memory";
        case AQ_ENODEV: return "no HIP device";
        case AQ_ERCCL: return "RCCL error";
        case AQ_ERESIDENT: return "the persistent grid cannot be co-resident on the device";
        case AQ_ENOCONV: return "an integral missed its tolerance within max_rounds";
        default: return "unknown error";
    }
}

const char* aq_user_integrand_name(void) { return user::name; }

int aq_param_count(void) { return param::nparams; }

const char* aq_param_integrand_name(void) { return param::name; }

int aq_device_count(int* count) {
    if (!count) return AQ_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return n > 0 ? AQ_OK : AQ_ENODEV;
}

constexpr int MAXB = 8192;            // level-step grid cap (grid-stride beyond); AQ_LEVEL_GRID sets a smaller one
constexpr int LP_CAP = 8 * MAXB;      // level-step rows held for one deferred fold

static int ctx_init(aq_ctx* c, int device) {
    c->device = device;
    AQ_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    AQ_HIP(hipGetDeviceProperties(&prop, device));
    c->num_cus = prop.multiProcessorCount;
    int occ = 0;
    AQ_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)k_stream<F_COSH4, true, false, false>, PT, 0));
    if (occ < 1) return AQ_ENODEV;
    // One workgroup per CU (the LDS rings take most of a CU's LDS); the whole grid must be
    // resident, because idle workgroups wait on the queue for busy ones.
    c->grid = std::min(c->num_cus, MAXG);
    if (const char* e = getenv("AQ_GRID")) {
        const int g = atoi(e);
        if (g > 0) c->grid = std::min(g, MAXG);
    }
    if (const char* e = getenv("AQ_COOP")) c->coop = atoi(e) != 0;
    if (const char* e = getenv("AQ_GSPLIT")) c->gsplit_env = atoi(e);
    if (const char* e = getenv("AQ_STALL_MS")) {
        const double v = atof(e);
        if (v > 0) c->stall_ms = v;
    }
    c->level_grid = MAXB;
    if (const char* e = getenv("AQ_LEVEL_GRID")) c->level_grid = std::min(std::max(atoi(e), 1), MAXB);
    AQ_HIP(c->stream.create());
    const size_t G = (size_t)c->grid;
    AQ_HIP(c->d_tab.alloc(128, false));
    AQ_HIP(hipMemcpy(c->d_tab, aq_exp_tab_host, sizeof(ExpPair) * 128, hipMemcpyHostToDevice));
    AQ_HIP(c->d_ctl.alloc(NSLOTS_ALL, true));
    AQ_HIP(c->d_parts.alloc(2 * (size_t)(NPARTS + 1) * G, true));
    AQ_HIP(c->d_parea.alloc(2 * (size_t)(NPARTS + 1) * G, true));
    AQ_HIP(c->d_bounds.alloc(NSLOTS_ALL, false));
    AQ_HIP(c->d_shard.alloc(NSLOTS_ALL, false));
    AQ_HIP(c->d_hint.alloc(1, true));
    AQ_HIP(c->d_q.alloc(2, true));
    AQ_HIP(c->d_cu_acc.alloc(AQ_CU_SLOTS, true));
    AQ_HIP(c->h_bounds.alloc((size_t)NSLOTS * NSTAGE, false));
    AQ_HIP(c->h_shard.alloc((size_t)NSLOTS * NSTAGE, false));
    for (Event& e : c->stage_ev) {
        AQ_HIP(e.create(hipEventDisableTiming));
        AQ_HIP(hipEventRecord(e, c->stream));
    }
    AQ_HIP(c->d_chunks.alloc(QCAP, false));
    AQ_HIP(c->d_cellar.alloc(G * NW, false));
    AQ_HIP(c->d_ready.alloc((size_t)QCAP * READY_STRIDE, true));
    AQ_HIP(c->h_parts.alloc(2 * G, false));
    AQ_HIP(c->h_sums.alloc(1, false));
    AQ_HIP(c->h_area.alloc(1, false));
    AQ_HIP(c->h_hist.alloc(2 * AQ_MAX_LEVELS, false));
    AQ_HIP(c->h_lres.alloc(1, false));
    AQ_HIP(c->h_sync.alloc(1, true, hipHostMallocCoherent | hipHostMallocMapped));
    AQ_HIP(hipHostGetDevicePointer((void**)&c->d_sync, c->h_sync, 0));
    AQ_HIP(c->d_lres.alloc(1, false));
    AQ_HIP(c->front.d_count.alloc(AQ_MAX_LEVELS + 2, false));
    AQ_HIP(hipDeviceSynchronize());
    return AQ_OK;
}

int aq_ctx_create(int device, aq_ctx** out) {
    if (!out) return AQ_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AQ_ENODEV;
    if (device < 0 || device >= n) return AQ_EINVAL;
    aq_ctx* c = new aq_ctx();
    const int rc = ctx_init(c, device);
    if (rc) {   // release whatever was allocated before the failure
        aq_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return AQ_OK;
}

void aq_ctx_destroy(aq_ctx* c) {
    if (!c) return;
    c->pool.reset();
    (void)hipSetDevice(c->device);
    for (const Stream* s : {&c->stream, &c->s_h2d, &c->s_pre, &c->s_d2h})
        if (*s) (void)hipStreamSynchronize(*s);
    delete c;   // (the members free themselves: aq_host_mem.h)
}

int aq_ctx_num_cus(const aq_ctx* c) { return c ? c->num_cus : 0; }
int aq_ctx_num_workers(const aq_ctx* c) { return c ? c->grid * NW : 0; }

int aq_ctx_device_bytes(const aq_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return AQ_EINVAL;
    *bytes = c->dev_bytes;
    return AQ_OK;
}

int aq_set_level_histograms(aq_ctx* c, int enable) {
    if (!c) return AQ_EINVAL;
    c->histograms = enable != 0;
    return AQ_OK;
}

int aq_set_stall_timeout(aq_ctx* c, double ms) {
    if (!c || !(ms > 0.0) || ms > 1e9) return AQ_EINVAL;
    c->stall_ms = ms;
    return AQ_OK;
}

int aq_set_diagnostics(aq_ctx* c, int enable) {
    if (!c) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(c->device));
    AQ_HIP(hipStreamSynchronize(c->stream));
    if (enable && !c->d_diag) AQ_HIP(c->d_diag.alloc((size_t)DIAG_WORDS * MAXG, true));
    if (!enable) c->d_diag.reset();
    return AQ_OK;
}

int aq_diagnostics(aq_ctx* c, uint64_t* out, int cap_words) {
    if (!c || !out || !c->d_diag) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(c->device));
    const size_t words = std::min<size_t>((size_t)cap_words, (size_t)DIAG_WORDS * c->grid);
    AQ_HIP(hipStreamSynchronize(c->stream));
    AQ_HIP(hipMemcpy(out, c->d_diag, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return (int)(words / DIAG_WORDS);
}

int aq_async_slots(void) { return NSLOTS; }

int aq_max_integrals_per_launch(void) { return MAXK; }

// theta goes with AQ_F_PARAM and with nothing else
static bool theta_ok(int integrand, const double* theta) {
    return integrand == AQ_F_PARAM ? theta != nullptr : (integrand_ok(integrand) && theta == nullptr);
}

// Every launch entry point's end: the argument rules (the ranges of aq_host_args.h, each integral's domain and
// shard), then the launch with the context's histogram setting. The synchronous calls pass NSLOTS_ALL as the
// slot limit (SYNC_SLOT).
static int checked_launch(aq_ctx* ctx, LaunchArgs g, int slot_limit = NSLOTS) {
    if (!ctx || !g.a || !g.b || !theta_ok(g.integrand, g.theta)) return AQ_EINVAL;
    if (!launch_ranges_ok(g.k, g.eps, g.max_depth, g.shard, g.nshards, g.shard_of != nullptr, g.first_slot, slot_limit))
        return AQ_EINVAL;
    for (int i = 0; i < g.k; ++i) {
        if (g.theta ? !params_ok(g.a[i], g.b[i], g.theta + (size_t)i * param::nparams)
                    : !bounds_ok(g.integrand, g.a[i], g.b[i]))
            return AQ_EINVAL;
        if (g.shard_of && (g.shard_of[i] < 0 || g.shard_of[i] >= g.nshards)) return AQ_EINVAL;
    }
    AQ_HIP(hipSetDevice(ctx->device));
    g.hist = ctx->histograms;
    return launch(ctx, g);
}

// the arguments of k integrals as one shard
static LaunchArgs many_args(int integrand, int k, const double* a, const double* b, const double* theta, double eps,
                            int max_depth, int shard, int nshards, int first_slot) {
    LaunchArgs g;
    g.integrand = integrand;
    g.k = k;
    g.a = a;
    g.b = b;
    g.theta = theta;
    g.eps = eps;
    g.max_depth = max_depth;
    g.shard = shard;
    g.nshards = nshards;
    g.first_slot = first_slot;
    return g;
}

// ... and of a synchronous call's one integral, into SYNC_SLOT
static LaunchArgs sync_args(const aq_problem* p, const double* theta, int shard, int nshards) {
    return many_args(p->integrand, 1, &p->a, &p->b, theta, p->eps, p->max_depth, shard, nshards, SYNC_SLOT);
}

int aq_integrate_many_async(aq_ctx* ctx, int integrand, int k, const double* a, const double* b, double eps,
                            int max_depth, int shard, int nshards, int first_slot) {
    return checked_launch(ctx, many_args(integrand, k, a, b, nullptr, eps, max_depth, shard, nshards, first_slot));
}

int aq_integrate_mixed_async(aq_ctx* ctx, int integrand, int k, const double* a, const double* b,
                             const int32_t* shard, int nshards, double eps, int max_depth, int first_slot) {
    if (!shard) return AQ_EINVAL;
    if (nshards == 1) {
        // whole integrals (shard 0 of 1 each, e.g. dist.py's whole-integral units): an unsharded launch,
        // which sizes its jobs adaptively and fills the waves when the integrals are few
        for (int i = 0; i < k; ++i)
            if (shard[i] != 0) return AQ_EINVAL;
        shard = nullptr;
    }
    LaunchArgs g = many_args(integrand, k, a, b, nullptr, eps, max_depth, 0, nshards, first_slot);
    g.shard_of = shard;
    return checked_launch(ctx, g);
}

int aq_integrate_async(aq_ctx* ctx, const aq_problem* p, int shard, int nshards, int slot) {
    if (!ctx) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    return aq_integrate_many_async(ctx, p->integrand, 1, &p->a, &p->b, p->eps, p->max_depth, shard, nshards, slot);
}

int aq_gather_results(aq_ctx* ctx, int first_slot, int n, void* d_out) {
    if (!ctx || !d_out || !slot_range_ok(first_slot, n)) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_gather, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, ctx->d_ctl, ctx->d_parts, ctx->grid,
                       first_slot, n, NSLOTS, (double*)d_out);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

int aq_gather_exact(aq_ctx* ctx, int first_slot, int n, void* d_out) {
    if (!ctx || !d_out || !slot_range_ok(first_slot, n)) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_gather_exact, dim3(n), dim3(64), 0, ctx->stream, ctx->d_ctl, ctx->d_parts, ctx->grid,
                       first_slot, n, NSLOTS, (long long*)d_out);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

int aq_fetch(aq_ctx* ctx, int slot, aq_result* res) {
    if (!ctx || slot < 0 || slot >= NSLOTS) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    return fetch_slot(ctx, slot, res);
}

int aq_fetch_exact(aq_ctx* ctx, int slot, int64_t* row) {
    if (!ctx || !row || slot < 0 || slot >= NSLOTS) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    return fetch_exact_slot(ctx, slot, row);
}

double aq_exact_round(const int64_t* limbs) {
    if (!limbs) return 0.0;
    XSum x;
    for (int i = 0; i < XS_LIMBS; ++i) x.limb[i] = limbs[i];
    return xs_round(x);
}

static int fold_pending(aq_ctx* ctx);

int aq_synchronize(aq_ctx* ctx) {
    if (!ctx) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    const int rc = fold_pending(ctx);   // deferred level-step rows (aq_level_defer_fold)
    if (rc) return rc;
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return AQ_OK;
}

// A synchronous call: the launch into SYNC_SLOT and its read-back (err: an ERR launch, its sums into *err).
static int sync_call(aq_ctx* ctx, const aq_problem* p, const double* theta, int shard, int nshards, aq_result* res,
                     aq_err* err) {
    LaunchArgs g = sync_args(p, theta, shard, nshards);
    g.err = err != nullptr;
    g.sync_fold = true;   // fetch_sync's k_fetch_sync folds the per-CU area words itself
    const int rc = checked_launch(ctx, g, NSLOTS_ALL);
    return rc ? rc : fetch_sync(ctx, res, err);
}

int aq_integrate_shard(aq_ctx* ctx, const aq_problem* p, int shard, int nshards, aq_result* res) {
    if (!ctx) return AQ_EINVAL;
    const int rc = validate(p);
    return rc ? rc : sync_call(ctx, p, nullptr, shard, nshards, res, nullptr);
}

int aq_integrate_shard_exact(aq_ctx* ctx, const aq_problem* p, int shard, int nshards, int64_t* row) {
    if (!ctx || !row) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    if ((rc = checked_launch(ctx, sync_args(p, nullptr, shard, nshards), NSLOTS_ALL))) return rc;
    // the slot stays marked used: the next launch into it resets it first (ensure_clean)
    return fetch_exact_slot(ctx, SYNC_SLOT, row);
}

int aq_integrate(aq_ctx* ctx, const aq_problem* p, aq_result* res) {
    if (p && p->n_gpus > 1) return AQ_EINVAL;   // several GPUs: aq_integrate_group
    return aq_integrate_shard(ctx, p, 0, 1, res);
}

// ---- per-integral parameters (AQ_F_PARAM) -----------------------------------------------------------
int aq_integrate_many_params_async(aq_ctx* ctx, int k, const double* a, const double* b, const double* theta,
                                   double eps, int max_depth, int shard, int nshards, int first_slot) {
    return checked_launch(ctx, many_args(AQ_F_PARAM, k, a, b, theta, eps, max_depth, shard, nshards, first_slot));
}

int aq_integrate_params(aq_ctx* ctx, const aq_problem* p, const double* theta, aq_result* res) {
    if (!ctx || !p || !theta) return AQ_EINVAL;
    if (p->integrand != AQ_F_PARAM || p->n_gpus > 1 || p->n_gpus < 0) return AQ_EINVAL;
    return sync_call(ctx, p, theta, 0, 1, res, nullptr);
}

// ---- error estimate (the ERR launches) -----------------------------------------------------------------
double aq_err_extrapolate(double area, const aq_err* e) { return e ? area + e->err_signed / 3.0 : area; }

int aq_integrate_many_err_async(aq_ctx* ctx, int integrand, int k, const double* a, const double* b, const double* theta,
                                double eps, int max_depth, int shard, int nshards, int first_slot) {
    LaunchArgs g = many_args(integrand, k, a, b, theta, eps, max_depth, shard, nshards, first_slot);
    g.err = true;
    return checked_launch(ctx, g);
}

int aq_integrate_err(aq_ctx* ctx, const aq_problem* p, const double* theta, aq_result* res, aq_err* err) {
    if (!ctx || !p || !res || !err) return AQ_EINVAL;
    if (!theta_ok(p->integrand, theta) || p->n_gpus > 1) return AQ_EINVAL;
    if (!theta) {
        const int rc = validate(p);
        if (rc) return rc;
    } else if (p->n_gpus < 0) {
        return AQ_EINVAL;
    }
    return sync_call(ctx, p, theta, 0, 1, res, err);
}

int aq_fetch_err(aq_ctx* ctx, int slot, aq_err* err) {
    if (!ctx || !err || slot < 0 || slot >= NSLOTS) return AQ_EINVAL;
    if (!ctx->d_err || !ctx->slot_err[slot]) return AQ_EINVAL;   // the slot's last launch was no ERR launch
    AQ_HIP(hipSetDevice(ctx->device));
    AQ_HIP(hipMemcpyAsync(ctx->h_err, ctx->d_err + 2 * (size_t)slot, 2 * sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    err->err_abs = ctx->h_err[0];
    err->err_signed = ctx->h_err[1];
    return AQ_OK;
}

// (aq_integrate_batch_err: beside the batch front end, below)

// ---- RCCL group ----------------------------------------------------------------------------------
int aq_group_unique_id(void* id) {
    if (!id) return AQ_EINVAL;
    ncclUniqueId u;
    AQ_NCCL(ncclGetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return AQ_OK;
}

int aq_group_create(aq_ctx* const* ctxs, int n, aq_group** out) {
    if (!ctxs || !out || n < 1) return AQ_EINVAL;
    *out = nullptr;
    std::vector<int> devs;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i] || ctxs[i]->grid != ctxs[0]->grid) return AQ_EINVAL;
        for (int d : devs)
            if (d == ctxs[i]->device) return AQ_EINVAL;   // one context per GPU
        devs.push_back(ctxs[i]->device);
    }
    aq_group* g = new aq_group(n, n);
    g->grid = ctxs[0]->grid;
    for (int i = 0; i < n; ++i) {
        g->ctx.push_back(ctxs[i]);
        g->rank.push_back(i);
    }
    return group_finish(g, ncclCommInitAll(g->comm.data(), n, devs.data()), "ncclCommInitAll", out);
}

int aq_group_join(aq_ctx* ctx, int nranks, int rank, const void* id, aq_group** out) {
    if (!ctx || !id || !out || nranks < 1 || rank < 0 || rank >= nranks) return AQ_EINVAL;
    *out = nullptr;
    AQ_HIP(hipSetDevice(ctx->device));
    aq_group* g = new aq_group(nranks, 1);
    g->grid = ctx->grid;
    g->ctx.push_back(ctx);
    g->rank.push_back(rank);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    return group_finish(g, ncclCommInitRank(&g->comm[0], nranks, u, rank), "ncclCommInitRank", out);
}

void aq_group_destroy(aq_group* g) {
    if (!g) return;
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        (void)hipSetDevice(g->ctx[m]->device);
        (void)hipStreamSynchronize(g->ctx[m]->stream);
        if (g->comm[m]) (void)ncclCommDestroy(g->comm[m]);
    }
    delete g;   // (the buffers free themselves: aq_host_mem.h)
}

int aq_group_size(const aq_group* g) { return g ? g->nranks : 0; }

int aq_integrate_group(aq_group* g, const aq_problem* p, aq_result* res) {
    if (!g) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    if (p->n_gpus != 0 && p->n_gpus != g->nranks) return AQ_EINVAL;
    const int N = g->nranks;
    const size_t info = 3 + (size_t)g->grid;
    // 1. every member runs its rank's shard in the internal SYNC_SLOT (a blocking call never touches
    //    the caller's async slots: a pending aq_integrate_async result in any slot survives), then
    //    packs its contribution on its stream
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        aq_ctx* c = g->ctx[m];
        AQ_HIP(hipSetDevice(c->device));
        LaunchArgs la = sync_args(p, nullptr, g->rank[m], N);
        la.hist = c->histograms;
        la.sync_fold = true;   // k_pack_group folds the per-CU area words itself
        if ((rc = launch(c, la))) return rc;
        AQ_HIP(hipMemsetAsync(g->d_sum[m], 0, sizeof(long long) * GROUP_SUM, c->stream));
        hipLaunchKernelGGL(k_pack_group, dim3(1), dim3(256), 0, c->stream, c->d_ctl, c->d_parts,
                           (const double*)c->d_parea, SYNC_SLOT, g->grid, c->parts_dirty[SYNC_SLOT] ? 1 : 0, g->d_sum[m],
                           g->d_mine[m]);
        AQ_HIP(hipGetLastError());
        if (c->slot_hist[SYNC_SLOT])
            AQ_HIP(hipMemcpyAsync(g->d_sum[m] + XS_LIMBS + 3, c->d_ctl[SYNC_SLOT].hist,
                                  sizeof(long long) * 2 * AQ_MAX_LEVELS, hipMemcpyDeviceToDevice, c->stream));
    }
    // 2. ONE grouped exchange: int64 sums of the exact limbs / counts / histograms, and every rank's
    //    task, level, error and per-CU words
    AQ_NCCL(ncclGroupStart());
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        aq_ctx* c = g->ctx[m];
        AQ_NCCL(ncclAllReduce(g->d_sum[m], g->d_sum[m], GROUP_SUM, ncclInt64, ncclSum, g->comm[m], c->stream));
        AQ_NCCL(ncclAllGather(g->d_mine[m], g->d_all[m], info, ncclUint64, g->comm[m], c->stream));
    }
    AQ_NCCL(ncclGroupEnd());
    aq_ctx* c0 = g->ctx[0];
    AQ_HIP(hipSetDevice(c0->device));
    AQ_HIP(hipMemcpyAsync(g->h_sum, g->d_sum[0], sizeof(long long) * GROUP_SUM, hipMemcpyDeviceToHost, c0->stream));
    AQ_HIP(hipMemcpyAsync(g->h_all, g->d_all[0], sizeof(unsigned long long) * info * N, hipMemcpyDeviceToHost,
                          c0->stream));
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        AQ_HIP(hipSetDevice(g->ctx[m]->device));
        AQ_HIP(hipStreamSynchronize(g->ctx[m]->stream));
    }
    // 3. the whole run's result, identical on every member
    XSum x;
    for (int i = 0; i < XS_LIMBS; ++i) x.limb[i] = g->h_sum[i];
    HostOut h;
    h.area = xs_round(x);
    h.tasks = (unsigned long long)g->h_sum[XS_LIMBS];
    h.leaves = (unsigned long long)g->h_sum[XS_LIMBS + 1];
    h.spilled = (unsigned long long)g->h_sum[XS_LIMBS + 2];
    for (int i = 0; i < 2 * AQ_MAX_LEVELS; ++i) h.hist[i] = (unsigned long long)g->h_sum[XS_LIMBS + 3 + i];
    std::vector<unsigned long long> cu((size_t)N * AQ_CU_SLOTS, 0ull);
    for (int r = 0; r < N; ++r) {
        const unsigned long long* row = g->h_all + info * r;
        h.levels = std::max<unsigned>(h.levels, (unsigned)row[1]);
        h.error |= (unsigned)row[2];
        for (int w = 0; w < g->grid; ++w) {
            const unsigned long long v = row[3 + w];
            cu[(size_t)r * AQ_CU_SLOTS + (v & ((1u << CU_BITS) - 1u))] += v >> CU_BITS;
        }
    }
    for (int s = 0; s < AQ_CU_SLOTS; ++s) h.cu[s] = cu[(size_t)g->rank[0] * AQ_CU_SLOTS + s];
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        aq_ctx* c = g->ctx[m];
        c->last = h;
        for (int s = 0; s < AQ_CU_SLOTS; ++s) c->last.cu[s] = cu[(size_t)g->rank[m] * AQ_CU_SLOTS + s];
        c->last_valid = true;
    }
    if (res) {
        fill_result(c0, h, res);
        unsigned ncu = 0;
        for (size_t i = 0; i < cu.size(); ++i) ncu += cu[i] ? 1u : 0u;
        res->n_cu = ncu;
        res->n_gpus = (uint32_t)N;
        for (int r = 0; r < N; ++r) {
            if (res->tasks_per_gpu) res->tasks_per_gpu[r] = g->h_all[info * r];
            if (res->tasks_per_cu) cu_row(&cu[(size_t)r * AQ_CU_SLOTS], res->tasks_per_cu + (size_t)r * c0->num_cus,
                                          c0->num_cus);
        }
    }
    return err_from_bits(h.error);
}

int aq_level_histogram(aq_ctx* ctx, uint64_t* tpl, uint64_t* lpl, int maxlev) {
    if (!ctx || maxlev < 0 || !ctx->last_valid) return AQ_EINVAL;
    for (int i = 0; i < maxlev; ++i) {
        const bool in = i < AQ_MAX_LEVELS;
        if (tpl) tpl[i] = in ? ctx->last.hist[i] : 0;
        if (lpl) lpl[i] = in ? ctx->last.hist[AQ_MAX_LEVELS + i] : 0;
    }
    return AQ_OK;
}

int aq_cu_task_counters(aq_ctx* ctx, uint64_t* out, int cap, int reset) {
    if (!ctx || (cap > 0 && !out) || cap < 0) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    std::vector<unsigned long long> h(AQ_CU_SLOTS, 0ull);
    // read and reset in the order of the context's (non-blocking) stream: the next launch's atomics
    // into the counters follow the zeroing
    AQ_HIP(hipMemcpyAsync(h.data(), ctx->d_cu_acc, sizeof(unsigned long long) * AQ_CU_SLOTS, hipMemcpyDeviceToHost,
                          ctx->stream));
    if (reset) AQ_HIP(hipMemsetAsync(ctx->d_cu_acc, 0, sizeof(unsigned long long) * AQ_CU_SLOTS, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    int n = 0;
    for (int i = 0; i < AQ_CU_SLOTS; ++i) {
        if (i < cap) out[i] = h[i];
        n += h[i] ? 1 : 0;
    }
    return n;
}

int aq_tasks_per_cu(aq_ctx* ctx, uint64_t* out, int cap) {
    if (!ctx || !ctx->last_valid) return AQ_EINVAL;
    int n = 0;
    for (int i = 0; i < AQ_CU_SLOTS; ++i) {
        if (out && i < cap) out[i] = ctx->last.cu[i];
        n += ctx->last.cu[i] ? 1 : 0;
    }
    return n;
}

int aq_integrate_levels(aq_ctx* ctx, const aq_problem* p, aq_result* res, uint64_t* tpl, uint64_t* lpl,
                        int maxlev) {
    if (!ctx) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    AQ_HIP(hipSetDevice(ctx->device));
    const int max_depth = p->max_depth ? p->max_depth : AQ_DEFAULT_MAX_DEPTH;
    // 16 M records (512 MiB) per buffer at least, whatever a frontier run left there before
    if ((rc = ctx->front.ensure_front((size_t)1 << 24))) return rc;
    const size_t front_cap = ctx->front.d_rec[0].count();
    DevResults* dres = ctx->d_lres;
    AQ_HIP(hipMemsetAsync(dres, 0, sizeof(DevResults), ctx->stream));
    AQ_HIP(hipMemsetAsync(ctx->front.d_count, 0, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), ctx->stream));
    with_fid(p->integrand, [&](auto F) {
        hipLaunchKernelGGL((k_root<decltype(F)::value>), dim3(1), dim3(64), 0, ctx->stream, p->a, p->b, ctx->front.d_rec[0],
                           ctx->d_tab);
    });
    AQ_HIP(hipGetLastError());
    unsigned n = 1;
    int depth = 0;
    for (; n > 0 && depth < AQ_MAX_LEVELS; ++depth) {
        Rec* in = ctx->front.d_rec[depth & 1];
        Rec* outb = ctx->front.d_rec[(depth + 1) & 1];
        unsigned* n_out = ctx->front.d_count + depth + 1;
        const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
        with_fid(p->integrand, [&](auto F) {
            hipLaunchKernelGGL((k_level<decltype(F)::value>), dim3(grid), dim3(256), 0, ctx->stream, in, n, outb, n_out,
                               (unsigned)front_cap, p->eps, depth, max_depth, dres, ctx->d_tab);
        });
        AQ_HIP(hipGetLastError());
        AQ_HIP(hipMemcpyAsync(ctx->h_lres, n_out, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        AQ_HIP(hipStreamSynchronize(ctx->stream));
        unsigned next = 0;
        memcpy(&next, ctx->h_lres, sizeof(unsigned));
        if (next > front_cap) next = (unsigned)front_cap;  // overflow flagged in res->error
        n = next;
    }
    AQ_HIP(hipMemcpyAsync(ctx->h_lres, dres, sizeof(DevResults), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    const DevResults& d = *ctx->h_lres;
    HostOut& h = ctx->last;
    h = HostOut();
    h.area = d.area;
    h.tasks = d.tasks;
    h.leaves = d.leaves;
    h.levels = d.levels;
    h.error = d.error;
    for (int i = 0; i < AQ_MAX_LEVELS; ++i) {
        h.hist[i] = d.tasks_per_level[i];
        h.hist[AQ_MAX_LEVELS + i] = d.leaves_per_level[i];
    }
    for (int i = 0; i < AQ_CU_SLOTS; ++i) h.cu[i] = d.cu_tasks[i];
    ctx->last_valid = true;
    fill_result(ctx, h, res);
    rc = err_from_bits(h.error);
    if (rc) return rc;
    if (n > 0) return AQ_EDEPTH;
    return aq_level_histogram(ctx, tpl, lpl, maxlev);
}

static int ensure_eval(aq_ctx* ctx, size_t n) {
    AQ_HIP(ctx->d_x.grow(n));
    AQ_HIP(ctx->d_y.grow(n));
    return AQ_OK;
}

static int eval_common(aq_ctx* ctx, int integrand, bool cosh_only, size_t n, const double* x, double* out) {
    if (!ctx || (!x && n) || (!out && n)) return AQ_EINVAL;
    if (!integrand_ok(integrand)) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    int rc = ensure_eval(ctx, n);
    if (rc) return rc;
    AQ_HIP(hipMemcpyAsync(ctx->d_x, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    if (cosh_only)
        hipLaunchKernelGGL((k_eval<F_COSH4, true>), dim3(grid), dim3(256), 0, ctx->stream, ctx->d_x, ctx->d_y, n, ctx->d_tab);
    else
        with_fid(integrand, [&](auto F) {
            hipLaunchKernelGGL((k_eval<decltype(F)::value, false>), dim3(grid), dim3(256), 0, ctx->stream, ctx->d_x,
                               ctx->d_y, n, ctx->d_tab);
        });
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipMemcpyAsync(out, ctx->d_y, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return AQ_OK;
}

int aq_eval_integrand(aq_ctx* ctx, int integrand, size_t n, const double* x, double* out) {
    return eval_common(ctx, integrand, false, n, x, out);
}

int aq_eval_cosh(aq_ctx* ctx, size_t n, const double* x, double* out) {
    return eval_common(ctx, AQ_F_COSH4, true, n, x, out);
}

// (theta rides in the second half of the x buffer: n points, then n rows)
int aq_eval_integrand_params(aq_ctx* ctx, size_t n, const double* x, const double* theta, double* out) {
    if (!ctx || (n && (!x || !theta || !out))) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    constexpr size_t NP = (size_t)param::nparams;
    AQ_HIP(hipSetDevice(ctx->device));
    const int rc = ensure_eval(ctx, n * (1 + NP));
    if (rc) return rc;
    double* const d_th = ctx->d_x + n;
    AQ_HIP(hipMemcpyAsync(ctx->d_x, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    AQ_HIP(hipMemcpyAsync(d_th, theta, n * NP * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_eval_params, dim3(grid), dim3(256), 0, ctx->stream, (const double*)ctx->d_x,
                       (const double*)d_th, ctx->d_y, n, (const ExpPair*)ctx->d_tab);
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipMemcpyAsync(out, ctx->d_y, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return AQ_OK;
}

#ifndef AQ_BATCH_FIRST
#define AQ_BATCH_FIRST 131072  // the first chunk: the host's serial work before the device starts
#endif
#ifndef AQ_BATCH_LAST
#define AQ_BATCH_LAST 0        // a remainder above 2x this leaves a last chunk this small: the copy-back
#endif                         // and unpacking after the last launch scale with its size

static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

// f(lo, hi, part) over [0, n) in up to 64 contiguous pieces, on the context's host pool and the caller:
// the batch's serial host work (the first chunk's checks and staging before the device starts, the
// last chunk's unpacking after it ends). AQ_HOST_THREADS sets the threads (default 8, the caller's
// included; read when the pool is created).
static_assert(AQ_F_COSH4 == F_COSH4 && AQ_F_SIN_RECIP == F_SIN_RECIP && AQ_F_USER == F_USER && AQ_F_PARAM == F_PARAM,
              "the batch front end compares the C ABI's integrand ids with the kernels' FIDs");

extern "C++" template <typename F>
static void host_parallel(aq_ctx* ctx, size_t n, size_t grain, F&& f) {
    if (!ctx->pool) {
        const int want = std::min(64, std::max(1, env_int("AQ_HOST_THREADS", 8)));
        ctx->pool.reset(new HostPool((size_t)(want - 1)));
    }
    // pieces: four per thread (balance when a worker wakes late), at least `grain` items each
    const size_t threads = ctx->pool->th.size() + 1;
    const size_t parts = std::max<size_t>(1, std::min<size_t>({64, 4 * threads, n / std::max<size_t>(grain, 1)}));
    if (parts == 1 || threads == 1) {
        for (size_t q = 0; q < parts; ++q) f(n * q / parts, n * (q + 1) / parts, q);
        return;
    }
    const std::function<void(size_t)> piece = [&](size_t q) { f(n * q / parts, n * (q + 1) / parts, q); };
    ctx->pool->run(parts, piece);
}

// ---- steps the batch front end and the tolerance loop share ----------------------------------------------
// Check m integrals [a[i], b[i]] (AQ_F_PARAM: with their theta rows) and stage them in the pinned hb (and ht),
// on the host pool. AQ_EINVAL on a bad row.
static int check_and_stage(aq_ctx* ctx, int integrand, size_t m, const double* a, const double* b, const double* theta,
                           double2* hb, double* ht) {
    const bool par = integrand == AQ_F_PARAM;
    constexpr size_t NP = (size_t)param::nparams;
    std::vector<char> ok(64, 1);
    host_parallel(ctx, m, 8192, [&](size_t i0, size_t i1, size_t p) {
        for (size_t i = i0; i < i1; ++i) {
            if (par ? !params_ok(a[i], b[i], theta + i * NP) : !bounds_ok(integrand, a[i], b[i])) {
                ok[p] = 0;
                return;
            }
            hb[i] = make_double2(a[i], b[i]);
            if (par)
                for (size_t j = 0; j < NP; ++j) ht[i * NP + j] = theta[i * NP + j];
        }
    });
    for (char o : ok)
        if (!o) return AQ_EINVAL;
    return AQ_OK;
}

// Behind a launch into slots 0 .. k-1, on the context's stream: slot s's row {area, tasks, accepted, error} to
// rows[perm ? perm[s] : s] (k_gather_reset) and, behind an ERR launch, its error sums to errrows likewise
// (k_gather_err; null: not an ERR launch). The kernels return the slots to zero: no k_reset before the next
// launch, and the slots count as clean.
// (slots [first, first + k) were returned to zero by a gather kernel -- their error sums too, if err)
static void mark_clean(aq_ctx* ctx, int first, int k, bool err) {
    if (err) memset(ctx->err_dirty + first, 0, (size_t)k);
    memset(ctx->dirty + first, 0, (size_t)k);
    memset(ctx->parts_dirty + first, 0, (size_t)k);
}

static int gather_clean(aq_ctx* ctx, int k, double* rows, double* errrows, const unsigned* perm) {
    hipLaunchKernelGGL(k_gather_reset, dim3((k + 63) / 64), dim3(64), 0, ctx->stream, ctx->d_ctl, ctx->d_parts, ctx->grid, 0,
                       k, rows, perm);
    if (errrows)
        hipLaunchKernelGGL(k_gather_err, dim3((k + 63) / 64), dim3(64), 0, ctx->stream, ctx->d_err, 0, k, errrows, perm);
    AQ_HIP(hipGetLastError());
    mark_clean(ctx, 0, k, errrows != nullptr);
    return AQ_OK;
}

// The size pre-pass of a sorted chunk of m rows, on stream s (the host batch's and the device-resident one's):
// size classes from the estimates, the bounds (and theta, where the view has some) into size order; preset: the
// scatter also sets the launch's job size from the estimates (AQ_F_* values are the kernels' FIDs)
static int size_prepass(aq_ctx* ctx, int integrand, int m, double eps, const BatchRings::View& v, unsigned* key,
                        bool preset, hipStream_t s) {
    constexpr size_t NP = (size_t)param::nparams;
    const unsigned blocks = (unsigned)((m + 255) / 256);
    if (v.theta)
        hipLaunchKernelGGL(k_batch_estimate_params, dim3(blocks), dim3(256), 0, s, v.bounds, (const double*)v.theta, m,
                           eps, key, v.cnt, v.est, ctx->d_tab);
    else
        with_fid(integrand, [&](auto F) {
            hipLaunchKernelGGL(k_batch_estimate<decltype(F)::value>, dim3(blocks), dim3(256), 0, s, v.bounds, m, eps, key,
                               v.cnt, v.est, ctx->d_tab);
        });
    hipLaunchKernelGGL(k_batch_scatter, dim3(blocks), dim3(256), 0, s, v.bounds, key, m, v.cnt, v.cnt + EST_KEYS,
                       v.sorted, v.perm, v.cnt_next, v.est, v.est_next, preset ? ctx->d_hint : nullptr,
                       (unsigned)(ctx->grid * NW));
    if (v.theta)
        hipLaunchKernelGGL(k_batch_scatter_theta, dim3((unsigned)(((size_t)m * NP + 255) / 256)), dim3(256), 0, s,
                           (const double*)v.theta, (const unsigned*)v.perm, m, (int)NP, v.thsorted);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

// a call's per-integral outputs (any may be null)
struct RowsOut {
    double* area;
    uint64_t *accepted, *tasks;
    double *err_abs, *err_signed;
    RowsOut from(size_t i) const {
        auto at = [i](auto* p) { return p ? p + i : p; };
        return RowsOut{at(area), at(accepted), at(tasks), at(err_abs), at(err_signed)};
    }
};

// m pinned rows {area, tasks, accepted, error bits, ...}, `stride` doubles apart, into o[0 .. m), and their
// {err_abs, err_signed} pairs, `estride` apart at errs, into o's error outputs; on the host pool. extra(i, row,
// piece) sees every row as well (a layout's further fields). Returns the OR of the rows' error bits.
extern "C++" template <typename Extra>
static unsigned unpack_rows(aq_ctx* ctx, size_t m, const double* rows, size_t stride, const double* errs, size_t estride,
                            const RowsOut& o, Extra&& extra) {
    std::vector<unsigned> e(64, 0u);
    host_parallel(ctx, m, 8192, [&](size_t i0, size_t i1, size_t p) {
        unsigned bits = 0;
        for (size_t i = i0; i < i1; ++i) {
            const double* row = rows + stride * i;
            if (o.area) o.area[i] = row[0];
            if (o.tasks) o.tasks[i] = (uint64_t)row[1];
            if (o.accepted) o.accepted[i] = (uint64_t)row[2];
            bits |= (unsigned)row[3];
            if (o.err_abs) o.err_abs[i] = errs[estride * i];
            if (o.err_signed) o.err_signed[i] = errs[estride * i + 1];
            extra(i, row, p);
        }
        e[p] = bits;
    });
    unsigned bits = 0;
    for (unsigned x : e) bits |= x;
    return bits;
}

// ---- the batch front end (SURVEY config 3) ----------------------------------------------------------------
// Up to MAXK integrals per persistent launch, every integral with its own slot, n integrals as chunks
// (batch_chunks): a small first chunk starts the device early, a small last one shortens the copy-back after
// it. Four streams (r05, r06; profiles/r05a/c3_timeline_r04code.json had the launches wait ~0.5 ms per chunk
// for a reset, a bounds copy, a full-width gather and a rows copy): the host checks and stages chunk c + 1
// while chunk c runs, s_h2d copies it into its own device rows, s_pre puts it into size order (largest trees
// first: the launch's tail is its smallest jobs; AQ_BATCH_SORT=0: off) as chunk c's launch frees the CUs, the
// context's stream runs the launches and gathers, s_d2h copies chunk c's rows back while chunk c + 1 runs and
// the host unpacks chunk c - 1. Which step runs where, behind what: batch_plan (aq_batch_plan.h); run_plan
// walks it. BatchCall is one call's state and one function per step kind -- it orders nothing.
//
// theta: the parametrised family's rows [n][nparams] (integrand AQ_F_PARAM), else null; they travel with the
// bounds. The ERR form's (plan.err) slots' error sums travel with the rows.

// the workload is fresh: the context holds no measured job-size hint for this integrand and tolerance (the
// sorted chunks' pre-passes preset the job size until a launch has measured one: aq_batch_plan.h)
static bool hint_is_fresh(const aq_ctx* ctx, int integrand, double eps) {
    return ctx->gsplit_env <= 0 &&
           !(ctx->hint.valid && ctx->hint.fid == integrand && ctx->hint.eps == eps && ctx->hint.nshards == 1);
}

// One call of either batch pipeline, and the steps the two run alike.
struct BatchSteps {
    aq_ctx* ctx;
    const BatchRings& R;       // the pipeline's rings
    const BatchPlan& plan;
    double eps;
    int integrand;
    const double *a = nullptr, *b = nullptr;   // the bounds on the host (device-resident batch: none)
    int max_depth = 0;
    std::vector<size_t> off;   // chunk c: integrals [off[c], off[c + 1])
    static constexpr size_t NP = (size_t)param::nparams;

    BatchSteps(aq_ctx* ctx_, const BatchRings& R_, const BatchPlan& plan_, double eps_, int integrand_)
        : ctx(ctx_), R(R_), plan(plan_), eps(eps_), integrand(integrand_), off(plan_.chunks.size() + 1, 0) {
        for (size_t c = 0; c < plan.chunks.size(); ++c) off[c + 1] = off[c] + (size_t)plan.chunks[c];
    }
    int zero(hipStream_t s) {
        AQ_HIP(hipMemsetAsync(R.cnt, 0, sizeof(unsigned) * 4 * EST_KEYS, s));
        AQ_HIP(hipMemsetAsync(R.est, 0, sizeof(double) * 2, s));
        return AQ_OK;
    }
    int pre(int c, hipStream_t s) {
        return size_prepass(ctx, integrand, plan.chunks[c], eps, R.at(c), R.key, plan.preset[c], s);
    }
    // (without bounds on the host, plan.first_slot keeps every chunk off the per-CU instance, which takes them
    // as kernel arguments)
    int launch_chunk(int c) {
        const BatchRings::View v = R.at(c);
        LaunchArgs g;   // (no histograms: hist stays false)
        g.integrand = integrand;
        g.k = plan.chunks[c];
        g.a = a ? a + off[c] : nullptr;
        g.b = b ? b + off[c] : nullptr;
        g.eps = eps;
        g.max_depth = max_depth;
        g.first_slot = plan.first_slot[c];
        g.dev_bounds = plan.sorted[c] ? v.sorted : v.bounds;
        g.dev_theta = plan.sorted[c] ? v.thsorted : v.theta;
        g.err = plan.err;
        g.heap = true;
        ctx->hint.preset = plan.preset[c];
        const int rc = launch(ctx, g);
        ctx->hint.preset = false;
        return rc;
    }
};

// Walks a plan: for each step that BatchWalk lets run, the waits on the step's stream (on the host for a host
// step), `step(s, stream)` for what the step does, and its event. streams: by BStream, the host apart; ev: by
// the plan's event numbers. Returns the call's code.
extern "C++" template <typename Step>
static int run_plan(const BatchPlan& plan, const hipStream_t* streams, const Event* ev, Step&& step) {
    static_assert(AQ_OK == 0, "BatchWalk's success code");
    BatchWalk walk;   // which steps a failure leaves out
    for (const BatchStep& s : plan.steps) {
        if (!walk.runs(s)) continue;
        const bool host = s.stream == BStream::HOST;
        const hipStream_t st = host ? nullptr : streams[(int)s.stream];
        auto issue = [&]() -> int {
            for (int w : s.wait)
                if (w >= 0) AQ_HIP(host ? hipEventSynchronize(ev[w]) : hipStreamWaitEvent(st, ev[w], 0));
            if (int rc = step(s, st)) return rc;
            if (s.record >= 0) AQ_HIP(hipEventRecord(ev[s.record], st));
            return AQ_OK;
        };
        walk.done(s, issue());
    }
    return walk.rc;
}

struct BatchCall : BatchSteps {
    const HostBatch& B;        // ctx->batch
    const double* theta;
    RowsOut out;
    unsigned errbits = 0;

    // (on several host threads: the first chunk's is the only host work before the device starts, the next
    // ones' must stay shorter than a launch)
    int stage(int c) {
        return check_and_stage(ctx, integrand, (size_t)plan.chunks[c], a + off[c], b + off[c],
                               plan.theta ? theta + off[c] * NP : nullptr, B.h_bounds + off[c],
                               plan.theta ? B.h_theta + off[c] * NP : nullptr);
    }
    int h2d(int c, hipStream_t s) {
        const BatchRings::View v = B.at(c);
        const size_t m = (size_t)plan.chunks[c];
        if (plan.theta)
            AQ_HIP(hipMemcpyAsync(v.theta, B.h_theta + off[c] * NP, sizeof(double) * NP * m, hipMemcpyHostToDevice, s));
        AQ_HIP(hipMemcpyAsync(v.bounds, B.h_bounds + off[c], sizeof(double2) * m, hipMemcpyHostToDevice, s));
        return AQ_OK;
    }
    // (k_gather_reset writes size-ordered slots back in input order)
    int gather(int c) {
        return gather_clean(ctx, plan.chunks[c], B.rows_at(c), B.errrows_at(c), plan.sorted[c] ? B.at(c).perm : nullptr);
    }
    int d2h(int c, hipStream_t s) {
        const size_t m = (size_t)plan.chunks[c];
        AQ_HIP(hipMemcpyAsync(B.h_rows + 4 * off[c], B.rows_at(c), sizeof(double) * 4 * m, hipMemcpyDeviceToHost, s));
        if (plan.err)
            AQ_HIP(hipMemcpyAsync(B.h_errrows + 2 * off[c], B.errrows_at(c), sizeof(double) * 2 * m, hipMemcpyDeviceToHost, s));
        return AQ_OK;
    }
    void unpack(int c) {
        errbits |= unpack_rows(ctx, (size_t)plan.chunks[c], B.h_rows + 4 * off[c], 4,
                               plan.err ? B.h_errrows + 2 * off[c] : nullptr, 2, out.from(off[c]),
                               [](size_t, const double*, size_t) {});
    }
};

// A bad bound fails the call (AQ_EINVAL) after the chunks before it ran; the outputs are then unspecified.
static int batch_run(aq_ctx* ctx, size_t n, const double* a, const double* b, const double* theta, double eps,
                     int integrand, double* area, uint64_t* accepted, uint64_t* tasks, bool err = false,
                     double* err_abs = nullptr, double* err_signed = nullptr) {
    if (!ctx || (n && (!a || !b))) return AQ_EINVAL;
    const bool par = integrand == AQ_F_PARAM;
    if (par ? !theta : !integrand_ok(integrand)) return AQ_EINVAL;
    if (!(eps >= 0.0)) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    // AQ_BATCH_TRACE=1: the host's phase times of this call on stderr (diagnostics: tools/c3_timeline.py)
    const bool trace = env_int("AQ_BATCH_TRACE", 0) != 0;
    const auto t_call = std::chrono::steady_clock::now();
    std::vector<std::pair<std::string, double>> tr;
    auto mark = [&](const char* what, long c) {
        if (trace)
            tr.emplace_back(std::string(what) + (c >= 0 ? " " + std::to_string(c) : std::string()),
                            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_call).count());
    };
    AQ_HIP(hipSetDevice(ctx->device));
    const std::vector<int> chunks = batch_chunks(n, (size_t)std::max(0, env_int("AQ_BATCH_FIRST", AQ_BATCH_FIRST)),
                                                 (size_t)std::max(0, env_int("AQ_BATCH_LAST", AQ_BATCH_LAST)));
    const bool sort = env_int("AQ_BATCH_SORT", 1) != 0;
    const BatchPlan plan = batch_plan(chunks, sort, par, err, hint_is_fresh(ctx, integrand, eps));
    int rc = ctx->batch.grow((size_t)*std::max_element(chunks.begin(), chunks.end()), n, par, err);
    if (rc) return rc;
    for (Stream* s : {&ctx->s_h2d, &ctx->s_d2h, &ctx->s_pre})
        if (!*s) AQ_HIP(s->create());
    const hipStream_t streams[] = {ctx->stream, ctx->s_h2d, ctx->s_d2h, ctx->s_pre, nullptr};   // by BStream (no caller's)
    // (destroyed on return, after every stream was synchronised: the plan's DRAIN)
    std::vector<Event> ev((size_t)plan.n_events());
    for (Event& e : ev) AQ_HIP(e.create(hipEventDisableTiming));
    BatchCall call{BatchSteps(ctx, ctx->batch, plan, eps, integrand), ctx->batch, theta,
                   RowsOut{area, accepted, tasks, err_abs, err_signed}};
    call.a = a, call.b = b;
    rc = run_plan(plan, streams, ev.data(), [&](const BatchStep& s, hipStream_t st) {
        const int c = s.chunk;
        int r = AQ_OK;
        switch (s.kind) {
            case BKind::START: case BKind::FENCE: break;   // their event is all they do
            case BKind::ZERO: return call.zero(st);
            case BKind::STAGE:
                if (c == 0) mark("setup", -1);
                return call.stage(c);
            case BKind::H2D: r = call.h2d(c, st), mark("staged", c); break;
            case BKind::PRE: return call.pre(c, st);
            case BKind::LAUNCH: r = call.launch_chunk(c), mark("launched", c); break;
            case BKind::GATHER: return call.gather(c);
            case BKind::D2H: return call.d2h(c, st);
            case BKind::WAIT: mark("rows on host", c); break;
            case BKind::UNPACK: call.unpack(c), mark("unpacked", c); break;
            case BKind::DRAIN:   // every enqueued chunk finishes before the buffers can be reused or the events destroyed
                for (int x = 0; x <= (int)BStream::PRE; ++x)
                    if (hipStreamSynchronize(streams[x]) != hipSuccess) r = AQ_EHIP;
                mark("device done", -1);
                break;
            default: return AQ_EINVAL;   // (no such step in a host plan)
        }
        return r;
    });
    if (rc) return rc;
    if (trace) {
        fprintf(stderr, "aq_integrate_batch n=%zu:", n);
        for (auto& m : tr) fprintf(stderr, " [%s %.1f us]", m.first.c_str(), m.second);
        fprintf(stderr, "\n");
    }
    return err_from_bits(call.errbits);
}

int aq_integrate_batch(aq_ctx* ctx, size_t n, const double* a, const double* b, double eps, int integrand,
                       double* area, uint64_t* accepted, uint64_t* tasks) {
    if (!integrand_ok(integrand)) return AQ_EINVAL;
    return batch_run(ctx, n, a, b, nullptr, eps, integrand, area, accepted, tasks);
}

int aq_integrate_batch_params(aq_ctx* ctx, size_t n, const double* a, const double* b, const double* theta, double eps,
                              double* area, uint64_t* accepted, uint64_t* tasks) {
    if (!ctx || !theta) return AQ_EINVAL;
    return batch_run(ctx, n, a, b, theta, eps, AQ_F_PARAM, area, accepted, tasks);
}

int aq_integrate_batch_err(aq_ctx* ctx, size_t n, const double* a, const double* b, const double* theta, double eps,
                           int integrand, double* area, uint64_t* accepted, uint64_t* tasks, double* err_abs,
                           double* err_signed) {
    if (!ctx || !theta_ok(integrand, theta)) return AQ_EINVAL;
    return batch_run(ctx, n, a, b, theta, eps, integrand, area, accepted, tasks, true, err_abs, err_signed);
}

// ---- device-resident batch (aq_integrate_batch_device) ---------------------------------------------------
// The caller's arrays are device memory and the call only enqueues: k_dev_check in place of the host's checks
// and staging, the host batch's size pre-pass and launches, k_gather_reset_soa in place of the gathers, the
// copy back and the unpacking. Which step runs where, behind what: device_batch_plan (aq_batch_plan.h).
// DevBatchCall is one call's state and one function per step kind of its own -- it orders nothing.
struct DevBatchCall : BatchSteps {
    const DevBatch& D;         // ctx->devbatch
    const aq_device_io& io;

    int check(int c, hipStream_t s) {
        const BatchRings::View v = D.at(c);
        const int m = plan.chunks[c];
        const unsigned blocks = (unsigned)((m + 255) / 256);
        const double *a = io.a + off[c], *b = io.b + off[c];
        if (plan.theta)
            hipLaunchKernelGGL(k_dev_check_params, dim3(blocks), dim3(256), 0, s, a, b, io.theta + off[c] * NP, m, v.bounds,
                               v.theta, D.flags(c), D.stat.get());
        else
            with_fid(integrand, [&](auto F) {
                hipLaunchKernelGGL(k_dev_check<decltype(F)::value>, dim3(blocks), dim3(256), 0, s, a, b, m, v.bounds,
                                   D.flags(c), D.stat.get());
            });
        AQ_HIP(hipGetLastError());
        return AQ_OK;
    }
    // (the kernel returns the slots and their error sums to zero, as gather_clean's two do: they count as clean)
    int gather(int c) {
        const BatchRings::View v = D.at(c);
        const int k = plan.chunks[c], first = plan.first_slot[c];
        auto at = [&](auto* p) { return p ? p + off[c] : p; };
        const SoaOut out{at(io.area), (unsigned long long*)at(io.accepted), (unsigned long long*)at(io.tasks),
                         at(io.err_abs), at(io.err_signed), at(io.status)};
        hipLaunchKernelGGL(k_gather_reset_soa, dim3((k + 63) / 64), dim3(64), 0, ctx->stream, ctx->d_ctl.get(),
                           (const unsigned long long*)ctx->d_parts, ctx->grid, first, k,
                           (const unsigned*)(plan.sorted[c] ? v.perm : nullptr), plan.err ? ctx->d_err.get() : nullptr,
                           (const unsigned*)D.flags(c), io.max_depth ? io.max_depth : AQ_DEFAULT_MAX_DEPTH, out,
                           D.stat.get());
        AQ_HIP(hipGetLastError());
        mark_clean(ctx, first, k, plan.err);
        return AQ_OK;
    }
};

int aq_integrate_batch_device(aq_ctx* ctx, size_t n, const aq_device_io* io, double eps, int integrand,
                              void* const* stream) {
    if (!ctx || !io || (n && (!io->a || !io->b))) return AQ_EINVAL;
    if (!theta_ok(integrand, io->theta)) return AQ_EINVAL;
    if (!(eps >= 0.0) || io->max_depth < 0 || io->max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    const bool par = integrand == AQ_F_PARAM, err = io->err_abs || io->err_signed;
    AQ_HIP(hipSetDevice(ctx->device));
    const std::vector<int> chunks = device_batch_chunks(n, device_batch_chunk_rows(env_int("AQ_DEVBATCH_CHUNK", MAXK)));
    const bool sort = env_int("AQ_BATCH_SORT", 1) != 0;
    const BatchPlan plan = device_batch_plan(chunks, sort, par, err, hint_is_fresh(ctx, integrand, eps), stream != nullptr);
    int rc = ctx->devbatch.ensure(par, (size_t)plan.n_events());
    if (rc) return rc;
    if (err && (rc = ensure_err(ctx))) return rc;
    if (!ctx->s_pre) AQ_HIP(ctx->s_pre.create());
    // by BStream (no copy streams)
    const hipStream_t streams[] = {ctx->stream, nullptr, nullptr, ctx->s_pre, stream ? (hipStream_t)*stream : nullptr};
    DevBatchCall call{BatchSteps(ctx, ctx->devbatch, plan, eps, integrand), ctx->devbatch, *io};
    call.max_depth = io->max_depth;
    // (a failed step ends the call: what it enqueued so far runs out on its own, and waits for no event that
    // is never recorded -- BatchWalk)
    return run_plan(plan, streams, ctx->devbatch.ev.data(), [&](const BatchStep& s, hipStream_t st) {
        switch (s.kind) {
            case BKind::JOIN_IN: case BKind::START: case BKind::FENCE: case BKind::JOIN_OUT: return AQ_OK;   // waits and records
            case BKind::ZERO: return call.zero(st);
            case BKind::CHECK: return call.check(s.chunk, st);
            case BKind::PRE: return call.pre(s.chunk, st);
            case BKind::LAUNCH: return call.launch_chunk(s.chunk);
            case BKind::GATHER_SOA: return call.gather(s.chunk);
            default: return AQ_EINVAL;   // (no such step in a device plan)
        }
    });
}

int aq_device_batch_check(aq_ctx* ctx, uint64_t* invalid_rows) {
    if (!ctx) return AQ_EINVAL;
    if (invalid_rows) *invalid_rows = 0;
    AQ_HIP(hipSetDevice(ctx->device));
    const DevBatch& D = ctx->devbatch;
    if (!D.stat) {   // no device batch yet
        AQ_HIP(hipStreamSynchronize(ctx->stream));
        return AQ_OK;
    }
    // (the pinned-word read of read_slot: an asynchronous copy into pinned memory, then the stream)
    AQ_HIP(hipMemcpyAsync(D.h_stat, D.stat, sizeof(DevBatchStat), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemsetAsync(D.stat, 0, sizeof(DevBatchStat), ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    const DevBatchStat st = *D.h_stat;
    if (invalid_rows) *invalid_rows = st.invalid;
    return st.invalid ? AQ_EINVAL : err_from_bits(st.errbits);
}

// ---- tolerance-driven batch (aq_integrate_batch_tol) -----------------------------------------------------
// a call's outputs (any may be null)
struct TolOut {
    RowsOut rows;
    double* eps_used;
    int32_t* rounds;
};

// One block: m <= R integrals [a[i], b[i]] (theta rows beside them), outputs at the same offsets. R: the
// call's rows per block, the distance of the ping-pong halves. t: defaulted. The rows' error bits are OR-ed
// into *errbits, *noconv is set if a row retired without converging.
static int tol_block(aq_ctx* ctx, size_t m, size_t R, const double* a, const double* b, const double* theta,
                     int integrand, const aq_tol& t, const TolOut& o, unsigned* errbits, bool* noconv) {
    const bool par = integrand == AQ_F_PARAM;
    constexpr size_t NP = (size_t)param::nparams;
    const TolBufs& T = ctx->tol;
    // 1. check and stage once, copy once into half 0, rows' indices 0 .. m-1
    int rc = check_and_stage(ctx, integrand, m, a, b, theta, T.h_bounds, T.h_theta);
    if (rc) return rc;
    AQ_HIP(hipMemcpyAsync(T.bounds, T.h_bounds, sizeof(double2) * m, hipMemcpyHostToDevice, ctx->stream));
    if (par) AQ_HIP(hipMemcpyAsync(T.theta, T.h_theta, sizeof(double) * NP * m, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_tol_init, dim3((unsigned)((m + TOL_T - 1) / TOL_T)), dim3(TOL_T), 0, ctx->stream, T.idx.get(),
                       (int)m, ctx->d_hint.get());
    AQ_HIP(hipGetLastError());
    // the trapezoid rule's d scales as h^3, so a leaf's width as eps^(1/3): a round's trees are about
    // shrink^(1/3) times the round before's
    const double growth = std::cbrt(t.shrink);
    // a launch of fewer than PCU_MAXK integrals takes its bounds from the host (kernel arguments)
    double ha[PCU_MAXK], hb[PCU_MAXK];
    for (size_t i = 0; i < m && i < (size_t)PCU_MAXK; ++i) ha[i] = a[i], hb[i] = b[i];
    int k = (int)m, half = 0;
    double eps = t.eps0;
    for (int r = 1; k > 0; ++r, eps /= t.shrink) {
        const bool last = r == t.max_rounds;
        const double2* bounds = T.bounds + (size_t)half * R;
        const double* th = par ? T.theta + (size_t)half * R * NP : nullptr;
        const unsigned* idx = T.idx + (size_t)half * R;
        // 2. the round: one ERR launch of the k live rows, then the batch front end's two gathers
        LaunchArgs g;
        g.integrand = integrand;
        g.k = k;
        g.a = k < PCU_MAXK ? ha : a;
        g.b = k < PCU_MAXK ? hb : b;
        g.eps = eps;
        g.max_depth = t.max_depth;
        g.dev_bounds = bounds;
        g.dev_theta = th;
        g.err = true;
        g.heap = true;
        // the job size comes from the hint the kernels before this launch preset (per-CU launches have none)
        ctx->hint.preset = k >= PCU_MAXK;
        rc = launch(ctx, g);
        ctx->hint.preset = false;
        if (rc) return rc;
        if ((rc = gather_clean(ctx, k, T.rows, T.err, nullptr))) return rc;
        // 3. test and retire; the survivors into the other half, their count to the host
        const unsigned nb = (unsigned)((k + TOL_T - 1) / TOL_T);
        hipLaunchKernelGGL(k_tol_test, dim3(nb), dim3(TOL_T), 0, ctx->stream, (const double*)T.rows, (const double*)T.err,
                           idx, k, t.epsabs, t.epsrel, eps, r, last ? 1 : 0, T.res.get(), T.flag.get(), T.cnt.get(),
                           T.tsum.get());
        AQ_HIP(hipGetLastError());
        if (last) break;   // every row retired
        const int other = half ^ 1;
        hipLaunchKernelGGL(k_tol_compact, dim3(nb), dim3(TOL_T), 0, ctx->stream, (const unsigned char*)T.flag,
                           (const unsigned*)T.cnt, k, bounds, th, idx, T.bounds + (size_t)other * R,
                           par ? T.theta + (size_t)other * R * NP : nullptr, T.idx + (size_t)other * R, par ? (int)NP : 0,
                           T.d_surv, (const double*)T.tsum, growth, ctx->d_hint.get(), (unsigned)(ctx->grid * ERR_NW));
        AQ_HIP(hipGetLastError());
        // 4. the host's one look per round
        AQ_HIP(hipStreamSynchronize(ctx->stream));
        const unsigned left = __atomic_load_n(&T.h_surv->count, __ATOMIC_ACQUIRE);
        if (left > (unsigned)k) return AQ_EHIP;   // (cannot happen: survivors are some of the k rows)
        k = (int)left;
        half = other;
        if (k < PCU_MAXK)
            for (int j = 0; j < k; ++j) {
                const unsigned i = T.h_surv->idx[j];
                if (i >= m) return AQ_EHIP;
                ha[j] = a[i], hb[j] = b[i];
            }
    }
    // 5. the block's records: one copy, unpacked on the host pool
    // (a record: the row's four fields, its error pair, eps_used, rounds)
    AQ_HIP(hipMemcpyAsync(T.h_res, T.res, sizeof(double) * TOL_REC * m, hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<char> nc(64, 0);
    *errbits |= unpack_rows(ctx, m, T.h_res, TOL_REC, T.h_res + 4, TOL_REC, o.rows, [&](size_t i, const double* rec, size_t p) {
        if (o.eps_used) o.eps_used[i] = rec[6];
        if (o.rounds) o.rounds[i] = (int32_t)rec[7];
        if (rec[7] < 0.0) nc[p] = 1;
    });
    for (char c : nc) *noconv |= c != 0;
    return AQ_OK;
}

int aq_integrate_batch_tol(aq_ctx* ctx, size_t n, const double* a, const double* b, const double* theta, int integrand,
                           const aq_tol* tol, double* area, uint64_t* accepted, uint64_t* tasks, double* err_abs,
                           double* err_signed, double* eps_used, int32_t* rounds) {
    if (!ctx || !tol || !theta_ok(integrand, theta) || (n && (!a || !b))) return AQ_EINVAL;
    if (!tol_args_ok(*tol)) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    const aq_tol t = tol_defaulted(*tol);
    constexpr size_t NP = (size_t)param::nparams;
    AQ_HIP(hipSetDevice(ctx->device));
    const size_t R = std::min(n, (size_t)tol_block_rows(env_int("AQ_TOL_BLOCK", 0)));
    int rc = ctx->tol.ensure(R, integrand == AQ_F_PARAM);
    if (rc) return rc;
    unsigned errbits = 0;
    bool noconv = false;
    const RowsOut rows{area, accepted, tasks, err_abs, err_signed};
    for (size_t off = 0; off < n; off += R) {
        const TolOut o{rows.from(off), eps_used ? eps_used + off : nullptr, rounds ? rounds + off : nullptr};
        rc = tol_block(ctx, std::min(R, n - off), R, a + off, b + off, theta ? theta + off * NP : nullptr, integrand, t, o,
                       &errbits, &noconv);
        if (rc) {
            (void)hipStreamSynchronize(ctx->stream);   // nothing of the call stays in flight
            return rc;
        }
    }
    if (errbits) return err_from_bits(errbits);
    return noconv ? AQ_ENOCONV : AQ_OK;
}

int aq_frontier_root(aq_ctx* ctx, int integrand, double a, double b, double* d_out) {
    if (!ctx || !d_out || !integrand_ok(integrand) || !bounds_ok(integrand, a, b)) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    with_fid(integrand, [&](auto F) {
        hipLaunchKernelGGL((k_frontier_root<decltype(F)::value>), dim3(1), dim3(64), 0, ctx->stream, a, b, (Rec*)d_out,
                           ctx->d_tab);
    });
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

// Fold the level-step rows written since the last fold into their accumulator (one k_level_fold).
static int fold_pending(aq_ctx* ctx) {
    if (ctx->lp_pending > 0) {
        hipLaunchKernelGGL(k_level_fold, dim3(1), dim3(FOLD_T), 0, ctx->stream, ctx->d_lparts, ctx->lp_pending, ctx->lp_acc);
        AQ_HIP(hipGetLastError());
    }
    ctx->lp_pending = 0;
    return AQ_OK;
}

// Which instance of k_level_step a step launches: the plain one, the leaf-emitting one (aq_integrate_mesh) or the
// batch form (aq_integrate_mesh_batch, aq_mesh_refine_batch), with that instance's trailing argument.
struct StepSink {
    enum Kind { NONE, LEAF, BATCH } kind = NONE;
    BatchSink batch{};   // LEAF: its `leaf` alone
    StepSink() = default;
    StepSink(const LeafSink& s) : kind(LEAF) { batch.leaf = s; }
    StepSink(const BatchSink& s) : kind(BATCH), batch(s) {}
};

static int level_step_impl(aq_ctx* ctx, int integrand, const double* d_in, uint32_t n_in, const uint32_t* d_n_in,
                           double* d_out, uint32_t cap_out, double eps, int depth, int max_depth, uint32_t* d_n_out,
                           double* d_acc, const StepSink& sink = {}) {
    if (!ctx || !d_n_out || !d_acc || (n_in && (!d_in || !d_out))) return AQ_EINVAL;
    // (the batch form alone gathers a theta row per record: AQ_F_PARAM only there)
    if (!integrand_ok(integrand) && !(sink.kind == StepSink::BATCH && integrand == AQ_F_PARAM)) return AQ_EINVAL;
    if (!(eps >= 0.0) || depth < 0 || max_depth < 1 || max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    int rc;
    AQ_HIP(ctx->d_lparts.grow(LP_CAP));
    if (!d_n_in) AQ_HIP(hipMemsetAsync(d_n_out, 0, sizeof(uint32_t), ctx->stream));
    if (n_in == 0) return AQ_OK;
    const int grid = (int)std::min<size_t>(((size_t)n_in + LEVEL_T * LEVEL_R - 1) / (LEVEL_T * LEVEL_R),
                                           (size_t)ctx->level_grid);
    // this step's rows follow the pending ones (folded first if they belong elsewhere or would not fit)
    if (ctx->lp_pending && (d_acc != ctx->lp_acc || ctx->lp_pending + grid > LP_CAP) && (rc = fold_pending(ctx)))
        return rc;
    LevelPart* rows = ctx->d_lparts + ctx->lp_pending;
    auto launch = [&](auto F, auto... s) {   // k_level_step<FID> with the sink's instance and trailing argument
        hipLaunchKernelGGL((k_level_step<decltype(F)::value, decltype(s)...>), dim3(grid), dim3(LEVEL_T), 0, ctx->stream,
                           (const Rec*)d_in, n_in, (Rec*)d_out, d_n_out, cap_out, eps, depth, max_depth, rows, ctx->d_tab,
                           d_n_in, s...);
    };
    if (sink.kind == StepSink::BATCH)   // every integrand, F_PARAM among them
        with_stream_fid(integrand, [&](auto F) { launch(F, sink.batch); });
    else if (sink.kind == StepSink::LEAF) with_fid(integrand, [&](auto F) { launch(F, sink.batch.leaf); });
    else with_fid(integrand, [&](auto F) { launch(F); });
    AQ_HIP(hipGetLastError());
    ctx->lp_pending += grid;
    ctx->lp_acc = d_acc;
    return ctx->defer_fold ? AQ_OK : fold_pending(ctx);
}

int aq_level_defer_fold(aq_ctx* ctx, int enable) {
    if (!ctx) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    ctx->defer_fold = enable != 0;
    return enable ? AQ_OK : fold_pending(ctx);
}

int aq_level_step(aq_ctx* ctx, int integrand, const double* d_in, uint32_t n_in, double* d_out, uint32_t cap_out,
                  double eps, int depth, int max_depth, uint32_t* d_n_out, double* d_acc) {
    return level_step_impl(ctx, integrand, d_in, n_in, nullptr, d_out, cap_out, eps, depth, max_depth, d_n_out, d_acc);
}

int aq_level_step_chained(aq_ctx* ctx, int integrand, const double* d_in, const uint32_t* d_n_in, uint32_t n_in_max,
                          double* d_out, uint32_t cap_out, double eps, int depth, int max_depth, uint32_t* d_n_out,
                          double* d_acc) {
    if (!d_n_in) return AQ_EINVAL;
    return level_step_impl(ctx, integrand, d_in, n_in_max, d_n_in, d_out, cap_out, eps, depth, max_depth, d_n_out,
                           d_acc);
}

static int level_narrow_impl(aq_ctx* ctx, int integrand, double* d_buf0, double* d_buf1, uint32_t cap,
                             uint32_t* d_counts, int depth, int levels, double eps, int max_depth, double* d_acc,
                             const LeafSink* sink) {
    if (!ctx || !d_buf0 || !d_buf1 || !d_counts || !d_acc || levels < 0) return AQ_EINVAL;
    if (!integrand_ok(integrand)) return AQ_EINVAL;
    if (!(eps >= 0.0) || depth < 0 || max_depth < 1 || max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    if (levels == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    with_fid(integrand, [&](auto F) {
        if (sink)
            hipLaunchKernelGGL((k_level_narrow<decltype(F)::value, LeafSink>), dim3(1), dim3(NARROW_T), 0, ctx->stream,
                               (Rec*)d_buf0, (Rec*)d_buf1, cap, d_counts, depth, levels, eps, max_depth, d_acc,
                               ctx->d_tab, *sink);
        else
            hipLaunchKernelGGL((k_level_narrow<decltype(F)::value>), dim3(1), dim3(NARROW_T), 0, ctx->stream,
                               (Rec*)d_buf0, (Rec*)d_buf1, cap, d_counts, depth, levels, eps, max_depth, d_acc,
                               ctx->d_tab);
    });
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

int aq_level_narrow(aq_ctx* ctx, int integrand, double* d_buf0, double* d_buf1, uint32_t cap, uint32_t* d_counts,
                    int depth, int levels, double eps, int max_depth, double* d_acc) {
    return level_narrow_impl(ctx, integrand, d_buf0, d_buf1, cap, d_counts, depth, levels, eps, max_depth, d_acc,
                             nullptr);
}

// The host side of a frontier walk, which aq_frontier_integrate / aq_integrate_mesh, aq_integrate_mesh_batch and
// aq_mesh_refine_batch share. The loop itself is aq_frontier_walk.h's, and the callers differ in its four
// parameters alone (FrontierWalk). A caller runs walk_begin, puts its first records and their count in place (the
// root and the narrow top; the rows' roots; the retested leaves' children in the seed buffer), then walk_run.
//
// walk_begin: the context's frontier buffers for `cap` records a level, the counts and the accumulator zeroed.
static int walk_begin(aq_ctx* ctx, uint32_t cap) {
    if (int rc = ctx->front.ensure_walk(cap)) return rc;
    AQ_HIP(hipMemsetAsync(ctx->front.d_count, 0, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), ctx->stream));
    AQ_HIP(hipMemsetAsync(ctx->front.d_acc, 0, sizeof(double) * 8, ctx->stream));
    return AQ_OK;
}

// What a walk left, read back and decoded (all zero unless `back`: the one wait behind the walk was reached).
struct WalkOut {
    bool back;
    const unsigned* counts;   // [AQ_MAX_LEVELS + 2] the records of every depth (pinned: until the next walk)
    double area_hi, area_lo;
    unsigned long long tasks, leaves;
    unsigned error;           // ERRB_* bits
    unsigned levels, widest;  // the deepest level stepped + 1; the widest level's records
    bool depth_left;          // records left at the depth the walk ended at: AQ_EDEPTH
};

// Level steps leave their rows for one later fold while this lives; defer_fold is put back on every way out.
struct DeferFold {
    aq_ctx* ctx;
    const bool was;
    explicit DeferFold(aq_ctx* c) : ctx(c), was(c->defer_fold) { c->defer_fold = true; }
    ~DeferFold() { ctx->defer_fold = was; }
};

// walk_run: chained level steps with deferred folds and a host look every w.sync_every levels, one fold of what is
// pending whether the walk succeeded or not, then the read-backs and ONE wait. `sink` chooses the step's instance;
// the batch form's rows travel in the mesh group's row arrays beside the frontier buffers. A walk with a seed table
// (w.seed_end: aq_mesh_refine_batch) appends from the mesh group's seed buffer and reads the depth table back too;
// the batch form reads the leaf count and the invalid rows back (h_bwords) -- all in front of the one wait.
static int walk_run(aq_ctx* ctx, const FrontierWalk& w, int integrand, double eps, const StepSink& sink, WalkOut* out) {
    FrontBufs& fb = ctx->front;
    MeshBufs& mb = ctx->mesh;
    unsigned* cnt = fb.d_count;
    double* acc = fb.d_acc;
    double* buf[2] = {reinterpret_cast<double*>(fb.d_rec[0].get()), reinterpret_cast<double*>(fb.d_rec[1].get())};
    unsigned* row[2] = {mb.d_brow[0].get(), mb.d_brow[1].get()};
    const uint32_t cap = (uint32_t)w.cap;
    const bool batch = sink.kind == StepSink::BATCH;
    *out = WalkOut{};
    DeferFold guard(ctx);
    const WalkEnd end = frontier_walk(
        w,   // seed, step, look:
        [&](int depth, unsigned long long ns) -> int {
            const unsigned long long at = w.seed_end[depth - 1];
            hipLaunchKernelGGL(k_mesh_refine_append, dim3((unsigned)((ns + REFINE_APPEND - 1) / REFINE_APPEND)), dim3(256), 0,
                               ctx->stream, (const Rec*)(mb.d_rseed.get() + at), (const unsigned*)(mb.d_rseedrow.get() + at),
                               (unsigned)ns, (Rec*)buf[depth & 1], row[depth & 1], cnt + depth, cap,
                               mb.d_rtab.get() + REFINE_TAB_ERR);
            AQ_HIP(hipGetLastError());
            return AQ_OK;
        },
        [&](int depth, unsigned long long n_in) -> int {
            StepSink s = sink;
            if (batch) s.batch.row_in = row[depth & 1], s.batch.row_out = row[(depth + 1) & 1];
            return level_step_impl(ctx, integrand, buf[depth & 1], (uint32_t)n_in, cnt + depth, buf[(depth + 1) & 1], cap, eps,
                                   depth, w.max_depth, cnt + depth + 1, acc, s);
        },
        [&](int depth, unsigned long long* now) -> int {
            if (int rc = fold_pending(ctx)) return rc;
            AQ_HIP(hipMemcpyAsync(fb.h_count, cnt + depth, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
            AQ_HIP(hipStreamSynchronize(ctx->stream));
            *now = fb.h_count[0];
            return AQ_OK;
        });
    int rc = end.rc;
    if (rc == AQ_OK) rc = fold_pending(ctx);
    else (void)fold_pending(ctx);
    AQ_HIP(hipMemcpyAsync(fb.h_count, cnt, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(fb.h_acc, acc, sizeof(double) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (batch) {
        AQ_HIP(hipMemcpyAsync(mb.h_bwords, mb.d_leafcnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        AQ_HIP(hipMemcpyAsync(mb.h_bwords + 1, mb.d_binvalid, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              ctx->stream));
    }
    if (w.seed_end)
        AQ_HIP(hipMemcpyAsync(mb.h_rtab, mb.d_rtab, sizeof(unsigned) * REFINE_TAB_WORDS, hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    const double* a = fb.h_acc;
    const unsigned* c = fb.h_count;
    *out = WalkOut{true, c, a[0], a[1], (unsigned long long)a[2], (unsigned long long)a[3], (unsigned)a[4], (unsigned)a[5],
                   *std::max_element(c, c + AQ_MAX_LEVELS + 2), !w.empty() && c[std::min(end.depth, AQ_MAX_LEVELS + 1)] > 0};
    return rc;
}

// aq_frontier_integrate's run: the frontier engine of ppls_amd/frontier.py for ONE GPU with its host loop in C --
// the root, the narrow top in one launch (<= 2^12 records a level), then the walk from there (the Python loop's
// per-level torch / ctypes work, several us a level, is what this saves). With `sink`, the same run through the
// leaf-emitting kernels (aq_integrate_mesh).
static int frontier_run(aq_ctx* ctx, const aq_problem* p, uint32_t cap, int sync_every, aq_result* res,
                        uint64_t* tpl, uint64_t* lpl, int maxlev, const LeafSink* sink) {
    if (!ctx || cap < 2 || sync_every < 1 || maxlev < 0) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    AQ_HIP(hipSetDevice(ctx->device));
    const int max_depth = p->max_depth ? p->max_depth : AQ_DEFAULT_MAX_DEPTH;
    if ((rc = walk_begin(ctx, cap))) return rc;
    unsigned* cnt = ctx->front.d_count;
    double* buf[2] = {reinterpret_cast<double*>(ctx->front.d_rec[0].get()),
                      reinterpret_cast<double*>(ctx->front.d_rec[1].get())};
    AQ_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cnt), 1, 1, ctx->stream));   // counts[0] = the root
    if ((rc = aq_frontier_root(ctx, p->integrand, p->a, p->b, buf[0]))) return rc;
    const int top = std::max(std::min(13, max_depth - 1), 0);   // the narrow top: one launch
    if (top > 0 && (rc = level_narrow_impl(ctx, p->integrand, buf[0], buf[1], cap, cnt, 0, top, p->eps, max_depth,
                                           ctx->front.d_acc, sink)))
        return rc;
    const FrontierWalk w{top, std::min<unsigned long long>(1ull << top, cap), cap, max_depth, sync_every};
    WalkOut o;
    if ((rc = walk_run(ctx, w, p->integrand, p->eps, sink ? StepSink(*sink) : StepSink(), &o))) return rc;
    HostOut& h = ctx->last;
    h = HostOut();
    h.area = o.area_hi + o.area_lo;
    h.tasks = o.tasks;
    h.leaves = o.leaves;
    h.error = o.error;
    h.levels = o.levels;
    for (int d = 0; d < AQ_MAX_LEVELS; ++d) {
        h.hist[d] = o.counts[d];
        h.hist[AQ_MAX_LEVELS + d] = o.counts[d] - o.counts[d + 1] / 2u;
    }
    ctx->last_valid = true;
    fill_result(ctx, h, res);
    if ((rc = err_from_bits(h.error))) return rc;
    if (o.depth_left) return AQ_EDEPTH;
    return aq_level_histogram(ctx, tpl, lpl, maxlev);
}

int aq_frontier_integrate(aq_ctx* ctx, const aq_problem* p, uint32_t cap, int sync_every, aq_result* res,
                          uint64_t* tpl, uint64_t* lpl, int maxlev) {
    return frontier_run(ctx, p, cap, sync_every, res, tpl, lpl, maxlev, nullptr);
}

// The accepted mesh: the frontier run through the leaf-emitting kernels, then leaves -> sorted nodes (aquad.hip
// k_mesh_*). Everything after the run is enqueued on the context's stream and waited for once.
int aq_integrate_mesh(aq_ctx* ctx, const aq_problem* p, uint32_t frontier_cap, int sync_every, uint64_t cap_nodes,
                      const aq_mesh_io* io, aq_result* res, uint64_t* n_nodes) {
    if (!ctx || !p || !io || !n_nodes || !io->x || !io->f || !io->cum) return AQ_EINVAL;
    if (cap_nodes < 3 || cap_nodes > (1ull << 31)) return AQ_EINVAL;
    if (frontier_cap < 2 || sync_every < 1) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    if (p->integrand == AQ_F_PARAM) return AQ_EINVAL;   // the frontier engine takes no theta
    *n_nodes = 0;
    AQ_HIP(hipSetDevice(ctx->device));
    const size_t cap_leaves = (size_t)((cap_nodes - 1) / 2);
    MeshBufs& mb = ctx->mesh;
    if ((rc = mb.ensure_leaves(cap_leaves))) return rc;
    AQ_HIP(hipMemsetAsync(mb.d_leafcnt, 0, sizeof(unsigned long long), ctx->stream));
    const LeafSink sink{mb.d_leaf, mb.d_leafcnt, (unsigned long long)cap_leaves};
    aq_result local{};
    aq_result* r = res ? res : &local;
    if ((rc = frontier_run(ctx, p, frontier_cap, sync_every, r, nullptr, nullptr, 0, &sink))) return rc;
    const uint64_t leaves = r->accepted;   // every accepted task emitted (or, past the capacity, counted) one leaf
    *n_nodes = 2 * leaves + 1;
    if (*n_nodes > cap_nodes) return AQ_EOVERFLOW;
    const unsigned n = (unsigned)leaves;
    const unsigned grid = (n + MESH_T - 1) / MESH_T;
    hipError_t he = hipSuccess;
    const size_t sort_bytes = mesh_sort_scratch_bytes(n, &he);
    AQ_HIP(he);
    if ((rc = mb.ensure_sort(n, sort_bytes, grid))) return rc;
    hipLaunchKernelGGL(k_mesh_keys, dim3(grid), dim3(MESH_T), 0, ctx->stream, mb.d_leaf.get(), n, mb.d_mkey[0].get(),
                       mb.d_midx[0].get());
    AQ_HIP(hipGetLastError());
    AQ_HIP(mesh_sort(mb.d_msort, sort_bytes, mb.d_mkey[0], mb.d_mkey[1], mb.d_midx[0], mb.d_midx[1], n, ctx->stream));
    // node pairs go out as one 16-byte store where the caller's arrays allow
    const bool vec = (((uintptr_t)io->x | (uintptr_t)io->f | (uintptr_t)io->cum) & 15u) == 0;
    const Leaf* lv = mb.d_leaf;
    const unsigned* idx = mb.d_midx[1];
    double2* parts = mb.d_mparts;
    if (vec)
        hipLaunchKernelGGL(k_mesh_expand<true>, dim3(grid), dim3(MESH_T), 0, ctx->stream, lv, idx, n, io->x, io->f,
                           io->cum, io->level, parts);
    else
        hipLaunchKernelGGL(k_mesh_expand<false>, dim3(grid), dim3(MESH_T), 0, ctx->stream, lv, idx, n, io->x, io->f,
                           io->cum, io->level, parts);
    AQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mesh_scan_parts, dim3(1), dim3(MESH_T), 0, ctx->stream, parts, grid);
    AQ_HIP(hipGetLastError());
    if (vec)
        hipLaunchKernelGGL(k_mesh_cum<true>, dim3(grid), dim3(MESH_T), 0, ctx->stream, n, io->cum, (const double2*)parts);
    else
        hipLaunchKernelGGL(k_mesh_cum<false>, dim3(grid), dim3(MESH_T), 0, ctx->stream, n, io->cum, (const double2*)parts);
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return AQ_OK;
}

// The back half of aq_integrate_mesh_batch, which aq_mesh_refine_batch shares: the nl leaves of n rows in the context's
// leaf buffer, in any order, sorted by (row, l) and laid out row after row (aquad.hip k_mesh_batch_*). Waits.
static int mesh_batch_back(aq_ctx* ctx, size_t n, const aq_mesh_batch_io* io, unsigned nl) {
    MeshBufs& mb = ctx->mesh;
    const unsigned nr = (unsigned)n;
    const unsigned grid = (nl + MESH_T - 1) / MESH_T, rgrid = (nr + 1 + MESH_T - 1) / MESH_T;
    unsigned bits = 0;
    while (bits < 32 && ((uint64_t)(n - 1) >> bits) != 0) ++bits;   // ceil(log2 n): the rows are < n
    const unsigned* idx = nullptr;
    if (nl > 0) {
        hipError_t he = hipSuccess;
        size_t sort_bytes = mesh_sort_scratch_bytes(nl, &he);
        AQ_HIP(he);
        if (n > 1) {
            sort_bytes = std::max(sort_bytes, mesh_sort_rows_scratch_bytes(nl, bits, &he));
            AQ_HIP(he);
        }
        if (int rc = mb.ensure_sort(nl, sort_bytes, grid, n)) return rc;
        hipLaunchKernelGGL(k_mesh_keys, dim3(grid), dim3(MESH_T), 0, ctx->stream, mb.d_leaf.get(), nl,
                           mb.d_mkey[0].get(), mb.d_midx[0].get());
        AQ_HIP(hipGetLastError());
        AQ_HIP(mesh_sort(mb.d_msort, sort_bytes, mb.d_mkey[0], mb.d_mkey[1], mb.d_midx[0], mb.d_midx[1], nl,
                         ctx->stream));
        idx = mb.d_midx[1];
        if (n > 1) {   // the second, stable pass: by row
            hipLaunchKernelGGL(k_mesh_batch_rowkeys, dim3(grid), dim3(MESH_T), 0, ctx->stream, mb.d_leaf.get(), idx, nl,
                               mb.d_bkey[0].get());
            AQ_HIP(hipGetLastError());
            AQ_HIP(mesh_sort_rows(mb.d_msort, sort_bytes, mb.d_bkey[0], mb.d_bkey[1], mb.d_midx[1], mb.d_midx[0],
                                  nl, bits, ctx->stream));
            idx = mb.d_midx[0];
        }
    }
    const Leaf* lv = mb.d_leaf;
    unsigned* first = mb.d_bfirst;
    hipLaunchKernelGGL(k_mesh_batch_first, dim3(rgrid), dim3(MESH_T), 0, ctx->stream, lv, idx, nl, nr, first);
    AQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mesh_batch_offsets, dim3(1), dim3(MESH_T), 0, ctx->stream, (const unsigned*)first, nr,
                       (unsigned long long*)io->offsets);
    AQ_HIP(hipGetLastError());
    if (nl > 0) {
        double2* parts = mb.d_mparts;
        hipLaunchKernelGGL(k_mesh_batch_expand, dim3(grid), dim3(MESH_T), 0, ctx->stream, lv, idx, nl,
                           (const unsigned*)first, (const unsigned long long*)io->offsets, io->x, io->f, io->cum,
                           io->level, mb.d_bnode.get(), parts, mb.d_bpflag.get());
        AQ_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_mesh_batch_scan_parts, dim3(1), dim3(MESH_T), 0, ctx->stream, parts,
                           (const unsigned*)mb.d_bpflag.get(), grid);
        AQ_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_mesh_batch_cum, dim3(grid), dim3(MESH_T), 0, ctx->stream, nl,
                           (const unsigned*)mb.d_bnode.get(), io->cum, (const double2*)parts);
        AQ_HIP(hipGetLastError());
    }
    if (io->area || io->accepted || io->tasks) {
        hipLaunchKernelGGL(k_mesh_batch_finish, dim3(rgrid), dim3(MESH_T), 0, ctx->stream, nr, (const unsigned*)first,
                           (const unsigned long long*)io->offsets, (const double*)io->cum, io->area,
                           (unsigned long long*)io->accepted, (unsigned long long*)io->tasks);
        AQ_HIP(hipGetLastError());
    }
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return AQ_OK;
}

// Many meshes per call: frontier_run's walk over ONE frontier that holds every row's records of a depth, from depth 0
// (the valid rows' roots, compacted by k_mesh_batch_roots; no narrow top -- level 0 is already n records wide, and a
// small batch's few narrow levels cost a launch each as a lone mesh's levels past the top do), then the leaves
// ordered by (row, l) and laid out row after row (aquad.hip k_mesh_batch_*). Blocks, as aq_integrate_mesh does.
int aq_integrate_mesh_batch(aq_ctx* ctx, size_t n, const aq_mesh_batch_io* io, double eps, int integrand,
                            uint32_t frontier_cap, int sync_every, uint64_t cap_nodes, aq_mesh_batch_info* info) {
    if (!ctx || !io || !info || !io->a || !io->b || !io->offsets || !io->x || !io->f || !io->cum) return AQ_EINVAL;
    if (!theta_ok(integrand, io->theta)) return AQ_EINVAL;
    if (!(eps >= 0.0) || io->max_depth < 0 || io->max_depth > AQ_MAX_LEVELS - 1 || sync_every < 1) return AQ_EINVAL;
    if (frontier_cap < std::max<size_t>(n, 2)) return AQ_EINVAL;
    if (cap_nodes < 3 || cap_nodes > (1ull << 31)) return AQ_EINVAL;
    *info = aq_mesh_batch_info{};
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    const int max_depth = io->max_depth ? io->max_depth : AQ_DEFAULT_MAX_DEPTH;
    const uint32_t cap = frontier_cap;
    const unsigned nr = (unsigned)n;   // n <= frontier_cap < 2^32
    const size_t cap_leaves = (size_t)(cap_nodes / 2);   // a mesh that fits has at most (cap_nodes - 1) / 2 leaves
    MeshBufs& mb = ctx->mesh;
    int rc;
    if ((rc = mb.ensure_batch(n, cap, cap_leaves, !io->status, false))) return rc;
    if ((rc = walk_begin(ctx, cap))) return rc;
    unsigned* status = io->status ? io->status : mb.d_bstatus.get();
    AQ_HIP(hipMemsetAsync(mb.d_leafcnt, 0, sizeof(unsigned long long), ctx->stream));
    AQ_HIP(hipMemsetAsync(mb.d_binvalid, 0, sizeof(unsigned long long), ctx->stream));
    with_stream_fid(integrand, [&](auto F) {
        hipLaunchKernelGGL((k_mesh_batch_roots<decltype(F)::value>), dim3((nr + 255u) / 256u), dim3(256), 0, ctx->stream,
                           io->a, io->b, io->theta, nr, ctx->front.d_rec[0].get(), mb.d_brow[0].get(),
                           ctx->front.d_count.get(), status, mb.d_binvalid.get(), ctx->d_tab);
    });
    AQ_HIP(hipGetLastError());
    const FrontierWalk w{0, nr, cap, max_depth, sync_every};   // from depth 0, which holds at most n records
    const BatchSink sink{LeafSink{mb.d_leaf, mb.d_leafcnt, (unsigned long long)cap_leaves}, nullptr, nullptr, io->theta,
                         status, nr};   // (the rows' arrays of a depth: walk_run's)
    WalkOut o;
    rc = walk_run(ctx, w, integrand, eps, sink, &o);
    if (o.back) info->invalid_rows = mb.h_bwords[1];
    if (rc) return rc;
    if ((rc = err_from_bits(o.error))) return rc;   // a level past frontier_cap, or a refine at max_depth
    if (o.depth_left) return AQ_EDEPTH;
    const uint64_t leaves = mb.h_bwords[0];   // every accepted task emitted (or, past the capacity, counted) one leaf
    info->leaves = leaves;
    info->tasks = o.tasks;
    info->levels = o.levels;
    info->widest_level = o.widest;
    info->n_nodes = 2 * leaves + (n - info->invalid_rows);
    if (info->n_nodes > cap_nodes) return AQ_EOVERFLOW;
    return mesh_batch_back(ctx, n, io, (unsigned)leaves);
}

// A batch mesh continued to a smaller eps: aq_integrate_mesh_batch with its roots kernel replaced by the retest of
// the input's leaves (aquad.hip k_mesh_refine_*). The survivors go straight to the leaf buffer; the failing leaves'
// children wait in the seed buffer, one segment per depth, and join the frontier of their depth just before that
// depth's step. The walk starts at the first depth that has seeds and ends at an empty level only when no deeper
// segment is left (aq_frontier_walk.h). Two host looks before the walk: the input's node count, then the per-depth
// counts.
int aq_mesh_refine_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_x, const double* d_f,
                         const uint8_t* d_level, const double* d_theta, const uint8_t* d_active, double eps, int integrand,
                         const aq_mesh_batch_io* out, uint32_t frontier_cap, int sync_every, uint64_t cap_nodes,
                         aq_mesh_refine_info* info) {
    if (!ctx || !out || !info || !out->offsets || !out->x || !out->f || !out->cum) return AQ_EINVAL;
    if (n > 0 && (!d_offsets || !d_x || !d_f || !d_level)) return AQ_EINVAL;
    if (!theta_ok(integrand, d_theta)) return AQ_EINVAL;
    if (!(eps >= 0.0) || out->max_depth < 0 || out->max_depth > AQ_MAX_LEVELS - 1 || sync_every < 1) return AQ_EINVAL;
    if (frontier_cap < 2 || n > 0x7fffffffull) return AQ_EINVAL;
    if (cap_nodes < 3 || cap_nodes > (1ull << 31)) return AQ_EINVAL;
    *info = aq_mesh_refine_info{};
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    const int max_depth = out->max_depth ? out->max_depth : AQ_DEFAULT_MAX_DEPTH;
    const uint32_t cap = frontier_cap;
    const unsigned nr = (unsigned)n;
    const size_t cap_leaves = (size_t)(cap_nodes / 2);
    MeshBufs& mb = ctx->mesh;
    int rc;
    if ((rc = mb.ensure_batch(n, cap, cap_leaves, !out->status, true))) return rc;
    unsigned* tab = mb.d_rtab;
    unsigned* status = out->status ? out->status : mb.d_bstatus.get();
    AQ_HIP(hipMemcpyAsync(mb.h_rnodes, d_offsets + n, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = walk_begin(ctx, cap))) return rc;
    AQ_HIP(hipMemsetAsync(tab, 0, sizeof(unsigned) * REFINE_TAB_WORDS, ctx->stream));
    AQ_HIP(hipMemsetAsync(mb.d_leafcnt, 0, sizeof(unsigned long long), ctx->stream));
    AQ_HIP(hipMemsetAsync(mb.d_binvalid, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_mesh_refine_rows, dim3((nr + REFINE_T - 1) / REFINE_T), dim3(REFINE_T), 0, ctx->stream,
                       (const unsigned long long*)d_offsets, nr, status, mb.d_binvalid.get());
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipStreamSynchronize(ctx->stream));   // the first look: the input's nodes
    const unsigned long long m_in = mb.h_rnodes[0];
    if (m_in > (1ull << 31)) return AQ_EINVAL;
    const RefineIn in{(const unsigned long long*)d_offsets, d_x, d_f, d_level, d_active, nr, m_in, eps, max_depth};
    const unsigned cgrid = (unsigned)((m_in + REFINE_T - 1) / REFINE_T);
    const LeafSink lsink{mb.d_leaf, mb.d_leafcnt, (unsigned long long)cap_leaves};
    if (cgrid) {
        hipLaunchKernelGGL(k_mesh_refine_classify, dim3(cgrid), dim3(REFINE_T), 0, ctx->stream, in, lsink, status, tab);
        AQ_HIP(hipGetLastError());
    }
    AQ_HIP(hipMemcpyAsync(mb.h_rtab, tab, sizeof(unsigned) * REFINE_TAB_WORDS, hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));   // the second look: the failing leaves by depth
    unsigned long long seg[AQ_MAX_LEVELS + 1];   // the seed records of depth e are [seg[e - 1], seg[e])
    int first_depth = -1, last_depth = -1;       // the first and the last depth that has seeds
    unsigned long long pre = 0;
    for (int d = 0; d < AQ_MAX_LEVELS; ++d) {    // the children of the failing leaves of depth d: depth d + 1
        seg[d] = 2 * pre;
        if (mb.h_rtab[d]) {
            if (first_depth < 0) first_depth = d + 1;
            last_depth = d + 1;
        }
        pre += mb.h_rtab[d];
    }
    seg[AQ_MAX_LEVELS] = 2 * pre;
    const unsigned long long n_seed = 2 * pre;   // <= the input's nodes <= 2^31
    const unsigned deep_fail = mb.h_rtab[REFINE_TAB_DEPTHFAIL];
    info->reseeded = pre + deep_fail;
    if (n_seed) {
        AQ_HIP(mb.d_rseed.grow(n_seed));
        AQ_HIP(mb.d_rseedrow.grow(n_seed));
        hipLaunchKernelGGL(k_mesh_refine_seed, dim3(cgrid), dim3(REFINE_T), 0, ctx->stream, in, tab, mb.d_rseed.get(),
                           mb.d_rseedrow.get(), n_seed);
        AQ_HIP(hipGetLastError());
    }
    // from the first depth that has seeds, empty until they join; nothing to walk without any
    const FrontierWalk w{std::max(first_depth, 0), 0, cap, max_depth, sync_every, seg, last_depth};
    const BatchSink sink{lsink, nullptr, nullptr, d_theta, status, nr};   // (the rows' arrays of a depth: walk_run's)
    WalkOut o;
    if ((rc = walk_run(ctx, w, integrand, eps, sink, &o))) return rc;
    info->evaluated = o.tasks;
    // a level past frontier_cap (a step's children, or the seeds behind them), or a refine at max_depth (a failing
    // input leaf, or a later task)
    if ((rc = err_from_bits(o.error | mb.h_rtab[REFINE_TAB_ERR] | (deep_fail ? (unsigned)ERRB_DEPTH : 0u)))) return rc;
    if (o.depth_left) return AQ_EDEPTH;
    const uint64_t leaves = mb.h_bwords[0], with_nodes = n - mb.h_bwords[1];
    info->leaves = leaves;
    info->tasks = 2 * leaves - with_nodes;
    info->levels = std::max((uint32_t)o.levels, (uint32_t)mb.h_rtab[REFINE_TAB_LEVELS]);
    info->widest_level = o.widest;
    info->n_nodes = 2 * leaves + with_nodes;
    if (info->n_nodes > cap_nodes) return AQ_EOVERFLOW;
    return mesh_batch_back(ctx, n, out, (unsigned)leaves);
}

// Σ|d| and Σd of every row of a batch mesh (aquad.hip k_mesh_err_*). Only enqueues.
int aq_mesh_err_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_x, const double* d_f,
                      double* d_err_abs, double* d_err_signed) {
    if (!ctx) return AQ_EINVAL;
    if (n > 0 && (!d_offsets || !d_x || !d_f)) return AQ_EINVAL;
    if (n == 0 || (!d_err_abs && !d_err_signed)) return AQ_OK;
    if (n > 0x7fffffffull / MESH_ERR_B) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    AQ_HIP(ctx->mesh.d_eparts.grow(n * MESH_ERR_B));
    hipLaunchKernelGGL(k_mesh_err_parts, dim3((unsigned)(n * MESH_ERR_B)), dim3(MESH_T), 0, ctx->stream,
                       (const unsigned long long*)d_offsets, d_x, d_f, ctx->mesh.d_eparts.get());
    AQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mesh_err_finish, dim3((unsigned)((n + MESH_T - 1) / MESH_T)), dim3(MESH_T), 0, ctx->stream,
                       (const unsigned long long*)d_offsets, (unsigned)n, (const double4*)ctx->mesh.d_eparts.get(), d_err_abs,
                       d_err_signed);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

// M_0 .. M_order of every row of a batch mesh over the row's range (aquad.hip k_mesh_moments_*). Only enqueues.
int aq_mesh_moments_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_x, const double* d_f,
                          int order, const double* d_center, const double* d_lo, const double* d_hi, double* d_out) {
    static_assert(AQ_MESH_MAX_MOMENT == 4, "one instance of k_mesh_moments_parts per order");
    if (!ctx) return AQ_EINVAL;
    if (order < 0 || order > AQ_MESH_MAX_MOMENT) return AQ_EINVAL;
    if (n > 0 && (!d_offsets || !d_x || !d_f || !d_out)) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    if (n > 0x7fffffffull / MESH_MOM_B) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    AQ_HIP(ctx->mesh.d_momparts.grow(n * MESH_MOM_B * (size_t)(order + 1)));
    using Parts = void (*)(const unsigned long long*, const double*, const double*, const double*, const double*,
                           const double*, double2*);
    static const Parts parts[AQ_MESH_MAX_MOMENT + 1] = {k_mesh_moments_parts<0>, k_mesh_moments_parts<1>, k_mesh_moments_parts<2>,
                                                        k_mesh_moments_parts<3>, k_mesh_moments_parts<4>};
    hipLaunchKernelGGL(parts[order], dim3((unsigned)(n * MESH_MOM_B)), dim3(MESH_T), 0, ctx->stream,
                       (const unsigned long long*)d_offsets, d_x, d_f, d_center, d_lo, d_hi, ctx->mesh.d_momparts.get());
    AQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mesh_moments_finish, dim3((unsigned)((n + MESH_T - 1) / MESH_T)), dim3(MESH_T), 0, ctx->stream,
                       (const unsigned long long*)d_offsets, (unsigned)n, d_x, order, d_lo, d_hi,
                       (const double2*)ctx->mesh.d_momparts.get(), d_out);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

// Mesh coarsening (aquad.hip k_mesh_coarsen_*, k_mesh_budget_*). The three calls block, and each begins with one host
// look: the input's node count, offsets[n].
static int coarsen_nodes(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, unsigned long long* m_in) {
    MeshBufs& mb = ctx->mesh;
    AQ_HIP(mb.h_rnodes.grow(1));
    AQ_HIP(hipMemcpyAsync(mb.h_rnodes, d_offsets + n, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    *m_in = mb.h_rnodes[0];
    return *m_in > (1ull << 31) ? AQ_EINVAL : AQ_OK;
}

// The leaves' positions and rows of `in` (n_nodes > 0) into the context's scratch, enqueued.
static int coarsen_positions(aq_ctx* ctx, const CoarsenIn& in) {
    MeshBufs& mb = ctx->mesh;
    const unsigned long long slots = (in.n_nodes + 1) / 2;
    AQ_HIP(hipMemsetAsync(mb.d_crow, 0xff, sizeof(unsigned) * slots, ctx->stream));
    hipLaunchKernelGGL(k_mesh_coarsen_pos, dim3(in.n_rows), dim3(COARSEN_T), 0, ctx->stream, in, mb.d_cpos.get(),
                       mb.d_crow.get());
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

// The thresholds of `in` (n_nodes > 0) into thr, enqueued; the positions and rows stay in the context's scratch.
static int coarsen_thresholds(aq_ctx* ctx, const CoarsenIn& in, double* thr) {
    MeshBufs& mb = ctx->mesh;
    const unsigned long long slots = (in.n_nodes + 1) / 2;
    const unsigned sgrid = (unsigned)((slots + COARSEN_T - 1) / COARSEN_T);
    if (int rc = coarsen_positions(ctx, in)) return rc;
    hipLaunchKernelGGL(k_mesh_coarsen_node, dim3(sgrid), dim3(COARSEN_T), 0, ctx->stream, in, slots,
                       (const ulonglong2*)mb.d_cpos.get(), (const unsigned*)mb.d_crow.get(), mb.d_cdabs.get(),
                       mb.d_cpar.get());
    AQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mesh_coarsen_thr, dim3(sgrid), dim3(COARSEN_T), 0, ctx->stream, in, slots,
                       (const unsigned*)mb.d_crow.get(), (const double*)mb.d_cdabs.get(), (const unsigned*)mb.d_cpar.get(),
                       thr);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

int aq_mesh_thresholds_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_x, const double* d_f,
                             const uint8_t* d_level, double* d_thr) {
    if (!ctx) return AQ_EINVAL;
    if (n > 0 && (!d_offsets || !d_x || !d_f || !d_level || !d_thr)) return AQ_EINVAL;
    if (n > 0x7fffffffull) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    unsigned long long m_in = 0;
    int rc;
    if ((rc = coarsen_nodes(ctx, n, d_offsets, &m_in))) return rc;
    if (m_in == 0) return AQ_OK;
    if ((rc = ctx->mesh.ensure_coarsen(m_in, false))) return rc;
    const CoarsenIn in{(const unsigned long long*)d_offsets, d_x, d_f, d_level, (unsigned)n, m_in};
    if ((rc = coarsen_thresholds(ctx, in, d_thr))) return rc;
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return AQ_OK;
}

// The nodes sorted by (row, key) -- the back half's two passes over the mesh's sort arrays -- then one pick per row.
int aq_mesh_budget_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_thr, uint64_t max_leaves,
                         double* d_eps) {
    if (!ctx || max_leaves < 1) return AQ_EINVAL;
    if (n > 0 && (!d_offsets || !d_thr || !d_eps)) return AQ_EINVAL;
    if (n > 0x7fffffffull) return AQ_EINVAL;
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    MeshBufs& mb = ctx->mesh;
    unsigned long long m_in = 0;
    int rc;
    if ((rc = coarsen_nodes(ctx, n, d_offsets, &m_in))) return rc;
    const unsigned nr = (unsigned)n;
    const unsigned long long* off = (const unsigned long long*)d_offsets;
    const unsigned* idx = nullptr;
    if (m_in > 0) {
        const unsigned grid = (unsigned)((m_in + COARSEN_T - 1) / COARSEN_T);
        unsigned bits = 0;
        while (bits < 32 && ((uint64_t)(n - 1) >> bits) != 0) ++bits;   // ceil(log2 n): the rows are < n
        hipError_t he = hipSuccess;
        size_t sort_bytes = mesh_sort_scratch_bytes(m_in, &he);
        AQ_HIP(he);
        if (n > 1) {
            sort_bytes = std::max(sort_bytes, mesh_sort_rows_scratch_bytes(m_in, bits, &he));
            AQ_HIP(he);
        }
        if ((rc = mb.ensure_sort(m_in, sort_bytes, grid, n))) return rc;
        unsigned* row_of = mb.d_bnode;   // [m_in]: the nodes' rows
        hipLaunchKernelGGL(k_mesh_budget_keys, dim3(grid), dim3(COARSEN_T), 0, ctx->stream, off, nr, m_in, d_thr,
                           mb.d_mkey[0].get(), mb.d_midx[0].get(), row_of);
        AQ_HIP(hipGetLastError());
        AQ_HIP(mesh_sort(mb.d_msort, sort_bytes, mb.d_mkey[0], mb.d_mkey[1], mb.d_midx[0], mb.d_midx[1], m_in,
                         ctx->stream));
        idx = mb.d_midx[1];
        if (n > 1) {
            hipLaunchKernelGGL(k_mesh_budget_rowkeys, dim3(grid), dim3(COARSEN_T), 0, ctx->stream, (const unsigned*)row_of,
                               idx, m_in, mb.d_bkey[0].get());
            AQ_HIP(hipGetLastError());
            AQ_HIP(mesh_sort_rows(mb.d_msort, sort_bytes, mb.d_bkey[0], mb.d_bkey[1], mb.d_midx[1], mb.d_midx[0], m_in,
                                  bits, ctx->stream));
            idx = mb.d_midx[0];
        }
    }
    hipLaunchKernelGGL(k_mesh_budget_pick, dim3((nr + COARSEN_T - 1) / COARSEN_T), dim3(COARSEN_T), 0, ctx->stream, off, nr,
                       m_in, d_thr, idx, (unsigned long long)max_leaves, d_eps);
    AQ_HIP(hipGetLastError());
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return AQ_OK;
}

// Any coarser mesh from a fine one: the heads' leaf records into the context's leaf buffer, then the back half of
// aq_integrate_mesh_batch, unchanged. A second host look, behind the emission: the output's leaves.
int aq_mesh_coarsen_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_x, const double* d_f,
                          const uint8_t* d_level, const double* d_thr, const double* d_eps, double eps,
                          const aq_mesh_batch_io* out, uint64_t cap_nodes, aq_mesh_coarsen_info* info) {
    if (!ctx || !out || !info || !out->offsets || !out->x || !out->f || !out->cum) return AQ_EINVAL;
    if (n > 0 && (!d_offsets || !d_x || !d_f || !d_level)) return AQ_EINVAL;
    if (!d_eps && !(eps >= 0.0)) return AQ_EINVAL;
    if (n > 0x7fffffffull || cap_nodes < 3 || cap_nodes > (1ull << 31)) return AQ_EINVAL;
    *info = aq_mesh_coarsen_info{};
    if (n == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    MeshBufs& mb = ctx->mesh;
    const unsigned nr = (unsigned)n;
    const size_t cap_leaves = (size_t)(cap_nodes / 2);
    unsigned long long m_in = 0;
    int rc;
    if ((rc = coarsen_nodes(ctx, n, d_offsets, &m_in))) return rc;
    if ((rc = mb.ensure_batch(n, 0, cap_leaves, !out->status, true))) return rc;   // (no frontier: no row arrays)
    if ((rc = mb.ensure_coarsen(m_in, !d_thr))) return rc;
    unsigned* status = out->status ? out->status : mb.d_bstatus.get();
    unsigned* levels = mb.d_rtab.get() + REFINE_TAB_LEVELS;
    AQ_HIP(hipMemsetAsync(levels, 0, sizeof(unsigned), ctx->stream));
    AQ_HIP(hipMemsetAsync(mb.d_leafcnt, 0, sizeof(unsigned long long), ctx->stream));
    AQ_HIP(hipMemsetAsync(mb.d_binvalid, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_mesh_refine_rows, dim3((nr + REFINE_T - 1) / REFINE_T), dim3(REFINE_T), 0, ctx->stream,
                       (const unsigned long long*)d_offsets, nr, status, mb.d_binvalid.get());
    AQ_HIP(hipGetLastError());
    if (m_in > 0) {
        const CoarsenIn in{(const unsigned long long*)d_offsets, d_x, d_f, d_level, nr, m_in};
        const unsigned long long slots = (m_in + 1) / 2;
        const double* thr = d_thr;
        if (!thr) {
            if ((rc = coarsen_thresholds(ctx, in, mb.d_cthr.get()))) return rc;
            thr = mb.d_cthr;
        } else if ((rc = coarsen_positions(ctx, in))) {   // the positions and the rows alone
            return rc;
        }
        const LeafSink sink{mb.d_leaf, mb.d_leafcnt, (unsigned long long)cap_leaves};
        hipLaunchKernelGGL(k_mesh_coarsen_emit, dim3((unsigned)((slots + COARSEN_T - 1) / COARSEN_T)), dim3(COARSEN_T), 0,
                           ctx->stream, in, slots, (const ulonglong2*)mb.d_cpos.get(), (const unsigned*)mb.d_crow.get(), thr,
                           d_eps, eps, sink, levels);
        AQ_HIP(hipGetLastError());
    }
    AQ_HIP(hipMemcpyAsync(mb.h_bwords, mb.d_leafcnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(mb.h_bwords + 1, mb.d_binvalid, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(mb.h_rtab + REFINE_TAB_LEVELS, levels, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t leaves = mb.h_bwords[0], with_nodes = n - mb.h_bwords[1];
    info->leaves = leaves;
    info->tasks = 2 * leaves - with_nodes;
    info->n_nodes = 2 * leaves + with_nodes;
    info->merged = (m_in - with_nodes) / 2 - leaves;
    info->levels = mb.h_rtab[REFINE_TAB_LEVELS];
    if (info->n_nodes > cap_nodes) return AQ_EOVERFLOW;
    return mesh_batch_back(ctx, n, out, (unsigned)leaves);
}

int aq_mesh_eval(aq_ctx* ctx, uint64_t n_nodes, const double* d_x, const double* d_f, const double* d_cum, size_t nq,
                 const double* d_q, double* d_out) {
    if (!ctx || n_nodes < 3) return AQ_EINVAL;
    if (nq > 0 && (!d_x || !d_f || !d_cum || !d_q || !d_out)) return AQ_EINVAL;
    if (nq == 0) return AQ_OK;
    const size_t grid = (nq + 255) / 256;
    if (grid > 0x7fffffffull) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_mesh_eval, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (unsigned long long)n_nodes, d_x,
                       d_f, d_cum, nq, d_q, d_out);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

// aq_mesh_invert's two instances of k_mesh_invert (aquad.hip) and the switch between them; the constants are the
// measured ones of DESIGN.md "Mesh inversion" (profiles/mesh_invert/).
constexpr int MINV_LOG_TAB = 11;               // the staged instance's table: 2048 entries of cum, 16 KiB of LDS
constexpr int MINV_WG_PER_CU = 8;              // its grid: workgroups per CU (every wave slot; 8 x 16 KiB of the CU's 160)
constexpr size_t MINV_QPT = 4;                 // ... and no more workgroups than give every thread this many queries
constexpr size_t MINV_STAGED_MIN_NQ = 1 << 21; // fewer queries than this: the plain search (the staging does not pay)

int aq_mesh_invert(aq_ctx* ctx, uint64_t n_nodes, const double* d_x, const double* d_f, const double* d_cum, size_t nq,
                   const double* d_y, double* d_out) {
    if (!ctx || n_nodes < 3) return AQ_EINVAL;
    if (nq > 0 && (!d_x || !d_f || !d_cum || !d_y || !d_out)) return AQ_EINVAL;
    if (nq == 0) return AQ_OK;
    if ((nq + 255) / 256 > 0x7fffffffull) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    // AQ_MESH_INVERT=0 / 1 in the environment, read per call, forces the plain / the staged instance
    const int force = env_int("AQ_MESH_INVERT", -1);
    const bool staged = force == 0 ? false : force == 1 ? true : nq >= MINV_STAGED_MIN_NQ;
    const uint64_t last = n_nodes - 2;   // m - 1, the last index the search may return
    auto kernel = k_mesh_invert<0>;
    unsigned grid = (unsigned)((nq + 255) / 256), sh = 0, entries = 0, top = 0;
    if (staged) {
        kernel = k_mesh_invert<MINV_LOG_TAB>;
        while ((last >> sh) + 1 > (1ull << MINV_LOG_TAB)) ++sh;
        entries = (unsigned)((last >> sh) + 1);
        // the first halving step: 2 * top is the least power of two >= entries (one entry: no step)
        if (entries > 1) for (top = 1; 2 * top < entries; top *= 2) {}
        const size_t want = (nq + 256 * MINV_QPT - 1) / (256 * MINV_QPT);
        grid = (unsigned)std::min<size_t>(want, (size_t)std::max(ctx->num_cus, 1) * MINV_WG_PER_CU);
    } else {
        while (sh < 64 && (last >> sh) != 0) ++sh;   // 2^sh > m - 1: the halving steps reach every index
    }
    EventPair ev;   // (aq_kernel_timing: tools/try_mesh_invert.py times the two instances with it)
    int rc = timing_begin(ctx, ev);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, ctx->stream, (unsigned long long)n_nodes, d_x, d_f, d_cum, nq,
                       d_y, d_out, sh, entries, top);
    AQ_HIP(hipGetLastError());
    return timing_end(ctx, ev);
}

// The batch forms: n rows x nq_per_row queries, one per lane, each on its row's slice of the batch mesh.
using MeshBatchQueryKernel = void (*)(const unsigned long long*, const double*, const double*, const double*, size_t,
                                      size_t, const double*, double*);
static int mesh_queries_batch(aq_ctx* ctx, MeshBatchQueryKernel kernel, size_t n, const uint64_t* d_offsets, const double* d_x,
                              const double* d_f, const double* d_cum, size_t nq, const double* d_q, double* d_out) {
    if (!ctx) return AQ_EINVAL;
    if (nq != 0 && n > (size_t)-1 / nq) return AQ_EINVAL;
    const size_t total = n * nq;
    if (total > 0 && (!d_offsets || !d_x || !d_f || !d_cum || !d_q || !d_out)) return AQ_EINVAL;
    if (total == 0) return AQ_OK;
    const size_t grid = (total + 255) / 256;
    if (grid > 0x7fffffffull) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const unsigned long long*)d_offsets, d_x,
                       d_f, d_cum, nq, total, d_q, d_out);
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

int aq_mesh_eval_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_x, const double* d_f,
                       const double* d_cum, size_t nq_per_row, const double* d_q, double* d_out) {
    return mesh_queries_batch(ctx, k_mesh_eval_batch, n, d_offsets, d_x, d_f, d_cum, nq_per_row, d_q, d_out);
}

int aq_mesh_invert_batch(aq_ctx* ctx, size_t n, const uint64_t* d_offsets, const double* d_x, const double* d_f,
                         const double* d_cum, size_t nq_per_row, const double* d_y, double* d_out) {
    return mesh_queries_batch(ctx, k_mesh_invert_batch, n, d_offsets, d_x, d_f, d_cum, nq_per_row, d_y, d_out);
}

int aq_kernel_timing(aq_ctx* ctx, int enable) {
    if (!ctx) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    for (auto& e : ctx->ev_pending) ctx->ev_free.push_back(std::move(e));
    ctx->ev_pending.clear();
    ctx->timing = enable != 0;
    ctx->timed_ms = 0.0;
    ctx->timed_launches = 0;
    return AQ_OK;
}

int aq_kernel_time(aq_ctx* ctx, double* total_ms, uint64_t* launches) {
    if (!ctx) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    for (auto& e : ctx->ev_pending) {
        float ms = 0.f;
        AQ_HIP(hipEventElapsedTime(&ms, e.first, e.second));
        ctx->timed_ms += ms;
        ctx->timed_launches += 1;
        ctx->ev_free.push_back(std::move(e));
    }
    ctx->ev_pending.clear();
    if (total_ms) *total_ms = ctx->timed_ms;
    if (launches) *launches = ctx->timed_launches;
    return AQ_OK;
}

void aq_print_reference_procs(FILE* f, double area, const uint64_t* tpp, int nprocs) {
    if (!f) f = stdout;
    fprintf(f, "Area=%lf\n", area);             // :108
    fprintf(f, "\nTasks Per Process\n");         // :109
    for (int i = 0; i < nprocs; ++i) fprintf(f, "%d\t", i);                               // :110-112
    fprintf(f, "\n");
    for (int i = 0; i < nprocs; ++i) fprintf(f, "%llu\t", (unsigned long long)(tpp ? tpp[i] : 0));  // :114-116
    fprintf(f, "\n");
}

void aq_print_reference(FILE* f, const aq_result* r) {
    if (!r) return;
    const int ng = (r->tasks_per_gpu && r->n_gpus >= 1) ? (int)r->n_gpus : 1;
    std::vector<uint64_t> tpp((size_t)ng + 1, 0);
    for (int g = 0; g < ng; ++g) tpp[1 + g] = r->tasks_per_gpu ? r->tasks_per_gpu[g] : r->tasks;
    aq_print_reference_procs(f, r->area, tpp.data(), ng + 1);
}

}  // extern "C"
