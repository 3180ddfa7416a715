// ================================================================================================
// Host side: the C ABI of include/aquad.h (included by aquad.hip after the kernels).
// ================================================================================================
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

int err_from_bits(unsigned bits) {
    if (bits & ERRB_TIMEOUT) return AQ_ETIMEOUT;
    if (bits & ERRB_OVERFLOW) return AQ_EOVERFLOW;
    if (bits & ERRB_DEPTH) return AQ_EDEPTH;
    return AQ_OK;
}

int floor_log2(unsigned long long v) {
    int d = 0;
    while ((2ull << d) <= v) ++d;
    return d;
}

bool integrand_ok(int f) { return f == AQ_F_COSH4 || f == AQ_F_SIN_RECIP || f == AQ_F_USER; }

// The supported domain. The kernels compare DOUBLED areas (aq_device.h task_step_k), which are the
// reference's own products (F(l)+F(r))*(r-l) before its '/2'; the sums l2 + r2 must stay finite
// where the reference's halves do, so every |F| * width stays far below 2^1023: bounds within
// 2^900, and for cosh^4 (F ~ e^{4|x|}/16, 16 F in the rounds) |x| <= 170. The persistent kernel's
// rings hold HALVED endpoints (pair_step_halves), exact while every coordinate of the tree is 0 or
// at least 2^-1021 in magnitude: nonzero bounds of at least 2^-900 keep the smallest coordinate a
// 64-level tree can make (one cancelling midpoint, 2^-53 below the bounds' scale, then 64 halvings)
// far above that.
bool bounds_ok(int f, double a, double b) {
    if (!(std::isfinite(a) && std::isfinite(b) && b >= a)) return false;
    const double m = std::max(std::fabs(a), std::fabs(b));
    if (m > 0x1p900) return false;
    if ((a != 0.0 && std::fabs(a) < 0x1p-900) || (b != 0.0 && std::fabs(b) < 0x1p-900)) return false;
    if (f == AQ_F_COSH4) return m <= 170.0;
    if (f == AQ_F_USER) return user::domain_ok(a, b);
    return true;
}

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

}  // namespace

struct aq_ctx {
    int device = 0;
    int num_cus = 0;
    int grid = 0;                      // persistent workgroups per launch (one per CU, or AQ_GRID)
    std::unique_ptr<HostPool> pool;    // the batch front end's host threads (created on first use)
    int occ[4][2][6] = {};             // k_stream<FID,HIST> by Variant: resident workgroups per CU (0: not asked yet)
    bool batch_heap = false;           // the batch front end's launches: the heap-seeding instance (HEAPS)
    bool coop = false;                 // AQ_COOP=1: cooperative launches
    bool histograms = true;
    double stall_ms = DEFAULT_STALL_MS;
    unsigned long long dev_bytes = 0;  // device memory held
    hipStream_t stream = nullptr;
    ExpPair* d_tab = nullptr;
    Ctl* d_ctl = nullptr;              // NSLOTS control blocks (totals, exact area, histograms)
    QCtl* d_q = nullptr;               // two queue / termination blocks, used by launches in turn
    int qsel = 0;                      // the block the next launch uses
    unsigned long long* d_parts = nullptr;   // (NPARTS + 1) x grid per-workgroup pack_cu words (per-CU launches
                                             // into slots < NPARTS, and the sync slot: parts_row)
    double* d_parea = nullptr;               // ... and their area words (PCU_AREA: a double-double per workgroup)
    bool sync_fold = false;                  // the next per-CU launch's reader folds its area words itself
                                             // (k_fetch_sync, k_pack_group): no k_fold_parts after it
    bool dirty[NSLOTS_ALL] = {};       // slot's sums / area used since they were last reset
    bool parts_dirty[NSLOTS_ALL] = {}; // slot's per-workgroup words written (per-CU launches)
    bool slot_hist[NSLOTS_ALL] = {};
    double2* d_bounds = nullptr;       // NSLOTS {a, b}
    int* d_shard = nullptr;            // NSLOTS per-integral shard (mixed launches)
    double2* h_bounds = nullptr;       // pinned staging ring, NSTAGE x NSLOTS (a launch's copy may still be
                                       // pending when the host queues the next launch)
    int* h_shard = nullptr;            // pinned staging ring, NSTAGE x NSLOTS
    hipEvent_t stage_ev[NSTAGE] = {};  // recorded after each staging copy
    int stage = 0;
    Chunk* d_chunks = nullptr;
    Cellar* d_cellar = nullptr;        // grid * NW per-wave HBM overflow stacks
    unsigned* d_ready = nullptr;
    unsigned epoch = 0;
    LaunchHint* d_hint = nullptr;      // job-size hint carried from launch to launch
    HintState hint;                    // the workload the hint was measured on (aq_launch_plan.h)
    int gsplit_env = 0;                // AQ_GSPLIT: waves per job of a multi-integral launch (0 = default)
    // level path
    DevResults* d_lres = nullptr;
    Rec* d_front[2] = {nullptr, nullptr};
    size_t front_cap = 0;              // records per buffer (0 unless both are allocated)
    size_t front_bytes[2] = {0, 0};
    unsigned* d_count = nullptr;
    unsigned* h_fcount = nullptr;      // pinned: aq_frontier_integrate's per-level counts
    double* d_facc = nullptr;          // aq_frontier_integrate's accumulator (8 doubles, device)
    double* h_facc = nullptr;          // pinned copy
    LevelPart* d_lparts = nullptr;     // frontier engine: per-block partials of one level step
    bool defer_fold = false;           // aq_level_defer_fold: level steps leave their rows for one later fold
    int lp_pending = 0;                // level-step rows written and not yet folded
    double* lp_acc = nullptr;          // ... into this accumulator
    // batch front end: rows {area, tasks, accepted, error} and bounds, and the two copy streams that run
    // beside the launches. The device keeps two chunks' bounds and two chunks' rows (rings indexed by
    // chunk parity: at most chunk c + 1's bounds and chunks c, c - 1's rows are in flight) and one chunk's
    // size-order buffers, bdev_rows integrals each (grow-only up to MAXK, whatever n: ADVICE r5 -- they
    // had been sized to the whole batch, 72 B per integral); the pinned host copies cover the whole call
    // (grow-only, bhost_cap integrals)
    double* d_batch = nullptr;         // [2][bdev_rows][4]
    double* h_batch = nullptr;         // [bhost_cap][4]
    double2* d_bbounds = nullptr;      // [2][bdev_rows]
    double2* h_bbounds = nullptr;      // [bhost_cap]
    double2* d_bsorted = nullptr;      // the chunk's bounds in size order (k_batch_scatter; 2 parities)
    unsigned* d_bkey = nullptr;        // size class per integral (k_batch_estimate)
    unsigned* d_bperm = nullptr;       // sorted position -> integral (2 parities)
    unsigned* d_bcnt = nullptr;        // EST_KEYS counts + EST_KEYS cursors
    double* d_best = nullptr;          // the chunk's sum of size estimates (per chunk parity)
    size_t bdev_rows = 0, bhost_cap = 0;
    // per-integral parameters (AQ_F_PARAM), allocated by the first parametrised call (ensure_params; the
    // batch rings by the first aq_integrate_batch_params): NSLOTS + 1 rows on the device beside d_bounds,
    // their pinned staging ring, and the batch front end's rows -- two chunks' theta and two chunks' theta
    // in size order, sized like d_bbounds / d_bsorted, and the pinned copy of the whole call
    double* d_theta = nullptr;         // [NSLOTS_ALL][nparams]
    double* h_theta = nullptr;         // pinned staging ring, NSTAGE x NSLOTS x nparams
    double* d_btheta = nullptr;        // [2][btheta_rows][nparams]
    double* d_bthsorted = nullptr;     // [2][btheta_rows][nparams] (k_batch_scatter_theta)
    double* h_btheta = nullptr;        // [btheta_hcap][nparams]
    size_t btheta_rows = 0, btheta_hcap = 0;
    // error estimate (the ERR launches, aq_*_err), allocated by the first ERR call (ensure_err; the batch
    // rings by the first aq_integrate_batch_err): the slots' two sums, and the batch front end's rows -- two
    // chunks' {err_abs, err_signed} on the device and the pinned copy of the whole call
    double* d_err = nullptr;           // [NSLOTS_ALL][2] = Σ|d|, Σd over the slot's accepted tasks
    double* h_err = nullptr;           // pinned, one pair (aq_fetch_err)
    bool err_dirty[NSLOTS_ALL] = {};   // slot's pair written since it was last zeroed
    bool slot_err[NSLOTS_ALL] = {};    // slot's last launch was an ERR launch (beside slot_hist)
    int occ_err[4][6] = {};            // the ERR instances' resident workgroups per CU, by Variant (as occ)
    double* d_berr = nullptr;          // [2][berr_rows][2]
    double* h_berr = nullptr;          // [berr_hcap][2]
    size_t berr_rows = 0, berr_hcap = 0;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr, s_pre = nullptr;
    // eval buffers
    double* d_x = nullptr;
    double* d_y = nullptr;
    size_t eval_cap = 0;
    // host staging
    unsigned long long* h_parts = nullptr;  // pinned, grid words
    SlotSums* h_sums = nullptr;        // pinned, one
    XSum* h_area = nullptr;            // pinned, one
    unsigned long long* h_hist = nullptr;  // pinned, 2 * AQ_MAX_LEVELS
    DevResults* h_lres = nullptr;      // pinned
    SyncOut* h_sync = nullptr;         // pinned, coherent: k_fetch_sync's target (the synchronous path)
    SyncOut* d_sync = nullptr;         // its device address
    unsigned long long sync_seq = 0;   // the last synchronous call's sequence number (SyncOut::seq)
    HostOut last;
    bool last_valid = false;
    // diagnostics
    unsigned long long* d_diag = nullptr;
    unsigned long long* d_cu_acc = nullptr;   // [AQ_CU_SLOTS] tasks per CU slot since the last reset (every launch)
    // timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_free;
    double timed_ms = 0.0;
    unsigned long long timed_launches = 0;
};

namespace {

template <typename T>
int dmalloc(aq_ctx* c, T** p, size_t bytes, bool zero) {
    AQ_HIP(hipMalloc(reinterpret_cast<void**>(p), bytes));
    c->dev_bytes += bytes;
    if (zero) AQ_HIP(hipMemset(*p, 0, bytes));
    return AQ_OK;
}

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
using EventPair = std::pair<hipEvent_t, hipEvent_t>;
int timing_begin(aq_ctx* ctx, EventPair& ev) {
    if (!ctx->timing) return AQ_OK;
    if (!ctx->ev_free.empty()) {
        ev = ctx->ev_free.back();
        ctx->ev_free.pop_back();
    } else {
        AQ_HIP(hipEventCreate(&ev.first));
        AQ_HIP(hipEventCreate(&ev.second));
    }
    AQ_HIP(hipEventRecord(ev.first, ctx->stream));
    return AQ_OK;
}
int timing_end(aq_ctx* ctx, const EventPair& ev) {
    if (!ctx->timing) return AQ_OK;
    AQ_HIP(hipEventRecord(ev.second, ctx->stream));
    ctx->ev_pending.push_back(ev);
    return AQ_OK;
}

// One persistent launch of k integrals (slots first_slot ..). shard_of: per-integral shard of
// nshards (nullptr: every integral is shard `shard`). dev_bounds: the k {a, b} already on the device
// (the batch front end copies them ahead on its own stream), else they are staged and copied here.
// The launch's shape -- instance, waves, shares, seed depth, tail, job mode -- is plan_launch's
// (aq_launch_plan.h); this enqueues it.
template <int FID, bool HIST>
int launch_stream(aq_ctx* ctx, int k, const double* a, const double* b, const int32_t* shard_of, double eps,
                  int max_depth, int shard, int nshards, int first_slot, const double2* dev_bounds = nullptr,
                  const double* theta = nullptr, const double* dev_theta = nullptr, bool err = false) {
    static_assert(FID >= 0 && FID < 4, "aq_ctx::occ holds one row per integrand");
    // err: an ERR launch (its instances keep no histograms: the callers pass HIST = false); ctx->d_err exists
    if (err && (HIST || !ctx->d_err)) return AQ_EINVAL;
    // F_PARAM: the k parameter rows, on the host (staged and copied here, per-CU launches too: theta is
    // not a kernel argument) or already on the device in the launch's order (the batch front end)
    constexpr int NP = param::nparams;
    const bool stage_theta = FID == F_PARAM && !dev_theta;
    if (FID == F_PARAM && !theta && !dev_theta) return AQ_EINVAL;
    const int G = ctx->grid;
    const LaunchRequest rq{FID, G, k, shard_of != nullptr, nshards, first_slot, ctx->d_diag != nullptr,
                           ctx->batch_heap, ctx->gsplit_env, eps, err};
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
    EventPair ev{nullptr, nullptr};
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
    if (pcu && !ctx->sync_fold) {
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

int launch_any(aq_ctx* ctx, int integrand, int k, const double* a, const double* b, const int32_t* shard_of,
               double eps, int max_depth, int shard, int nshards, int first_slot, const double2* dev_bounds = nullptr,
               bool err = false) {
    return with_fid(integrand, [&](auto F) {
        constexpr int FID = decltype(F)::value;
        if (err)
            return launch_stream<FID, false>(ctx, k, a, b, shard_of, eps, max_depth, shard, nshards, first_slot, dev_bounds,
                                             nullptr, nullptr, true);
        return ctx->histograms
            ? launch_stream<FID, true>(ctx, k, a, b, shard_of, eps, max_depth, shard, nshards, first_slot, dev_bounds)
            : launch_stream<FID, false>(ctx, k, a, b, shard_of, eps, max_depth, shard, nshards, first_slot, dev_bounds);
    });
}

// The parametrised family's buffers, on the first parametrised call (a fresh context holds none of them:
// aq_ctx_device_bytes does not move until then).
int ensure_params(aq_ctx* ctx) {
    if (ctx->d_theta) return AQ_OK;
    constexpr size_t NP = (size_t)param::nparams;
    if (!ctx->h_theta) AQ_HIP(hipHostMalloc(&ctx->h_theta, sizeof(double) * NP * NSLOTS * NSTAGE, hipHostMallocDefault));
    return dmalloc(ctx, &ctx->d_theta, sizeof(double) * NP * NSLOTS_ALL, false);
}

// The error estimate's slot sums, on the first ERR call (a fresh context and the plain calls hold none of
// them: aq_ctx_device_bytes does not move until then). Zeroed once; ensure_clean and the readers keep the
// slots zero between launches.
int ensure_err(aq_ctx* ctx) {
    if (ctx->d_err) return AQ_OK;
    if (!ctx->h_err) AQ_HIP(hipHostMalloc(&ctx->h_err, 2 * sizeof(double), hipHostMallocDefault));
    return dmalloc(ctx, &ctx->d_err, 2 * sizeof(double) * NSLOTS_ALL, true);
}

// launch_any for AQ_F_PARAM (with_fid stays the three fixed integrands': no level or frontier kernel
// is instantiated for id 3)
int launch_params(aq_ctx* ctx, int k, const double* a, const double* b, const double* theta, double eps, int max_depth,
                  int shard, int nshards, int first_slot, const double2* dev_bounds = nullptr,
                  const double* dev_theta = nullptr, bool err = false) {
    const int rc = ensure_params(ctx);
    if (rc) return rc;
    if (err)
        return launch_stream<F_PARAM, false>(ctx, k, a, b, nullptr, eps, max_depth, shard, nshards, first_slot, dev_bounds,
                                             theta, dev_theta, true);
    return ctx->histograms
        ? launch_stream<F_PARAM, true>(ctx, k, a, b, nullptr, eps, max_depth, shard, nshards, first_slot, dev_bounds,
                                       theta, dev_theta)
        : launch_stream<F_PARAM, false>(ctx, k, a, b, nullptr, eps, max_depth, shard, nshards, first_slot, dev_bounds,
                                        theta, dev_theta);
}

// One integral of the parametrised family: the engine's bounds rule, finite parameters, the plug-in's domain.
bool params_ok(double a, double b, const double* th) {
    if (!bounds_ok(AQ_F_PARAM, a, b)) return false;
    for (int j = 0; j < param::nparams; ++j)
        if (!std::isfinite(th[j])) return false;
    return param::domain_ok(a, b, th);
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

int fetch_slot(aq_ctx* ctx, int slot, aq_result* out) {
    if (ctx->parts_dirty[slot])
        AQ_HIP(hipMemcpyAsync(ctx->h_parts, ctx->d_parts + 2 * parts_row(slot) * ctx->grid,
                              2 * sizeof(unsigned long long) * (size_t)ctx->grid, hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(ctx->h_sums, &ctx->d_ctl[slot].sums, sizeof(SlotSums), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(ctx->h_area, &ctx->d_ctl[slot].area, sizeof(XSum), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->slot_hist[slot])
        AQ_HIP(hipMemcpyAsync(ctx->h_hist, ctx->d_ctl[slot].hist, sizeof(unsigned long long) * 2 * AQ_MAX_LEVELS,
                              hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    return finish_fetch(ctx, *ctx->h_sums, *ctx->h_area, ctx->parts_dirty[slot] ? ctx->h_parts : nullptr,
                        ctx->slot_hist[slot] ? ctx->h_hist : nullptr, out);
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
        __builtin_ia32_pause();
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

bool slot_range_ok(int first, int n) { return first >= 0 && n >= 0 && n <= NSLOTS && first < NSLOTS; }

}  // namespace

// The RCCL group (aq_integrate_group).
struct aq_group {
    int nranks = 0;
    int grid = 0;
    bool own_ctx_order = false;
    std::vector<aq_ctx*> ctx;             // members driven by this process
    std::vector<int> rank;                // their ranks
    std::vector<ncclComm_t> comm;
    std::vector<long long*> d_sum;        // per member: GROUP_SUM int64 (all-reduced in place)
    std::vector<unsigned long long*> d_mine;   // per member: 3 + grid words (this rank's contribution)
    std::vector<unsigned long long*> d_all;    // per member: nranks * (3 + grid) words (all-gathered)
    long long* h_sum = nullptr;           // pinned copies of member 0's results
    unsigned long long* h_all = nullptr;
};

namespace {

int group_alloc(aq_group* g) {
    const size_t info = 3 + (size_t)g->grid;
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        AQ_HIP(hipSetDevice(g->ctx[m]->device));
        long long* s = nullptr;
        unsigned long long *mine = nullptr, *all = nullptr;
        AQ_HIP(hipMalloc(&s, sizeof(long long) * GROUP_SUM));
        AQ_HIP(hipMalloc(&mine, sizeof(unsigned long long) * info));
        AQ_HIP(hipMalloc(&all, sizeof(unsigned long long) * info * g->nranks));
        g->d_sum.push_back(s);
        g->d_mine.push_back(mine);
        g->d_all.push_back(all);
    }
    AQ_HIP(hipHostMalloc(&g->h_sum, sizeof(long long) * GROUP_SUM, hipHostMallocDefault));
    AQ_HIP(hipHostMalloc(&g->h_all, sizeof(unsigned long long) * info * g->nranks, hipHostMallocDefault));
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
    AQ_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    int rc;
    if ((rc = dmalloc(c, &c->d_tab, sizeof(ExpPair) * 128, false))) return rc;
    AQ_HIP(hipMemcpy(c->d_tab, aq_exp_tab_host, sizeof(ExpPair) * 128, hipMemcpyHostToDevice));
    if ((rc = dmalloc(c, &c->d_ctl, sizeof(Ctl) * NSLOTS_ALL, true))) return rc;
    if ((rc = dmalloc(c, &c->d_parts, 2 * sizeof(unsigned long long) * (size_t)(NPARTS + 1) * c->grid, true))) return rc;
    if ((rc = dmalloc(c, &c->d_parea, 2 * sizeof(double) * (size_t)(NPARTS + 1) * c->grid, true))) return rc;
    if ((rc = dmalloc(c, &c->d_bounds, sizeof(double2) * NSLOTS_ALL, false))) return rc;
    if ((rc = dmalloc(c, &c->d_shard, sizeof(int) * NSLOTS_ALL, false))) return rc;
    if ((rc = dmalloc(c, &c->d_hint, sizeof(LaunchHint), true))) return rc;
    if ((rc = dmalloc(c, &c->d_q, 2 * sizeof(QCtl), true))) return rc;
    if ((rc = dmalloc(c, &c->d_cu_acc, sizeof(unsigned long long) * AQ_CU_SLOTS, true))) return rc;
    AQ_HIP(hipHostMalloc(&c->h_bounds, sizeof(double2) * NSLOTS * NSTAGE, hipHostMallocDefault));
    AQ_HIP(hipHostMalloc(&c->h_shard, sizeof(int) * NSLOTS * NSTAGE, hipHostMallocDefault));
    for (int i = 0; i < NSTAGE; ++i) {
        AQ_HIP(hipEventCreateWithFlags(&c->stage_ev[i], hipEventDisableTiming));
        AQ_HIP(hipEventRecord(c->stage_ev[i], c->stream));
    }
    if ((rc = dmalloc(c, &c->d_chunks, sizeof(Chunk) * (size_t)QCAP, false))) return rc;
    if ((rc = dmalloc(c, &c->d_cellar, sizeof(Cellar) * (size_t)c->grid * NW, false))) return rc;
    if ((rc = dmalloc(c, &c->d_ready, sizeof(unsigned) * (size_t)QCAP * READY_STRIDE, true))) return rc;
    AQ_HIP(hipHostMalloc(&c->h_parts, 2 * sizeof(unsigned long long) * (size_t)c->grid, hipHostMallocDefault));
    AQ_HIP(hipHostMalloc(&c->h_sums, sizeof(SlotSums), hipHostMallocDefault));
    AQ_HIP(hipHostMalloc(&c->h_area, sizeof(XSum), hipHostMallocDefault));
    AQ_HIP(hipHostMalloc(&c->h_hist, sizeof(unsigned long long) * 2 * AQ_MAX_LEVELS, hipHostMallocDefault));
    AQ_HIP(hipHostMalloc(&c->h_lres, sizeof(DevResults), hipHostMallocDefault));
    AQ_HIP(hipHostMalloc(&c->h_sync, sizeof(SyncOut), hipHostMallocCoherent | hipHostMallocMapped));
    AQ_HIP(hipHostGetDevicePointer((void**)&c->d_sync, c->h_sync, 0));
    memset(c->h_sync, 0, sizeof(SyncOut));
    if ((rc = dmalloc(c, &c->d_lres, sizeof(DevResults), false))) return rc;
    if ((rc = dmalloc(c, &c->d_count, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), false))) return rc;
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
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& e : c->ev_pending) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : c->ev_free) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    (void)hipFree(c->d_tab);
    (void)hipFree(c->d_ctl);
    (void)hipFree(c->d_parts);
    (void)hipFree(c->d_parea);
    (void)hipFree(c->d_bounds);
    (void)hipFree(c->d_shard);
    (void)hipFree(c->d_hint);
    (void)hipFree(c->d_q);
    (void)hipFree(c->d_chunks);
    (void)hipFree(c->d_cellar);
    (void)hipFree(c->d_ready);
    (void)hipFree(c->d_lres);
    (void)hipFree(c->d_diag);
    (void)hipFree(c->d_cu_acc);
    (void)hipFree(c->d_front[0]);
    (void)hipFree(c->d_front[1]);
    (void)hipFree(c->d_count);
    (void)hipFree(c->d_facc);
    if (c->h_fcount) (void)hipHostFree(c->h_fcount);
    if (c->h_facc) (void)hipHostFree(c->h_facc);
    (void)hipFree(c->d_x);
    (void)hipFree(c->d_batch);
    (void)hipFree(c->d_lparts);
    (void)hipFree(c->d_y);
    if (c->h_batch) (void)hipHostFree(c->h_batch);
    (void)hipFree(c->d_bbounds);
    if (c->h_bbounds) (void)hipHostFree(c->h_bbounds);
    (void)hipFree(c->d_bsorted);
    (void)hipFree(c->d_bkey);
    (void)hipFree(c->d_bperm);
    (void)hipFree(c->d_bcnt);
    (void)hipFree(c->d_best);
    (void)hipFree(c->d_theta);
    (void)hipFree(c->d_err);
    (void)hipFree(c->d_berr);
    if (c->h_err) (void)hipHostFree(c->h_err);
    if (c->h_berr) (void)hipHostFree(c->h_berr);
    (void)hipFree(c->d_btheta);
    (void)hipFree(c->d_bthsorted);
    if (c->h_theta) (void)hipHostFree(c->h_theta);
    if (c->h_btheta) (void)hipHostFree(c->h_btheta);
    if (c->s_h2d) { (void)hipStreamSynchronize(c->s_h2d); (void)hipStreamDestroy(c->s_h2d); }
    if (c->s_pre) { (void)hipStreamSynchronize(c->s_pre); (void)hipStreamDestroy(c->s_pre); }
    if (c->s_d2h) { (void)hipStreamSynchronize(c->s_d2h); (void)hipStreamDestroy(c->s_d2h); }
    if (c->h_bounds) (void)hipHostFree(c->h_bounds);
    if (c->h_shard) (void)hipHostFree(c->h_shard);
    for (int i = 0; i < NSTAGE; ++i)
        if (c->stage_ev[i]) (void)hipEventDestroy(c->stage_ev[i]);
    if (c->h_parts) (void)hipHostFree(c->h_parts);
    if (c->h_sums) (void)hipHostFree(c->h_sums);
    if (c->h_area) (void)hipHostFree(c->h_area);
    if (c->h_hist) (void)hipHostFree(c->h_hist);
    if (c->h_lres) (void)hipHostFree(c->h_lres);
    if (c->h_sync) (void)hipHostFree(c->h_sync);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
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
    if (enable && !c->d_diag) {
        AQ_HIP(hipMalloc(&c->d_diag, sizeof(unsigned long long) * DIAG_WORDS * MAXG));
        AQ_HIP(hipMemset(c->d_diag, 0, sizeof(unsigned long long) * DIAG_WORDS * MAXG));
    } else if (!enable && c->d_diag) {
        (void)hipFree(c->d_diag);
        c->d_diag = nullptr;
    }
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

static int many_common(aq_ctx* ctx, int integrand, int k, const double* a, const double* b, const int32_t* shard_of,
                       double eps, int max_depth, int shard, int nshards, int first_slot, int slot_limit = NSLOTS) {
    if (!ctx || k < 1 || k > MAXK || !a || !b) return AQ_EINVAL;
    if (!integrand_ok(integrand)) return AQ_EINVAL;
    if (!(eps >= 0.0) || max_depth < 0 || max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    if (nshards < 1 || nshards > 64) return AQ_EINVAL;
    if (!shard_of && (shard < 0 || shard >= nshards)) return AQ_EINVAL;
    if (first_slot < 0 || first_slot + k > slot_limit) return AQ_EINVAL;
    for (int i = 0; i < k; ++i) {
        if (!bounds_ok(integrand, a[i], b[i])) return AQ_EINVAL;
        if (shard_of && (shard_of[i] < 0 || shard_of[i] >= nshards)) return AQ_EINVAL;
    }
    AQ_HIP(hipSetDevice(ctx->device));
    return launch_any(ctx, integrand, k, a, b, shard_of, eps, max_depth, shard, nshards, first_slot);
}

int aq_integrate_many_async(aq_ctx* ctx, int integrand, int k, const double* a, const double* b, double eps,
                            int max_depth, int shard, int nshards, int first_slot) {
    return many_common(ctx, integrand, k, a, b, nullptr, eps, max_depth, shard, nshards, first_slot);
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
    return many_common(ctx, integrand, k, a, b, shard, eps, max_depth, 0, nshards, first_slot);
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

static int fetch_exact_slot(aq_ctx* ctx, int slot, int64_t* row) {
    if (ctx->parts_dirty[slot])
        AQ_HIP(hipMemcpyAsync(ctx->h_parts, ctx->d_parts + 2 * parts_row(slot) * ctx->grid,
                              2 * sizeof(unsigned long long) * (size_t)ctx->grid, hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(ctx->h_sums, &ctx->d_ctl[slot].sums, sizeof(SlotSums), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(ctx->h_area, &ctx->d_ctl[slot].area, sizeof(XSum), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < XS_LIMBS; ++i) row[i] = ctx->h_area->limb[i];
    SlotSums s = *ctx->h_sums;
    if (!ctx->parts_dirty[slot]) s.pcu = 0;
    const Counts k = slot_counts(s, ctx->h_parts, ctx->grid);
    row[XS_LIMBS] = (int64_t)k.tasks;
    row[XS_LIMBS + 1] = (int64_t)k.leaves;
    row[XS_LIMBS + 2] = (int64_t)s.spilled;
    row[XS_LIMBS + 3] = (int64_t)k.levels | ((int64_t)s.error << 32);
    return err_from_bits(s.error);
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

int aq_integrate_shard(aq_ctx* ctx, const aq_problem* p, int shard, int nshards, aq_result* res) {
    if (!ctx) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    ctx->sync_fold = true;   // fetch_sync's k_fetch_sync folds the per-CU area words itself
    rc = many_common(ctx, p->integrand, 1, &p->a, &p->b, nullptr, p->eps, p->max_depth, shard, nshards, SYNC_SLOT,
                     NSLOTS_ALL);
    ctx->sync_fold = false;
    if (rc) return rc;
    return fetch_sync(ctx, res);
}

int aq_integrate_shard_exact(aq_ctx* ctx, const aq_problem* p, int shard, int nshards, int64_t* row) {
    if (!ctx || !row) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    rc = many_common(ctx, p->integrand, 1, &p->a, &p->b, nullptr, p->eps, p->max_depth, shard, nshards, SYNC_SLOT,
                     NSLOTS_ALL);
    if (rc) return rc;
    // the slot stays marked used: the next launch into it resets it first (ensure_clean)
    return fetch_exact_slot(ctx, SYNC_SLOT, row);
}

int aq_integrate(aq_ctx* ctx, const aq_problem* p, aq_result* res) {
    if (p && p->n_gpus > 1) return AQ_EINVAL;   // several GPUs: aq_integrate_group
    return aq_integrate_shard(ctx, p, 0, 1, res);
}

// ---- per-integral parameters (AQ_F_PARAM) -----------------------------------------------------------
static int many_params_common(aq_ctx* ctx, int k, const double* a, const double* b, const double* theta, double eps,
                              int max_depth, int shard, int nshards, int first_slot, int slot_limit = NSLOTS) {
    if (!ctx || k < 1 || k > MAXK || !a || !b || !theta) return AQ_EINVAL;
    if (!(eps >= 0.0) || max_depth < 0 || max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    if (nshards < 1 || nshards > 64 || shard < 0 || shard >= nshards) return AQ_EINVAL;
    if (first_slot < 0 || first_slot + k > slot_limit) return AQ_EINVAL;
    for (int i = 0; i < k; ++i)
        if (!params_ok(a[i], b[i], theta + (size_t)i * param::nparams)) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    return launch_params(ctx, k, a, b, theta, eps, max_depth, shard, nshards, first_slot);
}

int aq_integrate_many_params_async(aq_ctx* ctx, int k, const double* a, const double* b, const double* theta,
                                   double eps, int max_depth, int shard, int nshards, int first_slot) {
    return many_params_common(ctx, k, a, b, theta, eps, max_depth, shard, nshards, first_slot);
}

int aq_integrate_params(aq_ctx* ctx, const aq_problem* p, const double* theta, aq_result* res) {
    if (!ctx || !p || !theta) return AQ_EINVAL;
    if (p->integrand != AQ_F_PARAM || p->n_gpus > 1 || p->n_gpus < 0) return AQ_EINVAL;
    ctx->sync_fold = true;   // fetch_sync's k_fetch_sync folds the per-CU area words itself
    const int rc = many_params_common(ctx, 1, &p->a, &p->b, theta, p->eps, p->max_depth, 0, 1, SYNC_SLOT, NSLOTS_ALL);
    ctx->sync_fold = false;
    if (rc) return rc;
    return fetch_sync(ctx, res);
}

// ---- error estimate (the ERR launches) -----------------------------------------------------------------
double aq_err_extrapolate(double area, const aq_err* e) { return e ? area + e->err_signed / 3.0 : area; }

// theta goes with AQ_F_PARAM and with nothing else
static bool err_theta_ok(int integrand, const double* theta) {
    return integrand == AQ_F_PARAM ? theta != nullptr : (integrand_ok(integrand) && theta == nullptr);
}

static int many_err_common(aq_ctx* ctx, int integrand, int k, const double* a, const double* b, const double* theta,
                           double eps, int max_depth, int shard, int nshards, int first_slot, int slot_limit = NSLOTS) {
    if (!ctx || k < 1 || k > MAXK || !a || !b) return AQ_EINVAL;
    if (!err_theta_ok(integrand, theta)) return AQ_EINVAL;
    if (!(eps >= 0.0) || max_depth < 0 || max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    if (nshards < 1 || nshards > 64 || shard < 0 || shard >= nshards) return AQ_EINVAL;
    if (first_slot < 0 || first_slot + k > slot_limit) return AQ_EINVAL;
    for (int i = 0; i < k; ++i)
        if (theta ? !params_ok(a[i], b[i], theta + (size_t)i * param::nparams) : !bounds_ok(integrand, a[i], b[i]))
            return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    const int rc = ensure_err(ctx);
    if (rc) return rc;
    return theta ? launch_params(ctx, k, a, b, theta, eps, max_depth, shard, nshards, first_slot, nullptr, nullptr, true)
                 : launch_any(ctx, integrand, k, a, b, nullptr, eps, max_depth, shard, nshards, first_slot, nullptr, true);
}

int aq_integrate_many_err_async(aq_ctx* ctx, int integrand, int k, const double* a, const double* b, const double* theta,
                                double eps, int max_depth, int shard, int nshards, int first_slot) {
    return many_err_common(ctx, integrand, k, a, b, theta, eps, max_depth, shard, nshards, first_slot);
}

int aq_integrate_err(aq_ctx* ctx, const aq_problem* p, const double* theta, aq_result* res, aq_err* err) {
    if (!ctx || !p || !res || !err) return AQ_EINVAL;
    if (!err_theta_ok(p->integrand, theta) || p->n_gpus > 1) return AQ_EINVAL;
    if (!theta) {
        const int rc = validate(p);
        if (rc) return rc;
    } else if (p->n_gpus < 0) {
        return AQ_EINVAL;
    }
    ctx->sync_fold = true;   // fetch_sync's k_fetch_sync folds the per-CU area words itself
    const int rc = many_err_common(ctx, p->integrand, 1, &p->a, &p->b, theta, p->eps, p->max_depth, 0, 1, SYNC_SLOT,
                                   NSLOTS_ALL);
    ctx->sync_fold = false;
    if (rc) return rc;
    return fetch_sync(ctx, res, err);
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
    aq_group* g = new aq_group();
    g->nranks = n;
    g->grid = ctxs[0]->grid;
    g->comm.resize(n);
    for (int i = 0; i < n; ++i) {
        g->ctx.push_back(ctxs[i]);
        g->rank.push_back(i);
    }
    ncclResult_t r = ncclCommInitAll(g->comm.data(), n, devs.data());
    if (r != ncclSuccess) {
        fprintf(stderr, "aquad: ncclCommInitAll: %s\n", ncclGetErrorString(r));
        g->comm.clear();
        aq_group_destroy(g);
        return AQ_ERCCL;
    }
    const int rc = group_alloc(g);
    if (rc) {
        aq_group_destroy(g);
        return rc;
    }
    *out = g;
    return AQ_OK;
}

int aq_group_join(aq_ctx* ctx, int nranks, int rank, const void* id, aq_group** out) {
    if (!ctx || !id || !out || nranks < 1 || rank < 0 || rank >= nranks) return AQ_EINVAL;
    *out = nullptr;
    AQ_HIP(hipSetDevice(ctx->device));
    aq_group* g = new aq_group();
    g->nranks = nranks;
    g->grid = ctx->grid;
    g->ctx.push_back(ctx);
    g->rank.push_back(rank);
    g->comm.resize(1);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclResult_t r = ncclCommInitRank(&g->comm[0], nranks, u, rank);
    if (r != ncclSuccess) {
        fprintf(stderr, "aquad: ncclCommInitRank: %s\n", ncclGetErrorString(r));
        g->comm.clear();
        aq_group_destroy(g);
        return AQ_ERCCL;
    }
    const int rc = group_alloc(g);
    if (rc) {
        aq_group_destroy(g);
        return rc;
    }
    *out = g;
    return AQ_OK;
}

void aq_group_destroy(aq_group* g) {
    if (!g) return;
    for (size_t m = 0; m < g->ctx.size(); ++m) {
        (void)hipSetDevice(g->ctx[m]->device);
        (void)hipStreamSynchronize(g->ctx[m]->stream);
        if (m < g->comm.size() && g->comm[m]) (void)ncclCommDestroy(g->comm[m]);
        if (m < g->d_sum.size()) (void)hipFree(g->d_sum[m]);
        if (m < g->d_mine.size()) (void)hipFree(g->d_mine[m]);
        if (m < g->d_all.size()) (void)hipFree(g->d_all[m]);
    }
    if (g->h_sum) (void)hipHostFree(g->h_sum);
    if (g->h_all) (void)hipHostFree(g->h_all);
    delete g;
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
        c->sync_fold = true;   // k_pack_group folds the per-CU area words itself
        rc = launch_any(c, p->integrand, 1, &p->a, &p->b, nullptr, p->eps, p->max_depth, g->rank[m], N, SYNC_SLOT);
        c->sync_fold = false;
        if (rc) return rc;
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

// The context's two frontier buffers hold at least cap records each. They only grow; a failed
// allocation leaves neither (front_cap 0), so no caller ever launches on half a pair.
static void free_front(aq_ctx* ctx) {
    for (int i = 0; i < 2; ++i) {
        if (ctx->d_front[i]) {
            (void)hipFree(ctx->d_front[i]);
            ctx->dev_bytes -= ctx->front_bytes[i];
        }
        ctx->d_front[i] = nullptr;
        ctx->front_bytes[i] = 0;
    }
    ctx->front_cap = 0;
}

static int ensure_front(aq_ctx* ctx, size_t cap) {
    if (ctx->d_front[0] && ctx->d_front[1] && ctx->front_cap >= cap) return AQ_OK;
    free_front(ctx);
    for (int i = 0; i < 2; ++i) {
        const int rc = dmalloc(ctx, &ctx->d_front[i], cap * sizeof(Rec), false);
        if (rc) {
            ctx->d_front[i] = nullptr;
            free_front(ctx);
            return rc;
        }
        ctx->front_bytes[i] = cap * sizeof(Rec);
    }
    ctx->front_cap = cap;
    return AQ_OK;
}

int aq_integrate_levels(aq_ctx* ctx, const aq_problem* p, aq_result* res, uint64_t* tpl, uint64_t* lpl,
                        int maxlev) {
    if (!ctx) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    AQ_HIP(hipSetDevice(ctx->device));
    const int max_depth = p->max_depth ? p->max_depth : AQ_DEFAULT_MAX_DEPTH;
    // 16 M records (512 MiB) per buffer at least, whatever a frontier run left there before
    if ((rc = ensure_front(ctx, (size_t)1 << 24))) return rc;
    DevResults* dres = ctx->d_lres;
    AQ_HIP(hipMemsetAsync(dres, 0, sizeof(DevResults), ctx->stream));
    AQ_HIP(hipMemsetAsync(ctx->d_count, 0, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), ctx->stream));
    with_fid(p->integrand, [&](auto F) {
        hipLaunchKernelGGL((k_root<decltype(F)::value>), dim3(1), dim3(64), 0, ctx->stream, p->a, p->b, ctx->d_front[0],
                           ctx->d_tab);
    });
    AQ_HIP(hipGetLastError());
    unsigned n = 1;
    int depth = 0;
    for (; n > 0 && depth < AQ_MAX_LEVELS; ++depth) {
        Rec* in = ctx->d_front[depth & 1];
        Rec* outb = ctx->d_front[(depth + 1) & 1];
        unsigned* n_out = ctx->d_count + depth + 1;
        const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
        with_fid(p->integrand, [&](auto F) {
            hipLaunchKernelGGL((k_level<decltype(F)::value>), dim3(grid), dim3(256), 0, ctx->stream, in, n, outb, n_out,
                               (unsigned)ctx->front_cap, p->eps, depth, max_depth, dres, ctx->d_tab);
        });
        AQ_HIP(hipGetLastError());
        AQ_HIP(hipMemcpyAsync(ctx->h_lres, n_out, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        AQ_HIP(hipStreamSynchronize(ctx->stream));
        unsigned next = 0;
        memcpy(&next, ctx->h_lres, sizeof(unsigned));
        if (next > ctx->front_cap) next = (unsigned)ctx->front_cap;  // overflow flagged in res->error
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
    if (ctx->eval_cap >= n) return AQ_OK;
    (void)hipFree(ctx->d_x);
    (void)hipFree(ctx->d_y);
    ctx->d_x = ctx->d_y = nullptr;
    AQ_HIP(hipMalloc(&ctx->d_x, n * sizeof(double)));
    AQ_HIP(hipMalloc(&ctx->d_y, n * sizeof(double)));
    ctx->eval_cap = n;
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

// Chunk sizes of an n-integral batch: a first chunk of `first`, each next one twice the last up to
// MAXK (a chunk's launch then covers the host's checks and staging of the next, ~1.8 ns per integral
// against ~5 ns of kernel), the remainder last -- split so the last chunk is `last` when the remainder
// is large. AQ_BATCH_FIRST / AQ_BATCH_LAST in the environment override the defaults (0: no small
// first / last chunk).
static std::vector<int> batch_chunks(size_t n) {
    const size_t first = (size_t)std::max(0, env_int("AQ_BATCH_FIRST", AQ_BATCH_FIRST));
    const size_t last = (size_t)std::max(0, env_int("AQ_BATCH_LAST", AQ_BATCH_LAST));
    std::vector<int> c;
    size_t done = 0, next = first ? std::min(first, (size_t)MAXK) : (size_t)MAXK;
    while (n - done > next) {
        c.push_back((int)next);
        done += next;
        next = std::min(2 * next, (size_t)MAXK);
    }
    const size_t rem = n - done;
    if (last && rem > 2 * last) {
        c.push_back((int)(rem - last));
        c.push_back((int)last);
    } else if (rem) {
        c.push_back((int)rem);
    }
    return c;
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

// theta: the parametrised family's rows [n][nparams] (integrand AQ_F_PARAM, aq_integrate_batch_params), else
// null. The rows travel with the bounds: checked and staged with them, copied by the same stream into
// their own device ring, carried into size order behind k_batch_scatter (k_batch_scatter_theta).
// err: the ERR form (aq_integrate_batch_err) -- every chunk is an ERR launch, and its slots' error sums follow
// the rows: gathered behind them in the same order (k_gather_err), copied back by the same stream, unpacked
// with them into err_abs / err_signed (either may be null).
static int batch_run(aq_ctx* ctx, size_t n, const double* a, const double* b, const double* theta, double eps,
                     int integrand, double* area, uint64_t* accepted, uint64_t* tasks, bool err = false,
                     double* err_abs = nullptr, double* err_signed = nullptr) {
    // Batch front end (SURVEY config 3): up to MAXK integrals per persistent launch, every integral
    // with its own slot. Three streams (r05; profiles/r05a/c3_timeline_r04code.json had the launches
    // wait ~0.5 ms per chunk for a reset, a bounds copy, a full-width gather and a rows copy):
    //   * s_h2d copies chunk c + 1's bounds (checked and staged by the host while chunk c runs) into
    //     their own device rows, so the launch finds them in place (launch_stream dev_bounds);
    //   * the context's stream runs the launches, each followed by k_gather_reset, which writes the
    //     chunk's rows AND returns its slots to zero (no k_reset before the next launch);
    //   * s_d2h copies each chunk's rows back while the next chunk runs; the host unpacks chunk c - 1
    //     while chunk c runs;
    //   * s_pre runs each chunk's size-order pre-pass as soon as its bounds are on the device: chunk
    //     c + 1's waits for the CUs chunk c's launch frees and then runs beside chunk c's gather
    //     (r06: the two had run one after the other between the launches).
    // A small first chunk starts the device early; a small last chunk shortens the copy-back after it.
    // A bad bound fails the call (AQ_EINVAL) after the chunks before it ran; the outputs are then
    // unspecified.
    if (!ctx || (n && (!a || !b))) return AQ_EINVAL;
    const bool par = integrand == AQ_F_PARAM;
    constexpr size_t NP = (size_t)param::nparams;
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
    int rc;
    const std::vector<int> chunks = batch_chunks(n);
    const size_t nc = chunks.size();
    const size_t rows = (size_t)*std::max_element(chunks.begin(), chunks.end());   // <= MAXK
    if (ctx->bdev_rows < rows) {
        auto dfree = [&](void* p, size_t bytes) {
            if (p) { (void)hipFree(p); ctx->dev_bytes -= bytes; }
        };
        const size_t r0 = ctx->bdev_rows;
        dfree(ctx->d_batch, sizeof(double) * 8 * r0);
        dfree(ctx->d_bbounds, sizeof(double2) * 2 * r0);
        dfree(ctx->d_bsorted, sizeof(double2) * 2 * r0);
        dfree(ctx->d_bkey, sizeof(unsigned) * r0);
        dfree(ctx->d_bperm, sizeof(unsigned) * 2 * r0);
        ctx->d_batch = nullptr;
        ctx->d_bbounds = ctx->d_bsorted = nullptr;
        ctx->d_bkey = ctx->d_bperm = nullptr;
        ctx->bdev_rows = 0;
        if ((rc = dmalloc(ctx, &ctx->d_batch, sizeof(double) * 8 * rows, false))) return rc;
        if ((rc = dmalloc(ctx, &ctx->d_bbounds, sizeof(double2) * 2 * rows, false))) return rc;
        if ((rc = dmalloc(ctx, &ctx->d_bsorted, sizeof(double2) * 2 * rows, false))) return rc;
        if ((rc = dmalloc(ctx, &ctx->d_bkey, sizeof(unsigned) * rows, false))) return rc;
        if ((rc = dmalloc(ctx, &ctx->d_bperm, sizeof(unsigned) * 2 * rows, false))) return rc;
        ctx->bdev_rows = rows;
    }
    if (ctx->bhost_cap < n) {
        if (ctx->h_batch) AQ_HIP(hipHostFree(ctx->h_batch));
        if (ctx->h_bbounds) AQ_HIP(hipHostFree(ctx->h_bbounds));
        ctx->h_batch = nullptr;
        ctx->h_bbounds = nullptr;
        ctx->bhost_cap = 0;
        AQ_HIP(hipHostMalloc(&ctx->h_batch, sizeof(double) * 4 * n, hipHostMallocDefault));
        AQ_HIP(hipHostMalloc(&ctx->h_bbounds, sizeof(double2) * n, hipHostMallocDefault));
        ctx->bhost_cap = n;
    }
    if (par) {
        if ((rc = ensure_params(ctx))) return rc;
        if (ctx->btheta_rows < rows) {
            const size_t r0 = ctx->btheta_rows;
            if (ctx->d_btheta) { (void)hipFree(ctx->d_btheta); ctx->dev_bytes -= sizeof(double) * NP * 2 * r0; }
            if (ctx->d_bthsorted) { (void)hipFree(ctx->d_bthsorted); ctx->dev_bytes -= sizeof(double) * NP * 2 * r0; }
            ctx->d_btheta = ctx->d_bthsorted = nullptr;
            ctx->btheta_rows = 0;
            if ((rc = dmalloc(ctx, &ctx->d_btheta, sizeof(double) * NP * 2 * rows, false))) return rc;
            if ((rc = dmalloc(ctx, &ctx->d_bthsorted, sizeof(double) * NP * 2 * rows, false))) return rc;
            ctx->btheta_rows = rows;
        }
        if (ctx->btheta_hcap < n) {
            if (ctx->h_btheta) AQ_HIP(hipHostFree(ctx->h_btheta));
            ctx->h_btheta = nullptr;
            ctx->btheta_hcap = 0;
            AQ_HIP(hipHostMalloc(&ctx->h_btheta, sizeof(double) * NP * n, hipHostMallocDefault));
            ctx->btheta_hcap = n;
        }
    }
    if (err) {
        if ((rc = ensure_err(ctx))) return rc;
        if (ctx->berr_rows < rows) {
            if (ctx->d_berr) { (void)hipFree(ctx->d_berr); ctx->dev_bytes -= sizeof(double) * 4 * ctx->berr_rows; }
            ctx->d_berr = nullptr;
            ctx->berr_rows = 0;
            if ((rc = dmalloc(ctx, &ctx->d_berr, sizeof(double) * 4 * rows, false))) return rc;
            ctx->berr_rows = rows;
        }
        if (ctx->berr_hcap < n) {
            if (ctx->h_berr) AQ_HIP(hipHostFree(ctx->h_berr));
            ctx->h_berr = nullptr;
            ctx->berr_hcap = 0;
            AQ_HIP(hipHostMalloc(&ctx->h_berr, sizeof(double) * 2 * n, hipHostMallocDefault));
            ctx->berr_hcap = n;
        }
    }
    auto dev_err_rows_of = [&](size_t c) { return ctx->d_berr + 2 * (c & 1u) * ctx->berr_rows; };
    const size_t RT = ctx->btheta_rows;
    auto dev_theta_of = [&](size_t c) { return ctx->d_btheta + (c & 1u) * RT * NP; };
    auto thsorted_of = [&](size_t c) { return ctx->d_bthsorted + (c & 1u) * RT * NP; };
    // chunk c's device rings: bounds, rows and the size order at parity c & 1 (the keys live only
    // between a chunk's two pre-pass kernels, which run in order on s_pre)
    const size_t R = ctx->bdev_rows;
    auto dev_bounds_of = [&](size_t c) { return ctx->d_bbounds + (c & 1u) * R; };
    auto dev_rows_of = [&](size_t c) { return ctx->d_batch + 4 * (c & 1u) * R; };
    auto sorted_of = [&](size_t c) { return ctx->d_bsorted + (c & 1u) * R; };
    auto perm_of = [&](size_t c) { return ctx->d_bperm + (c & 1u) * R; };
    // size classes: counts + cursors per chunk parity (k_batch_scatter zeroes the other parity's)
    if (!ctx->d_bcnt && (rc = dmalloc(ctx, &ctx->d_bcnt, sizeof(unsigned) * 4 * EST_KEYS, false))) return rc;
    if (!ctx->d_best && (rc = dmalloc(ctx, &ctx->d_best, sizeof(double) * 2, false))) return rc;
    // chunks in size order (largest trees first: the launch's tail is its smallest jobs), unless
    // AQ_BATCH_SORT=0; chunks small enough for the per-CU instance keep their order (their bounds
    // travel as kernel arguments)
    const bool sort = env_int("AQ_BATCH_SORT", 1) != 0;
    if (!ctx->s_h2d) AQ_HIP(hipStreamCreateWithFlags(&ctx->s_h2d, hipStreamNonBlocking));
    if (!ctx->s_d2h) AQ_HIP(hipStreamCreateWithFlags(&ctx->s_d2h, hipStreamNonBlocking));
    if (!ctx->s_pre) AQ_HIP(hipStreamCreateWithFlags(&ctx->s_pre, hipStreamNonBlocking));
    std::vector<size_t> off(nc + 1, 0);
    for (size_t c = 0; c < nc; ++c) off[c + 1] = off[c] + (size_t)chunks[c];
    // four events per chunk: bounds on the device, rows gathered, rows on the host, size order done;
    // and one for the work already on the context's stream (the pre-pass stream starts behind it: a
    // caller's pending launch updates the job-size hint the first pre-pass may preset)
    std::vector<hipEvent_t> ev(4 * nc + 1, nullptr);
    for (auto& e : ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            for (auto& f : ev)
                if (f) (void)hipEventDestroy(f);
            return AQ_EHIP;
        }
    auto ev_h2d = [&](size_t c) { return ev[4 * c]; };
    auto ev_gath = [&](size_t c) { return ev[4 * c + 1]; };
    auto ev_d2h = [&](size_t c) { return ev[4 * c + 2]; };
    auto ev_pre = [&](size_t c) { return ev[4 * c + 3]; };
    const hipEvent_t ev_start = ev[4 * nc];
    unsigned errbits = 0;
    std::vector<char> sorted_chunk(nc, 0);
    // rows [i0, i1) into the outputs (k_gather_reset wrote size-ordered slots back in order)
    auto unpack_rows = [&](size_t i0, size_t i1) {
        unsigned e = 0;
        for (size_t i = i0; i < i1; ++i) {
            const double* row = ctx->h_batch + 4 * i;
            if (area) area[i] = row[0];
            if (tasks) tasks[i] = (uint64_t)row[1];
            if (accepted) accepted[i] = (uint64_t)row[2];
            e |= (unsigned)row[3];
            if (err_abs) err_abs[i] = ctx->h_berr[2 * i];
            if (err_signed) err_signed[i] = ctx->h_berr[2 * i + 1];
        }
        return e;
    };
    // chunk c's rows on several host threads (the last chunk's after the device is done; the others'
    // while the next chunk runs, beside its staging, which must stay shorter than a launch)
    auto unpack = [&](size_t c) {
        std::vector<unsigned> e(64, 0u);
        host_parallel(ctx, off[c + 1] - off[c], 8192,
                      [&](size_t i0, size_t i1, size_t p) { e[p] = unpack_rows(off[c] + i0, off[c] + i1); });
        for (unsigned x : e) errbits |= x;
    };
    // chunk c's order is preset (sets the launch's job size) while the workload is fresh
    auto sorted_at = [&](size_t c) { return sort && chunks[c] >= 64; };
    auto preset_at = [&](size_t c) {
        return sorted_at(c) && ctx->gsplit_env <= 0 &&
               !(ctx->hint.valid && ctx->hint.fid == integrand && ctx->hint.eps == eps && ctx->hint.nshards == 1);
    };
    // the size-order pre-pass of chunk c on s_pre (after its bounds arrived; the launch waits for it)
    // (preset: a fresh workload -- no measured hint for this integrand and tolerance: the pre-pass sets
    // the launch's job size from its estimates; AQ_F_* values are the kernels' FIDs)
    // (its sorted / perm parity was last read by chunk c - 2's launch and gather, which the bounds'
    // copy for chunk c already waited for)
    // The first chunk's copy and pre-pass and the last chunk's copy back run on the context's stream
    // itself: in order with the launches, where a wait across streams costs the device ~20-60 us
    // between the two operations (profiles/r06o: copy -> estimate 18 us, scatter -> launch 17 us,
    // gather -> last copy back 62 us, against ~7 us in order). The middle chunks' keep their own
    // streams, whose work overlaps the previous launch.
    auto h2d_stream = [&](size_t c) { return c == 0 ? ctx->stream : ctx->s_h2d; };
    auto pre_stream = [&](size_t c) { return c == 0 ? ctx->stream : ctx->s_pre; };
    auto d2h_stream = [&](size_t c) { return c + 1 == nc ? ctx->stream : ctx->s_d2h; };
    auto order = [&](size_t c, bool preset) -> int {
        const int m = chunks[c];
        const hipStream_t sp = pre_stream(c);
        if (hipStreamWaitEvent(sp, ev_h2d(c), 0) != hipSuccess) return AQ_EHIP;
        // (chunk 1's estimate adds into the counts chunk 0's scatter zeroed, on the context's stream)
        if (c == 1 && sorted_at(0) && hipStreamWaitEvent(sp, ev_pre(0), 0) != hipSuccess) return AQ_EHIP;
        const unsigned blocks = (unsigned)((m + 255) / 256);
        unsigned* const cnt = ctx->d_bcnt + 2 * EST_KEYS * (c & 1u);
        unsigned* const cnt_next = ctx->d_bcnt + 2 * EST_KEYS * ((c + 1) & 1u);
        if (par)
            hipLaunchKernelGGL(k_batch_estimate_params, dim3(blocks), dim3(256), 0, sp, dev_bounds_of(c),
                               (const double*)dev_theta_of(c), m, eps, ctx->d_bkey, cnt, ctx->d_best + (c & 1u), ctx->d_tab);
        else
            with_fid(integrand, [&](auto F) {
                hipLaunchKernelGGL(k_batch_estimate<decltype(F)::value>, dim3(blocks), dim3(256), 0, sp, dev_bounds_of(c), m,
                                   eps, ctx->d_bkey, cnt, ctx->d_best + (c & 1u), ctx->d_tab);
            });
        hipLaunchKernelGGL(k_batch_scatter, dim3(blocks), dim3(256), 0, sp, dev_bounds_of(c),
                           ctx->d_bkey, m, cnt, cnt + EST_KEYS, sorted_of(c),
                           perm_of(c), cnt_next, ctx->d_best + (c & 1u), ctx->d_best + ((c + 1) & 1u),
                           preset ? ctx->d_hint : nullptr, (unsigned)(ctx->grid * NW));
        if (par)
            hipLaunchKernelGGL(k_batch_scatter_theta, dim3((unsigned)(((size_t)m * NP + 255) / 256)), dim3(256), 0, sp,
                               (const double*)dev_theta_of(c), (const unsigned*)perm_of(c), m, (int)NP, thsorted_of(c));
        if (hipGetLastError() != hipSuccess || hipEventRecord(ev_pre(c), sp) != hipSuccess) return AQ_EHIP;
        return AQ_OK;
    };
    // check chunk c's bounds, stage them and copy them to the device on s_h2d (on several host threads:
    // the first chunk's is the only host work before the device starts)
    auto stage_rows = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            if (par) {
                if (!params_ok(a[i], b[i], theta + i * NP)) return false;
                for (size_t j = 0; j < NP; ++j) ctx->h_btheta[i * NP + j] = theta[i * NP + j];
            } else if (!bounds_ok(integrand, a[i], b[i])) {
                return false;
            }
            ctx->h_bbounds[i] = make_double2(a[i], b[i]);
        }
        return true;
    };
    auto stage = [&](size_t c) -> int {
        std::vector<char> ok(64, 1);
        host_parallel(ctx, (size_t)chunks[c], 8192,
                      [&](size_t i0, size_t i1, size_t p) { ok[p] = stage_rows(off[c] + i0, off[c] + i1); });
        for (char o : ok)
            if (!o) return AQ_EINVAL;
        // the ring slot chunk c - 2 used: its readers (size pre-pass, launch) are done at its gather
        if (c >= 2 && hipStreamWaitEvent(ctx->s_h2d, ev_gath(c - 2), 0) != hipSuccess) return AQ_EHIP;
        if (par && hipMemcpyAsync(dev_theta_of(c), ctx->h_btheta + off[c] * NP, sizeof(double) * NP * (size_t)chunks[c],
                                  hipMemcpyHostToDevice, h2d_stream(c)) != hipSuccess)
            return AQ_EHIP;
        if (hipMemcpyAsync(dev_bounds_of(c), ctx->h_bbounds + off[c], sizeof(double2) * (size_t)chunks[c],
                           hipMemcpyHostToDevice, h2d_stream(c)) != hipSuccess ||
            hipEventRecord(ev_h2d(c), h2d_stream(c)) != hipSuccess)
            return AQ_EHIP;
        return AQ_OK;
    };
    const bool hist = ctx->histograms;
    ctx->histograms = false;
    size_t ran = 0;   // chunks enqueued
    rc = AQ_OK;
    // (the counts are zeroed on s_pre, ahead of the first estimate, once the work already queued on the
    // context's stream is done -- a pending launch may still read or write the hint the first scatter
    // may preset)
    if (hipEventRecord(ev_start, ctx->stream) != hipSuccess || hipStreamWaitEvent(ctx->s_pre, ev_start, 0) != hipSuccess)
        rc = AQ_EHIP;
    if (rc == AQ_OK && sort &&
        (hipMemsetAsync(ctx->d_bcnt, 0, sizeof(unsigned) * 4 * EST_KEYS, pre_stream(0)) != hipSuccess ||
         hipMemsetAsync(ctx->d_best, 0, sizeof(double) * 2, pre_stream(0)) != hipSuccess))
        rc = AQ_EHIP;
    mark("setup", -1);
    if (rc == AQ_OK) rc = stage(0);
    mark("staged", 0);
    if (rc == AQ_OK && sorted_at(0)) rc = order(0, preset_at(0));
    for (size_t c = 0; c < nc && rc == AQ_OK; ++c) {
        const int m = chunks[c];
        sorted_chunk[c] = sorted_at(c);
        if (hipStreamWaitEvent(ctx->stream, sorted_chunk[c] ? ev_pre(c) : ev_h2d(c), 0) != hipSuccess) {
            rc = AQ_EHIP;
            break;
        }
        ctx->hint.preset = preset_at(c);
        ctx->batch_heap = true;
        rc = par ? launch_params(ctx, m, a + off[c], b + off[c], nullptr, eps, 0, 0, 1, 0,
                                 sorted_chunk[c] ? sorted_of(c) : dev_bounds_of(c),
                                 sorted_chunk[c] ? thsorted_of(c) : dev_theta_of(c), err)
                 : launch_any(ctx, integrand, m, a + off[c], b + off[c], nullptr, eps, 0, 0, 1, 0,
                              sorted_chunk[c] ? sorted_of(c) : dev_bounds_of(c), err);
        ctx->batch_heap = false;
        ctx->hint.preset = false;
        mark("launched", (long)c);
        if (rc) break;
        // the rows' ring slot: chunk c - 2's copy to the host must be done before they are overwritten
        if (c >= 2 && hipStreamWaitEvent(ctx->stream, ev_d2h(c - 2), 0) != hipSuccess) { rc = AQ_EHIP; break; }
        hipLaunchKernelGGL(k_gather_reset, dim3((m + 63) / 64), dim3(64), 0, ctx->stream, ctx->d_ctl, ctx->d_parts,
                           ctx->grid, 0, m, dev_rows_of(c), sorted_chunk[c] ? perm_of(c) : nullptr);
        if (err)   // (its rows' ring slot is free as the rows' is: the wait for chunk c - 2's copy above)
            hipLaunchKernelGGL(k_gather_err, dim3((m + 63) / 64), dim3(64), 0, ctx->stream, ctx->d_err, 0, m,
                               dev_err_rows_of(c), sorted_chunk[c] ? perm_of(c) : nullptr);
        if (hipGetLastError() != hipSuccess || hipEventRecord(ev_gath(c), ctx->stream) != hipSuccess) {
            rc = AQ_EHIP;
            break;
        }
        if (err) memset(ctx->err_dirty, 0, (size_t)m);   // k_gather_err zeroed them
        memset(ctx->dirty, 0, (size_t)m);   // k_gather_reset zeroed them
        memset(ctx->parts_dirty, 0, (size_t)m);
        ++ran;
        // the next chunk's bounds while this one runs (a bad bound stops the batch here), and its size
        // order behind them
        int rc_next = c + 1 < nc ? stage(c + 1) : AQ_OK;
        if (c + 1 < nc) mark("staged", (long)c + 1);
        if (rc_next == AQ_OK && c + 1 < nc && sorted_at(c + 1)) rc_next = order(c + 1, preset_at(c + 1));
        if (hipStreamWaitEvent(d2h_stream(c), ev_gath(c), 0) != hipSuccess ||
            hipMemcpyAsync(ctx->h_batch + 4 * off[c], dev_rows_of(c), sizeof(double) * 4 * (size_t)m,
                           hipMemcpyDeviceToHost, d2h_stream(c)) != hipSuccess ||
            (err && hipMemcpyAsync(ctx->h_berr + 2 * off[c], dev_err_rows_of(c), sizeof(double) * 2 * (size_t)m,
                                   hipMemcpyDeviceToHost, d2h_stream(c)) != hipSuccess) ||
            hipEventRecord(ev_d2h(c), d2h_stream(c)) != hipSuccess) {
            rc = AQ_EHIP;
            break;
        }
        if (c > 0) {   // the previous chunk's rows, while this one runs
            if (hipEventSynchronize(ev_d2h(c - 1)) != hipSuccess) { rc = AQ_EHIP; break; }
            mark("rows on host", (long)c - 1);
            unpack(c - 1);
            mark("unpacked", (long)c - 1);
        }
        rc = rc_next;
    }
    ctx->histograms = hist;
    // every enqueued chunk finishes before the buffers can be reused or the events destroyed
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == AQ_OK) rc = AQ_EHIP;
    if (hipStreamSynchronize(ctx->s_d2h) != hipSuccess && rc == AQ_OK) rc = AQ_EHIP;
    if (hipStreamSynchronize(ctx->s_h2d) != hipSuccess && rc == AQ_OK) rc = AQ_EHIP;
    if (hipStreamSynchronize(ctx->s_pre) != hipSuccess && rc == AQ_OK) rc = AQ_EHIP;
    for (auto& e : ev) (void)hipEventDestroy(e);
    mark("device done", -1);
    if (rc) return rc;
    if (ran) unpack(ran - 1);
    mark("unpacked", (long)ran - 1);
    if (trace) {
        fprintf(stderr, "aq_integrate_batch n=%zu:", n);
        for (auto& m : tr) fprintf(stderr, " [%s %.1f us]", m.first.c_str(), m.second);
        fprintf(stderr, "\n");
    }
    return err_from_bits(errbits);
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
    if (!ctx || !err_theta_ok(integrand, theta)) return AQ_EINVAL;
    return batch_run(ctx, n, a, b, theta, eps, integrand, area, accepted, tasks, true, err_abs, err_signed);
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

constexpr int MAXB = 8192;            // level-step grid cap (grid-stride beyond)
constexpr int LP_CAP = 8 * MAXB;      // level-step rows held for one deferred fold

// Fold the level-step rows written since the last fold into their accumulator (one k_level_fold).
static int fold_pending(aq_ctx* ctx) {
    if (ctx->lp_pending > 0) {
        hipLaunchKernelGGL(k_level_fold, dim3(1), dim3(FOLD_T), 0, ctx->stream, ctx->d_lparts, ctx->lp_pending, ctx->lp_acc);
        AQ_HIP(hipGetLastError());
    }
    ctx->lp_pending = 0;
    return AQ_OK;
}

static int level_step_impl(aq_ctx* ctx, int integrand, const double* d_in, uint32_t n_in, const uint32_t* d_n_in,
                           double* d_out, uint32_t cap_out, double eps, int depth, int max_depth, uint32_t* d_n_out,
                           double* d_acc) {
    if (!ctx || !d_n_out || !d_acc || (n_in && (!d_in || !d_out))) return AQ_EINVAL;
    if (!integrand_ok(integrand)) return AQ_EINVAL;
    if (!(eps >= 0.0) || depth < 0 || max_depth < 1 || max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    int rc;
    if (!ctx->d_lparts && (rc = dmalloc(ctx, &ctx->d_lparts, sizeof(LevelPart) * LP_CAP, false))) return rc;
    if (!d_n_in) AQ_HIP(hipMemsetAsync(d_n_out, 0, sizeof(uint32_t), ctx->stream));
    if (n_in == 0) return AQ_OK;
    const int grid = (int)std::min<size_t>(((size_t)n_in + LEVEL_T * LEVEL_R - 1) / (LEVEL_T * LEVEL_R), (size_t)MAXB);
    // this step's rows follow the pending ones (folded first if they belong elsewhere or would not fit)
    if (ctx->lp_pending && (d_acc != ctx->lp_acc || ctx->lp_pending + grid > LP_CAP) && (rc = fold_pending(ctx)))
        return rc;
    LevelPart* rows = ctx->d_lparts + ctx->lp_pending;
    with_fid(integrand, [&](auto F) {
        hipLaunchKernelGGL((k_level_step<decltype(F)::value>), dim3(grid), dim3(LEVEL_T), 0, ctx->stream, (const Rec*)d_in,
                           n_in, (Rec*)d_out, d_n_out, cap_out, eps, depth, max_depth, rows, ctx->d_tab, d_n_in);
    });
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

int aq_level_narrow(aq_ctx* ctx, int integrand, double* d_buf0, double* d_buf1, uint32_t cap, uint32_t* d_counts,
                    int depth, int levels, double eps, int max_depth, double* d_acc) {
    if (!ctx || !d_buf0 || !d_buf1 || !d_counts || !d_acc || levels < 0) return AQ_EINVAL;
    if (!integrand_ok(integrand)) return AQ_EINVAL;
    if (!(eps >= 0.0) || depth < 0 || max_depth < 1 || max_depth > AQ_MAX_LEVELS - 1) return AQ_EINVAL;
    if (levels == 0) return AQ_OK;
    AQ_HIP(hipSetDevice(ctx->device));
    with_fid(integrand, [&](auto F) {
        hipLaunchKernelGGL((k_level_narrow<decltype(F)::value>), dim3(1), dim3(NARROW_T), 0, ctx->stream, (Rec*)d_buf0,
                           (Rec*)d_buf1, cap, d_counts, depth, levels, eps, max_depth, d_acc, ctx->d_tab);
    });
    AQ_HIP(hipGetLastError());
    return AQ_OK;
}

int aq_frontier_integrate(aq_ctx* ctx, const aq_problem* p, uint32_t cap, int sync_every, aq_result* res,
                          uint64_t* tpl, uint64_t* lpl, int maxlev) {
    // The frontier engine of ppls_amd/frontier.py for ONE GPU with its host loop in C: the root, the
    // narrow top in one launch, then chained level steps (device counts, deferred folds) with a host
    // look at the frontier size every sync_every levels -- the Python loop's per-level torch / ctypes
    // work (several us a level) is what this saves.
    if (!ctx || cap < 2 || sync_every < 1 || maxlev < 0) return AQ_EINVAL;
    int rc = validate(p);
    if (rc) return rc;
    AQ_HIP(hipSetDevice(ctx->device));
    const int max_depth = p->max_depth ? p->max_depth : AQ_DEFAULT_MAX_DEPTH;
    if ((rc = ensure_front(ctx, cap))) return rc;
    if (!ctx->d_facc && (rc = dmalloc(ctx, &ctx->d_facc, sizeof(double) * 8, false))) return rc;
    if (!ctx->h_fcount) AQ_HIP(hipHostMalloc(&ctx->h_fcount, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), hipHostMallocDefault));
    if (!ctx->h_facc) AQ_HIP(hipHostMalloc(&ctx->h_facc, sizeof(double) * 8, hipHostMallocDefault));
    unsigned* cnt = ctx->d_count;
    double* acc = ctx->d_facc;
    double* buf[2] = {reinterpret_cast<double*>(ctx->d_front[0]), reinterpret_cast<double*>(ctx->d_front[1])};
    AQ_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), ctx->stream));
    AQ_HIP(hipMemsetAsync(acc, 0, sizeof(double) * 8, ctx->stream));
    AQ_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cnt), 1, 1, ctx->stream));   // counts[0] = the root
    if ((rc = aq_frontier_root(ctx, p->integrand, p->a, p->b, buf[0]))) return rc;
    const bool defer0 = ctx->defer_fold;
    ctx->defer_fold = true;
    int depth = std::min(13, max_depth - 1);   // the narrow top (<= 2^12 records a level): one launch
    if (depth > 0 && (rc = aq_level_narrow(ctx, p->integrand, buf[0], buf[1], cap, cnt, 0, depth, p->eps, max_depth, acc))) {
        ctx->defer_fold = defer0;
        return rc;
    }
    depth = std::max(depth, 0);
    unsigned long long bound = std::min<unsigned long long>(1ull << depth, cap);
    unsigned n = 1;
    int since = 0;
    while (depth <= max_depth && depth < AQ_MAX_LEVELS) {
        rc = level_step_impl(ctx, p->integrand, buf[depth & 1], (uint32_t)bound, cnt + depth, buf[(depth + 1) & 1], cap,
                             p->eps, depth, max_depth, cnt + depth + 1, acc);
        if (rc) break;
        ++depth;
        bound = std::min<unsigned long long>(2 * bound, cap);
        if (++since == sync_every) {
            since = 0;
            if ((rc = fold_pending(ctx))) break;
            AQ_HIP(hipMemcpyAsync(ctx->h_fcount, cnt + depth, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
            AQ_HIP(hipStreamSynchronize(ctx->stream));
            n = ctx->h_fcount[0];
            if (n == 0) break;
            if (n > cap) { rc = AQ_EOVERFLOW; break; }
            bound = n;
        }
    }
    ctx->defer_fold = defer0;
    if (rc == AQ_OK) rc = fold_pending(ctx);
    else (void)fold_pending(ctx);
    AQ_HIP(hipMemcpyAsync(ctx->h_fcount, cnt, sizeof(unsigned) * (AQ_MAX_LEVELS + 2), hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipMemcpyAsync(ctx->h_facc, acc, sizeof(double) * 8, hipMemcpyDeviceToHost, ctx->stream));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    if (rc) return rc;
    const double* a = ctx->h_facc;
    const unsigned* c = ctx->h_fcount;
    HostOut& h = ctx->last;
    h = HostOut();
    h.area = a[0] + a[1];
    h.tasks = (unsigned long long)a[2];
    h.leaves = (unsigned long long)a[3];
    h.error = (unsigned)a[4];
    h.levels = (unsigned)a[5];
    for (int d = 0; d < AQ_MAX_LEVELS && d + 1 < AQ_MAX_LEVELS + 2; ++d) {
        h.hist[d] = c[d];
        h.hist[AQ_MAX_LEVELS + d] = c[d] - c[d + 1] / 2u;
    }
    ctx->last_valid = true;
    fill_result(ctx, h, res);
    rc = err_from_bits(h.error);
    if (rc) return rc;
    if (c[std::min(depth, AQ_MAX_LEVELS + 1)] > 0) return AQ_EDEPTH;
    return aq_level_histogram(ctx, tpl, lpl, maxlev);
}

int aq_kernel_timing(aq_ctx* ctx, int enable) {
    if (!ctx) return AQ_EINVAL;
    AQ_HIP(hipSetDevice(ctx->device));
    AQ_HIP(hipStreamSynchronize(ctx->stream));
    for (auto& e : ctx->ev_pending) ctx->ev_free.push_back(e);
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
        ctx->ev_free.push_back(e);
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
