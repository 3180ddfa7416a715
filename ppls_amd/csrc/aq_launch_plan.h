// aq_launch_plan.h -- the shape of one persistent launch (k_stream, aq_stream.h): which instance runs, with
// how many waves, shares, seed depth, tail and job mode, and what the launch leaves in the job-size hint's
// host state. Pure integer arithmetic on the request: aq_abi.inc launch_stream enqueues what this decides.
//
// Plain host C++17, no HIP: the CPU tests replay recorded plans through it (tests/test_launch_plan.py).
#pragma once
#include <algorithm>

#include "aquad.h"
#include "aq_shape.h"

namespace aq {

struct LaunchRequest {
    int fid = AQ_F_COSH4;      // AQ_F_* (= the kernels' FID)
    int grid = 0;              // persistent workgroups
    int k = 0;                 // integrals
    bool shard_array = false;  // a per-integral shard array is given (mixed launches)
    int nshards = 1;
    int first_slot = 0;
    bool diag = false;         // the context collects diagnostics (DIAG instances)
    bool batch_heap = false;   // a batch front end's launch
    int gsplit_env = 0;        // AQ_GSPLIT: waves per job of a multi-integral launch (0 = default)
    double eps = 0.0;
    bool err = false;          // an ERR launch: the error estimate's sums beside the area (k_stream ERR)
};

// Waves per workgroup of every ERR launch, whatever its shape (two per SIMD: the ERR instances' registers,
// aq_stream.h k_stream). One value for all of them, so every ERR launch of one nshards deals the same
// partition and an integral's shards add up; the counts do not depend on the partition.
constexpr int ERR_NW = 8;
static_assert(ERR_NW <= NW && ERR_NW % 4 == 0, "whole waves per SIMD, within the LDS rings");

// The workload the device's job-size hint (LaunchHint) was measured on, as the host knows it.
struct HintState {
    bool valid = false;
    bool preset = false;       // the next launch takes the hint the batch pre-pass just set
    bool per_ok = false;       // the hint's per_next is current (its last writer: a HEAPS launch)
    int fid = -1, nshards = 0;
    double eps = 0.0;
};

// k_stream<FID, HIST, ...>'s instances: <DIAG, PCU> | lone (PCU, AQ_LONE_NW waves) | heap (HEAPS)
enum class Variant : int { PLAIN, PCU, DIAG, DIAG_PCU, LONE, HEAP };

struct LaunchPlan {
    int rc = AQ_OK;            // AQ_EINVAL: refused, nothing else is set and the hint is unchanged
    Variant variant = Variant::PLAIN;
    int nwt = NW;              // waves per workgroup
    int shares = 0, D = 0;     // shares per integral, seed depth
    int tail_from = 0, tail_mult = 1;
    int per_cu = 0, static_jobs = 0, adaptive = 0;
    HintState hint;            // the hint state after the launch
    bool err = false;          // the request's ERR flag: the variant's ERR instance runs (PCU, LONE -> the per-CU
                               // one; PLAIN; HEAP), without diagnostics
};

// seeding keeps F and flags of every path node of a share in the wave's ring: (D + 1) levels x
// ceil(2^D / V) positions, + 2, within cap slots
inline bool seed_fits(int D, unsigned long long V, unsigned long long cap) {
    const unsigned long long nb = ((1ull << D) + V - 1) / V;
    return (unsigned long long)(D + 1) * nb + 2 <= cap;
}

inline LaunchPlan plan_launch(const LaunchRequest& r, const HintState& hint) {
    LaunchPlan p;
    p.hint = hint;
    const int k = r.k, nshards = r.nshards;
    const bool sin_recip = r.fid == AQ_F_SIN_RECIP;
    // per-CU launches (k < PCU_MAXK) pass their bounds as kernel arguments: no staging copy
    // (per-CU launches keep per-workgroup words: slots below NPARTS and the sync slot only)
    const bool pcu = k < PCU_MAXK && (r.first_slot + k <= NPARTS || r.first_slot == SYNC_SLOT);
    const bool unsharded = nshards == 1 && !r.shard_array;
    // unsharded lone launches run AQ_LONE_NW waves per workgroup (r05, VERDICT r4 #4: the set-up and
    // seeding of a lone integral are VALU-bound at three waves per SIMD); sharded ones keep NW, the
    // partition the oracle restates (and every rank's shards must share)
    // (not the skewed integrand: its lone tree sits in one small region, and 8 waves per CU measured
    // 69.3 us against 67.3 at 12, profiles/r05k)
    // (one integral only, k == 1: the measured case and the partition include/aquad.h documents; launches
    // of 2-11 integrals keep NW)
    // (ERR launches run no diagnostics instance)
    const bool diag = r.diag && !r.err;
    const bool lone = !sin_recip && AQ_LONE_NW != NW && pcu && !diag && unsharded && k == 1;
    p.nwt = r.err ? ERR_NW : lone ? AQ_LONE_NW : NW;
    p.err = r.err;
    const int W = r.grid * p.nwt;
    // the batch front end's multi-integral launches and unsharded launches of fewer integrals than waves:
    // the instance with heap-order seeding of whole-integral jobs and up to one job per wave (aq_stream.h
    // HEAPS, MIN_JOB_TASKS)
    const bool heap = !pcu && !diag && (r.batch_heap || (k < W && unsharded));
    p.variant = heap ? Variant::HEAP : lone ? Variant::LONE
              : diag ? (pcu ? Variant::DIAG_PCU : Variant::DIAG) : (pcu ? Variant::PCU : Variant::PLAIN);
    // jobs: one integral is split into one share per wave (the partition the oracle restates); a
    // multi-integral launch uses gsplit-times larger shares, so one seeding pass feeds more rounds.
    // A shard of N holds 1/N of each integral: its shares are N times fewer, so a job (and its
    // seeding overhead) stays the same size whatever N (strong scaling).
    // (launches of few whole integrals: LONE_GSPLIT waves per share -- with 3 only a quarter of each
    // workgroup's waves, one per SIMD, seed, and the pool hands the others work; shards keep one share
    // per wave, the partition oracle/aq_oracle.c restates)
    // unsharded launches of more than a per-CU launch's integrals claim jobs (adaptive, the fill rule); the
    // static one-share-per-wave deal stays for per-CU launches and for shards below STATIC_MAXK (r06: an
    // unsharded 12-15-integral launch had dealt W shares of each integral statically -- every wave k jobs,
    // k flushes onto the same k slots' lines: 392-458 us at eps=1e-10 where 11 took 152 and 16 157,
    // profiles/r06zd)
    const int static_below = unsharded ? PCU_MAXK : STATIC_MAXK;
    // (an unsharded static launch of k > 1 integrals deals ~W / k shares of each, one job per wave: with
    // W shares each, every wave had seeded k jobs of a few hundred tasks -- cosh4 8 integrals 109 -> 75 us
    // at eps=1e-10, 85 -> 31 us at 1e-8; the skewed sin(1/x) keeps W shares up to 4 integrals, where its
    // heavy region wants the finer deal: 2 / 4 integrals 86 / 123 us against 94 / 132, 8 / 11 199 / 245
    // -> 142 / 164 us; profiles/r06zf)
    const int lone_gs = sin_recip && k <= 4 ? AQ_LONE_GSPLIT : std::max(AQ_LONE_GSPLIT, k);
    int gs = (k >= static_below || r.shard_array) ? DEFAULT_GSPLIT * std::max(1, nshards) : (unsharded ? lone_gs : 1);
    // (an unsharded launch of fewer integrals than waves, before any hint: at least one share per wave,
    // as the hint's fill rule gives the next launches -- aq_stream.h MIN_JOB_TASKS; r06)
    if (k >= static_below && unsharded) gs = std::min(gs, k);
    gs = std::min(gs, W);
    if (r.gsplit_env > 0) gs = r.gsplit_env;
    while (gs > 1 && W % gs != 0) gs >>= 1;
    p.shares = W / gs;
    const unsigned long long V = (unsigned long long)p.shares * (unsigned long long)nshards;
    // (a lone integral seeded 1-2 levels deeper -- ~6-11 positions per share -- fell to the
    // multi-pass seeding path: +11 us at eps=1e-10, r02; it seeds at the same depth as the rest)
    p.D = seed_depth_job(V);
    // the skewed integrand's unsharded lone launches seed one level deeper (the seeding's dual path,
    // up to 128 nodes): its one heavy region then spreads over twice the positions (config-4 lone
    // 78.8 -> 67.7 us, r04r; for cosh4 the dual path's +3 us outweighs the balance at eps=1e-10). The
    // partition of sharded launches (the oracle's) is unchanged.
    if (sin_recip && pcu && unsharded && seed_fits(p.D + 1, V, 128)) ++p.D;
    if (!seed_fits(p.D, V, WCAP)) {
        p = LaunchPlan{};
        p.rc = AQ_EINVAL;
        p.hint = hint;
        return p;
    }
    // smaller jobs for the launch's last ~1/32 of its integrals (unsharded multi-integral launches):
    // the end-of-launch tail (waves idle behind the longest last jobs, ~0.6 ms per launch at
    // eps=1e-10) shrinks with the jobs drawn last. Not for shards: every shard of an integral must
    // use the same partition, and a shard's place in its launch says nothing about where the
    // integral's other shards sit (dist.integrate_batch_distributed packs units of different
    // integrals and shards in any order; a sharded tail, +0.3-0.5 % per task in the bench's aligned
    // launches, broke test_rebalanced_batch_over_rccl's counts, profiles/r04n6).
    p.tail_from = k;
    p.tail_mult = 1;
    if (k >= 64 && unsharded && r.gsplit_env <= 0) {
        // (the in-kernel hint may raise the shares; seeding then backs off to the slow path if the
        // tail's nodes exceed one wave, never past WCAP: D grows by log2(mult) only)
        const unsigned long long Vt = std::min<unsigned long long>(V * AQ_TAIL_MULT, (unsigned long long)W);
        if (seed_fits(seed_depth_job(Vt), Vt, WCAP)) {
            p.tail_from = k - std::max(1, k / AQ_TAIL_DIV);
            p.tail_mult = AQ_TAIL_MULT;
        }
    }
    p.per_cu = pcu ? 1 : 0;   // per-CU task counts for lone integrals (the reference's per-worker printout)
    p.static_jobs = k < static_below ? 1 : 0;   // few integrals: one share per wave, static stride
    // multi-integral launches size their jobs from the previous launch's tasks per integral, when
    // that launch integrated the same integrand at the same tolerance (a context that switches
    // workload starts from the default shares and a fresh hint). Not for shards: every shard of an
    // integral must use the same partition (shares, seed depth), and each rank's hint would come
    // from its own, slightly different, share of the work.
    if (k >= static_below && r.gsplit_env <= 0 && unsharded) {
        const bool same_workload = hint.valid && hint.fid == r.fid && hint.eps == r.eps && hint.nshards == nshards;
        // (hint.preset: the batch front end's pre-pass set this launch's job size on the device)
        p.adaptive = same_workload || hint.preset ? 3 : 2;
        // per_next is written by the HEAPS instance (and the batch pre-pass's preset) only
        if (hint.preset || (same_workload && hint.per_ok)) p.adaptive |= 4;
        p.hint.per_ok = heap;
        p.hint.valid = true;
        p.hint.fid = r.fid;
        p.hint.eps = r.eps;
        p.hint.nshards = nshards;
    }
    return p;
}

}  // namespace aq
