// aquad.hip -- MI355X (gfx950) adaptive trapezoid quadrature: kernels + the C ABI of include/aquad.h.
//
// The design -- sibling pairs, one wavefront per worker with its own LDS ring, cellar / pool / HBM queue,
// wave-local seeding, exact area accumulators -- is described at the top of aq_stream.h (k_stream). This file
// holds the other kernels (batch size ordering, level and frontier paths, the accepted mesh, gather / reset /
// read-back).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (ppls_amd/build.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "aquad.h"
#include "aq_exp_table.h"
#include "aq_libm.h"
#include "aq_domain.h"
#include "aq_device.h"
#include "aq_stream.h"
#include "aq_launch_plan.h"
#include "aq_host_pool.h"
#include "aq_mesh_sort.h"

#include <rccl/rccl.h>

#pragma clang fp contract(off)

namespace aq {

// ------------------------------------------------------------------------------------------------
// Result block of the level-synchronous path (aq_integrate_levels), zeroed before each call.
// ------------------------------------------------------------------------------------------------
struct DevResults {
    double area;
    unsigned long long tasks;
    unsigned long long leaves;
    unsigned long long spilled;
    unsigned int levels;
    unsigned int error;        // AQ_E* as positive bit flags (see err_bit)
    unsigned long long tasks_per_level[AQ_MAX_LEVELS];
    unsigned long long leaves_per_level[AQ_MAX_LEVELS];
    unsigned long long cu_tasks[AQ_CU_SLOTS];
};


// ------------------------------------------------------------------------------------------------
// Parity helper: evaluate F or cosh on an array.
// ------------------------------------------------------------------------------------------------
template <int FID, bool COSH_ONLY>
__global__ __launch_bounds__(256) void k_eval(const double* __restrict__ x, double* __restrict__ out, size_t n,
                                              const ExpPair* __restrict__ gtab) {
    constexpr int TF = COSH_ONLY ? F_COSH4 : FID;
    __shared__ ExpEntry tab[ftab_entries<TF>()];
    stage_f_table<TF>(tab, gtab);
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if constexpr (FID == F_COSH4 && !COSH_ONLY) {
        // F through the persistent kernel's batched path (integrand_k: two interleaved cosh chains,
        // 2 cosh and 16 F), two points per lane; aq_eval_cosh keeps the scalar one
        const ExpConsts kk = pinned_exp_consts();
        for (size_t i = 2 * gid; i < n; i += 2 * stride) {
            const double xx[2] = {x[i], x[i + 1 < n ? i + 1 : i]};
            double ff[2];
            integrand_k<F_COSH4, 2, true>(xx, ff, tab, kk);   // 16 F, as k_stream's rounds (exact /16)
            out[i] = ff[0] / f_scale<F_COSH4>();
            if (i + 1 < n) out[i + 1] = ff[1] / f_scale<F_COSH4>();
        }
    } else {
        for (size_t i = gid; i < n; i += stride) out[i] = COSH_ONLY ? cosh_glibc(x[i], tab) : integrand<FID>(x[i], tab);
    }
}

// F_PARAM at n points, each with its own parameter row theta[i * nparams ..] (aq_eval_integrand_params).
__global__ __launch_bounds__(256) void k_eval_params(const double* __restrict__ x, const double* __restrict__ theta,
                                                     double* __restrict__ out, size_t n,
                                                     const ExpPair* __restrict__ gtab) {
    __shared__ ExpEntry tab[ftab_entries<F_PARAM>()];
    stage_f_table<F_PARAM>(tab, gtab);
    __syncthreads();
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = gid; i < n; i += stride) {
        Theta<F_PARAM> th;
#pragma unroll
        for (int j = 0; j < param::nparams; ++j) th.v[j] = theta[i * param::nparams + j];
        out[i] = integrand<F_PARAM>(x[i], tab, th);
    }
}

// ------------------------------------------------------------------------------------------------
// Batch ordering (aq_integrate_batch, r05): a launch of whole tiny trees ends when its last-claimed jobs
// do, so the batch front end hands its launches their integrals largest first. The size of a tree is
// predicted from its top: the reference's task body (:185-191) on the 15 nodes of depths 0..3 -- F at
// the 17 points of a 1/16 grid by recursive midpoints -- and, for every depth-3 node the tree reaches
// and refines, (|diff| / eps)^(1/3) (trapezoid error ~ h^3, so the leaves a subtree needs scale like
// the cube root of its top error). Over 20 000 C3 integrals this predicts the task count with
// correlation 0.9996 (Spearman 0.9995; an offline check with the host integrand). Only the ORDER
// uses it: the counts and areas of every integral are those of its own tree whatever the order.
// ------------------------------------------------------------------------------------------------
// Size classes: key 0 = largest, EST_PER_OCTAVE classes per doubling of 1 + est, so the 256 classes span
// 2^32 (r06: 64 classes at 6 per octave ran out at est ~ 1 450, ~4 000 tasks -- at eps=1e-10 187 of the
// 200 golden C3 integrals shared key 0 and the chunk ran unsorted; 8 per octave over 256 classes order
// them with no pair more than 30 % out of order)
constexpr int EST_KEYS = 256;
constexpr double EST_PER_OCTAVE = 8.0;
// tasks per unit of the estimate: 2.77-2.90 over cosh4 [0,5] at eps = 1e-3 ... 1e-12 and 2.84 for C3's
// mean at 1e-3 and 1e-10 (an offline check with the host integrand), so a fresh workload's first launch
// can size its jobs from it (k_batch_scatter)
constexpr double EST_TASKS = 2.84;
// (theta: F_PARAM's parameter rows, integral i's at theta[i * nparams ..]; the other integrands pass null)
template <int FID>
__device__ __forceinline__ void batch_estimate(const double2* __restrict__ bounds, int n, double eps,
                                               unsigned* __restrict__ key_of, unsigned* __restrict__ counts,
                                               double* __restrict__ est_sum, const ExpPair* __restrict__ gtab,
                                               const double* __restrict__ theta) {
    __shared__ ExpEntry tab[ftab_entries<FID>()];
    __shared__ unsigned s_cnt[EST_KEYS];
    __shared__ double s_est[4];
    stage_f_table<FID>(tab, gtab);
    if (threadIdx.x < EST_KEYS) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    double est = 0.0;
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        const double2 ab = bounds[i];
        Theta<FID> th{};
        if constexpr (FID == F_PARAM) {
#pragma unroll
            for (int j = 0; j < param::nparams; ++j) th.v[j] = theta[(size_t)i * param::nparams + j];
        }
        double x[17], f[17];
        x[0] = ab.x;
        x[16] = ab.y;
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1)           // midpoints, level by level (:187)
#pragma unroll
            for (int k = s; k < 16; k += 2 * s) x[k] = (x[k - s] + x[k + s]) / 2;
#pragma unroll
        for (int k = 0; k < 17; ++k) f[k] = integrand<FID>(x[k], tab, th);   // :188
        bool alive[16] = {true};
#pragma unroll
        for (int d = 0, s = 16; d < 4; ++d, s >>= 1) {
#pragma unroll
            for (int k = 0; k < (1 << d); ++k) {
                const int lo = k * s, hi = lo + s, md = lo + s / 2;
                const double lrarea = (f[lo] + f[hi]) * (x[hi] - x[lo]) / 2;    // :185
                const double larea = (f[lo] + f[md]) * (x[md] - x[lo]) / 2;     // :189
                const double rarea = (f[md] + f[hi]) * (x[hi] - x[md]) / 2;     // :190
                const double diff = fabs((larea + rarea) - lrarea);
                const bool refine = alive[k << (3 - d)] && diff > eps;           // :191
                if (d < 3) {
                    alive[k << (3 - d)] = refine;                                // the children's slots
                    alive[(2 * k + 1) << (2 - d)] = refine;
                } else if (refine) {
                    est += cbrt(diff / eps);
                }
            }
        }
        const double lg = EST_PER_OCTAVE * log2(1.0 + est);
        const unsigned key = (unsigned)(EST_KEYS - 1) - (unsigned)min((double)(EST_KEYS - 1), lg);
        key_of[i] = key;
        atomicAdd(&s_cnt[key], 1u);
    }
    // the block's sum of the estimates (one atomic per block)
    for (int o = 32; o >= 1; o >>= 1) est += __shfl_xor(est, o, 64);
    if ((threadIdx.x & 63u) == 0u) s_est[threadIdx.x >> 6] = est;
    __syncthreads();
    if (threadIdx.x < EST_KEYS && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
    if (threadIdx.x == 0) atomicAdd(est_sum, (s_est[0] + s_est[1]) + (s_est[2] + s_est[3]));
}
template <int FID>
__global__ __launch_bounds__(256) void k_batch_estimate(const double2* __restrict__ bounds, int n, double eps,
                                                        unsigned* __restrict__ key_of, unsigned* __restrict__ counts,
                                                        double* __restrict__ est_sum, const ExpPair* __restrict__ gtab) {
    static_assert(FID != F_PARAM, "the parametrised family's estimate takes theta (k_batch_estimate_params)");
    batch_estimate<FID>(bounds, n, eps, key_of, counts, est_sum, gtab, nullptr);
}
__global__ __launch_bounds__(256) void k_batch_estimate_params(const double2* __restrict__ bounds,
                                                               const double* __restrict__ theta, int n, double eps,
                                                               unsigned* __restrict__ key_of,
                                                               unsigned* __restrict__ counts, double* __restrict__ est_sum,
                                                               const ExpPair* __restrict__ gtab) {
    batch_estimate<F_PARAM>(bounds, n, eps, key_of, counts, est_sum, gtab, theta);
}

// Scatter the chunk into size order: sorted[pos] = bounds[i], perm[pos] = i, pos = the key's offset (an
// exclusive scan of counts) + this block's reserved range + the thread's rank within it. Block 0 also
// zeroes `next` / `next_est` (the other chunk parity's counts, cursors and estimate sum: the next
// chunk's estimate adds into them; the previous chunk's scatter is done with them) and, for a fresh
// workload (hint != null), sets the launch's job size from the chunk's mean estimate: shares per
// integral for ~TASKS_PER_JOB tasks per job, as the end of an adaptive launch does from its measured
// tasks (a first launch of tiny trees with the default 16 shares had been seeding-bound, profiles/r05w).
__global__ __launch_bounds__(256) void k_batch_scatter(const double2* __restrict__ bounds, const unsigned* __restrict__ key_of,
                                                       int n, const unsigned* __restrict__ counts,
                                                       unsigned* __restrict__ cursor, double2* __restrict__ sorted,
                                                       unsigned* __restrict__ perm, unsigned* __restrict__ next,
                                                       const double* __restrict__ est_sum, double* __restrict__ next_est,
                                                       LaunchHint* __restrict__ hint, unsigned max_shares) {
    static_assert(EST_KEYS == 256, "one class per thread of the block (the scan below)");
    __shared__ unsigned s_off[EST_KEYS], s_cnt[EST_KEYS], s_base[EST_KEYS];
    const unsigned t = threadIdx.x;
    if (blockIdx.x == 0) {
        for (unsigned i = t; i < 2u * EST_KEYS; i += blockDim.x) next[i] = 0u;
        if (t == 0) {
            *next_est = 0.0;
            if (hint) {
                const double per = EST_TASKS * *est_sum / (double)max(n, 1);   // predicted tasks per integral
                const double sh = floor((per + 0.5 * TASKS_PER_JOB) / TASKS_PER_JOB);
                hint->shares_next = (unsigned)fmin(fmax(sh, 1.0), (double)max_shares);
                hint->per_next = (unsigned long long)fmax(per, 0.0);
            }
        }
    }
    // the classes' offsets: an exclusive scan of the counts, one class per thread (Hillis-Steele in LDS)
    s_cnt[t] = 0u;
    s_off[t] = counts[t];
    __syncthreads();
    for (unsigned d = 1; d < (unsigned)EST_KEYS; d <<= 1) {
        const unsigned v = t >= d ? s_off[t - d] : 0u;
        __syncthreads();
        s_off[t] += v;
        __syncthreads();
    }
    s_base[t] = t ? s_off[t - 1] : 0u;   // inclusive -> exclusive
    __syncthreads();
    s_off[t] = s_base[t];
    __syncthreads();
    const int i = (int)(blockIdx.x * blockDim.x + t);
    unsigned key = 0, rank = 0;
    if (i < n) {
        key = key_of[i];
        rank = atomicAdd(&s_cnt[key], 1u);
    }
    __syncthreads();
    if (t < EST_KEYS && s_cnt[t]) s_base[t] = s_off[t] + atomicAdd(&cursor[t], s_cnt[t]);
    __syncthreads();
    if (i < n) {
        const unsigned pos = s_base[key] + rank;
        sorted[pos] = bounds[i];
        perm[pos] = (unsigned)i;
    }
}

// The parameter rows of a size-ordered chunk (aq_integrate_batch_params), after k_batch_scatter on the same
// stream: sorted position pos holds integral perm[pos], so its row follows its bounds into the launch's order
// (a sorted theta buffer per chunk parity; the launch then reads theta by tag, like the bounds).
__global__ __launch_bounds__(256) void k_batch_scatter_theta(const double* __restrict__ theta,
                                                             const unsigned* __restrict__ perm, int n, int np,
                                                             double* __restrict__ sorted) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n * (size_t)np) return;
    const size_t pos = i / (size_t)np, j = i - pos * (size_t)np;
    sorted[i] = theta[(size_t)perm[pos] * (size_t)np + j];
}

// ------------------------------------------------------------------------------------------------
// Level-synchronous breadth-first path: one launch per tree level (debug / cross-check schedule).
// ------------------------------------------------------------------------------------------------
struct Rec {
    double l, r, fl, fr;
};

template <int FID>
__global__ __launch_bounds__(64) void k_root(double a, double b, Rec* out, const ExpPair* __restrict__ gtab) {
    __shared__ ExpEntry tab[ftab_entries<FID>()];
    stage_f_table<FID>(tab, gtab);
    __syncthreads();
    if (threadIdx.x == 0) {
        Rec r;
        r.l = a;
        r.r = b;
        r.fl = integrand<FID>(a, tab);
        r.fr = integrand<FID>(b, tab);
        out[0] = r;
    }
}

template <int FID>
__global__ __launch_bounds__(256) void k_level(const Rec* __restrict__ in, unsigned n_in, Rec* __restrict__ out,
                                               unsigned* __restrict__ n_out, unsigned cap_out, double eps, int depth,
                                               int max_depth, DevResults* __restrict__ res,
                                               const ExpPair* __restrict__ gtab) {
    __shared__ ExpEntry tab[ftab_entries<FID>()];
    __shared__ double s_area[4];
    __shared__ unsigned s_cnt[2][4];
    stage_f_table<FID>(tab, gtab);
    __syncthreads();
    double area = 0.0;
    unsigned tasks = 0, leaves = 0;
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned base = blockIdx.x * blockDim.x; base < n_in; base += stride) {
        const unsigned i = base + threadIdx.x;
        const bool active = i < n_in;
        const Rec rc = active ? in[i] : Rec{0.0, 0.0, 0.0, 0.0};
        bool refine = false;
        double mid = 0.0, fmid = 0.0;
        if (active) {
            const Step s = task_step<FID>(rc.l, rc.r, rc.fl, rc.fr, eps, tab);
            mid = s.mid;
            fmid = s.fmid;
            ++tasks;
            if (!s.refine) {
                area += s.larea + s.rarea;  // :199
                ++leaves;
            } else if (depth + 1 >= max_depth) {
                atomicOr(&res->error, ERRB_DEPTH);
            } else {
                refine = true;
            }
        }
        const unsigned long long mask = __ballot(refine);
        const unsigned cnt = __popcll(mask);
        unsigned wbase = 0;
        if (cnt) {
            if (lane_id() == 0) wbase = atomicAdd(n_out, 2u * cnt);
            wbase = __shfl(wbase, 0, 64);
        }
        if (refine) {
            const unsigned pos = wbase + 2u * mbcnt(mask);
            if (pos + 1 < cap_out) {
                out[pos] = Rec{rc.l, mid, rc.fl, fmid};      // [l, mid]  (:192-194)
                out[pos + 1] = Rec{mid, rc.r, fmid, rc.fr};  // [mid, r]  (:195-197)
            } else {
                atomicOr(&res->error, ERRB_OVERFLOW);
            }
        }
    }
    // workgroup reduction -> one atomic per counter
    const unsigned w = threadIdx.x >> 6;
    double wa = wave_sum(area);
    unsigned wt = wave_sum_u(tasks), wl = wave_sum_u(leaves);
    if (lane_id() == 0) {
        s_area[w] = wa;
        s_cnt[0][w] = wt;
        s_cnt[1][w] = wl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ba = 0.0;
        unsigned bt = 0, bl = 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
            ba += s_area[k];
            bt += s_cnt[0][k];
            bl += s_cnt[1][k];
        }
        if (bt) {
            atomicAdd(&res->area, ba);
            atomicAdd(&res->tasks, (unsigned long long)bt);
            atomicAdd(&res->leaves, (unsigned long long)bl);
            atomicAdd(&res->tasks_per_level[depth], (unsigned long long)bt);
            atomicAdd(&res->leaves_per_level[depth], (unsigned long long)bl);
            atomicAdd(&res->cu_tasks[cu_slot()], (unsigned long long)bt);
            atomicMax(&res->levels, (unsigned)(depth + 1));
        }
    }
}

// Frontier engine step (caller-owned buffers, ppls_amd/frontier.py): one task step per record, the
// refining records' children appended to `out` (wave-aggregated atomic), each block's accepted area
// (double-double), task / accepted counts, error bits and deepest level written to its own partial
// row; k_level_fold (one workgroup) folds the rows, in block order, into the caller's accumulator.
struct LevelPart {
    double hi, lo, tasks, leaves, err, levels, pad0, pad1;
};

// Children are appended with ONE atomic per workgroup and chunk of LEVEL_R x 256 records: a wave-level
// atomic per 64 records had made the wide levels a serial fan-in on the one counter (cosh4 eps=1e-12,
// 1.65 M records: 25.8 k atomics, 202 us = 0.5 TB/s; profiles/r02t). Each lane takes LEVEL_R records
// of the chunk (coalesced, LEVEL_R F chains interleaved); the block's wave counts meet in LDS
// (double-buffered by chunk parity, so two barriers per chunk suffice).
#ifndef AQ_LEVEL_R
#define AQ_LEVEL_R 4
#endif
constexpr int LEVEL_R = AQ_LEVEL_R;
// Threads per block (a chunk of LEVEL_T x LEVEL_R records per append). r03 A/B over cosh4 eps=1e-12
// under rocprofv3 (tools/frontier_ab.sh; profiles/r03_ab/frontier_ab.txt): widest level 256 threads
// 33.5 us, 512 33.2, 1024 37.6, 1024 x 8 records 54.4; a decoupled look-back scan in place of the
// atomic (chunk-ordered output, wave-parallel look-back) 40.4 us -- the PRE frontier advances ~64
// chunks per L2 round trip while all 1.6 k chunks finish at once, slower than the atomics' fan-in.
#ifndef AQ_LEVEL_T
#define AQ_LEVEL_T 256
#endif
constexpr int LEVEL_T = AQ_LEVEL_T;
#ifndef AQ_LEVEL_HOIST
#define AQ_LEVEL_HOIST 0   // r03 A/B (profiles/r03q/front_ab.txt): widest level 32.4 -> 35.4 us with it -- off
#endif
constexpr int LEVEL_NW = LEVEL_T / 64;

// The accepted mesh (aq_integrate_mesh): in their leaf-emitting form (MESH) the two level kernels append one
// record per ACCEPTED task to a leaf buffer -- all that rebuilds its two panels bit for bit, F(mid) included, so
// nothing is evaluated again -- in schedule order; k_mesh_* below put them in x order. `count` counts every
// accepted task, `cap` bounds the records stored: past it a lane only counts.
struct Leaf {
    double l, r, fl, fmid, fr;
    unsigned long long depth;
};
struct LeafSink {
    Leaf* buf;
    unsigned long long* count;
    unsigned long long cap;
};

// A level kernel's leaf-emitting form is its instance with ONE trailing LeafSink argument (k_level_step<FID,
// LeafSink>); k_level_step<FID> has an empty pack: no argument, no leaf word, the kernel as it always was.
__device__ __forceinline__ const LeafSink& leaf_sink(const LeafSink& s) { return s; }

// Many meshes in one run (aq_integrate_mesh_batch): the frontier holds every row's records of one depth, and each
// record carries its row -- not in Rec, which stays 32 bytes and two 16-byte loads, but in an index array beside
// each frontier buffer (row_in beside `in`, row_out beside `out`; children inherit it). A leaf keeps its row in
// the upper half of its depth word. theta: F_PARAM's parameter rows, gathered per record (null otherwise);
// status: the rows' AQ_ROW_* words, which a refine at max_depth ORs AQ_ROW_DEPTH into (rare: a plain atomic).
// k_level_step<FID, BatchSink> is the template's third form: the trailing pack again, nothing copied.
struct BatchSink {
    LeafSink leaf;
    const unsigned* row_in;
    unsigned* row_out;
    const double* theta;
    unsigned* status;
    unsigned n_rows;   // a row read from the frontier is clamped below it: behind a frontier overflow the last record of
                       // an odd capacity is one no step wrote, and its row indexes theta and status
};
__device__ __forceinline__ const LeafSink& leaf_sink(const BatchSink& s) { return s.leaf; }
template <typename... Sink>
constexpr bool is_batch_sink = (std::is_same<Sink, BatchSink>::value || ...);
__device__ __forceinline__ const BatchSink& batch_sink(const BatchSink& s) { return s; }

template <int FID, typename... Sink>
__global__ __launch_bounds__(LEVEL_T) void k_level_step(const Rec* __restrict__ in, unsigned n_in, Rec* __restrict__ out,
                                                    unsigned* __restrict__ n_out, unsigned cap_out, double eps,
                                                    int depth, int max_depth, LevelPart* __restrict__ parts,
                                                    const ExpPair* __restrict__ gtab,
                                                    const unsigned* __restrict__ n_in_dev, Sink... sink) {
    constexpr int R = LEVEL_R;
    constexpr bool MESH = sizeof...(Sink) == 1;
    constexpr bool BATCH = is_batch_sink<Sink...>;   // MESH with a row index per record (BatchSink)
    static_assert(sizeof...(Sink) <= 1, "at most one LeafSink or BatchSink");
    static_assert(BATCH || FID != F_PARAM, "theta comes with the batch form's rows");
    constexpr int LW = MESH ? LEVEL_NW : 1;
    __shared__ unsigned s_wl[2][LW];              // MESH: the waves' accepted counts of a chunk, by chunk parity
    __shared__ unsigned long long s_lbase[2];     // MESH: the chunk's first leaf slot
    // chained levels: the count a previous step appended (read once; uniform), clamped to n_in = the
    // host's bound (<= the input buffer's capacity; a count beyond it was flagged as an overflow)
    if (n_in_dev) n_in = min(*n_in_dev, n_in);
    __shared__ ExpEntry tab[ftab_entries<FID>()];
    __shared__ double s_h[LEVEL_NW], s_l[LEVEL_NW];
    __shared__ unsigned s_t[LEVEL_NW], s_a[LEVEL_NW], s_e[LEVEL_NW];
    __shared__ unsigned s_wc[2][LEVEL_NW], s_base[2];
    const unsigned chunk = (unsigned)LEVEL_T * R;
    // the first chunk's records are requested BEFORE the exp table is staged (AQ_LEVEL_HOIST): a block
    // of a wide level runs one chunk, and the table's global read (then the barrier) had preceded every
    // record load, adding its latency to every block's
    Rec rn[R];
    bool an[R];
    unsigned rown[BATCH ? R : 1];   // BATCH: the records' rows (an inactive lane: row 0, a valid one)
    auto load_chunk = [&](unsigned base) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const unsigned i = base + (unsigned)k * (unsigned)LEVEL_T + threadIdx.x;
            an[k] = i < n_in;
            rn[k] = an[k] ? in[i] : Rec{1.0, 1.0, 0.0, 0.0};
            if constexpr (BATCH)
                rown[k] = an[k] ? min(batch_sink(sink...).row_in[i], batch_sink(sink...).n_rows - 1u) : 0u;
        }
    };
    if (AQ_LEVEL_HOIST && blockIdx.x * chunk < n_in) load_chunk(blockIdx.x * chunk);
    stage_f_table<FID>(tab, gtab);
    __syncthreads();
    double hi = 0.0, lo = 0.0;
    unsigned tasks = 0, leaves = 0, err = 0;
    const unsigned w = threadIdx.x >> 6;
    unsigned parity = 0;
    // the loop bound depends on blockIdx only: every thread of the block runs every chunk (barriers)
    for (unsigned base = blockIdx.x * chunk; base < n_in; base += gridDim.x * chunk, parity ^= 1u) {
        Rec rc[R];
        bool active[R];
        double x[R], f[R];
        if (!AQ_LEVEL_HOIST || base != blockIdx.x * chunk) load_chunk(base);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            active[k] = an[k];
            rc[k] = rn[k];
            x[k] = (rc[k].l + rc[k].r) / 2;                              // :187
        }
        if constexpr (FID == F_PARAM) {   // every record under its own row's parameters
#pragma unroll
            for (int k = 0; k < R; ++k) {
                Theta<FID> th;
#pragma unroll
                for (int j = 0; j < param::nparams; ++j)
                    th.v[j] = batch_sink(sink...).theta[(size_t)rown[k] * param::nparams + j];
                f[k] = integrand<FID>(x[k], tab, th);                    // :188
            }
        } else {
            integrand_k<FID, R>(x, f, tab);                              // :188
        }
        bool refine[R];
        unsigned long long m[R];
        unsigned c[R + 1];
        c[0] = 0;
        bool leaf[MESH ? R : 1];
        unsigned long long ml[MESH ? R : 1];
        unsigned cl[MESH ? R + 1 : 1];
        cl[0] = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const double mid = x[k], fmid = f[k];
            const double lrarea = (rc[k].fl + rc[k].fr) * (rc[k].r - rc[k].l) / 2;   // :185
            const double larea = (rc[k].fl + fmid) * (mid - rc[k].l) / 2;            // :189
            const double rarea = (fmid + rc[k].fr) * (rc[k].r - mid) / 2;            // :190
            const bool ref = active[k] && fabs((larea + rarea) - lrarea) > eps;       // :191
            refine[k] = false;
            if (active[k]) {
                ++tasks;
                if (!ref) {
                    dd_add(hi, lo, larea + rarea);                       // :199 -> :149
                    ++leaves;
                } else if (depth + 1 >= max_depth) {
                    err |= ERRB_DEPTH;
                    if constexpr (BATCH) atomicOr(&batch_sink(sink...).status[rown[k]], (unsigned)AQ_ROW_DEPTH);
                } else {
                    refine[k] = true;
                }
            }
            m[k] = __ballot(refine[k]);
            c[k + 1] = c[k] + (unsigned)__popcll(m[k]);
            if constexpr (MESH) {
                leaf[k] = active[k] && !ref;
                ml[k] = __ballot(leaf[k]);
                cl[k + 1] = cl[k] + (unsigned)__popcll(ml[k]);
            }
        }
        // the chunk's offset: one atomic per block and chunk
        if (lane_id() == 0) s_wc[parity][w] = c[R];
        if constexpr (MESH) {
            if (lane_id() == 0) s_wl[parity][w] = cl[R];
        }
        __syncthreads();
        if (threadIdx.x == 0) {   // one atomic for the block's chunk
            unsigned tot = 0;
            for (int v = 0; v < LEVEL_NW; ++v) tot += s_wc[parity][v];
            s_base[parity] = tot ? atomicAdd(n_out, 2u * tot) : 0u;
            if constexpr (MESH) {   // ... and one for its leaves (64-bit: the count goes on past the capacity)
                unsigned totl = 0;
                for (int v = 0; v < LEVEL_NW; ++v) totl += s_wl[parity][v];
                s_lbase[parity] = totl ? atomicAdd(leaf_sink(sink...).count, (unsigned long long)totl) : 0ull;
            }
        }
        __syncthreads();
        if constexpr (MESH) {
            const LeafSink& ls = leaf_sink(sink...);
            unsigned long long loff = s_lbase[parity];
            for (unsigned v = 0; v < w; ++v) loff += s_wl[parity][v];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                if (leaf[k]) {
                    const unsigned long long pos = loff + cl[k] + mbcnt(ml[k]);
                    unsigned long long dw = (unsigned long long)depth;
                    if constexpr (BATCH) dw |= (unsigned long long)rown[k] << 32;
                    if (pos < ls.cap) ls.buf[pos] = Leaf{rc[k].l, rc[k].r, rc[k].fl, f[k], rc[k].fr, dw};
                }
            }
        }
        unsigned off = s_base[parity];
        for (unsigned v = 0; v < w; ++v) off += 2u * s_wc[parity][v];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            if (refine[k]) {
                const unsigned pos = off + 2u * (c[k] + mbcnt(m[k]));
                if (pos + 1 < cap_out) {
                    out[pos] = Rec{rc[k].l, x[k], rc[k].fl, f[k]};       // [l, mid]  (:192-194)
                    out[pos + 1] = Rec{x[k], rc[k].r, f[k], rc[k].fr};   // [mid, r]  (:195-197)
                    if constexpr (BATCH)
                        *reinterpret_cast<uint2*>(batch_sink(sink...).row_out + pos) = make_uint2(rown[k], rown[k]);
                } else {
                    err |= ERRB_OVERFLOW;
                }
            }
        }
    }
    wave_sum_dd(hi, lo);
    const unsigned wt = wave_sum_u(tasks), wl = wave_sum_u(leaves), we = wave_or_u(err);
    if (lane_id() == 0) { s_h[w] = hi; s_l[w] = lo; s_t[w] = wt; s_a[w] = wl; s_e[w] = we; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double H = 0.0, L = 0.0;
        unsigned T = 0, A = 0, E = 0;
        for (int k = 0; k < LEVEL_NW; ++k) { dd_add_dd(H, L, s_h[k], s_l[k]); T += s_t[k]; A += s_a[k]; E |= s_e[k]; }
        LevelPart p;
        p.hi = H; p.lo = L; p.tasks = (double)T; p.leaves = (double)A; p.err = (double)E;
        p.levels = T ? (double)(depth + 1) : 0.0;
        p.pad0 = p.pad1 = 0.0;
        parts[blockIdx.x] = p;
    }
}

// 256 threads each fold an interleaved share of the rows in row order, then a fixed pairwise tree
// (strides 128 .. 1) folds the 256 partials: the same order for a given row count (deterministic).
// One thread folding every row had cost 1.1 ms for the 4096 rows of a chained wide level, a serial
// fold of the 256 partials 18 us per level (profiles/r02u, r02v).
constexpr int FOLD_T = 256;
__global__ __launch_bounds__(FOLD_T) void k_level_fold(const LevelPart* __restrict__ parts, int nparts,
                                                       double* __restrict__ acc) {
    __shared__ double s_h[FOLD_T], s_l[FOLD_T], s_t[FOLD_T], s_a[FOLD_T], s_v[FOLD_T];
    __shared__ unsigned s_e[FOLD_T];
    const int t = threadIdx.x;
    double H = 0.0, L = 0.0, T = 0.0, A = 0.0, lev = 0.0;
    unsigned E = 0;
    for (int i = t; i < nparts; i += FOLD_T) {
        const LevelPart p = parts[i];
        dd_add_dd(H, L, p.hi, p.lo);
        T += p.tasks;
        A += p.leaves;
        E |= (unsigned)p.err;
        lev = fmax(lev, p.levels);
    }
    s_h[t] = H; s_l[t] = L; s_t[t] = T; s_a[t] = A; s_v[t] = lev; s_e[t] = E;
    __syncthreads();
    for (int s = FOLD_T / 2; s > 0; s >>= 1) {
        if (t < s) {
            double h = s_h[t], l = s_l[t];
            dd_add_dd(h, l, s_h[t + s], s_l[t + s]);
            s_h[t] = h; s_l[t] = l;
            s_t[t] += s_t[t + s];
            s_a[t] += s_a[t + s];
            s_v[t] = fmax(s_v[t], s_v[t + s]);
            s_e[t] |= s_e[t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    H = acc[0]; L = acc[1];
    dd_add_dd(H, L, s_h[0], s_l[0]);
    acc[0] = H; acc[1] = L; acc[2] += s_t[0]; acc[3] += s_a[0];
    acc[4] = (double)((unsigned)acc[4] | s_e[0]);
    acc[5] = fmax(acc[5], s_v[0]);
}

// The frontier's narrow levels in ONE launch: a single workgroup runs `levels`
// consecutive levels, level depth + k reading counts[depth + k] records from buf[k & 1] and writing
// its children to buf[(k + 1) & 1] and their number to counts[depth + k + 1]. The appends need no
// global atomic (one block: a block-wide prefix of the wave counts in LDS), the levels no host round
// trip and no launch each (the tree's first ~13 levels hold <= 8 k records: launch- and
// latency-bound as one launch per level, 2 launches each with the fold). The block's accumulators go
// into d_acc once at the end, as k_level_fold's would.
constexpr int NARROW_T = 1024;
// MESH: the accepted records' leaves go to `sink` behind the block-wide prefix the children use -- the launch is
// one workgroup and runs alone on its stream, so the leaf count is read once, carried block-uniform, and
// written back at the end: no atomic.
template <int FID, typename... Sink>
__global__ __launch_bounds__(NARROW_T) void k_level_narrow(Rec* __restrict__ buf0, Rec* __restrict__ buf1, unsigned cap,
                                                           unsigned* __restrict__ counts, int d0, int levels, double eps,
                                                           int max_depth, double* __restrict__ acc,
                                                           const ExpPair* __restrict__ gtab, Sink... sink) {
    constexpr int NWV = NARROW_T / 64;
    constexpr bool MESH = sizeof...(Sink) == 1;
    static_assert(sizeof...(Sink) <= 1, "at most one LeafSink");
    __shared__ unsigned s_wl[MESH ? NWV : 1];
    unsigned long long n_leaf = 0;   // MESH: leaves so far (block-uniform)
    if constexpr (MESH) n_leaf = *leaf_sink(sink...).count;
    __shared__ ExpEntry tab[ftab_entries<FID>()];
    __shared__ unsigned s_wc[NWV];
    __shared__ unsigned s_n;
    __shared__ double s_h[NWV], s_l[NWV];
    __shared__ unsigned s_t[NWV], s_a[NWV], s_e[NWV], s_v[NWV];
    stage_f_table<FID>(tab, gtab);
    if (threadIdx.x == 0) s_n = min(counts[d0], cap);
    __syncthreads();
    double hi = 0.0, lo = 0.0;
    unsigned tasks = 0, leaves = 0, err = 0, lev = 0;
    const unsigned w = threadIdx.x >> 6;
    for (int k = 0; k < levels; ++k) {
        const int depth = d0 + k;
        const Rec* __restrict__ in = (k & 1) ? buf1 : buf0;
        Rec* __restrict__ out = (k & 1) ? buf0 : buf1;
        const unsigned n_in = s_n;
        unsigned n_ref = 0;   // refining records of this level so far (block-uniform)
        for (unsigned base = 0; base < n_in; base += NARROW_T) {
            const unsigned i = base + threadIdx.x;
            const bool active = i < n_in;
            const Rec rc = active ? in[i] : Rec{1.0, 1.0, 0.0, 0.0};
            double x[1] = {(rc.l + rc.r) / 2}, f[1];                       // :187
            integrand_k<FID, 1>(x, f, tab);                                 // :188
            const double lrarea = (rc.fl + rc.fr) * (rc.r - rc.l) / 2;      // :185
            const double larea = (rc.fl + f[0]) * (x[0] - rc.l) / 2;        // :189
            const double rarea = (f[0] + rc.fr) * (rc.r - x[0]) / 2;        // :190
            bool refine = false;
            if (active) {
                ++tasks;
                lev = max(lev, (unsigned)depth + 1u);
                if (!(fabs((larea + rarea) - lrarea) > eps)) {              // :191
                    dd_add(hi, lo, larea + rarea);                          // :199 -> :149
                    ++leaves;
                } else if (depth + 1 >= max_depth) {
                    err |= ERRB_DEPTH;
                } else {
                    refine = true;
                }
            }
            const unsigned long long m = __ballot(refine);
            if (lane_id() == 0) s_wc[w] = (unsigned)__popcll(m);
            const bool leaf = MESH && active && !(fabs((larea + rarea) - lrarea) > eps);
            unsigned long long ml = 0;
            if constexpr (MESH) {
                ml = __ballot(leaf);
                if (lane_id() == 0) s_wl[w] = (unsigned)__popcll(ml);
            }
            __syncthreads();
            unsigned off = n_ref, tot = 0;
            for (unsigned v = 0; v < (unsigned)NWV; ++v) {
                const unsigned c = s_wc[v];
                off += v < w ? c : 0u;
                tot += c;
            }
            if constexpr (MESH) {
                unsigned long long loff = n_leaf;
                for (unsigned v = 0; v < (unsigned)NWV; ++v) {
                    const unsigned c = s_wl[v];
                    loff += v < w ? c : 0u;
                    n_leaf += c;
                }
                const unsigned long long pos = loff + mbcnt(ml);
                if (leaf && pos < leaf_sink(sink...).cap)
                    leaf_sink(sink...).buf[pos] = Leaf{rc.l, rc.r, rc.fl, f[0], rc.fr, (unsigned long long)depth};
            }
            __syncthreads();   // s_wc is rewritten by the next chunk
            if (refine) {
                const unsigned pos = 2u * (off + mbcnt(m));
                if (pos + 1 < cap) {
                    out[pos] = Rec{rc.l, x[0], rc.fl, f[0]};        // [l, mid]  (:192-194)
                    out[pos + 1] = Rec{x[0], rc.r, f[0], rc.fr};    // [mid, r]  (:195-197)
                } else {
                    err |= ERRB_OVERFLOW;
                }
            }
            n_ref += tot;
        }
        __syncthreads();   // the level's children are written (and visible to the block) before the next reads them
        if (threadIdx.x == 0) {
            counts[depth + 1] = 2u * n_ref;
            s_n = min(2u * n_ref, cap);
        }
        __syncthreads();
    }
    wave_sum_dd(hi, lo);
    const unsigned wt = wave_sum_u(tasks), wl = wave_sum_u(leaves), we = wave_or_u(err), wv = wave_max_u(lev);
    if (lane_id() == 0) { s_h[w] = hi; s_l[w] = lo; s_t[w] = wt; s_a[w] = wl; s_e[w] = we; s_v[w] = wv; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double H = acc[0], L = acc[1];
        unsigned T = 0, A = 0, E = 0, V = 0;
        for (int v = 0; v < NWV; ++v) {
            dd_add_dd(H, L, s_h[v], s_l[v]);
            T += s_t[v]; A += s_a[v]; E |= s_e[v]; V = max(V, s_v[v]);
        }
        acc[0] = H; acc[1] = L; acc[2] += (double)T; acc[3] += (double)A;
        acc[4] = (double)((unsigned)acc[4] | E);
        acc[5] = fmax(acc[5], (double)V);
        if constexpr (MESH) *leaf_sink(sink...).count = n_leaf;
    }
}

template <int FID>
__global__ __launch_bounds__(64) void k_frontier_root(double a, double b, Rec* out, const ExpPair* __restrict__ gtab) {
    __shared__ ExpEntry tab[ftab_entries<FID>()];
    stage_f_table<FID>(tab, gtab);
    __syncthreads();
    if (threadIdx.x == 0) out[0] = Rec{a, b, integrand<FID>(a, tab), integrand<FID>(b, tab)};
}

// ------------------------------------------------------------------------------------------------
// The accepted mesh: leaves (schedule order) -> nodes in x order with the running integral.
//   k_mesh_keys      key = the leaf's l, value = its index (sorted by aq_mesh_sort.hip, keys are unique)
//   k_mesh_expand    one sorted leaf per lane: x, f, level of its two panels; its two terms larea and
//                    larea + rarea (:189-190, :199, as k_level_step writes them) parked in cum[2j + 1] and
//                    cum[2j]; the block's double-double sum of larea + rarea
//   k_mesh_scan_parts  one block: exclusive double-double scan of the block sums, in place
//   k_mesh_cum       the parked terms back (one 16-byte load per lane), block scan, cum[2j] = P_j and
//                    cum[2j + 1] = P_j + larea_j rounded once each; the last leaf adds the closing node
// The scan's tree depends on the leaf count alone (MESH_T leaves per block, lanes in order, a shuffle scan per
// wave, the waves in order; the partials in fixed contiguous shares), so cum is bit-identical from run to run.
// ------------------------------------------------------------------------------------------------
constexpr int MESH_T = 256;
constexpr int MESH_NW = MESH_T / 64;

__global__ __launch_bounds__(MESH_T) void k_mesh_keys(const Leaf* __restrict__ leaves, unsigned n,
                                                      double* __restrict__ keys, unsigned* __restrict__ idx) {
    const unsigned i = blockIdx.x * MESH_T + threadIdx.x;
    if (i >= n) return;
    keys[i] = leaves[i].l;
    idx[i] = i;
}

// Inclusive double-double scan over the block's lanes in thread order; `tot` receives the block's sum.
__device__ __forceinline__ void mesh_block_scan(double& hi, double& lo, double& tot_hi, double& tot_lo) {
    __shared__ double s_h[MESH_NW], s_l[MESH_NW];
    const unsigned lane = lane_id(), w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double h2 = __shfl_up(hi, o, 64), l2 = __shfl_up(lo, o, 64);
        if (lane >= (unsigned)o) dd_add_dd(hi, lo, h2, l2);
    }
    if (lane == 63) { s_h[w] = hi; s_l[w] = lo; }
    __syncthreads();
    double ph = 0.0, pl = 0.0;   // the waves before this one, in order
    tot_hi = 0.0; tot_lo = 0.0;
    for (unsigned v = 0; v < (unsigned)MESH_NW; ++v) {
        if (v == w) { ph = tot_hi; pl = tot_lo; }
        dd_add_dd(tot_hi, tot_lo, s_h[v], s_l[v]);
    }
    dd_add_dd(ph, pl, hi, lo);
    hi = ph; lo = pl;
    __syncthreads();   // s_h / s_l may be written again
}

// VEC: x, f and cum are 16-byte aligned (node pairs 2j, 2j + 1 go out as one double2).
template <bool VEC>
__device__ __forceinline__ void mesh_store2(double* __restrict__ p, size_t j, double v0, double v1) {
    if constexpr (VEC) {
        reinterpret_cast<double2*>(p)[j] = make_double2(v0, v1);
    } else {
        p[2 * j] = v0;
        p[2 * j + 1] = v1;
    }
}

template <bool VEC>
__global__ __launch_bounds__(MESH_T) void k_mesh_expand(const Leaf* __restrict__ leaves, const unsigned* __restrict__ idx,
                                                        unsigned n, double* __restrict__ x, double* __restrict__ f,
                                                        double* __restrict__ cum, unsigned char* __restrict__ level,
                                                        double2* __restrict__ parts) {
    const unsigned j = blockIdx.x * MESH_T + threadIdx.x;
    double hi = 0.0, lo = 0.0;
    if (j < n) {
        const Leaf lf = leaves[idx[j]];
        const double mid = (lf.l + lf.r) / 2;                          // :187
        const double larea = (lf.fl + lf.fmid) * (mid - lf.l) / 2;     // :189
        const double rarea = (lf.fmid + lf.fr) * (lf.r - mid) / 2;     // :190
        hi = larea + rarea;                                            // :199
        mesh_store2<VEC>(x, j, lf.l, mid);
        mesh_store2<VEC>(f, j, lf.fl, lf.fmid);
        mesh_store2<VEC>(cum, j, hi, larea);
        if (level) {
            level[2 * (size_t)j] = (unsigned char)lf.depth;
            level[2 * (size_t)j + 1] = (unsigned char)lf.depth;
        }
        if (j == n - 1) {   // the closing node (its cum: k_mesh_cum)
            x[2 * (size_t)n] = lf.r;
            f[2 * (size_t)n] = lf.fr;
        }
    }
    double th, tl;
    mesh_block_scan(hi, lo, th, tl);
    if (threadIdx.x == 0) parts[blockIdx.x] = make_double2(th, tl);
}

__global__ __launch_bounds__(MESH_T) void k_mesh_scan_parts(double2* __restrict__ parts, unsigned nparts) {
    // thread t owns the contiguous share [t * per, (t + 1) * per)
    const unsigned per = (nparts + MESH_T - 1) / MESH_T;
    const unsigned b0 = min(threadIdx.x * per, nparts), b1 = min(b0 + per, nparts);
    double hi = 0.0, lo = 0.0;
    for (unsigned i = b0; i < b1; ++i) {
        const double2 p = parts[i];
        dd_add_dd(hi, lo, p.x, p.y);
    }
    double th, tl;
    mesh_block_scan(hi, lo, th, tl);
    // the share's exclusive prefix is the inclusive one of the thread before (nothing is subtracted)
    __shared__ double s_eh[MESH_T], s_el[MESH_T];
    s_eh[threadIdx.x] = hi; s_el[threadIdx.x] = lo;
    __syncthreads();
    double eh = 0.0, el = 0.0;
    if (threadIdx.x > 0) { eh = s_eh[threadIdx.x - 1]; el = s_el[threadIdx.x - 1]; }
    for (unsigned i = b0; i < b1; ++i) {
        const double2 p = parts[i];
        parts[i] = make_double2(eh, el);
        dd_add_dd(eh, el, p.x, p.y);
    }
}

template <bool VEC>
__global__ __launch_bounds__(MESH_T) void k_mesh_cum(unsigned n, double* __restrict__ cum,
                                                     const double2* __restrict__ parts) {
    const unsigned j = blockIdx.x * MESH_T + threadIdx.x;
    double area = 0.0, larea = 0.0;
    if (j < n) {
        if constexpr (VEC) {
            const double2 t = reinterpret_cast<const double2*>(cum)[j];
            area = t.x; larea = t.y;
        } else {
            area = cum[2 * (size_t)j]; larea = cum[2 * (size_t)j + 1];
        }
    }
    double hi = area, lo = 0.0, th, tl;
    mesh_block_scan(hi, lo, th, tl);
    __shared__ double s_ih[MESH_T], s_il[MESH_T];   // every lane's inclusive prefix, for the lane after it
    s_ih[threadIdx.x] = hi; s_il[threadIdx.x] = lo;
    __syncthreads();
    if (j >= n) return;
    const double2 base = parts[blockIdx.x];
    double ih = base.x, il = base.y;          // P_{j+1}: the blocks before, then this block's inclusive prefix
    dd_add_dd(ih, il, hi, lo);
    // P_j: the blocks before and the inclusive prefix of the lane before (the block's first lane: the base alone)
    double ph = base.x, pl = base.y;
    if (threadIdx.x > 0) dd_add_dd(ph, pl, s_ih[threadIdx.x - 1], s_il[threadIdx.x - 1]);
    double mh = ph, ml = pl;
    dd_add_dd(mh, ml, larea, 0.0);
    mesh_store2<VEC>(cum, j, ph + pl, mh + ml);
    if (j == n - 1) cum[2 * (size_t)n] = ih + il;
}

// Integral from x_0 to q on a mesh (aq_mesh_eval): the trapezoid rule on the partial panel, one IEEE operation
// per step (the file is built with -ffp-contract=off). One query per lane, a binary search over x for the last
// node <= q among 0 .. m - 1.
// (one query, shared with k_mesh_eval_batch, which runs it on a row's slice)
__device__ __forceinline__ double mesh_eval_one(unsigned long long n_nodes, const double* __restrict__ x,
                                                const double* __restrict__ f, const double* __restrict__ cum,
                                                double qq) {
    const unsigned long long m = n_nodes - 1;
    if (!(qq >= x[0] && qq <= x[m])) return __longlong_as_double(0x7ff8000000000000ll);   // outside, or NaN
    unsigned long long lo = 0, hi = m - 1;   // x[lo] <= q; the answer is in [lo, hi]
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo + 1) / 2;
        if (x[mid] <= qq) lo = mid;
        else hi = mid - 1;
    }
    const double xk = x[lo], fk = f[lo];
    const double h = qq - xk;
    const double w = x[lo + 1] - xk;
    const double fq = fk + (f[lo + 1] - fk) * (h / w);
    return cum[lo] + (fk + fq) * h / 2;
}
__global__ __launch_bounds__(256) void k_mesh_eval(unsigned long long n_nodes, const double* __restrict__ x,
                                                   const double* __restrict__ f, const double* __restrict__ cum,
                                                   size_t nq, const double* __restrict__ q, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    out[i] = mesh_eval_one(n_nodes, x, f, cum, q[i]);
}

// The x at which the running integral reaches y (aq_mesh_invert): k = the largest index <= m - 1 with cum_k <= y,
// then the stable root of r = f_k h + s h^2 / 2 on that panel, one IEEE operation per step (the header states
// them). The search is the cost -- 21 halving steps on the 1.5 M nodes of eps = 1e-10, each a dependent load -- and
// every step tests the one monotone predicate "index <= m - 1 and cum <= y" at lo + 2^b, b counting down, so for a
// non-decreasing cum any split of the steps returns the k defined above, equal runs included. Two instances:
//   LOG_TAB == 0  every step in global memory, one query per lane: sh = the bits of m - 1 (few queries);
//   LOG_TAB  > 0  every workgroup stages cum[j << sh], j < entries <= 2^LOG_TAB, into LDS (sh the least stride that
//                 fits; pad = NaN, which no y is >=, so the pad is never stepped onto), answers its queries
//                 grid-stride, and takes the steps above bit sh in the table -- halving from `top`, 2 * top the
//                 least power of two >= entries -- and only the sh below it in global memory. sh == 0
//                 (m <= 2^LOG_TAB): the table is cum.
// Either way the last three steps run on registers: the 8 nodes from lo and the one after them, loaded in one round
// trip, are also the panel's cum_k and cum_k+1. For any cum, monotone or not, a table index stays below `entries`
// and a node index in [0, m - 1] (loads past it are clamped to m and not looked at).
// The steps below bit sh from `lo`, the last three on registers, and the panel's root (every instance, and
// k_mesh_invert_batch on a row's slice): x, f, cum are the mesh's, last = m - 1, q a y inside [cum_0, cum_m].
__device__ __forceinline__ double mesh_invert_from(unsigned long long lo, unsigned sh, unsigned long long last,
                                                   const double* __restrict__ x, const double* __restrict__ f,
                                                   const double* __restrict__ cum, double q) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (unsigned b = sh; b-- > 3;) {
        const unsigned long long mid = lo + (1ull << b);
        const double c = cum[min(mid, last)];
        if (mid <= last && c <= q) lo = mid;
    }
    // steps 4, 2, 1 on v[e] = cum[lo + e], e <= rem in range. (Where fewer than three steps were left, sh < 3,
    // the run of 8 is wider than needed and holds the answer all the same: lo <= k.)
    const unsigned long long rem = last - lo;
    double v[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) v[e] = cum[min(lo + e, last + 1)];
    const bool t4 = 4 <= rem && v[4] <= q;
    const unsigned e2 = t4 ? 6 : 2;                 // the candidates at lo + e2 - 1 .. lo + e2 + 2
    const double a1 = t4 ? v[5] : v[1], a2 = t4 ? v[6] : v[2], a3 = t4 ? v[7] : v[3], a4 = t4 ? v[8] : v[4];
    const bool t2 = e2 <= rem && a2 <= q;
    const unsigned e1 = e2 + (t2 ? 1 : -1);         // ... at lo + e1, lo + e1 + 1
    const double c1 = t2 ? a3 : a1, c2 = t2 ? a4 : a2;
    const bool t1 = e1 <= rem && c1 <= q;
    const unsigned long long k = lo + e1 - (t1 ? 0 : 1);
    const double ck = t1 ? c1 : t2 ? a2 : t4 ? v[4] : v[0];
    const double ck1 = t1 ? c2 : c1;
    double res = nan;
    if (ck <= q && q <= ck1) {   // (fails only where cum is not non-decreasing)
        const double xk = x[k], fk = f[k];
        const double w = x[k + 1] - xk;
        const double r = q - ck;
        const double s = (f[k + 1] - fk) / w;
        const double disc = fmax(fk * fk + (2 * s) * r, 0.0);
        const double den = fk + __dsqrt_rn(disc);
        double h = r == 0 ? 0.0 : (2 * r) / den;
        h = fmin(h, w);
        res = xk + h;
    }
    return res;
}
template <int LOG_TAB>
__global__ __launch_bounds__(256) void k_mesh_invert(unsigned long long n_nodes, const double* __restrict__ x,
                                                     const double* __restrict__ f, const double* __restrict__ cum,
                                                     size_t nq, const double* __restrict__ y, double* __restrict__ out,
                                                     unsigned sh, unsigned entries, unsigned top) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const unsigned long long last = n_nodes - 2;   // m - 1: the largest k
    __shared__ double tab[1u << LOG_TAB];
    if constexpr (LOG_TAB > 0) {
        const unsigned fill = top ? 2 * top : 1;   // the steps read tab[1 .. 2 * top - 1]
        for (unsigned j = threadIdx.x; j < fill; j += 256) tab[j] = j < entries ? cum[(unsigned long long)j << sh] : nan;
        __syncthreads();
    }
    const double c0 = cum[0], cm = cum[last + 1];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (size_t)gridDim.x * 256) {
        const double q = y[i];
        if (!(q >= c0 && q <= cm)) {   // outside, or NaN
            out[i] = nan;
            continue;
        }
        unsigned long long lo = 0;
        if constexpr (LOG_TAB > 0) {
            unsigned j = 0;
            for (unsigned step = top; step; step >>= 1)
                if (tab[j + step] <= q) j += step;
            lo = (unsigned long long)j << sh;
        }
        out[i] = mesh_invert_from(lo, sh, last, x, f, cum, q);
    }
}

// aq_mesh_eval_batch / aq_mesh_invert_batch: row i's nq queries on the slice [off[i], off[i + 1]) of a batch mesh,
// one query per lane, the search and the arithmetic those of the single-mesh kernels (mesh_eval_one; the plain
// instance's halving steps from sh = the bits of the row's m - 1). A row of fewer than 3 nodes answers NaN.
__global__ __launch_bounds__(256) void k_mesh_eval_batch(const unsigned long long* __restrict__ off,
                                                         const double* __restrict__ x, const double* __restrict__ f,
                                                         const double* __restrict__ cum, size_t nq, size_t total,
                                                         const double* __restrict__ q, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / nq;
    const unsigned long long o0 = off[row], nn = off[row + 1] - o0;
    double res = __longlong_as_double(0x7ff8000000000000ll);
    if (nn >= 3) res = mesh_eval_one(nn, x + o0, f + o0, cum + o0, q[i]);
    out[i] = res;
}
__global__ __launch_bounds__(256) void k_mesh_invert_batch(const unsigned long long* __restrict__ off,
                                                           const double* __restrict__ x, const double* __restrict__ f,
                                                           const double* __restrict__ cum, size_t nq, size_t total,
                                                           const double* __restrict__ y, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / nq;
    const unsigned long long o0 = off[row], nn = off[row + 1] - o0;
    double res = __longlong_as_double(0x7ff8000000000000ll);
    if (nn >= 3) {
        const double* c = cum + o0;
        const unsigned long long last = nn - 2;
        const double qq = y[i];
        if (qq >= c[0] && qq <= c[last + 1]) {
            const unsigned sh = 64u - (unsigned)__clzll((long long)last);   // 2^sh > m - 1 (last >= 1)
            res = mesh_invert_from(0ull, sh, last, x + o0, f + o0, c, qq);
        }
    }
    out[i] = res;
}

// ------------------------------------------------------------------------------------------------
// Many meshes in one call (aq_integrate_mesh_batch): every row's tree in ONE frontier (k_level_step<FID,
// BatchSink>), the leaves ordered by (row, l) -- the sort by l, then a stable sort of the rows gathered in that
// order -- and laid out row after row:
//   k_mesh_batch_roots    one row per thread: the domain predicate (aq_domain.h), F(a), F(b), the status word; the
//                         valid rows' roots compacted into level 0, one ballot-aggregated atomic per wave
//   k_mesh_batch_rowkeys  the rows of the l-sorted leaves (the second sort's keys)
//   k_mesh_batch_first    first[i] = the first sorted leaf of row i (a lower bound per row; first[n] = leaves)
//   k_mesh_batch_offsets  one block: offsets = the exclusive scan of nodes_i = 2 leaves_i + (leaves_i > 0)
//   k_mesh_batch_expand   k_mesh_expand's arithmetic, leaf j of row i at node offsets[i] + 2 (j - first[i]) (8-byte
//                         stores: a row at an odd offset has no 16-byte aligned pairs); the row's last leaf adds
//                         the closing node; the block's SEGMENTED double-double sum: (sum since the last row head,
//                         has a head)
//   k_mesh_batch_scan_parts  one block: exclusive segmented scan of the block partials, in place
//   k_mesh_batch_cum      the parked terms back, segmented block scan, cum as k_mesh_cum writes it -- every row's
//                         prefix starts at 0 and adds that row's terms alone
//   k_mesh_batch_finish   one row per thread: area = the row's last cum (NaN without nodes), accepted, tasks
// The scan's tree depends on the rows' leaf counts alone (they fix every head's lane and block), so cum is
// bit-identical from run to run.
// ------------------------------------------------------------------------------------------------
template <int FID>
__global__ __launch_bounds__(256) void k_mesh_batch_roots(const double* __restrict__ a, const double* __restrict__ b,
                                                          const double* __restrict__ theta, unsigned n,
                                                          Rec* __restrict__ out, unsigned* __restrict__ row_out,
                                                          unsigned* __restrict__ count0, unsigned* __restrict__ status,
                                                          unsigned long long* __restrict__ invalid,
                                                          const ExpPair* __restrict__ gtab) {
    __shared__ ExpEntry tab[ftab_entries<FID>()];
    stage_f_table<FID>(tab, gtab);
    __syncthreads();
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    bool ok = false;
    Rec rc{0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const double x = a[i], y = b[i];
        Theta<FID> th{};
        if constexpr (FID == F_PARAM) {
            constexpr int NP = param::nparams;
            double t[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) t[j] = theta[(size_t)i * NP + j];
            ok = params_ok(x, y, t);
#pragma unroll
            for (int j = 0; j < NP; ++j) th.v[j] = t[j];
        } else {
            ok = bounds_ok(FID, x, y);
        }
        status[i] = ok ? 0u : (unsigned)AQ_ROW_INVALID;
        if (ok) rc = Rec{x, y, integrand<FID>(x, tab, th), integrand<FID>(y, tab, th)};
    }
    const unsigned long long m = __ballot(ok), bad = __ballot(i < n && !ok);
    unsigned base = 0;
    if (lane_id() == 0) {
        if (m != 0ull) base = atomicAdd(count0, (unsigned)__popcll(m));
        if (bad != 0ull) atomicAdd(invalid, (unsigned long long)__popcll(bad));
    }
    base = __shfl(base, 0, 64);
    if (ok) {
        const unsigned pos = base + mbcnt(m);   // < n <= the frontier's capacity
        out[pos] = rc;
        row_out[pos] = i;
    }
}

__global__ __launch_bounds__(MESH_T) void k_mesh_batch_rowkeys(const Leaf* __restrict__ leaves,
                                                               const unsigned* __restrict__ idx, unsigned n,
                                                               unsigned* __restrict__ keys) {
    const unsigned j = blockIdx.x * MESH_T + threadIdx.x;
    if (j < n) keys[j] = (unsigned)(leaves[idx[j]].depth >> 32);
}

__global__ __launch_bounds__(MESH_T) void k_mesh_batch_first(const Leaf* __restrict__ leaves,
                                                             const unsigned* __restrict__ idx, unsigned n_leaves,
                                                             unsigned n_rows, unsigned* __restrict__ first) {
    const unsigned i = blockIdx.x * MESH_T + threadIdx.x;
    if (i > n_rows) return;
    unsigned lo = 0, hi = n_leaves;   // the first leaf whose row is >= i
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if ((unsigned)(leaves[idx[mid]].depth >> 32) < i) lo = mid + 1;
        else hi = mid;
    }
    first[i] = lo;
}

__global__ __launch_bounds__(MESH_T) void k_mesh_batch_offsets(const unsigned* __restrict__ first, unsigned n_rows,
                                                               unsigned long long* __restrict__ offsets) {
    __shared__ unsigned long long s_sum[MESH_T];
    const unsigned per = (n_rows + MESH_T - 1) / MESH_T;
    const unsigned r0 = min(threadIdx.x * per, n_rows), r1 = min(r0 + per, n_rows);
    unsigned long long sum = 0;
    for (unsigned i = r0; i < r1; ++i) {
        const unsigned lv = first[i + 1] - first[i];
        sum += 2ull * lv + (lv ? 1ull : 0ull);
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    unsigned long long pre = 0;
    for (unsigned t = 0; t < threadIdx.x; ++t) pre += s_sum[t];
    for (unsigned i = r0; i < r1; ++i) {
        const unsigned lv = first[i + 1] - first[i];
        offsets[i] = pre;
        pre += 2ull * lv + (lv ? 1ull : 0ull);
    }
    if (threadIdx.x == MESH_T - 1) offsets[n_rows] = pre;   // (the last share ends at n_rows, empty or not)
}

// mesh_block_scan with head flags: an inclusive scan of (value, flag) under (v1, f1) + (v2, f2) = (f2 ? v2 : v1 + v2,
// f1 | f2) -- a lane's result is the double-double sum from the last head at or before it (or from the block's first
// lane), its flag whether the block has such a head; `tot` receives the block's pair.
__device__ __forceinline__ void mesh_block_scan_seg(double& hi, double& lo, bool& flag, double& tot_hi, double& tot_lo,
                                                    bool& tot_flag) {
    __shared__ double s_h[MESH_NW], s_l[MESH_NW];
    __shared__ unsigned s_f[MESH_NW];
    const unsigned lane = lane_id(), w = threadIdx.x >> 6;
    unsigned fl = flag ? 1u : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double h2 = __shfl_up(hi, o, 64), l2 = __shfl_up(lo, o, 64);
        const unsigned f2 = __shfl_up(fl, o, 64);
        if (lane >= (unsigned)o) {
            if (!fl) dd_add_dd(hi, lo, h2, l2);
            fl |= f2;
        }
    }
    if (lane == 63) { s_h[w] = hi; s_l[w] = lo; s_f[w] = fl; }
    __syncthreads();
    double ph = 0.0, pl = 0.0;   // the waves before this one, in order
    unsigned pf = 0u, tf = 0u;
    tot_hi = 0.0; tot_lo = 0.0;
    for (unsigned v = 0; v < (unsigned)MESH_NW; ++v) {
        if (v == w) { ph = tot_hi; pl = tot_lo; pf = tf; }
        if (s_f[v]) { tot_hi = s_h[v]; tot_lo = s_l[v]; }
        else dd_add_dd(tot_hi, tot_lo, s_h[v], s_l[v]);
        tf |= s_f[v];
    }
    if (!fl) {
        dd_add_dd(ph, pl, hi, lo);
        hi = ph; lo = pl;
    }
    flag = (fl | pf) != 0u;
    tot_flag = tf != 0u;
    __syncthreads();   // s_h / s_l / s_f may be written again
}

constexpr unsigned MESH_HEAD = 0x80000000u;   // node word of a sorted leaf: its first node (< 2^31) | its row's head bit

__global__ __launch_bounds__(MESH_T) void k_mesh_batch_expand(const Leaf* __restrict__ leaves,
                                                              const unsigned* __restrict__ idx, unsigned n,
                                                              const unsigned* __restrict__ first,
                                                              const unsigned long long* __restrict__ offsets,
                                                              double* __restrict__ x, double* __restrict__ f,
                                                              double* __restrict__ cum, unsigned char* __restrict__ level,
                                                              unsigned* __restrict__ node_of, double2* __restrict__ parts,
                                                              unsigned* __restrict__ pflag) {
    const unsigned j = blockIdx.x * MESH_T + threadIdx.x;
    double hi = 0.0, lo = 0.0;
    bool head = false;
    if (j < n) {
        const Leaf lf = leaves[idx[j]];
        const unsigned row = (unsigned)(lf.depth >> 32);
        const unsigned jr = j - first[row];
        const size_t k = (size_t)offsets[row] + 2 * (size_t)jr;
        head = jr == 0;
        const double mid = (lf.l + lf.r) / 2;                          // :187
        const double larea = (lf.fl + lf.fmid) * (mid - lf.l) / 2;     // :189
        const double rarea = (lf.fmid + lf.fr) * (lf.r - mid) / 2;     // :190
        hi = larea + rarea;                                            // :199
        x[k] = lf.l; x[k + 1] = mid;
        f[k] = lf.fl; f[k + 1] = lf.fmid;
        cum[k] = hi; cum[k + 1] = larea;
        if (level) {
            level[k] = (unsigned char)lf.depth;
            level[k + 1] = (unsigned char)lf.depth;
        }
        if (j + 1 == first[row + 1]) {   // the row's closing node (its cum: k_mesh_batch_cum)
            x[k + 2] = lf.r;
            f[k + 2] = lf.fr;
        }
        node_of[j] = (unsigned)k | (head ? MESH_HEAD : 0u);
    }
    double th, tl;
    bool tf;
    mesh_block_scan_seg(hi, lo, head, th, tl, tf);
    if (threadIdx.x == 0) {
        parts[blockIdx.x] = make_double2(th, tl);
        pflag[blockIdx.x] = tf ? 1u : 0u;
    }
}

__global__ __launch_bounds__(MESH_T) void k_mesh_batch_scan_parts(double2* __restrict__ parts,
                                                                  const unsigned* __restrict__ pflag, unsigned nparts) {
    // thread t owns the contiguous share [t * per, (t + 1) * per)
    const unsigned per = (nparts + MESH_T - 1) / MESH_T;
    const unsigned b0 = min(threadIdx.x * per, nparts), b1 = min(b0 + per, nparts);
    double hi = 0.0, lo = 0.0;
    bool fl = false;
    for (unsigned i = b0; i < b1; ++i) {
        const double2 p = parts[i];
        if (pflag[i]) { hi = p.x; lo = p.y; fl = true; }
        else dd_add_dd(hi, lo, p.x, p.y);
    }
    double th, tl;
    bool tf;
    mesh_block_scan_seg(hi, lo, fl, th, tl, tf);
    // the share's carry-in is the inclusive pair of the thread before (nothing is subtracted)
    __shared__ double s_eh[MESH_T], s_el[MESH_T];
    s_eh[threadIdx.x] = hi; s_el[threadIdx.x] = lo;
    __syncthreads();
    double eh = 0.0, el = 0.0;
    if (threadIdx.x > 0) { eh = s_eh[threadIdx.x - 1]; el = s_el[threadIdx.x - 1]; }
    for (unsigned i = b0; i < b1; ++i) {
        const double2 p = parts[i];
        parts[i] = make_double2(eh, el);   // the sum since the last head before block i
        if (pflag[i]) { eh = p.x; el = p.y; }
        else dd_add_dd(eh, el, p.x, p.y);
    }
}

__global__ __launch_bounds__(MESH_T) void k_mesh_batch_cum(unsigned n, const unsigned* __restrict__ node_of,
                                                           double* __restrict__ cum, const double2* __restrict__ parts) {
    const unsigned j = blockIdx.x * MESH_T + threadIdx.x;
    double area = 0.0, larea = 0.0;
    size_t k = 0;
    bool head = false, last = false;
    if (j < n) {
        const unsigned w = node_of[j];
        k = (size_t)(w & ~MESH_HEAD);
        head = (w & MESH_HEAD) != 0u;
        last = j + 1 == n || (node_of[j + 1] & MESH_HEAD) != 0u;
        area = cum[k]; larea = cum[k + 1];
    }
    double hi = area, lo = 0.0, th, tl;
    bool fl = head, tf;
    mesh_block_scan_seg(hi, lo, fl, th, tl, tf);
    const double2 base = parts[blockIdx.x];
    // P_{j+1} within the row: this block's segment sum, behind the blocks before where no head precedes the lane
    double ih = hi, il = lo;
    if (!fl) {
        ih = base.x; il = base.y;
        dd_add_dd(ih, il, hi, lo);
    }
    __shared__ double s_ih[MESH_T], s_il[MESH_T];   // every lane's inclusive prefix, for the lane after it
    s_ih[threadIdx.x] = ih; s_il[threadIdx.x] = il;
    __syncthreads();
    if (j >= n) return;
    // P_j: 0 at a row's head, else the inclusive prefix of the lane before (the block's first lane: the base alone)
    double ph = 0.0, pl = 0.0;
    if (!head) {
        if (threadIdx.x > 0) { ph = s_ih[threadIdx.x - 1]; pl = s_il[threadIdx.x - 1]; }
        else { ph = base.x; pl = base.y; }
    }
    double mh = ph, ml = pl;
    dd_add_dd(mh, ml, larea, 0.0);
    cum[k] = ph + pl;
    cum[k + 1] = mh + ml;
    if (last) cum[k + 2] = ih + il;
}

__global__ __launch_bounds__(MESH_T) void k_mesh_batch_finish(unsigned n_rows, const unsigned* __restrict__ first,
                                                              const unsigned long long* __restrict__ offsets,
                                                              const double* __restrict__ cum, double* __restrict__ area,
                                                              unsigned long long* __restrict__ accepted,
                                                              unsigned long long* __restrict__ tasks) {
    const unsigned i = blockIdx.x * MESH_T + threadIdx.x;
    if (i >= n_rows) return;
    const unsigned long long lv = first[i + 1] - first[i];
    if (area) area[i] = lv ? cum[offsets[i + 1] - 1] : __longlong_as_double(0x7ff8000000000000ll);
    if (accepted) accepted[i] = lv;
    if (tasks) tasks[i] = lv ? 2 * lv - 1 : 0ull;
}

// ------------------------------------------------------------------------------------------------
// Mesh refinement (aq_mesh_refine_batch): a batch mesh continued to a smaller eps. A mesh keeps, bit for bit, what
// the task step computed for every accepted task -- l, mid, r, F(l), F(mid), F(r), its depth -- so the test is
// redone and the two children are formed without one evaluation of F:
//   k_mesh_refine_rows      one row per thread: status = 0, or AQ_ROW_INVALID for a row without nodes (counted)
//   k_mesh_refine_classify  one node per thread; the even nodes before a row's last are its leaves. A leaf of an
//                           active row that fails :191 at the new eps is counted by depth (LDS histogram, one global
//                           atomic per non-empty bin and block); every other leaf goes to the leaf buffer as
//                           k_level_step emits one (wave ballots, one atomic per block; past the capacity: counted)
//   k_mesh_refine_seed      the same pass again, once the host has seen the counts: the failing leaves' children
//                           into the seed buffer, one segment per depth (the exclusive prefix of the counts), the
//                           row beside each record; positions from a block-local count and one atomic per bin
//   k_mesh_refine_append    before the level step of depth d: segment d behind the children the step of depth
//                           d - 1 appended, one atomic on counts[d] per block of 1024 records
// Then k_level_step<FID, BatchSink> walks on and the back half of aq_integrate_mesh_batch sorts by (row, l).
// The depth table `tab` (unsigned words): [0, AQ_MAX_LEVELS) failing leaves by depth, [AQ_MAX_LEVELS, 2 AQ_MAX_LEVELS)
// the seed pass's cursors, then the leaves that fail at max_depth, the deepest input leaf + 1, the error bits.
// ------------------------------------------------------------------------------------------------
constexpr int REFINE_T = 256;
constexpr int REFINE_TAB_CURSOR = AQ_MAX_LEVELS, REFINE_TAB_DEPTHFAIL = 2 * AQ_MAX_LEVELS,
              REFINE_TAB_LEVELS = 2 * AQ_MAX_LEVELS + 1, REFINE_TAB_ERR = 2 * AQ_MAX_LEVELS + 2,
              REFINE_TAB_WORDS = 2 * AQ_MAX_LEVELS + 4;
constexpr unsigned REFINE_APPEND = 1024;   // records per block of k_mesh_refine_append

struct RefineIn {   // the input mesh and what it is retested with
    const unsigned long long* off;
    const double* x;
    const double* f;
    const unsigned char* level;
    const unsigned char* active;   // null: every row
    unsigned n_rows;
    unsigned long long n_nodes;    // off[n_rows], read by the host
    double eps;
    int max_depth;
};

__global__ __launch_bounds__(REFINE_T) void k_mesh_refine_rows(const unsigned long long* __restrict__ off, unsigned n_rows,
                                                                unsigned* __restrict__ status,
                                                                unsigned long long* __restrict__ invalid) {
    const unsigned i = blockIdx.x * REFINE_T + threadIdx.x;
    const bool in = i < n_rows;
    const bool empty = in && off[i + 1] == off[i];
    if (in) status[i] = empty ? (unsigned)AQ_ROW_INVALID : 0u;
    const unsigned long long bad = __ballot(empty);
    if (lane_id() == 0 && bad != 0ull) atomicAdd(invalid, (unsigned long long)__popcll(bad));
}

// Node k of the input: false unless it is the first node of a leaf. Otherwise the leaf as k_level_step emits one
// and whether it fails the test at in.eps (an inactive row's never does).
__device__ __forceinline__ bool mesh_refine_leaf(const RefineIn& in, unsigned long long k, Leaf& lf, unsigned& row,
                                                 unsigned& depth, bool& fail) {
    if (k + 2 >= in.n_nodes) return false;
    unsigned lo = 0, hi = in.n_rows - 1;   // the last row that starts at or before k (rows without nodes start where
    while (lo < hi) {                      // the next one does, so it has nodes)
        const unsigned m = lo + (hi - lo + 1) / 2;
        if (in.off[m] <= k) lo = m;
        else hi = m - 1;
    }
    const unsigned long long o0 = in.off[lo], o1 = in.off[lo + 1];
    if (k < o0 || ((k - o0) & 1ull) != 0ull || k + 2 >= o1) return false;
    row = lo;
    depth = in.level[k];
    const double mid = in.x[k + 1];
    lf = Leaf{in.x[k], in.x[k + 2], in.f[k], in.f[k + 1], in.f[k + 2], (unsigned long long)depth | ((unsigned long long)lo << 32)};
    const double lrarea = (lf.fl + lf.fr) * (lf.r - lf.l) / 2;       // :185
    const double larea = (lf.fl + lf.fmid) * (mid - lf.l) / 2;       // :189
    const double rarea = (lf.fmid + lf.fr) * (lf.r - mid) / 2;       // :190
    fail = (!in.active || in.active[lo] != 0) && fabs((larea + rarea) - lrarea) > in.eps;   // :191
    return true;
}

__global__ __launch_bounds__(REFINE_T) void k_mesh_refine_classify(RefineIn in, LeafSink sink, unsigned* __restrict__ status,
                                                                    unsigned* __restrict__ tab) {
    __shared__ unsigned s_hist[AQ_MAX_LEVELS];
    __shared__ unsigned s_wl[REFINE_T / 64], s_deep, s_levels;
    __shared__ unsigned long long s_lbase;
    if (threadIdx.x < AQ_MAX_LEVELS) s_hist[threadIdx.x] = 0u;
    if (threadIdx.x == 0) { s_deep = 0u; s_levels = 0u; }
    __syncthreads();
    const unsigned long long k = (unsigned long long)blockIdx.x * REFINE_T + threadIdx.x;
    Leaf lf{};
    unsigned row = 0, depth = 0;
    bool fail = false;
    const bool leaf = mesh_refine_leaf(in, k, lf, row, depth, fail);
    const bool keep = leaf && !fail;
    if (leaf) {
        atomicMax(&s_levels, depth + 1u);
        if (fail) {
            if ((int)depth + 1 >= in.max_depth) {   // (so a counted depth is below AQ_MAX_LEVELS - 2)
                atomicOr(&status[row], (unsigned)AQ_ROW_DEPTH);
                atomicAdd(&s_deep, 1u);
            } else {
                atomicAdd(&s_hist[depth], 1u);
            }
        }
    }
    const unsigned long long mk = __ballot(keep);
    const unsigned w = threadIdx.x >> 6;
    if (lane_id() == 0) s_wl[w] = (unsigned)__popcll(mk);
    __syncthreads();
    if (threadIdx.x == 0) {   // one atomic for the block's leaves (64-bit: the count goes on past the capacity)
        unsigned tot = 0;
        for (int v = 0; v < REFINE_T / 64; ++v) tot += s_wl[v];
        s_lbase = tot ? atomicAdd(sink.count, (unsigned long long)tot) : 0ull;
        if (s_deep) atomicAdd(&tab[REFINE_TAB_DEPTHFAIL], s_deep);
        if (s_levels) atomicMax(&tab[REFINE_TAB_LEVELS], s_levels);
    }
    if (threadIdx.x < AQ_MAX_LEVELS && s_hist[threadIdx.x]) atomicAdd(&tab[threadIdx.x], s_hist[threadIdx.x]);
    __syncthreads();
    if (keep) {
        unsigned long long pos = s_lbase + mbcnt(mk);
        for (unsigned v = 0; v < w; ++v) pos += s_wl[v];
        if (pos < sink.cap) sink.buf[pos] = lf;
    }
}

__global__ __launch_bounds__(REFINE_T) void k_mesh_refine_seed(RefineIn in, unsigned* __restrict__ tab, Rec* __restrict__ seed,
                                                                unsigned* __restrict__ seed_row, unsigned long long seed_cap) {
    __shared__ unsigned s_hist[AQ_MAX_LEVELS], s_base[AQ_MAX_LEVELS], s_seg[AQ_MAX_LEVELS];
    if (threadIdx.x < AQ_MAX_LEVELS) s_hist[threadIdx.x] = 0u;
    if (threadIdx.x == REFINE_T - 1) {   // the segments: the exclusive prefix of the counts
        unsigned pre = 0;
        for (int d = 0; d < AQ_MAX_LEVELS; ++d) { s_seg[d] = pre; pre += tab[d]; }
    }
    __syncthreads();
    const unsigned long long k = (unsigned long long)blockIdx.x * REFINE_T + threadIdx.x;
    Leaf lf{};
    unsigned row = 0, depth = 0, rank = 0;
    bool fail = false;
    const bool seeds = mesh_refine_leaf(in, k, lf, row, depth, fail) && fail && (int)depth + 1 < in.max_depth;
    if (seeds) rank = atomicAdd(&s_hist[depth], 1u);
    __syncthreads();
    if (threadIdx.x < AQ_MAX_LEVELS && s_hist[threadIdx.x])
        s_base[threadIdx.x] = atomicAdd(&tab[REFINE_TAB_CURSOR + threadIdx.x], s_hist[threadIdx.x]);
    __syncthreads();
    if (seeds) {
        const unsigned long long p = 2ull * ((unsigned long long)s_seg[depth] + s_base[depth] + rank);
        if (p + 1 < seed_cap) {   // (always, for an input that did not change between the two passes)
            const double mid = in.x[k + 1];
            seed[p] = Rec{lf.l, mid, lf.fl, lf.fmid};       // [l, mid]  (:192-194)
            seed[p + 1] = Rec{mid, lf.r, lf.fmid, lf.fr};   // [mid, r]  (:195-197)
            seed_row[p] = row;
            seed_row[p + 1] = row;
        }
    }
}

__global__ __launch_bounds__(256) void k_mesh_refine_append(const Rec* __restrict__ seed, const unsigned* __restrict__ seed_row,
                                                            unsigned n, Rec* __restrict__ out, unsigned* __restrict__ row_out,
                                                            unsigned* __restrict__ count, unsigned cap,
                                                            unsigned* __restrict__ err) {
    __shared__ unsigned s_base;
    const unsigned first = blockIdx.x * REFINE_APPEND;
    if (threadIdx.x == 0) s_base = atomicAdd(count, min(REFINE_APPEND, n - first));
    __syncthreads();
    bool over = false;
    for (unsigned i = first + threadIdx.x; i < min(first + REFINE_APPEND, n); i += 256u) {
        const unsigned pos = s_base + (i - first);
        if (pos < cap && pos >= s_base) {
            out[pos] = seed[i];
            row_out[pos] = seed_row[i];
        } else {
            over = true;
        }
    }
    if (over) atomicOr(err, (unsigned)ERRB_OVERFLOW);
}

// aq_mesh_err_batch: per row Σ|d| and Σd over its leaves, d = (larea + rarea) - lrarea recomputed from the nodes
// (:185-191), carried in double-double. The reduction's shape is fixed by the row's own leaf count: block (i, b) of
// MESH_ERR_B takes the row's chunks of MESH_T leaves c = b, b + MESH_ERR_B, ... from the ROW's first leaf -- a thread
// its leaves in order, the wave's lanes a butterfly, the waves in order -- and k_mesh_err_finish adds a row's
// partials in block order and rounds once. So a row's sums are the same bits in any batch, at any offset.
constexpr int MESH_ERR_B = 8;
__global__ __launch_bounds__(MESH_T) void k_mesh_err_parts(const unsigned long long* __restrict__ off,
                                                           const double* __restrict__ x, const double* __restrict__ f,
                                                           double4* __restrict__ parts) {
    __shared__ double s_v[MESH_NW][4];
    const unsigned row = blockIdx.x / MESH_ERR_B, b = blockIdx.x % MESH_ERR_B;
    const unsigned long long o0 = off[row], o1 = off[row + 1];
    const unsigned long long nn = o1 > o0 ? o1 - o0 : 0ull, leaves = nn >= 3 ? (nn - 1) / 2 : 0ull;
    double ah = 0.0, al = 0.0, sh = 0.0, sl = 0.0;
    for (unsigned long long j = (unsigned long long)b * MESH_T + threadIdx.x; j < leaves;
         j += (unsigned long long)MESH_ERR_B * MESH_T) {
        const double* xs = x + o0 + 2 * j;
        const double* fs = f + o0 + 2 * j;
        const double l = xs[0], mid = xs[1], r = xs[2], fl = fs[0], fmid = fs[1], fr = fs[2];
        const double lrarea = (fl + fr) * (r - l) / 2;       // :185
        const double larea = (fl + fmid) * (mid - l) / 2;    // :189
        const double rarea = (fmid + fr) * (r - mid) / 2;    // :190
        const double d = (larea + rarea) - lrarea;           // :191
        dd_add(ah, al, fabs(d));
        dd_add(sh, sl, d);
    }
    wave_sum_dd(ah, al);
    wave_sum_dd(sh, sl);
    const unsigned w = threadIdx.x >> 6;
    if (lane_id() == 0) { s_v[w][0] = ah; s_v[w][1] = al; s_v[w][2] = sh; s_v[w][3] = sl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double AH = 0.0, AL = 0.0, SH = 0.0, SL = 0.0;
        for (int v = 0; v < MESH_NW; ++v) {
            dd_add_dd(AH, AL, s_v[v][0], s_v[v][1]);
            dd_add_dd(SH, SL, s_v[v][2], s_v[v][3]);
        }
        parts[blockIdx.x] = make_double4(AH, AL, SH, SL);
    }
}

__global__ __launch_bounds__(MESH_T) void k_mesh_err_finish(const unsigned long long* __restrict__ off, unsigned n_rows,
                                                            const double4* __restrict__ parts, double* __restrict__ err_abs,
                                                            double* __restrict__ err_signed) {
    const unsigned i = blockIdx.x * MESH_T + threadIdx.x;
    if (i >= n_rows) return;
    double AH = 0.0, AL = 0.0, SH = 0.0, SL = 0.0;
    for (int b = 0; b < MESH_ERR_B; ++b) {
        const double4 p = parts[(size_t)i * MESH_ERR_B + b];
        dd_add_dd(AH, AL, p.x, p.y);
        dd_add_dd(SH, SL, p.z, p.w);
    }
    const bool none = off[i + 1] < off[i] + 3;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (err_abs) err_abs[i] = none ? nan : AH + AL;
    if (err_signed) err_signed[i] = none ? nan : SH + SL;
}

// aq_mesh_moments_batch: per row M_k = the integral over [lo, hi] of (x - c)^k times the piecewise-linear function
// through the row's nodes, k = 0 .. K, every panel's term the sequence include/aquad.h states (one IEEE operation
// per line), carried in double-double. The arrangement is k_mesh_err_*'s: block (i, b) of MESH_MOM_B takes the row's
// chunks of MESH_T leaves b, b + MESH_MOM_B, ... from the ROW's first leaf, skipping the chunks before the leaf that
// holds lo and after the one that holds hi; a thread adds the two panels of its leaf in order, the wave's lanes
// meet in a butterfly, the waves in order, and k_mesh_moments_finish adds a row's partials in block order and
// rounds once. The shape depends on the row's leaf count and the two panel indices alone. The row's range is found
// by ONE thread per block (two searches of the row's x, side by side) and handed to the others through LDS; a block
// without a chunk in the range -- b * MESH_T >= the row's leaves, most blocks of a batch of small rows -- writes
// (0, 0), the sum of no terms, and leaves before any search, barrier or butterfly.
constexpr int MESH_MOM_B = 8;
enum : int { MOM_NAN = 0, MOM_ZERO = 1, MOM_SUM = 2 };
struct MomRange {
    double c, lo, hi, flo, fhi;       // the centre, the range and the interpolant at an end inside a panel
    unsigned long long kl, kh;        // the panels that hold lo and hi
    int state;
    bool lo_node, hi_node;            // the end is a node: its stored f
};

// what a row's outputs are: NaN (fewer than 3 nodes, or not x_0 <= lo <= hi <= x_m: NaN fails every comparison), +0.0
// (lo == hi: no panel is touched), or a sum
__device__ __forceinline__ int mesh_mom_state(double x0, double xm, double lo, double hi) {
    if (!(x0 <= lo && lo <= hi && hi <= xm)) return MOM_NAN;
    return lo == hi ? MOM_ZERO : MOM_SUM;
}

// one panel's terms t_0 .. t_K into the accumulators: include/aquad.h's sequence, line for line
template <int K>
__device__ __forceinline__ void mesh_mom_panel(double x0, double x1, double g0, double g1, double c, double (&ah)[K + 1],
                                               double (&al)[K + 1]) {
    const double u0 = x0 - c;
    const double u1 = x1 - c;
    const double w = x1 - x0;
    double p0[K + 1], p1[K + 1];
    p0[0] = 1.0;
    p1[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= K; ++i) {
        p0[i] = p0[i - 1] * u0;
        p1[i] = p1[i - 1] * u1;
    }
#pragma unroll
    for (int k = 0; k <= K; ++k) {
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int j = 0; j <= k; ++j) {
            const double a = p0[k - j] * p1[j];
            s0 = s0 + (double)(k + 1 - j) * a;
            s1 = s1 + (double)(j + 1) * a;
        }
        const double t = (g0 * s0 + g1 * s1) * w / (double)((k + 1) * (k + 2));
        dd_add(ah[k], al[k], t);
    }
}

template <int K>
__global__ __launch_bounds__(MESH_T) void k_mesh_moments_parts(const unsigned long long* __restrict__ off,
                                                               const double* __restrict__ x, const double* __restrict__ f,
                                                               const double* __restrict__ center,
                                                               const double* __restrict__ d_lo,
                                                               const double* __restrict__ d_hi,
                                                               double2* __restrict__ parts) {
    __shared__ MomRange s_r;
    __shared__ double s_v[MESH_NW][2 * (K + 1)];
    const unsigned row = blockIdx.x / MESH_MOM_B, b = blockIdx.x % MESH_MOM_B;
    const unsigned long long o0 = off[row], o1 = off[row + 1];
    const unsigned long long nn = o1 > o0 ? o1 - o0 : 0ull, leaves = nn >= 3 ? (nn - 1) / 2 : 0ull;
    const double* xr = x + o0;
    const double* fr = f + o0;
    // a block without a chunk (seven of eight on a row of at most MESH_T leaves) adds nothing: (0, 0), what the
    // reduction of untouched accumulators gives, without the search, the barriers and the butterflies
    if ((unsigned long long)b * MESH_T >= leaves) {
        if ((int)threadIdx.x <= K) parts[(size_t)blockIdx.x * (K + 1) + threadIdx.x] = make_double2(0.0, 0.0);
        return;
    }
    if (threadIdx.x == 0) {
        // (nn >= 3 here: the block has a chunk.) Everything the classification reads, in one round trip; for the
        // row's own ends -- the NULL arrays -- nothing more is loaded before the barrier.
        const unsigned long long m = 2 * leaves;   // panels; the nodes past 2 * leaves (an even count) are not read
        const double x0 = xr[0], xlast = xr[nn - 1], x1 = xr[1], xm1 = xr[m - 1], xm = xr[m];
        const double lo = d_lo ? d_lo[row] : x0, hi = d_hi ? d_hi[row] : xlast;
        s_r.c = center ? center[row] : 0.0;
        const int state = mesh_mom_state(x0, xlast, lo, hi);
        unsigned long long kl = 0, kh = 0;
        bool lo_node = true, hi_node = true;
        if (state == MOM_SUM) {
            // aq_mesh_eval's rule for lo and hi -- the largest k <= m - 1 with x_k <= q, mesh_eval_one's search -- the
            // two searches side by side (their loads overlap); x_1 > lo leaves panel 0 and x_(m-1) <= hi panel m - 1
            // without a step. xkl, xkh: x at the two answers.
            unsigned long long el = x1 > lo ? 0 : m - 1, eh = m - 1;
            kh = xm1 <= hi ? m - 1 : 0;
            double xkl = x0, xkh = kh ? xm1 : x0;
            while (kl < el || kh < eh) {
                const unsigned long long ml = kl + (el - kl + 1) / 2, mh = kh + (eh - kh + 1) / 2;
                const double xl = xr[ml], xh = xr[mh];
                if (kl < el) {
                    if (xl <= lo) { kl = ml; xkl = xl; }
                    else el = ml - 1;
                }
                if (kh < eh) {
                    if (xh <= hi) { kh = mh; xkh = xh; }
                    else eh = mh - 1;
                }
            }
            if (kh > kl && hi == xkh) --kh;          // hi at a node: the panel that ends there, and the node's own f
            else hi_node = kh == m - 1 && hi == xm;  // (else inside panel kh, or at the row's last node)
            lo_node = lo == xkl;
            if (!lo_node || !hi_node) {              // an end inside a panel: aq_mesh_eval's expression on its two nodes
                const double xl = xr[kl], fl = fr[kl], xl1 = xr[kl + 1], fl1 = fr[kl + 1];
                const double xh = xr[kh], fh = fr[kh], xh1 = xr[kh + 1], fh1 = fr[kh + 1];
                s_r.flo = fl + (fl1 - fl) * ((lo - xl) / (xl1 - xl));
                s_r.fhi = fh + (fh1 - fh) * ((hi - xh) / (xh1 - xh));
            }
        }
        s_r.lo = lo;
        s_r.hi = hi;
        s_r.kl = kl;
        s_r.kh = kh;
        s_r.lo_node = lo_node;
        s_r.hi_node = hi_node;
        s_r.state = state;
    }
    __syncthreads();
    const unsigned long long kl = s_r.kl, kh = s_r.kh;
    // the first chunk at or after the one that holds leaf kl / 2, among b, b + MESH_MOM_B, ...
    const unsigned long long c0 = (kl >> 1) / MESH_T;
    const unsigned long long cb = c0 + (b + MESH_MOM_B - (unsigned)(c0 % MESH_MOM_B)) % MESH_MOM_B;
    if (s_r.state != MOM_SUM || cb * MESH_T > (kh >> 1)) {   // a NaN or +0.0 row, or no chunk of this block in the range
        if ((int)threadIdx.x <= K) parts[(size_t)blockIdx.x * (K + 1) + threadIdx.x] = make_double2(0.0, 0.0);
        return;
    }
    double ah[K + 1], al[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) ah[k] = al[k] = 0.0;
    {
        const double c = s_r.c, lo = s_r.lo, hi = s_r.hi, flo = s_r.flo, fhi = s_r.fhi;
        const bool lo_in = !s_r.lo_node, hi_in = !s_r.hi_node;   // an end inside its panel: the interpolated value
        for (unsigned long long j = cb * MESH_T + threadIdx.x; j <= (kh >> 1); j += (unsigned long long)MESH_MOM_B * MESH_T) {
            const double* xs = xr + 2 * j;   // kh <= 2 * leaves - 1: j < leaves
            const double* fs = fr + 2 * j;
            const double l = xs[0], mid = xs[1], r = xs[2], fl = fs[0], fmid = fs[1], fr2 = fs[2];
            const unsigned long long p = 2 * j;
            if (p >= kl && p <= kh)
                mesh_mom_panel<K>(p == kl ? lo : l, p == kh ? hi : mid, p == kl && lo_in ? flo : fl,
                                  p == kh && hi_in ? fhi : fmid, c, ah, al);
            if (p + 1 >= kl && p + 1 <= kh)
                mesh_mom_panel<K>(p + 1 == kl ? lo : mid, p + 1 == kh ? hi : r, p + 1 == kl && lo_in ? flo : fmid,
                                  p + 1 == kh && hi_in ? fhi : fr2, c, ah, al);
        }
    }
    const unsigned w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k <= K; ++k) {
        wave_sum_dd(ah[k], al[k]);
        if (lane_id() == 0) { s_v[w][2 * k] = ah[k]; s_v[w][2 * k + 1] = al[k]; }
    }
    __syncthreads();
    if ((int)threadIdx.x <= K) {   // accumulator k's waves, in order
        double H = 0.0, L = 0.0;
        for (int v = 0; v < MESH_NW; ++v) dd_add_dd(H, L, s_v[v][2 * threadIdx.x], s_v[v][2 * threadIdx.x + 1]);
        parts[(size_t)blockIdx.x * (K + 1) + threadIdx.x] = make_double2(H, L);
    }
}

__global__ __launch_bounds__(MESH_T) void k_mesh_moments_finish(const unsigned long long* __restrict__ off, unsigned n_rows,
                                                                const double* __restrict__ x, int K,
                                                                const double* __restrict__ d_lo,
                                                                const double* __restrict__ d_hi,
                                                                const double2* __restrict__ parts, double* __restrict__ out) {
    const unsigned i = blockIdx.x * MESH_T + threadIdx.x;
    if (i >= n_rows) return;
    const unsigned long long o0 = off[i], o1 = off[i + 1];
    const unsigned long long nn = o1 > o0 ? o1 - o0 : 0ull;
    int state = MOM_NAN;
    if (nn >= 3) {
        const double x0 = x[o0], xm = x[o0 + nn - 1];
        state = mesh_mom_state(x0, xm, d_lo ? d_lo[i] : x0, d_hi ? d_hi[i] : xm);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int k = 0; k <= K; ++k) {
        double H = 0.0, L = 0.0;
        if (state == MOM_SUM)
            for (int b = 0; b < MESH_MOM_B; ++b) {
                const double2 p = parts[((size_t)i * MESH_MOM_B + b) * (K + 1) + k];
                dd_add_dd(H, L, p.x, p.y);
            }
        out[(size_t)i * (K + 1) + k] = state == MOM_NAN ? nan : state == MOM_ZERO ? 0.0 : H + L;
    }
}

// ------------------------------------------------------------------------------------------------
// Mesh coarsening (aq_mesh_thresholds_batch, aq_mesh_budget_batch, aq_mesh_coarsen_batch): the converse of
// refinement. The tree at eps' >= eps is a sub-tree of the tree at eps, and every value its tasks computed is a
// node value of the fine mesh, so any coarser mesh follows from the node arrays alone -- no F, no theta.
// Leaf j of a row (x order, depth lev_j) starts at the position pos_j = sum_{i<j} 2^(127 - lev_i), an exact 128-bit
// integer (the row ends at 2^127). The tree node of depth k over leaf j starts at pos_j with its low 127 - k bits
// cleared; a leaf j >= 1 starts at the midpoint of exactly one internal node N(j), of depth 126 - ctz(pos_j).
//   k_mesh_coarsen_pos    one block per row: the exclusive scan of 2^(127 - lev) over the row's leaves, chunk after
//                         chunk of COARSEN_T (wave shuffles, the waves' totals in LDS, an integer carry: no atomics);
//                         it also writes every leaf's row beside its position
//   k_mesh_coarsen_node   one leaf j >= 1 per thread: N(j)'s start and end by two clamped searches of the row's
//                         positions, |d| = fabs((larea + rarea) - lrarea) from the six node values (the task step's
//                         expressions), and N(j)'s parent: N(il) when N(j) is a right child, else N(ir)
//   k_mesh_coarsen_thr    thr = the minimum of |d| over N(j) and its ancestors (the parent chain, at most
//                         AQ_MAX_LEVELS loads); +inf at a row's two ends, 0 at its odd nodes. x[k] bounds a leaf of
//                         the row's mesh at eps' iff thr[k] > eps'
//   k_mesh_coarsen_emit   a head (the row's first leaf, or thr > the row's eps; every leaf of a row whose eps is
//                         negative or NaN) emits ONE leaf record as k_mesh_refine_classify does: r from the next
//                         head (a forward walk bounded by the row's end), the depth from the position difference,
//                         F(mid) from one search. The back half of aq_integrate_mesh_batch lays the records out.
//   k_mesh_budget_keys / _rowkeys / _pick   the row's max_leaves-th largest threshold: the nodes sorted by (row,
//                         key), key = thr at an even interior node and 0 elsewhere (aq_mesh_sort.hip, two passes)
// A leaf's scratch slot is (its first node) >> 1: a row of L leaves at offset o0 owns the slots [o0 >> 1, (o0 >> 1) + L),
// which no other row's leaf maps to (a row has 2 L + 1 nodes). Every index below is clamped into its row's slice, so
// `level` may hold any bytes.
// ------------------------------------------------------------------------------------------------
constexpr int COARSEN_T = 256;
constexpr int COARSEN_NW = COARSEN_T / 64;

struct U128 {
    unsigned long long lo, hi;
};
__device__ __forceinline__ U128 u128_add(U128 a, U128 b) {
    U128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1ull : 0ull);
    return r;
}
__device__ __forceinline__ U128 u128_sub(U128 a, U128 b) {
    U128 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull);
    return r;
}
__device__ __forceinline__ bool u128_lt(U128 a, U128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ U128 u128_pow2(unsigned e) {   // e <= 127
    return U128{e < 64u ? 1ull << e : 0ull, e >= 64u ? 1ull << (e - 64u) : 0ull};
}
__device__ __forceinline__ U128 u128_half(U128 a) { return U128{(a.lo >> 1) | (a.hi << 63), a.hi >> 1}; }
__device__ __forceinline__ unsigned u128_ctz(U128 a) {   // 128 for 0
    return a.lo ? (unsigned)__ffsll((unsigned long long)a.lo) - 1u : a.hi ? 63u + (unsigned)__ffsll((unsigned long long)a.hi) : 128u;
}
__device__ __forceinline__ unsigned u128_clz(U128 a) {   // 128 for 0
    return a.hi ? (unsigned)__clzll((long long)a.hi) : a.lo ? 64u + (unsigned)__clzll((long long)a.lo) : 128u;
}
__device__ __forceinline__ U128 u128_of(ulonglong2 v) { return U128{v.x, v.y}; }

struct CoarsenIn {   // the input mesh
    const unsigned long long* off;
    const double* x;
    const double* f;
    const unsigned char* level;
    unsigned n_rows;
    unsigned long long n_nodes;    // off[n_rows], read by the host
};

// The leaves of a row of nodes [o0, o1) (none below 3 nodes).
__device__ __forceinline__ unsigned coarsen_leaves(unsigned long long o0, unsigned long long o1) {
    return o1 >= o0 + 3 ? (unsigned)((o1 - o0 - 1) / 2) : 0u;
}

// The first index in [lo, hi) of the row's positions that is not below `key`, or hi.
__device__ __forceinline__ unsigned coarsen_lower_bound(const ulonglong2* __restrict__ p, unsigned lo, unsigned hi, U128 key) {
    while (lo < hi) {
        const unsigned m = lo + (hi - lo) / 2;
        if (u128_lt(u128_of(p[m]), key)) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// Slot s of the scratch arrays: false unless it is a leaf's. Otherwise its row, the row's first node and first slot,
// its leaves, and the leaf's index in the row.
__device__ __forceinline__ bool coarsen_slot(const CoarsenIn& in, const unsigned* __restrict__ rowof, unsigned long long s,
                                             unsigned long long n_slots, unsigned& row, unsigned long long& o0,
                                             unsigned long long& sb, unsigned& L, unsigned& j) {
    if (s >= n_slots) return false;
    row = rowof[s];
    if (row >= in.n_rows) return false;   // 0xffffffff: no leaf's slot (rows are < 2^31)
    o0 = in.off[row];
    L = coarsen_leaves(o0, in.off[row + 1]);
    sb = o0 >> 1;
    if (s < sb || s - sb >= L) return false;
    j = (unsigned)(s - sb);
    return true;
}

__global__ __launch_bounds__(COARSEN_T) void k_mesh_coarsen_pos(CoarsenIn in, ulonglong2* __restrict__ pos,
                                                                 unsigned* __restrict__ rowof) {
    __shared__ U128 s_w[COARSEN_NW];
    const unsigned row = blockIdx.x;
    const unsigned long long o0 = in.off[row], o1 = in.off[row + 1];
    const unsigned L = o1 <= in.n_nodes ? coarsen_leaves(o0, o1) : 0u;
    const unsigned long long sb = o0 >> 1;
    const unsigned lane = lane_id(), w = threadIdx.x >> 6;
    U128 carry{0ull, 0ull};   // the chunks before this one (the same in every thread)
    for (unsigned c = 0; c < L; c += COARSEN_T) {
        const unsigned j = c + threadIdx.x;
        U128 v{0ull, 0ull};
        if (j < L) v = u128_pow2(127u - min((unsigned)in.level[o0 + 2ull * j], 127u));
        U128 inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const U128 up{__shfl_up(inc.lo, o, 64), __shfl_up(inc.hi, o, 64)};
            if (lane >= (unsigned)o) inc = u128_add(inc, up);
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        U128 pre{0ull, 0ull}, tot{0ull, 0ull};   // the waves before this one, in order
        for (unsigned v2 = 0; v2 < (unsigned)COARSEN_NW; ++v2) {
            if (v2 == w) pre = tot;
            tot = u128_add(tot, s_w[v2]);
        }
        if (j < L) {
            const U128 p = u128_add(carry, u128_add(pre, u128_sub(inc, v)));
            pos[sb + j] = make_ulonglong2(p.lo, p.hi);
            rowof[sb + j] = row;
        }
        carry = u128_add(carry, tot);
        __syncthreads();   // s_w is written again
    }
}

__global__ __launch_bounds__(COARSEN_T) void k_mesh_coarsen_node(CoarsenIn in, unsigned long long n_slots,
                                                                  const ulonglong2* __restrict__ pos,
                                                                  const unsigned* __restrict__ rowof,
                                                                  double* __restrict__ dabs, unsigned* __restrict__ par) {
    const unsigned long long s = (unsigned long long)blockIdx.x * COARSEN_T + threadIdx.x;
    unsigned row, L, j;
    unsigned long long o0, sb;
    if (!coarsen_slot(in, rowof, s, n_slots, row, o0, sb, L, j) || j == 0u) return;
    const ulonglong2* rp = pos + sb;
    const U128 p = u128_of(rp[j]);
    const unsigned tz = min(u128_ctz(p), 126u);           // N(j)'s depth is 126 - tz
    const U128 start = u128_sub(p, u128_pow2(tz));        // p with its low tz + 1 bits cleared
    const U128 end = u128_add(start, u128_pow2(tz + 1u));
    const unsigned il = min(coarsen_lower_bound(rp, 0u, j, start), j - 1u);   // < j
    const unsigned ir = coarsen_lower_bound(rp, j + 1u, L, end);              // in (j, L]: L is the row's last node
    const unsigned long long kl = o0 + 2ull * il, km = o0 + 2ull * j, kr = o0 + 2ull * ir;
    const double l = in.x[kl], mid = in.x[km], r = in.x[kr], fl = in.f[kl], fmid = in.f[km], fr = in.f[kr];
    const double lrarea = (fl + fr) * (r - l) / 2;        // :185
    const double larea = (fl + fmid) * (mid - l) / 2;     // :189
    const double rarea = (fmid + fr) * (r - mid) / 2;     // :190
    dabs[s] = fabs((larea + rarea) - lrarea);             // :191
    unsigned q = 0u;                                      // 0: no parent (leaf 0 starts at no node's midpoint)
    if (tz < 126u) {
        const U128 bit = u128_pow2(tz + 1u);              // set in `start`: N(j) is a right child, its parent's mid is `start`
        const bool right = ((start.lo & bit.lo) | (start.hi & bit.hi)) != 0ull;
        q = right ? il : ir;
        if (q >= L || q == j) q = 0u;
    }
    par[s] = q;
}

__global__ __launch_bounds__(COARSEN_T) void k_mesh_coarsen_thr(CoarsenIn in, unsigned long long n_slots,
                                                                 const unsigned* __restrict__ rowof,
                                                                 const double* __restrict__ dabs,
                                                                 const unsigned* __restrict__ par, double* __restrict__ thr) {
    const unsigned long long s = (unsigned long long)blockIdx.x * COARSEN_T + threadIdx.x;
    unsigned row, L, j;
    unsigned long long o0, sb;
    if (!coarsen_slot(in, rowof, s, n_slots, row, o0, sb, L, j)) return;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double t = inf;
    if (j > 0u) {
        t = dabs[s];
        unsigned q = par[s];
        for (int it = 0; it < AQ_MAX_LEVELS && q != 0u; ++it) {
            t = fmin(t, dabs[sb + q]);
            q = par[sb + q];
        }
    }
    const unsigned long long k = o0 + 2ull * j;
    thr[k] = t;
    thr[k + 1] = 0.0;
    if (j + 1u == L) thr[k + 2] = inf;
}

__global__ __launch_bounds__(COARSEN_T) void k_mesh_coarsen_emit(CoarsenIn in, unsigned long long n_slots,
                                                                  const ulonglong2* __restrict__ pos,
                                                                  const unsigned* __restrict__ rowof,
                                                                  const double* __restrict__ thr,
                                                                  const double* __restrict__ row_eps, double eps,
                                                                  LeafSink sink, unsigned* __restrict__ levels) {
    __shared__ unsigned s_wl[COARSEN_NW], s_levels;
    __shared__ unsigned long long s_lbase;
    if (threadIdx.x == 0) s_levels = 0u;
    __syncthreads();
    const unsigned long long s = (unsigned long long)blockIdx.x * COARSEN_T + threadIdx.x;
    unsigned row, L, j;
    unsigned long long o0, sb;
    bool head = false;
    Leaf lf{};
    if (coarsen_slot(in, rowof, s, n_slots, row, o0, sb, L, j)) {
        const double e = row_eps ? row_eps[row] : eps;
        const bool all = !(e >= 0.0);   // negative or NaN: the row is copied
        head = j == 0u || all || thr[o0 + 2ull * j] > e;
        if (head) {
            unsigned jn = j + 1u;       // the next head, or the row's end
            if (!all) while (jn < L && !(thr[o0 + 2ull * jn] > e)) ++jn;
            const ulonglong2* rp = pos + sb;
            const unsigned long long k = o0 + 2ull * j, kn = o0 + 2ull * jn;
            unsigned depth = in.level[k];
            double fmid = in.f[k + 1];
            if (jn > j + 1u) {          // merged: a tree node of 2^(127 - depth) positions, its mid at their half
                const U128 pj = u128_of(rp[j]);
                const U128 width = u128_sub(jn < L ? u128_of(rp[jn]) : u128_pow2(127u), pj);
                depth = min(u128_clz(width), 127u);
                const unsigned jm = min(coarsen_lower_bound(rp, j + 1u, jn, u128_add(pj, u128_half(width))), jn - 1u);
                fmid = in.f[o0 + 2ull * jm];
            }
            lf = Leaf{in.x[k], in.x[kn], in.f[k], fmid, in.f[kn], (unsigned long long)depth | ((unsigned long long)row << 32)};
            atomicMax(&s_levels, depth + 1u);
        }
    }
    const unsigned long long mk = __ballot(head);
    const unsigned w = threadIdx.x >> 6;
    if (lane_id() == 0) s_wl[w] = (unsigned)__popcll(mk);
    __syncthreads();
    if (threadIdx.x == 0) {   // one atomic for the block's leaves (64-bit: the count goes on past the capacity)
        unsigned tot = 0;
        for (int v = 0; v < COARSEN_NW; ++v) tot += s_wl[v];
        s_lbase = tot ? atomicAdd(sink.count, (unsigned long long)tot) : 0ull;
        if (s_levels) atomicMax(levels, s_levels);
    }
    __syncthreads();
    if (head) {
        unsigned long long p = s_lbase + mbcnt(mk);
        for (unsigned v = 0; v < w; ++v) p += s_wl[v];
        if (p < sink.cap) sink.buf[p] = lf;
    }
}

// Node k's row: the last row that starts at or before k (rows without nodes start where the next one does).
__device__ __forceinline__ unsigned coarsen_row_of(const unsigned long long* __restrict__ off, unsigned n_rows,
                                                   unsigned long long k) {
    unsigned lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const unsigned m = lo + (hi - lo + 1) / 2;
        if (off[m] <= k) lo = m;
        else hi = m - 1;
    }
    return lo;
}

__global__ __launch_bounds__(COARSEN_T) void k_mesh_budget_keys(const unsigned long long* __restrict__ off, unsigned n_rows,
                                                                 unsigned long long n_nodes, const double* __restrict__ thr,
                                                                 double* __restrict__ keys, unsigned* __restrict__ idx,
                                                                 unsigned* __restrict__ row_of) {
    const unsigned long long k = (unsigned long long)blockIdx.x * COARSEN_T + threadIdx.x;
    if (k >= n_nodes) return;
    const unsigned row = coarsen_row_of(off, n_rows, k);
    const unsigned long long o0 = off[row], o1 = off[row + 1];
    const bool interior = k > o0 && k + 1 < o1 && ((k - o0) & 1ull) == 0ull;
    keys[k] = interior ? thr[k] : 0.0;
    idx[k] = (unsigned)k;
    row_of[k] = row;
}

__global__ __launch_bounds__(COARSEN_T) void k_mesh_budget_rowkeys(const unsigned* __restrict__ row_of,
                                                                    const unsigned* __restrict__ idx, unsigned long long n_nodes,
                                                                    unsigned* __restrict__ keys) {
    const unsigned long long j = (unsigned long long)blockIdx.x * COARSEN_T + threadIdx.x;
    if (j < n_nodes) keys[j] = row_of[min((unsigned long long)idx[j], n_nodes - 1)];
}

// One row per thread: the nodes of row i, sorted by (row, key), are [off[i], off[i + 1]) of idx.
__global__ __launch_bounds__(COARSEN_T) void k_mesh_budget_pick(const unsigned long long* __restrict__ off, unsigned n_rows,
                                                                 unsigned long long n_nodes, const double* __restrict__ thr,
                                                                 const unsigned* __restrict__ idx, unsigned long long max_leaves,
                                                                 double* __restrict__ eps) {
    const unsigned i = blockIdx.x * COARSEN_T + threadIdx.x;
    if (i >= n_rows) return;
    const unsigned long long o0 = off[i], o1 = off[i + 1];
    const unsigned long long L = o1 <= n_nodes ? coarsen_leaves(o0, o1) : 0u;
    double e = -1.0;
    if (L > max_leaves) e = thr[min((unsigned long long)idx[o1 - max_leaves], n_nodes - 1)];   // L - 1 >= max_leaves keys are thresholds
    eps[i] = e;
}

// Gather n slots' totals into a caller device buffer as f64 [area, tasks, accepted, error] rows,
// ready for one collective (counts are exact in f64 below 2^53). One thread per slot: the area is
// the correctly rounded value of the slot's exact accumulator.
__global__ __launch_bounds__(64) void k_gather(const Ctl* __restrict__ ctls, const unsigned long long* __restrict__ parts,
                                               int grid, int first, int n, int nslots, double* __restrict__ out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int slot = (first + i) % nslots;
    const Ctl& c = ctls[slot];
    const Counts k = slot_counts(c.sums, parts + 2 * parts_row(slot) * grid, grid);
    double* o = out + 4 * (size_t)i;
    o[0] = xs_round(c.area);
    o[1] = (double)k.tasks;
    o[2] = (double)k.leaves;
    o[3] = (double)c.sums.error;
}

// The batch front end's gather (aq_integrate_batch): k_gather's rows, then every slot back to the
// all-zero state the next launch needs -- its sums and the limbs of its window, the only ones any flush
// added to (SlotSums win_lo_not / win_hi) -- so no k_reset runs before the next chunk's launch on the
// same slots, and only a slot's touched lines are read and written (k_gather + k_reset read and wrote
// all 68 limbs of every slot: 115 + 76 us per 262144-slot chunk, profiles/r05a/c3_timeline_r04code.json).
constexpr int GATHER_WIN = 16;   // limbs a window may span to take the short path (a cosh4 tree: ~4-6)
// perm (size-ordered batch chunks): slot i holds integral perm[i], whose row it writes.
__global__ __launch_bounds__(64) void k_gather_reset(Ctl* __restrict__ ctls, const unsigned long long* __restrict__ parts,
                                                     int grid, int first, int n, double* __restrict__ out,
                                                     const unsigned* __restrict__ perm) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int slot = first + i;
    Ctl& c = ctls[slot];
    const SlotSums sm = c.sums;
    const Counts k = slot_counts(sm, parts + 2 * parts_row(slot) * grid, grid);
    const int lo = sm.win_hi ? (int)~sm.win_lo_not : 0;
    const int hi = sm.win_hi ? min((int)sm.win_hi, XS_LIMBS) : 0;
    double area;
    if (hi - lo <= GATHER_WIN) {
        long long w[GATHER_WIN];
#pragma unroll
        for (int j = 0; j < GATHER_WIN; ++j) w[j] = lo + j < hi ? c.area.limb[lo + j] : 0ll;
        area = xs_round_span<GATHER_WIN>(w, hi - lo, XS_E0 + 32 * lo);
#pragma unroll
        for (int j = 0; j < GATHER_WIN; ++j)
            if (lo + j < hi) c.area.limb[lo + j] = 0ll;
    } else {
        area = xs_round(c.area);
        for (int j = 0; j < XS_LIMBS; ++j) c.area.limb[j] = 0ll;
    }
    double* o = out + 4 * (size_t)(perm ? perm[i] : (unsigned)i);
    o[0] = area;
    o[1] = (double)k.tasks;
    o[2] = (double)k.leaves;
    o[3] = (double)sm.error;
    c.sums = SlotSums{};
}

// The ERR batch's second gather (aq_integrate_batch_err), behind k_gather_reset: the slots' error sums as
// rows {err_abs, err_signed} in the order k_gather_reset wrote its rows, and the sums back to zero.
__global__ __launch_bounds__(64) void k_gather_err(double* __restrict__ err, int first, int n, double* __restrict__ out,
                                                   const unsigned* __restrict__ perm) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    double* e = err + 2 * (size_t)(first + i);
    double* o = out + 2 * (size_t)(perm ? perm[i] : (unsigned)i);
    o[0] = e[0];
    o[1] = e[1];
    e[0] = e[1] = 0.0;
}

// ---- the device-resident batch (aq_integrate_batch_device) ------------------------------------------------
// Its two ends, in place of the host batch's staging threads and unpacking threads: k_dev_check before a
// chunk's size pre-pass and launch, k_gather_reset_soa behind the launch. Both read and write the CALLER's
// device arrays at the chunk's offset (the host passes the offset pointers); the schedule is
// device_batch_plan's (aq_batch_plan.h).
constexpr unsigned ROW_INVALID = AQ_ROW_INVALID;
static_assert(AQ_ROW_TIMEOUT == ERRB_TIMEOUT && AQ_ROW_OVERFLOW == ERRB_OVERFLOW && AQ_ROW_DEPTH == ERRB_DEPTH &&
                  (AQ_ROW_INVALID & (ERRB_TIMEOUT | ERRB_OVERFLOW | ERRB_DEPTH)) == 0,
              "aquad.h's row status bits are the slots' error bits, and one more");
// What aq_device_batch_check reads and zeroes: rows that failed the check, the OR of the rows' error bits.
struct DevBatchStat {
    unsigned long long invalid;
    unsigned errbits, pad;
};

// One row per thread: the domain predicate the host's checks use (aq_domain.h), the row into the chunk's
// bounds ring (theta ring) -- a row outside the domain as the empty interval [0, 0] with a zeroed theta row,
// which every integrand accepts at its root (width 0: the difference is 0 or NaN, never > eps) and the size
// pre-pass puts in its smallest class (estimate 0) -- and its flag. The invalid rows are counted per wave
// (ballot) and added by the wave's first lane: one atomic per wave that saw one, none otherwise.
template <int FID>
__device__ __forceinline__ void dev_check(const double* __restrict__ a, const double* __restrict__ b,
                                          const double* __restrict__ theta, int n, double2* __restrict__ bounds,
                                          double* __restrict__ th_out, unsigned* __restrict__ flag,
                                          DevBatchStat* __restrict__ stat) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    bool bad = false;
    if (i < n) {
        double x = a[i], y = b[i];
        if constexpr (FID == F_PARAM) {
            constexpr int NP = param::nparams;
            double th[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) th[j] = theta[(size_t)i * NP + j];
            bad = !params_ok(x, y, th);
#pragma unroll
            for (int j = 0; j < NP; ++j) th_out[(size_t)i * NP + j] = bad ? 0.0 : th[j];
        } else {
            bad = !bounds_ok(FID, x, y);
        }
        if (bad) x = y = 0.0;
        bounds[i] = make_double2(x, y);
        flag[i] = bad ? ROW_INVALID : 0u;
    }
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(&stat->invalid, (unsigned long long)__popcll(m));
}
template <int FID>
__global__ __launch_bounds__(256) void k_dev_check(const double* __restrict__ a, const double* __restrict__ b, int n,
                                                   double2* __restrict__ bounds, unsigned* __restrict__ flag,
                                                   DevBatchStat* __restrict__ stat) {
    static_assert(FID != F_PARAM, "the parametrised family's check takes theta (k_dev_check_params)");
    dev_check<FID>(a, b, nullptr, n, bounds, nullptr, flag, stat);
}
__global__ __launch_bounds__(256) void k_dev_check_params(const double* __restrict__ a, const double* __restrict__ b,
                                                          const double* __restrict__ theta, int n,
                                                          double2* __restrict__ bounds, double* __restrict__ th_out,
                                                          unsigned* __restrict__ flag, DevBatchStat* __restrict__ stat) {
    dev_check<F_PARAM>(a, b, theta, n, bounds, th_out, flag, stat);
}

// k_gather_reset and k_gather_err in one, for the device-resident batch: slot first + i's results (integral
// perm[i]'s, or i's) straight into the caller's typed arrays, any of which may be null -- the area, the counts
// through the same f64 the host batch's rows carry them in (unpack_rows: exact below 2^53), the error sums
// (err: the slots' sums behind an ERR launch, else null), status = the slot's error bits | the check's flag --
// and the slot (and its sums) back to zero. k_stream ORs a wave's error bits into every slot of its launch; the
// depth bit is kept only on the rows whose own tree reached the launch's max_depth (levels, which the slot does
// count per integral), so a shallow row beside a capped one reports 0 -- a stall or an overflow cannot be
// attributed and stays on every row of the chunk. A row the check flagged gets a NaN area and sums and zero counts
// (its slot ran the empty interval). The chunk's error bits are OR-ed into the context's word, one atomic per
// wave that saw one.
struct SoaOut {
    double* area;
    unsigned long long *accepted, *tasks;
    double *err_abs, *err_signed;
    unsigned* status;
};
__global__ __launch_bounds__(64) void k_gather_reset_soa(Ctl* __restrict__ ctls, const unsigned long long* __restrict__ parts,
                                                         int grid, int first, int n, const unsigned* __restrict__ perm,
                                                         double* __restrict__ err, const unsigned* __restrict__ flag,
                                                         int max_depth, SoaOut out, DevBatchStat* __restrict__ stat) {
    // the digits of a whole accumulator (a window wider than GATHER_WIN limbs: rare), one lane at a time
    __shared__ uint32_t s_dg[XS_LIMBS + 2];
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int slot = first + min(i, n - 1);
    Ctl& c = ctls[slot];
    SlotSums sm{};
    int lo = 0, hi = 0;
    if (i < n) {
        sm = c.sums;
        lo = sm.win_hi ? (int)~sm.win_lo_not : 0;
        hi = sm.win_hi ? min((int)sm.win_hi, XS_LIMBS) : 0;
    }
    double area = 0.0;
    for (unsigned long long wide = __ballot(hi - lo > GATHER_WIN); wide != 0ull; wide &= wide - 1ull) {
        if ((int)threadIdx.x == __builtin_ctzll(wide)) {
            uint32_t* const dg = s_dg;
            area = xs_round_digits(dg, c.area.limb, XS_LIMBS, XS_E0);
            for (int j = 0; j < XS_LIMBS; ++j) c.area.limb[j] = 0ll;
        }
    }
    unsigned bits = 0u;
    if (i < n) {
        const Counts k = slot_counts(sm, parts + 2 * parts_row(slot) * grid, grid);
        if (hi - lo <= GATHER_WIN) {
            long long w[GATHER_WIN];
#pragma unroll
            for (int j = 0; j < GATHER_WIN; ++j) w[j] = lo + j < hi ? c.area.limb[lo + j] : 0ll;
            area = xs_round_span<GATHER_WIN>(w, hi - lo, XS_E0 + 32 * lo);
#pragma unroll
            for (int j = 0; j < GATHER_WIN; ++j)
                if (lo + j < hi) c.area.limb[lo + j] = 0ll;
        }
        c.sums = SlotSums{};
        double ea = 0.0, es = 0.0;
        if (err) {
            double* e = err + 2 * (size_t)slot;
            ea = e[0], es = e[1];
            e[0] = e[1] = 0.0;
        }
        const size_t r = perm ? perm[i] : (unsigned)i;
        const bool bad = flag[r] != 0u;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        bits = sm.error & (k.levels >= (unsigned)max_depth ? ~0u : ~(unsigned)ERRB_DEPTH);
        if (out.area) out.area[r] = bad ? nan : area;
        if (out.tasks) out.tasks[r] = bad ? 0ull : (unsigned long long)(double)k.tasks;
        if (out.accepted) out.accepted[r] = bad ? 0ull : (unsigned long long)(double)k.leaves;
        if (out.err_abs) out.err_abs[r] = bad ? nan : ea;
        if (out.err_signed) out.err_signed[r] = bad ? nan : es;
        if (out.status) out.status[r] = bits | flag[r];
    }
    unsigned any = 0u;
#pragma unroll
    for (unsigned bit = 1u; bit <= ERRB_DEPTH; bit <<= 1)
        if (__ballot((bits & bit) != 0u) != 0ull) any |= bit;
    if (any && threadIdx.x == 0) atomicOr(&stat->errbits, any);
}

// ---- aq_integrate_batch_tol: between two rounds' launches -----------------------------------------------
// A round's ERR launch of the k live rows is followed by k_gather_reset and k_gather_err (rows {area, tasks,
// accepted, error bits} and {err_abs, err_signed} in launch order); the three kernels below read those rows
// and know nothing of Ctl. They run in stream order, and no workgroup waits for another: k_tol_test leaves a
// survivor flag per row and a count per workgroup, k_tol_compact sums the counts below its own workgroup.
// The next round's launch sizes its jobs from the job-size hint (LaunchHint, as a batch chunk's launch does
// from its pre-pass's preset): every round has another EPSILON, so the launches' own launch-to-launch hint
// never applies. Round 1 has no figure to go by and runs one job per integral (k_tol_init); later rounds
// take the survivors' mean tasks of the round before times `growth` (k_tol_compact).
constexpr int TOL_T = 256;     // threads per workgroup of the two kernels (they must agree: the counts are per workgroup)
constexpr int TOL_REC = 8;     // doubles per retired row: area, tasks, accepted, error bits, err_abs, err_signed, eps, +-round
struct TolSurv {               // pinned host memory, written by k_tol_compact
    unsigned count;                 // rows that survive the round
    unsigned idx[PCU_MAXK - 1];     // the first survivors' original indices: a launch of fewer than PCU_MAXK
};                                  // integrals takes its bounds from the host

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(TOL_T) void k_tol_init(unsigned* __restrict__ idx, int n, LaunchHint* __restrict__ hint) {
    const int i = (int)(blockIdx.x * TOL_T + threadIdx.x);
    if (i < n) idx[i] = (unsigned)i;
    if (i == 0) {
        hint->shares_next = 1u;
        hint->per_next = 0ull;   // (unknown: the launch's fill rule adds no shares)
    }
}

// Test and retire. Row i of the round (original index idx[i]) has converged when err_abs <= fmax(epsabs,
// epsrel * |area|), in double, a tie included, a NaN in err_abs or area excluded. It retires -- its record
// written at its original index -- when it converged, carries error bits, or this is the last round; the
// record's round is negative unless it converged free of error bits.
__global__ __launch_bounds__(TOL_T) void k_tol_test(const double* __restrict__ rows, const double* __restrict__ err,
                                                    const unsigned* __restrict__ idx, int k, double epsabs, double epsrel,
                                                    double eps, int round, int last, double* __restrict__ res,
                                                    unsigned char* __restrict__ flag, unsigned* __restrict__ cnt,
                                                    double* __restrict__ tsum) {
    __shared__ unsigned s_wc[TOL_T / 64];
    __shared__ double s_wt[TOL_T / 64];
    const int i = (int)(blockIdx.x * TOL_T + threadIdx.x);
    bool live = false;
    double live_tasks = 0.0;   // a survivor's tasks this round (whole numbers: the sums are exact)
    if (i < k) {
        const double area = rows[4 * (size_t)i], tasks = rows[4 * (size_t)i + 1], acc = rows[4 * (size_t)i + 2];
        const double bits = rows[4 * (size_t)i + 3];
        const double ea = err[2 * (size_t)i], es = err[2 * (size_t)i + 1];
        const bool conv = !(ea != ea) && !(area != area) && ea <= fmax(epsabs, epsrel * fabs(area));
        const bool clean = bits == 0.0;
        live = !(conv || !clean || last);
        if (!live) {
            double* o = res + TOL_REC * (size_t)idx[i];
            o[0] = area; o[1] = tasks; o[2] = acc; o[3] = bits;
            o[4] = ea; o[5] = es; o[6] = eps;
            o[7] = conv && clean ? (double)round : -(double)round;
        }
        flag[i] = live ? 1 : 0;
        if (live) live_tasks = tasks;
    }
    const unsigned long long m = __ballot(live);
    const double wt = wave_sum_f64(live_tasks);
    if (lane_id() == 0) {
        s_wc[threadIdx.x >> 6] = (unsigned)__popcll(m);
        s_wt[threadIdx.x >> 6] = wt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0;
        double t = 0.0;
        for (int v = 0; v < TOL_T / 64; ++v) c += s_wc[v], t += s_wt[v];
        cnt[blockIdx.x] = c;
        tsum[blockIdx.x] = t;
    }
}

// Stable compaction of the survivors' {a, b}, theta rows (np doubles each; none when np == 0) and original
// indices into the other ping-pong buffers, in input order: a row's place is the survivors of the workgroups
// below (cnt) + of the waves below in its workgroup + of the lanes below in its wave (ballot / mbcnt). The
// count and the first survivors' indices go to pinned host memory. The last workgroup, which sums every count,
// also sums the survivors' tasks (tsum) and presets the next launch's job size from their mean times `growth`
// (k_batch_scatter's rule: about TASKS_PER_JOB tasks per job, at most max_shares shares per integral).
__global__ __launch_bounds__(TOL_T) void k_tol_compact(const unsigned char* __restrict__ flag, const unsigned* __restrict__ cnt,
                                                       int k, const double2* __restrict__ b_in,
                                                       const double* __restrict__ th_in, const unsigned* __restrict__ i_in,
                                                       double2* __restrict__ b_out, double* __restrict__ th_out,
                                                       unsigned* __restrict__ i_out, int np, TolSurv* __restrict__ host,
                                                       const double* __restrict__ tsum, double growth,
                                                       LaunchHint* __restrict__ hint, unsigned max_shares) {
    __shared__ unsigned s_base[TOL_T / 64], s_wc[TOL_T / 64];
    __shared__ double s_wt[TOL_T / 64];
    const bool last_wg = blockIdx.x == gridDim.x - 1;
    unsigned part = 0;
    for (unsigned j = threadIdx.x; j < blockIdx.x; j += TOL_T) part += cnt[j];
    part = wave_sum_u(part);
    double tpart = 0.0;
    if (last_wg)
        for (unsigned j = threadIdx.x; j < gridDim.x; j += TOL_T) tpart += tsum[j];
    tpart = wave_sum_f64(tpart);
    const int i = (int)(blockIdx.x * TOL_T + threadIdx.x);
    const bool live = i < k && flag[i] != 0;
    const unsigned long long m = __ballot(live);
    const unsigned w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        s_base[w] = part;
        s_wc[w] = (unsigned)__popcll(m);
        s_wt[w] = tpart;
    }
    __syncthreads();
    unsigned off = 0, mine = 0;
    for (unsigned v = 0; v < (unsigned)(TOL_T / 64); ++v) {
        off += s_base[v] + (v < w ? s_wc[v] : 0u);
        mine += s_base[v] + s_wc[v];
    }
    if (live) {
        const unsigned pos = off + mbcnt(m);   // < k: at most the rows before this one survive
        const unsigned orig = i_in[i];
        b_out[pos] = b_in[i];
        i_out[pos] = orig;
        for (int j = 0; j < np; ++j) th_out[(size_t)pos * np + j] = th_in[(size_t)i * np + j];
        if (pos < (unsigned)(PCU_MAXK - 1)) host->idx[pos] = orig;
    }
    if (last_wg && threadIdx.x == 0) {
        host->count = mine;
        if (mine) {
            double t = 0.0;
            for (int v = 0; v < TOL_T / 64; ++v) t += s_wt[v];
            const double per = growth * t / (double)mine;   // predicted tasks per surviving integral
            const double sh = floor((per + 0.5 * TASKS_PER_JOB) / TASKS_PER_JOB);
            hint->shares_next = (unsigned)fmin(fmax(sh, 1.0), (double)max_shares);
            hint->per_next = (unsigned long long)fmax(per, 0.0);
        }
    }
}

// The same slots as exact int64 rows (AQ_EXACT_ROW each): limbs, tasks, accepted, spilled,
// levels | error << 32. Sums of such rows (an int64 all-reduce) keep the area exact.
__global__ __launch_bounds__(64) void k_gather_exact(const Ctl* __restrict__ ctls,
                                                     const unsigned long long* __restrict__ parts, int grid, int first,
                                                     int n, int nslots, long long* __restrict__ out) {
    const int i = (int)blockIdx.x;
    if (i >= n) return;
    const int slot = (first + i) % nslots;
    const Ctl& c = ctls[slot];
    long long* o = out + (size_t)AQ_EXACT_ROW * i;
    for (int k = threadIdx.x; k < XS_LIMBS; k += blockDim.x) o[k] = c.area.limb[k];
    if (threadIdx.x == 0) {
        const Counts k = slot_counts(c.sums, parts + 2 * parts_row(slot) * grid, grid);
        o[XS_LIMBS] = (long long)k.tasks;
        o[XS_LIMBS + 1] = (long long)k.leaves;
        o[XS_LIMBS + 2] = (long long)c.sums.spilled;
        o[XS_LIMBS + 3] = (long long)k.levels | ((long long)c.sums.error << 32);
    }
}

// PCU_AREA (aq_stream.h): add the exact sum of a per-CU launch's workgroup area words -- 2 x grid doubles,
// one double-double per workgroup -- to sx[XS_LIMBS] (block-shared). Every thread of the block calls it
// between barriers; LDS int64 atomics keep the sum exact in any order.
__device__ __forceinline__ void add_wg_area(long long* sx, const double* __restrict__ pa, int grid) {
    for (int i = threadIdx.x; i < 2 * grid; i += blockDim.x) {
        XDigits g;
        if (xs_digits(pa[i], g)) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (g.d[k]) atomicAdd(reinterpret_cast<unsigned long long*>(&sx[g.i + k]), (unsigned long long)g.d[k]);
        }
    }
}

// After an asynchronous per-CU launch of k integrals (slots first .. first + k - 1; pa: the launch's area
// row, integral b's words at pa + 2 * b * grid): each slot's workgroup areas into its exact accumulator,
// one workgroup per slot -- every reader (k_gather*, aq_fetch*) then sees the whole area in the slot.
__global__ __launch_bounds__(256) void k_fold_parts(Ctl* __restrict__ ctls, const double* __restrict__ pa, int grid,
                                                    int first) {
    __shared__ long long sx[XS_LIMBS];
    for (int i = threadIdx.x; i < XS_LIMBS; i += blockDim.x) sx[i] = 0;
    __syncthreads();
    add_wg_area(sx, pa + 2 * (size_t)blockIdx.x * grid, grid);
    __syncthreads();
    Ctl& c = ctls[first + (int)blockIdx.x];
    for (int i = threadIdx.x; i < XS_LIMBS; i += blockDim.x)
        if (sx[i]) c.area.limb[i] += sx[i];
}

// Return slots [first, first + n) to the all-zero state a launch needs: sums and the exact area
// accumulator; the histograms when they were written.
__global__ __launch_bounds__(128) void k_reset(Ctl* __restrict__ ctls, int first, int zero_hist) {
    Ctl& c = ctls[first + (int)blockIdx.x];
    for (int i = threadIdx.x; i < XS_LIMBS; i += blockDim.x) c.area.limb[i] = 0;
    if (zero_hist)
        for (int i = threadIdx.x; i < 2 * AQ_MAX_LEVELS; i += blockDim.x) c.hist[i] = 0ull;
    if (threadIdx.x == 0) {
        c.sums = SlotSums{};
    }
}

// The synchronous path's read-back (aq_integrate / aq_integrate_shard): one workgroup copies the
// internal sync slot's result -- sums, exact limbs, the per-workgroup words of a per-CU launch, the
// histograms when written -- straight into pinned host memory, then zeroes the slot for the next
// call. One small launch in place of a reset kernel, a memset and three or four device-to-host
// copies around every call.
struct SyncOut {
    unsigned long long seq;   // the call's sequence number, stored last (the host waits on it)
    SlotSums sums;
    XSum area;
    unsigned long long hist[2 * AQ_MAX_LEVELS];
    unsigned long long parts[2 * MAXG];
    double err[2];            // ERR calls: the slot's error sums {Σ|d|, Σd} (aq_integrate_err)
};
__global__ __launch_bounds__(256) void k_fetch_sync(Ctl* __restrict__ c, unsigned long long* __restrict__ parts,
                                                    const double* __restrict__ parea, int grid, int with_parts,
                                                    int with_hist, SyncOut* __restrict__ out,
                                                    unsigned long long seq) {
    const int t = threadIdx.x;
    __shared__ long long sx[XS_LIMBS];
    if (t == 0) out->sums = c->sums;
    for (int i = t; i < XS_LIMBS; i += blockDim.x) sx[i] = c->area.limb[i];
    __syncthreads();
    if (with_parts) add_wg_area(sx, parea, grid);   // a per-CU launch's workgroup areas (PCU_AREA)
    __syncthreads();
    for (int i = t; i < XS_LIMBS; i += blockDim.x) out->area.limb[i] = sx[i];
    if (with_hist)
        for (int i = t; i < 2 * AQ_MAX_LEVELS; i += blockDim.x) out->hist[i] = c->hist[i];
    if (with_parts)
        for (int i = t; i < 2 * grid; i += blockDim.x) out->parts[i] = parts[i];
    __syncthreads();   // every read precedes the zeroing
    if (t == 0) c->sums = SlotSums{};
    for (int i = t; i < XS_LIMBS; i += blockDim.x) c->area.limb[i] = 0;
    if (with_hist)
        for (int i = t; i < 2 * AQ_MAX_LEVELS; i += blockDim.x) c->hist[i] = 0ull;
    if (with_parts)
        for (int i = t; i < 2 * grid; i += blockDim.x) parts[i] = 0ull;
    // the result is complete in host memory: every thread's stores made visible system-wide, then the
    // sequence number released. The host sees it before the kernel's completion signal would arrive
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(&out->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The ERR synchronous call (aq_integrate_err): the sync slot's pair of error sums (err: its two doubles) into
// the pinned result and back to zero -- launched on the stream IN FRONT of k_fetch_sync, whose sequence
// number the host waits for: this kernel has completed, its stores visible system-wide, before that one starts.
__global__ __launch_bounds__(64) void k_fetch_sync_err(double* __restrict__ err, SyncOut* __restrict__ out) {
    const int t = threadIdx.x;
    if (t < 2) {
        out->err[t] = err[t];
        err[t] = 0.0;
    }
    __threadfence_system();
}

// aq_integrate_group: one rank's contribution to the RCCL exchange. sum_row (int64, summed over
// ranks): limbs, tasks, accepted, spilled. info (gathered from every rank): tasks, levels, error,
// then the rank's per-workgroup pack_cu words (grid of them; zero when not kept).
__global__ __launch_bounds__(256) void k_pack_group(const Ctl* __restrict__ ctls, const unsigned long long* parts,
                                                    const double* __restrict__ parea, int slot, int grid, int with_parts,
                                                    long long* __restrict__ sum_row, unsigned long long* __restrict__ info) {
    const Ctl& c = ctls[slot];
    const unsigned long long* wp = parts + 2 * parts_row(slot) * grid;
    __shared__ long long sx[XS_LIMBS];
    for (int k = threadIdx.x; k < XS_LIMBS; k += blockDim.x) sx[k] = c.area.limb[k];
    __syncthreads();
    if (with_parts) add_wg_area(sx, parea + 2 * parts_row(slot) * grid, grid);   // PCU_AREA
    __syncthreads();
    for (int k = threadIdx.x; k < XS_LIMBS; k += blockDim.x) sum_row[k] = sx[k];
    for (int k = threadIdx.x; k < grid; k += blockDim.x) info[3 + k] = with_parts ? wp[2 * k] : 0ull;
    if (threadIdx.x == 0) {
        const Counts k = slot_counts(c.sums, wp, grid);
        sum_row[XS_LIMBS] = (long long)k.tasks;
        sum_row[XS_LIMBS + 1] = (long long)k.leaves;
        sum_row[XS_LIMBS + 2] = (long long)c.sums.spilled;
        info[0] = k.tasks;
        info[1] = k.levels;
        info[2] = c.sums.error;
    }
}

}  // namespace aq

#include "aq_abi.inc"   // host side: the C ABI (include/aquad.h)
