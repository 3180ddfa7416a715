// aq_shape.h -- the launch-shape constants of the persistent kernel (aq_stream.h) and the seed-depth rule:
// what the kernel and the host's launch plan (aq_launch_plan.h) must agree on.
//
// Plain C++ (host and device): the CPU tests compile this header with g++ (tests/test_launch_plan.py).
#pragma once

// (as aq_xsum.h's AQ_HD, without the forced inlining: the seed-depth functions below keep the attributes
// they had in aq_stream.h)
#if defined(__HIPCC__)
#define AQ_SHAPE_HD __host__ __device__
#else
#define AQ_SHAPE_HD
#endif

namespace aq {

#ifndef AQ_PT
#define AQ_PT 768
#endif
#ifndef AQ_WCAP
#define AQ_WCAP 256
#endif
constexpr int PT = AQ_PT;           // threads per workgroup
constexpr int NW = PT / 64;         // waves (workers) per workgroup: 12, three per SIMD
constexpr int WCAP = AQ_WCAP;       // per-wave LDS ring, pairs: a round pops <= 64, pushes <= 128
#ifndef AQ_LONE_NW
#define AQ_LONE_NW 8   // waves per workgroup of unsharded lone (per-CU) launches; NW (12) for all others
#endif
#ifndef AQ_S_W
#define AQ_S_W 2
#endif
constexpr int S_W = AQ_S_W;              // seed depth D = floor(log2 V) + S_W: 3 or 4 positions per share
#ifndef AQ_S_W1
#define AQ_S_W1 2
#endif
// seed depth of a job: floor(log2 V) + S_W for V = shares x shards virtual workers; a whole-integral
// job (V = 1, tiny trees of big batches) seeds at S_W1 (its partition is the whole tree at any depth)
AQ_SHAPE_HD constexpr int seed_depth(unsigned long long V) {
    return V <= 1ull ? AQ_S_W1 : 63 - __builtin_clzll(V) + S_W;
}
// positions per share, ceil(2^D / V): with L = floor(log2 V), 2^D / V lies in (2^(D-L-1), 2^(D-L)], so a
// count-down of at most 2^(D-L-1) steps instead of a 64-bit division (cold code at every seeding)
AQ_SHAPE_HD constexpr unsigned seed_nb(int D, unsigned long long V) {
    if (V <= 1ull) return 1u << D;
    unsigned nb = 1u << (D - (63 - __builtin_clzll(V)));
    while (nb > 1u && (unsigned long long)(nb - 1u) * V >= (1ull << D)) --nb;
    return nb;
}
// a job's seed depth: seed_depth(V), one level deeper where the seeding's one-wave fast path
// ((D + 1) levels x nb positions <= 64 nodes) still holds the deeper seeding -- the bench's adaptive
// jobs (V ~ 24: 3 -> 6 positions per share) and whole-integral jobs (V = 1: 4 -> 8 positions); not a
// lone launch (V = 3072: 42 -> 90 nodes). r04n A/B at 32768 integrals: -0.8 %, C3 unchanged
// (profiles/r04n2). The oracle's shard partition restates this rule (tests' device_seed_S).
AQ_SHAPE_HD constexpr int seed_depth_job(unsigned long long V) {
    return (unsigned long long)(seed_depth(V) + 2) * seed_nb(seed_depth(V) + 1, V) <= 64ull
        ? seed_depth(V) + 1 : seed_depth(V);
}
// launches of fewer integrals keep per-workgroup (per-CU) counts and LDS exact accumulators (the LDS
// left beside the pair block holds 12)
constexpr int PCU_MAXK = 12;
constexpr int STATIC_MAXK = 16;     // sharded launches of fewer integrals: one share per wave, static stride
                                    // (unsharded: below PCU_MAXK, aq_launch_plan.h plan_launch)
// max integrals per launch: 8 x 32768, so that N = 8 ranks holding 1/8 of each integral of a batch
// pack the same work into one launch as one GPU does with the whole batch (r04)
constexpr int MAXK = 1 << 18;
constexpr int NSLOTS = MAXK;
// one more, internal slot for the synchronous calls (aq_integrate / aq_integrate_shard): they never
// touch the caller's async slots, and k_fetch_sync leaves it zeroed for the next call
constexpr int SYNC_SLOT = NSLOTS;
// slots whose per-CU launches keep per-workgroup words (parts), plus one row for the sync slot
// PCU_AREA: a per-CU launch's area is kept per workgroup -- each wave adds its flushes' double-doubles
// into its own LDS pair per integral (flush_acc), the workgroup's last wave sums its waves' into two
// doubles beside the count words (StreamParams::parea) -- and readers add the grid's pairs into the slot's
// exact accumulator: k_fold_parts after an asynchronous per-CU launch, k_fetch_sync / k_pack_group on the
// synchronous and group paths. So the area of a lone integral is the correctly rounded sum of 2 x grid
// doubles, each a double-double of its workgroup's waves' partials (no far atomic at the launch's end).
// (r06: 16384, was 65536 -- with the per-workgroup area words beside the counts, PCU_AREA, the two blocks
// take 134 MB where the counts alone took 268 MB)
constexpr int NPARTS = 16384;
#ifndef AQ_GSPLIT_DEFAULT
// sharded launches / first launch: 16 shares per integral over all shards (2-rank rehearsal, r03: 32 ->
// 1.743e11, 64 -> 1.778e11, 96 -> 1.803e11; r04, per task of a launch of N x 16384 integrals sharded
// N ways, profiles/r04n5/shard_ab.txt: 96 -> 192 = +1.3 / +0.3 / +0 % at N = 2 / 4 / 8, 384 -0.8 % at 8)
#define AQ_GSPLIT_DEFAULT 192
#endif
constexpr int DEFAULT_GSPLIT = AQ_GSPLIT_DEFAULT;  // a multi-integral launch's job = the share of this many waves
#ifndef AQ_LONE_GSPLIT
#define AQ_LONE_GSPLIT 1   // waves per share in launches of < 16 unsharded integrals (aq_launch_plan.h)
#endif
#ifndef AQ_TAIL_DIV
#define AQ_TAIL_DIV 32   // r02 A/B (8192 x eps=1e-10 per launch): no tail 27.45, /64 x4 27.30, /32 x4 27.17 ms
#endif
#ifndef AQ_TAIL_MULT
#define AQ_TAIL_MULT 4
#endif

}  // namespace aq

#undef AQ_SHAPE_HD
