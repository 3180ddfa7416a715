// aq_frontier_walk.h -- the frontier engine's host loop: chained level steps from depth to depth over one frontier,
// with a host look at the device's record count every sync_every levels. One description of a walk and one function
// that runs it over the caller's operations: aq_abi.inc walk_run supplies the ones that enqueue (level_step_impl,
// k_mesh_refine_append, the one-word count copy) for aq_frontier_integrate / aq_integrate_mesh,
// aq_integrate_mesh_batch and aq_mesh_refine_batch.
//
// Plain host C++17, no HIP: the CPU tests run it over a table of level sizes (tests/test_frontier_walk.py).
#pragma once
#include <algorithm>

#include "aquad.h"

namespace aq {

// The callers differ in four places: where the walk starts (start_depth), how wide that level may be (start_bound),
// whether seed records join a depth before its step (seed_end, last_seed_depth), and when an empty level may end
// the walk (only past last_seed_depth).
struct FrontierWalk {
    int start_depth = 0;
    unsigned long long start_bound = 0;   // the records level start_depth may hold before any seeds
    unsigned long long cap = 0;           // the frontier buffers' records: no level is stepped wider
    int max_depth = 0;
    int sync_every = 1;                   // levels between two host looks
    // the seed records of depth e are [seed_end[e - 1], seed_end[e]) of the caller's seed buffer, 1 <= e <=
    // AQ_MAX_LEVELS (seed_end has AQ_MAX_LEVELS + 1 entries); null: no seeds
    const unsigned long long* seed_end = nullptr;
    int last_seed_depth = -1;             // the last depth that has seeds (-1: none)

    unsigned long long seeds_of(int depth) const {
        return seed_end && depth >= 1 && depth <= AQ_MAX_LEVELS ? seed_end[depth] - seed_end[depth - 1] : 0ull;
    }
    bool empty() const { return start_bound == 0 && last_seed_depth < 0; }   // nothing to walk: no call at all
};

struct WalkEnd {
    int rc;      // AQ_OK, AQ_EOVERFLOW (a look read more than cap), or the first non-zero code of an operation
    int depth;   // the depth whose frontier the walk left unstepped: records there mean AQ_EDEPTH
};

// The caller's operations: seed(depth, ns) appends the ns seed records of `depth` to its frontier; step(depth, n_in)
// is the level step of `depth` over at most n_in records; look(depth, &now) folds what is pending and reads the
// device's count of `depth`. Each returns AQ_OK or the code that ends the walk.
//
// `bound` is what the host knows of the next level's width without looking: twice the level before, within cap,
// until a look replaces it by the true count. An empty level ends the walk -- known from the bound or seen at a
// look -- once no deeper seeds are left.
template <typename Seed, typename Step, typename Look>
WalkEnd frontier_walk(const FrontierWalk& w, Seed&& seed, Step&& step, Look&& look) {
    int depth = w.start_depth, since = 0, rc = AQ_OK;
    if (w.empty()) return {rc, depth};
    unsigned long long bound = w.start_bound;
    while (depth <= w.max_depth && depth < AQ_MAX_LEVELS) {
        const unsigned long long ns = w.seeds_of(depth);
        if (ns && (rc = seed(depth, ns))) break;
        const unsigned long long n_in = std::min(bound + ns, w.cap);
        if ((rc = step(depth, n_in))) break;
        ++depth;
        bound = std::min(2 * n_in, w.cap);
        if (bound == 0 && depth > w.last_seed_depth) break;
        if (++since == w.sync_every) {
            since = 0;
            unsigned long long now = 0;
            if ((rc = look(depth, &now))) break;
            if (now == 0 && depth > w.last_seed_depth) break;
            if (now > w.cap) {
                rc = AQ_EOVERFLOW;
                break;
            }
            bound = now;
        }
    }
    return {rc, depth};
}

}  // namespace aq
