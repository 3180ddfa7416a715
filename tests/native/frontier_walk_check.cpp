// Run aq::frontier_walk (ppls_amd/csrc/aq_frontier_walk.h) over fake operations, g++ alone: no device, a table of
// the true level sizes instead -- what a look would read. Input (a file, argv[1]), one case per line:
//   start_depth start_bound cap max_depth sync_every last_seed_depth  fail_kind fail_at fail_code
//   K (depth size) x K   M (depth seeds) x M
// fail_kind 1 / 2 / 3: the fail_at-th (from 0) seed / step / look returns fail_code; 0: none fails. M = -1: a walk
// without a seed table. Output: one JSON line per call, {"op", "depth", "n"} (n: a seed's ns, a step's n_in, what a
// look read), then {"rc", "depth"} for the case. Built and run by tests/test_frontier_walk.py.
#include <cstdio>
#include <vector>

#include "aq_frontier_walk.h"

using namespace aq;

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: frontier_walk_check CASES\n");
        return 2;
    }
    int cases = 0, fail_kind, fail_at, fail_code, k, m;
    FrontierWalk w;
    while (fscanf(f, "%d %llu %llu %d %d %d %d %d %d %d", &w.start_depth, &w.start_bound, &w.cap, &w.max_depth,
                  &w.sync_every, &w.last_seed_depth, &fail_kind, &fail_at, &fail_code, &k) == 10) {
        std::vector<unsigned long long> size(AQ_MAX_LEVELS + 2, 0), seeds(AQ_MAX_LEVELS + 1, 0), seed_end(AQ_MAX_LEVELS + 1, 0);
        int d;
        unsigned long long v;
        for (int i = 0; i < k; ++i) {
            if (fscanf(f, "%d %llu", &d, &v) != 2 || d < 0 || d > AQ_MAX_LEVELS + 1) return 2;
            size[d] = v;
        }
        if (fscanf(f, "%d", &m) != 1) return 2;
        for (int i = 0; i < m; ++i) {
            if (fscanf(f, "%d %llu", &d, &v) != 2 || d < 1 || d > AQ_MAX_LEVELS) return 2;
            seeds[d] = v;
        }
        for (int e = 1; e <= AQ_MAX_LEVELS; ++e) seed_end[e] = seed_end[e - 1] + seeds[e];
        w.seed_end = m < 0 ? nullptr : seed_end.data();
        int seen[4] = {0, 0, 0, 0};
        auto call = [&](int kind, const char* op, int depth, unsigned long long n) {
            printf("{\"op\": \"%s\", \"depth\": %d, \"n\": %llu}\n", op, depth, n);
            return kind == fail_kind && seen[kind]++ == fail_at ? fail_code : AQ_OK;
        };
        const WalkEnd end = frontier_walk(
            w, [&](int depth, unsigned long long ns) { return call(1, "seed", depth, ns); },
            [&](int depth, unsigned long long n_in) { return call(2, "step", depth, n_in); },
            [&](int depth, unsigned long long* now) {
                *now = size[depth];   // (depth <= AQ_MAX_LEVELS: the walk steps below AQ_MAX_LEVELS)
                return call(3, "look", depth, *now);
            });
        printf("{\"rc\": %d, \"depth\": %d}\n", end.rc, end.depth);
        ++cases;
    }
    const bool eof = feof(f) != 0;
    fclose(f);
    if (!eof) {
        fprintf(stderr, "unreadable case after %d cases\n", cases);
        return 2;
    }
    return 0;
}
