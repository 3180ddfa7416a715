// The lines of a wave's LDS ring: one definition for k_stream's outer loop, its burst and the CPU model
// (tests/test_ring_window.py walks every transition of these rules; tools/ring_sim.py --mode carried
// restates them on the real tree).
//
// A wave keeps its pairs in a ring of `wcap` slots (chunks of CHUNK = 64 pairs move between the ring's
// bottom and the wave's HBM cellar) and, inside a burst, one held pair per lane in registers. With
//   S = R + H    the wave's pairs: R in the ring, H held (H <= 64; H = 0 outside a burst)
//   L            the spill line on S
// the rules are
//   round:    runs while  lo < S <= L.  The fill moves min(64 - H, R) pairs from the ring to idle lanes
//             (S unchanged); each of the na held pairs is evaluated and leaves, each of its two tasks
//             that refines adds one pair: task 1's children are pushed (<= na pairs), task 0's stay held.
//             So S' <= S + na <= S + 64, and the ring after the round holds at most
//             (S - na) + na = S <= L <= wcap pairs: THE RING NEVER HOLDS MORE THAN S AT THE ROUND'S START.
//   spill:    S' > L  =>  R' = S' - H' >= L + 1 - 64 >= CHUNK (L >= 2 CHUNK - 1), so a whole chunk lies at
//             the bottom; one spill restores S' - 64 <= L.
//   issue:    S <= issue line, cellar not empty, nothing in flight: 64 cellar pairs are loaded (registers).
//   landing:  S <= landing line with a prefetch in flight: +64 at the bottom, S + 64 <= land + 64 <= L.
//   exit:     a burst can end with S up to L + 64 (its give / poll round came due, the cellar is full, the
//             depth cap). The held pairs go back on top of the ring: while R + H > wcap the bottom chunk
//             moves out first (cellar, else pool, else an HBM chunk) -- R + H <= L + 64, so that is
//             exit_chunks() <= 1 chunk for L <= wcap, and R >= wcap + 1 - 64 >= CHUNK holds one.
//   outside:  H = 0 and R <= wcap; above L the bottom chunk moves out, as before.
//   refill:   an empty ring takes up to refill <= L pairs (whole chunks) from the cellar or the pool.
//
// Until r06 the line sat at wcap - 64: the popped-pairs round (r03) took 64 pairs out and put up to 128
// back, so 64 slots of headroom were physical. The carried round needs none (above).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AQ_RW_HD __host__ __device__
#else
#define AQ_RW_HD
#endif

namespace aq {

constexpr int RING_CHUNK = 64;   // pairs per cellar move (one per lane)

struct RingLines {
    int wcap;       // ring slots
    int line;       // L: spill above this S
    int pf_issue;   // issue a cellar prefetch at or below this S
    int pf_below;   // land it at or below this S
    int refill;     // most pairs an empty ring takes at once
};

AQ_RW_HD constexpr bool ring_lines_valid(const RingLines& l) {
    return l.wcap >= 2 * RING_CHUNK && l.wcap % RING_CHUNK == 0 &&
           l.line <= l.wcap &&                    // R <= S <= L <= wcap at every round
           l.line >= 2 * RING_CHUNK - 1 &&        // a spill finds a whole chunk in the ring
           l.pf_below >= 0 && l.pf_below + RING_CHUNK <= l.line &&   // a landing stays at or below L
           l.pf_issue >= l.pf_below && l.pf_issue < l.line &&        // the window between the edges is not empty
           l.refill >= RING_CHUNK && l.refill % RING_CHUNK == 0 && l.refill <= l.line;
}

// the burst window: rounds go on while  b_lo1 <= S < b_lo1 + b_span  (one unsigned compare of S - b_lo1)
AQ_RW_HD constexpr unsigned burst_lo1(const RingLines& l, bool pf_in_flight, bool cellar_nonempty) {
    return (unsigned)(pf_in_flight ? l.pf_below : (cellar_nonempty ? l.pf_issue : 0)) + 1u;
}
AQ_RW_HD constexpr unsigned burst_span(const RingLines& l, unsigned lo1) { return (unsigned)l.line + 1u - lo1; }
AQ_RW_HD constexpr bool above_line(const RingLines& l, unsigned S) { return S > (unsigned)l.line; }
// chunks a burst's end moves out of the ring's bottom before it pushes `held` pairs back on top of `ring`
AQ_RW_HD constexpr unsigned exit_chunks(const RingLines& l, unsigned ring, unsigned held) {
    return ring + held > (unsigned)l.wcap
               ? (ring + held - (unsigned)l.wcap + (unsigned)RING_CHUNK - 1u) / (unsigned)RING_CHUNK
               : 0u;
}
// the most pairs a wave can hold when a burst ends (a round from S = L with 64 lanes, every task refining)
AQ_RW_HD constexpr unsigned max_exit_pairs(const RingLines& l) { return (unsigned)l.line + (unsigned)RING_CHUNK; }

}  // namespace aq
