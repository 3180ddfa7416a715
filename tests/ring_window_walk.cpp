// Walks every reachable state of a wave's ring under the rules of ppls_amd/csrc/aq_ring_window.h, the way
// k_stream applies them (aq_stream.h: the outer loop's landing / refill / overflow / give / issue steps,
// the burst's rounds and cellar edges, the burst's end), and checks the capacity invariants at every step.
//
//   ring_window_walk WCAP LINE PF_ISSUE PF_BELOW REFILL [--no-exit-drain]
//
// State: R pairs in the ring, H held pairs (inside a burst), pf (a prefetch in flight), c cellar chunks
// (the cellar holds CCH chunks at most, so the "cellar full" paths are walked too). A round from (R, H):
// the fill takes k = min(64 - H, R) pairs, na = H + k lanes are active, and ANY p <= na pairs are pushed
// and ANY h <= na pairs stay held (each lane's two tasks refine or not, independently). A burst may end
// after any round (its give / poll round came due). Exit status 0: every invariant held; 1: a violation
// (printed); 2: the lines themselves are invalid (ring_lines_valid).
// --no-exit-drain leaves out the burst end's chunk moves: the walk must then find the overflow.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "aq_ring_window.h"

using namespace aq;

namespace {

constexpr unsigned CCH = 3;   // cellar capacity in chunks (small: the full-cellar paths are reached)
RingLines RL;
bool exit_drain = true;
unsigned long long n_states = 0, n_trans = 0, n_spills = 0, n_lands = 0, n_exits = 0, n_exit_moves = 0;
unsigned max_ring = 0, max_S = 0;

struct St {
    unsigned R, H, pf, c;
};

[[noreturn]] void fail(const char* what, const St& s, unsigned p = 0, unsigned h = 0) {
    std::printf("VIOLATION: %s at R=%u H=%u pf=%u c=%u (pushes %u, held after %u)\n", what, s.R, s.H, s.pf, s.c, p, h);
    std::exit(1);
}

// visited sets: states at a round's start, and states at the outer loop's top (H = 0)
unsigned RMAX;
std::vector<unsigned char> seen_round, seen_outer, seen_post;
std::vector<St> work_round, work_outer;

size_t idx(const St& s) { return (((size_t)s.R * 65u + s.H) * 2u + s.pf) * (CCH + 1u) + s.c; }

void push_round(const St& s) {
    // a round's start: the ring within its slots, the wave's pairs at or below the line
    if (s.R > (unsigned)RL.wcap) fail("ring above WCAP at a round's start", s);
    if (s.R + s.H > (unsigned)RL.line) fail("S above the line at a round's start", s);
    if (s.R + s.H == 0) fail("a round without pairs", s);
    if (!seen_round[idx(s)]) {
        seen_round[idx(s)] = 1;
        work_round.push_back(s);
    }
}
void push_outer(const St& s) {
    if (s.H) fail("held pairs outside a burst", s);
    if (s.R > (unsigned)RL.wcap) fail("ring above WCAP in the outer loop", s);
    if (!seen_outer[idx(s)]) {
        seen_outer[idx(s)] = 1;
        work_outer.push_back(s);
    }
}

// chunk_out: the bottom chunk leaves the ring (cellar when it has room -- a prefetch in flight is
// cancelled first -- else the pool or an HBM chunk)
void chunk_out(St& s, const char* where) {
    if (s.R < (unsigned)RING_CHUNK) fail(where, s);
    if (s.pf) {
        s.c += 1;
        s.pf = 0;
    }
    if (s.c + 1 <= CCH) s.c += 1;
    s.R -= RING_CHUNK;
}

// the burst's end from (R, H): move chunks out, push the held pairs back, hand over to the outer loop
void burst_exit(St s) {
    ++n_exits;
    if (exit_drain) {
        const unsigned n = exit_chunks(RL, s.R, s.H);
        const unsigned before = s.R + s.H;
        for (unsigned i = 0; i < n; ++i) chunk_out(s, "the burst's end found no whole chunk to move out");
        n_exit_moves += n;
        if (n && before - (n - 1) * RING_CHUNK <= (unsigned)RL.wcap) fail("the burst's end moved out more chunks than needed", s);
        if (n > 1) fail("the burst's end moved out more than one chunk", s);
    }
    if (s.R + s.H > (unsigned)RL.wcap) fail("the push-back overflows the ring", s);
    s.R += s.H;
    s.H = 0;
    if (s.R > max_ring) max_ring = s.R;
    push_outer(s);
}

void round_from(const St& s0) {
    const unsigned k = std::min(64u - s0.H, s0.R);
    const unsigned na = s0.H + k, Rf = s0.R - k;
    const unsigned S0 = s0.R + s0.H;
    if (S0 > max_S) max_S = S0;
    const unsigned lo1 = burst_lo1(RL, s0.pf != 0, s0.c > 0), span = burst_span(RL, lo1);
    for (unsigned p = 0; p <= na; ++p) {
        const unsigned R1 = Rf + p;
        if (R1 > (unsigned)RL.wcap) fail("a round's push overflows the ring", s0, p);
        if (R1 > S0) fail("the ring holds more than S at the round's start", s0, p);
        if (R1 > max_ring) max_ring = R1;
        for (unsigned h = 0; h <= na; ++h) {
            ++n_trans;
            St s{R1, h, s0.pf, s0.c};
            const unsigned S = R1 + h;
            if (S > S0 + 64u) fail("S grew by more than 64 in a round", s0, p, h);
            // what follows the round depends on the state after it alone: walked once per such state
            if (seen_post[idx(s)]) continue;
            seen_post[idx(s)] = 1;
            burst_exit(s);   // the give / poll round came due (b_rem == 0)
            if (S - lo1 < span) {   // inside the window: the next round
                push_round(s);
                continue;
            }
            if (S == 0) continue;   // ran dry: the exit above
            if (above_line(RL, S)) {
                if (s.c + (s.pf ? 1u : 0u) + 1u <= CCH) {   // (b_ctop + SPILL <= CCAP, b_ctop not yet holding the prefetch)
                    ++n_spills;
                    chunk_out(s, "a spill found no whole chunk in the ring");
                    if (above_line(RL, s.R + s.H)) fail("one spill did not restore S <= line", s, p, h);
                    push_round(s);
                }
                // cellar full: the burst ends (the exit above)
            } else if (s.pf) {
                ++n_lands;
                if (S > (unsigned)RL.pf_below) fail("a landing above the landing line", s, p, h);
                s.R += RING_CHUNK;
                s.pf = 0;
                if (s.R > (unsigned)RL.wcap) fail("a landing overflows the ring", s, p, h);
                if (above_line(RL, s.R + s.H)) fail("a landing crosses the line", s, p, h);
                push_round(s);
            } else if (s.c > 0) {
                s.pf = 1;
                s.c -= 1;
                push_round(s);
            } else {
                fail("left the window with nothing to do", s, p, h);
            }
        }
    }
}

void outer_from(St s) {
    // the loop's top: a landing
    if (s.pf && s.R <= (unsigned)RL.pf_below) {
        s.R += RING_CHUNK;
        s.pf = 0;
        if (s.R > (unsigned)RL.wcap || above_line(RL, s.R)) fail("an outer landing crosses the line", s);
        ++n_lands;
    }
    if (s.R == 0) {
        if (s.c > 0) {   // the cellar's top chunks, at most `refill` pairs
            const unsigned kc = std::min(s.c, (unsigned)RL.refill / RING_CHUNK);
            St t{kc * RING_CHUNK, 0, s.pf, s.c - kc};
            if (above_line(RL, t.R)) fail("a refill crosses the line", t);
            push_outer(t);
            return;
        }
        // pool takes (<= refill pairs) and seedings (<= 128 pairs: one or two per lane), any count
        const unsigned most = std::max((unsigned)RL.refill, std::min(128u, (unsigned)RL.line));
        for (unsigned n = 1; n <= most; ++n) push_outer(St{n, 0, s.pf, 0});
        return;
    }
    if (above_line(RL, s.R)) {
        chunk_out(s, "the outer overflow path found no whole chunk");
        push_outer(s);
        return;
    }
    // a donation or a give of half the ring (both optional), then on with the rest
    if (s.R / 2u > (unsigned)RL.wcap / 2u) fail("a give above half a ring", s);
    if (s.R >= 2u) push_outer(St{s.R - s.R / 2u, 0, s.pf, s.c});
    if (s.c > 0 && !s.pf && s.R <= (unsigned)RL.pf_issue) {
        s.pf = 1;
        s.c -= 1;
    }
    push_round(s);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s WCAP LINE PF_ISSUE PF_BELOW REFILL [--no-exit-drain]\n", argv[0]);
        return 2;
    }
    RL = RingLines{std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])};
    exit_drain = !(argc > 6 && std::strcmp(argv[6], "--no-exit-drain") == 0);
    if (!ring_lines_valid(RL)) {
        std::printf("INVALID lines\n");
        return 2;
    }
    RMAX = (unsigned)RL.wcap;
    const size_t n = ((size_t)(RMAX + 1u) * 65u) * 2u * (CCH + 1u);
    seen_round.assign(n, 0);
    seen_outer.assign(n, 0);
    seen_post.assign(n, 0);
    push_outer(St{0, 0, 0, 0});
    while (!work_round.empty() || !work_outer.empty()) {
        if (!work_outer.empty()) {
            const St s = work_outer.back();
            work_outer.pop_back();
            ++n_states;
            outer_from(s);
        } else {
            const St s = work_round.back();
            work_round.pop_back();
            ++n_states;
            round_from(s);
        }
    }
    std::printf("OK states=%llu transitions=%llu spills=%llu landings=%llu exits=%llu exit_moves=%llu max_ring=%u max_S=%u\n",
                n_states, n_trans, n_spills, n_lands, n_exits, n_exit_moves, max_ring, max_S);
    return 0;
}
