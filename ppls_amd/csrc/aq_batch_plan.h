// aq_batch_plan.h -- the batch front end's pipeline (aq_integrate_batch, _params, _err) as data: every step
// of a call in the order the host issues it, with its stream, the events it waits for and the one it
// records, and beside the step kinds the table of what each reads and writes. batch_run (aq_abi.inc)
// walks the plan and holds no ordering rule of its own; tests/test_batch_plan.py checks the plan against a
// restatement of the schedule and proves from the table that every reuse of a ring is ordered.
//
// Plain host C++17, no HIP: the CPU tests build it with g++.
#pragma once
#include <vector>

#include "aq_shape.h"

namespace aq {

// Four device streams and the host. The middle chunks' copies and pre-passes have streams of their own,
// whose work overlaps the previous launch; the first chunk's copy and pre-pass and the last chunk's copy
// back run on the context's stream, in order with the launches, where a wait across streams costs the
// device ~20-60 us between the two operations (profiles/r06o: copy -> estimate 18 us, scatter -> launch
// 17 us, gather -> last copy back 62 us, against ~7 us in order).
enum class BStream : int { CTX, H2D, D2H, PRE, HOST };

enum class BKind : int {
    START,    // records ev_start behind the work already on the context's stream
    FENCE,    // s_pre starts behind ev_start: a caller's pending launch may still read or write the job-size
              // hint the first pre-pass may preset
    ZERO,     // zero the size-class counts and estimate sums, both parities (sorted calls)
    STAGE,    // host: check the chunk's rows and stage them in the pinned input (a bad row ends the call)
    H2D,      // the chunk's bounds (and theta rows) into their device rings
    PRE,      // size pre-pass of a sorted chunk: estimate, scatter into size order (and theta behind it)
    LAUNCH,   // the chunk's persistent launch, from the size-ordered rows if sorted, else from the bounds ring
    GATHER,   // the slots' rows (and error sums) into the row rings, in input order; returns the slots to zero
    D2H,      // the rows (and error rows) into the pinned output
    WAIT,     // host: until the chunk's rows are in the pinned output
    UNPACK,   // host: the pinned rows into the caller's arrays
    DRAIN,    // host: until all four streams are idle (always reached, also by a failed call)
};

constexpr int BATCH_SORT_MIN = 64;   // smaller chunks keep their order (few enough for the per-CU instance)

struct BatchStep {
    BKind kind;
    int chunk;         // -1: the call's
    BStream stream;
    int wait[2];       // events waited for on `stream` before the step (-1: none)
    int record;        // event recorded on `stream` behind it (-1: none)
};

struct BatchPlan {
    std::vector<int> chunks;
    std::vector<char> sorted, preset;   // per chunk: runs in size order; its pre-pass presets the job size
    bool theta = false, err = false;    // theta rows / error rows travel with the bounds / rows
    std::vector<BatchStep> steps;
    // four events per chunk -- bounds on the device, rows gathered, rows on the host, size order done -- and
    // two per call
    int nc() const { return (int)chunks.size(); }
    static int ev_h2d(int c) { return 4 * c; }
    static int ev_gath(int c) { return 4 * c + 1; }
    static int ev_d2h(int c) { return 4 * c + 2; }
    static int ev_pre(int c) { return 4 * c + 3; }
    int ev_start() const { return 4 * nc(); }
    int ev_zero() const { return 4 * nc() + 1; }
    int n_events() const { return 4 * nc() + 2; }
};

// The call's steps in host issue order, for its chunk sizes, the sort switch, whether theta rows and error
// rows travel, and `fresh`: the context holds no measured job-size hint for the call's workload.
//
// Preset chunks: the pre-pass of a sorted chunk sets its launch's job size from its estimates (k_batch_scatter
// writes the job-size hint, LaunchHint) while the workload is still fresh, that is until a launch of the call
// has measured a hint: plan_launch (aq_launch_plan.h) makes the hint valid for every unsharded launch of k >=
// PCU_MAXK, and launch_stream (aq_abi.inc) commits that state as it enqueues -- the rule here restates the two.
// The hint is not in the resource table below: a preset pre-pass has only static launches of its own call
// before it, which neither read nor write the hint, and the caller's earlier ones behind ev_start.
//
// Every device ring holds two chunks (parity c & 1), so chunk c writes what chunk c - 2 used:
//   * its copy waits for ev_gath(c - 2) -- the readers of the bounds and theta rings (pre-pass, launch) and
//     of the size order its pre-pass will overwrite (launch, gather) are done at that gather;
//   * its gather waits for ev_d2h(c - 2), the copy back of the rows it overwrites. (Implied: the host
//     waited for ev_d2h(c - 2) one iteration earlier, before it issued this gather. Kept as it was.)
// The size-class counts are one chain: chunk c's scatter zeroes the other parity's for chunk c + 1, whose
// pre-pass follows it on s_pre -- chunk 1's follows chunk 0's on the context's stream through ev_pre(0),
// or, behind an unsorted chunk 0, the call's zeroing through ev_zero (it had added into counts
// not yet zeroed). A later first pre-pass follows the zeroing through its copy's wait for a gather.
inline BatchPlan batch_plan(const std::vector<int>& chunks, bool sort, bool theta, bool err, bool fresh) {
    BatchPlan p;
    p.chunks = chunks;
    p.theta = theta;
    p.err = err;
    const int nc = p.nc();
    for (int c = 0; c < nc; ++c) {
        p.sorted.push_back(sort && chunks[c] >= BATCH_SORT_MIN);
        p.preset.push_back(p.sorted[c] && fresh);
        fresh = fresh && chunks[c] < PCU_MAXK;
    }
    auto add = [&](BKind k, int c, BStream s, int w0 = -1, int w1 = -1, int rec = -1) {
        p.steps.push_back(BatchStep{k, c, s, {w0, w1}, rec});
    };
    // chunk c's rows to the device and into size order: before the first launch, then while chunk c - 1 runs
    auto feed = [&](int c) {
        add(BKind::STAGE, c, BStream::HOST);
        add(BKind::H2D, c, c == 0 ? BStream::CTX : BStream::H2D, c >= 2 ? p.ev_gath(c - 2) : -1, -1, p.ev_h2d(c));
        if (p.sorted[c])
            add(BKind::PRE, c, c == 0 ? BStream::CTX : BStream::PRE, p.ev_h2d(c),
                c == 1 ? (p.sorted[0] ? p.ev_pre(0) : p.ev_zero()) : -1, p.ev_pre(c));
    };
    add(BKind::START, -1, BStream::CTX, -1, -1, p.ev_start());
    add(BKind::FENCE, -1, BStream::PRE, p.ev_start());
    if (sort) add(BKind::ZERO, -1, BStream::CTX, -1, -1, nc && !p.sorted[0] ? p.ev_zero() : -1);
    if (nc) feed(0);
    for (int c = 0; c < nc; ++c) {
        add(BKind::LAUNCH, c, BStream::CTX, p.sorted[c] ? p.ev_pre(c) : p.ev_h2d(c));
        add(BKind::GATHER, c, BStream::CTX, c >= 2 ? p.ev_d2h(c - 2) : -1, -1, p.ev_gath(c));
        if (c + 1 < nc) feed(c + 1);
        add(BKind::D2H, c, c + 1 == nc ? BStream::CTX : BStream::D2H, p.ev_gath(c), -1, p.ev_d2h(c));
        if (c > 0) {   // the previous chunk's rows, while this one runs
            add(BKind::WAIT, c - 1, BStream::HOST, p.ev_d2h(c - 1));
            add(BKind::UNPACK, c - 1, BStream::HOST);
        }
    }
    add(BKind::DRAIN, -1, BStream::HOST);
    if (nc) add(BKind::UNPACK, nc - 1, BStream::HOST);
    return p;
}

// What a failed step does to the rest of the walk (codes: 0 is success). A failure while a chunk is fed to
// the device -- STAGE (a bad bound), H2D, PRE -- skips the rest of that feed and ends the call where the chunk
// would be launched: the running chunk's copy back and the host's unpacking before it still happen. Any other
// failure skips everything after it. DRAIN is always issued; the call returns `rc`.
struct BatchWalk {
    int rc = 0, rc_feed = 0;
    static bool feeds(BKind k) { return k == BKind::STAGE || k == BKind::H2D || k == BKind::PRE; }
    // is s issued? (asked once per step, in order)
    bool runs(const BatchStep& s) {
        if (s.kind == BKind::LAUNCH && rc == 0) rc = rc_feed;
        return s.kind == BKind::DRAIN || (rc == 0 && !(feeds(s.kind) && rc_feed != 0));
    }
    // s was issued and returned r
    void done(const BatchStep& s, int r) {
        if (feeds(s.kind)) rc_feed = r;
        else if (rc == 0) rc = r;
    }
};

// ---- what the steps touch ---------------------------------------------------------------------------
enum class BRes : int {
    BOUNDS, THETA, SORTED, THSORTED, PERM, ROWS, ERRROWS,   // device rings, two parities
    CNT, EST,                                               // size-class counts + cursors, estimate sums; two parities
    KEY,                                                    // size class per row: one buffer
    SLOTS,                                                  // the launch slots' sums (and error sums)
    PIN_IN, PIN_OUT,                                        // the chunk's region of the pinned inputs / outputs
};
enum class BWhich : int { OWN, OTHER, BOTH, ONE, CHUNK };   // parity c & 1 | the other | both | the only one | region c
constexpr unsigned IF_THETA = 1, IF_ERR = 2, IF_SORTED = 4, IF_UNSORTED = 8;   // a use's conditions (all must hold)

struct BatchUse {
    BKind kind;
    BRes res;
    BWhich which;
    bool write;      // (a step that updates in place writes)
    unsigned when;
};

constexpr BatchUse BATCH_USES[] = {
    {BKind::ZERO, BRes::CNT, BWhich::BOTH, true, 0},
    {BKind::ZERO, BRes::EST, BWhich::BOTH, true, 0},
    {BKind::STAGE, BRes::PIN_IN, BWhich::CHUNK, true, 0},
    {BKind::H2D, BRes::PIN_IN, BWhich::CHUNK, false, 0},
    {BKind::H2D, BRes::BOUNDS, BWhich::OWN, true, 0},
    {BKind::H2D, BRes::THETA, BWhich::OWN, true, IF_THETA},
    {BKind::PRE, BRes::BOUNDS, BWhich::OWN, false, 0},
    {BKind::PRE, BRes::THETA, BWhich::OWN, false, IF_THETA},
    {BKind::PRE, BRes::KEY, BWhich::ONE, true, 0},
    {BKind::PRE, BRes::CNT, BWhich::OWN, true, 0},     // the estimate adds into them, the scatter scans them
    {BKind::PRE, BRes::EST, BWhich::OWN, true, 0},
    {BKind::PRE, BRes::CNT, BWhich::OTHER, true, 0},   // the scatter zeroes the next chunk's
    {BKind::PRE, BRes::EST, BWhich::OTHER, true, 0},
    {BKind::PRE, BRes::SORTED, BWhich::OWN, true, 0},
    {BKind::PRE, BRes::PERM, BWhich::OWN, true, 0},
    {BKind::PRE, BRes::THSORTED, BWhich::OWN, true, IF_THETA},
    {BKind::LAUNCH, BRes::BOUNDS, BWhich::OWN, false, IF_UNSORTED},
    {BKind::LAUNCH, BRes::THETA, BWhich::OWN, false, IF_UNSORTED | IF_THETA},
    {BKind::LAUNCH, BRes::SORTED, BWhich::OWN, false, IF_SORTED},
    {BKind::LAUNCH, BRes::THSORTED, BWhich::OWN, false, IF_SORTED | IF_THETA},
    {BKind::LAUNCH, BRes::SLOTS, BWhich::ONE, true, 0},
    {BKind::GATHER, BRes::SLOTS, BWhich::ONE, true, 0},
    {BKind::GATHER, BRes::PERM, BWhich::OWN, false, IF_SORTED},
    {BKind::GATHER, BRes::ROWS, BWhich::OWN, true, 0},
    {BKind::GATHER, BRes::ERRROWS, BWhich::OWN, true, IF_ERR},
    {BKind::D2H, BRes::ROWS, BWhich::OWN, false, 0},
    {BKind::D2H, BRes::ERRROWS, BWhich::OWN, false, IF_ERR},
    {BKind::D2H, BRes::PIN_OUT, BWhich::CHUNK, true, 0},
    {BKind::UNPACK, BRes::PIN_OUT, BWhich::CHUNK, false, 0},
};

// does step s of plan p make use u?
inline bool batch_use_applies(const BatchPlan& p, const BatchStep& s, const BatchUse& u) {
    if (u.kind != s.kind) return false;
    const bool sorted = s.chunk >= 0 && p.sorted[s.chunk];
    return !((u.when & IF_THETA) && !p.theta) && !((u.when & IF_ERR) && !p.err) && !((u.when & IF_SORTED) && !sorted) &&
           !((u.when & IF_UNSORTED) && sorted);
}

}  // namespace aq
