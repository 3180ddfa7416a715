// aq_batch_plan.h -- the batch pipelines as data, the host batch's (aq_integrate_batch, _params, _err) and the
// device-resident one's (aq_integrate_batch_device): every step of a call in the order the host issues it,
// with its stream, the events it waits for and the one it records, and beside the step kinds the table of what
// each reads and writes. One vocabulary, two builders: batch_plan and device_batch_plan. run_plan (aq_abi.inc)
// walks either and holds no ordering rule of its own; tests/test_batch_plan.py and
// tests/test_device_batch_plan.py check the plans against restatements of the schedules and prove from the
// table that every reuse of a ring is ordered.
//
// Plain host C++17, no HIP: the CPU tests build it with g++.
#pragma once
#include <vector>

#include "aq_shape.h"

namespace aq {

// Four device streams of the context, the caller's stream (device batch) and the host. The host batch's middle
// chunks' copies and pre-passes have streams of their own, whose work overlaps the previous launch; the first
// chunk's copy and pre-pass and the last chunk's copy back run on the context's stream, in order with the
// launches, where a wait across streams costs the device ~20-60 us between the two operations (profiles/r06o:
// copy -> estimate 18 us, scatter -> launch 17 us, gather -> last copy back 62 us, against ~7 us in order).
enum class BStream : int { CTX, H2D, D2H, PRE, CALLER, HOST };

enum class BKind : int {
    JOIN_IN,     // caller's stream: records ev_in behind everything the caller enqueued so far
    START,       // context's stream: waits for ev_in (if any), records ev_start behind the work already there
    FENCE,       // s_pre starts behind ev_start: the caller's inputs are complete, and a pending launch may still
                 // read or write the job-size hint the first pre-pass may preset
    ZERO,        // zero the size-class counts and estimate sums, both parities (sorted calls)
    STAGE,       // host: check the chunk's rows and stage them in the pinned input (a bad row ends the call)
    H2D,         // the chunk's bounds (and theta rows) into their device rings
    CHECK,       // k_dev_check: the chunk's rows from the caller's arrays, checked, into the bounds (theta) ring
                 // -- an invalid row as the empty interval [0, 0] with a zeroed theta row -- and its flag ring
    PRE,         // size pre-pass of a sorted chunk: estimate, scatter into size order (and theta behind it)
    LAUNCH,      // the chunk's persistent launch, from the size-ordered rows if sorted, else from the bounds ring
    GATHER,      // the slots' rows (and error sums) into the row rings, in input order; returns the slots to zero
    GATHER_SOA,  // k_gather_reset_soa: the slots' results into the caller's output arrays in input order, the
                 // slots back to zero
    D2H,         // the rows (and error rows) into the pinned output
    WAIT,        // host: until the chunk's rows are in the pinned output
    UNPACK,      // host: the pinned rows into the caller's arrays
    JOIN_OUT,    // caller's stream: waits for ev_out, recorded behind the last gather
    DRAIN,       // host: until all four streams are idle (always reached, also by a failed call)
};

constexpr int BATCH_SORT_MIN = 64;   // smaller chunks keep their order (few enough for the per-CU instance)

struct BatchStep {
    BKind kind;
    int chunk;         // -1: the call's
    BStream stream;
    int wait[2];       // events waited for on `stream` before the step (-1: none)
    int record;        // event recorded on `stream` behind it (-1: none)
};

// A plan's events, by what they mark: per chunk that its rows are in the bounds ring (the copy's or the
// check's), in size order, gathered, and on the host; per call the start, the zeroing, and the two joins.
enum class BEv : int { FED, PRE, GATH, D2H, START, ZERO, IN, OUT };

struct BatchPlan {
    std::vector<int> chunks;
    std::vector<char> sorted, preset;   // per chunk: runs in size order; its pre-pass presets the job size
    std::vector<int> first_slot;        // per chunk: its launch's first slot (host batch: 0)
    bool theta = false, err = false;    // theta rows travel with the bounds; error rows / ERR launches
    std::vector<BatchStep> steps;
    // The host batch has all four events per chunk and START, ZERO per call (4 nc + 2); the device batch has
    // no copy back, and the joins' two (3 nc + 4).
    int per_chunk = 4, per_call = 2;
    int nc() const { return (int)chunks.size(); }
    int ev(BEv what, int c = -1) const {
        return what < BEv::START ? per_chunk * c + (int)what : per_chunk * nc() + (int)what - (int)BEv::START;
    }
    int n_events() const { return per_chunk * nc() + per_call; }
};

// A launch of fewer than PCU_MAXK integrals into slots below NPARTS is a per-CU launch, whose bounds are
// kernel arguments from the host (aq_launch_plan.h plan_launch). The device batch has no bounds on the host,
// so such a chunk goes into slots from NPARTS: plan_launch then picks a bulk instance, which reads the bounds
// (and theta) from device memory.
inline int device_batch_first_slot(int rows) { return rows < PCU_MAXK ? NPARTS : 0; }

// What the two builders share. `fresh`: the context holds no measured job-size hint for the call's workload.
//
// Preset chunks: the pre-pass of a sorted chunk sets its launch's job size from its estimates (k_batch_scatter
// writes the job-size hint, LaunchHint) while the workload is still fresh, that is until a launch of the call
// has measured a hint: plan_launch (aq_launch_plan.h) makes the hint valid for every unsharded launch of k >=
// PCU_MAXK, and launch_stream (aq_abi.inc) commits that state as it enqueues -- the rule here restates the two.
// The hint is not in the resource table below: a preset pre-pass has only static launches of its own call
// before it, which neither read nor write the hint, and the caller's earlier ones behind ev_start.
//
// Every device ring holds two chunks (parity c & 1), so chunk c's feed writes what chunk c - 2 used and waits
// for ev(GATH, c - 2): the readers of the bounds, theta and flag rings (pre-pass, launch, gather) and of the
// size order its pre-pass will overwrite (launch, gather) are done at that gather.
// The size-class counts are one chain: chunk c's scatter zeroes the other parity's for chunk c + 1, whose
// pre-pass follows it on s_pre -- chunk 1's follows chunk 0's on the context's stream through ev(PRE, 0),
// or, behind an unsorted chunk 0, the call's zeroing through ev(ZERO) (it had added into counts
// not yet zeroed). A later first pre-pass follows the zeroing through its feed's wait for a gather.
struct PlanBuilder {
    BatchPlan p;
    PlanBuilder(const std::vector<int>& chunks, bool sort, bool theta, bool err, bool fresh, bool device) {
        p.chunks = chunks;
        p.theta = theta;
        p.err = err;
        if (device) p.per_chunk = 3, p.per_call = 4;
        for (int m : chunks) {
            p.sorted.push_back(sort && m >= BATCH_SORT_MIN);
            p.preset.push_back(p.sorted.back() && fresh);
            p.first_slot.push_back(device ? device_batch_first_slot(m) : 0);
            fresh = fresh && m < PCU_MAXK;
        }
    }
    void add(BKind k, int c, BStream s, int w0 = -1, int w1 = -1, int rec = -1) {
        p.steps.push_back(BatchStep{k, c, s, {w0, w1}, rec});
    }
    // the call's start on the context's stream, behind ev_in if the caller has a stream to join
    void open(bool sort, int ev_in) {
        add(BKind::START, -1, BStream::CTX, ev_in, -1, p.ev(BEv::START));
        add(BKind::FENCE, -1, BStream::PRE, p.ev(BEv::START));
        if (sort) add(BKind::ZERO, -1, BStream::CTX, -1, -1, p.nc() && !p.sorted[0] ? p.ev(BEv::ZERO) : -1);
    }
    // chunk c's pre-pass, behind `fed` (-1: its feed ran on the same stream) and the counts chain
    void pre(int c, int fed) {
        if (!p.sorted[c]) return;
        add(BKind::PRE, c, c == 0 ? BStream::CTX : BStream::PRE, fed,
            c == 1 ? (p.sorted[0] ? p.ev(BEv::PRE, 0) : p.ev(BEv::ZERO)) : -1, p.ev(BEv::PRE, c));
    }
    void launch(int c) { add(BKind::LAUNCH, c, BStream::CTX, p.ev(p.sorted[c] ? BEv::PRE : BEv::FED, c)); }
    int gathered(int c) const { return c >= 0 ? p.ev(BEv::GATH, c) : -1; }
};

// The host batch's steps in host issue order, for its chunk sizes, the sort switch, whether theta rows and
// error rows travel, and `fresh`. Chunk c's gather also waits for ev(D2H, c - 2), the copy back of the rows it
// overwrites. (Implied: the host waited for it one iteration earlier, before it issued this gather. Kept as
// it was.)
inline BatchPlan batch_plan(const std::vector<int>& chunks, bool sort, bool theta, bool err, bool fresh) {
    PlanBuilder b(chunks, sort, theta, err, fresh, false);
    const BatchPlan& p = b.p;
    const int nc = p.nc();
    // chunk c's rows to the device and into size order: before the first launch, then while chunk c - 1 runs
    auto feed = [&](int c) {
        b.add(BKind::STAGE, c, BStream::HOST);
        b.add(BKind::H2D, c, c == 0 ? BStream::CTX : BStream::H2D, b.gathered(c - 2), -1, p.ev(BEv::FED, c));
        b.pre(c, p.ev(BEv::FED, c));
    };
    b.open(sort, -1);
    if (nc) feed(0);
    for (int c = 0; c < nc; ++c) {
        b.launch(c);
        b.add(BKind::GATHER, c, BStream::CTX, c >= 2 ? p.ev(BEv::D2H, c - 2) : -1, -1, p.ev(BEv::GATH, c));
        if (c + 1 < nc) feed(c + 1);
        b.add(BKind::D2H, c, c + 1 == nc ? BStream::CTX : BStream::D2H, p.ev(BEv::GATH, c), -1, p.ev(BEv::D2H, c));
        if (c > 0) {   // the previous chunk's rows, while this one runs
            b.add(BKind::WAIT, c - 1, BStream::HOST, p.ev(BEv::D2H, c - 1));
            b.add(BKind::UNPACK, c - 1, BStream::HOST);
        }
    }
    b.add(BKind::DRAIN, -1, BStream::HOST);
    if (nc) b.add(BKind::UNPACK, nc - 1, BStream::HOST);
    return b.p;
}

// The device-resident batch's steps in enqueue order; `caller`: the call has a caller's stream to join. No
// step is the host's: the caller's arrays are device memory, the rows are checked, sized, launched and gathered
// into the caller's output arrays by kernels, and the call returns when the last of them is enqueued. Chunk
// c + 1's CHECK and pre-pass are enqueued on s_pre behind chunk c's launch and gather, and run while chunk c's
// launch runs; chunk 0's run on the context's stream, in order with its launch.
inline BatchPlan device_batch_plan(const std::vector<int>& chunks, bool sort, bool theta, bool err, bool fresh,
                                   bool caller) {
    PlanBuilder b(chunks, sort, theta, err, fresh, true);
    const BatchPlan& p = b.p;
    const int nc = p.nc();
    auto feed = [&](int c) {
        b.add(BKind::CHECK, c, c == 0 ? BStream::CTX : BStream::PRE, b.gathered(c - 2), -1, p.ev(BEv::FED, c));
        b.pre(c, -1);
    };
    if (caller) b.add(BKind::JOIN_IN, -1, BStream::CALLER, -1, -1, p.ev(BEv::IN));
    b.open(sort, caller ? p.ev(BEv::IN) : -1);
    if (nc) feed(0);
    for (int c = 0; c < nc; ++c) {
        b.launch(c);
        // (nothing waits for the last gather but the caller's stream)
        b.add(BKind::GATHER_SOA, c, BStream::CTX, -1, -1, c + 1 < nc ? p.ev(BEv::GATH, c) : caller ? p.ev(BEv::OUT) : -1);
        if (c + 1 < nc) feed(c + 1);
    }
    if (caller) b.add(BKind::JOIN_OUT, -1, BStream::CALLER, p.ev(BEv::OUT));
    return b.p;
}

// What a failed step does to the rest of the walk (codes: 0 is success). A failure while a chunk is fed to
// the device -- STAGE (a bad bound), H2D, CHECK, PRE -- skips the rest of that feed and ends the call where the
// chunk would be launched: the running chunk's copy back and the host's unpacking before it still happen. Any
// other failure skips everything after it. DRAIN is always issued; the call returns `rc`. A device plan has no
// DRAIN and nothing between a feed and its launch: the steps issued are those up to the failing one, so what
// was enqueued waits for no event that is never recorded.
struct BatchWalk {
    int rc = 0, rc_feed = 0;
    static bool feeds(BKind k) { return k == BKind::STAGE || k == BKind::H2D || k == BKind::CHECK || k == BKind::PRE; }
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
    BOUNDS, THETA, FLAG, SORTED, THSORTED, PERM, ROWS, ERRROWS,   // device rings, two parities
    CNT, EST,                                                     // size-class counts + cursors, estimate sums; two parities
    KEY,                                                          // size class per row: one buffer
    SLOTS,                                                        // the launch slots' sums (and error sums)
    PIN_IN, PIN_OUT,                                              // the chunk's region of the pinned inputs / outputs
    IN, OUT,                                                      // the chunk's region of the caller's device inputs / outputs
    INVALID, ERRBITS,                                             // the context's invalid-row counter and error-bit word
};
enum class BWhich : int { OWN, OTHER, BOTH, ONE, CHUNK, ALL };   // parity c & 1 | the other | both | the only one |
                                                                 // region c | every chunk's region
enum class BMode : int { READ, WRITE, ADD };   // WRITE: also an update in place; ADD: a device atomic add / or --
                                               // two ADDs commute, neither is ordered
constexpr unsigned IF_THETA = 1, IF_ERR = 2, IF_SORTED = 4, IF_UNSORTED = 8;   // a use's conditions (all must hold)

struct BatchUse {
    BKind kind;
    BRes res;
    BWhich which;
    BMode mode;
    unsigned when;
};

constexpr BatchUse BATCH_USES[] = {
    // (the caller's work before the call writes the inputs, after it reads the outputs and may free or
    // overwrite the inputs)
    {BKind::JOIN_IN, BRes::IN, BWhich::ALL, BMode::WRITE, 0},
    {BKind::JOIN_OUT, BRes::IN, BWhich::ALL, BMode::WRITE, 0},
    {BKind::JOIN_OUT, BRes::OUT, BWhich::ALL, BMode::READ, 0},
    {BKind::ZERO, BRes::CNT, BWhich::BOTH, BMode::WRITE, 0},
    {BKind::ZERO, BRes::EST, BWhich::BOTH, BMode::WRITE, 0},
    {BKind::STAGE, BRes::PIN_IN, BWhich::CHUNK, BMode::WRITE, 0},
    {BKind::H2D, BRes::PIN_IN, BWhich::CHUNK, BMode::READ, 0},
    {BKind::H2D, BRes::BOUNDS, BWhich::OWN, BMode::WRITE, 0},
    {BKind::H2D, BRes::THETA, BWhich::OWN, BMode::WRITE, IF_THETA},
    {BKind::CHECK, BRes::IN, BWhich::CHUNK, BMode::READ, 0},
    {BKind::CHECK, BRes::BOUNDS, BWhich::OWN, BMode::WRITE, 0},
    {BKind::CHECK, BRes::THETA, BWhich::OWN, BMode::WRITE, IF_THETA},
    {BKind::CHECK, BRes::FLAG, BWhich::OWN, BMode::WRITE, 0},
    {BKind::CHECK, BRes::INVALID, BWhich::ONE, BMode::ADD, 0},
    {BKind::PRE, BRes::BOUNDS, BWhich::OWN, BMode::READ, 0},
    {BKind::PRE, BRes::THETA, BWhich::OWN, BMode::READ, IF_THETA},
    {BKind::PRE, BRes::KEY, BWhich::ONE, BMode::WRITE, 0},
    {BKind::PRE, BRes::CNT, BWhich::OWN, BMode::WRITE, 0},     // the estimate adds into them, the scatter scans them
    {BKind::PRE, BRes::EST, BWhich::OWN, BMode::WRITE, 0},
    {BKind::PRE, BRes::CNT, BWhich::OTHER, BMode::WRITE, 0},   // the scatter zeroes the next chunk's
    {BKind::PRE, BRes::EST, BWhich::OTHER, BMode::WRITE, 0},
    {BKind::PRE, BRes::SORTED, BWhich::OWN, BMode::WRITE, 0},
    {BKind::PRE, BRes::PERM, BWhich::OWN, BMode::WRITE, 0},
    {BKind::PRE, BRes::THSORTED, BWhich::OWN, BMode::WRITE, IF_THETA},
    {BKind::LAUNCH, BRes::BOUNDS, BWhich::OWN, BMode::READ, IF_UNSORTED},
    {BKind::LAUNCH, BRes::THETA, BWhich::OWN, BMode::READ, IF_UNSORTED | IF_THETA},
    {BKind::LAUNCH, BRes::SORTED, BWhich::OWN, BMode::READ, IF_SORTED},
    {BKind::LAUNCH, BRes::THSORTED, BWhich::OWN, BMode::READ, IF_SORTED | IF_THETA},
    {BKind::LAUNCH, BRes::SLOTS, BWhich::ONE, BMode::WRITE, 0},
    {BKind::GATHER, BRes::SLOTS, BWhich::ONE, BMode::WRITE, 0},
    {BKind::GATHER, BRes::PERM, BWhich::OWN, BMode::READ, IF_SORTED},
    {BKind::GATHER, BRes::ROWS, BWhich::OWN, BMode::WRITE, 0},
    {BKind::GATHER, BRes::ERRROWS, BWhich::OWN, BMode::WRITE, IF_ERR},
    {BKind::GATHER_SOA, BRes::SLOTS, BWhich::ONE, BMode::WRITE, 0},
    {BKind::GATHER_SOA, BRes::PERM, BWhich::OWN, BMode::READ, IF_SORTED},
    {BKind::GATHER_SOA, BRes::FLAG, BWhich::OWN, BMode::READ, 0},
    {BKind::GATHER_SOA, BRes::OUT, BWhich::CHUNK, BMode::WRITE, 0},
    {BKind::GATHER_SOA, BRes::ERRBITS, BWhich::ONE, BMode::ADD, 0},
    {BKind::D2H, BRes::ROWS, BWhich::OWN, BMode::READ, 0},
    {BKind::D2H, BRes::ERRROWS, BWhich::OWN, BMode::READ, IF_ERR},
    {BKind::D2H, BRes::PIN_OUT, BWhich::CHUNK, BMode::WRITE, 0},
    {BKind::UNPACK, BRes::PIN_OUT, BWhich::CHUNK, BMode::READ, 0},
};

// does step s of plan p make use u?
inline bool use_applies(const BatchPlan& p, const BatchStep& s, const BatchUse& u) {
    if (u.kind != s.kind) return false;
    const bool sorted = s.chunk >= 0 && p.sorted[s.chunk];
    return !((u.when & IF_THETA) && !p.theta) && !((u.when & IF_ERR) && !p.err) && !((u.when & IF_SORTED) && !sorted) &&
           !((u.when & IF_UNSORTED) && sorted);
}

}  // namespace aq
