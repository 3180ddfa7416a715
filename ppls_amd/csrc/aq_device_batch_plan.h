// aq_device_batch_plan.h -- the device-resident batch's pipeline (aq_integrate_batch_device) as data, in the
// manner of aq_batch_plan.h: every step of a call in the order the host ENQUEUES it, with its stream, the
// events it waits for and the one it records, and beside the step kinds the table of what each reads and
// writes. aq_integrate_batch_device (aq_abi.inc) walks the plan and holds no ordering rule of its own;
// tests/test_device_batch_plan.py proves from the table that every reuse of a ring is ordered.
//
// No step is the host's: the caller's arrays are device memory, the rows are checked (k_dev_check), sized,
// launched and gathered into the caller's output arrays (k_gather_reset_soa) by kernels, and the call returns
// when the last of them is enqueued.
//
// Plain host C++17, no HIP: the CPU tests build it with g++.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "aq_batch_plan.h"   // BATCH_SORT_MIN, the size-order rule the two front ends share
#include "aq_shape.h"

namespace aq {

// The context's stream, its pre-pass stream and the caller's stream (none: the call has no JOIN steps).
enum class DStream : int { CTX, PRE, CALLER };

enum class DKind : int {
    JOIN_IN,   // caller's stream: records ev_in behind everything the caller enqueued so far
    START,     // context's stream: waits for ev_in, records ev_start (the caller's work and the context's earlier)
    FENCE,     // s_pre starts behind ev_start: the caller's inputs are complete, and a pending launch of the
               // context may still read or write the job-size hint the first pre-pass may preset
    ZERO,      // zero the size-class counts and estimate sums, both parities (sorted calls)
    CHECK,     // k_dev_check: the chunk's rows from the caller's arrays, checked, into the bounds (theta) ring
               // -- an invalid row as the empty interval [0, 0] with a zeroed theta row -- and its flag ring
    PRE,       // size pre-pass of a sorted chunk: estimate, scatter into size order (and theta behind it)
    LAUNCH,    // the chunk's persistent launch, from the size-ordered rows if sorted, else from the bounds ring
    GATHER,    // k_gather_reset_soa: the slots' results into the caller's output arrays in input order, the
               // slots back to zero
    JOIN_OUT,  // caller's stream: waits for ev_out, recorded behind the last gather
};

struct DevBatchStep {
    DKind kind;
    int chunk;         // -1: the call's
    DStream stream;
    int wait[2];       // events waited for on `stream` before the step (-1: none)
    int record;        // event recorded on `stream` behind it (-1: none)
};

struct DevBatchPlan {
    std::vector<int> chunks;
    std::vector<char> sorted, preset;   // per chunk: runs in size order; its pre-pass presets the job size
    std::vector<int> first_slot;        // per chunk: its launch's first slot (below)
    bool theta = false, err = false, caller = false;
    std::vector<DevBatchStep> steps;
    // three events per chunk -- rows checked into the rings, size order done, results gathered -- and four
    // per call
    int nc() const { return (int)chunks.size(); }
    static int ev_check(int c) { return 3 * c; }
    static int ev_pre(int c) { return 3 * c + 1; }
    static int ev_gath(int c) { return 3 * c + 2; }
    int ev_in() const { return 3 * nc(); }
    int ev_start() const { return 3 * nc() + 1; }
    int ev_zero() const { return 3 * nc() + 2; }
    int ev_out() const { return 3 * nc() + 3; }
    int n_events() const { return 3 * nc() + 4; }
};

// Chunk sizes of an n-row call: `chunk` rows each (MAXK, or the AQ_DEVBATCH_CHUNK override clamped to
// [1, MAXK]), the remainder last. No small first or last chunk: there is no host work to hide.
inline int device_batch_chunk_rows(long long env) { return (int)std::min<long long>(std::max<long long>(env, 1), MAXK); }
inline std::vector<int> device_batch_chunks(size_t n, int chunk) {
    std::vector<int> c;
    for (size_t done = 0; done < n; done += (size_t)chunk) c.push_back((int)std::min(n - done, (size_t)chunk));
    return c;
}

// A launch of fewer than PCU_MAXK integrals into slots below NPARTS is a per-CU launch, whose bounds are
// kernel arguments from the host (aq_launch_plan.h plan_launch). The device batch has no bounds on the host,
// so such a chunk goes into slots from NPARTS: plan_launch then picks a bulk instance, which reads the bounds
// (and theta) from device memory.
inline int device_batch_first_slot(int rows) { return rows < PCU_MAXK ? NPARTS : 0; }

// The call's steps in enqueue order, for its chunk sizes, the sort switch, whether theta rows travel, whether
// the launches are ERR launches, `fresh` (the context holds no measured job-size hint for the call's workload:
// batch_plan's rule for the preset chunks, restated), and whether the call has a caller's stream to join.
//
// Chunk c + 1's CHECK and pre-pass are enqueued on s_pre behind chunk c's launch and gather, and run while
// chunk c's launch runs; chunk 0's run on the context's stream, in order with its launch. Every ring holds
// two chunks (parity c & 1), so chunk c's CHECK, which overwrites what chunk c - 2 used, waits for
// ev_gath(c - 2): the readers of the bounds, theta and flag rings (pre-pass, launch, gather) and of the size
// order its pre-pass will overwrite (launch, gather) are done at that gather. The size-class counts are one
// chain, as in batch_plan: chunk c's scatter zeroes the other parity's for chunk c + 1, whose pre-pass
// follows it on s_pre -- chunk 1's follows chunk 0's on the context's stream through ev_pre(0), or, behind
// an unsorted chunk 0, the call's zeroing through ev_zero.
inline DevBatchPlan device_batch_plan(const std::vector<int>& chunks, bool sort, bool theta, bool err, bool fresh,
                                      bool caller) {
    DevBatchPlan p;
    p.chunks = chunks;
    p.theta = theta;
    p.err = err;
    p.caller = caller;
    const int nc = p.nc();
    for (int c = 0; c < nc; ++c) {
        p.sorted.push_back(sort && chunks[c] >= BATCH_SORT_MIN);
        p.preset.push_back(p.sorted[c] && fresh);
        p.first_slot.push_back(device_batch_first_slot(chunks[c]));
        fresh = fresh && chunks[c] < PCU_MAXK;
    }
    auto add = [&](DKind k, int c, DStream s, int w0 = -1, int w1 = -1, int rec = -1) {
        p.steps.push_back(DevBatchStep{k, c, s, {w0, w1}, rec});
    };
    auto feed = [&](int c) {
        const DStream s = c == 0 ? DStream::CTX : DStream::PRE;
        add(DKind::CHECK, c, s, c >= 2 ? p.ev_gath(c - 2) : -1, -1, p.ev_check(c));
        if (p.sorted[c])   // (behind its check on the same stream)
            add(DKind::PRE, c, s, c == 1 ? (p.sorted[0] ? p.ev_pre(0) : p.ev_zero()) : -1, -1, p.ev_pre(c));
    };
    if (caller) add(DKind::JOIN_IN, -1, DStream::CALLER, -1, -1, p.ev_in());
    add(DKind::START, -1, DStream::CTX, caller ? p.ev_in() : -1, -1, p.ev_start());
    add(DKind::FENCE, -1, DStream::PRE, p.ev_start());
    if (sort) add(DKind::ZERO, -1, DStream::CTX, -1, -1, nc && !p.sorted[0] ? p.ev_zero() : -1);
    if (nc) feed(0);
    for (int c = 0; c < nc; ++c) {
        add(DKind::LAUNCH, c, DStream::CTX, p.sorted[c] ? p.ev_pre(c) : p.ev_check(c));
        // (nothing waits for the last gather but the caller's stream)
        add(DKind::GATHER, c, DStream::CTX, -1, -1, c + 1 < nc ? p.ev_gath(c) : caller ? p.ev_out() : -1);
        if (c + 1 < nc) feed(c + 1);
    }
    if (caller) add(DKind::JOIN_OUT, -1, DStream::CALLER, p.ev_out());
    return p;
}

// ---- what the steps touch ---------------------------------------------------------------------------
enum class DRes : int {
    BOUNDS, THETA, FLAG, SORTED, THSORTED, PERM,   // device rings, two parities
    CNT, EST,                                      // size-class counts + cursors, estimate sums; two parities
    KEY,                                           // size class per row: one buffer
    SLOTS,                                         // the launch slots' sums (and error sums)
    IN, OUT,                                       // the chunk's region of the caller's inputs / outputs
    INVALID, ERRBITS,                              // the context's invalid-row counter and error-bit word
};
enum class DWhich : int { OWN, OTHER, BOTH, ONE, CHUNK, ALL };   // parity c & 1 | the other | both | the only one |
                                                                 // region c | every chunk's region
enum class DMode : int { READ, WRITE, ADD };   // ADD: a device atomic add / or; two ADDs commute, neither is ordered
constexpr unsigned DIF_THETA = 1, DIF_SORTED = 4, DIF_UNSORTED = 8;   // a use's conditions (all must hold)

struct DevBatchUse {
    DKind kind;
    DRes res;
    DWhich which;
    DMode mode;
    unsigned when;
};

constexpr DevBatchUse DEVICE_BATCH_USES[] = {
    // (the caller's work before the call writes the inputs, after it reads the outputs and may free or
    // overwrite the inputs)
    {DKind::JOIN_IN, DRes::IN, DWhich::ALL, DMode::WRITE, 0},
    {DKind::JOIN_OUT, DRes::IN, DWhich::ALL, DMode::WRITE, 0},
    {DKind::JOIN_OUT, DRes::OUT, DWhich::ALL, DMode::READ, 0},
    {DKind::ZERO, DRes::CNT, DWhich::BOTH, DMode::WRITE, 0},
    {DKind::ZERO, DRes::EST, DWhich::BOTH, DMode::WRITE, 0},
    {DKind::CHECK, DRes::IN, DWhich::CHUNK, DMode::READ, 0},
    {DKind::CHECK, DRes::BOUNDS, DWhich::OWN, DMode::WRITE, 0},
    {DKind::CHECK, DRes::THETA, DWhich::OWN, DMode::WRITE, DIF_THETA},
    {DKind::CHECK, DRes::FLAG, DWhich::OWN, DMode::WRITE, 0},
    {DKind::CHECK, DRes::INVALID, DWhich::ONE, DMode::ADD, 0},
    {DKind::PRE, DRes::BOUNDS, DWhich::OWN, DMode::READ, 0},
    {DKind::PRE, DRes::THETA, DWhich::OWN, DMode::READ, DIF_THETA},
    {DKind::PRE, DRes::KEY, DWhich::ONE, DMode::WRITE, 0},
    {DKind::PRE, DRes::CNT, DWhich::OWN, DMode::WRITE, 0},     // the estimate adds into them, the scatter scans them
    {DKind::PRE, DRes::EST, DWhich::OWN, DMode::WRITE, 0},
    {DKind::PRE, DRes::CNT, DWhich::OTHER, DMode::WRITE, 0},   // the scatter zeroes the next chunk's
    {DKind::PRE, DRes::EST, DWhich::OTHER, DMode::WRITE, 0},
    {DKind::PRE, DRes::SORTED, DWhich::OWN, DMode::WRITE, 0},
    {DKind::PRE, DRes::PERM, DWhich::OWN, DMode::WRITE, 0},
    {DKind::PRE, DRes::THSORTED, DWhich::OWN, DMode::WRITE, DIF_THETA},
    {DKind::LAUNCH, DRes::BOUNDS, DWhich::OWN, DMode::READ, DIF_UNSORTED},
    {DKind::LAUNCH, DRes::THETA, DWhich::OWN, DMode::READ, DIF_UNSORTED | DIF_THETA},
    {DKind::LAUNCH, DRes::SORTED, DWhich::OWN, DMode::READ, DIF_SORTED},
    {DKind::LAUNCH, DRes::THSORTED, DWhich::OWN, DMode::READ, DIF_SORTED | DIF_THETA},
    {DKind::LAUNCH, DRes::SLOTS, DWhich::ONE, DMode::WRITE, 0},
    {DKind::GATHER, DRes::SLOTS, DWhich::ONE, DMode::WRITE, 0},
    {DKind::GATHER, DRes::PERM, DWhich::OWN, DMode::READ, DIF_SORTED},
    {DKind::GATHER, DRes::FLAG, DWhich::OWN, DMode::READ, 0},
    {DKind::GATHER, DRes::OUT, DWhich::CHUNK, DMode::WRITE, 0},
    {DKind::GATHER, DRes::ERRBITS, DWhich::ONE, DMode::ADD, 0},
};

// does step s of plan p make use u?
inline bool device_batch_use_applies(const DevBatchPlan& p, const DevBatchStep& s, const DevBatchUse& u) {
    if (u.kind != s.kind) return false;
    const bool sorted = s.chunk >= 0 && p.sorted[s.chunk];
    return !((u.when & DIF_THETA) && !p.theta) && !((u.when & DIF_SORTED) && !sorted) && !((u.when & DIF_UNSORTED) && sorted);
}

}  // namespace aq
