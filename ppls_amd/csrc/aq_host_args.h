// aq_host_args.h -- the C ABI's argument rules that need no device: the range rules every launch entry point
// shares, the slot-range rule of the gathers, the error code of a slot's error bits, and the batch front
// end's chunk schedule. aq_domain.h holds the integrands' domain predicates (they need the plug-ins).
//
// Plain host C++17, no HIP: the CPU tests build it with g++ (tests/test_host_args.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "aquad.h"
#include "aq_shape.h"

namespace aq {

// a slot's error bits (aq_device.h ERRB_*: aq_abi.inc asserts that they agree)
constexpr unsigned HB_TIMEOUT = 1, HB_OVERFLOW = 2, HB_DEPTH = 4;

inline int err_from_bits(unsigned bits) {
    if (bits & HB_TIMEOUT) return AQ_ETIMEOUT;
    if (bits & HB_OVERFLOW) return AQ_EOVERFLOW;
    if (bits & HB_DEPTH) return AQ_EDEPTH;
    return AQ_OK;
}

inline bool slot_range_ok(int first, int n) { return first >= 0 && n >= 0 && n <= NSLOTS && first < NSLOTS; }

// One launch of k integrals into slots [first_slot, first_slot + k) below slot_limit, as shard `shard` of
// nshards (shard_array: every integral names its own shard, checked by the caller; `shard` is unused).
inline bool launch_ranges_ok(int k, double eps, int max_depth, int shard, int nshards, bool shard_array, int first_slot,
                             int slot_limit) {
    if (k < 1 || k > MAXK) return false;
    if (!(eps >= 0.0) || max_depth < 0 || max_depth > AQ_MAX_LEVELS - 1) return false;
    if (nshards < 1 || nshards > 64) return false;
    if (!shard_array && (shard < 0 || shard >= nshards)) return false;
    return first_slot >= 0 && first_slot <= slot_limit - k;
}

// Chunk sizes of an n-integral batch: a first chunk of `first`, each next one twice the last up to
// MAXK (a chunk's launch then covers the host's checks and staging of the next, ~1.8 ns per integral
// against ~5 ns of kernel), the remainder last -- split so the last chunk is `last` when the remainder
// is large. 0: no small first / last chunk.
inline std::vector<int> batch_chunks(size_t n, size_t first, size_t last) {
    std::vector<int> c;
    size_t done = 0, next = first ? std::min(first, (size_t)MAXK) : (size_t)MAXK;
    while (n - done > next) {
        c.push_back((int)next);
        done += next;
        next = std::min(2 * next, (size_t)MAXK);
    }
    const size_t rem = n - done;
    if (last && rem > 2 * last) {
        c.push_back((int)(rem - last));
        c.push_back((int)last);
    } else if (rem) {
        c.push_back((int)rem);
    }
    return c;
}

// Chunk sizes of an n-row call of the device-resident batch: `chunk` rows each (MAXK, or the AQ_DEVBATCH_CHUNK
// override clamped to [1, MAXK]), the remainder last. No small first or last chunk: there is no host work to hide.
inline int device_batch_chunk_rows(long long env) { return (int)std::min<long long>(std::max<long long>(env, 1), MAXK); }
inline std::vector<int> device_batch_chunks(size_t n, int chunk) {
    std::vector<int> c;
    for (size_t done = 0; done < n; done += (size_t)chunk) c.push_back((int)std::min(n - done, (size_t)chunk));
    return c;
}

// ---- aq_integrate_batch_tol's rules -------------------------------------------------------------------
constexpr double TOL_DEFAULT_SHRINK = 8.0;   // err_abs of the trapezoid rule scales as eps^(2/3): a quarter per round
constexpr int TOL_DEFAULT_ROUNDS = 12;
constexpr int TOL_MAX_ROUNDS = 64;

// the caller's aq_tol with its zeros replaced by the defaults
inline aq_tol tol_defaulted(aq_tol t) {
    if (t.shrink == 0.0) t.shrink = TOL_DEFAULT_SHRINK;
    if (t.max_rounds == 0) t.max_rounds = TOL_DEFAULT_ROUNDS;
    return t;
}

// EPSILON of round r (1-based) of a defaulted aq_tol: eps0 divided by shrink r - 1 times, one IEEE division
// per round (not a power: a caller's loop `eps /= shrink` gives the same bits)
inline double tol_round_eps(const aq_tol& t, int r) {
    double e = t.eps0;
    for (int i = 1; i < r; ++i) e /= t.shrink;
    return e;
}

// the caller's aq_tol (zeros allowed where they mean the default); the last round's EPSILON must still be a
// normal double (a subnormal one has lost bits of the schedule, zero would never refine less)
inline bool tol_args_ok(const aq_tol& t0) {
    if (!(t0.epsabs >= 0.0 && t0.epsrel >= 0.0) || t0.epsabs > 0x1.fffffffffffffp1023 || t0.epsrel > 0x1.fffffffffffffp1023)
        return false;
    if (t0.epsabs == 0.0 && t0.epsrel == 0.0) return false;
    if (!(t0.eps0 > 0.0) || t0.eps0 > 0x1.fffffffffffffp1023) return false;
    if (t0.shrink != 0.0 && !(t0.shrink >= 2.0 && t0.shrink <= 1024.0)) return false;
    if (t0.max_rounds < 0 || t0.max_rounds > TOL_MAX_ROUNDS) return false;
    if (t0.max_depth < 0 || t0.max_depth > AQ_MAX_LEVELS - 1) return false;
    const aq_tol t = tol_defaulted(t0);
    return tol_round_eps(t, t.max_rounds) >= 0x1p-1022;
}

// rows per block of an n-integral call: a whole launch, or the AQ_TOL_BLOCK override within [1, MAXK]
inline int tol_block_rows(long long env) { return env >= 1 && env <= MAXK ? (int)env : MAXK; }

}  // namespace aq
