// The device-resident batch's pipeline plan (ppls_amd/csrc/aq_device_batch_plan.h), g++ alone. Built and run by
// tests/test_device_batch_plan.py, which holds the happens-before check.
//   --constants                                   MAXK, PCU_MAXK, NPARTS and BATCH_SORT_MIN as JSON
//   chunks N ENV                                  the chunk sizes of an N-row call under AQ_DEVBATCH_CHUNK=ENV, as JSON
//   plan SORT THETA ERR FRESH CALLER SIZE...      the plan of these chunk sizes as JSON: chunks, sorted, preset,
//                                                 first_slot, and per step kind, chunk, stream, waits, record and
//                                                 uses [mode, resource, instance] (instance: the ring's parity, or
//                                                 the chunk for the regions of the caller's arrays)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aq_device_batch_plan.h"

using namespace aq;

static const char* const KIND[] = {"join_in", "start", "fence", "zero", "check", "pre", "launch", "gather", "join_out"};
static const char* const STREAM[] = {"ctx", "pre", "caller"};
static const char* const RES[] = {"bounds", "theta", "flag", "sorted", "thsorted", "perm", "cnt", "est",
                                  "key", "slots", "in", "out", "invalid", "errbits"};
static const char* const MODE[] = {"r", "w", "add"};

static std::string event_name(const DevBatchPlan& p, int e) {
    if (e == p.ev_in()) return "in";
    if (e == p.ev_start()) return "start";
    if (e == p.ev_zero()) return "zero";
    if (e == p.ev_out()) return "out";
    static const char* const per_chunk[] = {"check", "pre", "gath"};
    return std::string(per_chunk[e % 3]) + ":" + std::to_string(e / 3);
}

static void print_ints(const char* name, const std::vector<int>& v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
    printf("]");
}

static void print_plan(const DevBatchPlan& p) {
    printf("{");
    print_ints("chunks", p.chunks);
    printf(", ");
    print_ints("sorted", std::vector<int>(p.sorted.begin(), p.sorted.end()));
    printf(", ");
    print_ints("preset", std::vector<int>(p.preset.begin(), p.preset.end()));
    printf(", ");
    print_ints("first_slot", p.first_slot);
    printf(", \"n_events\": %d, \"steps\": [", p.n_events());
    bool first_step = true;
    for (const DevBatchStep& s : p.steps) {
        printf("%s{\"kind\": \"%s\", \"chunk\": %d, \"stream\": \"%s\", \"waits\": [", first_step ? "" : ", ",
               KIND[(int)s.kind], s.chunk, STREAM[(int)s.stream]);
        first_step = false;
        bool sep = false;
        for (int w : s.wait)
            if (w >= 0) printf("%s\"%s\"", sep ? ", " : "", event_name(p, w).c_str()), sep = true;
        printf("], \"record\": ");
        if (s.record >= 0) printf("\"%s\"", event_name(p, s.record).c_str());
        else printf("null");
        printf(", \"uses\": [");
        sep = false;
        for (const DevBatchUse& u : DEVICE_BATCH_USES) {
            if (!device_batch_use_applies(p, s, u)) continue;
            const int own = s.chunk & 1;
            std::vector<int> inst;
            switch (u.which) {
                case DWhich::OWN: inst = {own}; break;
                case DWhich::OTHER: inst = {own ^ 1}; break;
                case DWhich::BOTH: inst = {0, 1}; break;
                case DWhich::ONE: inst = {0}; break;
                case DWhich::CHUNK: inst = {s.chunk}; break;
                case DWhich::ALL:
                    for (int c = 0; c < p.nc(); ++c) inst.push_back(c);
                    break;
            }
            for (int i : inst) printf("%s[\"%s\", \"%s\", %d]", sep ? ", " : "", MODE[(int)u.mode], RES[(int)u.res], i), sep = true;
        }
        printf("]}");
    }
    printf("]}\n");
}

int main(int argc, char** argv) {
    static_assert(sizeof(KIND) / sizeof(*KIND) == (size_t)DKind::JOIN_OUT + 1 && sizeof(RES) / sizeof(*RES) == (size_t)DRes::ERRBITS + 1 &&
                      sizeof(STREAM) / sizeof(*STREAM) == (size_t)DStream::CALLER + 1 && sizeof(MODE) / sizeof(*MODE) == (size_t)DMode::ADD + 1,
                  "one name per enumerator");
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("{\"MAXK\": %d, \"PCU_MAXK\": %d, \"NPARTS\": %d, \"BATCH_SORT_MIN\": %d}\n", MAXK, PCU_MAXK, NPARTS, BATCH_SORT_MIN);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "chunks")) {
        printf("{");
        print_ints("chunks", device_batch_chunks((size_t)strtoull(argv[2], nullptr, 10), device_batch_chunk_rows(atoll(argv[3]))));
        printf("}\n");
        return 0;
    }
    if (argc >= 7 && !strcmp(argv[1], "plan")) {
        std::vector<int> chunks;
        for (int i = 7; i < argc; ++i) chunks.push_back(atoi(argv[i]));
        print_plan(device_batch_plan(chunks, atoi(argv[2]) != 0, atoi(argv[3]) != 0, atoi(argv[4]) != 0, atoi(argv[5]) != 0,
                                     atoi(argv[6]) != 0));
        return 0;
    }
    fprintf(stderr, "usage: device_batch_plan_check --constants | chunks N ENV | plan SORT THETA ERR FRESH CALLER SIZE...\n");
    return 2;
}
