// The batch pipelines' plans (ppls_amd/csrc/aq_batch_plan.h), g++ alone. Built and run by tests/batch_plan_util.py
// for tests/test_batch_plan.py and tests/test_device_batch_plan.py, which hold the expected schedules;
// batch_plan_util holds the happens-before check.
//   --constants       MAXK, PCU_MAXK, NPARTS and BATCH_SORT_MIN as JSON
//   chunks N ENV      the chunk sizes of an N-row device-resident call under AQ_DEVBATCH_CHUNK=ENV, as JSON
//   plan CASE         the case's plan as one line of JSON: chunks, sorted, preset, first_slot, n_events, and per
//                     step kind, chunk, stream, waits, record and uses [mode, resource, instance] (instance: the
//                     ring's parity, or the chunk for the regions of the pinned copies and the caller's arrays)
//   walk CASE         the indices of the plan's steps that BatchWalk still issues when step FAIL (-1: none)
//                     returns CODE, then "rc <the call's code>"
//   plan @FILE, walk @FILE     one CASE per line
// CASE, for plan:     host N FIRST LAST SORT THETA ERR FRESH  |  dev SORT THETA ERR FRESH CALLER SIZE...
//       for walk:     host N FIRST LAST SORT FAIL CODE        |  dev SORT CALLER FAIL CODE SIZE...
//                     (a walk's plan has theta rows and error rows and is fresh)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "aq_batch_plan.h"
#include "aq_host_args.h"

using namespace aq;

static const char* const KIND[] = {"join_in", "start", "fence", "zero", "stage", "h2d", "check", "pre", "launch", "gather",
                                   "gather_soa", "d2h", "wait", "unpack", "join_out", "drain"};
static const char* const STREAM[] = {"ctx", "h2d", "d2h", "pre", "caller", "host"};
static const char* const RES[] = {"bounds", "theta", "flag", "sorted", "thsorted", "perm", "rows", "errrows", "cnt", "est",
                                  "key", "slots", "pin_in", "pin_out", "in", "out", "invalid", "errbits"};
static const char* const MODE[] = {"r", "w", "add"};
// (the event behind a chunk's feed prints as the step that records it: the host's copy, the device's check)
static const char* const EVENT[2][8] = {{"h2d", "pre", "gath", "d2h", "start", "zero", "in", "out"},
                                        {"check", "pre", "gath", "d2h", "start", "zero", "in", "out"}};

static std::string event_name(const BatchPlan& p, bool dev, int e) {
    const int c = e / p.per_chunk;
    if (c < p.nc()) return std::string(EVENT[dev][e % p.per_chunk]) + ":" + std::to_string(c);
    return EVENT[dev][(int)BEv::START + e - p.per_chunk * p.nc()];
}

static void print_ints(const char* name, const std::vector<int>& v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
    printf("]");
}

static void print_plan(const BatchPlan& p, bool dev) {
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
    for (const BatchStep& s : p.steps) {
        printf("%s{\"kind\": \"%s\", \"chunk\": %d, \"stream\": \"%s\", \"waits\": [", first_step ? "" : ", ",
               KIND[(int)s.kind], s.chunk, STREAM[(int)s.stream]);
        first_step = false;
        bool sep = false;
        for (int w : s.wait)
            if (w >= 0) printf("%s\"%s\"", sep ? ", " : "", event_name(p, dev, w).c_str()), sep = true;
        printf("], \"record\": ");
        if (s.record >= 0) printf("\"%s\"", event_name(p, dev, s.record).c_str());
        else printf("null");
        printf(", \"uses\": [");
        sep = false;
        for (const BatchUse& u : BATCH_USES) {
            if (!use_applies(p, s, u)) continue;
            const int own = s.chunk & 1;
            std::vector<int> inst;
            switch (u.which) {
                case BWhich::OWN: inst = {own}; break;
                case BWhich::OTHER: inst = {own ^ 1}; break;
                case BWhich::BOTH: inst = {0, 1}; break;
                case BWhich::ONE: inst = {0}; break;
                case BWhich::CHUNK: inst = {s.chunk}; break;
                case BWhich::ALL:
                    for (int c = 0; c < p.nc(); ++c) inst.push_back(c);
                    break;
            }
            for (int i : inst) printf("%s[\"%s\", \"%s\", %d]", sep ? ", " : "", MODE[(int)u.mode], RES[(int)u.res], i), sep = true;
        }
        printf("]}");
    }
    printf("]}\n");
}

// one CASE (above), already split into words; false: not a case
static bool run_case(bool walk, const std::vector<std::string>& w) {
    if (w.empty()) return false;
    const bool dev = w[0] == "dev";
    if (!dev && w[0] != "host") return false;
    std::vector<long long> v;
    for (size_t i = 1; i < w.size(); ++i) v.push_back(atoll(w[i].c_str()));
    if (dev ? v.size() < (walk ? 4u : 5u) : v.size() != (walk ? 6u : 7u)) return false;
    BatchPlan p;
    if (dev) {
        const std::vector<int> chunks(v.begin() + (walk ? 4 : 5), v.end());
        p = walk ? device_batch_plan(chunks, v[0] != 0, true, true, true, v[1] != 0)
                 : device_batch_plan(chunks, v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0);
    } else {
        const std::vector<int> chunks = batch_chunks((size_t)v[0], (size_t)v[1], (size_t)v[2]);
        p = walk ? batch_plan(chunks, v[3] != 0, true, true, true) : batch_plan(chunks, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0);
    }
    if (!walk) {
        print_plan(p, dev);
        return true;
    }
    const long long fail = v[dev ? 2 : 4], code = v[dev ? 3 : 5];
    BatchWalk bw;
    for (size_t i = 0; i < p.steps.size(); ++i) {
        if (!bw.runs(p.steps[i])) continue;
        printf("%zu ", i);
        bw.done(p.steps[i], (long long)i == fail ? (int)code : 0);
    }
    printf("rc %d\n", bw.rc);
    return true;
}

static std::vector<std::string> words(const char* line) {
    std::vector<std::string> w;
    for (const char* s = line; *s;) {
        const size_t n = strcspn(s, " \t\r\n");
        if (n) w.emplace_back(s, n);
        s += n + (s[n] ? 1 : 0);
    }
    return w;
}

int main(int argc, char** argv) {
    static_assert(sizeof(KIND) / sizeof(*KIND) == (size_t)BKind::DRAIN + 1 && sizeof(RES) / sizeof(*RES) == (size_t)BRes::ERRBITS + 1 &&
                      sizeof(STREAM) / sizeof(*STREAM) == (size_t)BStream::HOST + 1 && sizeof(MODE) / sizeof(*MODE) == (size_t)BMode::ADD + 1 &&
                      sizeof(EVENT[0]) / sizeof(*EVENT[0]) == (size_t)BEv::OUT + 1,
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
    const bool walk = argc >= 3 && !strcmp(argv[1], "walk");
    if (argc >= 3 && (walk || !strcmp(argv[1], "plan"))) {
        if (argv[2][0] != '@') {
            if (run_case(walk, std::vector<std::string>(argv + 2, argv + argc))) return 0;
        } else if (FILE* f = argc == 3 ? fopen(argv[2] + 1, "r") : nullptr) {
            int rows = 0;
            char line[4096];
            bool ok = true;
            while (ok && fgets(line, sizeof line, f)) ok = run_case(walk, words(line)), rows += ok;
            fclose(f);
            if (ok && rows) return 0;
            fprintf(stderr, "unreadable row after %d rows\n", rows);
            return 2;
        }
    }
    fprintf(stderr, "usage: batch_plan_check --constants | chunks N ENV | plan CASE | plan @FILE | walk CASE | walk @FILE\n");
    return 2;
}
