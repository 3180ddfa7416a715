// The batch front end's pipeline plan (ppls_amd/csrc/aq_batch_plan.h), g++ alone. Built and run by
// tests/test_batch_plan.py, which holds the expected schedule and the happens-before check.
//   --constants     MAXK, PCU_MAXK and BATCH_SORT_MIN as JSON
//   plan FILE       one "n first last sort theta err fresh" per line -> per case
//                     case <the line>
//                     chunks <sizes>
//                     <kind> <chunk> <stream> <sorted><preset> <waits,|-> <record|-> <uses,|->    per step
//                     end
//   walk FILE       one "n first last sort fail code" per line -> the indices of the plan's steps that BatchWalk
//                   still issues when step `fail` (-1: none) returns `code`, then "rc <the call's code>"
//                   events print as h2d:c gath:c d2h:c pre:c start zero, uses as r:res:i / w:res:i (i: the
//                   ring's parity, or the chunk for the pinned regions)
#include <cstdio>
#include <cstring>
#include <string>

#include "aq_batch_plan.h"
#include "aq_host_args.h"

using namespace aq;

static const char* const KIND[] = {"start", "fence", "zero", "stage", "h2d", "pre", "launch", "gather", "d2h", "wait",
                                   "unpack", "drain"};
static const char* const STREAM[] = {"ctx", "h2d", "d2h", "pre", "host"};
static const char* const RES[] = {"bounds", "theta", "sorted", "thsorted", "perm", "rows", "errrows", "cnt", "est",
                                  "key", "slots", "pin_in", "pin_out"};

static std::string event_name(const BatchPlan& p, int e) {
    if (e < 0) return "-";
    if (e == p.ev_start()) return "start";
    if (e == p.ev_zero()) return "zero";
    static const char* const per_chunk[] = {"h2d", "gath", "d2h", "pre"};
    return std::string(per_chunk[e % 4]) + ":" + std::to_string(e / 4);
}

static void print_plan(const BatchPlan& p) {
    printf("chunks");
    for (int m : p.chunks) printf(" %d", m);
    printf("\n");
    for (const BatchStep& s : p.steps) {
        const bool of_chunk = s.chunk >= 0;
        printf("%s %d %s %d%d ", KIND[(int)s.kind], s.chunk, STREAM[(int)s.stream], of_chunk && p.sorted[s.chunk] ? 1 : 0,
               of_chunk && p.preset[s.chunk] ? 1 : 0);
        std::string waits;
        for (int w : s.wait)
            if (w >= 0) waits += (waits.empty() ? "" : ",") + event_name(p, w);
        printf("%s %s ", waits.empty() ? "-" : waits.c_str(), event_name(p, s.record).c_str());
        std::string uses;
        for (const BatchUse& u : BATCH_USES) {
            if (!batch_use_applies(p, s, u)) continue;
            const int own = s.chunk & 1;
            int inst[2] = {0, -1};
            switch (u.which) {
                case BWhich::OWN: inst[0] = own; break;
                case BWhich::OTHER: inst[0] = own ^ 1; break;
                case BWhich::BOTH: inst[1] = 1; break;
                case BWhich::ONE: break;
                case BWhich::CHUNK: inst[0] = s.chunk; break;
            }
            for (int i : inst)
                if (i >= 0)
                    uses += (uses.empty() ? "" : ",") + std::string(u.write ? "w:" : "r:") + RES[(int)u.res] + ":" +
                            std::to_string(i);
        }
        printf("%s\n", uses.empty() ? "-" : uses.c_str());
    }
    printf("end\n");
}

int main(int argc, char** argv) {
    static_assert(sizeof(KIND) / sizeof(*KIND) == (size_t)BKind::DRAIN + 1 && sizeof(RES) / sizeof(*RES) == (size_t)BRes::PIN_OUT + 1 &&
                      sizeof(STREAM) / sizeof(*STREAM) == (size_t)BStream::HOST + 1,
                  "one name per enumerator");
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("{\"MAXK\": %d, \"PCU_MAXK\": %d, \"BATCH_SORT_MIN\": %d}\n", MAXK, PCU_MAXK, BATCH_SORT_MIN);
        return 0;
    }
    const bool walk = argc == 3 && !strcmp(argv[1], "walk");
    FILE* f = argc == 3 && (walk || !strcmp(argv[1], "plan")) ? fopen(argv[2], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: batch_plan_check --constants | plan FILE | walk FILE\n");
        return 2;
    }
    int rows = 0;
    unsigned long long n, first, last;
    int sort, theta, err, fresh;
    int fail, code;
    while (walk && fscanf(f, "%llu %llu %llu %d %d %d", &n, &first, &last, &sort, &fail, &code) == 6) {
        ++rows;
        const BatchPlan p = batch_plan(batch_chunks((size_t)n, (size_t)first, (size_t)last), sort != 0, true, true, true);
        BatchWalk w;
        for (size_t i = 0; i < p.steps.size(); ++i) {
            if (!w.runs(p.steps[i])) continue;
            printf("%zu ", i);
            w.done(p.steps[i], (int)i == fail ? code : 0);
        }
        printf("rc %d\n", w.rc);
    }
    while (!walk && fscanf(f, "%llu %llu %llu %d %d %d %d", &n, &first, &last, &sort, &theta, &err, &fresh) == 7) {
        ++rows;
        printf("case %llu %llu %llu %d %d %d %d\n", n, first, last, sort, theta, err, fresh);
        const std::vector<int> chunks = batch_chunks((size_t)n, (size_t)first, (size_t)last);
        print_plan(batch_plan(chunks, sort != 0, theta != 0, err != 0, fresh != 0));
    }
    const bool eof = feof(f) != 0;
    fclose(f);
    if (!eof || !rows) {
        fprintf(stderr, "unreadable row after %d rows\n", rows);
        return 2;
    }
    return 0;
}
