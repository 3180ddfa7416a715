// aq_integrate_batch_tol's HIP-free rules (ppls_amd/csrc/aq_host_args.h), g++ alone. Built and run by
// tests/test_tol.py, which holds the expected answers.
//   ok FILE         one "epsabs epsrel eps0 shrink max_rounds max_depth" per line (doubles as hex floats, "nan" or
//                   "inf") -> tol_args_ok as 0 / 1 per line
//   schedule FILE   one "eps0 shrink max_rounds" per line -> the defaulted shrink and max_rounds, then the EPSILON of
//                   every round 1 .. max_rounds as hex floats, on one line each
//   block FILE      one AQ_TOL_BLOCK value per line -> the rows per block
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "aq_host_args.h"

using namespace aq;

int main(int argc, char** argv) {
    FILE* f = argc == 3 ? fopen(argv[2], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: tol_args_check ok FILE | schedule FILE | block FILE\n");
        return 2;
    }
    int rows = 0;
    if (!strcmp(argv[1], "ok")) {
        char ea[64], er[64], e0[64], sh[64];
        int max_rounds, max_depth;
        while (fscanf(f, "%63s %63s %63s %63s %d %d", ea, er, e0, sh, &max_rounds, &max_depth) == 6) {
            ++rows;
            const aq_tol t{strtod(ea, nullptr), strtod(er, nullptr), strtod(e0, nullptr), strtod(sh, nullptr), max_rounds,
                           max_depth};
            printf("%d\n", tol_args_ok(t) ? 1 : 0);
        }
    } else if (!strcmp(argv[1], "schedule")) {
        char e0[64], sh[64];
        int max_rounds;
        while (fscanf(f, "%63s %63s %d", e0, sh, &max_rounds) == 3) {
            ++rows;
            const aq_tol t = tol_defaulted(aq_tol{0.0, 1.0, strtod(e0, nullptr), strtod(sh, nullptr), max_rounds, 0});
            printf("%a %d", t.shrink, t.max_rounds);
            for (int r = 1; r <= t.max_rounds; ++r) printf(" %a", tol_round_eps(t, r));
            printf("\n");
        }
    } else if (!strcmp(argv[1], "block")) {
        long long v;
        while (fscanf(f, "%lld", &v) == 1) {
            ++rows;
            printf("%d\n", tol_block_rows(v));
        }
    }
    const bool eof = feof(f) != 0;
    fclose(f);
    if (!eof || !rows) {
        fprintf(stderr, "unreadable row after %d rows\n", rows);
        return 2;
    }
    return 0;
}
