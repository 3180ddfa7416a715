// The C ABI's HIP-free argument rules (ppls_amd/csrc/aq_host_args.h), g++ alone. Built and run by
// tests/test_host_args.py, which holds the expected answers.
//   --constants     MAXK, NSLOTS, AQ_MAX_LEVELS and the error codes of the bits 0..7, as JSON
//   chunks FILE     one "n first last" per line -> one line of batch_chunks' sizes each ("-" for none)
//   ranges FILE     one "k eps max_depth shard nshards shard_array first_slot slot_limit" per line (eps as a hex
//                   float, "nan" or "-0.0") -> launch_ranges_ok as 0 / 1 per line
//   slots FILE      one "first n" per line -> slot_range_ok as 0 / 1 per line
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "aq_host_args.h"

using namespace aq;

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("{\"MAXK\": %d, \"NSLOTS\": %d, \"AQ_MAX_LEVELS\": %d, \"err_from_bits\": [", MAXK, NSLOTS, AQ_MAX_LEVELS);
        for (unsigned b = 0; b < 8; ++b) printf("%s%d", b ? ", " : "", err_from_bits(b));
        printf("]}\n");
        return 0;
    }
    FILE* f = argc == 3 ? fopen(argv[2], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: host_args_check --constants | chunks FILE | ranges FILE | slots FILE\n");
        return 2;
    }
    int rows = 0;
    if (!strcmp(argv[1], "chunks")) {
        unsigned long long n, first, last;
        while (fscanf(f, "%llu %llu %llu", &n, &first, &last) == 3) {
            ++rows;
            const std::vector<int> c = batch_chunks((size_t)n, (size_t)first, (size_t)last);
            if (c.empty()) printf("-");
            for (size_t i = 0; i < c.size(); ++i) printf("%s%d", i ? " " : "", c[i]);
            printf("\n");
        }
    } else if (!strcmp(argv[1], "ranges")) {
        int k, max_depth, shard, nshards, shard_array, first_slot, slot_limit;
        char eps[64];
        while (fscanf(f, "%d %63s %d %d %d %d %d %d", &k, eps, &max_depth, &shard, &nshards, &shard_array, &first_slot,
                      &slot_limit) == 8) {
            ++rows;
            printf("%d\n", launch_ranges_ok(k, strtod(eps, nullptr), max_depth, shard, nshards, shard_array != 0, first_slot,
                                            slot_limit) ? 1 : 0);
        }
    } else if (!strcmp(argv[1], "slots")) {
        int first, n;
        while (fscanf(f, "%d %d", &first, &n) == 2) {
            ++rows;
            printf("%d\n", slot_range_ok(first, n) ? 1 : 0);
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
