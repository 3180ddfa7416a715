// Replay recorded launch plans through aq::plan_launch (ppls_amd/csrc/aq_launch_plan.h), g++ alone.
// Input (a file, argv[1]), one row per line:
//   fid grid k shard_array nshards first_slot diag batch_heap gsplit_env eps | hint: valid preset per_ok fid nshards eps |
//   plan: rc variant nwt shares D tail_from tail_mult per_cu static_jobs adaptive | hint after: valid preset per_ok fid nshards eps
// (eps values as hex floats). Every field must match; a refused row (rc != 0) records rc and the hint only.
// Prints one line per mismatch and "ok <rows>" when there is none. `--constants` prints the constants the
// plans depend on, as JSON. Built and run by tests/test_launch_plan.py. `--plan REQUESTS` prints plans (print_plans).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "aq_launch_plan.h"

using namespace aq;

static bool same_hint(const HintState& h, int valid, int preset, int per_ok, int fid, int nshards, double eps) {
    return h.valid == (valid != 0) && h.preset == (preset != 0) && h.per_ok == (per_ok != 0) && h.fid == fid &&
           h.nshards == nshards && h.eps == eps;
}

// `--plan REQUESTS`: print plan_launch's plan for every request row instead of comparing (tests/test_shape_matrix.py).
// Input, one row per line:
//   fid grid k shard_array nshards first_slot diag batch_heap gsplit_env eps err | hint: valid preset per_ok fid nshards eps
// A hint whose `valid` is -1 is the previous row's hint after its launch, with this row's `preset` (a batch front
// end's chunk sets it for its own launch only): a sequence of launches on one context. Output, one line per row:
//   rc variant nwt shares D tail_from tail_mult per_cu static_jobs adaptive err deeper | hint after (as above)
// `deeper`: D is one level past seed_depth_job (the skewed integrand's unsharded per-CU launches), 0 or 1.
static int print_plans(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        return 2;
    }
    int rows = 0;
    int fid, grid, k, sa, nshards, first_slot, diag, bh, gse, err, hv, hp, hpo, hf, hn;
    char se[64], she[64];
    HintState prev;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %63s %d %d %d %d %d %d %63s", &fid, &grid, &k, &sa, &nshards, &first_slot,
                  &diag, &bh, &gse, se, &err, &hv, &hp, &hpo, &hf, &hn, she) == 17) {
        ++rows;
        LaunchRequest r;
        r.fid = fid;
        r.grid = grid;
        r.k = k;
        r.shard_array = sa != 0;
        r.nshards = nshards;
        r.first_slot = first_slot;
        r.diag = diag != 0;
        r.batch_heap = bh != 0;
        r.gsplit_env = gse;
        r.eps = strtod(se, nullptr);
        r.err = err != 0;
        HintState h = prev;
        if (hv >= 0) {
            h.valid = hv != 0;
            h.per_ok = hpo != 0;
            h.fid = hf;
            h.nshards = hn;
            h.eps = strtod(she, nullptr);
        }
        h.preset = hp != 0;
        const LaunchPlan p = plan_launch(r, h);
        const int deeper = p.rc == AQ_OK && p.D > seed_depth_job((unsigned long long)p.shares * (unsigned long long)nshards);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %a\n", p.rc, (int)p.variant, p.nwt, p.shares, p.D,
               p.tail_from, p.tail_mult, p.per_cu, p.static_jobs, p.adaptive, (int)p.err, deeper, (int)p.hint.valid,
               (int)p.hint.preset, (int)p.hint.per_ok, p.hint.fid, p.hint.nshards, p.hint.eps);
        prev = p.hint;
        prev.preset = false;   // (the caller's, for the one launch)
    }
    const bool eof = feof(f) != 0;
    fclose(f);
    if (!eof) {
        fprintf(stderr, "unreadable row after %d rows\n", rows);
        return 2;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--constants")) {
        printf("{\"NW\": %d, \"WCAP\": %d, \"S_W\": %d, \"S_W1\": %d, \"LONE_NW\": %d, \"PCU_MAXK\": %d, \"STATIC_MAXK\": %d, "
               "\"MAXK\": %d, \"NPARTS\": %d, \"SYNC_SLOT\": %d, \"DEFAULT_GSPLIT\": %d, \"LONE_GSPLIT\": %d, "
               "\"TAIL_DIV\": %d, \"TAIL_MULT\": %d}\n", NW, WCAP, S_W, AQ_S_W1, AQ_LONE_NW, PCU_MAXK, STATIC_MAXK, MAXK, NPARTS,
               SYNC_SLOT, DEFAULT_GSPLIT, AQ_LONE_GSPLIT, AQ_TAIL_DIV, AQ_TAIL_MULT);
        return 0;
    }
    if (argc > 2 && !strcmp(argv[1], "--plan")) return print_plans(argv[2]);
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: launch_plan_check ROWS | --constants | --plan REQUESTS\n");
        return 2;
    }
    int rows = 0, bad = 0;
    int fid, grid, k, sa, nshards, first_slot, diag, bh, gse, hv, hp, hpo, hf, hn;
    int rc, variant, nwt, shares, D, tail_from, tail_mult, per_cu, static_jobs, adaptive, av, ap, apo, af, an;
    char se[64], she[64], ae[64];
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %63s %d %d %d %d %d %63s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %63s",
                  &fid, &grid, &k, &sa, &nshards, &first_slot, &diag, &bh, &gse, se, &hv, &hp, &hpo, &hf, &hn, she, &rc,
                  &variant, &nwt, &shares, &D, &tail_from, &tail_mult, &per_cu, &static_jobs, &adaptive, &av, &ap, &apo,
                  &af, &an, ae) == 32) {
        ++rows;
        LaunchRequest r;
        r.fid = fid;
        r.grid = grid;
        r.k = k;
        r.shard_array = sa != 0;
        r.nshards = nshards;
        r.first_slot = first_slot;
        r.diag = diag != 0;
        r.batch_heap = bh != 0;
        r.gsplit_env = gse;
        r.eps = strtod(se, nullptr);
        HintState h;
        h.valid = hv != 0;
        h.preset = hp != 0;
        h.per_ok = hpo != 0;
        h.fid = hf;
        h.nshards = hn;
        h.eps = strtod(she, nullptr);
        const LaunchPlan p = plan_launch(r, h);
        bool ok = p.rc == rc && same_hint(p.hint, av, ap, apo, af, an, strtod(ae, nullptr));
        if (ok && rc == AQ_OK)
            ok = (int)p.variant == variant && p.nwt == nwt && p.shares == shares && p.D == D && p.tail_from == tail_from &&
                 p.tail_mult == tail_mult && p.per_cu == per_cu && p.static_jobs == static_jobs && p.adaptive == adaptive;
        if (!ok) {
            ++bad;
            printf("row %d: got rc %d variant %d nwt %d shares %d D %d tail %d x%d per_cu %d static %d adaptive %d "
                   "hint %d %d %d %d %d %a\n", rows, p.rc, (int)p.variant, p.nwt, p.shares, p.D, p.tail_from, p.tail_mult,
                   p.per_cu, p.static_jobs, p.adaptive, (int)p.hint.valid, (int)p.hint.preset, (int)p.hint.per_ok,
                   p.hint.fid, p.hint.nshards, p.hint.eps);
        }
    }
    const bool eof = feof(f) != 0;
    fclose(f);
    if (!eof) {
        fprintf(stderr, "unreadable row after %d rows\n", rows);
        return 2;
    }
    if (bad) return 1;
    printf("ok %d\n", rows);
    return 0;
}
