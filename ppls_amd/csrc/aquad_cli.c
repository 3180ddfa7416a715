/*
 * aquad_cli.c -- drop-in for `mpirun -n P ./aquadPartA` (/root/reference/aquadPartA.c main(), :78-123).
 *
 *   aquad [-n P] [--gpus G] [--eps E] [--a A] [--b B] [--f cosh4|sin_recip|user|param] [--theta v0,v1,...]
 *         [--per-cu] [--levels] [--err] [--epsrel R] [--epsabs A] [--eps0 E0] [--shrink S]
 *
 * Same observable surface as the reference: `Area=%lf`, a blank line, `Tasks Per Process`, the index
 * row and the count row (tab-terminated entries). Process 0 is the farmer and always reports 0 tasks
 * (:162 only counts dispatches to workers). Processes 1..P-1 are the on-device workers: every CU of
 * every GPU used, dealt round-robin (GPU-major, CU slot order) over the P-1 columns; P defaults to
 * 1 + G, i.e. one column per GPU. `--per-cu` prints one column per CU. P < 2 reproduces the
 * reference's error exactly (:86-90). Defaults are the reference's macros (:45-48).
 * With G > 1 the run is sharded over an RCCL group (aq_group_create: one host thread drives every
 * GPU; aq_integrate_group combines the shards with one grouped all-reduce / all-gather).
 * `--f param --theta v0,v1,...` integrates the parametrised family F(x; theta) (aq_integrate_params; as many
 * values as aq_param_count(); one GPU). The printout is the same.
 * `--err` (one GPU, no --levels) runs the error-estimate form (aq_integrate_err): the printout is unchanged,
 * and two lines follow it, `Error estimate=%.6e` (the sum of |d| over the accepted intervals, d the
 * difference the test at :191 bounds) and `Extrapolated area=%.17g` (aq_err_extrapolate).
 * `--epsrel R` and / or `--epsabs A` (one GPU, no --levels, one worker column, no --per-cu) refine the integral
 * until its error estimate is at most max(A, R * |area|) (aq_integrate_batch_tol on the one integral: rounds at
 * EPSILON E0, E0 / S, ...; --eps0 defaults to --eps, --shrink to 8): the printout of the round it retired in,
 * the two --err lines, and `Rounds=<r> eps=<EPSILON of that round, %.17g>` (r negative: not converged, exit 3).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aquad.h"

static void usage(void) {
    fprintf(stderr,
            "usage: aquad [-n P] [--gpus G] [--eps E] [--a A] [--b B] [--f cosh4|sin_recip|user|param] "
            "[--theta v0,v1,...] [--per-cu] [--levels] [--err] [--epsrel R] [--epsabs A] [--eps0 E0] [--shrink S]\n");
}

int main(int argc, char **argv) {
    aq_problem p = {AQ_F_COSH4, 0, 0.0, 5.0, 1e-3, 0, 0}; /* aquadPartA.c:45-48 */
    int nprocs = -1, gpus = 1, per_cu = 0, levels = 0, with_err = 0;
    aq_err err = {0.0, 0.0};
    double theta[AQ_MAX_PARAMS] = {0};
    int ntheta = 0;
    aq_tol tol = {0.0, 0.0, 0.0, 0.0, 0, 0};
    int with_tol = 0, rounds = 0;
    double eps_used = 0.0;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        const char *v = (i + 1 < argc) ? argv[i + 1] : NULL;
        if ((!strcmp(a, "-n") || !strcmp(a, "-c") || !strcmp(a, "-np")) && v) { nprocs = atoi(v); ++i; }
        else if (!strcmp(a, "--gpus") && v) { gpus = atoi(v); ++i; }
        else if (!strcmp(a, "--eps") && v) { p.eps = atof(v); ++i; }
        else if (!strcmp(a, "--a") && v) { p.a = atof(v); ++i; }
        else if (!strcmp(a, "--b") && v) { p.b = atof(v); ++i; }
        else if (!strcmp(a, "--f") && v) {
            if (!strcmp(v, "cosh4")) p.integrand = AQ_F_COSH4;
            else if (!strcmp(v, "sin_recip")) p.integrand = AQ_F_SIN_RECIP;
            else if (!strcmp(v, "user")) p.integrand = AQ_F_USER;
            else if (!strcmp(v, "param")) p.integrand = AQ_F_PARAM;
            else { usage(); return 2; }
            ++i;
        } else if (!strcmp(a, "--theta") && v) {
            const char *s = v;
            for (ntheta = 0; *s;) {
                char *end;
                const double x = strtod(s, &end);
                if (end == s || ntheta == AQ_MAX_PARAMS) { usage(); return 2; }
                theta[ntheta++] = x;
                s = *end == ',' ? end + 1 : end;
                if (*end && *end != ',') { usage(); return 2; }
            }
            ++i;
        } else if (!strcmp(a, "--per-cu")) per_cu = 1;
        else if (!strcmp(a, "--levels")) levels = 1;
        else if (!strcmp(a, "--err")) with_err = 1;
        else if (!strcmp(a, "--epsrel") && v) { tol.epsrel = atof(v); with_tol = 1; ++i; }
        else if (!strcmp(a, "--epsabs") && v) { tol.epsabs = atof(v); with_tol = 1; ++i; }
        else if (!strcmp(a, "--eps0") && v) { tol.eps0 = atof(v); ++i; }
        else if (!strcmp(a, "--shrink") && v) { tol.shrink = atof(v); ++i; }
        else { usage(); return 2; }
    }
    if (p.integrand == AQ_F_PARAM ? (ntheta != aq_param_count() || gpus != 1) : ntheta != 0) {
        fprintf(stderr, "aquad: --f param takes --theta with %d value(s) (%s) on one GPU; no other integrand takes it\n",
                aq_param_count(), aq_param_integrand_name());
        return 2;
    }
    if (with_err && (gpus != 1 || levels)) {
        fprintf(stderr, "aquad: --err runs on one GPU and keeps no level histograms\n");
        return 2;
    }
    if (with_tol && (gpus != 1 || levels || per_cu || (nprocs != -1 && nprocs != 2))) {
        fprintf(stderr, "aquad: --epsrel / --epsabs run on one GPU with one worker column and keep no level histograms\n");
        return 2;
    }
    if (nprocs == -1) nprocs = 1 + gpus;
    if (nprocs < 2) { /* aquadPartA.c:86-90 */
        fprintf(stderr, "ERROR: Must have at least 2 processes to run\n");
        exit(1);
    }
    int ndev = 0;
    if (aq_device_count(&ndev) != AQ_OK || gpus < 1 || gpus > ndev) {
        fprintf(stderr, "aquad: need %d GPU(s), found %d\n", gpus, ndev);
        return 1;
    }
    aq_ctx **ctx = calloc((size_t)gpus, sizeof(*ctx));
    aq_group *grp = NULL;
    int rc = AQ_OK;
    for (int g = 0; g < gpus && rc == AQ_OK; ++g) rc = aq_ctx_create(g, &ctx[g]);
    const int ncu = rc == AQ_OK ? aq_ctx_num_cus(ctx[0]) : 0;
    uint64_t *per_gpu = calloc((size_t)gpus, sizeof(uint64_t));
    uint64_t *cu = calloc((size_t)gpus * (size_t)(ncu > 0 ? ncu : 1), sizeof(uint64_t));
    aq_result res;
    memset(&res, 0, sizeof(res));
    res.tasks_per_gpu = per_gpu;
    res.tasks_per_cu = cu;
    if (rc == AQ_OK) {
        if (with_tol) {
            if (tol.eps0 == 0.0) tol.eps0 = p.eps;
            tol.max_depth = p.max_depth;
            uint64_t accepted = 0;
            rc = aq_integrate_batch_tol(ctx[0], 1, &p.a, &p.b, p.integrand == AQ_F_PARAM ? theta : NULL, p.integrand, &tol,
                                        &res.area, &accepted, &res.tasks, &err.err_abs, &err.err_signed, &eps_used,
                                        &rounds);
            res.accepted = accepted;
            res.n_gpus = 1;
            per_gpu[0] = res.tasks;
            if (rc == AQ_ENOCONV) rc = AQ_OK;   /* reported by the sign of Rounds= and the exit code */
        } else if (with_err) {
            rc = aq_integrate_err(ctx[0], &p, p.integrand == AQ_F_PARAM ? theta : NULL, &res, &err);
        } else if (gpus == 1) {
            rc = p.integrand == AQ_F_PARAM ? aq_integrate_params(ctx[0], &p, theta, &res) : aq_integrate(ctx[0], &p, &res);
        } else {
            p.n_gpus = gpus;
            rc = aq_group_create(ctx, gpus, &grp);
            if (rc == AQ_OK) rc = aq_integrate_group(grp, &p, &res);
        }
    }
    if (rc != AQ_OK) {
        fprintf(stderr, "aquad: %s\n", aq_strerror(rc));
        return 1;
    }
    if (!per_cu && nprocs - 1 == gpus) {
        aq_print_reference(stdout, &res);
    } else {
        int cols = per_cu ? 0 : nprocs - 1;
        if (per_cu)
            for (int k = 0; k < gpus * ncu; ++k) cols += cu[k] ? 1 : 0;
        uint64_t *tpp = calloc((size_t)cols + 1, sizeof(uint64_t));
        int k = 0;
        for (int c = 0; c < gpus * ncu; ++c)
            if (cu[c]) { tpp[1 + (k % cols)] += cu[c]; ++k; }
        aq_print_reference_procs(stdout, res.area, tpp, cols + 1);
        free(tpp);
    }
    if (with_err || with_tol) {
        fprintf(stdout, "Error estimate=%.6e\n", err.err_abs);
        fprintf(stdout, "Extrapolated area=%.17g\n", aq_err_extrapolate(res.area, &err));
    }
    if (with_tol) fprintf(stdout, "Rounds=%d eps=%.17g\n", rounds, eps_used);
    if (levels) {
        uint64_t t[AQ_MAX_LEVELS], l[AQ_MAX_LEVELS];
        aq_level_histogram(ctx[0], t, l, AQ_MAX_LEVELS);
        fprintf(stdout, "\nLevel\tTasks\tAccepted\n");
        for (uint32_t d = 0; d < res.levels; ++d)
            fprintf(stdout, "%u\t%llu\t%llu\n", d, (unsigned long long)t[d], (unsigned long long)l[d]);
        fprintf(stdout, "Total\t%llu\t%llu\n", (unsigned long long)res.tasks, (unsigned long long)res.accepted);
    }
    aq_group_destroy(grp);
    for (int g = 0; g < gpus; ++g) aq_ctx_destroy(ctx[g]);
    free(cu);
    free(per_gpu);
    free(ctx);
    if (with_tol && rounds < 0) return 3;
    return 0;
}
