// The domain predicate the host's argument checks and the device's k_dev_check share (ppls_amd/csrc/aq_domain.h,
// with the two shipped plug-ins' domain_ok), g++ alone: the host side of "one predicate, two callers". Built
// and run by tests/test_domain_predicate.py.
//   domain_check FILE    one "integrand a b [theta...]" per line (C99 hex floats, nan, inf) -> one 0 / 1 per line
#include <cstdio>
#include <cstdlib>
#include <cstring>

// what the plug-in headers need from aq_libm.h to be read by a host compiler: their F is device code, never
// called here
#define __device__
#define __forceinline__ inline
namespace aq {
struct ExpEntry;
double exp_glibc_any(double x, const ExpEntry* tab);
}  // namespace aq
#include "aq_domain_hd.h"
#include "plugins/aq_user_gauss.h"
#include "plugins/aq_param_gauss.h"
#include "aq_domain.h"

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        fprintf(stderr, "usage: domain_check FILE\n");
        return 2;
    }
    char line[512];
    while (fgets(line, sizeof line, f)) {
        char* p = line;
        const int fid = (int)strtol(p, &p, 10);
        const double a = strtod(p, &p), b = strtod(p, &p);
        double th[aq::param::nparams];
        for (double& t : th) t = strtod(p, &p);
        printf("%d\n", fid == AQ_F_PARAM ? (int)aq::params_ok(a, b, th) : (int)aq::bounds_ok(fid, a, b));
    }
    fclose(f);
    return 0;
}
