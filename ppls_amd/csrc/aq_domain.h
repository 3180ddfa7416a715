// aq_domain.h -- the supported domain of one integral, as ONE predicate for the host's argument checks
// (aq_abi.inc: every launch entry point, the batch front end's staging) and the device's (k_dev_check,
// aquad.hip: the device-resident batch checks its rows where they are). include/aquad.h's AQ_EINVAL text
// states the rule; tests/test_domain_predicate.py compares this header with it value by value.
//
// Host and device C++: hipcc compiles the functions for both sides, g++ (the CPU tests) for the host. The
// plug-ins' domain_ok carry the same qualifier, AQ_DOMAIN_HD (aq_domain_hd.h). Needs aq::user::domain_ok,
// aq::param::domain_ok and aq::param::nparams declared before it (aq_libm.h includes the plug-ins).
#pragma once
#include <cmath>

#include "aquad.h"
#include "aq_domain_hd.h"

namespace aq {

// (no std::isfinite / std::max: one spelling that is the same code on both sides)
AQ_DOMAIN_HD inline bool dom_finite(double x) { return fabs(x) <= 0x1.fffffffffffffp1023; }   // false for a NaN

// The kernels compare DOUBLED areas (aq_device.h task_step_k), which are the reference's own products
// (F(l)+F(r))*(r-l) before its '/2'; the sums l2 + r2 must stay finite where the reference's halves do, so
// every |F| * width stays far below 2^1023: bounds within 2^900, and for cosh^4 (F ~ e^{4|x|}/16, 16 F in
// the rounds) |x| <= 170. The persistent kernel's rings hold HALVED endpoints (pair_step_halves), exact
// while every coordinate of the tree is 0 or at least 2^-1021 in magnitude: nonzero bounds of at least
// 2^-900 keep the smallest coordinate a 64-level tree can make (one cancelling midpoint, 2^-53 below the
// bounds' scale, then 64 halvings) far above that.
AQ_DOMAIN_HD inline bool bounds_ok(int f, double a, double b) {
    if (!(dom_finite(a) && dom_finite(b) && b >= a)) return false;
    const double fa = fabs(a), fb = fabs(b), m = fa > fb ? fa : fb;
    if (m > 0x1p900) return false;
    if ((a != 0.0 && fa < 0x1p-900) || (b != 0.0 && fb < 0x1p-900)) return false;
    if (f == AQ_F_COSH4) return m <= 170.0;
    if (f == AQ_F_USER) return user::domain_ok(a, b);
    return true;
}

// One integral of the parametrised family: the engine's bounds rule, finite parameters, the plug-in's domain.
AQ_DOMAIN_HD inline bool params_ok(double a, double b, const double* th) {
    if (!bounds_ok(AQ_F_PARAM, a, b)) return false;
    for (int j = 0; j < param::nparams; ++j)
        if (!dom_finite(th[j])) return false;
    return param::domain_ok(a, b, th);
}

}  // namespace aq
