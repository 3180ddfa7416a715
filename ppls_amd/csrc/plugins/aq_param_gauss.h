// aq_param_gauss.h -- the default AQ_F_PARAM plug-in (and the template for writing one).
//
// AQ_F_PARAM is the reference's integrand macro (aquadPartA.c:46) with constants that differ from
// integral to integral: a family F(x; theta), one row theta[nparams] per integral. This plug-in is the
// Gaussian with location and inverse scale, theta = {mu, s}:
//     #define F(arg) exp(-(((arg) - mu) * s) * (((arg) - mu) * s))
// evaluated as t = (x - mu) * s (two roundings), (-t) * t rounded once, then glibc 2.35 exp
// (aq::exp_glibc_any, bit-exact). At theta = {0, 1}, (x - 0) * 1 is exact, so the function is bit for
// bit the AQ_F_USER Gaussian (aq_user_gauss.h), whose trees the reference binary pins
// (tests/golden/trees.json).
//
// To plug in another family, copy this file, change name / nparams / F / domain_ok, and rebuild:
//     PPLS_AMD_PARAM_F=/path/to/my_family.h python ppls_amd/build.py --force
// F runs on the GPU inside the persistent kernel, where `th` is wave-uniform (scalar registers): use it
// as an operand, do not index it with a per-lane value. It may call aq::exp_glibc_any, aq::cosh_glibc
// (both take the LDS exp table `tab`) and the device libm (faithful, not glibc-exact).
#pragma once

namespace aq {
namespace param {

constexpr const char* name = "gauss: exp(-((arg - mu) * s)^2), theta = {mu, s}";
constexpr int nparams = 2;

__device__ __forceinline__ double F(double x, const double (&th)[nparams], const ExpEntry* __restrict__ tab) {
    const double t = (x - th[0]) * th[1];
    return exp_glibc_any(-t * t, tab);   // (-t)*t rounded once, then glibc-exact exp, as aq_user_gauss.h
}

// Finite bounds and parameters within +-1e150 (t * t may overflow to inf: exp(-inf) = 0, never a NaN),
// and a non-zero inverse scale. F is in [0, 1], so no area can overflow. AQ_DOMAIN_HD (aq_domain_hd.h): the
// host's argument checks and the device-resident batch's check kernel both call it, so it is plain arithmetic
// on its arguments -- no host-only library call, no global.
AQ_DOMAIN_HD inline bool domain_ok(double a, double b, const double* th) {
    return a >= -1e150 && b <= 1e150 && th[0] >= -1e150 && th[0] <= 1e150 && th[1] >= -1e150 && th[1] <= 1e150 &&
           th[1] != 0.0;
}

}  // namespace param
}  // namespace aq
