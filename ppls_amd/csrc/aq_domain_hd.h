// aq_domain_hd.h -- the qualifier of the domain predicates (aq_domain.h bounds_ok / params_ok and the
// plug-ins' domain_ok): host and device under hipcc, where the device-resident batch checks its rows in a
// kernel, nothing under a host compiler.
#pragma once
#if defined(__HIPCC__)
#define AQ_DOMAIN_HD __host__ __device__
#else
#define AQ_DOMAIN_HD
#endif
