// chi2.h -- ln of the chi-square survival function, pure host FP64
// (ulg_chi2_log_sf; host/chi2_check.cpp compiles it stand-alone).
//
// ln Q(a, z) with a = dof / 2, z = x / 2, the regularised upper incomplete
// gamma function.  Everything is kept in log space, so the result stays
// finite where Q itself would underflow (x up to 1e7, dof up to 32768):
//   z < a + 1   the series of the lower tail P = 1 - Q,
//               ln P = a ln z - z - lgamma(a + 1) + ln sum_k z^k / ((a+1)...(a+k)),
//               then ln Q = log1p(-P)  (here Q is never small);
//   z >= a + 1  the continued fraction of the upper tail by modified Lentz,
//               ln Q = a ln z - z - lgamma(a) + ln h,
//               h = 1 / (z+1-a - 1(1-a) / (z+3-a - 2(2-a) / (z+5-a - ...))).
// dof = 2 is the closed form Q = exp(-z).
#pragma once

#include <cmath>

namespace ulg {

inline double chi2_log_sf(double x, double dof) {
    if (std::isnan(x) || std::isnan(dof)) return NAN;
    if (!(x > 0.0)) return 0.0;
    if (!(dof > 0.0)) return -INFINITY;  // a point mass at 0
    const double a = dof / 2.0, z = x / 2.0;
    if (a == 1.0) return -z;
    const double eps = 1e-17;
    if (z < a + 1.0) {
        double term = 1.0, sum = 1.0, ap = a;
        for (int k = 0; k < 1000000; ++k) {
            ap += 1.0;
            term *= z / ap;
            sum += term;
            if (term < sum * eps) break;
        }
        const double lnP = a * std::log(z) - z - std::lgamma(a + 1.0) + std::log(sum);
        return std::log1p(-std::exp(lnP));
    }
    const double tiny = 1e-300;
    double b = z + 1.0 - a;
    double c = 1.0 / tiny;
    double d = 1.0 / b;
    double h = d;
    for (int i = 1; i < 1000000; ++i) {
        const double an = -(double)i * ((double)i - a);
        b += 2.0;
        d = an * d + b;
        if (std::fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 3e-16) break;
    }
    return a * std::log(z) - z - std::lgamma(a) + std::log(h);
}

}  // namespace ulg
