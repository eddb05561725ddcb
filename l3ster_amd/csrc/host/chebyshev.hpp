// chebyshev.hpp -- the scalar side of the Chebyshev-Jacobi preconditioner (include/l3k.h: l3k_cheb_create): option checks
// (defined in host/chebyshev.cpp) and the coefficients of the recurrence.  Host-only, no HIP: a stand-alone program can use both.
#ifndef L3K_HOST_CHEBYSHEV_HPP
#define L3K_HOST_CHEBYSHEV_HPP

#include <vector>

namespace l3k::host
{
// The library's device translation units are built with -ffinite-math-only: there the compiler may assume that no double it sees
// is NaN or infinite, and folds std::isfinite(v), v != v and even a test of the bits of a value it can follow to a constant.
// The two checks are therefore defined in host/chebyshev.cpp, a host-only translation unit built without the finite-math flags,
// and are not inline: the caller's optimiser cannot look through the call.  They take the doubles by pointer and read the bits
// from memory.
bool chebFinite(const double* p);
// Ifpack2ChebyshevPreconditioner::Options (solve/Ifpack2Preconditioners.hpp:107-118); nullptr = fine, else what is wrong
const char* chebCheckOpts(int degree, const double* cond_est, int max_power_iters, const double* boost_factor,
                          const double* lambda_max);
// z <- p(D^-1 A) D^-1 r:  w = z = c0 D^-1 r;  step k = 1 .. degree - 1:  w = a[k-1] w + b[k-1] D^-1 (r - A z), z += w
struct ChebCoeffs
{
    double                c0 = 0.;
    std::vector< double > a, b;
};
inline ChebCoeffs chebCoeffs(double lambda_max, double lambda_min, int degree)
{
    const double theta = (lambda_max + lambda_min) / 2., delta = (lambda_max - lambda_min) / 2., sigma = theta / delta;
    ChebCoeffs   c;
    c.c0       = 1. / theta;
    double rho = 1. / sigma;
    for (int k = 1; k < degree; ++k)
    {
        const double rho_new = 1. / (2. * sigma - rho);
        c.a.push_back(rho_new * rho);
        c.b.push_back(2. * rho_new / delta);
        rho = rho_new;
    }
    return c;
}
} // namespace l3k::host
#endif
