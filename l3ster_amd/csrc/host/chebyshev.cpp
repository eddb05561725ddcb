// chebyshev.cpp -- the option and eigenvalue-estimate checks of the Chebyshev-Jacobi preconditioner (host/chebyshev.hpp).
// A host-only translation unit built WITHOUT -ffinite-math-only (l3ster_amd/build.py), so that a test for NaN or infinity
// means what it says; the bits are read from memory through volatile, which no optimisation level may fold either.
#include "host/chebyshev.hpp"

#include <cstdint>

namespace l3k::host
{
bool chebFinite(const double* p)
{
    static_assert(sizeof(std::uint64_t) == sizeof(double));
    const volatile unsigned char* b = reinterpret_cast< const volatile unsigned char* >(p);
    std::uint64_t                 u = 0;
    for (unsigned k = 0; k < sizeof u; ++k) // (little-endian, as every target of this library)
        u |= std::uint64_t(b[k]) << (8 * k);
    return ((u >> 52) & 0x7ff) != 0x7ff;
}
const char* chebCheckOpts(int degree, const double* cond_est, int max_power_iters, const double* boost_factor,
                          const double* lambda_max)
{
    if (degree < 1)
        return "degree < 1";
    if (!chebFinite(cond_est) || !(*cond_est > 1.))
        return "cond_est <= 1 (lambda_min = lambda_max / cond_est must lie below lambda_max)";
    if (!chebFinite(boost_factor) || !(*boost_factor >= 1.))
        return "boost_factor < 1";
    if (!chebFinite(lambda_max))
        return "lambda_max is not finite";
    if (!(*lambda_max > 0.) && max_power_iters < 1)
        return "max_power_iters < 1 and no lambda_max given";
    return nullptr;
}
} // namespace l3k::host
