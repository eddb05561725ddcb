// periodic.hpp -- the host-only side of the periodic boundary conditions (include/l3k.h: l3k_periodic_match, l3k_periodic_merge).
// The finiteness checks of l3k_periodic_match live in host/periodic.cpp for the reason given in host/chebyshev.hpp: the device
// translation units are built with -ffinite-math-only, which folds std::isfinite.  Not inline, operands read from memory.
#ifndef L3K_HOST_PERIODIC_HPP
#define L3K_HOST_PERIODIC_HPP

#include <cstddef>

namespace l3k::host
{
bool allFinite(const double* v, size_t n);
// nullptr = fine, else what is wrong with the translation (its first dim entries) or the tolerance
const char* periodicCheckReals(int dim, const double* translation, const double* tolerance);
} // namespace l3k::host
#endif
