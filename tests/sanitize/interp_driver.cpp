// interp_driver.cpp -- sanitizer driver for the 1-D transfer table of the p-multigrid levels (l3k::host::interp1d, the table behind
// l3k_interp_1d): every order pair 1 .. 8 in both directions, with the properties the transfer kernels rely on.  Built with
// -fsanitize=address,undefined by tests/test_pmg_cpu.py; stands beside san_driver.cpp, which covers the other host tables.
#include "host/tables.hpp"

#include <cmath>
#include <cstdio>

int main()
{
    int bad = 0;
    for (int pf = 1; pf <= 8; ++pf)
        for (int pt = 1; pt <= 8; ++pt)
        {
            const auto T  = l3k::host::interp1d(pf, pt);
            const int  nf = pf + 1, nt = pt + 1;
            if (T.size() != size_t(nf) * nt)
                ++bad;
            for (int i = 0; i < nt; ++i)
            {
                double sum = 0.;
                for (int j = 0; j < nf; ++j)
                    sum += T[size_t(i) * nf + j];
                if (std::fabs(sum - 1.) > 1e-14) // (a partition of unity)
                    ++bad;
            }
            for (int j = 0; j < nf; ++j) // the end rows are exact unit vectors
                if (T[j] != (j == 0 ? 1. : 0.) || T[size_t(nt - 1) * nf + j] != (j == nf - 1 ? 1. : 0.))
                    ++bad;
            if (pf == pt)
                for (int i = 0; i < nt; ++i)
                    for (int j = 0; j < nf; ++j)
                        if (T[size_t(i) * nf + j] != (i == j ? 1. : 0.))
                            ++bad;
        }
    if (bad)
    {
        std::printf("interp driver: %d violations\n", bad);
        return 1;
    }
    std::printf("interp driver: ok\n");
    return 0;
}
