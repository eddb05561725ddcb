// chol_symbolic.hpp -- the symbolic phase of the band Cholesky solver (include/l3k.h: l3k_chol_create, l3k_chol_order), host only:
// the active rows of a CSR graph, the check of its structural symmetry, the reverse Cuthill-McKee ordering and the monotone block
// envelope the factor lives in.  tests/chol_ref.py restates every rule here in numpy; the two must give identical results.
#ifndef L3K_HOST_CHOL_SYMBOLIC_HPP
#define L3K_HOST_CHOL_SYMBOLIC_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

namespace l3k::host
{
struct CholSymbolic
{
    int64_t n = 0, n_active = 0; // rows of the operator; rows that store at least one entry
    int     nb = 0;              // block edge: 32 or 64
    int64_t n_blocks = 0;        // block columns: ceil(n_active / nb)
    int64_t max_height = 0;      // largest H(K)
    int64_t total_blocks = 0;    // sum over K of 1 + H(K)
    size_t  factor_bytes = 0;    // total_blocks * nb * nb * 8
    double  factor_flops = 0.;   // of one numeric factorisation, update_flops included
    double  update_flops = 0.;   // ... of its trailing updates alone (the matrix-core launches)
    std::vector< int32_t > perm;    // [n_active]: perm[new] = old
    std::vector< int32_t > inv;     // [n]: inv[old] = new, -1 on a row outside the factorisation
    std::vector< int32_t > heights; // [n_blocks]: H(K)
    std::vector< int64_t > col_off; // [n_blocks + 1]: first block of block column K in the storage
};
// block: 0 (choose: 64 once the ordered matrix has an entry 64 or more off the diagonal, else 32), 32 or 64.  0, or -1 with the
// error set (prefixed with `who`): an invalid graph, a structurally unsymmetric one, an unknown block size
int cholSymbolic(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, int block, CholSymbolic& out, const char* who);
// the memory guard: -1 with the bytes needed and the largest H in the message if the factor exceeds max_bytes (0: no limit)
int cholCheckBytes(const CholSymbolic& s, size_t max_bytes, const char* who);
} // namespace l3k::host
#endif
