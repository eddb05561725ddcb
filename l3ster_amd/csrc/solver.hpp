// solver.hpp -- what api_solver.hip (the PCG loops, the Chebyshev-Jacobi preconditioner) and api_pmg.hip (the p-multigrid cycle on
// top of them) share: the operator value, the Chebyshev object, the preconditioner value of the PCG that keeps r.
#ifndef L3K_SOLVER_HPP
#define L3K_SOLVER_HPP

#include "objects.hpp"

#include "host/chebyshev.hpp"

namespace l3k::solver
{
// The operator of a single-rank solve: n rows, y <- A x, and y <- A x with s[1] <- <x, A x>, on the context's stream.  The PCG
// loops, the power method and the Chebyshev recurrence are written ONCE over this value; mfOp and csrOp make it
struct LinOp
{
    l3k_ctx* ctx;
    int64_t  n;
    void*    object; // the l3k_mf or l3k_csr behind it
    int (*apply_fn)(void*, const double*, double*, size_t);
    int (*energy_fn)(void*, const double*, double*, double*);
    int apply(const double* d_x, double* d_y) const { return apply_fn(object, d_x, d_y, size_t(n)); }
    int applyEnergy(const double* d_x, double* d_y, double* d_s) const { return energy_fn(object, d_x, d_y, d_s); }
};
LinOp mfOp(l3k_mf* mf);
// The preconditioner of the PCG that keeps r (pcgSolvePrecond): z <- M^-1 r with s[2] <- <r, z> behind it on the stream, the
// frozen-row mask (rows with mask == 0 keep x and carry r = 0) and the sizes.  w and az are two vectors of the loop's workspace
// that are free during the application
struct Precond
{
    void*         object;
    const void*   system; // the l3k_mf or l3k_csr it was created on
    const double* mask;
    int64_t       n, ld; // rows; distance between the vectors of the workspace (a multiple of 4)
    int (*apply_fn)(void* object, const double* r, double* z, double* w, double* az, double* d_s);
    int apply(const double* r, double* z, double* w, double* az, double* d_s) const { return apply_fn(object, r, z, w, az, d_s); }
};
// the iteration of l3k_pcg_solve_cheb / l3k_csr_pcg_solve_cheb / l3k_pcg_solve_pmg (include/l3k.h; `who` in the messages)
int pcgSolvePrecond(const LinOp& A, const char* who, const double* d_b, double* d_x, const Precond& M, const l3k_cg_opts* opts,
                    l3k_cg_result* result);
// s[slot] <- <u, v> in the fixed order of the PCG's reductions
int dotInto(l3k_ctx* ctx, const double* d_u, const double* d_v, int64_t n, double* d_s, int slot);
} // namespace l3k::solver

// the object behind l3k_cheb (include/l3k.h): the operator it was created on, coefficients, the caller's minv, and two vectors of its own -- x and y of the power
// method during creation, w and A z of l3k_cheb_apply afterwards
struct l3k_cheb
{
    l3k::solver::LinOp    op; // the operator it was created on (mfOp or csrOp)
    const double*         minv;
    l3k_cheb_info         info;
    l3k::host::ChebCoeffs coef;
    DevBuf< double >      work; // w | az | s[8]
    int64_t               n, ld; // owned dofs; distance between the vectors (a multiple of 4: the applies want aligned columns)
};
namespace l3k::solver
{
// z <- p(D^-1 A) D^-1 r with the caller's w and az (n doubles each); d_s != nullptr: s[2] = <r, z> from the last kernel
int chebApply(l3k_cheb* c, const double* r, double* z, double* w, double* az, double* d_s);
} // namespace l3k::solver
#endif
