// solver.hpp -- what api_solver.hip (the PCG loops, the Chebyshev-Jacobi preconditioner) and api_pmg.hip (the p-multigrid cycle on
// top of them) share: the operator value, the Chebyshev object, the preconditioner value of the PCG that keeps r.
#ifndef L3K_SOLVER_HPP
#define L3K_SOLVER_HPP

#include "objects.hpp"

#include "host/chebyshev.hpp"

namespace l3k::solver
{
// The operator of a solve: n rows (of a partitioned system: this rank's owned rows), y <- A x, and y <- A x with s[1] <- this rank's
// <x, A x>, on the context's stream.  The PCG loops, the power method and the Chebyshev recurrence are written ONCE over this
// value; mfOp, mfsOp and csrOp make it for one rank, mfDistOp and csrDistOp for a partitioned system.  reduce_fn and its object `halo` are the reduction hook:
// the loops call reduce(s, first, count) wherever a dot product has landed in s[first .. first + count); the partitioned makers
// set l3k_halo_allreduce_sum over the halo's ranks, the single-rank makers leave it null and nothing is enqueued.  The collective
// GMRES (api_gmres.hip) puts the wide reduction there: its passes land in the halo's block (l3k::halo::reduceRow) and the hook sums
// the rows into d_vals (l3k::halo::allreduceRow)
struct LinOp
{
    l3k_ctx* ctx;
    int64_t  n;
    void*    object; // the l3k_mf, l3k_mfs, l3k_csr or l3k_csr_dist behind it
    int (*apply_fn)(const LinOp&, const double*, double*);
    int (*energy_fn)(const LinOp&, const double*, double*, double*);
    int (*reduce_fn)(void* halo, double* d_vals, int count) = nullptr;
    l3k_halo* halo                                           = nullptr;
    // partitioned matrix-free operator: where <x, A x> comes from -- 0 not agreed yet, 1 the element kernels on every rank, 2
    // l3k_cg_dot_pap on every rank (element-wise and row-wise shares do not add up across ranks)
    mutable int energy_route = 0;
    int apply(const double* d_x, double* d_y) const { return apply_fn(*this, d_x, d_y); }
    int applyEnergy(const double* d_x, double* d_y, double* d_s) const { return energy_fn(*this, d_x, d_y, d_s); }
    int reduce(double* d_s, int first, int count) const { return reduce_fn ? reduce_fn(halo, d_s + first, count) : 0; }
};
LinOp mfOp(l3k_mf* mf);
// the sum of several matrix-free terms (api_mfs.hip): l3k_mfs_apply, and <x, A x> from the fixed-order dot product behind it
LinOp mfsOp(l3k_mfs* S);
// the partitioned operators: (l3k_mf, l3k_halo) through l3k_mf_apply_dist, l3k_csr_dist through l3k_csr_dist_apply / _apply_energy
LinOp mfDistOp(l3k_mf* mf, l3k_halo* halo);
LinOp csrDistOp(l3k_csr_dist* D);
// -1 with a message from `who` unless the halo is on the system's context and matches its mesh (dofs per node, ghost range)
int haloFitsSystem(const char* who, const l3k_mf* mf, const l3k_halo* h);
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
// what api_gmres.hip takes from the PCG's files: the CSR operator value, the Chebyshev object and the p-multigrid cycle as Precond
// values (apply with d_s == nullptr: no <r, z>), and the test that an l3k_mfs can be solved on one rank (`message` takes `who`)
LinOp   csrOp(l3k_csr* A);
Precond chebPrecond(l3k_cheb* c);
Precond pmgPrecond(l3k_pmg* M);
int     mfsSolvable(const l3k_mfs* S, const char* message, const char* who);
// the triangular preconditioner (api_tri.hip) as a Precond value: the mask is the object's own, 1 on the rows that store an entry;
// triReady: -1 with a message from `who` unless the object's last l3k_tri_factor succeeded
Precond triPrecond(l3k_tri* T);
int     triReady(const l3k_tri* T, const char* who);
// s[slot] <- <u, v> in the fixed order of the PCG's reductions
int dotInto(l3k_ctx* ctx, const double* d_u, const double* d_v, int64_t n, double* d_s, int slot);
} // namespace l3k::solver

// the object behind l3k_cheb (include/l3k.h): the operator it was created on, coefficients, the caller's minv, and two vectors of its own -- x and y of the power
// method during creation, w and A z of l3k_cheb_apply afterwards
struct l3k_cheb
{
    l3k::solver::LinOp    op; // the operator it was created on (mfOp, csrOp, mfDistOp or csrDistOp: its applies are collective then)
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
