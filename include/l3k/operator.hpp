// operator.hpp -- C++ host-side mirror of the reference's interface for the hot path, on top of the C ABI (l3k.h).
//
// The reference is C++ (header-only); this header gives its maintainers the same vocabulary over libl3k.so:
//   l3k::CubeMesh                ~ generateAndDistributeMesh<order>(makeCubeMesh(...))   comm/DistributeMesh.hpp:284-299
//   l3k::MatrixFreeSystem        ~ algsys::MatrixFreeSystem                               algsys/MatrixFreeSystem.hpp:19-249
//       .apply(X, Y, alpha, beta)   ~ Operator::apply                                      :34-41
//       .diagAndRhs(...)            ~ endAssembly() -> computeDiagAndRhs                   :877-941
//       .assembleLocal(...)         ~ assembleLocalSystem                                  algsys/AssembleLocalSystem.hpp:234-256
//       .assembleProblem(bnd)       ~ assembleProblem(boundary kernel, boundary_ids)      algsys/MatrixFreeSystem.hpp:58-68
//       .assembleBoundary(on)       ~ the boundary overload of assembleGlobalSystem          algsys/AssembleGlobalSystem.hpp:55-96
//       .apply(halo, X, Y, ...)     ~ applyImpl of a partitioned system, exchange included    :1020-1140
//       .scatterLocalSystems(...)   ~ scatterLocalSystem / assembleGlobalSystem             algsys/ScatterLocalSystem.hpp:24-54
//   l3k::Halo                    ~ comm::ImportExportContext + comm::Import / comm::Export  comm/ImportExport.hpp:29-72,130-215
//   l3k::Transfer                ~ (no counterpart: the p-multigrid transfer of a partitioned mesh, next to l3k_pmg_*)
//   l3k::SquareMesh              ~ makeSquareMesh(...) at an order, one rank              mesh/primitives/SquareMesh.hpp
//   l3k::MultiTermSystem         ~ algsys::MatrixFreeSystem as the sum of its assembleProblem calls     algsys/MatrixFreeSystem.hpp:24-89
//   l3k::ElementSubset           ~ the elements of some domains as a mesh over the same nodes (a term of a MultiTermSystem)
//   l3k::AssembledSystem         ~ algsys::AssembledSystem: beginAssembly / assembleProblem / endAssembly, hexes and quads
//   l3k::CsrOperator             ~ the assembled / condensed tpetra_crsmatrix_t in front of Belos  solve/BelosSolvers.hpp:116-122
//   l3k::Gmres                   ~ Gmres, the restarted GMRES in front of the same operators      solve/BelosSolvers.hpp:124-130
//   l3k::DistributedCsr          ~ ... of an MPI run: the ranks' local matrices applied as one (sub-assembled form)
//       AssembledSystem(mesh, halo, ...) ~ algsys::AssembledSystem on one rank of a partitioned mesh
//   l3k::BoundaryTerm            ~ a BoundaryEquationKernel on a set of boundary views   algsys/EvaluateLocalOperator.hpp:238-330
//   l3k::computeIntegral / computeNormL2 ~ post/Integral.hpp:113-128, post/NormL2.hpp:31-62 (one rank)
//   l3k::ExportDefinition / PvtuExporter ~ post/VtkExport.hpp:16-97: .vtu / .pvtu files from the field storage on the device
// Errors: the reference throws std::runtime_error from util::throwingAssert (util/Assertion.hpp:88-95); so does this
// wrapper, with the text of l3k_last_error().  RAII handles, no torch, no other dependency than l3k.h + the HIP runtime
// of the caller for device memory.
#ifndef L3K_OPERATOR_HPP
#define L3K_OPERATOR_HPP

#include "l3k.h"

#include <array>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <span>
#include <stdexcept>
#include <string>
#include <vector>

namespace l3k
{
inline void check(int rc)
{
    if (rc != 0)
        throw std::runtime_error{std::string{"libl3k: "} + l3k_last_error()};
}

// AssemblyOptions, algsys/AssembleLocalSystem.hpp:24-49
struct AssemblyOptions
{
    int value_order = 1, derivative_order = 0, eval_strategy = 0;
};

class Context
{
public:
    explicit Context(int hip_device = 0, void* hip_stream = nullptr) { check(l3k_ctx_create(hip_device, hip_stream, &m_ctx)); }
    Context(const Context&)            = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { l3k_ctx_destroy(m_ctx); }
    void     setStream(void* hip_stream) { check(l3k_ctx_set_stream(m_ctx, hip_stream)); }
    // bitwise-reproducible element launches for the meshes created from now on (the reference's relaxed atomics,
    // algsys/MatrixFreeSystem.hpp:513, are not reproducible run to run)
    void     setDeterministic(bool on = true) { check(l3k_ctx_set_deterministic(m_ctx, on ? 1 : 0)); }
    // the point a domain kernel sees under sum factorisation: the true z (default) or the reference's z = 0
    // (algsys/SumFactorization.hpp:732)
    void setReferenceZ0(bool on = true) { check(l3k_ctx_set_reference_z0(m_ctx, on ? 1 : 0)); }
    // launch-route settings (the defaults are the measured choices; tests and tools take the other routes on purpose)
    l3k_tuning tuning() const
    {
        l3k_tuning t{};
        check(l3k_ctx_get_tuning(m_ctx, &t));
        return t;
    }
    void setTuning(const l3k_tuning& t) { check(l3k_ctx_set_tuning(m_ctx, &t)); }
    void     synchronize() { check(l3k_ctx_synchronize(m_ctx)); }
    l3k_ctx* get() const { return m_ctx; }

private:
    l3k_ctx* m_ctx{};
};

// One rank's block of the synthetic structured hex mesh (host arrays, reference numbering conventions)
class CubeMesh
{
public:
    CubeMesh(std::array< int, 3 > ne, int order, std::array< int, 3 > parts = {1, 1, 1}, int rank = 0, double perturb = 0.)
    {
        check(l3k_cube_partition_create(ne.data(), order, parts.data(), rank, perturb, &m_mesh));
        check(l3k_hostmesh_view_get(m_mesh, &m_view));
    }
    CubeMesh(const CubeMesh&)            = delete;
    CubeMesh& operator=(const CubeMesh&) = delete;
    ~CubeMesh() { l3k_hostmesh_destroy(m_mesh); }
    const l3k_hostmesh_view& view() const { return m_view; }
    int64_t                  nLocalNodes() const { return m_view.n_owned_nodes + m_view.n_ghost_nodes; }
    // the boundary views of makeCubeMesh (mesh/primitives/CubeMesh.hpp:66-138): (element, side) pairs of this rank's
    // element sides on the cube sides selected by bit s of `sides`
    struct Sides
    {
        std::vector< int64_t > elems;
        std::vector< uint8_t > sides;
    };
    Sides boundarySides(unsigned sides = 0x3f) const
    {
        Sides out;
        for (int s = 0; s < 6; ++s)
            if (sides & (1u << s))
                for (int64_t e = 0; e < m_view.n_elems; ++e)
                    if (m_view.elem_boundary[e] & (1u << s))
                    {
                        out.elems.push_back(e);
                        out.sides.push_back(static_cast< uint8_t >(s));
                    }
        return out;
    }
    // BCDefinition::defineDirichlet(boundary_ids, {unknowns}) as a byte mask over local dofs; sides as in
    // mesh/ElementTraits.hpp:84-95 (bit s of `sides`)
    std::vector< uint8_t > dirichletMask(int dofs_per_node, std::span< const int > unknowns, unsigned sides = 0x3f) const
    {
        std::vector< uint8_t > mask(static_cast< size_t >(nLocalNodes()) * dofs_per_node, 0);
        for (int64_t n = 0; n < nLocalNodes(); ++n)
            if (m_view.node_boundary[n] & sides)
                for (int u : unknowns)
                    mask[n * dofs_per_node + u] = 1;
        return mask;
    }

private:
    l3k_hostmesh*     m_mesh{};
    l3k_hostmesh_view m_view{};
};

// The single-rank structured quad mesh of [0,1]^2 (l3k_square_mesh_create): the same view with dim = 2, elem_verts [n_elems][4][3]
// and the quad side order 0 y=0, 1 y=1, 2 x=0, 3 x=1 (mesh/ElementTraits.hpp:84-95)
class SquareMesh
{
public:
    using Sides = CubeMesh::Sides;
    SquareMesh(std::array< int, 2 > ne, int order, double perturb = 0.)
    {
        check(l3k_square_mesh_create(ne.data(), order, perturb, &m_mesh));
        check(l3k_hostmesh_view_get(m_mesh, &m_view));
    }
    SquareMesh(const SquareMesh&)            = delete;
    SquareMesh& operator=(const SquareMesh&) = delete;
    ~SquareMesh() { l3k_hostmesh_destroy(m_mesh); }
    const l3k_hostmesh_view& view() const { return m_view; }
    int64_t                  nLocalNodes() const { return m_view.n_owned_nodes + m_view.n_ghost_nodes; }
    Sides                    boundarySides(unsigned sides = 0xf) const
    {
        Sides out;
        for (int s = 0; s < 4; ++s)
            if (sides & (1u << s))
                for (int64_t e = 0; e < m_view.n_elems; ++e)
                    if (m_view.elem_boundary[e] & (1u << s))
                    {
                        out.elems.push_back(e);
                        out.sides.push_back(static_cast< uint8_t >(s));
                    }
        return out;
    }
    std::vector< uint8_t > dirichletMask(int dofs_per_node, std::span< const int > unknowns, unsigned sides = 0xf) const
    {
        std::vector< uint8_t > mask(static_cast< size_t >(nLocalNodes()) * dofs_per_node, 0);
        for (int64_t n = 0; n < nLocalNodes(); ++n)
            if (m_view.node_boundary[n] & sides)
                for (int u : unknowns)
                    mask[n * dofs_per_node + u] = 1;
        return mask;
    }

private:
    l3k_hostmesh*     m_mesh{};
    l3k_hostmesh_view m_view{};
};

class DeviceMesh
{
public:
    // Mesh: CubeMesh or SquareMesh (anything with the l3k_hostmesh_view of its arrays)
    template < typename Mesh >
    DeviceMesh(Context& ctx, const Mesh& mesh, int dofs_per_node, const uint8_t* dirichlet = nullptr) : m_dpn{dofs_per_node}
    {
        const auto&         v = mesh.view();
        const l3k_mesh_desc d{v.dim, v.order, v.n_elems, v.n_interior_elems, v.elem_nodes, v.elem_verts, v.n_owned_nodes,
                              v.n_ghost_nodes, dofs_per_node, dirichlet};
        check(l3k_mesh_create(ctx.get(), &d, &m_mesh));
        m_owned = v.n_owned_nodes * dofs_per_node;
        m_ctx   = ctx.get();
    }
    DeviceMesh(const DeviceMesh&)            = delete;
    DeviceMesh& operator=(const DeviceMesh&) = delete;
    ~DeviceMesh() { l3k_mesh_destroy(m_mesh); }
    l3k_mesh* get() const { return m_mesh; }
    l3k_ctx*  ctx() const { return m_ctx; }
    int64_t   nOwnedDofs() const { return m_owned; }

private:
    l3k_mesh* m_mesh{};
    l3k_ctx*  m_ctx{};
    int64_t   m_owned{};
    int       m_dpn{};
};

// The mailboxes of the in-process transport: the ranks are threads of this process, each with its own Context (one GPU or
// several); must outlive the halos built on its tables
class InprocGroup
{
public:
    explicit InprocGroup(int world) { check(l3k_inproc_group_create(world, &m_group)); }
    InprocGroup(const InprocGroup&)            = delete;
    InprocGroup& operator=(const InprocGroup&) = delete;
    ~InprocGroup() { l3k_inproc_group_destroy(m_group); }
    l3k_halo_transport transport(int rank) const
    {
        l3k_halo_transport t{};
        check(l3k_inproc_transport(m_group, rank, &t));
        return t;
    }

private:
    l3k_inproc_group* m_group{};
};

// One rank's ghost exchange (ImportExportContext + Import / Export, comm/ImportExport.hpp:29-72,130-215) carried by RCCL
// inside the library.  uniqueId(): 128 bytes drawn by one rank and handed to the others by the host's own means (the
// reference has MPI_Bcast); the constructor is collective over the `world` ranks.
class Halo
{
public:
    static std::array< char, 128 > uniqueId()
    {
        std::array< char, 128 > id{};
        check(l3k_halo_unique_id(id.data()));
        return id;
    }
    Halo(Context& ctx, const CubeMesh& mesh, int dofs_per_node, const std::array< char, 128 >& unique_id, int rank, int world)
    {
        const auto& v = mesh.view();
        check(l3k_halo_create(ctx.get(), unique_id.data(), rank, world, dofs_per_node, v.n_nbrs, v.nbr_rank, v.send_offsets,
                              v.send_nodes, v.ghost_offsets, &m_halo));
    }
    // With a transport table instead of RCCL: the host's own (e.g. MPI on device pointers), or the library's in-process
    // transport for the threads of one process (InprocGroup above).  Not collective.  Mesh: CubeMesh, or SquareMesh (one part)
    template < typename Mesh >
    Halo(Context& ctx, const Mesh& mesh, int dofs_per_node, const l3k_halo_transport& transport, int rank, int world)
    {
        const auto& v = mesh.view();
        check(l3k_halo_create_transport(ctx.get(), &transport, rank, world, dofs_per_node, v.n_nbrs, v.nbr_rank, v.send_offsets,
                                        v.send_nodes, v.ghost_offsets, &m_halo));
    }
    Halo(const Halo&)            = delete;
    Halo& operator=(const Halo&) = delete;
    ~Halo() { l3k_halo_destroy(m_halo); }
    int64_t nGhostDofs() const { return l3k_halo_n_ghost_dofs(m_halo); }
    // comm::Import: ghost rows <- owners' rows; comm::Export: owners' rows += ghost rows
    void importGhosts(const double* d_owned, size_t ld, int ncols, double* d_ghost, size_t ldg) const
    {
        check(l3k_halo_import(m_halo, d_owned, ld, ncols, d_ghost, ldg));
    }
    void exportAdd(const double* d_ghost, size_t ldg, int ncols, double* d_owned, size_t ld) const
    {
        check(l3k_halo_export_add(m_halo, d_ghost, ldg, ncols, d_owned, ld));
    }
    // sum of d_vals[0 .. count), count <= 8, over all ranks in ascending rank order, in place: the same bits on every rank
    void allreduceSum(double* d_vals, int count) const { check(l3k_halo_allreduce_sum(m_halo, d_vals, count)); }
    // the same sum for 1 <= count <= capacity values, behind reduceReserve(capacity) (local; the collective GMRES reserves its own)
    void reduceReserve(int capacity) const { check(l3k_halo_reduce_reserve(m_halo, capacity)); }
    void allreduceSumN(double* d_vals, int count) const { check(l3k_halo_allreduce_sum_n(m_halo, d_vals, count)); }
    l3k_halo* get() const { return m_halo; }

private:
    l3k_halo* m_halo{};
};

// The inter-order transfer of one level pair of a mesh that may be partitioned (l3k_transfer_*): the p-multigrid transfer for hosts
// that keep the hierarchy of a partitioned run themselves.  d_elem_map: device, nullptr = identity; it and the meshes must outlive
// the object.  A vector of a level is its owned rows plus its ghost rows (Halo::importGhosts before prolong on the coarse level,
// Halo::exportAdd of the ghost rows after restrict); the ghost pointers may be null on meshes without ghosts.
class Transfer
{
public:
    Transfer(Context& ctx, const DeviceMesh& fine, const DeviceMesh& coarse, const int64_t* d_elem_map = nullptr)
    {
        check(l3k_transfer_create(ctx.get(), fine.get(), coarse.get(), d_elem_map, &m_transfer));
    }
    Transfer(const Transfer&)            = delete;
    Transfer& operator=(const Transfer&) = delete;
    ~Transfer() { l3k_transfer_destroy(m_transfer); }
    l3k_transfer_info info() const
    {
        l3k_transfer_info i{};
        check(l3k_transfer_info_get(m_transfer, &i));
        return i;
    }
    // x_f <- P x_c (add: x_f += P x_c) on the owned fine rows; d_frozen: owned fine rows with 0 there are left alone
    void prolong(const double* d_xc, const double* d_xc_ghost, double* d_xf, bool add = false, const double* d_frozen = nullptr) const
    {
        check(l3k_transfer_prolong(m_transfer, d_xc, d_xc_ghost, d_xf, add ? 1 : 0, d_frozen));
    }
    // r_c, r_c_ghost <- this rank's share of P^T r_f
    void restrict(const double* d_rf, double* d_rc, double* d_rc_ghost) const
    {
        check(l3k_transfer_restrict(m_transfer, d_rf, d_rc, d_rc_ghost));
    }
    l3k_transfer* get() const { return m_transfer; }

private:
    l3k_transfer* m_transfer{};
};
// d = r - az on the rows with minv != 0, 0 on the others: the masked residual of the p-multigrid cycle (l3k_pmg_residual)
inline void pmgResidual(Context& ctx, double* d_d, const double* d_r, const double* d_az, const double* d_minv, int64_t n)
{
    check(l3k_pmg_residual(ctx.get(), d_d, d_r, d_az, d_minv, n));
}

// A boundary equation kernel on a list of element sides (the reference's assembleProblem(kernel, boundary_ids))
class BoundaryTerm
{
public:
    template < typename KernelParamBlock >
    BoundaryTerm(const DeviceMesh& mesh, int kernel_id, const KernelParamBlock& params, const CubeMesh::Sides& sides,
                 AssemblyOptions opts = {}, std::span< const int > field_inds = {}, int n_rhs = 1)
    {
        const l3k_asmopts o{opts.value_order, opts.derivative_order, opts.eval_strategy};
        check(l3k_bnd_create(mesh.ctx(), mesh.get(), kernel_id, &params, sizeof params, &o,
                             field_inds.empty() ? nullptr : field_inds.data(), n_rhs, int64_t(sides.elems.size()),
                             sides.elems.data(), sides.sides.data(), &m_bnd));
    }
    BoundaryTerm(const DeviceMesh& mesh, int kernel_id, const CubeMesh::Sides& sides, AssemblyOptions opts = {}, int n_rhs = 1)
    {
        const l3k_asmopts o{opts.value_order, opts.derivative_order, opts.eval_strategy};
        check(l3k_bnd_create(mesh.ctx(), mesh.get(), kernel_id, nullptr, 0, &o, nullptr, n_rhs,
                             int64_t(sides.elems.size()), sides.elems.data(), sides.sides.data(), &m_bnd));
    }
    BoundaryTerm(const BoundaryTerm&)            = delete;
    BoundaryTerm& operator=(const BoundaryTerm&) = delete;
    ~BoundaryTerm() { l3k_bnd_destroy(m_bnd); }
    void     setFields(const double* d_soa, size_t ld) { check(l3k_bnd_set_fields(m_bnd, d_soa, ld)); }
    void     setTime(double t) { check(l3k_bnd_set_time(m_bnd, t)); } // in.point.time of the boundary kernel
    // assembleLocalSystem on the sides [first, first+count) of the list (AssembleLocalSystem.hpp:77-216): K_s (row-major Nd x Nd),
    // F_s (column-major Nd x n_rhs) of the whole element from the side quadrature; either may be nullptr (hexes)
    void assembleLocal(int64_t first, int64_t count, double* d_K, double* d_F) const
    {
        check(l3k_bnd_local_assemble(m_bnd, first, count, d_K, d_F));
    }
    // the boundary overload of assembleGlobalSystem (AssembleGlobalSystem.hpp:55-96) for the sides [first, first+count): summed into
    // the caller's CSR values / rhs, additive; returns the number of entries outside the graph
    int64_t assembleGlobal(int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind, double* d_values, double* d_rhs,
                           size_t ldr, bool skip_dirichlet = false, size_t workspace_bytes = 0) const
    {
        int64_t missing = 0;
        check(l3k_bnd_assemble_global(m_bnd, first, count, d_row_ptr, d_col_ind, d_values, d_rhs, ldr, skip_dirichlet ? 1 : 0, workspace_bytes,
                                      &missing));
        return missing;
    }
    l3k_bnd* get() const { return m_bnd; }

private:
    l3k_bnd* m_bnd{};
};

// computeIntegral (post/Integral.hpp:113-128) for one rank: integral of a residual kernel over the mesh (sides == nullptr)
// or over element sides; fields = SoA device array [n_fields][ld]
template < typename KernelParamBlock >
std::vector< double > computeIntegral(const DeviceMesh& mesh, int residual_id, const KernelParamBlock* params,
                                      const double* d_fields, size_t ldf, AssemblyOptions opts = {},
                                      const CubeMesh::Sides* sides = nullptr, bool square = false, double time = 0.)
{
    l3k_kparams kp{};
    check(l3k_residual_info(residual_id, &kp, nullptr, nullptr));
    std::vector< double > out(static_cast< size_t >(kp.n_equations));
    const l3k_asmopts     o{opts.value_order, opts.derivative_order, opts.eval_strategy};
    check(l3k_integrate(mesh.ctx(), mesh.get(), residual_id, params, params ? sizeof(KernelParamBlock) : 0, &o, d_fields,
                        ldf, time, square ? 1 : 0, sides ? int64_t(sides->elems.size()) : -1,
                        sides ? sides->elems.data() : nullptr, sides ? sides->sides.data() : nullptr, out.data()));
    return out;
}
// computeNormL2 (post/NormL2.hpp:31-62): squared residual, doubled quadrature orders, square root
template < typename KernelParamBlock >
std::vector< double > computeNormL2(const DeviceMesh& mesh, int residual_id, const KernelParamBlock* params,
                                    const double* d_fields, size_t ldf, AssemblyOptions opts = {},
                                    const CubeMesh::Sides* sides = nullptr, double time = 0.)
{
    opts.value_order *= 2;
    opts.derivative_order *= 2;
    auto out = computeIntegral(mesh, residual_id, params, d_fields, ldf, opts, sides, true, time);
    for (auto& v : out)
        v = std::sqrt(v);
    return out;
}

// algsys::MatrixFreeSystem for one rank without ghosts.  Kernel = registered functor id + POD parameter block
// (l3ster_amd/csrc/user_kernels.hpp); vectors are DEVICE pointers, column-major with leading dimension.
// MatrixFreeSystem::updateSolution(sol_inds, sol_man, sol_man_inds) (algsys/MatrixFreeSystem.hpp:1231-1273): the solution's per-node
// dofs sol_inds of every column into the fields sol_man_inds (index-major, one per (index, column)) of the SoA field storage that a
// kernel's FieldAccess reads; ghost rows from d_xghost (the imported values; nullptr on a rank without ghosts)
// computeValuesAtNodes (algsys/ComputeValuesAtNodes.hpp:217-594; the engine of setDirichletBCValues / setValues) on one rank: the
// residual kernel evaluated at the nodes of the listed element sides (sides == nullptr: of every element), equation e written to
// per-node dof dof_inds[e] of d_values (all local dofs), element contributions averaged; entries no listed node touches keep
// their values.  d_work: 2 * n_local_dofs doubles of device scratch, ZEROED by the caller (sums and counts accumulate).  (A
// partitioned host exports the ghost rows of sum and count between l3k_values_at_nodes and l3k_average_values itself.)
template < typename KernelParamBlock >
void computeValuesAtNodes(const DeviceMesh& mesh, int residual_id, const KernelParamBlock* params, std::span< const int > dof_inds,
                          const CubeMesh::Sides* sides, const double* d_fields, size_t ldf, double time, int64_t n_local_dofs,
                          double* d_values, double* d_work)
{
    check(l3k_values_at_nodes(mesh.ctx(), mesh.get(), residual_id, params, params ? sizeof(KernelParamBlock) : 0, d_fields, ldf, time,
                              sides ? int64_t(sides->elems.size()) : -1, sides ? sides->elems.data() : nullptr,
                              sides ? sides->sides.data() : nullptr, dof_inds.data(), d_work, d_work + n_local_dofs));
    check(l3k_average_values(mesh.ctx(), d_work, d_work + n_local_dofs, n_local_dofs, d_values));
}

// NativeJacobiImpl::init (solve/NativePreconditioners.hpp:75-96): minv = sign(d) * damping / max(|d|, threshold)
inline void jacobiInverse(const DeviceMesh& mesh, const double* d_diag, int64_t n, double* d_minv, double damping = 1., double threshold = 0.)
{
    check(l3k_jacobi_inverse(mesh.ctx(), d_diag, n, damping, threshold, d_minv));
}

inline void updateSolution(const DeviceMesh& mesh, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, int ncols,
                           std::span< const int > sol_inds, std::span< const int > sol_man_inds, double* d_fields, size_t ldf, int n_fields)
{
    if (sol_man_inds.size() != sol_inds.size() * size_t(ncols))
        throw std::runtime_error{"Source and destination indices lengths must match"};
    check(l3k_update_solution(mesh.ctx(), mesh.get(), d_x, ldx, d_xghost, ldxg, ncols, int(sol_inds.size()), sol_inds.data(),
                              sol_man_inds.data(), d_fields, ldf, n_fields));
}

// The Chebyshev-Jacobi preconditioner of a partitioned operator (Ifpack2ChebyshevPreconditioner in an MPI run,
// solve/Ifpack2Preconditioners.hpp:26-36,107-131): made by MatrixFreeSystem::chebyshev(halo, ...) or DistributedCsr::chebyshev(...)
// (collective), handed to their pcgSolve.  The operator, the halo and d_minv must outlive it.  RAII, move-only.
class Chebyshev
{
public:
    explicit Chebyshev(l3k_cheb* handle) : m_cheb{handle} {}
    Chebyshev(const Chebyshev&)            = delete;
    Chebyshev& operator=(const Chebyshev&) = delete;
    Chebyshev(Chebyshev&& o) noexcept : m_cheb{o.m_cheb} { o.m_cheb = nullptr; }
    ~Chebyshev() { l3k_cheb_destroy(m_cheb); }
    l3k_cheb_info info() const
    {
        l3k_cheb_info i{};
        check(l3k_cheb_info_get(m_cheb, &i));
        return i;
    }
    // z <- p(D^-1 A) D^-1 r over the owned rows; collective on a partitioned operator
    void      apply(const double* d_r, double* d_z) const { check(l3k_cheb_apply(m_cheb, d_r, d_z)); }
    l3k_cheb* get() const { return m_cheb; }

private:
    l3k_cheb* m_cheb{};
};

class Gmres;
class MatrixFreeSystem
{
public:
    template < typename KernelParamBlock >
    MatrixFreeSystem(const DeviceMesh& mesh, int kernel_id, const KernelParamBlock& params, AssemblyOptions opts = {},
                     std::span< const int > field_inds = {}, int n_rhs = 1)
    {
        const l3k_asmopts o{opts.value_order, opts.derivative_order, opts.eval_strategy};
        check(l3k_mf_create(mesh.ctx(), mesh.get(), kernel_id, &params, sizeof params, &o,
                            field_inds.empty() ? nullptr : field_inds.data(), n_rhs, &m_mf));
    }
    MatrixFreeSystem(const DeviceMesh& mesh, int kernel_id, AssemblyOptions opts = {}, int n_rhs = 1)
    {
        const l3k_asmopts o{opts.value_order, opts.derivative_order, opts.eval_strategy};
        check(l3k_mf_create(mesh.ctx(), mesh.get(), kernel_id, nullptr, 0, &o, nullptr, n_rhs, &m_mf));
    }
    MatrixFreeSystem(const MatrixFreeSystem&)            = delete;
    MatrixFreeSystem& operator=(const MatrixFreeSystem&) = delete;
    ~MatrixFreeSystem() { l3k_mf_destroy(m_mf); }

    void setFields(const double* d_soa, size_t ld) { check(l3k_mf_set_fields(m_mf, d_soa, ld)); } // post::FieldAccess
    void setTime(double t) { check(l3k_mf_set_time(m_mf, t)); }
    // assembleProblem(boundary kernel, boundary ids): the term takes part in apply / diagAndRhs from now on and must
    // outlive this system
    void assembleProblem(const BoundaryTerm& term) { check(l3k_mf_attach_boundary(m_mf, term.get())); }
    // ... and, once switched on, in assembleLocal, assembleGlobal and the condensation calls: K_e + sum K_s, F_e + sum F_s over the
    // attached sides of each element, as the reference's assembled path forms them (AssembleGlobalSystem.hpp:55-96)
    void assembleBoundary(bool on = true) { check(l3k_mf_assemble_boundary(m_mf, on ? 1 : 0)); }
    // Y <- alpha*A*X + beta*Y (Operator::apply; the operator is symmetric, `mode` is ignored by the reference too)
    void apply(const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols = 1, double alpha = 1., double beta = 0.) const
    {
        check(l3k_mf_apply(m_mf, d_x, ldx, d_y, ldy, ncols, alpha, beta));
    }
    // the same on the owned rows of a partitioned system: import || interior elements, border elements, export || interior
    // elements, unpack-add, Dirichlet rows (MatrixFreeSystem::applyImpl :1020-1140), the exchange through `halo`
    void apply(const Halo& halo, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols = 1, double alpha = 1.,
               double beta = 0.) const
    {
        check(l3k_mf_apply_dist(m_mf, halo.get(), d_x, ldx, d_y, ldy, ncols, alpha, beta));
    }
    // scatterLocalSystem for the batch [first, first + count) of assembleLocal's output into the CSR values of the caller's
    // graph and the global right-hand sides (algsys/ScatterLocalSystem.hpp:24-54); returns the number of entries outside
    // the graph (skipped, as sumIntoLocalValues does)
    int64_t scatterLocalSystems(int64_t first, int64_t count, const double* d_K, const double* d_F, const int64_t* d_row_ptr,
                                const int32_t* d_col_ind, double* d_values, double* d_rhs, size_t ldr, bool skip_dirichlet = false) const
    {
        int64_t missing = 0;
        check(l3k_assembled_scatter(m_mf, first, count, d_K, d_F, d_row_ptr, d_col_ind, d_values, d_rhs, ldr, skip_dirichlet ? 1 : 0,
                                    &missing));
        return missing;
    }
    // assembleGlobalSystem (algsys/AssembleGlobalSystem.hpp:20-53) in one call: element systems formed and summed into the CSR
    // values / right-hand sides inside the library, sub-batch by sub-batch on two streams; returns the entries outside the graph
    int64_t assembleGlobal(int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind, double* d_values,
                           double* d_rhs, size_t ldr, bool skip_dirichlet = false, size_t workspace_bytes = 0) const
    {
        int64_t missing = 0;
        check(l3k_assemble_global(m_mf, first, count, d_row_ptr, d_col_ind, d_values, d_rhs, ldr, skip_dirichlet ? 1 : 0, workspace_bytes,
                                  &missing));
        return missing;
    }
    // diag(A) and rhs with Dirichlet lifting; the caller zeroes d_diag / d_rhs first (computeDiagAndRhs :921-923)
    void diagAndRhs(const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr) const
    {
        check(l3k_mf_diag_rhs(m_mf, 2, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, nullptr, nullptr, 0, 1));
    }
    // K_e (row-major Nd x Nd), F_e (column-major Nd x n_rhs) of elements [first, first+count)
    void assembleLocal(int64_t first, int64_t count, double* d_K, double* d_F, double* d_checksum = nullptr) const
    {
        check(l3k_local_assemble(m_mf, first, count, d_K, d_F, d_checksum));
    }
    // alg_sys.solve(CG{opts, NativeJacobiOpts{}}) for one rank (solve/BelosSolvers.hpp:116-122 + NativePreconditioners.hpp):
    // d_x holds the initial guess and the result; d_minv from l3k_jacobi_inverse (or nullptr); throws if not converged
    // like the reference (solve/BelosSolvers.hpp:103)
    l3k_cg_result solve(const double* d_b, double* d_x, const double* d_minv, l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        l3k_cg_result res{};
        check(l3k_pcg_solve(m_mf, d_b, d_x, d_minv, &opts, &res));
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    // the n_rhs columns of a multivector one after the other (the reference hands them to Belos "Block CG")
    std::vector< l3k_cg_result > solve(const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                                       l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        std::vector< l3k_cg_result > res(static_cast< size_t >(ncols));
        check(l3k_pcg_solve_cols(m_mf, d_b, ldb, d_x, ldx, ncols, d_minv, &opts, res.data()));
        for (const auto& r : res)
            if (!r.converged)
                throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    // alg_sys.solve(CG{...}) on every rank of an MPI run (solve/BelosSolvers.hpp:116-122): the collective solve of the partitioned
    // system over the owned rows, the reductions through `halo`; cheb == nullptr: Jacobi with d_minv, else the preconditioner of
    // chebyshev(halo, ...) (d_minv may then be nullptr).  Every rank returns the same result; throws if not converged
    l3k_cg_result pcgSolve(const Halo& halo, const double* d_b, double* d_x, const double* d_minv, l3k_cg_opts opts = {1e-6, 10000, 0, 1},
                           const Chebyshev* cheb = nullptr) const
    {
        l3k_cg_result res{};
        check(l3k_pcg_solve_dist(m_mf, halo.get(), d_b, d_x, d_minv, cheb ? cheb->get() : nullptr, &opts, &res));
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    // alg_sys.solve(Gmres{...}) on every rank of an MPI run (solve/BelosSolvers.hpp:124-131): the collective GMRES over the owned rows
    // with the workspace Gmres::collective(ctx, n_owned, restart_length), the same restart_length on every rank (defined below
    // Gmres).  cheb == nullptr: Jacobi with d_minv, or no preconditioner when d_minv is nullptr too; else the preconditioner of
    // chebyshev(halo, ...).  Every rank returns the same result; throws if not converged
    l3k_gmres_result gmresSolve(const Gmres& workspace, const Halo& halo, const double* d_b, double* d_x, const double* d_minv,
                                l3k_gmres_opts opts = {1e-6, 10000, 0, 1, 39}, const Chebyshev* cheb = nullptr) const;
    // collective; lambda_max == 0: estimated by the power method on D^-1 A across the ranks
    Chebyshev chebyshev(const Halo& halo, const double* d_minv, l3k_cheb_opts opts = {1, 30., 10, 1.1, 0.}) const
    {
        l3k_cheb* c = nullptr;
        check(l3k_cheb_create_dist(m_mf, halo.get(), d_minv, &opts, &c));
        return Chebyshev{c};
    }
    // the kernel a launch of this system takes (which: 0 all / 1 interior / 2 border elements), as text
    std::string route(int which = 0, int ncols = 1, bool with_energy = false) const
    {
        char buf[512] = {};
        check(l3k_mf_route(m_mf, which, ncols, with_energy ? 1 : 0, buf, sizeof buf));
        return buf;
    }
    // Y <- A X and d_s[1] <- <X, A X> in one pass (what a CG iteration needs of the operator; d_s: 8 device doubles)
    void applyEnergy(const double* d_x, double* d_y, double* d_s) const { check(l3k_mf_apply_energy(m_mf, d_x, d_y, d_s)); }
    l3k_mf* get() const { return m_mf; }

private:
    l3k_mf* m_mf{};
};

// Some of the elements of a mesh (CubeMesh, SquareMesh, anything with a view()) as a mesh over the SAME nodes: what DeviceMesh
// takes for a term of a MultiTermSystem that lives on part of the mesh.  The order of `elems` is kept, except that the interior
// elements come first, stably; the node-level arrays are the parent's, which must outlive this object
class ElementSubset
{
public:
    template < typename Mesh >
    ElementSubset(const Mesh& mesh, std::span< const int64_t > elems) : m_view{mesh.view()}
    {
        const auto&   v  = mesh.view();
        const int64_t n1 = v.order + 1, N = v.dim == 2 ? n1 * n1 : n1 * n1 * n1, nvd = (int64_t(1) << v.dim) * 3;
        for (const int64_t e : elems)
            if (e < 0 || e >= v.n_elems)
                throw std::runtime_error{"ElementSubset: element " + std::to_string(e) + " outside the mesh"};
        int64_t n_interior = 0;
        for (int cls = 0; cls < 2; ++cls)
            for (const int64_t e : elems)
                if ((e < v.n_interior_elems) == (cls == 0))
                {
                    m_nodes.insert(m_nodes.end(), v.elem_nodes + e * N, v.elem_nodes + (e + 1) * N);
                    m_verts.insert(m_verts.end(), v.elem_verts + e * nvd, v.elem_verts + (e + 1) * nvd);
                    m_boundary.push_back(v.elem_boundary ? v.elem_boundary[e] : uint8_t{0});
                    n_interior += cls == 0;
                }
        m_view.n_elems          = int64_t(elems.size());
        m_view.n_interior_elems = n_interior;
        m_view.elem_nodes       = m_nodes.data();
        m_view.elem_verts       = m_verts.data();
        m_view.elem_boundary    = m_boundary.data();
    }
    ElementSubset(const ElementSubset&)            = delete;
    ElementSubset& operator=(const ElementSubset&) = delete;
    const l3k_hostmesh_view& view() const { return m_view; }

private:
    l3k_hostmesh_view       m_view;
    std::vector< uint32_t > m_nodes;
    std::vector< double >   m_verts;
    std::vector< uint8_t >  m_boundary;
};

// algsys::MatrixFreeSystem as the sum of its assembleProblem calls (l3k_mfs_*; algsys/MatrixFreeSystem.hpp:24-89, :789-802): domain
// and boundary terms over the rows of `rows`, each on `rows` or on a DeviceMesh of an ElementSubset with the same dofs_per_node and
// Dirichlet mask.  assembleProblem(term) ..., endAssembly(), then apply / diagAndRhs / jacobiInverse / solve as on a
// MatrixFreeSystem.  Rows no term covers get beta*y from apply and 0 from jacobiInverse, so a solve leaves x as it is there.  The
// terms and `rows` must outlive the object.  RAII, move-only
class MultiTermSystem
{
public:
    explicit MultiTermSystem(const DeviceMesh& rows, int n_rhs = 1) : m_n{rows.nOwnedDofs()} { check(l3k_mfs_create(rows.get(), n_rhs, &m_sys)); }
    MultiTermSystem(const MultiTermSystem&)            = delete;
    MultiTermSystem& operator=(const MultiTermSystem&) = delete;
    MultiTermSystem(MultiTermSystem&& o) noexcept : m_sys{o.m_sys}, m_n{o.m_n} { o.m_sys = nullptr; }
    ~MultiTermSystem() { l3k_mfs_destroy(m_sys); }
    void assembleProblem(const MatrixFreeSystem& term) { check(l3k_mfs_add_domain(m_sys, term.get())); }
    void assembleProblem(const BoundaryTerm& term) { check(l3k_mfs_add_boundary(m_sys, term.get())); }
    // the coverage mask and the count of active rows; no term may be added afterwards
    void         endAssembly() { check(l3k_mfs_finalize(m_sys)); }
    l3k_mfs_info info() const
    {
        l3k_mfs_info i{};
        check(l3k_mfs_info_get(m_sys, &i));
        return i;
    }
    // 1 on the local dofs a term has an entry on, 0 elsewhere, into d_mask [n_local_dofs]
    void active(uint8_t* d_mask) const { check(l3k_mfs_active(m_sys, d_mask)); }
    // Y <- alpha*A*X + beta*Y, A the sum of the terms (Operator::apply)
    void apply(const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols = 1, double alpha = 1., double beta = 0.) const
    {
        check(l3k_mfs_apply(m_sys, d_x, ldx, d_y, ldy, ncols, alpha, beta));
    }
    // diag(A) and rhs with Dirichlet lifting, summed over the terms; the caller zeroes d_diag / d_rhs first
    void diagAndRhs(const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr) const
    {
        check(l3k_mfs_diag_rhs(m_sys, 2, d_dirichlet_vals, ldg, d_diag, d_rhs, ldr, nullptr, nullptr, 0, 1));
    }
    void jacobiInverse(const double* d_diag, double* d_minv, double damping = 1., double threshold = 0.) const
    {
        check(l3k_mfs_jacobi_inverse(m_sys, d_diag, damping, threshold, d_minv));
    }
    // alg_sys.solve(CG{opts, NativeJacobiOpts{}}): d_x holds the initial guess and the result; throws if not converged
    l3k_cg_result solve(const double* d_b, double* d_x, const double* d_minv, l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        l3k_cg_result res{};
        check(l3k_mfs_pcg_solve(m_sys, d_b, d_x, d_minv, &opts, &res));
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    std::vector< l3k_cg_result > solve(const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                                       l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        std::vector< l3k_cg_result > res(static_cast< size_t >(ncols));
        check(l3k_mfs_pcg_solve_cols(m_sys, d_b, ldb, d_x, ldx, ncols, d_minv, &opts, res.data()));
        for (const auto& r : res)
            if (!r.converged)
                throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    // the Chebyshev-Jacobi preconditioner of the sum and the solve with it
    Chebyshev chebyshev(const double* d_minv, l3k_cheb_opts opts = {1, 30., 10, 1.1, 0.}) const
    {
        l3k_cheb* c = nullptr;
        check(l3k_mfs_cheb_create(m_sys, d_minv, &opts, &c));
        return Chebyshev{c};
    }
    l3k_cg_result solve(const double* d_b, double* d_x, const Chebyshev& cheb, l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        l3k_cg_result res{};
        check(l3k_mfs_pcg_solve_cheb(m_sys, d_b, d_x, cheb.get(), &opts, &res));
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    void     applyEnergy(const double* d_x, double* d_y, double* d_s) const { check(l3k_mfs_apply_energy(m_sys, d_x, d_y, d_s)); }
    int64_t  nOwnedDofs() const { return m_n; }
    l3k_mfs* get() const { return m_sys; }

private:
    l3k_mfs* m_sys{};
    int64_t  m_n{};
};

// The assembled or condensed system in front of the solver: a square CSR matrix on the device (row_ptr int64 [n + 1], col_ind
// int32 strictly ascending within a row, values -- the arrays assembleGlobal / l3k_condense_global fill).  Nothing is copied: the
// caller keeps the arrays alive and may assemble the values again.  The constructor validates the graph on the device and throws
// on one through which an apply could gather out of bounds.  Applies and solves are bitwise reproducible on any context.
//   apply            ~ tpetra_crsmatrix_t::apply under Belos              solve/BelosSolvers.hpp:116-122
//   diag             ~ getLocalDiagCopy + NativeJacobiImpl::init          solve/NativePreconditioners.hpp:75-96
//   applyDirichlet   ~ DirichletBCAlgebraic::apply                        bcs/DirichletBC.hpp:82-150
//   solve            ~ alg_sys.solve(CG{opts, NativeJacobiOpts{}}) on the assembled matrix
class TriangularPreconditioner;
class CsrOperator
{
public:
    CsrOperator(Context& ctx, int64_t n, const int64_t* d_row_ptr, const int32_t* d_col_ind, double* d_values, int lanes_per_row = 0)
        : m_values{d_values}
    {
        check(l3k_csr_create(ctx.get(), n, d_row_ptr, d_col_ind, d_values, lanes_per_row, &m_csr));
    }
    CsrOperator(const CsrOperator&)            = delete;
    CsrOperator& operator=(const CsrOperator&) = delete;
    ~CsrOperator() { l3k_csr_destroy(m_csr); }
    l3k_csr_info info() const
    {
        l3k_csr_info i{};
        check(l3k_csr_info_get(m_csr, &i));
        return i;
    }
    // Y <- alpha*A*X + beta*Y; beta == 0: Y is not read
    void apply(const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols = 1, double alpha = 1., double beta = 0.) const
    {
        check(l3k_csr_apply(m_csr, d_x, ldx, d_y, ldy, ncols, alpha, beta));
    }
    // Y <- A X and d_s[1] <- <X, A X> in one pass (d_s: 8 device doubles)
    void applyEnergy(const double* d_x, double* d_y, double* d_s) const { check(l3k_csr_apply_energy(m_csr, d_x, d_y, d_s)); }
    // the stored diagonal (0 where none) and / or minv = sign(d) damping / max(|d|, threshold), 0 on an empty row (frozen in the
    // solve); either may be nullptr
    void diag(double* d_diag, double* d_minv, double damping = 1., double threshold = 0.) const
    {
        check(l3k_csr_diag(m_csr, d_diag, damping, threshold, d_minv));
    }
    // in place: identity rows and prescribed values on the flagged dofs, rhs -= A_fd g and A_fd = 0 elsewhere; throws, with
    // nothing changed, if a flagged row stores no diagonal entry
    void applyDirichlet(const uint8_t* d_mask, const double* d_bc_vals, size_t ldg, double* d_rhs, size_t ldr, int ncols = 1) const
    {
        check(l3k_csr_dirichlet(m_csr, m_values, d_mask, d_bc_vals, ldg, d_rhs, ldr, ncols));
    }
    // d_x holds the initial guess and the result; d_minv from diag() (or nullptr); throws if not converged, like the reference
    l3k_cg_result solve(const double* d_b, double* d_x, const double* d_minv, l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        l3k_cg_result res{};
        check(l3k_csr_pcg_solve(m_csr, d_b, d_x, d_minv, &opts, &res));
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    std::vector< l3k_cg_result > solve(const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                                       l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        std::vector< l3k_cg_result > res(static_cast< size_t >(ncols));
        check(l3k_csr_pcg_solve_cols(m_csr, d_b, ldb, d_x, ldx, ncols, d_minv, &opts, res.data()));
        for (const auto& r : res)
            if (!r.converged)
                throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    // alg_sys.solve(CG{opts, Ifpack2SGSOpts{}}) / Ifpack2IluKOpts: PCG with a factored TriangularPreconditioner of this operator
    // (defined below it); the rows that store nothing keep x; throws if not converged
    l3k_cg_result solve(const double* d_b, double* d_x, const TriangularPreconditioner& precond, l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const;
    // the rank-local Dirichlet step with the owner rule on the local matrix of a partitioned system (l3k_csr_dirichlet_dist): mask,
    // values and rhs over the LOCAL dofs [owned | ghost], ghost values imported by the caller; a flagged owned row becomes the
    // identity row with rhs = g, a flagged ghost row an all-zero row with rhs = 0
    void applyDirichletLocal(const uint8_t* d_mask, const double* d_bc_vals_local, size_t ldg, double* d_rhs, size_t ldr, int64_t n_owned,
                             int ncols = 1) const
    {
        check(l3k_csr_dirichlet_dist(m_csr, m_values, d_mask, d_bc_vals_local, ldg, d_rhs, ldr, ncols, n_owned));
    }
    l3k_csr* get() const { return m_csr; }

private:
    l3k_csr* m_csr{};
    double*  m_values{};
};

// The assembled or condensed matrix of a partitioned mesh in front of the solver (l3k_csr_dist_*), in the SUB-ASSEMBLED form: every
// rank keeps the matrix of its own elements over its local dofs [owned | ghost] (a CsrOperator, or the l3k_csr of a partitioned
// AssembledSystem), the global matrix -- their sum -- is never formed, and the halo's exchanges run inside every apply: the Tpetra
// matrix of an MPI run of the reference in front of Belos (solve/BelosSolvers.hpp:116-122).  Vectors hold the owned rows only.
//   apply   ~ tpetra_crsmatrix_t::apply: import || interior rows, border and ghost rows, export || interior rows, unpack-add
//   diag    ~ getLocalDiagCopy of the global matrix on the owned rows + NativeJacobiImpl::init; collective
//   info    ~ n_owned, n_ghost, the three row counts and lists, the local l3k_csr
// The local operator and the halo must outlive the object.
class DistributedCsr
{
public:
    DistributedCsr(const CsrOperator& local, const Halo& halo, int64_t n_owned) : m_owner{true}
    {
        check(l3k_csr_dist_create(local.get(), halo.get(), n_owned, &m_dist));
    }
    // a handle that belongs to somebody else (AssembledSystem::distributed)
    explicit DistributedCsr(l3k_csr_dist* handle) : m_dist{handle}, m_owner{false} {}
    DistributedCsr(const DistributedCsr&)            = delete;
    DistributedCsr& operator=(const DistributedCsr&) = delete;
    DistributedCsr(DistributedCsr&& o) noexcept : m_dist{o.m_dist}, m_owner{o.m_owner} { o.m_dist = nullptr; }
    ~DistributedCsr()
    {
        if (m_owner)
            l3k_csr_dist_destroy(m_dist);
    }
    l3k_csr_dist_info info() const
    {
        l3k_csr_dist_info i{};
        check(l3k_csr_dist_info_get(m_dist, &i));
        return i;
    }
    // Y <- alpha*A*X + beta*Y on the owned rows; beta == 0: Y is not read
    void apply(const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols = 1, double alpha = 1., double beta = 0.) const
    {
        check(l3k_csr_dist_apply(m_dist, d_x, ldx, d_y, ldy, ncols, alpha, beta));
    }
    // the global diagonal on the owned rows and / or minv = sign(d) damping / max(|d|, threshold), 0 on an empty owned row
    void diag(double* d_diag, double* d_minv, double damping = 1., double threshold = 0.) const
    {
        check(l3k_csr_dist_diag(m_dist, d_diag, damping, threshold, d_minv));
    }
    // Y <- A X on the owned rows and d_s[1] <- this rank's share of <X, A X> (d_s: 8 device doubles; collective)
    void applyEnergy(const double* d_x, double* d_y, double* d_s) const { check(l3k_csr_dist_apply_energy(m_dist, d_x, d_y, d_s)); }
    // alg_sys.solve(CG{...}) on every rank of an MPI run of the reference (solve/BelosSolvers.hpp:116-122): the collective solve over
    // the owned rows, the reductions through the operator's halo; cheb == nullptr: Jacobi with d_minv from diag(), else the
    // preconditioner of chebyshev(...) (d_minv may then be nullptr).  Every rank returns the same result; throws if not converged
    l3k_cg_result pcgSolve(const double* d_b, double* d_x, const double* d_minv, l3k_cg_opts opts = {1e-6, 10000, 0, 1},
                           const Chebyshev* cheb = nullptr) const
    {
        l3k_cg_result res{};
        check(l3k_csr_dist_pcg_solve(m_dist, d_b, d_x, d_minv, cheb ? cheb->get() : nullptr, &opts, &res));
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    // alg_sys.solve(Gmres{...}) on every rank (solve/BelosSolvers.hpp:124-131): the collective GMRES over the owned rows with the
    // workspace Gmres::collective(ctx, n_owned, restart_length), the reductions through the operator's halo (defined below Gmres).
    // cheb == nullptr: Jacobi with d_minv, or no preconditioner when d_minv is nullptr too.  Every rank returns the same result;
    // throws if not converged
    l3k_gmres_result gmresSolve(const Gmres& workspace, const double* d_b, double* d_x, const double* d_minv,
                                l3k_gmres_opts opts = {1e-6, 10000, 0, 1, 39}, const Chebyshev* cheb = nullptr) const;
    // collective; lambda_max == 0: estimated by the power method on D^-1 A across the ranks
    Chebyshev chebyshev(const double* d_minv, l3k_cheb_opts opts = {1, 30., 10, 1.1, 0.}) const
    {
        l3k_cheb* c = nullptr;
        check(l3k_csr_dist_cheb_create(m_dist, d_minv, &opts, &c));
        return Chebyshev{c};
    }
    l3k_csr_dist* get() const { return m_dist; }

private:
    l3k_csr_dist* m_dist{};
    bool          m_owner{};
};

// The sparse direct solver on a single-rank CSR operator (l3k_chol_*): band Cholesky for the symmetric positive definite systems
// of the assembled path, where the reference solves with Amesos2 (alg_sys.solve(Klu2{}) / Lapack{}, solve/Amesos2Solvers.hpp:18-32).
// The constructor runs the symbolic phase (host) and throws on a structurally unsymmetric graph or a factor above max_bytes
// (0 = 8 GiB); block: 0 = chosen, 32 or 64.  The operator (a CsrOperator, or the l3k_csr of a closed AssembledSystem) must outlive
// the object.  RAII, move-only.
//   factor   ~ numericFactorization of the operator's current values; throws "matrix is not positive definite" (see info)
//   solve    ~ X <- A^-1 B on the rows that store entries, ncols columns; B and X may be the same buffer
//   info     ~ n, n_active, n_blocks, block, max_height, factor_bytes, factor_flops, n_bad_pivots, first_bad_row, factored
class Cholesky
{
public:
    explicit Cholesky(l3k_csr* A, size_t max_bytes = 0, int block = 0)
    {
        const l3k_chol_opts o{max_bytes, block};
        check(l3k_chol_create(A, &o, &m_chol));
    }
    explicit Cholesky(const CsrOperator& A, size_t max_bytes = 0, int block = 0) : Cholesky{A.get(), max_bytes, block} {}
    Cholesky(const Cholesky&)            = delete;
    Cholesky& operator=(const Cholesky&) = delete;
    Cholesky(Cholesky&& o) noexcept : m_chol{o.m_chol} { o.m_chol = nullptr; }
    ~Cholesky() { l3k_chol_destroy(m_chol); }
    void factor() { check(l3k_chol_factor(m_chol)); }
    void solve(const double* d_b, double* d_x) const { check(l3k_chol_solve(m_chol, d_b, 0, d_x, 0, 1)); }
    void solve(const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols) const
    {
        check(l3k_chol_solve(m_chol, d_b, ldb, d_x, ldx, ncols));
    }
    l3k_chol_info info() const
    {
        l3k_chol_info i{};
        check(l3k_chol_info_get(m_chol, &i));
        return i;
    }
    l3k_chol* get() const { return m_chol; }

private:
    l3k_chol* m_chol{};
};

// Symmetric Gauss-Seidel or ILU(0) on a single-rank CSR operator (l3k_tri_*), where the reference uses Ifpack2 (Ifpack2SGSOpts,
// Ifpack2IluKOpts with level of fill 0: solve/Ifpack2Preconditioners.hpp:97-101,134-157; tests/SolverTests.cpp:221-232): level-scheduled
// sparse triangular solves in the operator's pattern.  The constructor runs the symbolic phase (host) and throws on an active row
// without a stored diagonal entry; opts as l3k_tri_opts (kind L3K_TRI_SGS or L3K_TRI_ILU0, damping, the two thresholds, fuse_rows).
// The operator (a CsrOperator, or the l3k_csr of a closed AssembledSystem) must outlive the object.  RAII, move-only.
//   factor       ~ compute() on the operator's current values; throws on a zero or non-finite pivot (see info)
//   apply        ~ z <- M^-1 r; r and z distinct; 0 on the rows that store nothing
//   solveLower, solveUpper ~ the two halves of apply
//   values       ~ ILU(0): the nnz factor values in the operator's pattern
//   info         ~ levels, launches, bytes, n_bad_pivots, first_bad_row, factored
// CsrOperator::solve and Gmres::solve take the factored object as the preconditioner.
class TriangularPreconditioner
{
public:
    static constexpr l3k_tri_opts sgs{L3K_TRI_SGS, 1., 0., 1., 0}, ilu0{L3K_TRI_ILU0, 1., 0., 1., 0};
    explicit TriangularPreconditioner(l3k_csr* A, const l3k_tri_opts& opts = ilu0) { check(l3k_tri_create(A, &opts, &m_tri)); }
    explicit TriangularPreconditioner(const CsrOperator& A, const l3k_tri_opts& opts = ilu0) : TriangularPreconditioner{A.get(), opts} {}
    TriangularPreconditioner(const TriangularPreconditioner&)            = delete;
    TriangularPreconditioner& operator=(const TriangularPreconditioner&) = delete;
    TriangularPreconditioner(TriangularPreconditioner&& o) noexcept : m_tri{o.m_tri} { o.m_tri = nullptr; }
    ~TriangularPreconditioner() { l3k_tri_destroy(m_tri); }
    void factor() { check(l3k_tri_factor(m_tri)); }
    void apply(const double* d_r, double* d_z) const { check(l3k_tri_apply(m_tri, d_r, d_z)); }
    void solveLower(const double* d_r, double* d_y) const { check(l3k_tri_solve_lower(m_tri, d_r, d_y)); }
    void solveUpper(const double* d_y, double* d_z) const { check(l3k_tri_solve_upper(m_tri, d_y, d_z)); }
    void values(double* d_out) const { check(l3k_tri_values(m_tri, d_out)); }
    l3k_tri_info info() const
    {
        l3k_tri_info i{};
        check(l3k_tri_info_get(m_tri, &i));
        return i;
    }
    l3k_tri* get() const { return m_tri; }

private:
    l3k_tri* m_tri{};
};
inline l3k_cg_result CsrOperator::solve(const double* d_b, double* d_x, const TriangularPreconditioner& precond, l3k_cg_opts opts) const
{
    l3k_cg_result res{};
    check(l3k_csr_pcg_solve_tri(m_csr, d_b, d_x, precond.get(), &opts, &res));
    if (!res.converged)
        throw std::runtime_error{"Solver failed to converge"};
    return res;
}

// Restarted GMRES(restart_length) on a single-rank operator (l3k_gmres_*): alg_sys.solve(Gmres{opts, precond}), the reference's
// second Krylov solver (solve/BelosSolvers.hpp:124-130, restart_length = 250 and max_restarts = 39 of solve/SolverInterface.hpp:26-37),
// for systems that are not symmetric positive definite.  The object is the workspace on n rows (restart_length above n is lowered
// to n; max_bytes: 0 = no guard, otherwise the constructor throws and names the bytes needed); it serves any number of solves.
// The preconditioner acts on the right: achieved_tol is the true residual over the rows with minv != 0, which keep x.  RAII, move-only.
//   solve(system, b, x, minv)  ~ no preconditioner (nullptr) or Jacobi; throws "Solver failed to converge" like the reference
//   solve(system, b, x, cheb)  ~ with the Chebyshev-Jacobi preconditioner created on that system
//   info                       ~ n, ld, restart_length, bytes
class Gmres
{
public:
    static constexpr l3k_gmres_opts default_opts{1e-6, 10000, 0, 1, 39};
    Gmres(Context& ctx, int64_t n, int restart_length = 250, size_t max_bytes = 0)
    {
        check(l3k_gmres_create(ctx.get(), n, restart_length, max_bytes, &m_gmres));
    }
    // the workspace of one rank of a collective solve (MatrixFreeSystem::gmresSolve(halo, ...), DistributedCsr::gmresSolve): n_owned
    // may be 0 and does not lower restart_length, which every rank gives alike (l3k_gmres_create_dist)
    static Gmres collective(Context& ctx, int64_t n_owned, int restart_length = 250, size_t max_bytes = 0)
    {
        l3k_gmres* g = nullptr;
        check(l3k_gmres_create_dist(ctx.get(), n_owned, restart_length, max_bytes, &g));
        return Gmres{g};
    }
    Gmres(const Gmres&)            = delete;
    Gmres& operator=(const Gmres&) = delete;
    Gmres(Gmres&& o) noexcept : m_gmres{o.m_gmres} { o.m_gmres = nullptr; }
    ~Gmres() { l3k_gmres_destroy(m_gmres); }
    l3k_gmres_result solve(const MatrixFreeSystem& A, const double* d_b, double* d_x, const double* d_minv, l3k_gmres_opts opts = default_opts) const
    {
        l3k_gmres_result res{};
        check(l3k_gmres_solve(m_gmres, A.get(), d_b, d_x, d_minv, &opts, &res));
        return converged(res);
    }
    l3k_gmres_result solve(const MatrixFreeSystem& A, const double* d_b, double* d_x, const Chebyshev& cheb, l3k_gmres_opts opts = default_opts) const
    {
        l3k_gmres_result res{};
        check(l3k_gmres_solve_cheb(m_gmres, A.get(), d_b, d_x, cheb.get(), &opts, &res));
        return converged(res);
    }
    l3k_gmres_result solve(const MultiTermSystem& A, const double* d_b, double* d_x, const double* d_minv, l3k_gmres_opts opts = default_opts) const
    {
        l3k_gmres_result res{};
        check(l3k_mfs_gmres_solve(m_gmres, A.get(), d_b, d_x, d_minv, &opts, &res));
        return converged(res);
    }
    l3k_gmres_result solve(const MultiTermSystem& A, const double* d_b, double* d_x, const Chebyshev& cheb, l3k_gmres_opts opts = default_opts) const
    {
        l3k_gmres_result res{};
        check(l3k_mfs_gmres_solve_cheb(m_gmres, A.get(), d_b, d_x, cheb.get(), &opts, &res));
        return converged(res);
    }
    l3k_gmres_result solve(const CsrOperator& A, const double* d_b, double* d_x, const double* d_minv, l3k_gmres_opts opts = default_opts) const
    {
        l3k_gmres_result res{};
        check(l3k_csr_gmres_solve(m_gmres, A.get(), d_b, d_x, d_minv, &opts, &res));
        return converged(res);
    }
    l3k_gmres_result solve(const CsrOperator& A, const double* d_b, double* d_x, const Chebyshev& cheb, l3k_gmres_opts opts = default_opts) const
    {
        l3k_gmres_result res{};
        check(l3k_csr_gmres_solve_cheb(m_gmres, A.get(), d_b, d_x, cheb.get(), &opts, &res));
        return converged(res);
    }
    l3k_gmres_result solve(const CsrOperator& A, const double* d_b, double* d_x, const TriangularPreconditioner& precond,
                           l3k_gmres_opts opts = default_opts) const
    {
        l3k_gmres_result res{};
        check(l3k_csr_gmres_solve_tri(m_gmres, A.get(), d_b, d_x, precond.get(), &opts, &res));
        return converged(res);
    }
    l3k_gmres_info info() const
    {
        l3k_gmres_info i{};
        check(l3k_gmres_info_get(m_gmres, &i));
        return i;
    }
    l3k_gmres* get() const { return m_gmres; }

    static l3k_gmres_result converged(const l3k_gmres_result& res)
    {
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"}; // solve/BelosSolvers.hpp:103
        return res;
    }

private:
    explicit Gmres(l3k_gmres* handle) : m_gmres{handle} {}
    l3k_gmres* m_gmres{};
};
inline l3k_gmres_result MatrixFreeSystem::gmresSolve(const Gmres& workspace, const Halo& halo, const double* d_b, double* d_x,
                                                     const double* d_minv, l3k_gmres_opts opts, const Chebyshev* cheb) const
{
    l3k_gmres_result res{};
    check(l3k_gmres_solve_dist(workspace.get(), m_mf, halo.get(), d_b, d_x, d_minv, cheb ? cheb->get() : nullptr, &opts, &res));
    return Gmres::converged(res);
}
inline l3k_gmres_result DistributedCsr::gmresSolve(const Gmres& workspace, const double* d_b, double* d_x, const double* d_minv,
                                                   l3k_gmres_opts opts, const Chebyshev* cheb) const
{
    l3k_gmres_result res{};
    check(l3k_csr_dist_gmres_solve(workspace.get(), m_dist, d_b, d_x, d_minv, cheb ? cheb->get() : nullptr, &opts, &res));
    return Gmres::converged(res);
}

// The CSR sparsity graph of a mesh over its local dofs, built on the device: computeLocalGraph in front of makeSparsityGraph
// (algsys/SparsityGraph.hpp:26-81, :299) for one rank.  field_inds strictly ascending, empty = all dofs of the node; kind
// L3K_GRAPH_FULL or L3K_GRAPH_CONDENSED (primary nodes only, hexes).  The mesh must outlive the object.
//   info   ~ n, nnz, n_empty_rows, max_row_len, n_rows_scratch, workspace_bytes, max_elems_per_node, lds_key_capacity
//   fill   ~ d_row_ptr int64 [n + 1], d_col_ind int32 [nnz] (columns ascending): what assembleGlobal / condenseGlobal and
//            CsrOperator take; may be called more than once
class Graph
{
public:
    Graph(const DeviceMesh& mesh, std::span< const int > field_inds = {}, int kind = L3K_GRAPH_FULL)
    {
        check(l3k_graph_create(mesh.get(), int(field_inds.size()), field_inds.empty() ? nullptr : field_inds.data(), kind, &m_graph));
    }
    Graph(const Graph&)            = delete;
    Graph& operator=(const Graph&) = delete;
    ~Graph() { l3k_graph_destroy(m_graph); }
    l3k_graph_info info() const
    {
        l3k_graph_info i{};
        check(l3k_graph_info_get(m_graph, &i));
        return i;
    }
    void       fill(int64_t* d_row_ptr, int32_t* d_col_ind) const { check(l3k_graph_fill(m_graph, d_row_ptr, d_col_ind)); }
    l3k_graph* get() const { return m_graph; }

private:
    l3k_graph* m_graph{};
};

// algsys::AssembledSystem for one rank, on hexes and on quads (l3k_asm_*): the object owns the CSR arrays of the full sparsity graph
// of field_inds (empty: all dofs of the node) and the right-hand sides; workspace_bytes sizes the sub-batches.  RAII, move-only.
//   beginAssembly          ~ AssembledSystem::beginAssembly: values and rhs <- 0, the system is open (any state)
//   assembleProblem(term)  ~ assembleProblem(domain kernel, domain ids) / (boundary kernel, boundary ids): the element / side
//                            systems of the term's elements / sides [first, first + count) summed into values and rhs
//   endAssembly            ~ endAssembly + DirichletBCAlgebraic::apply with the mesh's mask; d_dirichlet_vals [n_rhs][ldg] or nullptr
//   solve                  ~ alg_sys.solve(CG{opts, NativeJacobiOpts{}}): Jacobi PCG on the closed system's CSR operator, column 0
//   info                   ~ n, nnz, n_missing, ldr, n_rhs, state, the device arrays and (closed) the l3k_csr handle for l3k_csr_*
// Condensation::ElementBoundary (quads; CondensationPolicy::ElementBoundary, algsys/StaticCondensationManager.hpp:259-473) eliminates
// the element-internal dofs in endAssembly (l3k_asm_create_condensed): the matrix couples the primary dofs only, and
//   recover                ~ recoverSolution: the internal dofs of d_x [n_rhs][ldx] from its solved primary dofs
//   schurUpdates           ~ K_bi K_ii^-1 K_ib [count][Nb][Nb] and K_bi K_ii^-1 F_i [count][n_rhs][Nb] of the elements, either may be null
//   condInfo               ~ the sizes of the per-element store and the elements that failed the pivot test of the last endAssembly
enum class Condensation
{
    None,
    ElementBoundary
};
class AssembledSystem
{
public:
    AssembledSystem(const DeviceMesh& mesh, std::span< const int > field_inds = {}, int n_rhs = 1, size_t workspace_bytes = 0,
                    Condensation condensation = Condensation::None)
    {
        check((condensation == Condensation::ElementBoundary ? l3k_asm_create_condensed : l3k_asm_create)(
            mesh.get(), int(field_inds.size()), field_inds.empty() ? nullptr : field_inds.data(), n_rhs, workspace_bytes, &m_asm));
    }
    // One rank of a partitioned mesh (l3k_asm_create_dist): the arrays hold the local matrix over the local dofs [owned | ghost];
    // beginAssembly and assembleProblem are rank-local, endAssembly is collective and takes d_dirichlet_vals over the OWNED dofs
    // (ldg >= n_owned), distributed() is then the operator for the solver and the first n_owned entries of a row of info().d_rhs
    // the owned right-hand side; recover is collective and takes d_x over the local dofs with the owned part filled
    AssembledSystem(const DeviceMesh& mesh, const Halo& halo, std::span< const int > field_inds = {}, int n_rhs = 1,
                    size_t workspace_bytes = 0, Condensation condensation = Condensation::None)
    {
        check(l3k_asm_create_dist(mesh.get(), halo.get(), int(field_inds.size()), field_inds.empty() ? nullptr : field_inds.data(), n_rhs,
                                  workspace_bytes, condensation == Condensation::ElementBoundary ? 1 : 0, &m_asm));
    }
    AssembledSystem(const AssembledSystem&)            = delete;
    AssembledSystem& operator=(const AssembledSystem&) = delete;
    AssembledSystem(AssembledSystem&& o) noexcept : m_asm{o.m_asm} { o.m_asm = nullptr; }
    AssembledSystem& operator=(AssembledSystem&& o) noexcept
    {
        if (this != &o)
        {
            l3k_asm_destroy(m_asm);
            m_asm   = o.m_asm;
            o.m_asm = nullptr;
        }
        return *this;
    }
    ~AssembledSystem() { l3k_asm_destroy(m_asm); }
    void beginAssembly() { check(l3k_asm_begin(m_asm)); }
    void assembleProblem(const MatrixFreeSystem& term, int64_t first, int64_t count)
    {
        check(l3k_asm_add_domain(m_asm, term.get(), first, count));
    }
    void assembleProblem(const BoundaryTerm& term, int64_t first, int64_t count)
    {
        check(l3k_asm_add_boundary(m_asm, term.get(), first, count));
    }
    void endAssembly(const double* d_dirichlet_vals = nullptr, size_t ldg = 0) { check(l3k_asm_end(m_asm, d_dirichlet_vals, ldg)); }
    l3k_asm_info info() const
    {
        l3k_asm_info i{};
        check(l3k_asm_info_get(m_asm, &i));
        return i;
    }
    // d_x holds the initial guess and the result, d_minv [n] receives the Jacobi preconditioner of the matrix; throws if the
    // system is not closed or the solver does not converge
    l3k_cg_result solve(double* d_x, double* d_minv, l3k_cg_opts opts = {1e-6, 10000, 0, 1}) const
    {
        const l3k_asm_info i = info();
        if (!i.csr)
            throw std::runtime_error{"AssembledSystem::solve: the system is not closed (endAssembly)"};
        check(l3k_csr_diag(i.csr, nullptr, 1., 0., d_minv));
        l3k_cg_result res{};
        check(l3k_csr_pcg_solve(i.csr, i.d_rhs, d_x, d_minv, &opts, &res));
        if (!res.converged)
            throw std::runtime_error{"Solver failed to converge"};
        return res;
    }
    void recover(double* d_x, size_t ldx) { check(l3k_asm_recover(m_asm, d_x, ldx)); }
    void schurUpdates(int64_t first, int64_t count, double* d_W, double* d_w) { check(l3k_asm_schur_updates(m_asm, first, count, d_W, d_w)); }
    l3k_asm_cond_info condInfo() const
    {
        l3k_asm_cond_info i{};
        check(l3k_asm_cond_info_get(m_asm, &i));
        return i;
    }
    // a partitioned system: n_owned, n_ghost and (closed) the l3k_csr_dist handle
    l3k_asm_dist_info distInfo() const
    {
        l3k_asm_dist_info i{};
        check(l3k_asm_dist_info_get(m_asm, &i));
        return i;
    }
    // the operator of a closed partitioned system (the system owns the handle and must outlive the result)
    DistributedCsr distributed() const
    {
        const l3k_asm_dist_info i = distInfo();
        if (!i.dist)
            throw std::runtime_error{"AssembledSystem::distributed: the system is not closed (endAssembly)"};
        return DistributedCsr{i.dist};
    }
    l3k_asm* get() const { return m_asm; }

private:
    l3k_asm* m_asm{};
};

// convertMeshToOrder< order >(mesh_o1) for one rank's hexahedra (mesh/ConvertMeshToOrder.hpp:51-104), on the device:
// conn = [n_elems][8] vertex ids, local vertex i + 2j + 4k.  Returns the element-node table [n_elems][(order+1)^3] in the
// numbering [vertices | edge nodes | face nodes | element-internal nodes]; n_nodes receives the node count.
inline std::vector< uint32_t > elevateOrder(Context& ctx, std::span< const uint32_t > conn, int64_t n_vertices, int order,
                                            int64_t& n_nodes)
{
    const int64_t           n_elems = int64_t(conn.size() / 8), N = int64_t(order + 1) * (order + 1) * (order + 1);
    std::vector< uint32_t > elem_nodes(size_t(n_elems * N));
    int64_t                 n_noninternal = 0;
    check(l3k_elevate_order(ctx.get(), n_elems, conn.data(), n_vertices, order, elem_nodes.data(), &n_nodes, &n_noninternal));
    return elem_nodes;
}

// BCDefinition::definePeriodic(src_ids, dst_ids, translation) (bcs/BCDefinition.hpp:92-104, bcs/PeriodicBC.hpp) in two steps, as in
// l3k.h.  periodicMatch: the node pairs (source node, the destination node it is the image of) of the listed element sides, found
// from geometry on the device; throws through check() on bad arguments, reports unmatched source nodes in the result.
struct PeriodicPairs
{
    std::vector< uint32_t > src, dst;
    int64_t                 n_unmatched = 0, n_ambiguous = 0, first_unmatched = -1;
};
inline PeriodicPairs periodicMatch(Context& ctx, int dim, int order, std::span< const uint32_t > elem_nodes,
                                   std::span< const double > elem_verts, std::span< const int64_t > src_elem,
                                   std::span< const uint8_t > src_side, std::span< const int64_t > dst_elem,
                                   std::span< const uint8_t > dst_side, const std::array< double, 3 >& translation,
                                   double tolerance = 1e-12)
{
    int64_t nodes_per_elem = 1, nodes_per_side = 1;
    for (int a = 0; a < dim; ++a)
        nodes_per_side = nodes_per_elem, nodes_per_elem *= order + 1;
    const int64_t n_elems = nodes_per_elem ? int64_t(elem_nodes.size()) / nodes_per_elem : 0;
    PeriodicPairs out;
    out.src.resize(src_elem.size() * size_t(nodes_per_side));
    out.dst.resize(out.src.size());
    int64_t n_pairs = 0;
    check(l3k_periodic_match(ctx.get(), dim, order, n_elems, elem_nodes.data(), elem_verts.data(), int64_t(src_elem.size()),
                             src_elem.data(), src_side.data(), int64_t(dst_elem.size()), dst_elem.data(), dst_side.data(),
                             translation.data(), tolerance, out.src.data(), out.dst.data(), &n_pairs, &out.n_unmatched,
                             &out.n_ambiguous, &out.first_unmatched));
    out.src.resize(size_t(n_pairs));
    out.dst.resize(size_t(n_pairs));
    return out;
}
// periodicMerge: the pairs (of one or several periodicMatch calls on the unmerged mesh) carried out on elem_nodes in place; returns
// node_map (old -> new); n_nodes and n_noninternal are updated.
inline std::vector< uint32_t > periodicMerge(std::span< uint32_t > elem_nodes, int64_t& n_nodes, int64_t& n_noninternal,
                                             std::span< const uint32_t > pair_a, std::span< const uint32_t > pair_b,
                                             int64_t* n_components = nullptr)
{
    if (pair_a.size() != pair_b.size())
        throw std::runtime_error{"periodicMerge: pair_a and pair_b must have the same length"};
    std::vector< uint32_t > node_map(size_t(n_nodes > 0 ? n_nodes : 0));
    int64_t                 nn = 0, nni = 0, nc = 0;
    check(l3k_periodic_merge(n_nodes, n_noninternal, int64_t(pair_a.size()), pair_a.data(), pair_b.data(), int64_t(elem_nodes.size()),
                             elem_nodes.data(), node_map.data(), &nn, &nni, &nc));
    n_nodes       = nn;
    n_noninternal = nni;
    if (n_components)
        *n_components = nc;
    return node_map;
}

// save(comm, mesh, solution_manager, path, inds, comment) / Loader::loadResults of post/NativeIO.hpp for this rank's owned
// nodes [node_begin, node_begin + n_local): fields = [n_fields][ld] host values
inline void saveResults(const char* path, const char* comment, size_t n_fields, int64_t n_global_nodes, int64_t node_begin,
                        int64_t n_local, const double* fields, size_t ld, bool write_header = true)
{
    check(l3k_results_save(path, comment, n_fields, n_global_nodes, node_begin, n_local, fields, ld, write_header ? 1 : 0));
}
inline std::vector< double > loadResults(const char* path, size_t field, std::span< const int64_t > node_ids)
{
    std::vector< double > out(node_ids.size());
    check(l3k_results_load(path, field, int64_t(node_ids.size()), node_ids.data(), 0, out.data()));
    return out;
}

// save(comm, mesh, path, comment) / loadPartitionedMesh of post/NativeIO.hpp:75-108, :219-232 for this rank's part; the
// sizes of all parts are gathered by the caller (the reference: comm.gather at :83)
inline size_t meshFilePartBytes(const l3k_meshfile_part_desc& desc)
{
    size_t bytes = 0;
    check(l3k_meshfile_part_bytes(&desc, &bytes));
    return bytes;
}
inline void saveMesh(const char* path, const char* comment, std::span< const size_t > part_bytes, size_t part,
                     const l3k_meshfile_part_desc& desc)
{
    check(l3k_meshfile_save(path, comment, part_bytes.size(), part_bytes.data(), part, &desc, part == 0 ? 1 : 0));
}
class LoadedMeshPart
{
public:
    LoadedMeshPart(const char* path, size_t part, int order) { check(l3k_meshfile_load(path, part, order, &m_part)); }
    ~LoadedMeshPart() { l3k_meshfile_part_destroy(m_part); }
    LoadedMeshPart(const LoadedMeshPart&)            = delete;
    LoadedMeshPart& operator=(const LoadedMeshPart&) = delete;
    l3k_meshfile_part_desc get() const // the arrays live as long as this object
    {
        l3k_meshfile_part_desc d{};
        check(l3k_meshfile_part_get(m_part, &d));
        return d;
    }

private:
    l3k_meshfile_part* m_part = nullptr;
};

// ExportDefinition (post/VtkExport.hpp:16-39): a file name and named groups of 1, 2 or 3 rows of the SoA field storage
class ExportDefinition
{
public:
    struct FieldDef
    {
        std::string        name;
        std::vector< int > inds;
    };
    explicit ExportDefinition(std::string file_name) : m_file_name{std::move(file_name)} {}
    void defineField(std::string name, std::span< const int > inds)
    {
        m_defs.push_back(FieldDef{std::move(name), {inds.begin(), inds.end()}});
    }
    void               defineField(std::string name, std::initializer_list< int > inds) { defineField(std::move(name), std::span{inds}); }
    const std::string& fileName() const { return m_file_name; }
    auto               begin() const { return m_defs.begin(); }
    auto               end() const { return m_defs.end(); }
    size_t             size() const { return m_defs.size(); }

private:
    std::string             m_file_name;
    std::vector< FieldDef > m_defs;
};

// PvtuExporter (post/VtkExport.hpp:41-97) of one rank's DeviceMesh (l3k_vtk_*): the constructor computes the node coordinates and
// the sub-cell topology on the device and keeps their text; exportSolution writes `<name>_<rank>.vtu` and, on rank 0, `<name>.pvtu`
// from the SoA field storage d_fields (n_fields, ld) on the device.  Where the reference takes the communicator, this takes rank and
// size: no rank talks to another.  The files are complete on return (no write queue, hence no flushWriteQueue); meshes are immutable
// (no updateNodeCoords: create a new exporter).  RAII, move-only; the mesh must outlive the object.
class PvtuExporter
{
public:
    explicit PvtuExporter(const DeviceMesh& mesh, int rank = 0, int n_ranks = 1, size_t chunk_bytes = 0) : m_rank{rank}, m_n_ranks{n_ranks}
    {
        const l3k_vtk_opts o{chunk_bytes};
        check(l3k_vtk_create(mesh.get(), &o, &m_vtk));
    }
    PvtuExporter(const PvtuExporter&)            = delete;
    PvtuExporter& operator=(const PvtuExporter&) = delete;
    PvtuExporter(PvtuExporter&& o) noexcept : m_vtk{o.m_vtk}, m_rank{o.m_rank}, m_n_ranks{o.m_n_ranks} { o.m_vtk = nullptr; }
    ~PvtuExporter() { l3k_vtk_destroy(m_vtk); }
    void exportSolution(const ExportDefinition& export_def, const double* d_fields, size_t ld, int n_fields) const
    {
        std::vector< const char* > names;
        std::vector< int >         n_comps, inds;
        for (const auto& def : export_def)
        {
            names.push_back(def.name.c_str());
            n_comps.push_back(int(def.inds.size()));
            inds.insert(inds.end(), def.inds.begin(), def.inds.end());
        }
        check(l3k_vtk_export(m_vtk, export_def.fileName().c_str(), m_rank, m_n_ranks, int(names.size()), names.data(), n_comps.data(),
                             inds.data(), d_fields, ld, n_fields));
    }
    l3k_vtk_info info() const
    {
        l3k_vtk_info i{};
        check(l3k_vtk_info_get(m_vtk, &i));
        return i;
    }
    l3k_vtk* get() const { return m_vtk; }

private:
    l3k_vtk* m_vtk{};
    int      m_rank{}, m_n_ranks{};
};
} // namespace l3k
#endif
