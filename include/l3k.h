/* l3k.h -- C ABI of the MI355X-native element-local hot path (libl3k.so).
 *
 * Drop-in boundary for the L3STER hot path.  The reference is header-only C++ with no FFI; each entry
 * point below names the reference interface (file:line under /root/reference/include/l3ster) it stands in for.  Plain
 * pointers and sizes only; never throws across the boundary: every function returns 0 on success, < 0 on error, and
 * l3k_last_error() gives the text (the reference throws std::runtime_error from util::throwingAssert,
 * util/Assertion.hpp:88-95).
 *
 * Pointer conventions: arguments named d_* are DEVICE pointers (HBM of the ctx's GPU); everything else is host memory.
 * Vectors are column-major [row][col] with an explicit leading dimension, owned rows only, exactly like the host view
 * of the Tpetra multivectors the reference's Operator::apply works on (algsys/ComputeValuesAtNodes.hpp:27-31,62-65).
 * Calls on one l3k_ctx are serialised by the caller (the reference's apply is not re-entrant either: shared
 * import/export buffers, algsys/MatrixFreeSystem.hpp:1008-1009).  All device work is enqueued on the ctx's HIP stream
 * and is asynchronous with respect to the host unless stated otherwise.
 */
#ifndef L3K_H
#define L3K_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 101 (round 4): l3k_cg_update_xr / _update_p replaced by l3k_cg_update_z / _update_px (the iteration keeps z = M^-1 r; d_r holds z),
 * new: l3k_ctx_set_reference_z0, l3k_ctx_get/set_tuning, l3k_mf_route, l3k_update_solution, l3k_pcg_solve_cols */
/* Quadrilateral meshes (dim = 2) on the device -- l3k_mesh_create, the matrix-free apply and l3k_mf_diag_rhs, kernels
 * L3K_KERNEL_DIFFUSION2D / _VAR, l3k_square_mesh_create; then l3k_bnd_create, l3k_integrate and l3k_values_at_nodes with
 * dim = 2 and the 2-D boundary / residual kernels -- are additions only: no existing entry point changed its behaviour on
 * hexes, so the version stays (tests/test_cabi_cpu.py pins it). */
#define L3K_VERSION 101

typedef struct l3k_ctx      l3k_ctx;
typedef struct l3k_mesh     l3k_mesh;
typedef struct l3k_mf       l3k_mf;
typedef struct l3k_hostmesh l3k_hostmesh;

int         l3k_version(void);
const char* l3k_last_error(void);

/* ---- compile-time structs of the reference, as runtime descriptors ---------------------------------------------- */
/* KernelParams, common/KernelInterface.hpp:13-20 */
typedef struct
{
    int dimension, n_equations, n_unknowns, n_fields, n_rhs;
} l3k_kparams;
/* AssemblyOptions, algsys/AssembleLocalSystem.hpp:24-49.  eval_strategy: 0 Auto, 1 LocalElement, 2 SumFactorization,
 * 3 SumFactorizationOddEvenDecomposition (LocalEvalStrategy, :16-22).  On the device every strategy runs the same
 * sum-factorised kernel (collocation-derivative form, mathematically identical). */
typedef struct
{
    int value_order, derivative_order, eval_strategy;
} l3k_asmopts;

/* ---- tables (host; no GPU needed) ------------------------------------------------------------------------------- */
/* math::getLobattoRuleAbsc, math/LobattoRuleAbsc.hpp:30-35 */
int l3k_gll_nodes(int n, double* x);
/* quad::getReferenceQuadrature<GaussLegendre>, quad/ReferenceQuadrature.hpp:24-51 (nq = QO/2+1 points) */
int l3k_gl_rule(int nq, double* x, double* w);
/* AssemblyOptions::order + getRefQuadSize: nq1d = value_order*p + derivative_order*(p-1) + 1 */
int l3k_n_qps1d(int p, int value_order, int derivative_order);
/* interpolation_matrix / derivative_matrix, algsys/SumFactorization.hpp:25-65: row-major [p+1][nq] */
int l3k_basis_1d(int p, int nq, double* I, double* D);
/* collocation derivative matrix on the nq Gauss points: C[q'][q] = l_q'^GL '(x_q), row-major [nq][nq] (device algorithm
 * table; D = I * C for nq >= p+1) */
int l3k_colloc_deriv(int nq, double* C);

/* out[i][j] = l_j(x_i), row-major [p_to+1][p_from+1]: the order-p_from GLL Lagrange basis at the GLL nodes of order p_to, the 1-D
 * factor of the tensor-product transfer between two orders on one element (l3k_pmg_* below).  The rows of the end nodes are exact
 * unit vectors and p_from == p_to gives the exact identity.  Orders 1 .. 8. */
int l3k_interp_1d(int p_from, int p_to, double* out);

/* ---- kernel registry ------------------------------------------------------------------------------------------------
 * The reference takes the operator definition as a C++ callable wrapped by wrapDomainEquationKernel<params>
 * (common/KernelInterface.hpp:178-183) and instantiates the element loops on its type.  Here kernels are
 * __host__ __device__ functors with the same (in, out) signature (include/l3k/kernel_interface.hpp), registered in
 * l3ster_amd/csrc/user_kernels.hpp and instantiated into the HIP templates at build time; they are selected by id and
 * carry an optional POD parameter block. */
enum
{
    L3K_KERNEL_DIFFUSION3D     = 0, /* benchmarks/Diffusion3D.hpp:51-79; params {double k, s}                        */
    L3K_KERNEL_DIFFUSION3D_VAR = 1, /* tests/Kernels.hpp:84-118, n_fields = 1                                          */
    L3K_KERNEL_DIFFUSION2D     = 2, /* tests/Kernels.hpp:5-24: quads, E = 4, U = 3 (T, qx, qy), zero rhs              */
    L3K_KERNEL_DIFFUSION2D_VAR = 3, /* tests/Kernels.hpp:27-52: quads, n_fields = 1 (diffusivity, value + derivatives) */
    L3K_KERNEL_ADVDIFF3D       = 4, /* config-5 synthetic; params {double k, sigma, s}, n_fields = 3 */
    /* boundary equation kernels (wrapBoundaryEquationKernel: the input carries the outward normal); l3k_bnd_create */
    L3K_KERNEL_ADIABATIC2D     = 5, /* tests/Kernels.hpp:120-128: quads, U = 3 (T, qx, qy), E = 1, q.n = 0           */
    L3K_KERNEL_ADIABATIC3D     = 6, /* 3-D twin of tests/Kernels.hpp:120-128: q.n = 0                                 */
    L3K_KERNEL_ROBIN3D         = 7  /* synthetic: q.n + h T = h T_inf; params {double h, t_inf}                      */
};
/* residual kernels (wrapDomainResidualKernel / wrapBoundaryResidualKernel) for l3k_integrate */
enum
{
    L3K_RESIDUAL_DIFFUSION3D_ERROR = 0, /* benchmarks/Diffusion3D.hpp:81-103; fields (T,qx,qy,qz); params {double k, s} */
    L3K_RESIDUAL_LINEAR2D_ERROR    = 1, /* tests/Diffusion2D.hpp:84-92 (quads): fields (T,qx,qy), error against T = x   */
    L3K_RESIDUAL_LINEAR3D_ERROR    = 2, /* 3-D twin of tests/Diffusion2D.hpp:84-92: error against T = x, q = (1,0,0)   */
    L3K_RESIDUAL_UNIT2D            = 3, /* quads: integrand 1 (area, side length)                                     */
    L3K_RESIDUAL_UNIT3D            = 4, /* tests/MappingTests.cpp:567-569: integrand 1                                */
    L3K_RESIDUAL_COORDX2D          = 5, /* tests/Diffusion2D.hpp:49-50 (quads): out[0] = x (Dirichlet value kernel)     */
    L3K_RESIDUAL_COORDX3D          = 6  /* 3-D twin of tests/Diffusion2D.hpp:49-50: out[0] = x (Dirichlet value kernel) */
};
int l3k_kernel_info(int kernel_id, l3k_kparams* params, const char** name, size_t* param_bytes);
/* Kernels that are not compiled into libl3k.so: a kernel PLUGIN is a shared library built from the user's functor (the
 * reference compiles the user's lambda with the application; here `l3ster_amd.plugin.compile_kernel` / the Makefile
 * fragment in INTEGRATION.md run hipcc on a generated translation unit that instantiates the element kernels for the
 * functor and the requested (order, nq, ncols) shapes).  Loading it registers the kernel id and its instantiations;
 * ids >= 1000 are free for plugins. */
int l3k_plugin_load(const char* path);
/* number of (kernel, order, nq, ncols) device instantiations, and the i-th one: for "is this shape built?" queries */
int l3k_instance_count(void);
int l3k_instance_info(int i, int* kernel_id, int* order, int* nq, int* ncols);

/* ---- context ----------------------------------------------------------------------------------------------------- */
/* One ctx per GPU / per process.  hip_stream is a hipStream_t (NULL = default stream); torch users pass
 * torch.cuda.current_stream().cuda_stream. */
int l3k_ctx_create(int hip_device, void* hip_stream, l3k_ctx** out);
int l3k_ctx_set_stream(l3k_ctx* ctx, void* hip_stream);
/* Bitwise-reproducible mode (also: environment L3K_DETERMINISTIC=1 when the context is created).  The reference scatters
 * with relaxed atomics (algsys/MatrixFreeSystem.hpp:513), so its global results change in the last bits from run to run
 * and PCG iteration counts move with them; for parity runs this build can fix the order instead: meshes created while the
 * mode is on carry a colouring of their elements (no two elements of a colour share a node) and every domain-kernel
 * launch (apply, diag / rhs) goes colour by colour, so each row receives its contributions in a fixed order; <p, A p>
 * comes from the fixed-order dot product.  Boundary terms created while the mode is on colour their element sides the
 * same way and launch per colour behind the domain kernel.  Slower (one launch per colour). */
int l3k_ctx_set_deterministic(l3k_ctx* ctx, int on);
/* Which point a DOMAIN kernel sees in the matrix-free apply.  The reference is not consistent with itself here: its hex
 * sum-factorisation path builds SpaceTimePoint{Point<3>{x, y, 0.}, time} (algsys/SumFactorization.hpp:732, a copy of the 2-D
 * line :656), its local-element path -- assembleLocalSystem, evaluateLocalOperator, precomputeOperatorDiagonalAndRhs -- the
 * true point (algsys/AssembleLocalSystem.hpp:229-230).  Default (on = 0): the true point everywhere, i.e. apply, diag / rhs
 * and LocalAssembly describe ONE operator.  on = 1: applies launched from this context afterwards pass z = 0 like the
 * reference's evalAtHexQPs (bit-for-bit reference behaviour for a kernel that reads point.space.z() under
 * sum-factorisation); diag / rhs and LocalAssembly keep the true point, as in the reference.  Kernels that do not read z
 * are unaffected. */
int l3k_ctx_set_reference_z0(l3k_ctx* ctx, int on);
/* Launch-route settings of a context.  The defaults are what the measurements recorded in DESIGN.md chose; the fields exist so
 * that tests and tools can take the other route ON PURPOSE.  The environment is consulted once, in l3k_ctx_create
 * (L3K_GENERIC_BELOW, L3K_FAST_STATIC, L3K_FAST_WAVES_PER_CU, L3K_NO_AFFINE, L3K_COLUMN_BY_COLUMN, L3K_ASSEMBLE_DENSE,
 * L3K_ASM_TWO_LAUNCHES, L3K_SCATTER_PER_ENTRY, L3K_ASM_DIRECT_STORE, L3K_ASM_NO_SYMMETRISE initialise the fields below, L3K_DETERMINISTIC the deterministic mode): nothing on the
 * launch path reads the environment, and l3k_mf_route names the kernel a launch takes. */
typedef struct
{
    int64_t generic_below;         /* element launches of fewer elements take the generic LDS kernel (latency-bound sizes); 1500 */
    int     static_deal;           /* single-wave kernel: static deal of the element batches instead of the dynamic one; 0      */
    int     waves_per_cu;          /* single-wave kernel: persistent waves per CU, 0 = as many as LDS and registers admit; 0    */
    int     no_affine;             /* never take the affine variant (one Jacobian per element) on all-affine meshes; 0          */
    int     column_by_column;      /* multi-column applies as one launch per column (cross-check of the one-pass variant); 0    */
    int     assemble_dense;        /* LocalAssembly as the dense FP64-MFMA product instead of the sum-factorised kernels; 0     */
    int     assemble_two_launches; /* stored row-major LocalAssembly as two launches (diagonal / off-diagonal blocks); 0        */
    int     scatter_per_entry;     /* l3k_assembled_scatter: one wave per row with a search per entry (round-2 kernel); 0       */
    int     assemble_direct_store; /* stored row-major LocalAssembly written by the assembly kernel itself (8-byte stores at a
                                      32-byte stride, 3.9 x write traffic) instead of x-major tiled layout + mirroring
                                      transposition kernel; 0                                                                   */
    int     assemble_sub_batch;    /* stored row-major LocalAssembly: elements per pipelined sub-batch, 0 = chosen by size; 0      */
    int     assemble_no_symmetrise; /* stored row-major LocalAssembly through the plain tiled layout and the plain transposition
                                      (both triangles formed, each in its own summation order): K_e symmetric to rounding
                                      (1e-13) instead of bit for bit like the reference's -- the cross-check of the default; 0  */
} l3k_tuning;
int l3k_ctx_get_tuning(const l3k_ctx* ctx, l3k_tuning* out);
int l3k_ctx_set_tuning(l3k_ctx* ctx, const l3k_tuning* in);
int l3k_ctx_synchronize(l3k_ctx* ctx);
int l3k_ctx_destroy(l3k_ctx* ctx);

/* ---- device mesh --------------------------------------------------------------------------------------------------
 * What the reference keeps in LocalMeshView / LocalElementView (mesh/LocalMeshView.hpp:13-145), LocalDofMap
 * (dofs/NodeToDofMap.hpp:84-109) and LocalDirichletBC (bcs/LocalDirichletBC.hpp:13-32), flattened.  Uploaded once. */
typedef struct
{
    int             dim;            /* 3 (hex) or 2 (quad: apply, diag / rhs, boundary kernels, integrals and values
                                       at nodes; no LocalAssembly or assembled path on quads)                          */
    int             order;          /* p; nodes per element N = (p+1)^dim, lexicographic, xi fastest               */
    int64_t         n_elems;        /* elements [0, n_interior_elems) touch owned dofs only, the rest are "border" */
    int64_t         n_interior_elems; /* splitBorderAndInterior, algsys/MatrixFreeSystem.hpp:969-981              */
    const uint32_t* elem_nodes;     /* [n_elems][N] local node ids (n_loc_id_t, common/Typedefs.h:14)              */
    const double*   elem_verts;     /* [n_elems][2^dim][3], vertex v = i + 2j + 4k (mesh/primitives/CubeMesh.hpp);
                                       quads: [n_elems][4][3], v = i + 2j, z ignored                                   */
    int64_t         n_owned_nodes;  /* local node numbering: owned first, then ghosts (LocalMeshView.hpp:425-458)  */
    int64_t         n_ghost_nodes;
    int             dofs_per_node;  /* dof(node,k) = node*dofs_per_node + k (dofs/NodeToDofMap.hpp:250-264)        */
    const uint8_t*  dirichlet;      /* [(n_owned+n_ghost)*dofs_per_node] byte mask or NULL (isDirichletDof)       */
} l3k_mesh_desc;
int l3k_mesh_create(l3k_ctx* ctx, const l3k_mesh_desc* desc, l3k_mesh** out);
int l3k_mesh_destroy(l3k_mesh* mesh);

/* ---- matrix-free operator ------------------------------------------------------------------------------------------
 * Stands in for algsys::MatrixFreeSystem (assembleProblem + Operator::apply), algsys/MatrixFreeSystem.hpp:24-89.
 * field_inds[n_unknowns]: which per-node dof each unknown maps to (detail::getDofs, :298-311). */
int l3k_mf_create(l3k_ctx* ctx, l3k_mesh* mesh, int kernel_id, const void* kparam_blob, size_t kparam_bytes,
                  const l3k_asmopts* opts, const int* field_inds, int n_rhs, l3k_mf** out);
int l3k_mf_destroy(l3k_mf* mf);
/* external fields read by the kernel: SoA [n_fields][ld] over local nodes, value(node, f) = d_soa[node + f*ld]
 * (post::FieldAccess, post/FieldAccess.hpp:21-30).  The pointer is kept, not copied. */
int l3k_mf_set_fields(l3k_mf* mf, const double* d_soa, size_t ld);
int l3k_mf_set_time(l3k_mf* mf, double time);
/* Which kernel would l3k_mf_apply_elems(mf, which, ..., ncols, ...) launch for its elements right now?  Writes a one-line
 * description into buf (NUL-terminated, truncated to n bytes): kernel template and variant, lanes, LDS, waves per CU, grid --
 * decided by the same code as the launch itself.  For run-time reports (bench.py prints it) and for tests that assert a route.
 * with_energy != 0: as inside l3k_mf_apply_energy / between l3k_mf_energy_begin and _end. */
int l3k_mf_route(l3k_mf* mf, int which, int ncols, int with_energy, char* buf, size_t n);
/* The variant of the single-wave element kernel that the calling thread launched last (0: none yet).  l3k_mf_route is made
 * without the operands, so it cannot tell whether ghost rows directly behind the owned rows were recognised; this can.  Bits:
 * 1 launched, 2 split-ghost, 4 affine, 8 energy, 16 multi-column, 32 strided-dofs, 64 dynamic batches, 128 right-hand side. */
int l3k_last_fast_launch(unsigned* variant);

/* Y <- alpha*A*X + beta*Y.  Operator::apply / applyImpl, algsys/MatrixFreeSystem.hpp:34-41,1020-1140, for a rank
 * without ghosts (n_ghost_nodes == 0): scale (:1038), gather with Dirichlet -> 0 (:421-467), sum-factorised element
 * kernel (algsys/SumFactorization.hpp:882-917), scatter-add skipping Dirichlet dofs (:494-537), y[d] += alpha*x[d] on
 * owned Dirichlet rows (:1087-1098).  ncols <= n_rhs, else error (:1035-1037). */
/* Alignment: when the kernel's unknowns are all dofs of a node (the dense layout), x, y and the ghost buffers must be
 * 16-byte aligned and leading dimensions even when ncols > 1 (a node's dofs move with 16-byte accesses); align node rows
 * to 32 bytes for full speed. */
int l3k_mf_apply(l3k_mf* mf, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha,
                 double beta);

/* Split-phase form for ranks with ghosts (the pieces applyImpl interleaves with comm::Import/Export,
 * algsys/MatrixFreeSystem.hpp:1046-1111).  Ghost values live in separate [n_ghost_dofs][ncols] buffers exactly like
 * m_import_shared_buf / m_export_shared_buf (:1008-1009), accessed through BorderAccessor semantics
 * (algsys/ComputeValuesAtNodes.hpp:21-50): local dof < n_owned -> owned vector, else ghost buffer.
 *   which: 0 = interior elements, 1 = border elements, 2 = all; 3 / 4 = first / second half of the interior elements
 *   (the schedule import || first half, border, export || second half hides both exchanges; the reference overlaps
 *   only the import, :1046-1086). */
/* Y <- beta*Y (:1038) on the rows the element kernels ACCUMULATE into.  Rows of nodes that belong to exactly one element
 * (the element-internal nodes of the reference's numbering, mesh/LocalMeshView.hpp:425-458) are not touched here when
 * the operator covers all dofs of a node: l3k_mf_apply_elems WRITES alpha*A*x + beta*y there (no atomics, and for
 * beta = 0 no read), so it must be given the same beta.  Together the two calls equal the reference's scale + scatter. */
int l3k_mf_scale(l3k_mf* mf, double* d_y, size_t ldy, int ncols, double beta);
int l3k_mf_apply_elems(l3k_mf* mf, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg,
                       double* d_y, size_t ldy, double* d_yghost, size_t ldyg, int ncols, double alpha, double beta);
int l3k_mf_dirichlet_rows(l3k_mf* mf, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols,
                          double alpha);                                                        /* :1087-1098      */
/* comm::Import pack (owner side gathers owned rows through m_owned_inds, comm/ImportExport.hpp:356-372) and
 * comm::Export unpack-add (util::AtomicSumInto through m_owned_inds, :448-470), on DOF rows:
 *   pack:       d_dst[i + n*c]  = d_src[idx[i] + ld*c]
 *   unpack_add: d_dst[idx[i] + ld*c] += d_src[i + n*c]      (idx must not repeat within one call)                  */
int l3k_pack_rows(l3k_ctx* ctx, const double* d_src, size_t ld, int ncols, const int32_t* d_idx, int64_t n,
                  double* d_dst);
int l3k_unpack_add_rows(l3k_ctx* ctx, const double* d_src, int64_t n, const int32_t* d_idx, double* d_dst, size_t ld,
                        int ncols);

/* diag(A) and rhs with Dirichlet lifting: computeDiagAndRhs, algsys/MatrixFreeSystem.hpp:888-941 around
 * precomputeOperatorDiagonalAndRhs (algsys/EvaluateLocalOperator.hpp:172-208,276-301).  d_dirichlet_vals
 * [n_local_dofs][n_rhs] (ld) or NULL (= 0); outputs accumulate into owned rows d_diag[n_owned_dofs],
 * d_rhs[n_owned_dofs][n_rhs] and ghost rows d_diag_ghost / d_rhs_ghost (may be NULL when n_ghost_nodes == 0);
 * the caller zeroes them first (:921-923).  finalize != 0 sets diag = 1, rhs = g on owned Dirichlet rows (:911-915). */
int l3k_mf_diag_rhs(l3k_mf* mf, int which, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs,
                    size_t ldr, double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg, int finalize);
/* the finalisation alone (diag = 1, rhs = g on owned Dirichlet rows, :911-915): partitioned systems call l3k_mf_diag_rhs
 * with finalize = 0, export-add the ghost rows to their owners (:925-938), then this */
int l3k_mf_dirichlet_finalize(l3k_mf* mf, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr);

/* ---- boundary equation kernels on element sides ---------------------------------------------------------------------
 * assembleProblem(kernel, boundary_ids) with a BoundaryEquationKernel (algsys/MatrixFreeSystem.hpp:58-68): the term
 * sum over the listed element sides of  int_side B^T B  with the side quadrature, surface jacobian and outward normal
 * of map::mapBoundary (algsys/EvaluateLocalOperator.hpp:238-274,303-330; mapping/BoundaryNormal.hpp:8-64;
 * mapping/BoundaryIntegralJacobian.hpp:9-29; basisfun/ReferenceElementBasisAtQuadrature.hpp:57-97).
 * A side is (element index in the mesh, side): hex sides 0..5 = z-, z+, y-, y+, x-, x+ (mesh/ElementTraits.hpp:84-95);
 * quad sides 0..3 = y- (eta = -1), y+ (eta = +1), x- (xi = -1), x+ (xi = +1).  A side index >= 2 * dim is refused.
 * l3k_bnd_create, l3k_integrate and l3k_values_at_nodes take hex and quad meshes, with kernels of the mesh's dimension.
 * l3k_mf_attach_boundary registers the term with a system: l3k_mf_apply / l3k_mf_apply_elems / l3k_mf_diag_rhs then
 * include it, like the reference evaluates every kernel passed to assembleProblem.  `which` as in l3k_mf_apply_elems:
 * sides of interior elements (0), of border elements (1), all (2).  The term does not own the system or the mesh and
 * must outlive the systems it is attached to.  The assembled and condensed entry points (l3k_local_assemble,
 * l3k_assemble_global, l3k_condense_local, l3k_condense_global, l3k_condensed_recover) include the attached terms only after
 * l3k_mf_assemble_boundary(mf, 1), below. */
typedef struct l3k_bnd l3k_bnd;
int l3k_bnd_create(l3k_ctx* ctx, l3k_mesh* mesh, int kernel_id, const void* kparam_blob, size_t kparam_bytes,
                   const l3k_asmopts* opts, const int* field_inds, int n_rhs, int64_t n_faces, const int64_t* face_elem,
                   const uint8_t* face_side, l3k_bnd** out);
int l3k_bnd_destroy(l3k_bnd* bnd);
int l3k_bnd_set_fields(l3k_bnd* bnd, const double* d_soa, size_t ld);
int l3k_bnd_set_time(l3k_bnd* bnd, double time);
/* y += alpha * A_b x  (Dirichlet columns read as 0, Dirichlet rows skipped: same semantics as the element kernels) */
int l3k_bnd_apply(l3k_bnd* bnd, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y,
                  size_t ldy, double* d_yghost, size_t ldyg, int ncols, double alpha);
/* diag += diag(A_b) (d_diag may be NULL), rhs += B_b^T W (f_b - B_b g) */
int l3k_bnd_diag_rhs(l3k_bnd* bnd, int which, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs,
                     size_t ldr, double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg);
int l3k_mf_attach_boundary(l3k_mf* mf, l3k_bnd* bnd);
/* ---- ... in the assembled and condensed paths (hexes; quads are refused) ------------------------------------------------
 * assembleLocalSystem on a BoundaryElementView (algsys/AssembleLocalSystem.hpp:77-216): the local system of the WHOLE element
 * from the side quadrature, K_s = sum_q w jac B_q^T B_q, F_s = sum_q w jac B_q^T f_q, for the sides [first, first + count) of the
 * term's list in the order l3k_bnd_create was given.  Layouts of l3k_local_assemble: d_K [count][Nd][Nd] row-major, d_F
 * [count][n_rhs][Nd], Nd = (p+1)^3 * n_unknowns; either may be NULL; no Dirichlet lifting, no mask.  Every entry is written
 * (zeros included); K_s is bitwise symmetric and bitwise reproducible. */
int l3k_bnd_local_assemble(l3k_bnd* bnd, int64_t first, int64_t count, double* d_K, double* d_F);
/* The boundary overload of assembleGlobalSystem (algsys/AssembleGlobalSystem.hpp:55-96) for the sides [first, first + count) of one
 * term: side systems formed in sub-batches (the library's own workspace, workspace_bytes in total, 0 = 1 GiB) and summed into
 * d_values / d_rhs over the rows node * dofs_per_node + field_inds[u] of the term.  Graph, ldr, skip_dirichlet and n_missing as
 * for l3k_assemble_global.  Additive: after l3k_assemble_global on the same arrays the result is A_domain + A_boundary. */
int l3k_bnd_assemble_global(l3k_bnd* bnd, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind,
                            double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes,
                            int64_t* n_missing);
/* on != 0: from now on l3k_local_assemble, l3k_assemble_global, l3k_condense_local, l3k_condense_global and
 * l3k_condensed_recover work on K_e + sum K_s, F_e + sum F_s over the attached sides of each element, as the reference's assembled
 * path does with CondensationPolicy::ElementBoundary (StaticCondensationManager.hpp:354-407: the side matrix joins the element's
 * blocks before the internal dofs are eliminated).  The sides of an element are added in a fixed order (terms in attachment
 * order, a term's sides in list order): results stay bitwise symmetric and reproducible.  Refused (-1) while it is on: a term
 * whose n_unknowns, field_inds or n_rhs differ from the system's or whose shape has no assembly launcher, l3k_local_assemble
 * with a checksum, and l3k_local_assemble_tiled.  Default 0: every call does exactly what it did without this switch. */
int l3k_mf_assemble_boundary(l3k_mf* mf, int on);

/* ---- integrals of residual kernels (post-processing) -----------------------------------------------------------------
 * evalLocalIntegral, post/Integral.hpp:54-111: h_out[n_equations] (HOST) = sum over all elements (n_faces < 0) or over
 * the listed element sides of the integral of the residual kernel evaluated on the fields d_fields (SoA [F][ld], local
 * node index); square != 0 integrates the squared components.  computeNormL2 (post/NormL2.hpp:31-62) is
 * sqrt(all-reduce(l3k_integrate(opts with value_order and derivative_order doubled, square = 1))).  The quadrature
 * size follows from opts as for the operator kernels.  Results are bitwise reproducible (fixed summation order). */
int l3k_residual_info(int residual_id, l3k_kparams* params, const char** name, size_t* param_bytes);
int l3k_integrate(l3k_ctx* ctx, l3k_mesh* mesh, int residual_id, const void* kparam_blob, size_t kparam_bytes,
                  const l3k_asmopts* opts, const double* d_fields, size_t ldf, double time, int square, int64_t n_faces,
                  const int64_t* face_elem, const uint8_t* face_side, double* h_out);

/* ---- values of residual kernels at the nodes (Dirichlet values, initial conditions) ---------------------------------------
 * computeValuesAtNodes (algsys/ComputeValuesAtNodes.hpp:371-448 domain, :508-594 boundary), the engine behind
 * setDirichletBCValues / setValues: the kernel is evaluated at the nodes of the listed element sides (n_faces >= 0) or of
 * every element (n_faces < 0) with the nodal field values, their physical derivatives, the point and (sides) the outward
 * normal; equation e is ADDED to d_sum[node * dofs_per_node + dof_inds[e]] and 1 to d_count[...] (both over all local
 * dofs, owned then ghost; the caller zeroes them, and in a partitioned run exports the ghost rows of both to their owners
 * before averaging).  l3k_average_values: values[i] = sum[i] / count[i] where count[i] > 0, other entries untouched
 * (averageElementContributions :112-154). */
int l3k_values_at_nodes(l3k_ctx* ctx, l3k_mesh* mesh, int residual_id, const void* kparam_blob, size_t kparam_bytes,
                        const double* d_fields, size_t ldf, double time, int64_t n_faces, const int64_t* face_elem,
                        const uint8_t* face_side, const int* dof_inds, double* d_sum, double* d_count);
int l3k_average_values(l3k_ctx* ctx, const double* d_sum, const double* d_count, int64_t n, double* d_values);
/* MatrixFreeSystem::updateSolution(sol_inds, sol_man, sol_man_inds) (algsys/MatrixFreeSystem.hpp:1231-1273; AlgebraicSystem's
 * twin): the solution's per-node dofs sol_inds[i] of column r copied into field sol_man_inds[i * ncols + r] of the SoA field
 * storage a kernel's FieldAccess reads (value(node, f) = d_fields[node + f * ldf], the layout of l3k_mf_set_fields), for EVERY
 * local node: owned rows from d_x, ghost rows from d_xghost -- the values the reference imports inside updateSolution; a
 * partitioned host calls l3k_halo_import first (NULL on a rank without ghosts).  Index lists are host arrays.  Errors as the
 * reference's asserts: "Source index out of bounds" (>= dofs_per_node), "Destination index out of bounds" (>= n_fields). */
int l3k_update_solution(l3k_ctx* ctx, l3k_mesh* mesh, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, int ncols,
                        int n_inds, const int* sol_inds, const int* sol_man_inds, double* d_fields, size_t ldf, int n_fields);

/* ---- Jacobi-preconditioned conjugate gradients ------------------------------------------------------------------------
 * The reference hands the iteration to Trilinos Belos ("Block CG", solve/BelosSolvers.hpp:116-122) with its native Jacobi
 * preconditioner (solve/NativePreconditioners.hpp:36-96); Belos is not part of the reference tree, the arithmetic here
 * is the textbook Hestenes-Stiefel PCG for one column, pinned end to end.  Everything stays on the
 * context's stream; dot products are two-stage reductions in a fixed order.
 *   l3k_jacobi_inverse : minv = sign(d) * damping / max(|d|, threshold)          (NativeJacobiImpl::init :75-96)
 *   l3k_pcg_solve      : single rank (no ghost nodes); x holds the initial guess and the result; d_minv may be NULL;
 *                        residual_scaling 0 none / 1 initial residual / 2 norm of b (IterSolverOpts,
 *                        solve/SolverInterface.hpp:26-37); check_every = iterations between convergence checks (each is
 *                        one 32-byte device-to-host copy).  opts == NULL: {1e-6, 10000, 0, 1}.
 *                        Rows with minv == 0 (a preconditioner zeroed on constrained dofs; damping 0) are frozen: x keeps
 *                        its initial value there and the row is left out of the residual norm (the iteration keeps
 *                        z = M^-1 r, from which r cannot be recovered where minv = 0)
 *   l3k_cg_*           : the fused vector kernels of one iteration for partitioned vectors; the caller all-reduces the
 *                        device scalar block s[8] (0 <r,z>, 1 <p,Ap>, 2 <r,z> new, 3 <r,r>) between them.  Protocol below
 *                        (l3k_cg_init, _dot_pap, _update_z, _update_px): init and update_z write LOCAL sums into s[2], s[3];
 *                        all-reduce them before the next call.  init also stores its LOCAL s[2] in s[0] (all a single rank
 *                        needs); a host that reduces across ranks copies s[2] to s[0] again once the reduced value is in
 *                        place.  Slots written: init 0, 2, 3; dot_pap 1; update_z 2, 3; update_px 0.  No call writes any
 *                        other slot: 4..7 are the caller's. */
typedef struct
{
    double tol;
    int    max_iters;
    int    residual_scaling;
    int    check_every;
} l3k_cg_opts;
typedef struct
{
    double achieved_tol;
    int    iterations;
    int    converged;
} l3k_cg_result;
int l3k_jacobi_inverse(l3k_ctx* ctx, const double* d_diag, int64_t n, double damping, double threshold, double* d_minv);
int l3k_pcg_solve(l3k_mf* mf, const double* d_b, double* d_x, const double* d_minv, const l3k_cg_opts* opts,
                  l3k_cg_result* result);
/* ... for the ncols columns of a multivector (column c at + c * ld), one after the other as Belos "Block CG" with block size 1
 * does for the reference's n_rhs right-hand sides; results[ncols] */
int l3k_pcg_solve_cols(l3k_mf* mf, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                       const l3k_cg_opts* opts, l3k_cg_result* results);
/* The pieces of the iteration for hosts that reduce the scalars across ranks themselves (d_s: device block, 0 <r,z> old, 1 <p,Ap>,
 * 2 <r,z> new, 3 <r,r>).  The iteration keeps the preconditioned residual z = M^-1 r instead of r (9 instead of 11 vector passes):
 *   l3k_cg_init:      d_z holds A x0 on entry; z = minv (b - A x0), p = z, s[2] = <r,z>, s[3] = <r,r> (this rank's share),
 *                     s[0] <- s[2] (this rank's share as well: all-reduce s[2], s[3], then copy s[2] to s[0])
 *   l3k_cg_dot_pap:   s[1] = <p, Ap> (this rank's share)
 *   l3k_cg_update_z:  alpha = s[0]/s[1]; z -= alpha minv Ap; s[2], s[3] as above (r = z / minv)
 *   l3k_cg_update_px: x += alpha p; beta = s[2]/s[0]; p = z + beta p; then s[0] <- s[2]
 * d_minv may be NULL (no preconditioner: z = r). */
int l3k_cg_init(l3k_ctx* ctx, double* d_z, const double* d_b, double* d_p, const double* d_minv, int64_t n, double* d_s);
int l3k_cg_dot_pap(l3k_ctx* ctx, const double* d_p, const double* d_ap, int64_t n, double* d_s);
/* One rank, one column: y <- A x and s[1] <- <x, A x> in one pass (what the PCG needs of an apply followed by
 * l3k_cg_dot_pap).  On the single-wave route of domain kernels the element kernel accumulates x^T A x = sum_q w detJ |B_q x|^2
 * at the quadrature points (the Dirichlet rows, identity rows of the operator, add x_d^2): no pass over x and y afterwards.
 * Otherwise (small meshes, attached boundary terms, other dof layouts) it is the apply followed by the dot product.     */
int l3k_mf_apply_energy(l3k_mf* mf, const double* d_x, double* d_y, double* d_s);
/* The same for the split-phase (partitioned) apply: l3k_mf_energy_begin zeroes s[1] and arms the accumulation for the
 * l3k_mf_apply_elems calls that follow; l3k_mf_energy_end adds the owned Dirichlet rows' share, disarms, and reports in
 * *fused whether every element launch in between accumulated (if not, s[1] is incomplete: take l3k_cg_dot_pap instead).
 * s[1] then holds this rank's share of <x, A x>; the all-reduce over the ranks is the caller's, as for the other scalars. */
int l3k_mf_energy_begin(l3k_mf* mf, double* d_s);
int l3k_mf_energy_end(l3k_mf* mf, const double* d_x, int* fused);
int l3k_cg_update_z(l3k_ctx* ctx, double* d_z, const double* d_ap, const double* d_minv, int64_t n, double* d_s);
int l3k_cg_update_px(l3k_ctx* ctx, double* d_p, double* d_x, const double* d_z, int64_t n, double* d_s);

/* ---- Chebyshev-Jacobi preconditioner, matrix-free -------------------------------------------------------------------
 * Ifpack2ChebyshevPreconditioner (solve/Ifpack2Preconditioners.hpp:26-36,107-131: degree, cond_est, max_power_iters,
 * boost_factor; its diag_threshold is the threshold of l3k_jacobi_inverse).  The reference builds it from an assembled CRS
 * matrix; its arithmetic needs y <- A x and diag(A) only, so here it sits on the matrix-free apply.  Ifpack2 is not part of
 * the reference tree: the arithmetic is the textbook Chebyshev iteration with Jacobi scaling.  With
 *     theta = (lambda_max + lambda_min) / 2, delta = (lambda_max - lambda_min) / 2, sigma = theta / delta, rho_0 = 1 / sigma,
 * z <- p(D^-1 A) D^-1 r is
 *     w = D^-1 r / theta, z = w
 *     k = 1 .. degree - 1:  rho' = 1 / (2 sigma - rho);  w = rho' rho w + (2 rho' / delta) D^-1 (r - A z);  z += w;  rho = rho'
 * (degree 1 is Jacobi scaled by 1 / theta; degree d costs d - 1 applies).  The coefficients are computed on the host once, in
 * l3k_cheb_create.  Rows with minv == 0 are frozen as in l3k_pcg_solve: w = z = 0 is stored there (not 0 * something: a
 * non-finite A z cannot reach them), they are zero in the power-iteration vectors and left out of <r, r>; x keeps its value.
 *
 * lambda_max: opts->lambda_max if > 0 (Ifpack2's "chebyshev: max eigenvalue"; no power iteration, no boost), else boost_factor
 * times the estimate of max_power_iters (>= 1) steps of the power method on D^-1 A, run inside l3k_cheb_create:
 *     start   v_i = h(i) * 2^-31 - 1 in [-1, 1) on rows with minv != 0, else 0, where for the row index i
 *             h = (uint32) i;  h ^= h >> 16;  h *= 0x7feb352d;  h ^= h >> 15;  h *= 0x846ca68b;  h ^= h >> 16   (mod 2^32)
 *             x = v * (1 / sqrt(<v, v>))
 *     step    y = D^-1 (A x);  lambda = <x, y>;  x = y * (1 / sqrt(<y, y>))     (the estimate is the lambda of the last step)
 * The dot products are the fixed-order two-stage reductions of the PCG: two creations give the same estimate bit for bit (on a
 * context in deterministic mode, where the apply is reproducible too).  The estimate is read back once, at the end of creation;
 * an estimate that is not finite and positive is an error (the operator or the diagonal is unusable).  lambda_min =
 * lambda_max / cond_est.
 *
 * l3k_cheb_create: d_minv (required) is the output of l3k_jacobi_inverse; the object keeps the pointer, the caller keeps the array
 * (and mf) alive.  opts == NULL: {1, 30., 10, 1.1, 0.}.  Single-rank systems only, like l3k_pcg_solve.  Errors (-1): null
 * arguments, degree < 1, cond_est <= 1, boost_factor < 1, max_power_iters < 1 without lambda_max, a mesh with ghost nodes, an
 * unusable estimate.
 * l3k_pcg_solve_cheb: Hestenes-Stiefel PCG that keeps r itself (M^-1 is not diagonal: r cannot be recovered from z); options,
 * residual scalings, check_every and the result as l3k_pcg_solve; <p, Ap> from l3k_mf_apply_energy; one allocation per solve
 * (r, z, p, Ap, w, s[8]).  An iteration is 1 + (degree - 1) applies and 14 + 7 (degree - 1) vector passes (reads + writes of a
 * vector): cgUpdateRXKernel 7 (x, r, p, Ap, minv in; x, r out), chebFirstKernel 4 (r, minv in; w, z out), every chebStepKernel 7
 * (r, Az, minv, w, z in; w, z out), cgUpdatePKernel 3 (z, p in; p out) -- against the 9 of an iteration of l3k_pcg_solve.     */
typedef struct l3k_cheb l3k_cheb;
typedef struct
{
    int    degree;          /* >= 1; degree d costs d - 1 applies per application              */
    double cond_est;        /* lambda_min = lambda_max / cond_est            (default 30)      */
    int    max_power_iters; /* power iterations on D^-1 A for lambda_max     (default 10)      */
    double boost_factor;    /* lambda_max = boost_factor * estimate          (default 1.1)     */
    double lambda_max;      /* > 0: take this value, run no power iteration                    */
} l3k_cheb_opts;
typedef struct
{
    double lambda_max, lambda_min, lambda_est; /* lambda_est: the power method's estimate (= lambda_max where that was given) */
    int    degree, power_iters, applies_per_call;
} l3k_cheb_info;
int l3k_cheb_create(l3k_mf* mf, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out);
int l3k_cheb_info_get(const l3k_cheb* c, l3k_cheb_info* out);
/* z <- p(D^-1 A) D^-1 r.  r and z must not overlap (z is written before r is read for the last time); z is a vector of
 * l3k_mf_apply and is aligned as that call asks (it refuses a misaligned one), r is read 8 bytes at a time. */
int l3k_cheb_apply(l3k_cheb* c, const double* d_r, double* d_z);
int l3k_cheb_destroy(l3k_cheb* c);
int l3k_pcg_solve_cheb(l3k_mf* mf, const double* d_b, double* d_x, l3k_cheb* c, const l3k_cg_opts* opts, l3k_cg_result* result);
/* The pieces for hosts that iterate partitioned vectors themselves (explicit coefficients; the applies in between and the
 * all-reduces of the scalar block s[8], slots as above, are the caller's; d_minv may be NULL = no frozen rows, 1 in the products):
 *   l3k_cheb_first:   w = z = c0 minv r                                  (c0 = 1 / theta)
 *   l3k_cheb_step:    w = a w + b minv (r - Az); z += w                  (a = rho' rho, b = 2 rho' / delta; d_az holds A z)
 *                     both: d_s != NULL: s[2] = <r, z> (this rank's share) -- pass it on the last step of an application,
 *                     NULL on the others
 *   l3k_cg_update_rx: alpha = s[0]/s[1]; x += alpha p; r -= alpha Ap (frozen rows: r = 0, x untouched); s[3] = <r, r>
 *   l3k_cg_update_p:  beta = s[2]/s[0]; p = z + beta p; then s[0] <- s[2]
 * Slots written: cheb_first and cheb_step 2 (none with d_s == NULL); update_rx 3; update_p 0.  No call writes any other slot. */
int l3k_cheb_first(l3k_ctx* ctx, const double* d_r, const double* d_minv, double c0, double* d_w, double* d_z, int64_t n, double* d_s);
int l3k_cheb_step(l3k_ctx* ctx, const double* d_r, const double* d_az, const double* d_minv, double a, double b, double* d_w,
                  double* d_z, int64_t n, double* d_s);
int l3k_cg_update_rx(l3k_ctx* ctx, double* d_x, double* d_r, const double* d_p, const double* d_ap, const double* d_minv, int64_t n,
                     double* d_s);
int l3k_cg_update_p(l3k_ctx* ctx, double* d_p, const double* d_z, int64_t n, double* d_s);

/* ---- p-multigrid preconditioner, matrix-free -----------------------------------------------------------------------------
 * The same elements rediscretised at strictly decreasing orders p_0 > p_1 > ... (level 0 = finest), the Chebyshev-Jacobi
 * polynomial of l3k_cheb_create as the smoother of every level (Ifpack2ChebyshevPreconditioner, solve/Ifpack2Preconditioners.hpp:
 * 26-36,107-131, stands next to it) and the tensor-product interpolation between the GLL node sets (l3k_interp_1d) as the
 * transfer.  The reference has no multigrid of its own (it hands an assembled matrix to Ifpack2): like the matrix-free Chebyshev
 * this exists because a matrix-free path has no matrix to hand to someone else's preconditioner.  Single rank.
 *
 * A level pair is a fine and a coarse mesh with the same elements: the same dim, n_elems, dofs_per_node and -- element by element --
 * bitwise equal elem_verts; their own order, elem_nodes, node count and Dirichlet mask.  d_elem_map[e_fine] = e_coarse (device,
 * kept by the object, the caller keeps it alive) pairs the elements, NULL = the same index.  Creation validates every pair on the
 * device with one readback per pair (element map in range and a permutation, equal vertices) and refuses with -1 and a message
 * naming the first offending fine element, so that no later call can transfer between two different elements.
 *
 * Ownership: owner[fine node] = the lowest fine element index that contains it (an integer atomicMin at creation).  The global
 * prolongation P has one row per fine dof: the values of the coarse basis functions of the OWNING element at the node; all
 * dofs_per_node components of a node move alike.  Rows of fine Dirichlet dofs and columns of coarse Dirichlet dofs are zero.
 *   l3k_pmg_prolong:  x_f <- P x_c (add = 0) or x_f += P x_c (add != 0); coarse Dirichlet dofs are read as 0 (not loaded), fine
 *                     Dirichlet dofs are written as 0 (add: left alone).  One writer per dof, plain stores, no floating-point
 *                     atomics: bitwise reproducible on any context.
 *   l3k_pmg_restrict: r_c <- P^T r_f, the exact transpose; r_c is zeroed by the call, fine Dirichlet dofs and the nodes an element
 *                     does not own are not loaded, coarse Dirichlet dofs stay 0.  Accumulates with double atomics; on a context
 *                     in deterministic mode (hierarchy and meshes created with the mode on) it launches colour by colour on the
 *                     coarse mesh's colouring and is bitwise reproducible.
 * coarse_level in [1, n_levels) names the pair (coarse_level - 1, coarse_level); vectors are the owned dofs of their level.
 *
 * l3k_pmg_apply: z <- M^-1 r, one symmetric V-cycle.  With S_l the level's smoother (z = S r is l3k_cheb_apply: zero initial guess):
 *     cycle(l, r): z = S_l r;  last level: return z
 *                  d = r - A_l z;  r_{l+1} = P^T d;  z += P cycle(l + 1, r_{l+1});  d = r - A_l z;  z += S_l d
 * (the post-smoothing is the same polynomial, so M^-1 is symmetric).  On the last level the smoother is the coarse solve: a fixed
 * polynomial, e.g. of a higher degree and cond_est.  Rows frozen by a level's smoother (minv == 0) behave as in
 * l3k_pcg_solve_cheb: z = 0 there -- d is stored as 0 on them and the prolongation leaves them alone.  Dirichlet rows are identity
 * rows of every A_l with diag = 1; the transfers do not touch them, so there M^-1 is the smoother's polynomial alone (pre- and
 * post-smoothing of the row's own residual).  All vectors of all levels are allocated at creation.  Cost of a cycle on a level
 * that is not the last: 2 (degree - 1) + 2 applies, the smoother's passes twice, and 4 + 4 + 3 vector passes of its own (d = r - Az
 * with the mask twice, z += e once); on the last level degree - 1 applies.
 *
 * l3k_pcg_solve_pmg: the loop of l3k_pcg_solve_cheb with this cycle as the preconditioner (mf must be level 0's operator); options,
 * result, frozen rows (level 0's smoother's minv), check_every and max_iters as there.  <r, z> takes a pass of its own behind the
 * cycle (2 reads).
 *
 * Errors (-1): null arguments, n_levels outside 2 .. 8, levels on different contexts, a level with ghost nodes, a smoother created
 * for another system than its level's mf, orders not strictly decreasing, a failed pair validation, r and z overlapping, a level
 * index out of range, l3k_pcg_solve_pmg with an mf that is not level 0's. */
typedef struct l3k_pmg l3k_pmg;
typedef struct
{
    l3k_mf*        mf;         /* the operator of this level (level 0 = finest)                                              */
    l3k_cheb*      smoother;   /* created by the caller on mf with l3k_cheb_create: degree, cond_est, lambda_max per level   */
    const int64_t* d_elem_map; /* element of this level for each element of level - 1; NULL = identity; ignored on level 0   */
} l3k_pmg_level;
typedef struct
{
    int     n_levels;
    int     order[8];             /* per level                                     */
    int64_t n_dofs[8];
    int     applies_per_cycle[8]; /* applies of A_l in one l3k_pmg_apply           */
} l3k_pmg_info;
int l3k_pmg_create(l3k_ctx* ctx, int n_levels, const l3k_pmg_level* levels, l3k_pmg** out);
int l3k_pmg_info_get(const l3k_pmg* M, l3k_pmg_info* out);
int l3k_pmg_prolong(l3k_pmg* M, int coarse_level, const double* d_xc, double* d_xf, int add);
int l3k_pmg_restrict(l3k_pmg* M, int coarse_level, const double* d_rf, double* d_rc);
int l3k_pmg_apply(l3k_pmg* M, const double* d_r, double* d_z); /* r and z must not overlap */
int l3k_pmg_destroy(l3k_pmg* M);
int l3k_pcg_solve_pmg(l3k_mf* mf, const double* d_b, double* d_x, l3k_pmg* M, const l3k_cg_opts* opts, l3k_cg_result* result);

/* ---- p-multigrid on partitioned meshes: the transfer of one level pair, ghost rows included -------------------------------
 * l3k_pmg_* above serves single-rank systems.  A partitioned host keeps its hierarchy itself, as it keeps the Chebyshev iteration
 * (l3k_cheb_first / _step above): the smoothers are those pieces around l3k_mf_apply_dist, the exchanges are l3k_halo_import /
 * _export_add, and what is left -- the transfer between two orders of this rank's elements and the masked residual -- is here.
 *
 * l3k_transfer_create stands beside the pair set-up of l3k_pmg_create and validates the pair as it does (same dim, element count
 * and dofs_per_node, coarse order below the fine one, element map in range and a permutation, bitwise equal elem_verts; the same
 * message texts, with this call's name).  The meshes may have ghost nodes; both must live on ctx, and d_elem_map (device, NULL =
 * identity) and the meshes are kept, not copied: the caller keeps them alive.
 *
 * A vector of a level is two buffers, owned rows [n_owned_dofs] and ghost rows [n_ghost_dofs]; local dof < n_owned_dofs selects
 * the buffer, as in l3k_mf_apply_elems.  Ownership: a fine node is handled by the rank that owns it, there by the lowest local fine
 * element that contains it; ghost fine nodes have no handler on this rank.  The owned fine nodes of all ranks are the global fine
 * nodes once each, so the ranks' rows together are one P with one row per global fine dof -- the P of l3k_pmg_prolong on the
 * whole mesh up to the order of the sums (the interpolated value at a shared node does not depend on the element that computes
 * it: the end rows of l3k_interp_1d are unit vectors).  Creation counts the owned fine nodes that no local element contains
 * (one more word in the validation's readback) and refuses if there are any.
 *   l3k_transfer_prolong:  (beside l3k_pmg_prolong) x_f <- P x_c (add = 0) or x_f += P x_c; reads coarse owned rows d_xc and coarse
 *                          ghost rows d_xc_ghost -- the caller has run l3k_halo_import of d_xc on the coarse level -- and writes
 *                          OWNED fine rows only, one writer per dof, plain stores.  Fine ghost rows do not exist here: the next
 *                          apply imports them itself.  d_frozen (NULL: none): owned fine rows with d_frozen[row] == 0, tested on
 *                          the bits, are left alone (the smoother's minv).  Dirichlet dofs as in l3k_pmg_prolong.
 *   l3k_transfer_restrict: (beside l3k_pmg_restrict) r_c <- P^T r_f; reads OWNED fine rows only (no exchange on the fine level),
 *                          zeroes d_rc and d_rc_ghost and accumulates into both; the caller then runs l3k_halo_export_add of
 *                          d_rc_ghost into d_rc on the coarse level.  Deterministic mode as in l3k_pmg_restrict (colour by colour
 *                          on the coarse mesh's colouring); reproducibility ACROSS ranks is not claimed -- it depends on the add
 *                          order of the halo.
 * On meshes without ghost nodes the ghost pointers may be NULL and the prolongation equals l3k_pmg_prolong bit for bit.  A rank
 * with no elements creates the object and its calls return 0 (pointers to vectors of length 0 may be NULL).
 *
 * l3k_pmg_residual: d = r - az on the rows with minv != 0 (tested on the bits), 0 on the others: the masked residual of the cycle
 * of l3k_pmg_apply (az holds A z) for hosts that run the cycle themselves; n rows, all four arrays required.
 *
 * Errors (-1, the message names the call): null arguments (owned pointers of a non-empty vector included), meshes on another
 * context, a failed pair validation, owned fine nodes without a local element, NULL ghost pointers on a coarse mesh with ghosts. */
typedef struct l3k_transfer l3k_transfer;
typedef struct
{
    int     order_fine, order_coarse;
    int64_t n_owned_dofs_fine, n_ghost_dofs_fine, n_owned_dofs_coarse, n_ghost_dofs_coarse;
} l3k_transfer_info;
int l3k_transfer_create(l3k_ctx* ctx, l3k_mesh* mesh_fine, l3k_mesh* mesh_coarse, const int64_t* d_elem_map, l3k_transfer** out);
int l3k_transfer_info_get(const l3k_transfer* T, l3k_transfer_info* out);
int l3k_transfer_prolong(l3k_transfer* T, const double* d_xc, const double* d_xc_ghost, double* d_xf, int add, const double* d_frozen);
int l3k_transfer_restrict(l3k_transfer* T, const double* d_rf, double* d_rc, double* d_rc_ghost);
int l3k_transfer_destroy(l3k_transfer* T);
int l3k_pmg_residual(l3k_ctx* ctx, double* d_d, const double* d_r, const double* d_az, const double* d_minv, int64_t n);

/* ---- device CSR operator: the assembled and the condensed system in front of the solver -----------------------------------
 * A square CSR matrix in the format l3k_assembled_scatter, l3k_assemble_global and l3k_condense_global fill: d_row_ptr int64
 * [n + 1], d_col_ind int32 strictly ascending within a row, d_values double; single rank, rows and columns in the local dofs.
 * The object keeps the three pointers and copies nothing: the caller keeps the arrays alive and may rewrite d_values between
 * calls (a time loop assembles again), but not the graph.
 *
 * Nothing here accumulates atomically in floating point (one writer per row, a fixed butterfly over the lanes of a row, the
 * two-stage reduction of the PCG for <x, A x>): applies, and the solves below, are bitwise reproducible on ANY context, in
 * deterministic mode or not.
 *
 * l3k_csr_create: one validation pass on the device with a single readback (synchronises the context's stream).  Refused with
 *   -1 and a message naming the first offence: row_ptr[0] != 0, a decreasing row_ptr, a column outside [0, n), columns not
 *   strictly ascending within a row -- no later call can gather out of bounds.  The columns are only read once row_ptr has
 *   passed.  lanes_per_row: the lanes of a wave64 that share a row, 4, 16 or 64; 0 = chosen from the mean length of the
 *   non-empty rows (<= 8: 4, <= 64: 16, else 64).  Also -1: any other lanes_per_row, n < 0, n >= 2^31.
 * l3k_csr_info_get: the statistics the validation pass gathered.
 * l3k_csr_apply: y <- alpha A x + beta y for ncols columns (column c at + c * ld), tpetra_crsmatrix_t::apply as Belos calls it
 *   under solve/BelosSolvers.hpp:116-122.  beta == 0: y is not read (a NaN in it does not survive); an empty row gives beta y.
 *   Up to four columns share one pass over the matrix.  x and y must not overlap.
 * l3k_csr_apply_energy: y <- A x and s[1] <- <x, A x> for one column in one pass (what l3k_mf_apply_energy is to the
 *   matrix-free operator); no other slot of the scalar block s[8] is written.
 * l3k_csr_diag: d_diag[i] = a_ii, 0 where the row stores none (getLocalDiagCopy, solve/NativePreconditioners.hpp:76);
 *   d_minv[i] = sign(a_ii) damping / max(|a_ii|, threshold), the formula of l3k_jacobi_inverse, on every non-empty row and 0 on
 *   an EMPTY row, so that the frozen-row rule of l3k_pcg_solve carries the internal dofs of a condensed graph and any skipped
 *   rows: x keeps its value there.  Either output may be NULL.
 * l3k_csr_dirichlet: DirichletBCAlgebraic::apply (bcs/DirichletBC.hpp:82-150) in place.  d_mask [n] flags the Dirichlet dofs,
 *   d_bc_vals [ncols][ldg] holds the prescribed values, d_rhs [ncols][ldr] the right-hand sides.  A flagged row becomes the
 *   identity row and its rhs the prescribed value; in every other row each entry in a flagged column j gives rhs_i -= a_ij g_j
 *   (summed in a fixed order, one writer per row) and is set to 0.  A flagged row without a stored diagonal entry is refused
 *   (-1, nothing written; the reference dereferences end() there): one readback, the call synchronises.  d_values is the
 *   operator's own values array, passed again because this is the one call that writes the matrix.
 *
 * The solver on a CSR operator -- the loops are those of l3k_pcg_solve, l3k_cheb_create, l3k_cheb_apply and l3k_pcg_solve_cheb,
 * run with l3k_csr_apply / l3k_csr_apply_energy in place of the matrix-free applies; options, results, frozen rows and vector
 * passes as documented there; vectors have n entries:
 * l3k_csr_pcg_solve, l3k_csr_pcg_solve_cols: Belos "Block CG" with NativeJacobi on the assembled matrix (solve/BelosSolvers.hpp:116-122).
 * l3k_csr_cheb_create: Ifpack2ChebyshevPreconditioner on a matrix (solve/Ifpack2Preconditioners.hpp:107-131); d_minv from
 *   l3k_csr_diag.  The object is an l3k_cheb: l3k_cheb_apply, l3k_cheb_info_get and l3k_cheb_destroy serve it.
 * l3k_csr_pcg_solve_cheb: l3k_pcg_solve_cheb with a preconditioner created on this operator.                                  */
typedef struct l3k_csr l3k_csr;
typedef struct
{
    int64_t n, nnz, n_empty_rows, max_row_len;
    double  mean_row_len;  /* of the non-empty rows; 0 if there is none */
    int     lanes_per_row; /* in use: 4, 16 or 64                       */
} l3k_csr_info;
int l3k_csr_create(l3k_ctx* ctx, int64_t n, const int64_t* d_row_ptr, const int32_t* d_col_ind, const double* d_values,
                   int lanes_per_row, l3k_csr** out);
int l3k_csr_info_get(const l3k_csr* A, l3k_csr_info* out);
int l3k_csr_apply(l3k_csr* A, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta);
int l3k_csr_apply_energy(l3k_csr* A, const double* d_x, double* d_y, double* d_s);
int l3k_csr_diag(l3k_csr* A, double* d_diag, double damping, double threshold, double* d_minv);
int l3k_csr_dirichlet(l3k_csr* A, double* d_values, const uint8_t* d_mask, const double* d_bc_vals, size_t ldg, double* d_rhs,
                      size_t ldr, int ncols);
int l3k_csr_destroy(l3k_csr* A);
int l3k_csr_pcg_solve(l3k_csr* A, const double* d_b, double* d_x, const double* d_minv, const l3k_cg_opts* opts,
                      l3k_cg_result* result);
int l3k_csr_pcg_solve_cols(l3k_csr* A, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                           const l3k_cg_opts* opts, l3k_cg_result* results);
int l3k_csr_cheb_create(l3k_csr* A, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out);
int l3k_csr_pcg_solve_cheb(l3k_csr* A, const double* d_b, double* d_x, l3k_cheb* c, const l3k_cg_opts* opts, l3k_cg_result* result);

/* ---- sparse direct solver on a CSR operator: band Cholesky ------------------------------------------------------------------
 * What the reference reaches through Amesos2 (Klu2 / Lapack, solve/Amesos2Solvers.hpp:18-32: pre-ordering and symbolic
 * factorisation on the first call, numeric factorisation and solve on every call), for the matrices this library hands to a
 * solver: after l3k_csr_dirichlet they are symmetric and positive definite, so the factorisation is A = L L^T without pivoting.
 * Single rank.  VALUE symmetry is assumed, not checked: only the lower triangle of the permuted matrix is read.
 *
 * Symbolic phase (host, once, in l3k_chol_create): the ACTIVE rows are the rows that store an entry; empty rows (internal dofs of
 * a condensed graph, dofs outside field_inds) stay outside the factorisation and x keeps its value there, the frozen-row rule of
 * l3k_csr_diag and the PCG.  The graph must be structurally symmetric (-1, the message names the first stored (i, j) without a
 * stored (j, i)).  The active rows are ordered by reverse Cuthill-McKee, component by component, each from a pseudo-peripheral
 * node, ties by lowest degree then lowest index: the same permutation on every run and machine.  The factor lives in blocks of
 * NB x NB (32 or 64): block column K stores its diagonal block and the H(K) blocks below it, H the smallest heights that hold every
 * entry of the permuted lower triangle with K + H(K) non-decreasing -- a variable band closed under fill; the last block is
 * padded with identity.
 * Numeric phase (device, the context's stream, ordinary launches): l3k_chol_factor copies A's CURRENT values into the storage
 * and factors right-looking, three launches per block column (diagonal block in LDS; panel; trailing update on the FP64 matrix
 * cores); l3k_chol_solve gathers b, substitutes forwards and backwards (two launches per block column each way, all columns
 * together) and scatters into x.  No kernel waits for another workgroup and nothing accumulates atomically in floating point:
 * factor and solve are bitwise reproducible.
 *
 * l3k_chol_opts: max_bytes = the most the factor may occupy, 0 = 8 GiB; block = NB: 32, 64, or 0 = 64 once the ordered matrix
 *   stores an entry 64 or more rows off the diagonal, else 32.
 * l3k_chol_create: symbolic only; A must outlive the object, and its graph must not change.  -1: a null argument, another block,
 *   an unsymmetric graph, a factor above max_bytes (the message states the bytes needed and the largest H; nothing is allocated
 *   -- a 3-D system too large for a band method is refused here, not by the allocator).  One readback of the graph: synchronises.
 * l3k_chol_factor: numeric; the call a time loop repeats after it has assembled again.  A pivot that is not positive and finite
 *   is replaced by 1 and counted, nothing faults and no NaN is made of it; one readback at the end (synchronises) returns -2,
 *   "matrix is not positive definite", with n_bad_pivots and first_bad_row (the caller's numbering) in the info.
 * l3k_chol_solve: x <- A^-1 b on the active rows for ncols columns (column c at + c * ld; ld >= n for ncols > 1); other rows of
 *   x are not written.  b and x may be the same buffer.  -1 unless the last l3k_chol_factor succeeded.  The workspace is the
 *   object's; it grows at the first solve with more columns than any before, never otherwise.
 * l3k_chol_order (host only, no context, host arrays): the symbolic phase alone.  perm_out [n]: perm_out[k] = the row ordered
 *   k-th for k < n_active, then -1; heights_out [at least n / 32 + 1]: H(K) for the ceil(n_active / nb) block columns; *nb in:
 *   0, 32 or 64 as l3k_chol_opts::block, out: the block size used; *bytes in: a limit as max_bytes with 0 = none, out: the bytes
 *   the factor needs (set before the limit is applied).  Validates the graph as l3k_csr_create does.                           */
typedef struct l3k_chol l3k_chol;
typedef struct
{
    size_t max_bytes;
    int    block; /* 0 = library's choice */
} l3k_chol_opts;
typedef struct
{
    int64_t n, n_active, n_blocks;
    int     block;        /* NB in use                                                                    */
    int64_t max_height;   /* largest H(K)                                                                 */
    size_t  factor_bytes; /* of the block storage                                                         */
    double  factor_flops; /* of one l3k_chol_factor                                                       */
    double  update_flops; /* ... the share of its trailing updates (the matrix-core launches)             */
    int64_t n_bad_pivots, first_bad_row; /* of the last l3k_chol_factor; first_bad_row = -1 if there was none */
    int     factored;     /* the last l3k_chol_factor succeeded                                           */
} l3k_chol_info;
int l3k_chol_create(l3k_csr* A, const l3k_chol_opts* opts, l3k_chol** out);
int l3k_chol_factor(l3k_chol* c);
int l3k_chol_solve(l3k_chol* c, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols);
int l3k_chol_info_get(const l3k_chol* c, l3k_chol_info* out);
int l3k_chol_destroy(l3k_chol* c);
int l3k_chol_order(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, int32_t* perm_out, int32_t* heights_out, int* nb,
                   int64_t* n_active, size_t* bytes);

/* ---- CSR sparsity graph of a mesh, built on the device -------------------------------------------------------------------
 * computeLocalGraph of the reference (algsys/SparsityGraph.hpp:26-81: rows over-allocated, filled with duplicates, then sorted
 * and de-duplicated) in front of makeSparsityGraph (:299), for one rank: the d_row_ptr / d_col_ind that l3k_assembled_scatter,
 * l3k_assemble_global, l3k_condense_global and l3k_csr_create take.  Rows and columns are the rank-local dofs of
 * l3k_assembled_scatter: n = (n_owned_nodes + n_ghost_nodes) * dofs_per_node, dof = node * dofs_per_node + field_inds[u].  The
 * rows a rank receives from its neighbours (serializeSharedGraph, computeInNbrData, :83-212) are not part of it.
 *
 * L3K_GRAPH_FULL: dof (a, f) is coupled with dof (b, f') iff f and f' are in field_inds and some element of the mesh contains
 *   both node a and node b; the rows of the dofs outside field_inds are empty.  Hexes and quads.
 * L3K_GRAPH_CONDENSED: the same rule over the primary nodes of each element only (any of ix, iy, iz equal to 0 or p,
 *   mesh/ElementTraits.hpp:37-59): the graph of the condensed system; the rows of element-internal dofs are empty.  Hexes only
 *   (a quad mesh: -1).
 * Several domain kernels with different dof sets: pass the union of their field_inds (a superset graph serves every consumer).
 *
 * Output: d_row_ptr int64 [n + 1], d_col_ind int32 [nnz], columns strictly ascending within a row -- what l3k_csr_create
 * validates and the scatter kernels search.  The result is a sorted set: the same bit for bit on every run and on any context,
 * whatever order the integer atomics of the builder land in.
 *
 * field_inds: n_fields indices, strictly ascending and inside [0, dofs_per_node), else -1; NULL with n_fields = 0: all dofs of
 *   the node.  Also -1: a null mesh or out, any other kind, n >= 2^31 (as l3k_csr_create).  A mesh without elements gives nnz = 0.
 * l3k_graph_create: everything except the caller's arrays -- the node -> element table, the number of coupled nodes of every
 *   node (one workgroup per node sorts and de-duplicates the node ids of its elements, in the LDS where they fit), the row
 *   offsets.  One readback (nnz, max_row_len, n_rows_scratch, max_elems_per_node), which synchronises the context's stream; a
 *   mesh with a node whose key list (elements at the node times selected nodes per element) exceeds lds_key_capacity takes a
 *   second one, after those nodes have been counted on slices of a global buffer sized by the largest list.
 *   The object holds memory that grows with the nodes and with n_elems * (selected nodes per element), never with the node
 *   pairs or with nnz; the mesh must outlive it.
 * l3k_graph_info_get: the statistics of the readback.
 * l3k_graph_fill: writes both arrays on the context's stream (no synchronisation); may be called more than once.  d_col_ind may
 *   be NULL iff nnz == 0; a null d_row_ptr: -1.                                                                               */
typedef struct l3k_graph l3k_graph;
enum { L3K_GRAPH_FULL = 0, L3K_GRAPH_CONDENSED = 1 };
typedef struct
{
    int64_t n, nnz, n_empty_rows, max_row_len; /* dof level, as l3k_csr_info counts them            */
    int64_t n_rows_scratch;                    /* row NODES whose key list did not fit the LDS      */
    int64_t workspace_bytes;                   /* device memory the object itself holds             */
    int     max_elems_per_node, lds_key_capacity;
} l3k_graph_info;
int l3k_graph_create(l3k_mesh* mesh, int n_fields, const int* field_inds, int kind, l3k_graph** out);
int l3k_graph_info_get(const l3k_graph* g, l3k_graph_info* out);
int l3k_graph_fill(l3k_graph* g, int64_t* d_row_ptr, int32_t* d_col_ind);
int l3k_graph_destroy(l3k_graph* g);

/* ---- LocalAssembly --------------------------------------------------------------------------------------------------
 * assembleLocalSystem for a batch of elements, algsys/AssembleLocalSystem.hpp:234-256: K_e row-major [Nd][Nd],
 * F_e column-major [Nd][n_rhs] per element, elements [first, first+count).  d_K may be NULL (then only the checksum
 * below is produced); d_checksum[count] receives sum_ij K_e[i][j]*(1 + ((i*31 + j*17) % 7)) (streaming mode,
 * SURVEY.md §0 D6).  K_e is symmetric bit for bit, like the reference's selfadjointView copy (:176-182).  From order 4 the stored
 * matrices are formed in the tiled layout of l3k_local_assemble_tiled and turned by a transposition kernel on a second stream
 * (the function returns when the matrices are complete); l3k_tuning selects the other routes (direct store, dense product). */
int l3k_local_assemble(l3k_mf* mf, int64_t first, int64_t count, double* d_K, double* d_F, double* d_checksum);

/* scatterLocalSystem for a batch, algsys/ScatterLocalSystem.hpp:24-54 (called per element by assembleGlobalSystem,
 * algsys/AssembleGlobalSystem.hpp:20-53): the element matrices / right-hand sides of elements [first, first+count) -- the
 * d_K / d_F of l3k_local_assemble, in its layouts -- are summed into the caller's global system on the device.
 *   matrix: d_values[nnz] over the caller's CSR graph of the rank-local matrix (d_row_ptr[n_local_dofs + 1], d_col_ind[nnz]
 *           ascending within a row; local dof numbering, rows and columns = node * dofs_per_node + field_inds[u], the
 *           reference's row_dofs / col_dofs): values[pos(row, col)] += K_e[i][j], atomically.  What Tpetra's
 *           sumIntoLocalValues does per element row happens here for the whole batch; the host takes the finished
 *           values array (one setAllValues, or one sumIntoLocalValues per batch of rows).
 *   rhs:    d_rhs[r * ldr + row] += F_e[i][r], atomically (the reference's std::atomic_ref fetch_add).
 * Entries whose (row, col) is not in the graph are skipped and counted in *n_missing (may be NULL), as
 * sumIntoLocalValues does.  skip_dirichlet != 0: rows and columns of dofs flagged in the mesh's Dirichlet mask are left
 * out, which makes the assembled operator the matrix-free one on the free dofs (gather reads Dirichlet dofs as 0, scatter
 * skips them, algsys/MatrixFreeSystem.hpp:441-466,517-536); 0 = the plain sum of the reference's assembled path.
 * Either of (d_K, d_values) / (d_F, d_rhs) may be NULL together. */
int l3k_assembled_scatter(l3k_mf* mf, int64_t first, int64_t count, const double* d_K, const double* d_F,
                          const int64_t* d_row_ptr, const int32_t* d_col_ind, double* d_values, double* d_rhs, size_t ldr,
                          int skip_dirichlet, int64_t* n_missing);
/* assembleGlobalSystem (algsys/AssembleGlobalSystem.hpp:20-53: for every element assembleLocalSystem, then scatterLocalSystem)
 * for the elements [first, first+count) in ONE call: the library forms sub-batches of element systems in a workspace of its
 * own (workspace_bytes in total, 0 = 1 GiB; two halves) on the context's stream while the previous sub-batch is summed into
 * d_values / d_rhs on a second stream -- the element matrices never leave the device and are never seen by the host.  Same
 * graph, rhs, skip_dirichlet and n_missing semantics as l3k_assembled_scatter; d_rhs may be NULL.  Returns when the work is
 * complete (it reads back the degenerate-element flag: error -2, "Encountered degenerate element", AssembleLocalSystem.hpp:249). */
/* K_e of the elements [first, first+count) in the TILED layout that l3k_assemble_global keeps between its two kernels, for
 * consumers that do not need the reference's row-major matrix: per element the U x U blocks K[(b,u),(b',u')] with the nodes
 * b = bx + n(by + n bz), b' = bx' + n(by' + n bz') (n = order + 1) stored as [u][u'][bx'][bz][bx][by][by'][bz'], bz' fastest --
 * Nd^2 doubles as in the row-major layout, every entry present (no mirroring left to the reader).  The stores of a wave of the
 * assembly kernel fill contiguous memory (the row-major stores are 8-byte pieces at a stride of 8U bytes, measured x3.9
 * write traffic), a reader finds a matrix row in 4n runs of n^2 doubles.  Shapes without the sum-factorised assembly
 * kernel (order 8) return an error. */
int l3k_local_assemble_tiled(l3k_mf* mf, int64_t first, int64_t count, double* d_Kt);
int l3k_assemble_global(l3k_mf* mf, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind,
                        double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes,
                        int64_t* n_missing);

/* ---- matrix-free systems of several terms over one set of rows -----------------------------------------------------------------
 * algsys::MatrixFreeSystem of the reference is the sum of every assembleProblem(kernel, domain ids / boundary ids, field_access,
 * dof_inds) call made on it (algsys/MatrixFreeSystem.hpp:24-89: the declarations; :722-802: each call pushes its kernels onto the
 * per-domain lists the operator walks); tests/MultiDomainTest.cpp runs four kernels on four domains, each on a dof of its own.  An
 * l3k_mf is ONE domain kernel over every element of its mesh.  l3k_mfs is the sum: any number of l3k_mf and l3k_bnd terms, each on
 * `rows` or on an l3k_mesh over the same nodes that holds only SOME of the elements (made with l3k_mesh_create from the selected
 * rows of elem_nodes / elem_verts, interior elements first; node counts, dofs_per_node, order, dim and Dirichlet mask those of the
 * whole mesh; such a mesh has launch ranges and, in deterministic mode, a colouring of its own).  No element kernel knows of it.
 *
 * l3k_mfs_create: `rows` fixes the row space, the ghost layout and the Dirichlet mask; n_rhs >= 1 the columns the sum serves.
 *   Nothing is owned: rows and every term must outlive the object.                                   (MatrixFreeSystem.hpp:24-54)
 * l3k_mfs_add_domain / l3k_mfs_add_boundary: assembleProblem(kernel, domain ids / boundary ids)       (:56-89, :789-802).  Refused
 *   with -1 and a message naming the offence: a finalized system; a term of another context; a term whose mesh differs from
 *   `rows` in dim, order, owned or ghost node count or dofs_per_node; a Dirichlet mask that differs from that of `rows` (compared
 *   byte for byte on the device, one readback; the message names the first differing dof; a mesh without a mask counts as all
 *   zero); an l3k_mf with attached boundary terms ("add them with l3k_mfs_add_boundary"); a term with n_rhs below the system's.
 * l3k_mfs_finalize: endAssembly's bookkeeping (:876-885): the coverage mask active[n_local_dofs] -- 1 on the dofs
 *   (node, field_inds[u]) of every node of a term's elements (of a boundary term: of its sides' elements), 0 elsewhere -- and the
 *   number of active owned rows.  Adds are refused afterwards; apply, diag_rhs and the solvers are refused before.
 * l3k_mfs_info_get: n_terms, n_rows (owned dofs), n_active_rows, n_dirichlet_rows (owned), n_rhs, finalized.
 * l3k_mfs_active: the coverage mask into d_mask [n_local_dofs] (device).
 *
 * l3k_mfs_apply: Y <- alpha A X + beta Y, A = the sum of the terms (Operator::apply, :1020-1140), single rank; the split-phase
 *   pieces follow l3k_mf_scale / l3k_mf_apply_elems / l3k_mf_dirichlet_rows and take the same arguments:
 *   l3k_mfs_scale: y <- beta y on EVERY owned row.  l3k_mfs_apply_elems: every term in the order added, domain terms with the
 *   `which` classes of l3k_mf_apply_elems on their own meshes, boundary terms as l3k_mf_apply_elems runs attached ones (which = 3:
 *   the sides of interior elements, 4: none).  l3k_mfs_dirichlet_rows: y += alpha x on the owned Dirichlet rows, once.
 *   Inside a sum no term writes rows: every row of every term is accumulated (a second kernel on the same element would overwrite
 *   the first, and the scale would miss rows) -- an override of the launch, the l3k_mf is not modified and keeps working alone.
 *   Rows no term covers get beta y.  Deterministic contexts: the terms in add order, each colour by colour -- the same bits on
 *   every run.  A refused call leaves y untouched.
 * l3k_mfs_diag_rhs: computeDiagAndRhs (:888-941) summed over the terms: the arguments and the `finalize` flag of l3k_mf_diag_rhs;
 *   accumulates, zeroes nothing.  Every term forms its own n_rhs columns: -1 unless all terms have the system's n_rhs.
 * l3k_mfs_jacobi_inverse: NativeJacobiImpl::init (solve/NativePreconditioners.hpp:75-96), l3k_jacobi_inverse's formula on the active
 *   owned rows and 0 on the others -- decided by the mask, not by the value of the diagonal -- so the PCG's frozen-row rule leaves
 *   x as it is on rows no term covers (as l3k_csr_diag does for empty rows).
 * l3k_mfs_apply_energy: y <- A x, s[1] <- <x, A x> by the fixed-order dot product behind the apply.
 * l3k_mfs_pcg_solve / _pcg_solve_cols / l3k_mfs_cheb_create / l3k_mfs_pcg_solve_cheb: alg_sys.solve(CG{...}) (solve/BelosSolvers.hpp:116-122)
 *   -- the loops of l3k_pcg_solve / l3k_pcg_solve_cols / l3k_cheb_create / l3k_pcg_solve_cheb on the sum; single rank.
 * Not provided for sums: the partitioned apply and solve in one call (l3k_mf_apply_dist, l3k_pcg_solve_dist; the split-phase
 * pieces above serve a partitioned host), p-multigrid, the fused stores of exclusive rows. */
typedef struct l3k_mfs l3k_mfs;
typedef struct
{
    int64_t n_terms, n_rows, n_active_rows, n_dirichlet_rows;
    int     n_rhs, finalized;
} l3k_mfs_info;
int l3k_mfs_create(l3k_mesh* rows, int n_rhs, l3k_mfs** out);
int l3k_mfs_add_domain(l3k_mfs* S, l3k_mf* term);
int l3k_mfs_add_boundary(l3k_mfs* S, l3k_bnd* term);
int l3k_mfs_finalize(l3k_mfs* S);
int l3k_mfs_info_get(const l3k_mfs* S, l3k_mfs_info* out);
int l3k_mfs_active(const l3k_mfs* S, uint8_t* d_mask);
int l3k_mfs_destroy(l3k_mfs* S);
int l3k_mfs_apply(l3k_mfs* S, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta);
int l3k_mfs_scale(l3k_mfs* S, double* d_y, size_t ldy, int ncols, double beta);
int l3k_mfs_apply_elems(l3k_mfs* S, int which, const double* d_x, size_t ldx, const double* d_xghost, size_t ldxg, double* d_y,
                        size_t ldy, double* d_yghost, size_t ldyg, int ncols, double alpha, double beta);
int l3k_mfs_dirichlet_rows(l3k_mfs* S, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha);
int l3k_mfs_diag_rhs(l3k_mfs* S, int which, const double* d_dirichlet_vals, size_t ldg, double* d_diag, double* d_rhs, size_t ldr,
                     double* d_diag_ghost, double* d_rhs_ghost, size_t ldrg, int finalize);
int l3k_mfs_jacobi_inverse(l3k_mfs* S, const double* d_diag, double damping, double threshold, double* d_minv);
int l3k_mfs_apply_energy(l3k_mfs* S, const double* d_x, double* d_y, double* d_s);
int l3k_mfs_pcg_solve(l3k_mfs* S, const double* d_b, double* d_x, const double* d_minv, const l3k_cg_opts* opts, l3k_cg_result* result);
int l3k_mfs_pcg_solve_cols(l3k_mfs* S, const double* d_b, size_t ldb, double* d_x, size_t ldx, int ncols, const double* d_minv,
                           const l3k_cg_opts* opts, l3k_cg_result* results);
int l3k_mfs_cheb_create(l3k_mfs* S, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out);
int l3k_mfs_pcg_solve_cheb(l3k_mfs* S, const double* d_b, double* d_x, l3k_cheb* c, const l3k_cg_opts* opts, l3k_cg_result* result);

/* ---- the assembled system as one object: hexes and quads ---------------------------------------------------------------------
 * algsys::AssembledSystem of the reference (algsys/AssembledSystem.hpp: beginAssembly / assembleProblem / endAssembly, then the
 * solver on the matrix), for one rank.  The calls above it in this header stay what they are (hexes; quads refused); this route
 * has entry points of its own and takes both element types.
 *
 * l3k_asm_element_systems: assembleLocalSystem for the elements [first, first + count) of a domain term
 *   (algsys/AssembleLocalSystem.hpp:234-256): d_K [count][Nd][Nd] row-major, bitwise symmetric (the mirrored lower triangle, as
 *   the selfadjointView copy, :176-182), d_F [count][n_rhs][Nd], Nd = (p+1)^dim U; either may be NULL.  Hexes: what
 *   l3k_local_assemble returns, through the same launchers.  Quads: device/quad_assemble.hpp -- every entry written, no atomics
 *   (the same bits on every run), no mask and no lifting.  A quadrature point with |J| <= 0: -2, "Encountered degenerate
 *   element" (:249).
 * l3k_asm_side_systems: assembleLocalSystem on a BoundaryElementView (algsys/AssembleLocalSystem.hpp:77-216) for the sides
 *   [first, first + count) of a boundary term, in the order of its list: the local system of the whole element from the side
 *   quadrature, layouts as above.  Hexes: what l3k_bnd_local_assemble returns.  Quads: the side kernel of quad_assemble.hpp.
 *
 * l3k_asm_create: the system over the local dofs of `mesh` (n = n_nodes * dofs_per_node): builds the full sparsity graph of
 *   field_inds with l3k_graph_create's machinery and rules (strictly ascending indices inside [0, dofs_per_node); NULL with
 *   n_fields = 0: all dofs; the union of the terms' dofs) and owns row_ptr, col_ind, values and rhs [n_rhs][ldr].  workspace_bytes
 *   (two halves, 0 = 1 GiB, as l3k_assemble_global) sizes the sub-batches: on quads the workspace is the object's own, allocated on
 *   first use; on hexes it is that of each term, as with l3k_assemble_global / l3k_bnd_assemble_global.  Single rank: a mesh
 *   with ghost nodes is refused (-1, "partitioned"); the CSR operator is single-rank.  The mesh must outlive the object.
 * l3k_asm_begin: beginAssembly (AssembledSystem.hpp: setAllToScalar(0) on matrix and rhs): values and rhs <- 0, the system is
 *   open.  Allowed in any state (the reference calls it again after a solve); the operator is not handed out while the system is open.
 * l3k_asm_add_domain / l3k_asm_add_boundary: assembleProblem(kernel, domain ids / boundary ids): assembleGlobalSystem
 *   (algsys/AssembleGlobalSystem.hpp:20-53 / :55-96) for the elements / sides [first, first + count) of the term, summed into
 *   the object's arrays sub-batch by sub-batch; the local systems never leave the device.  The plain sum of the reference's
 *   assembled path (skip_dirichlet = 0 of l3k_assembled_scatter).  Hexes go through the pipelines behind l3k_assemble_global
 *   and l3k_bnd_assemble_global, quads through the kernels of quad_assemble.hpp in front of the same scatter kernel.  Refused
 *   with -1 and a message naming the offence: a system that is not open, a term of another dimension, a term on another mesh,
 *   field_inds that are not a subset of the system's, another n_rhs, a shape without an assembly launcher, a range outside the
 *   term, a domain term with l3k_mf_assemble_boundary on (add its boundary terms here instead).  Entries outside the graph
 *   cannot happen by construction; they are counted all the same (l3k_asm_info::n_missing).  -2: a degenerate element.  The
 *   calls return when the work is complete.
 * l3k_asm_end: endAssembly, then DirichletBCAlgebraic::apply (bcs/DirichletBC.hpp:82-150) through l3k_csr_dirichlet with the
 *   mesh's own Dirichlet mask and the prescribed values d_dirichlet_vals [n_rhs][ldg] (NULL: homogeneous); a mesh without a
 *   mask skips that step.  Creates the l3k_csr over the object's arrays (nothing copied); the system is closed.  -1, still
 *   open: a system that is not open, ldg < n, whatever l3k_csr_create or l3k_csr_dirichlet refuse.
 * l3k_asm_info_get: sizes, state, n_missing, the device pointers of the four arrays (valid as long as the object) and, on a
 *   closed system, the operator: solving is l3k_csr_diag / l3k_csr_pcg_solve* / l3k_csr_cheb_create on that handle, which the
 *   object owns (do not destroy it).
 * Static condensation on hexes is not part of this object (l3k_condense_*); on quads it is a mode of it (below).  On a
 * partitioned mesh the object is made by l3k_asm_create_dist (behind the halo section: the distributed CSR operator). */
typedef struct l3k_asm l3k_asm;
enum { L3K_ASM_NEW = 0, L3K_ASM_OPEN = 1, L3K_ASM_CLOSED = 2 };
typedef struct
{
    int64_t        n, nnz, n_missing;
    size_t         ldr;
    int            n_rhs, state;
    const int64_t* d_row_ptr;
    const int32_t* d_col_ind;
    double *       d_values, *d_rhs;
    l3k_csr*       csr; /* NULL unless state == L3K_ASM_CLOSED */
} l3k_asm_info;
int l3k_asm_element_systems(l3k_mf* term, int64_t first, int64_t count, double* d_K, double* d_F);
int l3k_asm_side_systems(l3k_bnd* term, int64_t first, int64_t count, double* d_K, double* d_F);
int l3k_asm_create(l3k_mesh* mesh, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes, l3k_asm** out);
int l3k_asm_begin(l3k_asm* A);
int l3k_asm_add_domain(l3k_asm* A, l3k_mf* term, int64_t first, int64_t count);
int l3k_asm_add_boundary(l3k_asm* A, l3k_bnd* term, int64_t first, int64_t count);
int l3k_asm_end(l3k_asm* A, const double* d_dirichlet_vals, size_t ldg);
int l3k_asm_info_get(const l3k_asm* A, l3k_asm_info* out);
int l3k_asm_destroy(l3k_asm* A);

/* ---- static condensation of the element-internal dofs inside the assembled system (quads) ----------------------------------
 * StaticCondensationManager< ElementBoundary > of the reference (algsys/StaticCondensationManager.hpp:259-473), and stateful as it
 * is: the object keeps, per element, the internal rows [K_ii | K_ib | F_i] over the system's Us fields -- Ni Us rows of
 * Ni Us + Np Us + n_rhs doubles, Np = 4 p primary nodes (ix or iy in {0, p}) and Ni = (p-1)^2 internal ones, both in ascending
 * element-local index, dofs node-major -- so
 *     store_bytes = 8 n_elems (Ni Us) (Ni Us + Np Us + n_rhs)          (4.7 KB per element at p = 2, 16 KB at p = 4, 90 KB at p = 6; Us = 3)
 * allocated at creation.  Any number of domain and boundary terms add to it; recovery needs no second assembly.
 *
 * l3k_asm_create_condensed: the arguments and refusals of l3k_asm_create; quads only -- a hex mesh is refused (-1; hexes are
 *   condensed by l3k_condense_global).  The matrix is n x n over all local dofs in the CONDENSED graph: dof (a, f) couples with
 *   (b, f') iff some element holds a and b among its primary nodes; the rows of internal dofs are empty.  At order 1 it is the
 *   full graph.  begin / add_domain / add_boundary / end / info_get / destroy serve the object as they serve any l3k_asm.
 * l3k_asm_begin also zeroes the store.  l3k_asm_add_*: same checks; every local system is split: its primary x primary block and
 *   F_b are summed into the CSR arrays, its internal rows into the element's slot of the store (element systems: plain adds, one
 *   system per element is in flight; side systems: fp64 atomics).
 * l3k_asm_end: first one elimination pass over all elements: K_ii = L L^T, W = L^-1 K_ib, h = L^-1 F_i; -W^T W and -W^T h are summed
 *   into values and rhs (bitwise symmetric per element); L^T, W and h stay in the store.  A pivot that is not positive and finite:
 *   the element contributes no update and is counted (l3k_asm_cond_info::n_failed); -2, "non-positive pivot in the
 *   element-internal block", the system stays open.  Then l3k_csr_dirichlet and the operator as for any l3k_asm.  A mask flag on
 *   an element-internal dof is refused by l3k_csr_dirichlet itself (that row has no stored diagonal): -1, the system stays open.
 *   After an l3k_asm_end that got as far as the elimination, l3k_asm_add_* and l3k_asm_end are refused until l3k_asm_begin.
 *   Slots of at most 128 KiB per workgroup are factored in the LDS; larger ones (order 6 with 4 fields, order 7 with 3, order 8
 *   with 2, and above) in place in global memory, by the same code.
 * l3k_asm_recover: x [n_rhs][ldx] over the local dofs with the solved primary dofs; writes x_i = L^-T (h - W x_b) into the
 *   internal dofs of every element (plain stores, one writer per dof, a fixed summation order: the same bits on every call).
 *   -1: a system that is not closed, not condensed, ldx < n.  May be called once per solve of a time loop.
 * l3k_asm_schur_updates: the element-level observable, from the store of a closed system: W_e = K_bi K_ii^-1 K_ib
 *   [count][Nb][Nb] row-major, bitwise symmetric, and w_e = K_bi K_ii^-1 F_i [count][n_rhs][Nb], Nb = Np Us; either may be NULL.
 *   Order 1: zeros.  -1: not closed, not condensed, a range outside the elements.
 * Both return when the work is complete. */
typedef struct
{
    int     condensed;                         /* 0 for a system made by l3k_asm_create (the other members are 0 then) */
    int     n_primary_nodes, n_internal_nodes; /* per element: 4p, (p-1)^2 */
    int64_t n_elems, store_bytes;
    int64_t n_failed; /* elements whose internal block failed its pivot test in the last l3k_asm_end */
} l3k_asm_cond_info;
int l3k_asm_create_condensed(l3k_mesh* mesh, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes, l3k_asm** out);
int l3k_asm_cond_info_get(const l3k_asm* A, l3k_asm_cond_info* out);
int l3k_asm_recover(l3k_asm* A, double* d_x, size_t ldx);
int l3k_asm_schur_updates(l3k_asm* A, int64_t first, int64_t count, double* d_W, double* d_w);

/* ---- static condensation of the element-internal dofs (hexes) -----------------------------------------------------------
 * The reference's CondensationPolicy::ElementBoundary (algsys/StaticCondensationManager.hpp).  Per element, with the primary
 * dofs b (nodes on the element boundary) and the internal dofs i (nodes with 1 <= ix, iy, iz <= p-1), both in ascending
 * element-local node index (mesh/ElementTraits.hpp:37-59 boundary_node_inds / internal_node_inds), node-major b U + u:
 *   S_e = K_bb - K_bi K_ii^-1 K_ib,  g_e = F_b - K_bi K_ii^-1 F_i        (condenseSystem, StaticCondensationManager.hpp:322-350)
 *   x_i = K_ii^-1 (F_i - K_ib x_b)                                        (recoverSolution, :410-470)
 * through a Cholesky factorisation K_ii = L L^T on the device (the reference inverts K_ii with Eigen on the host; equal to
 * rounding).  Np = (p+1)^3 - (p-1)^3 primary nodes, Nbd = Np U.  At order 1 there are no internal nodes: S_e = K_e bit for bit,
 * g_e = F_e, recovery does nothing.  A pivot of K_ii that is not positive returns -2, "non-positive pivot in the
 * element-internal block": nothing of that element reaches S_e / G_e (zeros) or the global system.  A degenerate element
 * returns -2 as l3k_local_assemble does.  Quads are refused ("quads").
 *
 * l3k_condense_local: S_e [count][Nbd][Nbd] row-major, bitwise symmetric, G_e [count][Nbd][n_rhs] column-major (i.e.
 *   [count][n_rhs][Nbd]); either may be NULL.
 * l3k_condense_global: assemble + condense + scatter of S_e / g_e into the caller's CSR graph and rhs (condenseSystem for every
 *   element, then endAssembly's sum into the condensed matrix, :352-408): same graph, ldr, skip_dirichlet, workspace_bytes
 *   (0 = 2 GiB) and n_missing semantics as l3k_assemble_global; S_e never leaves the device.  Rows and columns use the local
 *   dof numbering of l3k_assembled_scatter; the rows of internal dofs get nothing, so a graph that couples the primary nodes of
 *   each element is enough.  skip_dirichlet leaves out the rows and columns of flagged dofs; a flag on an internal dof is
 *   ignored (a domain-boundary node is never element-internal).
 * l3k_condensed_recover: x [n_rhs][ldx] over the local dofs (owned + ghost, ghosts imported): reads the primary dofs of the
 *   elements [first, first+count), writes their internal dofs (plain stores: each internal dof belongs to one element, the
 *   result is bitwise reproducible).  Stateless: the element systems are formed and eliminated again from the system's
 *   current fields and time, which must therefore not change between condensing and recovering. */
/* S_e [count][Nbd][Nbd] row-major, G_e [count][Nbd][n_rhs] column-major (Nbd = Np*U); either may be NULL */
int l3k_condense_local(l3k_mf* mf, int64_t first, int64_t count, double* d_S, double* d_G);
int l3k_condense_global(l3k_mf* mf, int64_t first, int64_t count, const int64_t* d_row_ptr, const int32_t* d_col_ind,
                        double* d_values, double* d_rhs, size_t ldr, int skip_dirichlet, size_t workspace_bytes,
                        int64_t* n_missing);
int l3k_condensed_recover(l3k_mf* mf, int64_t first, int64_t count, double* d_x, size_t ldx);

/* ---- ghost exchange of a partitioned system: RCCL neighbour send / receive behind the C ABI -----------------------------
 * Stands in for comm::Import / comm::Export and their ImportExportContext (comm/ImportExport.hpp:29-72,130-215,295-372,
 * 402-470) and for the communication part of MatrixFreeSystem::applyImpl (algsys/MatrixFreeSystem.hpp:1046-1111).  The
 * reference exchanges host memory through MPI; here the host passes device pointers and the library issues one
 * ncclGroupStart / ncclSend + ncclRecv per neighbour / ncclGroupEnd per direction on a stream of its own (RCCL over xGMI),
 * ordered against the context's stream by events.  RCCL (librccl.so.1) is loaded when the first halo is created.
 *
 * l3k_halo_unique_id: ncclGetUniqueId (128 bytes) -- one rank calls it and hands the bytes to the others out of band (the
 *   reference's host has MPI_Bcast for that).
 * l3k_halo_create: collective over the `world` ranks (ncclCommInitRank).  Exchange lists as l3k_host_mesh_view holds them:
 *   neighbour i = nbr_rank[i]; owned nodes send_nodes[send_offsets[i] .. send_offsets[i+1]) are read by it (import send,
 *   export receive); ghost nodes [ghost_offsets[i], ghost_offsets[i+1]) (numbered from 0 behind the owned nodes) are owned
 *   by it (import receive, export send).  A rank may list itself (periodic identification of its own nodes).
 * l3k_halo_import:     ghost rows <- owners' rows           (owner -> sharer copy)
 * l3k_halo_export_add: owners' rows += ghost rows           (sharer -> owner add; per neighbour in list order)
 * l3k_mf_apply_dist:   y <- alpha A x + beta y on the owned rows, x and y [ncols][ld] over the owned rows only: scale, pack,
 *   post import || first half of the interior elements, border elements, post export || second half of the interior
 *   elements, unpack-add, Dirichlet rows.  Every call returns with the work queued on the context's stream.
 *
 * The transport is a small function table (RCCL unless the caller brings one): a group of point-to-point messages between
 * `begin` and `end`, every message on the given HIP stream (the halo's communication stream), complete in stream order behind
 * `end` -- the contract of ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd.  l3k_halo_create_transport takes any table
 * (an MPI-with-device-pointers host, a test double); `destroy` (may be NULL) is called with `user` when the halo is destroyed
 * (not if its creation fails).  The library's own second implementation is the IN-PROCESS transport: the ranks are threads
 * of one process, each with its own context and stream on one GPU or on several, and a message is a device-to-device copy
 * ordered by events -- for single-process multi-GPU hosts, and the seam through which the tests run l3k_mf_apply_dist with
 * several ranks on a one-GPU box (tests/MpiImportExportTest.cpp:17-136 runs the reference's exchange on np in {1, 2, 4}).
 * l3k_inproc_group_create(world): the shared mailboxes; l3k_inproc_transport(group, rank, &table): rank's table (the group
 * owns it and must outlive the halos). */
typedef struct l3k_halo_transport
{
    void* user;
    int (*group_begin)(void* user);
    int (*send)(void* user, const double* d_buf, size_t count, int peer, void* hip_stream);
    int (*recv)(void* user, double* d_buf, size_t count, int peer, void* hip_stream);
    int (*group_end)(void* user, void* hip_stream);
    void (*destroy)(void* user);
} l3k_halo_transport;
typedef struct l3k_inproc_group l3k_inproc_group;
typedef struct l3k_halo l3k_halo;
int     l3k_halo_unique_id(char* id128);
int     l3k_halo_create(l3k_ctx* ctx, const char* id128, int rank, int world, int dofs_per_node, int n_nbrs, const int* nbr_rank,
                        const int64_t* send_offsets, const int32_t* send_nodes, const int64_t* ghost_offsets, l3k_halo** out);
int     l3k_halo_create_transport(l3k_ctx* ctx, const l3k_halo_transport* transport, int rank, int world, int dofs_per_node,
                                  int n_nbrs, const int* nbr_rank, const int64_t* send_offsets, const int32_t* send_nodes,
                                  const int64_t* ghost_offsets, l3k_halo** out);
int     l3k_inproc_group_create(int world, l3k_inproc_group** out);
int     l3k_inproc_group_destroy(l3k_inproc_group* group);
int     l3k_inproc_transport(l3k_inproc_group* group, int rank, l3k_halo_transport* out);
int     l3k_halo_destroy(l3k_halo* halo);
int64_t l3k_halo_n_ghost_dofs(const l3k_halo* halo);
int     l3k_halo_import(l3k_halo* halo, const double* d_owned, size_t ld, int ncols, double* d_ghost, size_t ldg);
int     l3k_halo_export_add(l3k_halo* halo, const double* d_ghost, size_t ldg, int ncols, double* d_owned, size_t ld);
/* Sum all-reduce of d_vals[0 .. count), 1 <= count <= 8, in place on device memory, collective over ALL `world` ranks of the halo
 * (a rank without neighbours and a rank that owns nothing take part): what MPI_Allreduce is to Belos' dot products in an MPI run
 * of the reference (solve/BelosSolvers.hpp:116-122).  Built from the transport table alone, so every transport has it: in one
 * group every rank sends its values to every other rank and receives theirs into a [world][8] device block; a one-workgroup
 * kernel then adds the rows IN ASCENDING RANK ORDER, the rank's own row at its own position.  Every rank therefore ends with the
 * same bits, and so does every run -- the collective solves below rely on it: all ranks take the same branch at a convergence
 * check.  Queued on the context's stream and ordered against the communication stream by events, as import and export are;
 * consecutive calls need no host synchronisation between them.  world == 1: nothing is done, no group call.  2 (world - 1)
 * messages of at most 64 bytes per rank: O(world^2) in all, meant for the ranks of one node.  -1, d_vals untouched: a null
 * argument, count outside [1, 8]. */
int     l3k_halo_allreduce_sum(l3k_halo* halo, double* d_vals, int count);
/* The same reduction at any width: what a step of the collective GMRES needs (k + 1 dot products per pass).
 * l3k_halo_reduce_reserve: LOCAL.  Sets the capacity -- the largest count, and the row stride of a [world][capacity] device block
 *   of its own (no memory in a world of one), 1 <= capacity <= 65536.  The same capacity again does nothing; another one waits for
 *   the reductions queued so far and reallocates.  -1: a null halo, a capacity outside the range, or another capacity than the
 *   present one while a collective solve is writing into the block.  The ranks need not reserve the same capacity.
 * l3k_halo_allreduce_sum_n: d_vals[0 .. count) <- the sum over ALL ranks, 1 <= count <= capacity, in place, with the scheme, the
 *   rank order of the additions, the equal bits on every rank and the ordering of l3k_halo_allreduce_sum: one group of
 *   2 (world - 1) messages of count doubles, then a kernel with one thread per value (ceil(count / 256) workgroups) that adds its
 *   column down the ranks.  Consecutive reductions of either kind need no host synchronisation between them.  world == 1: nothing
 *   is enqueued, the values stay.  -1, d_vals untouched, no peer involved: a null argument, no capacity reserved, count < 1 or
 *   count > capacity.  The message count is still O(world^2). */
int     l3k_halo_reduce_reserve(l3k_halo* halo, int capacity);
int     l3k_halo_allreduce_sum_n(l3k_halo* halo, double* d_vals, int count);
/* HIP events around the three element launches (first interior half, border elements, second interior half) of the next
 * n_applies calls of l3k_mf_apply_dist, on the stream they run on; _get waits for that apply and returns the durations. */
int     l3k_halo_timing_begin(l3k_halo* halo, int n_applies);
int     l3k_halo_timing_get(l3k_halo* halo, int apply, double ms[3]);
int     l3k_mf_apply_dist(l3k_mf* mf, l3k_halo* halo, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols,
                          double alpha, double beta);

/* ---- the assembled and the condensed system on a partitioned mesh: the distributed CSR operator -------------------------------
 * algsys::AssembledSystem in an MPI run of the reference (algsys/AssembledSystem.hpp: beginAssembly / assembleProblem /
 * endAssembly on every rank, then Belos on the Tpetra matrix, solve/BelosSolvers.hpp:116-122).  SUB-ASSEMBLED FORM: every rank
 * keeps the LOCAL matrix A_r of its own elements and sides over its local dofs [owned | ghost]; the global matrix
 *     A = sum_r R_r^T A_r R_r             (R_r: global dofs -> the local dofs of rank r)
 * is never formed and no matrix entry travels between ranks.  Tpetra exports the ghost rows of the matrix once, at endAssembly
 * (fillComplete); here the ghost rows of y are export-added at every apply, exactly as l3k_mf_apply_dist does it
 * (comm/ImportExport.hpp:295-372 import, :402-470 export; the schedule of algsys/MatrixFreeSystem.hpp:1020-1140).  Vectors of
 * the operator hold OWNED rows only.
 *
 * l3k_csr_dist_create: the operator over a local l3k_csr `A` (n = n_owned + ghost dofs of the halo) -- any l3k_csr: the one of a
 *   partitioned l3k_asm, or one over arrays the caller filled through l3k_assemble_global / l3k_condense_global on a partitioned
 *   hex mesh.  Sorts the local rows once into three ascending int32 lists: INTERIOR (owned, every column < n_owned; an empty owned
 *   row is interior), BORDER (owned, at least one ghost column), GHOST (row >= n_owned); an ordered compaction: the lists do not
 *   depend on the order in which anything lands.  The lists depend on the graph only; values may be rewritten.  Owns the lists,
 *   copies nothing else; A and the halo must outlive it.  -1, *out untouched: a null argument, a halo on another context than
 *   the operator, A->n != n_owned + l3k_halo_n_ghost_dofs(halo).
 * l3k_csr_dist_info_get: sizes, the three row counts, the device pointers of the lists and the local operator.
 * l3k_csr_dist_apply: y <- alpha A x + beta y on the owned rows, x and y [ncols][ld] over the owned rows (collective):
 *   pack and post the import || first half of the interior list; wait; border and ghost rows (ghost rows write the halo's export
 *   buffer, every entry of it: no zeroing); post the export || second half of the interior list; wait; unpack-add into y.
 *   Per row it is l3k_csr_apply's kernel on a vector split into its owned and ghost part: one writer per row, no floating-point
 *   atomics, beta == 0: y is not read; more than four columns go in passes of four, two and one behind ONE exchange.  In a world of
 *   one rank the result equals l3k_csr_apply's bit for bit.  A rank without neighbours has no exchange to hide and runs its interior
 *   list in one launch; a rank that owns nothing (no row, no neighbour) returns 0.
 *   l3k_halo_timing_begin / _get time its three groups of launches as they time those of l3k_mf_apply_dist.
 * l3k_csr_dist_diag: the local diagonal over [owned | ghost], the ghost part export-added to the owners (collective), then
 *   l3k_csr_diag's formula on the owned rows: d_diag [n_owned] the diagonal of A, d_minv [n_owned] = sign damping / max(|a_ii|,
 *   threshold) and 0 on an EMPTY owned row (the frozen-row rule: the internal dofs of a condensed graph).  Either may be NULL, not
 *   both.
 * l3k_csr_dirichlet_dist: the rank-local step of DirichletBCAlgebraic::apply (bcs/DirichletBC.hpp:82-150) with an OWNER RULE, on
 *   a local operator: d_mask [n] and d_bc_vals_local [ncols][ldg] are over the LOCAL dofs (the caller, or l3k_asm_end, imports the
 *   ghost values), d_rhs [ncols][ldr] likewise.  A flagged owned row becomes the identity row with rhs = g; a flagged ghost row
 *   becomes an all-zero row with rhs = 0 (the owner holds the 1); every other row, owned or ghost, gives rhs_i -= a_ij g_j over its
 *   flagged columns in l3k_csr_dirichlet's fixed order and zeroes those entries.  Summed over the ranks this is the reference's
 *   step on the global matrix.  -1, nothing written: a flagged OWNED row without a stored diagonal, n_owned outside [0, n],
 *   l3k_csr_dirichlet's other refusals.  PRECONDITION, as on the matrix-free path: the flags of a ghost dof equal its owner's.
 *
 * l3k_asm_create_dist: l3k_asm_create (condensed == 0) or l3k_asm_create_condensed (!= 0) with their arguments and refusals,
 *   except that ghost nodes are accepted; also refused (-1): a null halo, a halo on another context, a halo whose dofs_per_node
 *   or ghost range differs from the mesh's, `condensed` on hexes.  l3k_asm_begin / _add_domain / _add_boundary serve it
 *   unchanged: they are rank-local.  l3k_asm_create and l3k_asm_create_condensed keep refusing a partitioned mesh.
 * l3k_asm_end on such a system is COLLECTIVE: d_dirichlet_vals [n_rhs][ldg] is over the OWNED dofs (ldg >= n_owned; NULL:
 *   homogeneous, on every rank) and is imported to the ghost rows inside the call; the element elimination of a condensed system
 *   is rank-local and unchanged; then l3k_csr_dirichlet_dist with the mesh's mask (same precondition; a mask on every rank or on
 *   none), then the ghost rows of rhs are export-added into their owners' rows and set to 0, then the local l3k_csr and the
 *   l3k_csr_dist are created (once; the object owns both).  l3k_asm_info keeps its layout; rhs [n_rhs][ldr]: the first n_owned
 *   entries of a row are the owned right-hand side.
 * l3k_asm_dist_info_get: n_owned, n_ghost and the distributed operator (NULL unless the system is closed).  -1 on a system
 *   that is not partitioned.
 * l3k_asm_recover on a partitioned condensed system (collective): x [n_rhs][ldx] over the LOCAL dofs, ldx >= n, with the owned
 *   part filled; the call imports the ghost part itself, then writes the internal dofs (always owned). */
typedef struct l3k_csr_dist l3k_csr_dist;
typedef struct
{
    int64_t        n_owned, n_ghost;
    int64_t        n_interior_rows, n_border_rows, n_ghost_rows;
    const int32_t *d_interior_rows, *d_border_rows, *d_ghost_rows;
    l3k_csr*       local;
} l3k_csr_dist_info;
typedef struct
{
    int64_t       n_owned, n_ghost;
    l3k_csr_dist* dist; /* NULL unless state == L3K_ASM_CLOSED */
} l3k_asm_dist_info;
int l3k_csr_dist_create(l3k_csr* A, l3k_halo* halo, int64_t n_owned, l3k_csr_dist** out);
int l3k_csr_dist_info_get(const l3k_csr_dist* D, l3k_csr_dist_info* out);
int l3k_csr_dist_apply(l3k_csr_dist* D, const double* d_x, size_t ldx, double* d_y, size_t ldy, int ncols, double alpha, double beta);
int l3k_csr_dist_diag(l3k_csr_dist* D, double* d_diag, double damping, double threshold, double* d_minv);
int l3k_csr_dist_destroy(l3k_csr_dist* D);
int l3k_csr_dirichlet_dist(l3k_csr* A, double* d_values, const uint8_t* d_mask, const double* d_bc_vals_local, size_t ldg,
                           double* d_rhs, size_t ldr, int ncols, int64_t n_owned);
int l3k_asm_create_dist(l3k_mesh* mesh, l3k_halo* halo, int n_fields, const int* field_inds, int n_rhs, size_t workspace_bytes,
                        int condensed, l3k_asm** out);
int l3k_asm_dist_info_get(const l3k_asm* A, l3k_asm_dist_info* out);

/* ---- the collective solve of a partitioned system -------------------------------------------------------------------------------
 * l3k_csr_dist_apply_energy: y <- A x on the schedule of l3k_csr_dist_apply for one column (alpha = 1, beta = 0; y comes out bit
 *   for bit as that call writes it) and s[1] <- THIS RANK'S share of <x, A x> over its owned rows; no other slot of s is written.
 *   The interior rows accumulate x_i y_i inside the row kernel; the border rows, whose y is complete only behind the unpack-add,
 *   in a pass over the border list behind it (x and y at border rows only).  An interior row that a neighbour holds as a ghost
 *   row is completed by the unpack-add too: a third pass, over each neighbour's message, adds x_i times what the message added
 *   to such a row (the border rows of the message are the border pass's).  Block sums in a fixed order and one finishing block:
 *   no floating-point atomics, two calls give the same bits.  The sum over the ranks is l3k_halo_allreduce_sum's.
 *
 * The solves: what alg_sys.solve(CG{...}) is on every MPI rank of a run of the reference (solve/BelosSolvers.hpp:116-122).  The
 * loops are those of l3k_pcg_solve (cheb == NULL: Jacobi), l3k_pcg_solve_cheb, l3k_cheb_create and l3k_cheb_apply -- the same
 * code, run with the partitioned applies (l3k_mf_apply_dist; l3k_csr_dist_apply / _apply_energy) and with l3k_halo_allreduce_sum
 * on the scalar block wherever a dot product ends: s[2:4] after the initial residual and after the z pass, s[1] after the energy
 * apply, s[3] after the r pass, s[2] after a preconditioner application, <b, b> once, both dot products of every power step.
 * Vectors hold the OWNED rows; x holds the initial guess and the result; options, residual scalings, check_every, frozen rows and
 * the result are those of l3k_pcg_solve.  All four calls are COLLECTIVE and every rank passes the same options.  The reduced scalars
 * are bit-identical on all ranks, so every rank stops at the same iteration and returns the same iterations, achieved_tol and
 * converged; a call returns when the solve is complete.  Matrix-free <p, A p>: from the element kernels (l3k_mf_energy_begin /
 * _end around the launches of the distributed apply) only if every rank's launches can; otherwise l3k_cg_dot_pap on every rank --
 * decided once, at the first iteration, by all-reducing a flag.
 * l3k_cheb_create_dist / l3k_csr_dist_cheb_create: l3k_cheb_create on the partitioned operator, the power method started from
 *   the hash of THIS RANK'S row index; l3k_cheb_info_get, l3k_cheb_apply (collective on such an object) and l3k_cheb_destroy serve
 *   the object unchanged.
 * A solve with cheb != NULL takes d_minv == NULL (the object's own minv) or that very array.
 * -1, with no collective call made before the refusal: a null argument (a rank that owns no row may pass null vectors), a cheb
 * created on another operator or halo, a halo on another context than the system or whose dofs per node or ghost range do not match
 * the mesh, the option errors of l3k_cheb_create. */
int l3k_csr_dist_apply_energy(l3k_csr_dist* D, const double* d_x, double* d_y, double* d_s);
int l3k_pcg_solve_dist(l3k_mf* mf, l3k_halo* halo, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* cheb /* NULL: Jacobi */,
                       const l3k_cg_opts* opts, l3k_cg_result* result);
int l3k_csr_dist_pcg_solve(l3k_csr_dist* D, const double* d_b, double* d_x, const double* d_minv, l3k_cheb* cheb /* NULL: Jacobi */,
                           const l3k_cg_opts* opts, l3k_cg_result* result);
int l3k_cheb_create_dist(l3k_mf* mf, l3k_halo* halo, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out);
int l3k_csr_dist_cheb_create(l3k_csr_dist* D, const double* d_minv, const l3k_cheb_opts* opts, l3k_cheb** out);

/* ---- host-side synthetic mesh + block partition --------------------------------------------------------------------
 * Stand-in for makeCubeMesh + convertMeshToOrder + partitionMesh + the ownership / import-export context
 * (mesh/primitives/CubeMesh.hpp:16-138, mesh/ConvertMeshToOrder.hpp:51-104, mesh/PartitionMesh.hpp:142-183,
 * util/SegmentedOwnership.hpp:11-45, comm/ImportExport.hpp:29-72) for structured hex cubes: ne[3] elements per edge
 * on [0,1]^3, order p, parts[3] blocks, this rank's block `rank` = bx + parts[0]*(by + parts[1]*bz).
 * perturb: vertices moved by perturb*h*sin(2 pi x)sin(2 pi y)sin(2 pi z).  Host only, no GPU. */
int l3k_cube_partition_create(const int ne[3], int order, const int parts[3], int rank, double perturb,
                              l3k_hostmesh** out);
/* The quad counterpart (makeSquareMesh, mesh/primitives/SquareMesh.hpp, + convertMeshToOrder): ne[2] elements per edge on
 * [0,1]^2, order p, a single part without ghosts, numbered [non-internal nodes | element-internal nodes, contiguous per element
 * and lexicographic].  dim = 2, elem_verts [n][4][3] with z = 0, node_grid_id = gx + NX*gy, boundary bits in the quad side
 * order 0 y=0, 1 y=1, 2 x=0, 3 x=1 (mesh/ElementTraits.hpp:84-95).  perturb: interior vertices moved by
 * perturb*h*sin(2 pi x)sin(2 pi y) in x and y (detJ > 0 for |perturb| < 1/4).  Host only, no GPU. */
int l3k_square_mesh_create(const int ne[2], int order, double perturb, l3k_hostmesh** out);
int l3k_hostmesh_destroy(l3k_hostmesh* hm);
typedef struct
{
    int             dim, order;
    int64_t         n_elems, n_interior_elems;
    int64_t         n_owned_nodes, n_ghost_nodes;
    int64_t         global_node_base;      /* first global node id owned by this rank (contiguous ownership)        */
    int64_t         n_global_nodes;
    const uint32_t* elem_nodes;            /* [n_elems][N], interior elements first                                  */
    const double*   elem_verts;            /* [n_elems][2^dim][3]                                                    */
    const int64_t*  node_grid_id;          /* [n_owned+n_ghost] partition-independent id gx + NX*(gy + NY*gz)        */
    const uint8_t*  node_boundary;         /* [n_owned+n_ghost] bit s set if the node lies on cube side s            */
                                           /* sides: 0 z=0, 1 z=1, 2 y=0, 3 y=1, 4 x=0, 5 x=1 (ElementTraits.hpp:84-95) */
    int             n_nbrs;                /* neighbours, ascending rank                                             */
    const int*      nbr_rank;              /* [n_nbrs]                                                               */
    const int64_t*  send_offsets;          /* [n_nbrs+1] into send_nodes: owned nodes each neighbour shares (import
                                              send / export receive), ascending local id                             */
    const int32_t*  send_nodes;
    const int64_t*  ghost_offsets;         /* [n_nbrs+1] ghost-node ranges (relative to n_owned_nodes) owned by each
                                              neighbour (import receive / export send); ghosts are sorted by global id */
    const uint8_t*  elem_boundary;         /* [n_elems] bit s set if side s of the element lies on cube side s: the
                                              boundary views of makeCubeMesh (mesh/primitives/CubeMesh.hpp:66-138)   */
    const int64_t*  ghost_global_id;       /* [n_ghost] global node id of every ghost (ascending)                    */
} l3k_hostmesh_view;
int l3k_hostmesh_view_get(const l3k_hostmesh* hm, l3k_hostmesh_view* out);

/* ---- order elevation on the device (mesh::convertMeshToOrder, mesh/ConvertMeshToOrder.hpp:51-104, followed
 * by the [non-internal | internal] renumbering of mesh/LocalMeshView.hpp:425-458) --------------------------------------
 * conn: host, [n_elems][8] vertex ids of an order-1 hex mesh, local vertex v = i + 2j + 4k.  Writes elem_nodes (host,
 * [n_elems][(order+1)^3], local node i + n(j + n k)) numbered [vertices | edge nodes | face nodes | element-internal
 * nodes, contiguous per element]: ready for l3k_mesh_desc.elem_nodes of a single-rank mesh (n_owned_nodes = *n_nodes).
 * Shared edges / faces are found by sorting their vertex keys on the device; every element is processed in parallel.    */
int l3k_elevate_order(l3k_ctx* ctx, int64_t n_elems, const uint32_t* conn, int64_t n_vertices, int order, uint32_t* elem_nodes,
                      int64_t* n_nodes, int64_t* n_noninternal);
/* The quad twin (mesh::convertMeshToOrder on Quad elements, mesh/ConvertMeshToOrder.hpp:51-104): conn host, [n_elems][4], local
 * vertex v = i + 2j; elem_nodes host, [n_elems][(order+1)^2], local node i + n j, numbered [vertices | (order-1) per unique edge |
 * (order-1)^2 per element, contiguous per element and lexicographic].  Unique edges are numbered in the order of their sorted
 * vertex pair; positions inside an edge run from its lower vertex id, so two elements that see an edge in opposite directions
 * agree.  order 1..8; otherwise the argument checks of l3k_elevate_order.                                                       */
int l3k_elevate_order_quads(l3k_ctx* ctx, int64_t n_elems, const uint32_t* conn, int64_t n_vertices, int order,
                            uint32_t* elem_nodes, int64_t* n_nodes, int64_t* n_noninternal);

/* ---- boundary elements -> (element, side) (the reference reads the dim-1 elements of a gmsh file into the domain of their
 * entity's physical tag, mesh/ReadMesh.hpp:197-242,286-302, and MeshPartition::getBoundary(id) pairs each with the element it
 * is a side of) -----------------------------------------------------------------------------------------------------------
 * dim 3: conn [n_elems][8] (v = i + 2j + 4k), bnd_conn [n_bnd][4] in any order; dim 2: conn [n_elems][4] (v = i + 2j), bnd_conn
 * [n_bnd][2].  All pointers are host pointers.  For every boundary element: the element and side (numbered as for
 * l3k_bnd_create above: hexes 0..5 = z-, z+, y-, y+, x-, x+; quads 0..3 = y-, y+, x-, x+) whose vertex SET equals its own.  No
 * such side, or a boundary element that repeats a vertex: face_elem = -1, face_side = 255, counted in *n_unmatched.  The sides of
 * two elements have the set (an interface inside the mesh): the lower element index is returned and the case is counted in
 * *n_interior.  Every element side emits its sorted vertices as a key with the value e * 2 dim + side, the pairs are sorted on
 * the device, every boundary element takes the lower bound of its own sorted vertices: memory is two key arrays of n_elems * 2 dim
 * entries, nothing quadratic; no floating point and one writer per output, so every run gives the same answer.
 * Errors (-1): dim outside {2, 3}, negative counts, null arrays with non-zero counts, n_elems * 2 dim >= 2^32.                  */
int l3k_boundary_match(l3k_ctx* ctx, int dim, int64_t n_elems, const uint32_t* conn, int64_t n_bnd, const uint32_t* bnd_conn,
                       int64_t* face_elem, uint8_t* face_side, int64_t* n_unmatched, int64_t* n_interior);

/* ---- periodic boundary conditions (BCDefinition::definePeriodic(src_ids, dst_ids, translation), bcs/BCDefinition.hpp:92-104;
 * bcs/PeriodicBC.hpp: getNodeLocationData, NodeMatcher, getComponents) ---------------------------------------------------------
 * Two steps: l3k_periodic_match finds, from geometry, the destination node every source node is the image of; l3k_periodic_merge
 * carries the identification out on the connectivity, which gives an ordinary mesh: l3k_mesh_create, the operators, the
 * partitioner and the sparsity graph take it as any other, since all of them read the node sharing off elem_nodes.
 *
 * l3k_periodic_match.  All pointers are host pointers.  elem_nodes [n_elems][(order+1)^dim] and elem_verts [n_elems][2^dim][3] as in
 * l3k_mesh_desc; (src_elem, src_side) and (dst_elem, dst_side) list element sides, numbered as for l3k_bnd_create.  The side nodes
 * of a listed side are the (order+1)^(dim-1) local nodes of that side; the location of a node is the bi-/tri-linear map of its
 * element's vertices at the GLL reference position (mesh/NodePhysicalLocation.hpp); with dim == 2, z and translation[2] are
 * ignored.  A node listed through several sides is one node (its location is taken from the first side that lists it; they agree
 * to rounding).  Source node s matches destination node d iff |x_s + translation - x_d|_2 < tolerance (strict, as in the reference,
 * whose default is 1e-12).  Several destinations qualify: the nearest wins, ties go to the lowest node id, and the source node is
 * counted in *n_ambiguous.  None qualifies: the source node is counted in *n_unmatched, and *first_unmatched is the lowest such
 * node id (-1 if there is none) -- the reference's contract is that each node at X belonging to the source has a node at X +
 * translation.  Destination nodes nobody matches are not an error.  Output: one (pair_src[i], pair_dst[i]) per matched source node,
 * ascending in the source node; pairs with s == d are dropped; *n_pairs of them (capacity n_src * (order+1)^(dim-1)).  Every run gives
 * the same answer.
 * Only the vertices and the side node ids of the listed sides are uploaded.  A kernel evaluates the locations, the nodes are made
 * unique by a device sort on the node id, the destination nodes are binned on a uniform grid whose cell edge is at least 2 tolerance
 * and sorted by cell, and every source node looks into its own and the adjacent 3^dim - 1 cells by binary search.  Memory grows with
 * the number of listed side nodes and nothing is quadratic as long as the tolerance is below the node spacing; a tolerance above the
 * node spacing is legal and merely slow.
 * Errors (-1, l3k_last_error names the call): dim outside {2, 3}, order outside 1..8, negative counts, null arrays with non-zero
 * counts, a listed side whose element index or side is "outside the mesh", a vertex of a listed side or a translation that is not
 * finite, a tolerance that is not finite and positive; and a box of the destination vertices or a tolerance from which no grid can
 * be made, whatever the counts: a box whose extent is not finite (vertices at -1e308 and 1e308), a tolerance whose double is not
 * finite, a cell edge h = max(2 tolerance, extent / 2^20) for which 1 / h is zero or not finite (a subnormal tolerance on a box of
 * one point) or for which the cell below the box has no finite origin.  The message names the box or the tolerance; as with every
 * error of this call, nothing is launched and nothing is written to the outputs.
 *
 * l3k_periodic_merge (host only, no context).  pair_a / pair_b: n_pairs node pairs, e.g. concatenated from several
 * l3k_periodic_match calls -- all computed on the UNMERGED numbering (periodic in x and in y on a square: the four corner nodes
 * form one component); a == b and duplicate pairs are accepted.  n_noninternal: the first n_noninternal node ids are the nodes that
 * lie on element boundaries (as l3k_elevate_order returns it).  The connected components of the pair graph are formed, the
 * representative of a component is its lowest node id, node_map[old] (out, [n_nodes]) is the rank of old's representative among the
 * kept nodes in ascending old id, and the n_entries entries of elem_nodes are rewritten through it: ids stay compact, and the
 * numbering [non-internal | internal, contiguous per element] survives.  *n_nodes_out: the kept nodes; *n_noninternal_out =
 * n_noninternal - (n_nodes - *n_nodes_out); *n_components: the components of two nodes or more.
 * Errors (-1, nothing written): a pair id >= n_noninternal (an element-internal or out-of-range node), an elem_nodes entry >=
 * n_nodes, null arrays with non-zero counts, n_noninternal outside [0, n_nodes].
 *
 * A mesh one element wide along a periodic axis is legal: an element then names a node twice.  Applies, diag and rhs on it are
 * correct; bitwise reproducibility in deterministic mode is not claimed for that shape (the colouring separates elements that
 * share a node, not the repeated rows inside one element).
 * Out of scope: periodicity restricted to a subset of a node's dofs (the reference's dof_inds: dofs here are node * dofs_per_node +
 * k with no indirection to carry it), rotational periodicity, and matching across ranks (every rank holds the whole order-p
 * connectivity before it partitions, so none is needed).                                                                          */
int l3k_periodic_match(l3k_ctx* ctx, int dim, int order, int64_t n_elems, const uint32_t* elem_nodes, const double* elem_verts,
                       int64_t n_src, const int64_t* src_elem, const uint8_t* src_side, int64_t n_dst, const int64_t* dst_elem,
                       const uint8_t* dst_side, const double translation[3], double tolerance, uint32_t* pair_src,
                       uint32_t* pair_dst, int64_t* n_pairs, int64_t* n_unmatched, int64_t* n_ambiguous, int64_t* first_unmatched);
int l3k_periodic_merge(int64_t n_nodes, int64_t n_noninternal, int64_t n_pairs, const uint32_t* pair_a, const uint32_t* pair_b,
                       int64_t n_entries, uint32_t* elem_nodes, uint32_t* node_map, int64_t* n_nodes_out, int64_t* n_noninternal_out,
                       int64_t* n_components);

/* ---- native results file (host only; post/NativeIO.hpp:15-60 save, :115-146 LoadedResults, :277-295 loadResultsImpl) --
 * "L3STER results file\nv1.0\n// <comment>\n", size_t n_fields, size_t n_nodes_global, then n_fields arrays of
 * n_nodes_global doubles indexed by global node id.  Every rank saves its owned slice [node_begin, node_begin + n_local)
 * of each field (fields: host, [n_fields][ld]); exactly one rank passes write_header != 0 (the reference: rank 0).  No
 * ordering between the ranks' calls is required.  Loading gathers field values by global node id (node_ids == NULL:
 * the contiguous range starting at node_begin), as Loader::loadResults does with the saved partition's node ids.       */
int l3k_results_save(const char* path, const char* comment, size_t n_fields, int64_t n_global_nodes, int64_t node_begin,
                     int64_t n_local_nodes, const double* fields, size_t ld, int write_header);
int l3k_results_info(const char* path, size_t* n_fields, size_t* n_nodes);
int l3k_results_load(const char* path, size_t field, int64_t n, const int64_t* node_ids, int64_t node_begin, double* out);

/* ---- native mesh file (host only; post/NativeIO.hpp:75-108 save(comm, mesh, path, comment), :161-232
 * extractSavedPartitionInfo / loadUnifiedMesh / loadPartitionedMesh; mesh/MeshUtils.hpp:318-360 serializeMesh /
 * deserializeMesh; util/Serialization.hpp:20-66) ------------------------------------------------------------------------
 * "L3STER mesh file\nv1.0\n// <comment>\n", size_t n_parts, n_parts size_t part sizes, then every rank's serialised
 * MeshPartition<order>: its domains in ascending id, each the elements of type Hex, Quad, Line (mesh/ElementType.hpp:11-16)
 * as { uint64 nodes[(p+1)^d] (GLOBAL ids); double vertices[2^d][3]; uint64 id }, then nodes_begin, num_owned_nodes and
 * the boundary domain ids.  The structs below are the structure-of-arrays view of one part.  Writing: every rank
 * computes its size (l3k_meshfile_part_bytes), the sizes are gathered by the caller (the reference: comm.gather, :83),
 * every rank then calls l3k_meshfile_save with the full size table and the SAME comment (its length fixes the offsets of
 * the parts); exactly one passes write_header != 0; no ordering between the ranks' calls is required.  Reading: l3k_meshfile_load parses part `part` as a mesh of the given order
 * (the order is not stored in the file: the reference's loader takes it as a template argument); all parts in turn give
 * loadUnifiedMesh.                                                                                                      */
typedef struct
{
    size_t          n;
    const uint64_t* nodes; /* [n][(order+1)^d] global node ids, element-local lexicographic order                       */
    const double*   verts; /* [n][2^d][3]                                                                                */
    const uint64_t* ids;   /* [n] element ids (unique over the whole mesh, boundary elements included)                   */
} l3k_meshfile_elems;
typedef struct
{
    uint16_t           id; /* d_id_t (common/Typedefs.hpp)                                                               */
    l3k_meshfile_elems hex, quad, line;
} l3k_meshfile_domain;
typedef struct
{
    int                        order;
    size_t                     n_domains;
    const l3k_meshfile_domain* domains;
    uint64_t                   nodes_begin;   /* first owned global node id (0 if none owned, MeshUtils.hpp:327)        */
    size_t                     n_owned_nodes;
    size_t                     n_boundary_ids;
    const uint16_t*            boundary_ids;
} l3k_meshfile_part_desc;
typedef struct l3k_meshfile_part l3k_meshfile_part;
int l3k_meshfile_part_bytes(const l3k_meshfile_part_desc* desc, size_t* bytes);
int l3k_meshfile_save(const char* path, const char* comment, size_t n_parts, const size_t* part_bytes, size_t part,
                      const l3k_meshfile_part_desc* desc, int write_header);
int l3k_meshfile_info(const char* path, size_t* n_parts, size_t* part_bytes, size_t capacity);
int l3k_meshfile_load(const char* path, size_t part, int order, l3k_meshfile_part** out);
int l3k_meshfile_part_get(const l3k_meshfile_part* part, l3k_meshfile_part_desc* out); /* pointers live as long as part */
int l3k_meshfile_part_destroy(l3k_meshfile_part* part);

/* ---- ParaView export: .vtu / .pvtu files of a solution (post/VtkExport.hpp) -------------------------------------------------------
 * PvtuExporter{comm, mesh} + ExportDefinition + exportSolution (:16-39, :524-549).  Every rank writes `<path without extension>_<rank>.vtu`
 * (makeVtuFileName :498-505), rank 0 also `<path without extension>.pvtu` (:586-596) naming one piece per rank by its stem; no rank
 * talks to another: the caller passes rank and n_ranks.  Missing parent directories are created (:544).
 * The .vtu (makeDataDescription :618-691): UnstructuredGrid, version 1.0, LittleEndian, header_type UInt64, one Piece of the rank's
 * local nodes (owned + ghost, getNNodes()) and sum p^d linear sub-cells; every DataArray is format="appended" with its offset into one
 * <AppendedData encoding="base64"> block that starts with `_`: Position (Float64 x 3, z = +0.0 on quads; makeCoordsSerialized :365-394),
 * connectivity, offsets (UInt32), types (UInt8: 12 hexes, 9 quads; serializeTopology :304-363), then one Float64 array per field group.
 * Each array is ONE base64 stream of `uint64 payload bytes || payload`, standard alphabet, `=` padding at the array's end only:
 * 4 * ceil((8 + bytes) / 3) text bytes (util/Base64.hpp:219-226).
 * Sub-cells (serializeElementSubtopo :252-285): an order-p element gives p^d cells over its lexicographic node grid, elements in mesh
 * order, sub-cells layer / row / column, vertices base, +1, +n+1, +n (quads; hexes: the same four one layer up after them), entries are
 * local node indices; offsets = 2^d, 2 * 2^d, ...
 * Field groups (encodeField :450-466): a group names 1, 2 or 3 rows of the SoA field storage (n_fields, ld); 1 row = 1 component, 2 or
 * 3 rows = 3 components node-interleaved, the third +0.0 for a group of 2.
 * PointData attributes, in both files: Scalars = the first 1-component group, Vectors = the first 3-component group, Scalars first.
 * (The reference's .pvtu loop :117-143 labels a second vector group as Scalars when there is no scalar group; not reproduced.)
 * Coordinates of a node shared by several elements come from the LOWEST local element that contains it (the reference: whichever
 * thread stores last, :378-388), so two creations give the same bytes.
 *
 * l3k_vtk_create runs the coordinate and topology kernels, encodes the four mesh sections on the device and keeps them as host text
 * (m_encoded_coords / m_encoded_topo, :95); an export encodes the field groups only, chunk by chunk through two device and two
 * pinned host buffers of opts->chunk_bytes text bytes (0 = default; rounded down to a multiple of 16, at least 16): the host writes
 * chunk k while chunk k + 1 is encoded and copied.  The calls are synchronous: the files are complete when l3k_vtk_export returns.
 * Refusals (-1, nothing written): null arguments; a group of 0 or more than 3 rows ("Field groupings must have size 1 (scalar), 2 (2D),
 * or 3 (3D)", :454-455); a row index >= n_fields ("Out of bounds index", :536-537); ld < local nodes; a group name that is empty or
 * contains " < > &; rank outside [0, n_ranks); a path whose directory cannot be created; more than 2^32 - 1 local nodes or
 * connectivity entries (the reference overflows its UInt32 arrays silently).  A file that could not be completed is removed.
 * Out of scope: writes that outlive the call (flushWriteQueue :712-717), updateNodeCoords (:566-571; meshes here are immutable:
 * create a new exporter), line elements, cell data, compression, .pvd series, MPI-IO.                                               */
typedef struct l3k_vtk l3k_vtk;
typedef struct
{
    size_t chunk_bytes; /* text bytes per pipeline chunk; 0 = default */
} l3k_vtk_opts;
typedef struct
{
    int      dim, order;
    int64_t  n_points, n_cells, n_conn; /* local nodes, sub-cells, connectivity entries                          */
    uint64_t raw_bytes[4];              /* payload of Position, connectivity, offsets, types                     */
    uint64_t encoded_bytes[4];          /* ... their text                                                        */
    size_t   chunk_bytes;               /* of an exporter: the chunk in use (not above the largest array's text) */
    int      store_bytes;               /* of an exporter: text bytes a lane of the encoder stores at once       */
} l3k_vtk_info;
/* host only: getLocalTopoSize :291-302 and the section sizes of serializeTopology / makeCoordsSerialized */
int l3k_vtk_sizes(int dim, int order, int64_t n_elems, int64_t n_nodes, l3k_vtk_info* out);
/* util::encodeAsBase64 (util/Base64.hpp) of `uint64 n_bytes || payload` on the device, the kernel on its own: d_payload 8-byte
 * aligned, d_text 16-byte aligned with text_capacity >= 4 * ceil((8 + n_bytes) / 3); queued on the context's stream */
int l3k_vtk_encode(l3k_ctx* ctx, const void* d_payload, uint64_t n_bytes, char* d_text, uint64_t text_capacity);
/* PvtuExporter::PvtuExporter :524-530 (updateNodeCoords + initTopo) */
int l3k_vtk_create(l3k_mesh* mesh, const l3k_vtk_opts* opts, l3k_vtk** out);
int l3k_vtk_info_get(const l3k_vtk* vtk, l3k_vtk_info* out);
int l3k_vtk_destroy(l3k_vtk* vtk);
/* PvtuExporter::exportSolution :532-549.  names [n_groups]; n_comps [n_groups] rows per group; comp_inds: the groups' row indices one
 * group after the other; d_fields: SoA (n_fields, ld) on the device */
int l3k_vtk_export(l3k_vtk* vtk, const char* path, int rank, int n_ranks, int n_groups, const char* const* names, const int* n_comps,
                   const int* comp_inds, const double* d_fields, size_t ld, int n_fields);
/* host only: makePvtuFileContents :170-182 and makeDataDescription :618-691 into buf (no terminator); *needed = the length; buf ==
 * NULL: the size query.  encoded_mesh_bytes: the text bytes of Position, connectivity, offsets, types */
int l3k_vtk_pvtu_text(const char* path, int n_ranks, int n_groups, const char* const* names, const int* n_comps, char* buf,
                      size_t capacity, size_t* needed);
int l3k_vtk_vtu_header_text(int64_t n_points, int64_t n_cells, const uint64_t* encoded_mesh_bytes, int n_groups, const char* const* names,
                            const int* n_comps, char* buf, size_t capacity, size_t* needed);

/* ---- restarted GMRES -----------------------------------------------------------------------------------------------------
 * The reference's second Krylov solver: Gmres, a Belos adapter (solve/BelosSolvers.hpp:124-130) with the restart options of
 * IterSolverOpts, max_restarts = 39 and restart_length = 250 (solve/SolverInterface.hpp:26-37).  Belos is not part of the reference
 * tree; the arithmetic is the textbook restarted GMRES(m) of Saad and Schultz for one column: Arnoldi with classical Gram-Schmidt
 * and one re-orthogonalisation (CGS2), Givens rotations on the Hessenberg matrix, all on the context's stream, single rank.  It
 * serves any square operator -- l3k_csr_create accepts matrices that are not symmetric positive definite, which the PCG cannot
 * solve -- on l3k_mf, l3k_mfs and l3k_csr, with the preconditioners of the PCG: none, Jacobi d_minv, l3k_cheb, l3k_pmg.
 *
 * The preconditioner is applied on the RIGHT (Belos's adapter calls setLeftPrec): the iteration is GMRES on the live principal block
 * of A M^-1, so the residual it minimises is the true residual b - A x over the live rows, and achieved_tol has the meaning it
 * has in l3k_cg_result.  A row is live where the mask -- d_minv, or the minv the l3k_cheb / the finest smoother of the l3k_pmg was
 * created on; NULL: every row -- is non-zero on its bits.  Frozen rows keep x bit for bit and carry r = 0.
 *
 *   cycle:  r = mask(b - A x); beta = ||r||; res = beta / scale   (residual_scaling as in l3k_cg_opts)
 *           stop if res <= tol, iterations = max_iters, or more than max_restarts restarts would be needed
 *           v_0 = r / beta; g = beta e_0
 *           for k = 0 .. m - 1:  z = M^-1 v_k;  w = A z
 *               h1 = V^T w;  w -= V h1, h2 = V^T w;  w -= V h2, t = V^T w, nu^2 = <w, w>        (V = [v_0 .. v_k])
 *               H[0..k, k] = h1 + h2, H[k+1, k] = nu; the stored Givens rotations, a new one, g;  estimate = |g_{k+1}| / scale
 *               orth_loss = max(orth_loss, max_j |t_j| / nu);  iterations += 1
 *               breakdown if nu <= 2^-52 ||H[0..k, k]||: the cycle ends here;  else v_{k+1} = w / nu
 *               every check_every iterations and at the end of the cycle the host reads 64 bytes and leaves if estimate <= tol
 *           y = R^-1 g;  x += M^-1 (V y)
 * iterations counts Arnoldi steps; the explicit residual at the head of every cycle is not counted.  The solve ends only on an
 * explicit residual: when the estimate passes and the residual does not, another cycle starts and counts as a restart.  Every dot
 * product is a two-stage reduction in a fixed order without atomics: equal bits for equal input on any context.
 *
 * l3k_gmres: the workspace of GMRES(restart_length) on n rows -- restart_length + 1 basis vectors at a distance ld (n rounded up to
 * a multiple of 4), w, z, u, H, g, the rotations, the partial sums, the scalar block.  restart_length above n is lowered to n
 * (l3k_gmres_info).  max_bytes: 0 = no guard; otherwise creation refuses a workspace above it and names the bytes needed, as
 * l3k_chol_create does.  One workspace serves any number of solves of its n, one at a time.
 * opts == NULL: {1e-6, 10000, 0, 1, 39}.  -1 with a message naming the call: a null argument; a workspace whose n is not the
 * operator's number of rows; restart_length < 1, or min(restart_length, n) above 2046; b and x overlapping; an l3k_mf with ghost nodes or an l3k_mfs that is not
 * finalized or has ghost nodes (these entry points are single rank: the collective ones are below the pieces); a cheb or pmg made for another system; in the
 * pieces k < 1 or an ld that is not a multiple of 4. */
typedef struct l3k_gmres l3k_gmres;
typedef struct
{
    double tol;
    int    max_iters;
    int    residual_scaling;
    int    check_every;
    int    max_restarts;
} l3k_gmres_opts;
typedef struct
{
    double achieved_tol; /* ||mask(b - A x)|| / scale of the last explicit residual                    */
    double estimate;     /* |g_{k+1}| / scale at the last step the host looked at                      */
    double orth_loss;    /* max over the steps of max_j |<v_j, w>| / nu after the two projections      */
    int    iterations, restarts, converged, breakdown;
} l3k_gmres_result;
typedef struct
{
    int64_t n, ld;
    int     restart_length;
    size_t  bytes;
} l3k_gmres_info;
/* solve/BelosSolvers.hpp:124-130, solve/SolverInterface.hpp:26-37 (all entries of this section) */
int l3k_gmres_create(l3k_ctx* ctx, int64_t n, int restart_length, size_t max_bytes, l3k_gmres** out);
int l3k_gmres_info_get(const l3k_gmres* G, l3k_gmres_info* out);
int l3k_gmres_destroy(l3k_gmres* G);
int l3k_gmres_solve(l3k_gmres* G, l3k_mf* mf, const double* d_b, double* d_x, const double* d_minv, const l3k_gmres_opts* opts,
                    l3k_gmres_result* result);
int l3k_gmres_solve_cheb(l3k_gmres* G, l3k_mf* mf, const double* d_b, double* d_x, l3k_cheb* c, const l3k_gmres_opts* opts,
                         l3k_gmres_result* result);
int l3k_gmres_solve_pmg(l3k_gmres* G, l3k_mf* mf, const double* d_b, double* d_x, l3k_pmg* M, const l3k_gmres_opts* opts,
                        l3k_gmres_result* result);
int l3k_csr_gmres_solve(l3k_gmres* G, l3k_csr* A, const double* d_b, double* d_x, const double* d_minv, const l3k_gmres_opts* opts,
                        l3k_gmres_result* result);
int l3k_csr_gmres_solve_cheb(l3k_gmres* G, l3k_csr* A, const double* d_b, double* d_x, l3k_cheb* c, const l3k_gmres_opts* opts,
                             l3k_gmres_result* result);
int l3k_mfs_gmres_solve(l3k_gmres* G, l3k_mfs* S, const double* d_b, double* d_x, const double* d_minv, const l3k_gmres_opts* opts,
                        l3k_gmres_result* result);
int l3k_mfs_gmres_solve_cheb(l3k_gmres* G, l3k_mfs* S, const double* d_b, double* d_x, l3k_cheb* c, const l3k_gmres_opts* opts,
                             l3k_gmres_result* result);
/* The pieces, for tests and for hosts that run the loop themselves (solve/BelosSolvers.hpp:124-130, solve/SolverInterface.hpp:26-37).
 * d_V: k basis vectors, column j at d_V + j * ld, ld a multiple of 4 and >= n; rows in [n, ld) are never read.  d_mask NULL: every
 * row live; w counts as 0 on a frozen row whatever it holds there.
 *   multi_dot: h[j] = <v_j, w> for j < k, h[k] = <w, w>
 *   project  : w -= V h_in (0 stored on the frozen rows), then h_out as multi_dot of the new w; h_in[k] is not read
 *   combine  : x += [minv (.)] sum_j y_j v_j on the live rows of minv
 * All three are queued on the context's stream; multi_dot and project keep their partial sums in a buffer of the context, grown
 * on demand, so two of them must not run at the same time on one context. */
int l3k_gmres_multi_dot(l3k_ctx* ctx, const double* d_V, size_t ld, int k, const double* d_w, const double* d_mask, int64_t n, double* d_h);
int l3k_gmres_project(l3k_ctx* ctx, const double* d_V, size_t ld, int k, double* d_w, const double* d_mask, int64_t n, const double* d_h_in,
                      double* d_h_out);
int l3k_gmres_combine(l3k_ctx* ctx, const double* d_V, size_t ld, int k, const double* d_y, const double* d_minv, int64_t n, double* d_x);
/* The collective GMRES of a partitioned system: what alg_sys.solve(Gmres{...}) is on every MPI rank of a run of the reference
 * (solve/BelosSolvers.hpp:116-131).  The loop is the one above -- the same code -- run with the partitioned applies
 * (l3k_mf_apply_dist, l3k_csr_dist_apply) and with ONE l3k_halo_allreduce_sum_n wherever a reducing pass has landed:
 *   <b, b>                            1 value, once (residual_scaling 2)
 *   <r, r>                            1 value, at the head of every cycle
 *   h1 = V^T w, <w, w>                k + 2 values   (the multiDot pass of step k)
 *   h2 = V^T w, <w, w>                k + 2 values   (the first projectRedot pass)
 *   t  = V^T w, nu^2 = <w, w>         k + 2 values   (the second one)
 * so a step has three reductions and a cycle one more.  Each pass writes this rank's sums over its OWNED rows straight into its row
 * of the halo's reduction block, and the sum over the ranks lands where the single-rank pass writes; the Hessenberg column, the
 * rotations, g, nu, the breakdown test, the triangular solve and the 64 bytes the host reads are computed from reduced values
 * alone.  These are bit-identical on all ranks, so the replicated small arrays stay identical without further messages and every
 * rank takes the same decision on convergence, breakdown, the valid columns and the restart, and returns the same result.  In a
 * world of one nothing is enqueued and the solve is the single-rank one bit for bit.
 * Vectors hold the OWNED rows.  The workspace is one of n = the owned rows; EVERY RANK'S WORKSPACE MUST HAVE THE SAME
 * restart_length, and l3k_gmres_create lowers it to n: l3k_gmres_create_dist does not (n is one rank's share) and takes n == 0, the
 * workspace of a rank that owns nothing -- it brings null vectors and takes part in every reduction.  Frozen rows, options,
 * residual scalings, check_every and the result are those of l3k_gmres_solve; every rank passes the same options.  cheb: NULL --
 * Jacobi d_minv, or no preconditioner when d_minv is NULL too -- or an object of l3k_cheb_create_dist / l3k_csr_dist_cheb_create on
 * this very operator and halo (d_minv then NULL or the array it was created on).  Both calls reserve restart_length + 1 doubles on
 * the halo (l3k_halo_reduce_reserve) unless it has that capacity already, and hold the block until they return.
 * COLLECTIVE.  Every refusal (-1) comes before the first collective call: a null argument, a workspace of another context or of
 * another n than the owned rows, a halo on another context than the system or not matching its mesh, a cheb made by a single-rank
 * creator or on another operator or halo, a d_minv that is not the cheb's, b and x overlapping.  A rank that returns early from a
 * collective call for any other reason -- a launch or transport error (-3) -- leaves its peers waiting in the next exchange, as in
 * the collective PCG.  Not provided: l3k_pmg, l3k_tri and l3k_mfs on a partitioned system, several columns. */
int l3k_gmres_create_dist(l3k_ctx* ctx, int64_t n_owned, int restart_length, size_t max_bytes, l3k_gmres** out);
int l3k_gmres_solve_dist(l3k_gmres* G, l3k_mf* mf, l3k_halo* halo, const double* d_b, double* d_x, const double* d_minv,
                         l3k_cheb* cheb /* NULL: Jacobi, or none when d_minv is NULL too */, const l3k_gmres_opts* opts,
                         l3k_gmres_result* result);
int l3k_csr_dist_gmres_solve(l3k_gmres* G, l3k_csr_dist* D, const double* d_b, double* d_x, const double* d_minv,
                             l3k_cheb* cheb /* NULL: Jacobi, or none when d_minv is NULL too */, const l3k_gmres_opts* opts,
                             l3k_gmres_result* result);

/* ---- triangular preconditioners on a CSR operator: symmetric Gauss-Seidel and ILU(0) ------------------------------------------
 * What the reference reaches through Ifpack2 (solve/Ifpack2Preconditioners.hpp:97-101: Ifpack2SGSOpts, "relaxation: type" =
 * "Symmetric Gauss-Seidel"; :134-157: Ifpack2IluKOpts with level of fill 0 by default), which its solver test runs under CG and
 * GMRES (tests/SolverTests.cpp:221-232).  Ifpack2 is not part of the reference tree; the arithmetic is the textbook one, stated
 * below and restated in numpy by tests/tri_ref.py.  Single rank, one column.
 *
 * Symbolic phase (host, once, in l3k_tri_create): the ACTIVE rows are the rows that store an entry, the rule of l3k_csr_diag and
 * l3k_chol.  Empty rows are frozen: apply writes z = 0 there and a solve keeps x bit for bit; stored entries in the column of an
 * empty row lie outside the active principal block, and the factorisation and the solves ignore them.  Every active row must store
 * its diagonal entry.  level(i) = 1 + max level(j) over the stored active j < i of row i (1 without one); for the upper solve the
 * mirror image over j > i with the rows walked downwards.  The rows are listed level by level, ascending within a level.
 * Launch plan: consecutive levels of at most fuse_rows rows each form ONE launch in which one workgroup walks the levels with a
 * barrier between them, at most 4096 levels per launch; every wider level is one launch of a grid.  All are ordinary launches on
 * the context's stream.  The arithmetic of a row does not depend on the plan: equal bits for every fuse_rows, on any context.
 *
 * ILU(0), row-wise IKJ in A's pattern: for row i, for every stored active k < i in ascending order: l_ik = a_ik / u_kk; for every
 * stored j > k of row k that row i also stores: a_ij -= l_ik u_kj.  L is strictly lower with a unit diagonal implied, U carries its
 * diagonal.  Before the factorisation a_ii <- sign(a_ii) * absolute_threshold + relative_threshold * a_ii (Ifpack2's "fact:
 * absolute threshold" / "fact: relative threshold").  z = M^-1 r:  L y = r, then U z = y.
 * SGS with damping omega is SSOR, M = (D / omega + L) (omega / (2 - omega)) D^-1 (D / omega + U) with D, L, U the diagonal and the
 * strict triangles of A (omega = 1: (D + L) D^-1 (D + U)); one sweep from a zero start (Ifpack2's "relaxation: sweeps" = 1,
 * "relaxation: damping factor" = omega).  z = M^-1 r:  (D / omega + L) y = r, then (D / omega + U) z = ((2 - omega) / omega) D y:
 * the diagonal scaling is folded into the upper solve, which is what l3k_tri_solve_upper computes for this kind.
 * A row's sum runs over its entries on the wanted side in entry order per lane (lane l of the operator's lanes_per_row takes the
 * entries l, l + L, ...), combined by the fixed butterfly of the CSR apply; no floating-point atomics, no kernel waits for another
 * workgroup: results are bitwise reproducible.
 *
 * l3k_tri_opts: NULL stands for {L3K_TRI_SGS, 1, 0, 1, 0}; fuse_rows = 0 is the library's choice, 256 / lanes_per_row.
 * l3k_tri_create: symbolic only; A must outlive the object, its graph must not change, its values may.  One readback of the graph:
 *   synchronises.  -1 with a message: a null argument, an unknown kind, a damping outside (0, 2), a negative fuse_rows, an active
 *   row without a stored diagonal entry (the message names the first).
 * l3k_tri_factor: numeric; the call a time loop repeats after it has assembled again.  SGS: reads A's current diagonal and stores
 *   omega / a_ii; the solves read A's values live, nothing is copied.  ILU0: copies A's current values, applies the thresholds and
 *   factors in place.  A pivot (SGS: a diagonal entry) that is zero or not finite is replaced by 1 and counted, nothing faults and
 *   no NaN or Inf is made of it; one readback at the end (synchronises) returns -2 with n_bad_pivots and first_bad_row in the info.
 * l3k_tri_apply: z <- M^-1 r on the active rows, 0 on the others; the same bits as solve_upper(solve_lower(r)).
 * l3k_tri_solve_lower / _upper: the two pieces.  In all three the input and the output must not overlap (-1), and all three and
 *   both solver entries return -1 unless the last l3k_tri_factor succeeded.
 * l3k_tri_values: ILU0 only (-1 on SGS): the nnz factor values in A's pattern -- l_ik below the diagonal, u_ij on and above it,
 *   A's values in the columns of empty rows.
 * l3k_tri_levels (host only, no context, host arrays): level_out [n]: the level of every row as above, 0 on an empty row;
 *   upper != 0: for the upper solve.  Validates the graph as l3k_csr_create does.
 * l3k_csr_pcg_solve_tri / l3k_csr_gmres_solve_tri: the loops of l3k_csr_pcg_solve_cheb / l3k_csr_gmres_solve_cheb with this
 *   preconditioner; the frozen rows are the empty ones.  -1: a tri made on another operator than A.  An l3k_csr_dist has none. */
typedef struct l3k_tri l3k_tri;
enum
{
    L3K_TRI_SGS  = 0,
    L3K_TRI_ILU0 = 1
};
typedef struct
{
    int    kind;
    double damping;            /* SGS: omega, 0 < omega < 2; 1 = plain symmetric Gauss-Seidel                          */
    double absolute_threshold; /* ILU0: a_ii <- sign(a_ii) * absolute_threshold + relative_threshold * a_ii before the */
    double relative_threshold; /*       factorisation; 0 and 1 change nothing                                          */
    int    fuse_rows;          /* launch plan; 0 = the library's choice                                                */
} l3k_tri_opts;
typedef struct
{
    int64_t n, n_active, nnz;
    int     kind, lanes_per_row;
    int64_t n_levels_lower, n_levels_upper, max_level_rows;
    int64_t n_launches_lower, n_launches_upper; /* of one solve each way, after fusing                               */
    size_t  bytes;                              /* device memory of the object                                       */
    int64_t n_bad_pivots, first_bad_row;        /* of the last l3k_tri_factor; first_bad_row = -1 if there was none  */
    int     factored;                           /* the last l3k_tri_factor succeeded                                 */
} l3k_tri_info;
/* solve/Ifpack2Preconditioners.hpp:97-101,134-157, tests/SolverTests.cpp:221-232 (all entries of this section) */
int l3k_tri_create(l3k_csr* A, const l3k_tri_opts* opts, l3k_tri** out);
int l3k_tri_factor(l3k_tri* T);
int l3k_tri_apply(l3k_tri* T, const double* d_r, double* d_z);
int l3k_tri_solve_lower(l3k_tri* T, const double* d_r, double* d_y);
int l3k_tri_solve_upper(l3k_tri* T, const double* d_y, double* d_z);
int l3k_tri_values(const l3k_tri* T, double* d_out);
int l3k_tri_info_get(const l3k_tri* T, l3k_tri_info* out);
int l3k_tri_destroy(l3k_tri* T);
int l3k_tri_levels(int64_t n, const int64_t* row_ptr, const int32_t* col_ind, int upper, int32_t* level_out, int64_t* n_levels);
int l3k_csr_pcg_solve_tri(l3k_csr* A, const double* d_b, double* d_x, l3k_tri* T, const l3k_cg_opts* opts, l3k_cg_result* result);
int l3k_csr_gmres_solve_tri(l3k_gmres* G, l3k_csr* A, const double* d_b, double* d_x, l3k_tri* T, const l3k_gmres_opts* opts,
                            l3k_gmres_result* result);

#ifdef __cplusplus
}
#endif
#endif
