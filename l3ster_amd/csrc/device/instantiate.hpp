// instantiate.hpp -- included by the generated per-TU instance files (l3ster_amd/build.py writes them from
// L3K_FOR_EACH_INSTANCE in user_kernels.hpp so that the heavy templates compile in parallel).
#ifndef L3K_DEVICE_INSTANTIATE_HPP
#define L3K_DEVICE_INSTANTIATE_HPP

#include <cstring>
#include <type_traits>

#include "../user_kernels.hpp"
#include "sumfact_apply.hpp"
#include "sumfact_fast.hpp"
#include "diag.hpp"
#include "assemble.hpp"
#include "condense.hpp"
#include "boundary.hpp"
#include "boundary_assemble.hpp"
#include "integral.hpp"
#include "quad.hpp"
#include "quad_boundary.hpp"
#include "quad_assemble.hpp"

namespace l3k::dev
{
#define L3K_X(id, T, name)                                                                                             \
    template <>                                                                                                        \
    struct KernelId< T >                                                                                               \
    {                                                                                                                  \
        static constexpr int value = id;                                                                               \
    };
L3K_FOR_EACH_KERNEL(L3K_X)
L3K_FOR_EACH_BOUNDARY_KERNEL(L3K_X)
#undef L3K_X
#define L3K_X(id, T, name)                                                                                             \
    template <>                                                                                                        \
    struct ResidualId< T >                                                                                             \
    {                                                                                                                  \
        static constexpr int value = id;                                                                               \
    };
L3K_FOR_EACH_RESIDUAL_KERNEL(L3K_X)
#undef L3K_X
} // namespace l3k::dev

namespace l3k::dev
{
// R columns through the one-wave-per-element kernel: all R in one pass of its multi-column variant (dense dof layouts), else one
// launch of the single-column kernel per column -- at order 6 it is ~3x faster per column than the generic LDS kernel, so R
// launches beat one R-column launch (the apply never reads the kernel's rhs, so the single-column instantiation of the functor
// gives the same operator); unknowns on a subset of the node's dofs: column by column through the strided-dof variant.
// launchColumnsFast launches it, selectRoute describes it.
template < typename T, int P, int NQ >
bool fastColumnsInOnePass(const ElemArgs& a)
{
    return FastCfg< T, P, NQ >::multi_column && a.dense;
}
template < typename T, int P, int NQ, int R >
int launchColumnsFast(const ElemArgs& a, const void* kparam_blob, hipStream_t stream)
{
    if constexpr (FastCfg< T, P, NQ >::multi_column)
        if (fastColumnsInOnePass< T, P, NQ >(a))
        {
            ElemArgs ac = a;
            ac.n_cols   = R;
            return launchSumfactFastCols< T, P, NQ >(ac, kparam_blob, stream);
        }
    return forEachColumn(a, R, [&](const ElemArgs& ac) { return launchSumfactFast< T, P, NQ >(ac, kparam_blob, stream); });
}
// the column-loop entry of a single-column instance (Instance::apply_cols), or nullptr where the single-wave kernel does not fit
template < typename T, int P, int NQ, int R >
constexpr LaunchFn selectApplyCols()
{
    if constexpr (R == 1 && FastCfg< T, P, NQ >::feasible && FastCfg< T, P, NQ >::multi_column)
        return &launchSumfactFastCols< T, P, NQ >;
    else
        return nullptr;
}
// applies use the register-resident pipelined kernel when its working set fits
template < typename T, int P, int NQ, int R >
constexpr LaunchFn selectApply()
{
    if constexpr (FastCfg< T, P, NQ >::feasible)
        return R == 1 ? &launchSumfactFast< T, P, NQ > : &launchColumnsFast< T, P, NQ, R >;
    else
        return &launchSumfactApply< T, P, NQ, R, false >;
}
// the route text of an instance's apply (l3k_mf_route)
template < typename T, int P, int NQ, int R >
constexpr RouteFn selectRoute()
{
    if constexpr (FastCfg< T, P, NQ >::feasible && R == 1)
        return &describeSumfactFast< T, P, NQ >;
    else if constexpr (FastCfg< T, P, NQ >::feasible)
        return +[](const ElemArgs& a, char* buf, size_t n) {
            const bool one_pass = fastColumnsInOnePass< T, P, NQ >(a);
            ElemArgs   ac       = a;
            ac.n_cols           = one_pass ? R : 1;
            const int rc        = describeSumfactFast< T, P, NQ >(ac, buf, n);
            if (rc == 0 && !one_pass)
                std::snprintf(buf + std::strlen(buf), n - std::strlen(buf), "; %d launches, one per column", R);
            return rc;
        };
    else
        return &describeSumfactApply< T, P, NQ, R >;
}
} // namespace l3k::dev

namespace l3k::dev
{
// The registry entry of one (functor, order, nq, columns) shape: quads (dimension 2) take the kernels of quad.hpp and the
// LocalAssembly of quad_assemble.hpp (no coefficient workspace, no tiled layout, no condensation); hexes the sum-factorised hex
// kernels and the condensation kernels of their (order, unknowns) shape.  `if constexpr` keeps the templates of the other
// dimension uninstantiated (here and in the boundary / residual entries below).
template < typename T, int P, int NQ, int R >
Instance makeInstance()
{
    if constexpr (T::params.dimension == 2)
        return {KernelId< T >::value, P, NQ, R, &launchQuadApply< T, P, NQ, R >, &launchQuadDiagRhs< T, P, NQ, R >,
                selectQuadAssemble< T, P, NQ, R >(), 0, nullptr, false, &describeQuadApply< T, P, NQ, R >};
    else
        return {KernelId< T >::value, P, NQ, R, selectApply< T, P, NQ, R >(), &launchDiagRhs< T, P, NQ, R >, &launchAssemble< T, P, NQ >,
                assembleWorkspaceDoublesPerElem< T, P, NQ >(), selectApplyCols< T, P, NQ, R >(), SfAsmCfg< P, NQ >::feasible,
                selectRoute< T, P, NQ, R >(), selectCondense< P, T::params.n_unknowns >()};
}
// ... of a boundary equation kernel: the side kernel of quad_boundary.hpp and the side assembly of quad_assemble.hpp on quads, those
// of boundary.hpp and boundary_assemble.hpp on hexes
template < typename T, int P, int NQ, int R >
BoundaryInstance makeBoundaryInstance()
{
    if constexpr (T::params.dimension == 2)
        return {KernelId< T >::value, P, NQ, R, &launchQuadSide< T, P, NQ, R, false >, &launchQuadSide< T, P, NQ, R, true >,
                selectQuadSideAssemble< T, P, NQ, R >(), 0};
    else
        return {KernelId< T >::value, P, NQ, R, &launchFace< T, P, NQ, R, false >, &launchFace< T, P, NQ, R, true >,
                &launchSideAssemble< T, P, NQ, R >, sideAssembleWorkspaceDoubles< T, NQ, R >()};
}
// ... of a residual kernel (integrals over elements and sides, values at nodes), chosen the same way
template < typename T, int P, int NQ >
IntegralInstance makeIntegralInstance()
{
    if constexpr (T::params.dimension == 2)
        return {ResidualId< T >::value, P, NQ, &launchQuadIntegral< T, P, NQ, false >, &launchQuadIntegral< T, P, NQ, true >,
                &launchQuadValuesAtNodesAny< T, P, NQ >};
    else
        return {ResidualId< T >::value, P, NQ, &launchIntegral< T, P, NQ, false >, &launchIntegral< T, P, NQ, true >,
                &launchValuesAtNodesAny< T, P, NQ >};
}
} // namespace l3k::dev

#define L3K_CAT2(a, b) a##b
#define L3K_CAT(a, b) L3K_CAT2(a, b)
#define L3K_INSTANTIATE(T, P, NQ, R)                                                                                   \
    namespace                                                                                                          \
    {                                                                                                                  \
    const struct L3K_CAT(Registrar_, __LINE__)                                                                         \
    {                                                                                                                  \
        L3K_CAT(Registrar_, __LINE__)()                                                                                \
        {                                                                                                              \
            ::l3k::dev::registerInstance(::l3k::dev::makeInstance< T, P, NQ, R >());                                   \
        }                                                                                                              \
    } L3K_CAT(registrar_, __LINE__);                                                                                   \
    }
// A kernel plugin announces its functor: id, kind (0 domain, 1 boundary, 2 residual), name
#define L3K_PLUGIN_KERNEL(ID, KIND, T, NAME)                                                                           \
    namespace                                                                                                          \
    {                                                                                                                  \
    const struct L3K_CAT(PRegistrar_, __LINE__)                                                                        \
    {                                                                                                                  \
        L3K_CAT(PRegistrar_, __LINE__)()                                                                               \
        {                                                                                                              \
            ::l3k::dev::registerPluginKernel({ID, KIND, T::params.dimension, T::params.n_equations, T::params.n_unknowns, \
                                              T::params.n_fields, T::params.n_rhs, NAME,                              \
                                              std::is_empty_v< T > ? size_t{0} : sizeof(T)});                         \
        }                                                                                                              \
    } L3K_CAT(pregistrar_, __LINE__);                                                                                  \
    }
#define L3K_INSTANTIATE_BOUNDARY(T, P, NQ, R)                                                                          \
    namespace                                                                                                          \
    {                                                                                                                  \
    const struct L3K_CAT(BRegistrar_, __LINE__)                                                                        \
    {                                                                                                                  \
        L3K_CAT(BRegistrar_, __LINE__)()                                                                               \
        {                                                                                                              \
            ::l3k::dev::registerBoundaryInstance(::l3k::dev::makeBoundaryInstance< T, P, NQ, R >());                   \
        }                                                                                                              \
    } L3K_CAT(bregistrar_, __LINE__);                                                                                  \
    }
#define L3K_INSTANTIATE_RESIDUAL(T, P, NQ)                                                                             \
    namespace                                                                                                          \
    {                                                                                                                  \
    const struct L3K_CAT(RRegistrar_, __LINE__)                                                                        \
    {                                                                                                                  \
        L3K_CAT(RRegistrar_, __LINE__)()                                                                               \
        {                                                                                                              \
            ::l3k::dev::registerIntegralInstance(::l3k::dev::makeIntegralInstance< T, P, NQ >());                      \
        }                                                                                                              \
    } L3K_CAT(rregistrar_, __LINE__);                                                                                  \
    }
#endif
