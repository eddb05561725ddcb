// launch.hpp -- the host-side steps the kernel launchers share: the functor from an element kernel's parameter blob, the
// dynamic-LDS attribute, the checked launch, the dispatch of a run-time shape to its instantiation, the grid of a global-scratch
// route, the column loop.
#ifndef L3K_DEVICE_LAUNCH_HPP
#define L3K_DEVICE_LAUNCH_HPP

#include "common.hpp"

#include <type_traits>
#include <utility>

namespace l3k::dev
{
// the user's functor from the kernel's parameter blob (nullptr: a functor without parameters)
template < typename K >
K functorFrom(const void* kparam_blob)
{
    K kern{};
    if (kparam_blob)
        __builtin_memcpy(&kern, kparam_blob, sizeof(K));
    return kern;
}

// dynamic LDS a kernel may take without the attribute; allowDynamicLds is a device query and a locked table look-up per call
inline constexpr size_t default_dynamic_lds = 64 * 1024;

// `kernel` on `stream` with `lds` bytes of dynamic LDS; -3 and "<name> launch failed: ..." on error.  LDS_BOUND: what the launcher
// knows at compile time that lds cannot exceed (0: a kernel without dynamic LDS); allowDynamicLds runs first unless that rules it out
template < size_t LDS_BOUND = SIZE_MAX, typename... Params, typename... Args >
int launchKernel(const char* name, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                 const Args&... args)
{
    if constexpr (LDS_BOUND > default_dynamic_lds)
        if (!allowDynamicLds(reinterpret_cast< const void* >(kernel), lds))
        {
            setError("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu) failed", lds);
            return -3;
        }
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
    {
        setError("%s launch failed: %s", name, hipGetErrorString(err));
        return -3;
    }
    return 0;
}

// f(std::integral_constant< int, K >) for the run-time k = K in [LO, LO + sizeof...(I)): the instantiated set; not_instantiated outside it
inline constexpr int not_instantiated = 1;
template < int LO, int... I, typename F >
int withConstant(int k, std::integer_sequence< int, I... >, F&& f)
{
    int rc = not_instantiated;
    (void)((k == LO + I && (rc = f(std::integral_constant< int, LO + I >{}), true)) || ...);
    return rc;
}
// ... for a kernel's number of unknowns U in 1 .. MAX
template < int MAX, typename F >
int withUnknowns(int U, F&& f)
{
    return withConstant< 1 >(U, std::make_integer_sequence< int, MAX >{}, f);
}
// ... for a hex element's nodes per direction N1 = order + 1 in 2 .. 8
template < typename F >
int withNodes1d(int N1, F&& f)
{
    return withConstant< 2 >(N1, std::make_integer_sequence< int, 7 >{}, f);
}

// The grid of a global-scratch route (the element's buffers exceed the LDS): persistent workgroups, two per CU (no LDS, the
// registers admit them), each on its own `bytes_per_wg` slice of the context's scratch arena.  Sets a.scratch, nullptr where the
// arena cannot be had (the caller reports it).
inline unsigned scratchGrid(ElemArgs& a, size_t bytes_per_wg)
{
    const int64_t  max_wgs = 2 * int64_t(deviceComputeUnits());
    const unsigned grid    = static_cast< unsigned >(a.elem_count < max_wgs ? a.elem_count : max_wgs);
    a.scratch              = a.scratch_alloc ? a.scratch_alloc(a.scratch_owner, bytes_per_wg * grid) : nullptr;
    return grid;
}

// f(args of column c) for the columns c < ncols of a launch (x, xg, y, yg, dirichlet_vals: column c at + c * ld), until one fails
template < typename F >
int forEachColumn(const ElemArgs& a, int ncols, F&& f)
{
    for (int c = 0; c < ncols; ++c)
    {
        ElemArgs ac       = a;
        ac.x              = a.x ? a.x + a.ldx * c : nullptr;
        ac.xg             = a.xg ? a.xg + a.ldxg * c : nullptr;
        ac.y              = a.y ? a.y + a.ldy * c : nullptr;
        ac.yg             = a.yg ? a.yg + a.ldyg * c : nullptr;
        ac.dirichlet_vals = a.dirichlet_vals ? a.dirichlet_vals + a.ldg * c : nullptr;
        if (int rc = f(ac))
            return rc;
    }
    return 0;
}
} // namespace l3k::dev
#endif
