// allreduce.hpp -- the adding kernels of l3k_halo_allreduce_sum and l3k_halo_allreduce_sum_n (include/l3k.h): the ranks' values,
// gathered into a [world][stride] block by point-to-point messages, summed in ascending rank order.
#ifndef L3K_DEVICE_ALLREDUCE_HPP
#define L3K_DEVICE_ALLREDUCE_HPP

#include <hip/hip_runtime.h>

namespace l3k::halo
{
constexpr int allreduce_max_count = 8; // doubles per reduction = the PCG's scalar block; the row stride of the gathered block
// vals[c] <- ((rows[0][c] + rows[1][c]) + ...) + rows[world - 1][c] for c < count: one workgroup, one thread per value, every
// rank adds the same numbers in the same order and so ends with the same bits.  Row `rank` of the block holds the rank's own values
static __global__ __launch_bounds__(64) void allreduceSumRowsKernel(const double* __restrict__ rows, int world, int count,
                                                                    double* __restrict__ vals)
{
    const int c = threadIdx.x;
    if (c >= count)
        return;
    double acc = rows[c];
    for (int r = 1; r < world; ++r)
        acc += rows[r * allreduce_max_count + c];
    vals[c] = acc;
}
// The adding kernel of l3k_halo_allreduce_sum_n: the same sum over a block whose rows are `stride` doubles apart (the capacity of
// l3k_halo_reduce_reserve), one thread per value, ceil(count / 256) workgroups; each thread adds its column down the ranks
constexpr int allreduce_n_threads  = 256;
constexpr int allreduce_n_capacity = 65536; // the largest capacity l3k_halo_reduce_reserve takes
static __global__ __launch_bounds__(allreduce_n_threads) void allreduceSumRowsNKernel(const double* __restrict__ rows, int world, int stride,
                                                                                      int count, double* __restrict__ vals)
{
    const int c = blockIdx.x * allreduce_n_threads + threadIdx.x;
    if (c >= count)
        return;
    double acc = rows[c];
    for (int r = 1; r < world; ++r)
        acc += rows[size_t(r) * stride + c];
    vals[c] = acc;
}
} // namespace l3k::halo
#endif
