"""The sum all-reduce of any width (l3k_halo_reduce_reserve, l3k_halo_allreduce_sum_n; NativeHalo.reduce_reserve / allreduce_n) with
the ranks as threads of this process, as in tests/test_gpu_pcg_dist.py: bit for bit the sum in ascending rank order of
tests/pcg_dist_ref.py, at counts on both sides of the 8 doubles of l3k_halo_allreduce_sum, of a wavefront (64), of a workgroup of
the adding kernel (256) and at the 2 047 of the longest restart; a chain of back-to-back reductions with nothing waiting on the
device in between; the refusals.  A rank body only computes and stores; every assertion runs afterwards in the main thread."""
import ctypes as C

import numpy as np
import pytest
import torch

import pcg_dist_ref as PD
from l3ster_amd import capi
from l3ster_amd.distributed import InprocGroup, NativeHalo
from test_gpu_asm_dist import dev, host, rank_context, run_ranks
from test_gpu_pcg_dist import bits, halo_parts

pytestmark = pytest.mark.gpu
COUNTS = (1, 8, 9, 64, 65, 257, 2047)
CAPACITY = 2048
STEPS, CHAIN_COUNT = 200, 65
LARGEST = 65536  # the largest capacity l3k_halo_reduce_reserve takes


@pytest.mark.parametrize("world,isolated", [(1, False), (2, False), (4, False), (2, True)])
def test_allreduce_n_is_the_sum_in_rank_order(world, isolated):
    """isolated: both ranks bring the halo of a whole mesh -- no neighbour, nothing to exchange -- and still take part"""
    q, parts = halo_parts(world)
    if isolated:
        parts = [q.whole] * world
    group, out, lib = InprocGroup(world), {}, capi.load()
    start = PD.order_dependent_rows(world, CHAIN_COUNT)

    def body(rank):
        d = out[rank] = {}
        halo = NativeHalo(rank_context(), parts[rank], q.U, rank, world, transport=group)
        keep = dev(np.arange(1.0, 10.0))
        vp = C.c_void_p(keep.data_ptr())
        # before a capacity is reserved
        d["unreserved"] = (lib.l3k_halo_allreduce_sum_n(halo._h, vp, 3), lib.l3k_last_error().decode())
        halo.reduce_reserve(CAPACITY)
        halo.reduce_reserve(CAPACITY)  # (the same capacity again: nothing happens)
        for count in COUNTS:
            t = dev(PD.order_dependent_rows(world, count)[rank])
            d[count] = (halo.allreduce_n(t) is t, host(t))
        # the narrow reduction between two wide ones: the two blocks follow one another on the stream
        t8, t9 = dev(PD.order_dependent_rows(world, 8)[rank]), dev(PD.order_dependent_rows(world, 9)[rank])
        halo.allreduce_n(t9)
        halo.allreduce(t8)
        t9b = dev(PD.order_dependent_rows(world, 9)[rank])
        halo.allreduce_n(t9b)
        d["mixed"] = (host(t8), host(t9), host(t9b))
        s = dev(start[rank])
        for _ in range(STEPS):  # (nothing waits for the device in here)
            halo.allreduce_n(s)
            s.mul_(0.5).add_(float(rank))
        d["chain"] = host(s)
        # refusals leave the values alone and involve no peer
        r = d["refused"] = []
        for count, ptr in ((0, vp), (CAPACITY + 1, vp), (-1, vp), (3, None)):
            r.append((lib.l3k_halo_allreduce_sum_n(halo._h, ptr, count), lib.l3k_last_error().decode()))
        r.append((lib.l3k_halo_allreduce_sum_n(None, vp, 3), lib.l3k_last_error().decode()))
        d["reserve_refused"] = [(lib.l3k_halo_reduce_reserve(h, cap), lib.l3k_last_error().decode())
                                for h, cap in ((halo._h, 0), (halo._h, -1), (halo._h, LARGEST + 1), (None, 16))]
        try:
            halo.allreduce_n(torch.zeros(CAPACITY + 1, dtype=torch.float64, device="cuda"))
            d["raised"] = False
        except capi.L3KError:
            d["raised"] = True
        d["keep"] = host(keep)
        # a smaller capacity afterwards: the block is reallocated behind the queued reductions and serves again
        halo.reduce_reserve(16)
        t = dev(PD.order_dependent_rows(world, 16)[rank])
        d["shrunk"] = (host(halo.allreduce_n(t)), lib.l3k_halo_allreduce_sum_n(halo._h, vp, 17))
        # the largest capacity: more values than GMRES ever sends, several workgroups of the adding kernel
        halo.reduce_reserve(LARGEST)
        t = dev(PD.order_dependent_rows(world, LARGEST)[rank])
        d["largest"] = host(halo.allreduce_n(t))

    run_ranks(world, body)
    for rank in range(world):
        d = out[rank]
        assert d["unreserved"][0] == -1 and "l3k_halo_allreduce_sum_n: no capacity reserved" in d["unreserved"][1]
        for count in COUNTS:
            same, got = d[count]
            assert same and bits(got) == bits(PD.sum_in_rank_order(PD.order_dependent_rows(world, count))), (count, rank)
        for got, count in zip(d["mixed"], (8, 9, 9)):
            assert bits(got) == bits(PD.sum_in_rank_order(PD.order_dependent_rows(world, count))), ("mixed", count, rank)
        assert all(rc == -1 and "l3k_halo_allreduce_sum_n" in msg for rc, msg in d["refused"]), d["refused"]
        assert all(rc == -1 and "l3k_halo_reduce_reserve" in msg for rc, msg in d["reserve_refused"]), d["reserve_refused"]
        assert d["raised"] and np.array_equal(d["keep"], np.arange(1.0, 10.0))
        assert bits(d["shrunk"][0]) == bits(PD.sum_in_rank_order(PD.order_dependent_rows(world, 16))) and d["shrunk"][1] == -1
        assert bits(d["largest"]) == bits(PD.sum_in_rank_order(PD.order_dependent_rows(world, LARGEST)))
    want = PD.chain(world, CHAIN_COUNT, STEPS, start)
    for rank in range(world):
        assert bits(out[rank]["chain"]) == bits(want[rank]), rank
    assert np.isfinite(want).all() and (world == 1 or not np.array_equal(want[0], start[0]))
    if world == 1:  # the values are left untouched
        assert all(np.array_equal(out[0][c][1], PD.order_dependent_rows(1, c)[0]) for c in COUNTS)
