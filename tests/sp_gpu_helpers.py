"""TEST INFRASTRUCTURE for the multi-rank tests that share ONE card: RCCL refuses two ranks on one device, so the collectives the
sequence-parallel and tile-parallel paths use are staged through the host and carried by gloo (a test-only transport; every byte of
compute stays the product's kernels), and a launcher that joins the ranks with a deadline."""
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


class _Done:
    def wait(self):
        return True


def stage_collectives_through_host():
    """gloo has no all_to_all for device tensors: copy to the host, exchange, copy back (synchronous; returns a finished work)."""
    real_a2a, real_ag, real_allgather = dist.all_to_all_single, dist.all_gather_into_tensor, dist.all_gather

    def a2a(output, input, group=None, async_op=False, **kw):
        o, i = torch.empty(output.shape, dtype=output.dtype), input.detach().cpu().contiguous()
        real_a2a(o, i, group=group)
        output.copy_(o)
        return _Done() if async_op else None

    def ag_into(output, input, group=None, async_op=False):
        world = dist.get_world_size(group)
        parts = [torch.empty(input.shape, dtype=input.dtype) for _ in range(world)]
        real_allgather(parts, input.detach().cpu().contiguous(), group=group)
        output.copy_(torch.cat(parts, 0).view(output.shape))
        return _Done() if async_op else None

    def ag(tensor_list, tensor, group=None, async_op=False):
        parts = [torch.empty(t.shape, dtype=t.dtype) for t in tensor_list]
        real_allgather(parts, tensor.detach().cpu().contiguous(), group=group)
        for d, s in zip(tensor_list, parts):
            d.copy_(s)
        return _Done() if async_op else None

    real_gather = dist.gather

    def gather(tensor, gather_list=None, dst=0, group=None, async_op=False):
        host_list = [torch.empty(t.shape, dtype=t.dtype) for t in gather_list] if gather_list is not None else None
        real_gather(tensor.detach().cpu().contiguous(), host_list, dst=dst, group=group)
        if gather_list is not None:
            for d, s in zip(gather_list, host_list):
                d.copy_(s)
        return _Done() if async_op else None

    dist.all_to_all_single, dist.all_gather_into_tensor, dist.all_gather, dist.gather = a2a, ag_into, ag, gather

    real_batch = dist.batch_isend_irecv

    class _RecvDone:
        def __init__(self, work, host, dev):
            self.work, self.host, self.dev = work, host, dev

        def wait(self):
            self.work.wait()
            self.dev.copy_(self.host.view(self.dev.shape))
            return True

    def batch(ops):
        """ring hops: sends leave from a host copy, receives land in a host buffer and are copied to the card on wait()"""
        host_ops, recvs = [], []
        for op in ops:
            if op.op is dist.isend:
                host_ops.append(dist.P2POp(dist.isend, op.tensor.detach().cpu().contiguous(), op.peer, op.group))
            else:
                h = torch.empty(op.tensor.shape, dtype=op.tensor.dtype)
                host_ops.append(dist.P2POp(dist.irecv, h, op.peer, op.group))
                recvs.append((len(host_ops) - 1, h, op.tensor))
        works = real_batch(host_ops)
        out = []
        if len(works) == len(host_ops):
            rmap = {i: (h, d) for i, h, d in recvs}
            for i, wk in enumerate(works):
                out.append(_RecvDone(wk, *rmap[i]) if i in rmap else wk)
        else:       # coalesced into one work object
            class _All:
                def wait(self_inner):
                    for wk in works:
                        wk.wait()
                    for _, h, d in recvs:
                        d.copy_(h.view(d.shape))
                    return True
            out = [_All()]
        return out

    dist.batch_isend_irecv = batch


def run_ranks(worker, world, args, start_method="forkserver", deadline=240.0):
    """Start `world` ranks of worker(rank, world, *args) and join them; a rank still alive at the deadline is ended and the call fails
    (a hang of one rank must not become a hang of the suite).  The ranks come from the fork server / a spawn: never a fork of the
    caller, which may hold the GPU."""
    ctx = mp.start_processes(worker, args=(world,) + tuple(args), nprocs=world, join=False, start_method=start_method)
    end = time.monotonic() + deadline
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > end:
                raise AssertionError(f"{world} ranks of {worker.__name__} did not finish within {deadline:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10.0)
            if p.is_alive():
                p.kill()
