"""GradAllReduce with a frozen prefix (a frozen encoder), world_size 2 on CPU with gloo.

As in test_ddp_gloo.py a stand-in program replays a backward that finishes parameter blocks in
reverse flat order.  The first two blocks are frozen: the all-reduce must cover only
``[first trainable offset, numel)``.  Each rank fills the frozen prefix of its flat gradient with a
rank-specific value; after ``finish()`` the prefix is untouched on both ranks and the rest is the
rank average.  A second step unfreezes everything: the whole buffer is reduced again."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_ddp_gloo import _Model, _free_port


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from stfunet.ddp import GradAllReduce
    torch.manual_seed(0)
    model = _Model()
    ddp = GradAllReduce(model, bucket_mb=0.02)
    flat = model.program.flat
    results = []
    for step, frozen in enumerate((2, 0)):
        for i, blk in enumerate(model.blocks):
            blk.requires_grad_(i >= frozen)
        lo = flat.first_trainable_offset()
        flat.fresh_grad()
        expect = [torch.randn(flat.numel, generator=torch.Generator().manual_seed(100 * step + r))
                  for r in range(world)]
        mine = expect[rank]
        flat.grad[:lo] = 1000.0 + rank                 # what a frozen slice happens to hold: never read
        launched = []
        for blk in reversed(model.blocks):
            first = next(blk.parameters())
            i = flat.index[id(first)]
            b0 = flat.offsets[i]
            b1 = flat.offsets[i + 2] if i + 2 < len(flat.offsets) else flat.numel
            if b0 >= lo:
                flat.grad[b0:b1] = mine[b0:b1]
            model.program.grad_ready_hook(b0)
            launched.append(len(ddp.works))
        model.program.grad_ready_hook(0)
        ddp.finish()
        avg = sum(expect) / world
        results.append(dict(lo=lo,
                            prefix=bool((flat.grad[:lo] == 1000.0 + rank).all()),
                            rest=torch.allclose(flat.grad[lo:], avg[lo:], atol=1e-6),
                            buckets=max(launched)))
    q.put((rank, results))
    dist.barrier()
    dist.destroy_process_group()


def test_grad_allreduce_skips_frozen_prefix():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, (frozen, full) in out:
        assert frozen["lo"] == 2 * (64 * 64 + 64) and full["lo"] == 0
        assert frozen["prefix"], f"rank {rank}: the frozen prefix of the flat gradient was reduced"
        assert frozen["rest"] and full["rest"], f"rank {rank}: trainable gradients are not the rank average"
        assert frozen["buckets"] >= 2, f"rank {rank}: buckets were not launched during backward"
