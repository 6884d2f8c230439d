"""FlatGradSync.begin_step(lo) under world-2 gloo on the CPU: with a pruned backward only [lo, n) of the flat gradient is reduced and
[0, lo) keeps each rank's own bits; a missing range inside [lo, n) still raises; lo = 0 reproduces the present result."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


class _FakeEngine:
    def __init__(self, n):
        self.flat_grads = torch.zeros(n)
        self.device = torch.device('cpu')
        self.base_seed = 1234


N, LO = 4096 + 8, 1032


def _grads(rank):
    return torch.randn(N, generator=torch.Generator().manual_seed(5 + rank))


def _worker(rank, world, port):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from hftt_hip.ddp import FlatGradSync
    own, total = _grads(rank), _grads(0) + _grads(1)
    # overlapped mode: the pruned backward reports the ranges it produced
    eng = _FakeEngine(N)
    sync = FlatGradSync(eng, world)
    eng.flat_grads.copy_(own)
    sync.begin_step(lo=LO)
    for lo, hi in ((3000, N), (LO, 3000)):
        sync.bucket_ready(lo, hi)
    assert sync(eng.flat_grads) == 0.5
    assert torch.equal(eng.flat_grads[LO:], total[LO:]) and torch.equal(eng.flat_grads[:LO], own[:LO])
    # a missing range inside [lo, n) is still an error, at its front and at its end
    for ranges in (((3000, N),), ((LO, 3000),)):
        eng.flat_grads.copy_(own)
        sync.begin_step(lo=LO)
        for lo, hi in ranges:
            sync.bucket_ready(lo, hi)
        try:
            sync(eng.flat_grads)
            raise AssertionError('missing range not detected')
        except RuntimeError as e:
            assert 'never reported ready' in str(e)
    # the plain path (no bucket_ready calls): the slices are cut at lo
    eng.flat_grads.copy_(own)
    sync3 = FlatGradSync(eng, world, buckets=3)
    sync3.begin_step(lo=LO)
    sync3(eng.flat_grads)
    assert torch.equal(eng.flat_grads[LO:], total[LO:]) and torch.equal(eng.flat_grads[:LO], own[:LO])
    # lo = 0: as ever, in both modes
    for explicit in (False, True):
        eng.flat_grads.copy_(own)
        sync.begin_step(lo=0) if explicit else sync.begin_step()
        for lo, hi in ((3000, N), (LO, 3000), (0, LO)):
            sync.bucket_ready(lo, hi)
        sync(eng.flat_grads)
        assert torch.equal(eng.flat_grads, total)
        eng.flat_grads.copy_(own)
        sync3.begin_step(lo=0) if explicit else sync3.begin_step()
        sync3(eng.flat_grads)
        assert torch.equal(eng.flat_grads, total)
    try:
        sync.begin_step(lo=N)
        raise AssertionError('lo outside the buffer not detected')
    except RuntimeError:
        pass
    dist.destroy_process_group()


def test_world2_pruned_ranges():
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)
