"""Two ranks on ONE GPU (gloo backend with device tensors): gradient averaging (dp.GradReducer), then the guarded optimizer
step.  After finish() both ranks hold the same arena bit for bit and the norm kernel is deterministic, so norm, decision and
parameters must agree bit for bit on every step - and a single inf on ONE rank must make BOTH ranks skip that step."""
import pytest
import torch
import torch.distributed as dist

from _ranks import init_group, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.multiproc]

SHAPES = [(33, 7), (5,), (257,), (64, 9)]
INF_STEP, STEPS = 1, 3


def _worker(rank, world):
    torch.cuda.set_device(0)
    init_group('gloo', rank, world)
    from xas_amd import _lib
    from xas_amd.dp import GradReducer
    from xas_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(100 + rank)             # different init and gradients per rank
    params = [torch.nn.Parameter((torch.rand(s, generator=g) * 2 - 1).cuda()) for s in SHAPES]
    opt = FusedAdam(params, lr=2e-4, betas=(0.5, 0.999), max_grad_norm=4.0, skip_nonfinite=True)
    opt.zero_grad()
    f = opt._flat
    red = GradReducer(f['g'], f['params'], f['offs'], 2, name='guarded')
    assert red.enabled and len(red.buckets) == 2
    dist.broadcast(opt.param_arena, src=0)
    rows = []
    for it in range(STEPS):
        red.arm()
        for p in params:
            p.grad.copy_((torch.randn(p.shape, generator=g) * (0.1 + it)).cuda())
        if it == INF_STEP and rank == 1:
            params[2].grad.view(-1)[100] = float('inf')
        red.finish()
        before = f['p'].clone()
        opt.step()
        bits = torch.stack([f['guard_i'][_lib.GUARD_NORM].long(), f['guard_i'][_lib.GUARD_SKIP].long(),
                            f['p'].view(torch.int32).long().sum()]).cpu()
        both = [torch.zeros_like(bits) for _ in range(world)]
        dist.all_gather(both, bits)
        assert all(torch.equal(both[0], b) for b in both), (it, both)
        rows.append(bits.tolist() + [bool(torch.equal(before, f['p'])), int(f['guard_i'][_lib.GUARD_T])])
        opt.zero_grad()
    skipped = int(opt.skipped_steps)
    dist.destroy_process_group()
    return rows, skipped


def test_two_ranks_take_the_same_decision():
    ret = run_ranks(_worker, 2)
    (rows0, skipped0), (rows1, skipped1) = ret[0], ret[1]
    assert rows0 == rows1 and skipped0 == skipped1 == 1
    for it, (norm_bits, skip, checksum, unchanged, t) in enumerate(rows0):
        assert skip == (1 if it == INF_STEP else 0), rows0
        assert unchanged == (it == INF_STEP), rows0
        assert t == it + 1 - (1 if it >= INF_STEP else 0)
    norm = torch.tensor([r[0] for r in rows0], dtype=torch.int32).view(torch.float32)
    assert torch.isinf(norm[INF_STEP]) and bool(torch.isfinite(norm[[0, 2]]).all()) and float(norm[2]) > 4.0      # step 2 is clipped
