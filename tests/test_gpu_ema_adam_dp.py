"""Averaged weights under data parallelism: two ranks on ONE GPU (gloo backend with device tensors), each with its own random
initialisation.  The arenas are built before engine.TrainStep broadcasts rank 0's parameters, so a rank's shadow starts as a
copy of ITS OWN parameters: TrainStep must make it follow rank 0's - the shadow as rank 0 holds it (a restored one survives),
not a fresh copy of the parameters - and one averaged step later the shadows must still agree bit for bit."""
import pytest
import torch
import torch.distributed as dist

from _ranks import init_group, run_ranks

pytestmark = [pytest.mark.gpu, pytest.mark.multiproc]

RESTORED_OFFSET = 0.25         # rank 0 moves the first slot of its shadow before TrainStep, as a restored checkpoint would


def _bits(t):
    return int(t.contiguous().view(torch.int32).long().sum())


def _worker(rank, world):
    torch.cuda.set_device(0)
    init_group('gloo', rank, world)
    from xas_amd import engine
    from xas_amd.synthetic import model_config, synthetic_batch
    cfg = model_config('HM36_Multi_SurS2')
    cfg['model_params']['cam_id_list'] = [0]
    cfg['train_params']['ema_decay'] = 0.9
    torch.manual_seed(100 + rank)                         # different init per rank: the broadcasts must fix it
    model, disc, od, odisc = engine.prepare_model(cfg)
    model.cuda().train(), disc.cuda().train()
    disc.smpl_discriminator.header.p = 0.0
    assert odisc.ema_arena is None and torch.equal(od.ema_arena, od.param_arena)
    if rank == 0:
        od.ema_views()[0].add_(RESTORED_OFFSET)
    step = engine.TrainStep(cfg, model, disc, od, odisc, num_buckets=3)
    assert step.red_det is not None
    n0 = od.ema_views()[0].numel()
    p, e = od.param_arena, od.ema_arena
    built = (_bits(p), _bits(e),
             bool(torch.equal(e[n0:], p[n0:])),                                   # untouched slots: the parameters, rank 0's
             bool(torch.equal(e[:n0], p[:n0] + RESTORED_OFFSET)))                 # rank 0's own shadow survives
    step(synthetic_batch(2, [0], torch.device('cuda'), seed=10 + rank))          # different data per rank
    torch.cuda.synchronize()
    after = (_bits(p), _bits(e), bool(torch.equal(e[n0:], p[n0:])))
    dist.destroy_process_group()
    return built, after


def test_shadow_follows_rank_zero_and_stays_identical():
    ret = run_ranks(_worker, 2)
    (built0, after0), (built1, after1) = ret[0], ret[1]
    assert built0 == built1 and built0[2] and built0[3], (built0, built1)
    assert after0 == after1 and not after0[2], (after0, after1)                   # an average now, the same on both ranks
    assert after0[0] != built0[0] and after0[1] != built0[1]
