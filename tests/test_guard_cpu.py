"""The guarded optimizer step without a GPU: GradGuard's defaults, tests/guard_ref.py against a
literal clip_grad_norm_ + Adam loop on hand cases, and the trainers' data-parallel wiring of the
guard (the loss averaged over the ranks before the decision) on two gloo ranks with the device
launches replaced by CPU stand-ins."""
import math
import os

import numpy as np
import torch
import torch.distributed as dist

import guard_ref
from image_denoising_amd.optim import FlatAdam, GradGuard
from test_dist_cpu import _cpu_stand_ins, _free_port, _spawn


def test_grad_guard_defaults_are_the_references():
    """train_opt.py:118-119: grad_clip=1.0, max_loss_skip=5.0, max_grad_norm=20.0; the step is
    skipped above max_grad_norm * 10 (:149)"""
    g = GradGuard()
    assert (g.grad_clip, g.max_loss_skip, g.max_grad_norm) == (1.0, 5.0, 20.0)
    assert g.max_norm_skip == 200.0
    assert GradGuard(max_grad_norm=None).max_norm_skip is None
    p = torch.zeros(4)
    assert FlatAdam(p).guard is None and FlatAdam(p, guard=g).guard is g


def _literal_loop(p0, batches, grad_clip=1.0, max_loss_skip=5.0, max_grad_norm=20.0):
    """train_opt.py:128-157 line by line on one parameter; batches: (grad, loss)"""
    p = torch.nn.Parameter(p0.clone())
    optimizer = torch.optim.Adam([p], lr=3e-4)
    taken = []
    for g, loss in batches:
        optimizer.zero_grad(set_to_none=True)
        loss = torch.tensor(loss, dtype=torch.float64)
        if not torch.isfinite(loss) or loss.item() > max_loss_skip:
            taken.append("skipped_loss")
            continue
        p.grad = g.clone()
        total_norm = 0.0
        for q in [p]:
            if q.grad is not None:
                total_norm += q.grad.detach().data.norm(2).item() ** 2
        total_norm = total_norm ** 0.5
        if not np.isfinite(total_norm) or total_norm > max_grad_norm * 10:
            optimizer.zero_grad(set_to_none=True)
            taken.append("skipped_norm")
            continue
        if grad_clip is not None:
            torch.nn.utils.clip_grad_norm_([p], max_norm=grad_clip)
        optimizer.step()
        taken.append("applied")
    return p.detach(), taken


def test_guard_ref_equals_literal_loop_on_hand_cases():
    """norm 0.5 (below the clip), 5 (above), 201 (skipped), a NaN gradient (skipped), loss 5.0
    (applies: the comparison is strict) and nextafter(5, inf) (skips); then one more ordinary step,
    which must see an Adam state that only the applied batches touched"""
    p0 = torch.tensor([0.25, -0.5, 0.125, 1.0])
    above5 = math.nextafter(5.0, math.inf)
    batches = [
        (torch.tensor([0.3, 0.4, 0.0, 0.0]), 0.1),
        (torch.tensor([3.0, 0.0, -4.0, 0.0]), 0.1),
        (torch.tensor([201.0, 0.0, 0.0, 0.0]), 0.1),
        (torch.tensor([0.1, float("nan"), 0.0, 0.0]), 0.1),
        (torch.tensor([0.0, 0.6, 0.0, 0.8]), 5.0),
        (torch.tensor([0.5, 0.5, 0.5, 0.5]), above5),
        (torch.tensor([0.01, -0.02, 0.03, 0.0]), float("nan")),
        (torch.tensor([0.01, -0.02, 0.03, 0.0]), 0.2),
    ]
    want = ["applied", "applied", "skipped_norm", "skipped_norm", "applied", "skipped_loss",
            "skipped_loss", "applied"]
    p_lit, taken = _literal_loop(p0, batches)
    assert taken == want
    ref = guard_ref.GuardRef(p0, GradGuard())
    assert [ref.step(g, 1.0, loss) for g, loss in batches] == want
    assert torch.equal(ref.params, p_lit)
    assert ref.stats["applied"] == 4 and ref.stats["skipped_loss"] == 2
    assert ref.stats["skipped_norm"] == 2
    assert guard_ref.norm64(batches[1][0]) == 5.0
    assert guard_ref.clip_coef(5.0, 1.0) == 1.0 / (5.0 + 1e-6) and guard_ref.clip_coef(0.5, 1.0) == 1.0
    # each guard off on its own
    for gd, kw in ((GradGuard(grad_clip=None), dict(grad_clip=None)),
                   (GradGuard(max_loss_skip=None), dict(max_loss_skip=math.inf)),
                   (GradGuard(max_grad_norm=None), dict(max_grad_norm=math.inf))):
        finite = [b for b in batches if math.isfinite(b[1])]
        p_lit, taken = _literal_loop(p0, finite, **kw)
        ref = guard_ref.GuardRef(p0, gd)
        assert [ref.step(g, 1.0, loss) for g, loss in finite] == taken
        assert torch.equal(ref.params, p_lit)


def test_guard_ref_scales_before_the_norm():
    """grad_scale is inside the square: the data-parallel norm is the mean gradient's"""
    g = torch.tensor([300.0, 400.0])
    ref = guard_ref.GuardRef(torch.zeros(2), GradGuard())
    assert ref.step(g, 1.0, None) == "skipped_norm"        # 500 > 200
    assert ref.step(g, 0.25, None) == "applied"            # 125: applied, clipped
    assert ref.stats["last_norm"] == 125.0


# ---------------------------------------------------------------------------------------------
# two gloo ranks: StructureTrainer(guard=GradGuard()) with rank 1's shard carrying one NaN pixel
# ---------------------------------------------------------------------------------------------
GH = GW = 32  # the smallest network shape, one image per rank


def _guarded_stand_in(outcomes):
    """optim.guarded_adam_launch on the CPU: guard_ref on the optimizer's own buffers"""
    refs = {}

    def launch(opt, grad, grad_scale, loss):
        ref = refs.get(id(opt))
        if ref is None:
            ref = refs[id(opt)] = guard_ref.GuardRef(opt.params, opt.guard, lr=opt.lr,
                                                     betas=opt.betas, eps=opt.eps)
        ref.set_lr(opt.lr)
        outcomes.append(ref.step(grad, grad_scale, None if loss is None else float(loss)))
        if outcomes[-1] == "applied":
            with torch.no_grad():
                opt.params.copy_(ref.params)
                opt.exp_avg.copy_(ref.exp_avg)
                opt.exp_avg_sq.copy_(ref.exp_avg_sq)

    return launch


def _guard_worker(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import image_denoising_amd.optim as optim_mod
    from image_denoising_amd import UNet
    from image_denoising_amd import dist as dp
    from image_denoising_amd.trainer import StructureTrainer

    dp.init_from_env("gloo")
    torch.manual_seed(0)
    net = UNet(1, 1, 48)
    if rank == 1:  # replicas differ before the trainer's broadcast
        with torch.no_grad():
            net.flat_params.add_(0.5)
    tr = StructureTrainer(net, distributed=True, guard=GradGuard())
    _cpu_stand_ins(net, tr)
    outcomes = []
    optim_mod.guarded_adam_launch = _guarded_stand_in(outcomes)
    g = torch.Generator().manual_seed(4)
    clean = torch.rand(world, 1, GH, GW, generator=g)
    noisy = (clean + 0.1 * torch.randn(world, 1, GH, GW, generator=g)).contiguous()
    sl = slice(rank, rank + 1)
    flats = [net.flat_params.detach().clone()]
    bad = noisy[sl].clone()
    if rank == 1:
        bad[0, 0, 3, 5] = float("nan")
    losses = [tr.train_step(clean[sl], bad, epoch=1).clone()]
    flats.append(net.flat_params.detach().clone())
    losses.append(tr.train_step(clean[sl], noisy[sl], epoch=1).clone())
    flats.append(net.flat_params.detach().clone())
    state = torch.stack([tr.opt.exp_avg, tr.opt.exp_avg_sq])
    mine = torch.stack(flats)
    gathered = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    states = [torch.empty_like(state) for _ in range(world)]
    dist.all_gather(states, state)
    taken = [None] * world
    dist.all_gather_object(taken, (outcomes, [float(l[4]) for l in losses]))
    if rank == 0:
        out_q.put(([t.numpy() for t in gathered], [s.numpy() for s in states], taken))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_guarded_trainer_skips_on_one_ranks_nan():
    flats, states, taken = _spawn(_guard_worker, (2, _free_port()), 2)
    (out0, loss0), (out1, loss1) = taken
    # rank 0's own loss is finite, rank 1's is not: the decision is taken on their mean
    assert math.isfinite(loss0[0]) and not math.isfinite(loss1[0])
    assert out0 == out1 == ["skipped_loss", "applied"]
    same = lambda a, b: np.array_equal(a.view(np.int32), b.view(np.int32))  # noqa: E731
    for r in range(2):
        assert same(flats[r][1], flats[0][0]), "a skipped step moved the parameters"
    assert same(flats[0][0], flats[1][0])          # the broadcast made the replicas identical
    assert same(flats[0][2], flats[1][2])          # and the clean step moves both identically
    assert not np.array_equal(flats[0][2], flats[0][0])
    assert np.isfinite(flats[0][2]).all()
    assert same(states[0], states[1]) and np.isfinite(states[0]).all()
