"""Sharpness-aware minimisation without a GPU: SamConfig, the torch form of ops.sam against an fp64 numpy evaluation
of the definition, TrainStep(sam=...) against the composition written out by hand (tests/sam_cases.py), dropout, the
NaN skip, two gloo ranks, and the trainer's start-up refusals."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep, moving_average_buffers
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import elementwise as E
from distributed_tensorflow_models_amd.ops import sam
from distributed_tensorflow_models_amd.ops.prune import PruneConfig
from distributed_tensorflow_models_amd.ops.sam import SamConfig
from distributed_tensorflow_models_amd.utils.testing import run_workers

import sam_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."
MB = 8
CONFIGS = [SamConfig(0.05), SamConfig(1.0, adaptive=True)]
IDS = ["sam", "asam"]


def test_config_validation():
    c = SamConfig(0.05)
    assert c.rho == 0.05 and c.adaptive is False and SamConfig(2, adaptive=True).adaptive is True
    for bad in (0.0, -0.1, float("inf"), float("nan"), None, "x"):
        with pytest.raises(ValueError):
            SamConfig(bad)
    with pytest.raises(ValueError):
        sam.SamPerturber([], (), config=0.05)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_cpu_form_against_numpy(cfg):
    gen = torch.Generator().manual_seed(11)
    shapes = [(3, 3, 4, 5), (7,), (1,), (130, 67)]
    ps = [torch.randn(s, generator=gen) * 0.3 for s in shapes]
    gs = [torch.randn(s, generator=gen) * 0.01 for s in shapes]
    ps[0].view(-1)[0] = -0.0
    ps[3].view(-1)[5] = 1e-41  # a subnormal
    p0, g0 = [p.clone() for p in ps], [g.clone() for g in gs]
    copies = [p.to(torch.bfloat16) if p.dim() >= 2 else None for p in ps]
    stat = torch.randn(9, generator=gen)
    stat0 = stat.clone()
    sp = sam.SamPerturber([(p, g, c) for p, g, c in zip(ps, gs, copies)], [stat], config=cfg)
    sp.perturb()
    C.check_norm_scale(sp.last_norm(), sp.last_scale(), p0, g0, cfg.rho, cfg.adaptive, "cpu")
    assert sp.last_norm().dtype == torch.float32 and float(sp.last_norm()) > 0.0
    scale = float(sp.last_scale())
    for p, a, g, c, gz in zip(ps, p0, g0, copies, gs):
        want = C.oracle_p_hat(a, g, scale, cfg.adaptive).view(a.shape)
        assert C.same_bits(p, want) and not torch.equal(p, a)
        assert not gz.any() and not torch.signbit(gz).any()
        if c is not None:
            assert C.same_bits(c, want.to(torch.bfloat16))
    stat.add_(1.0)  # the second forward's in-place update
    sp.restore()
    assert all(C.same_bits(p, a) for p, a in zip(ps, p0)) and C.same_bits(stat, stat0)
    assert all(C.same_bits(c, a.to(torch.bfloat16)) for c, a in zip(copies, p0) if c is not None)
    assert not any(g.any() for g in gs)  # restore leaves the gradients alone


def test_cpu_form_nonfinite_and_zero_gradient():
    p = torch.tensor([1.0, -2.0, 3.0, 0.5])
    for bad, all_nan in ((float("nan"), True), (float("inf"), False)):
        w, g = p.clone(), torch.tensor([0.1, bad, 0.2, -0.3])
        sp = sam.SamPerturber([(w, g, None)], config=SamConfig(0.05))
        sp.perturb()
        if all_nan:
            assert bool(torch.isnan(w).all()) and math.isnan(float(sp.last_scale()))
        else:
            assert float(sp.last_scale()) == 0.0 and torch.isnan(w).tolist() == [False, True, False, False]
            assert torch.equal(w[[0, 2, 3]], p[[0, 2, 3]])
        sp.restore()
        assert C.same_bits(w, p)
    w, g = p.clone(), torch.zeros(4)
    sp = sam.SamPerturber([(w, g, None)], config=SamConfig(0.05, adaptive=True))
    sp.perturb()
    assert float(sp.last_norm()) == 0.0 and C.same_bits(w, p)  # S == 0: e is 0


# ---- the step ---------------------------------------------------------------------------------------------------
def resnet8():
    torch.manual_seed(0)
    return nets_factory.build("cifar10_resnet_v2", num_classes=10, resnet_size=8)


def lenet(keep=1.0):
    torch.manual_seed(0)
    return nets_factory.build("lenet", 10, dropout_keep_prob=keep)


def cifar_rows(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 32, 32, 3, generator=g), torch.randint(0, 10, (n,), generator=g)


def mnist_rows(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 28, 28, 1, generator=g), torch.randint(0, 10, (n,), generator=g)


def run_pair(build, batches, cfg, n=1, seed=None, **kw):
    """TrainStep(sam=cfg) and the hand composition over ``batches`` from the same start; returns both final states,
    both loss lists and the step (still open)."""
    if seed is not None:
        E.set_base_seed(seed)
    model = build()
    step = TrainStep(model, sam=cfg, accum_steps=n, **kw)
    got_losses = [float(step(x, y)) for x, y in batches]
    got = C.model_state(model, step)
    if seed is not None:
        E.set_base_seed(seed)
    twin = build()
    plain = TrainStep(twin, **kw)
    hand = C.HandSam(plain, cfg)
    want_losses = [float(hand.step(list(x.chunk(n)), list(y.chunk(n)), kw["lr"])) for x, y in batches]
    want = C.model_state(twin, plain)
    plain.dp.close()
    return got, want, got_losses, want_losses, step


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_step_matches_the_hand_composition(cfg):
    x, y = cifar_rows(3 * MB)
    batches = list(zip(x.split(MB), y.split(MB)))
    start = [p.detach().clone() for p in resnet8().parameters()]
    got, want, gl, wl, step = run_pair(resnet8, batches, cfg, optimizer="momentum", lr=0.05, momentum=0.9,
                                       ema_decay=0.99)
    assert len(moving_average_buffers(step.model)) > 0 and len(got) > 30
    assert C.states_equal(got, want) and gl == wl and all(math.isfinite(v) for v in gl)
    assert not torch.equal(got[0], start[0])
    assert step.global_step == 3 and not step.poll_skipped() and step.last_sam_norm() > 0.0
    # and SAM is not the plain step
    model = resnet8()
    plain = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, ema_decay=0.99)
    for xb, yb in batches:
        plain(xb, yb)
    assert not C.states_equal(got, C.model_state(model, plain))
    plain.dp.close()
    step.dp.close()


def test_step_with_accumulation_matches_the_hand_composition():
    x, y = cifar_rows(2 * 2 * MB, seed=6)
    batches = list(zip(x.split(2 * MB), y.split(2 * MB)))
    got, want, gl, wl, step = run_pair(resnet8, batches, SamConfig(0.05), n=2, optimizer="adam", lr=0.002)
    assert C.states_equal(got, want) and gl == wl
    assert step.dp.grad_scale == 0.5 and step.nonfinite_micro() == [0, 0]
    step.dp.close()


def test_both_passes_draw_one_dropout_mask():
    x, y = mnist_rows(2 * MB)
    batches = list(zip(x.split(MB), y.split(MB)))
    kw = dict(optimizer="sgd", lr=0.1)
    got, want, gl, wl, step = run_pair(lambda: lenet(0.5), batches, SamConfig(0.1), seed=7, **kw)
    assert C.states_equal(got, want) and gl == wl
    step.dp.close()
    # a descent pass under a mask of its own would have been seen: the hand composition without the rewind
    E.set_base_seed(7)
    twin = lenet(0.5)
    plain = TrainStep(twin, **kw)
    hand = C.HandSam(plain, SamConfig(0.1))
    xb, yb = batches[0]
    plain._forward_backward(xb, yb)
    hand.samp.perturb()
    plain._forward_backward(xb, yb)  # (the seed stream went on)
    hand.samp.restore()
    plain.opt.step(0.1)
    E.set_base_seed(7)
    model = lenet(0.5)
    one = TrainStep(model, sam=SamConfig(0.1), **kw)
    one(xb, yb)
    assert not C.states_equal(C.model_state(model, one), C.model_state(twin, plain))
    one.dp.close()
    plain.dp.close()


def test_nan_input_skips_and_leaves_every_bit():
    x, y = cifar_rows(2 * MB, seed=8)
    model = resnet8()
    step = TrainStep(model, optimizer="adam", lr=0.002, ema_decay=0.99, sam=SamConfig(0.05))
    step(x[:MB], y[:MB])
    assert not step.poll_skipped()
    before = C.model_state(model, step)
    nstat = len(moving_average_buffers(model))
    bad = x[MB:].clone()
    bad[2, 5, 5, 0] = float("nan")
    step(bad, y[MB:])
    assert step.poll_skipped() and step.skipped == 1 and math.isnan(step.last_sam_norm())
    after = C.model_state(model, step)
    # every parameter, copy, slot and shadow (the BN statistics took the forward's update, as in a skipped plain step)
    assert C.states_equal(before[:-nstat], after[:-nstat])
    assert step.global_step == 2 and step.opt.adam_step() == 1
    loss = float(step(x[:MB], y[:MB]))  # nothing lingers: training-mode BN reads the batch's statistics
    assert math.isfinite(loss) and not step.poll_skipped()
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert not C.same_bits(before[0], model_first(model))
    step.dp.close()


def model_first(model):
    return next(iter(model.parameters())).detach()


def test_sam_with_prune_and_bad_config_are_refused():
    with pytest.raises(ValueError):
        TrainStep(lenet(), sam=0.05)
    with pytest.raises(ValueError):
        TrainStep(lenet(), sam=SamConfig(0.05), prune=PruneConfig(0.5, 0.0, 0, 10, 1))
    step = TrainStep(lenet())
    assert step.samp is None and step.last_sam_norm() is None
    step.dp.close()


# ---- two ranks ---------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world):
    import torch.distributed as dist
    calls = [0]
    real = dist.all_reduce

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    dist.all_reduce = counting
    out = {}
    g = torch.Generator().manual_seed(100 + rank)  # a different batch on every rank
    xs = [torch.randn(4, 32, 32, 3, generator=g) * (1 + rank) for _ in range(2)]
    ys = [torch.randint(0, 10, (4,), generator=g) for _ in range(2)]
    for name, cfg in (("plain", None), ("sam", SamConfig(0.05))):
        torch.manual_seed(0)
        model = nets_factory.build("cifar10_resnet_v2", num_classes=10, resnet_size=8)
        step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, bucket_mb=0.05, sam=cfg)
        per_step = []
        for x, y in zip(xs, ys):
            calls[0] = 0
            step(x, y)
            per_step.append(calls[0])
        out[name] = {"calls": per_step, "buckets": len(step.dp.buckets),
                     "params": torch.cat([p.detach().reshape(-1) for p in model.parameters()]),
                     "stats": torch.cat([b.reshape(-1) for b in moving_average_buffers(model)]).clone(),
                     "norm": step.last_sam_norm() if cfg is not None else 0.0}
        step.dp.close()
    return out


def test_two_ranks_stay_identical_at_the_collectives_of_a_plain_step():
    res = run_workers(_two_rank_worker, 2)
    for name in ("plain", "sam"):
        assert C.same_bits(res[0][name]["params"], res[1][name]["params"]), name
        assert C.same_bits(res[0][name]["stats"], res[1][name]["stats"]), name
        assert bool(torch.isfinite(res[0][name]["params"]).all())
    for r in res:
        assert r["sam"]["calls"] == r["plain"]["calls"] == [r["plain"]["buckets"] + 1] * 2  # buckets + BN statistics
        assert r["plain"]["buckets"] > 1
    assert res[0]["sam"]["norm"] != res[1]["sam"]["norm"]  # the ascent gradient is rank-local
    assert not torch.equal(res[0]["sam"]["params"], res[0]["plain"]["params"])


# ---- the trainer ---------------------------------------------------------------------------------------------------
def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--synthetic_data", "--batch_size=8", "--data_dir=/nonexistent", "--seed=3", "--max_steps=2"]


@pytest.mark.parametrize("mod,args,message", [
    ("mnist_lenet_bsp", ["--sam_rho=0.05", "--sync_mode=asp"], "--sam_rho needs --sync_mode bsp"),
    ("mnist_lenet_bsp", ["--sam_rho=0.05", "--prune_sparsity=0.5"], "--sam_rho and --prune_sparsity"),
    ("mobilenet_v1_train", ["--sam_rho=0.05", "--quantize"], "--sam_rho and --quantize"),
    ("mnist_lenet_bsp", ["--sam_rho=-0.05"], "--sam_rho must be"),
    ("mnist_lenet_bsp", ["--sam_rho=nan"], "--sam_rho must be"),
], ids=["asp", "prune", "quantize", "negative", "nan"])
def test_trainer_refuses_at_start_up(tmp_path, mod, args, message):
    d = tmp_path / "train"
    p = _trainer(mod, "--train_dir=%s" % d, *(COMMON + args))
    assert p.returncode != 0
    assert "ValueError" in p.stderr and message in p.stderr, p.stderr[-2000:]
    assert not d.exists()  # refused before anything was set up


def test_trainer_runs_sam_and_logs_the_ascent_norm(tmp_path):
    import json
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + d, "--sam_rho=0.05", "--sam_adaptive", "--accum_steps=2",
                 "--metrics_file=" + mf, *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    recs = [json.loads(line) for line in open(mf)]
    assert [r["global_step"] for r in recs] == [1, 2]
    assert all(math.isfinite(r["loss"]) and r["sam_grad_norm"] > 0.0 for r in recs)
    assert np.isfinite([r["sam_grad_norm"] for r in recs]).all()
