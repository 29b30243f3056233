"""Knowledge distillation without a GPU: the torch-op composition of mean_xent_loss(..., distill=...) against an fp64
oracle (loss and student-logit gradients), alpha == 0 as the plain loss, the argument checks, TrainStep(distill=...)
with a frozen BatchNorm teacher, the soft signal at alpha == 1, and the trainer flags."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.ckpt.saver import model_variables
from distributed_tensorflow_models_amd.engine import DistillConfig, TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import mix
from distributed_tensorflow_models_amd.ops import nn as F
from distributed_tensorflow_models_amd.ops.nn import Distill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ---- the loss ---------------------------------------------------------------------------------------------------
def hard_rows_fp64(logits, labels, plan, smoothing):
    """-sum_k t_k log p_k per row in fp64; t the smoothed one-hot target, or a MixPlan's mix of two of them."""
    B, K = logits.shape
    on, off = 1.0 - smoothing + smoothing / K, smoothing / K
    hot = torch.nn.functional.one_hot(labels.long(), K).double()
    if plan is not None:
        w = torch.from_numpy(plan.w_lab.astype(np.float64)).view(B, 1)
        lb = labels.long()[torch.from_numpy(plan.partner.astype(np.int64))]
        hot = w * hot + (1 - w) * torch.nn.functional.one_hot(lb, K).double()
    t = off + (on - off) * hot
    return torch.logsumexp(logits, -1) - (t * logits).sum(-1)


def kl_rows_fp64(s, z, T):
    log_q = z / T - torch.logsumexp(z / T, -1, keepdim=True)
    log_p = s / T - torch.logsumexp(s / T, -1, keepdim=True)
    return (torch.softmax(z / T, -1) * (log_q - log_p)).sum(-1)


def distill_loss_fp64(main, aux, teacher, labels, plan, smoothing, a, T, aux_w):
    """The issue's definition on fp64 copies of the same fp32 values: the soft term on the main head only, the aux
    head's hard loss at its own weight, unscaled by 1 - a."""
    rows = (1 - a) * hard_rows_fp64(main, labels, plan, smoothing) + a * T * T * kl_rows_fp64(main, teacher, T)
    return rows.mean() + aux_w * hard_rows_fp64(aux, labels, plan, smoothing).mean()


def a_plan(B):
    """Identity rows, equal labels' partners, a weight of 0: the two-label cases of the mixed loss."""
    g = np.random.RandomState(B)
    w = g.uniform(0.0, 1.0, B).astype(np.float32)
    w[0], w[1] = 1.0, 0.0
    return mix.make_plan(list(g.permutation(B)), [1.0] * B, list(w), [[0, 0, 0, 0]] * B, 4, 4)


@pytest.mark.parametrize("a", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("T", [1.0, 4.0])
@pytest.mark.parametrize("K", [10, 1001])
def test_composition_against_the_fp64_oracle(K, T, a):
    """Tolerances: 1e-5 relative on the loss, the bound tests/test_mix_cpu.py sets for the mixed loss of the same fp32
    composition; the same 1e-5 (L2-relative) on the gradients, which the same fp32 ops produce (unit roundoff 6e-8,
    sums over at most 1001 terms)."""
    g = torch.Generator().manual_seed(K + int(10 * T))
    B = 16
    main, aux = torch.randn(B, K, generator=g) * 3, torch.randn(B, K, generator=g)
    teacher = torch.randn(B, K, generator=g) * 3
    labels = torch.randint(0, K, (B,), generator=g)
    for smoothing in (0.0, 0.1):
        for plan in (None, a_plan(B)):
            m32, a32 = main.clone().requires_grad_(), aux.clone().requires_grad_()
            t32 = teacher.clone().requires_grad_()
            got = F.mean_xent_loss([(m32, 1.0), (a32, 0.4)], labels, smoothing, mix=plan, distill=Distill(t32, a, T))
            got.backward()
            got = got.detach()
            m64, a64 = main.double().requires_grad_(), aux.double().requires_grad_()
            want = distill_loss_fp64(m64, a64, teacher.double(), labels, plan, smoothing, a, T, 0.4)
            want.backward()
            want = want.detach()
            what = (K, T, a, smoothing, plan is not None)
            assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), (what, float(got), float(want))
            assert _rel(m32.grad, m64.grad) < 1e-5, what
            assert _rel(a32.grad, a64.grad) < 1e-5, what
            assert t32.grad is None  # no gradient flows to the teacher
            kl = F.mean_xent_loss.kl_rows
            assert kl.dtype == torch.float32 and tuple(kl.shape) == (B,) and not kl.requires_grad
            assert _rel(kl, kl_rows_fp64(main.double(), teacher.double(), T)) < 1e-5, what


@pytest.mark.parametrize("with_plan", [False, True])
def test_alpha_zero_is_the_loss_without_distill(with_plan):
    g = torch.Generator().manual_seed(2)
    B, K = 16, 37
    main, aux = torch.randn(B, K, generator=g) * 3, torch.randn(B, K, generator=g)
    teacher = torch.randn(B, K, generator=g) * 3
    labels = torch.randint(0, K, (B,), generator=g)
    plan = a_plan(B) if with_plan else None
    for T in (1.0, 4.0):
        got = F.mean_xent_loss([(main, 1.0), (aux, 0.4)], labels, 0.1, mix=plan, distill=Distill(teacher, 0.0, T))
        assert torch.equal(got, F.mean_xent_loss([(main, 1.0), (aux, 0.4)], labels, 0.1, mix=plan))
    half = F.mean_xent_loss([(main, 1.0), (aux, 0.4)], labels, 0.1, mix=plan, distill=Distill(teacher, 0.5, 4.0))
    assert not torch.equal(half, got)


def test_argument_checks():
    z = torch.zeros(4, 10)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Distill(z, 0.5, bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            Distill(z, bad, 4.0)
    with pytest.raises(ValueError):
        Distill(torch.zeros(4), 0.5, 4.0)
    labels = torch.zeros(4, dtype=torch.long)
    for wrong in (torch.zeros(4, 11), torch.zeros(3, 10)):
        with pytest.raises(ValueError):
            F.mean_xent_loss([(z, 1.0)], labels, distill=Distill(wrong, 0.5, 4.0))
    with pytest.raises(ValueError):
        F.mean_xent_loss([(z, 1.0)], labels, distill=(z, 0.5, 4.0))
    net = nets_factory.build("lenet", 10)
    for kw in (dict(alpha=2.0), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            DistillConfig(net, **kw)
    with pytest.raises(ValueError):
        DistillConfig(None)
    with pytest.raises(ValueError):
        TrainStep(net, distill=DistillConfig(net))  # the student as its own teacher
    with pytest.raises(ValueError):
        TrainStep(net, distill=(net, 0.5, 4.0))


# ---- the step -----------------------------------------------------------------------------------------------------
def test_step_leaves_a_batchnorm_teacher_unchanged():
    """Student CifarNet, teacher the CIFAR ResNet v2 of size 8 (BatchNorm in every block), 32 x 32 batches of 8.  (LeNet
    takes 28 x 28 x 1 images only and no BatchNorm model of the zoo runs those, so the student here is the zoo's
    other small network for CIFAR-shaped input.)"""
    torch.manual_seed(0)
    student = nets_factory.build("cifarnet", 10, dropout_keep_prob=1.0)
    torch.manual_seed(1)
    teacher = nets_factory.build("cifar10_resnet_v2", 10, resnet_size=8)
    with torch.no_grad():  # moving statistics that an update would visibly move
        for i, b in enumerate(teacher.buffers()):
            if b.is_floating_point():
                b.add_(0.25 * (i % 3))
    assert any("moving" in n for n, _b in teacher.named_buffers())
    before = [t.detach().clone() for t in list(teacher.parameters()) + list(teacher.buffers())]
    step = TrainStep(student, optimizer="momentum", lr=0.05, momentum=0.9, ema_decay=0.99,
                     distill=DistillConfig(teacher, alpha=0.5, temperature=4.0))
    assert not any(p.requires_grad for p in teacher.parameters())
    g = torch.Generator().manual_seed(3)
    p0 = [p.detach().clone() for p in student.parameters()]
    for _ in range(3):
        loss = step(torch.randn(8, 32, 32, 3, generator=g), torch.randint(0, 10, (8,), generator=g))
        assert math.isfinite(float(loss)) and math.isfinite(step.last_distill_kl())
    after = list(teacher.parameters()) + list(teacher.buffers())
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
    assert all(p.grad is None for p in teacher.parameters())
    assert not all(torch.equal(a, b) for a, b in zip(p0, student.parameters()))  # the student did train
    teacher_ids = {id(t) for t in after}
    assert not any(id(p) in teacher_ids for p in step.opt.params)
    variables = model_variables(student, step.opt, torch.zeros((), dtype=torch.int64))
    assert not any(id(v.tensor) in teacher_ids for v in variables)
    assert not any(id(b) in teacher_ids for b in step.bufsync.buffers)
    step.dp.close()


def lenet(seed):
    torch.manual_seed(seed)
    return nets_factory.build("lenet", 10, dropout_keep_prob=1.0)


def soft_run(labels, steps=30):
    student, teacher = lenet(0), lenet(1)
    step = TrainStep(student, optimizer="momentum", lr=0.05, momentum=0.9, label_smoothing=0.1,
                     distill=DistillConfig(teacher, alpha=1.0, temperature=4.0))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(16, 28, 28, 1, generator=g)
    losses, kls = [], []
    for _ in range(steps):
        losses.append(step(x, labels))
        kls.append(step.last_distill_kl())
    step.dp.close()
    return losses, kls, [p.detach().clone() for p in student.parameters()]


def test_soft_signal_trains_the_student_and_ignores_the_labels():
    g = torch.Generator().manual_seed(6)
    labels = torch.randint(0, 10, (16,), generator=g)
    l0, kl0, p0 = soft_run(labels)
    assert kl0[-1] < 0.5 * kl0[0], (kl0[0], kl0[-1])
    # alpha == 1: loss == T^2 * mean KL, and the labels are unused
    assert float(l0[-1]) == pytest.approx(16.0 * kl0[-1], rel=1e-5)
    l1, kl1, p1 = soft_run(labels[torch.randperm(16, generator=g)])
    assert all(torch.equal(a, b) for a, b in zip(l0, l1)) and kl0 == kl1
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))


def test_step_without_distill_reports_no_kl():
    step = TrainStep(lenet(0), optimizer="sgd", lr=0.05)
    assert step.distill is None and step.last_distill_kl() is None
    step.dp.close()


def test_accumulation_runs_the_teacher_per_micro_batch():
    student, teacher = lenet(0), lenet(1)
    calls = []
    fwd = teacher.forward

    def counted(x, training=True):
        calls.append((tuple(x.shape), training, torch.is_grad_enabled()))
        return fwd(x, training=training)
    teacher.forward = counted
    step = TrainStep(student, optimizer="momentum", lr=0.05, accum_steps=2, distill=DistillConfig(teacher))
    g = torch.Generator().manual_seed(7)
    step(torch.randn(16, 28, 28, 1, generator=g), torch.randint(0, 10, (16,), generator=g))
    assert calls == [((8, 28, 28, 1), False, False)] * 2
    assert len(step._kl_rows) == 2 and math.isfinite(step.last_distill_kl())
    step.dp.close()


# ---- trainer ----------------------------------------------------------------------------------------------------
def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--synthetic_data", "--batch_size=8", "--data_dir=/nonexistent", "--seed=3"]


def test_trainer_distills_from_a_checkpoint(tmp_path):
    from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
    from distributed_tensorflow_models_amd.ckpt.saver import latest_checkpoint
    td, sd, mf = str(tmp_path / "teacher"), str(tmp_path / "student"), str(tmp_path / "metrics.jsonl")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + td, "--max_steps=3", *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    ck = latest_checkpoint(td)
    assert ck and ck.endswith("-3")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + sd, "--max_steps=3", "--distill_teacher=lenet",
                 "--distill_checkpoint=" + ck, "--metrics_file=" + mf, "--seed=4", *COMMON[:-1])
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    recs = [json.loads(line) for line in open(mf)]
    assert [r["global_step"] for r in recs] == [1, 2, 3]
    assert all(math.isfinite(r["distill_kl"]) and r["distill_kl"] > 0 and math.isfinite(r["loss"]) for r in recs)
    teacher_names, student_names = (set(BundleReader(c).names()) for c in (ck, latest_checkpoint(sd)))
    assert student_names == teacher_names  # the same model trained the same way: no variable more for the teacher
    assert not any("teacher" in n.lower() or "distill" in n.lower() for n in student_names)


def test_trainer_refuses_a_teacher_under_asp_or_without_a_checkpoint(tmp_path):
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "asp"), "--sync_mode=asp", "--max_steps=2",
                 "--distill_teacher=lenet", "--distill_checkpoint=%s" % (tmp_path / "none"), *COMMON)
    assert p.returncode != 0
    assert "ValueError" in p.stderr and "needs --sync_mode bsp" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "asp").exists()  # refused at start-up, before anything was set up
    for extra in ([], ["--distill_checkpoint=%s" % (tmp_path / "none" / "model.ckpt-3")]):
        p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "nockpt"), "--max_steps=2",
                     "--distill_teacher=lenet", *extra, *COMMON)
        assert p.returncode != 0
        assert "ValueError" in p.stderr and "needs --distill_checkpoint" in p.stderr, p.stderr[-2000:]
        assert not (tmp_path / "nockpt").exists()
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "alpha"), "--max_steps=2",
                 "--distill_teacher=lenet", "--distill_alpha=1.5", "--distill_checkpoint=%s" % (tmp_path / "none"),
                 *COMMON)
    assert p.returncode != 0 and "ValueError" in p.stderr and "--distill_alpha" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "alpha").exists()
