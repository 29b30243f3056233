"""Knowledge distillation on the GPU: dtm_softmax_xent_distill against an fp64 oracle and, at alpha == 0, against the
bits of the plain and the mixed kernel; its argument checks; the fused mean_xent_loss(..., distill=...) against the
torch-op composition; TrainStep(distill=...) eager and captured, with accumulation and with mixing; the frozen teacher;
the NaN guard on a non-finite teacher."""
import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.engine import DistillConfig, TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops import nn as F
from distributed_tensorflow_models_amd.ops.mix import MixConfig, sample_plan
from distributed_tensorflow_models_amd.ops.nn import Distill
from test_mix_gpu import BOTH, _bits, _rel, deterministic, run_xent, xent_case  # noqa: F401 (deterministic: a fixture)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
KS = [10, 257, 1001]
DTYPES = [torch.float32, torch.bfloat16]


# ---- the kernel ---------------------------------------------------------------------------------------------------
def distill_case(K, dtype):
    """test_mix_gpu.xent_case (student rows at pitch K + 5, its labels and plan) and an independent teacher block at
    pitch K + 3, both randn * 3: the KL is O(1) and a relative error means something."""
    buf, labels, plan, ld = xent_case(K, dtype)
    g = torch.Generator().manual_seed(1000 + K)
    tbuf = (torch.randn(8, K + 3, generator=g) * 3).to(dtype)
    return buf, tbuf, labels, plan, ld, K + 3


def run_distill(buf, tbuf, labels, plan, K, ld, ldt, smoothing, alpha, T, gscale, mixed, want_kl=True):
    """One launch with guard values of 7 before and after loss, kl and dlogits (the check of run_xent)."""
    B = buf.shape[0]
    L, s = _lib.lib(), _lib.stream_ptr()
    lg, tz, lab = buf.to(DEV), tbuf.to(DEV), labels.to(DEV)
    loss = torch.full((B + 2,), 7.0, device=DEV)
    kl = torch.full((B + 2,), 7.0, device=DEV)
    dl = torch.full((B * K + 16,), 7.0, device=DEV).to(buf.dtype)
    pd = plan.to(DEV) if mixed else None
    rc = L.dtm_softmax_xent_distill(_lib.ptr(lg), int(buf.dtype == torch.bfloat16), _lib.ptr(tz), ldt, _lib.ptr(lab),
                                    _lib.ptr(pd.dev) if mixed else None, _lib.ptr(loss[1:]),
                                    _lib.ptr(kl[1:]) if want_kl else None, _lib.ptr(dl[8:]), B, K, smoothing, alpha, T,
                                    gscale, ld, s)
    assert rc == 0
    torch.cuda.synchronize()
    for v in (loss, kl):
        assert float(v[0]) == 7.0 and float(v[-1]) == 7.0
    if not want_kl:
        assert bool((kl == 7.0).all())
    assert bool((dl[:8].float() == 7.0).all()) and bool((dl[8 + B * K:].float() == 7.0).all())
    return loss[1:1 + B].cpu(), kl[1:1 + B].cpu(), dl[8:8 + B * K].view(B, K).cpu()


def oracle(buf, tbuf, labels, plan, K, smoothing, alpha, T, gscale, mixed):
    """fp64 on the stored values; an out-of-range label contributes nothing to the target."""
    x, z = buf[:, :K].double(), tbuf[:, :K].double()
    on, off = 1.0 - smoothing + smoothing / K, smoothing / K
    ks = torch.arange(K).view(1, K)
    la = labels.long()
    hot = (ks == la.view(-1, 1)).double()
    if mixed:
        lb = la[torch.from_numpy(plan.partner.astype(np.int64))]
        w = torch.from_numpy(plan.w_lab.astype(np.float64)).view(-1, 1)
        hot = w * hot + (1 - w) * (ks == lb.view(-1, 1)).double()
    t = off + (on - off) * hot
    hard = torch.logsumexp(x, -1) - (t * x).sum(-1)
    q, pT = torch.softmax(z / T, -1), torch.softmax(x / T, -1)
    kl = (q * (torch.log_softmax(z / T, -1) - torch.log_softmax(x / T, -1))).sum(-1)
    loss = (1 - alpha) * hard + alpha * T * T * kl
    dl = gscale * ((1 - alpha) * (torch.softmax(x, -1) - t) + alpha * T * (pT - q))
    return loss, kl, dl


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", KS)
def test_kernel_against_the_fp64_oracle(K, dtype):
    smoothing, gscale = 0.1, 0.125
    buf, tbuf, labels, plan, ld, ldt = distill_case(K, dtype)
    for T in (1.0, 4.0):
        for alpha in (0.5, 1.0):
            for mixed in (False, True):
                loss, kl, dl = run_distill(buf, tbuf, labels, plan, K, ld, ldt, smoothing, alpha, T, gscale, mixed)
                want_loss, want_kl, want_dl = oracle(buf, tbuf, labels, plan, K, smoothing, alpha, T, gscale, mixed)
                errs = (_rel(loss, want_loss), _rel(kl, want_kl), _rel(dl, want_dl))
                what = "K %d %s T %g alpha %g mixed %s: loss %.3g kl %.3g grad %.3g" % (
                    (K, str(dtype)[6:], T, alpha, mixed) + errs)
                print(what)
                assert float(want_kl.min()) > 0.05, what  # O(1): the relative error means something
                assert errs[0] < 1e-4 and errs[1] < 1e-4, what
                assert errs[2] < (1e-4 if dtype == torch.float32 else 1e-2), what
    # kl is optional: without it the same loss and gradient, and nothing written there
    loss2, _kl, dl2 = run_distill(buf, tbuf, labels, plan, K, ld, ldt, smoothing, 1.0, 4.0, gscale, True,
                                  want_kl=False)
    assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(dl2), _bits(dl))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("K", KS)
def test_alpha_zero_gives_the_bits_of_the_plain_and_the_mixed_kernel(K, dtype):
    smoothing, gscale = 0.1, 0.125
    buf, tbuf, labels, plan, ld, ldt = distill_case(K, dtype)
    for mixed in (False, True):
        want_loss, want_dl = run_xent(buf, labels, plan, K, ld, smoothing, gscale, mixed)
        for T in (1.0, 4.0):
            loss, kl, dl = run_distill(buf, tbuf, labels, plan, K, ld, ldt, smoothing, 0.0, T, gscale, mixed)
            assert torch.equal(_bits(loss), _bits(want_loss)), (mixed, T)
            assert torch.equal(_bits(dl), _bits(want_dl)), (mixed, T)
            assert bool(torch.isfinite(kl).all()) and float(kl.min()) > 0


def test_kernel_refuses_bad_arguments():
    B, K = 4, 10
    x, z = torch.zeros(B, K, device=DEV), torch.zeros(B, K, device=DEV)
    lab = torch.zeros(B, dtype=torch.int32, device=DEV)
    loss, dl = torch.ones(B, device=DEV), torch.ones(B, K, device=DEV)
    L, s = _lib.lib(), _lib.stream_ptr()

    def call(B=B, K=K, alpha=0.5, T=4.0, teacher=z):
        return L.dtm_softmax_xent_distill(_lib.ptr(x), 0, _lib.ptr(teacher) if teacher is not None else None, K,
                                          _lib.ptr(lab), None, _lib.ptr(loss), None, _lib.ptr(dl), B, K, 0.0, alpha, T,
                                          1.0, K, s)
    assert call(T=0.0) < 0 and call(T=-1.0) < 0 and call(T=float("nan")) < 0
    assert call(alpha=1.5) < 0 and call(alpha=-0.1) < 0 and call(alpha=float("nan")) < 0
    assert call(B=65536) < 0 and call(B=0) < 0 and call(K=0) < 0 and call(teacher=None) < 0
    torch.cuda.synchronize()
    assert bool((loss == 1).all()) and bool((dl == 1).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((loss != 1).all())


# ---- the fused loss -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
def test_mean_xent_loss_distill_fused_matches_composition(mixed):
    """As test_mean_xent_loss_mixed_fused_matches_composition: two heads at [64, 1001] bf16 from two FC producers; the
    fused op (teacher and plan on the device; the teacher a padded view, read in place) against the torch-op
    composition (the same teacher values on the host, the plan without a device record)."""
    torch.manual_seed(13)
    B, Kin, N = 64, 128, 1001
    x = torch.randn(B, Kin, device=DEV).to(torch.bfloat16)
    labels = torch.randint(0, N, (B,), device=DEV)
    ws = [torch.nn.Parameter(torch.randn(Kin, N, device=DEV) / Kin ** 0.5) for _ in range(2)]
    tpad = (torch.randn(B, 1008, device=DEV) * 2).to(torch.bfloat16)
    teacher = tpad[:, :N]
    host = sample_plan(MixConfig(**dict(BOTH, prob=0.7), per_row=True, seed=5), 0, 0, 0, B, 8, 8) if mixed else None
    out = []
    for fused in (True, False):
        for w in ws:
            w.grad = None
        xi = x.clone().requires_grad_()
        la, lb = F.linear(xi, ws[0], None), F.linear(xi * 2, ws[1], None)
        plan = (host.to(DEV) if fused else host) if mixed else None
        tz = teacher if fused else teacher.cpu()
        before = F._MeanXentDistillFn.kl_rows
        loss = F.mean_xent_loss([(la, 1.0), (lb, 0.4)], labels, 0.1, mix=plan, distill=Distill(tz, 0.5, 4.0))
        assert (F._MeanXentDistillFn.kl_rows is not before) == fused  # which path ran
        kl = F.mean_xent_loss.kl_rows
        assert kl.dtype == torch.float32 and tuple(kl.shape) == (B,)
        loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.detach()), xi.grad.float(), [w.grad.clone() for w in ws], kl.clone()))
    (l1, gx1, gw1, kl1), (l2, gx2, gw2, kl2) = out
    assert abs(l1 - l2) <= 1e-5 * abs(l2), (l1, l2)
    assert _rel(kl1, kl2) < 1e-4
    assert _rel(gx1, gx2) < 1e-2
    for a, b in zip(gw1, gw2):
        assert _rel(a, b) < 1e-2
    plain = float(F.mean_xent_loss([(la.detach(), 1.0), (lb.detach(), 0.4)], labels, 0.1, mix=plan))
    assert abs(plain - l1) > 1e-3 * abs(l1)  # the soft term did change the loss
    with pytest.raises(ValueError):
        F.mean_xent_loss([(la.detach(), 1.0)], labels, 0.1, distill=Distill(tpad, 0.5, 4.0))  # [64, 1008]


# ---- the step -----------------------------------------------------------------------------------------------------
MB = 16


def lenet(seed):
    torch.manual_seed(seed)
    return nets_factory.build("lenet", 10, dropout_keep_prob=1.0).to(DEV)


def batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(MB, 28, 28, 1, generator=g).to(DEV, torch.bfloat16),
             torch.randint(0, 10, (MB,), generator=g).to(DEV)) for _ in range(n)]


def teacher_state(teacher):
    ts = list(teacher.parameters()) + list(teacher.buffers())
    return ts + [p.bf16 for p in teacher.parameters() if getattr(p, "bf16", None) is not None]


def run_steps(steps, graph=False, accum=1, mix=None, alpha=0.5, distill=True, poison=False):
    model, teacher = lenet(0), lenet(1)
    kw = {}
    if distill:
        kw["distill"] = DistillConfig(teacher, alpha=alpha, temperature=4.0)
    elif distill is None:
        kw["distill"] = None
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, label_smoothing=0.1, ema_decay=0.99,
                     accum_steps=accum, mix=mix, use_graph=graph, **kw)
    if poison:  # one weight of the teacher's logits layer: every row's teacher logits hold a NaN
        w = [p for p in teacher.parameters() if p.dim() == 2][-1]
        with torch.no_grad():
            w[0, 3] = float("nan")
        F.invalidate_weight_copies(teacher.parameters())
    torch.cuda.synchronize()
    before = [t.detach().clone() for t in teacher_state(teacher)]
    assert not distill or len(before) > len(list(teacher.parameters()))  # the compute copies exist and are compared
    data = batches(steps * accum)
    losses, kls = [], []
    for s in range(steps):
        xs, ys = (list(v) for v in zip(*data[s * accum:(s + 1) * accum]))
        losses.append(float(step(xs, ys) if accum > 1 else step(xs[0], ys[0])))
        kls.append(step.last_distill_kl())
    torch.cuda.synchronize()
    assert (step._graph is not None) == graph and step.global_step == steps
    after = teacher_state(teacher)
    assert len(after) == len(before)
    for a, b in zip(before, after):  # bit-unchanged (a NaN weight included)
        assert torch.equal(_bits(a), _bits(b)) if a.is_floating_point() else torch.equal(a, b)
    assert not any(p.requires_grad for p in teacher.parameters()) or not distill
    step.dp.close()
    return losses, [p.detach().clone() for p in model.parameters()], kls, step


@pytest.mark.parametrize("accum,mixed", [(1, False), (2, False), (1, True)], ids=["plain", "accum2", "mix"])
def test_captured_step_matches_eager(deterministic, accum, mixed):
    """Two eager warm-up steps, the capture and three replays against six eager steps; the teacher (parameters, buffers
    and bf16 compute copies) is bit-unchanged in both runs (asserted in run_steps)."""
    cfg = MixConfig(**BOTH, seed=4) if mixed else None
    le, pe, ke, _ = run_steps(6, accum=accum, mix=cfg)
    lg, pg_, kg, _ = run_steps(6, graph=True, accum=accum, mix=cfg)
    assert le == lg, (le, lg)
    assert ke == kg and all(k is not None and np.isfinite(k) and k > 0 for k in ke), (ke, kg)
    assert len(set(ke)) == 6  # a live value, not a frozen one
    assert all(torch.equal(a, b) for a, b in zip(pe, pg_))
    plain = run_steps(6, accum=accum, mix=cfg, distill=False)[1]
    assert not all(torch.equal(a, b) for a, b in zip(pe, plain))  # and the teacher did steer the student


def test_without_distill_the_step_is_the_plain_step(deterministic):
    l0, p0, k0, s0 = run_steps(3, distill=False)     # the argument left out
    l1, p1, k1, s1 = run_steps(3, distill=None)      # distill=None
    assert l0 == l1 and k0 == k1 == [None] * 3 and s1.distill is None and s1._kl_rows == []
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    # alpha == 0: the teacher runs and the new kernel computes the loss, with the plain step's bits
    l2, p2, k2, _ = run_steps(3, alpha=0.0)
    assert l0 == l2 and all(k is not None and k > 0 for k in k2)
    assert all(torch.equal(a, b) for a, b in zip(p0, p2))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_a_nan_in_the_teacher_is_skipped_by_the_guard(deterministic, graph):
    model0 = [p.detach().clone() for p in lenet(0).parameters()]
    steps = 3 if graph else 1  # (captured: two eager warm-up steps and the capture's first replay)
    losses, params, kls, step = run_steps(steps, graph=graph, poison=True)
    assert step.poll_skipped() and step.skipped == steps
    assert all(l != l for l in losses) and all(k != k for k in kls)
    assert all(torch.equal(a, b) for a, b in zip(model0, params))  # the student is bit-unchanged
