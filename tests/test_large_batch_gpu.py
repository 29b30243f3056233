"""The multi-tensor norm pass, LARS and clip-by-global-norm on the GPU against fp64 CPU oracles; the scaled entry point
with null pointers against dtm_multi_tensor_opt; the captured LARS step against the eager one; the NaN guard."""
import math

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.compat.train import LinearWarmup
from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops.optim import KINDS, FusedOptimizer

pytestmark = pytest.mark.gpu

# 11 parameters + one EMA-only row.  Row 4 (257) has a zero gradient, row 10 is an all-zero weight.
SHAPES = [(1,), (7,), (255,), (256,), (257,), (8191,), (8192,), (8193,), (3 * 8192 + 5,), (64, 37), (5, 3)]
WDS = [0.0, 1e-4, 0.0, 1e-4, 1e-4, 0.0, 1e-4, 0.0, 1e-4, 1e-4, 1e-4]
ZERO_GRAD, ZERO_WEIGHT = 4, 10
NOT_ADAPTED = (1, 6)  # the LARS flag is a per-tensor table entry: two rows are left out by the predicate
GRAD_SCALE, STEPS = 0.5, 3
EETA, EPS, MU, LR = 0.02, 1e-9, 0.9, 0.5


@pytest.fixture(scope="module")
def ref():
    """Initial weights and STEPS gradients (fp32, CPU), shared and never modified."""
    g = torch.Generator().manual_seed(11)
    w = [torch.randn(s, generator=g) * 0.3 for s in SHAPES]
    w[ZERO_WEIGHT] = torch.zeros(SHAPES[ZERO_WEIGHT])
    grads = []
    for _ in range(STEPS):
        gr = [torch.randn(s, generator=g) for s in SHAPES]
        gr[ZERO_GRAD] = torch.zeros(SHAPES[ZERO_GRAD])
        grads.append(gr)
    return {"w": w, "grads": grads, "buf": torch.randn(300, generator=g)}


def _setup(ref, kind, **kw):
    """Parameters on the GPU with gradients as views into ONE flat buffer packed back to back (bases at any element
    offset).  Even rows live in a packed weight buffer too (weight and gradient misaligned alike: 16-byte loads with a
    scalar head), odd rows in allocations of their own (offset against the gradient: the 4-byte path)."""
    dev = torch.device("cuda", 0)
    n = [int(np.prod(s)) for s in SHAPES]
    flat_g = torch.zeros(sum(n) + 3, device=dev)
    flat_w = torch.zeros(sum(n) + 3, device=dev)
    params, off = [], 1  # (the first base is already off the 16-byte grid)
    for i, s in enumerate(SHAPES):
        if i % 2 == 0:
            flat_w[off:off + n[i]].copy_(ref["w"][i].reshape(-1))
            p = torch.nn.Parameter(flat_w[off:off + n[i]].view(s))
        else:
            p = torch.nn.Parameter(ref["w"][i].to(dev))
        p.weight_decay = WDS[i]
        p.main_grad = flat_g[off:off + n[i]].view(s)
        p.row = i
        params.append(p)
        off += n[i]
    assert sum(p.main_grad.data_ptr() % 16 != 0 for p in params) >= 6
    buf = ref["buf"].to(dev)
    opt = FusedOptimizer(params, kind, lr=LR, momentum=MU, ema_decay=0.9, ema_buffers=[buf],
                         lars_skip=lambda p: p.row in NOT_ADAPTED, **kw)
    opt._hold = (flat_g, flat_w, buf)
    return params, opt


def _load_grads(params, grads):
    for p, g in zip(params, grads):
        p.main_grad.copy_(g)


def _oracle_norms(w, grads):
    """fp64 sums of fp32 terms formed as the kernel forms them: gs = g*s, ge = g*s + wd*p."""
    out = torch.zeros(len(SHAPES) + 1, 3, dtype=torch.float64)
    for i, (p, g) in enumerate(zip(w, grads)):
        gs = g * GRAD_SCALE
        ge = g * GRAD_SCALE + WDS[i] * p
        out[i] = torch.stack([p.double().square().sum(), gs.double().square().sum(), ge.double().square().sum()])
    return out  # squared; the last row (EMA-only) stays 0


def _oracle_ratios(sq):
    r = torch.ones(len(SHAPES) + 1, dtype=torch.float64)
    for i in range(len(SHAPES)):
        pn, gn = math.sqrt(sq[i, 0]), math.sqrt(sq[i, 1])
        if i not in NOT_ADAPTED and pn > 0 and gn > 0:
            r[i] = EETA * pn / (gn + WDS[i] * pn + EPS)
    return r


def test_norm_pass_matches_fp64_oracle(ref):
    sq = _oracle_norms(ref["w"], ref["grads"][0])
    want = sq.sqrt()
    ratios = _oracle_ratios(sq)
    total = math.sqrt(float(sq[:, 2].sum()))
    clip = total / 3.0
    exactly_one = sorted(set(NOT_ADAPTED) | {ZERO_GRAD, ZERO_WEIGHT, len(SHAPES)})
    for kind, kw in (("lars", dict(lars_eeta=EETA, lars_epsilon=EPS)), ("momentum", dict(clip_global_norm=clip))):
        params, opt = _setup(ref, kind, **kw)
        _load_grads(params, ref["grads"][0])
        opt.set_dynamic(LR, GRAD_SCALE)
        opt.launch_norms()
        first = opt.last_norms().clone()
        first_r, first_c = opt.last_lr_scale().clone(), opt._gclip.clone()
        opt.launch_norms()  # the same pass again: bit-identical
        torch.cuda.synchronize()
        assert torch.equal(first, opt.last_norms())
        assert torch.equal(first_r, opt.last_lr_scale()) and torch.equal(first_c, opt._gclip)
        got = first.cpu().double()
        print(kind, "max rel err of norms", float(((got - want).abs() / want.clamp_min(1e-30)).max()))
        torch.testing.assert_close(got, want, rtol=1e-5, atol=0.0)
        assert float(got[ZERO_WEIGHT, 0]) == 0.0 and float(got[ZERO_GRAD, 1]) == 0.0
        assert got[len(SHAPES)].tolist() == [0.0, 0.0, 0.0]  # the EMA-only row writes a zero record
        r, c = first_r.cpu().double(), float(first_c)
        if kind == "lars":
            torch.testing.assert_close(r, ratios, rtol=1e-5, atol=0.0)
            assert all(float(r[i]) == 1.0 for i in exactly_one)
            assert all(float(r[i]) != 1.0 for i in range(len(SHAPES)) if i not in exactly_one)
            assert c == 1.0
        else:
            assert bool((r == 1.0).all())
            assert c == pytest.approx(clip / max(total, clip), rel=1e-5) and c < 0.5
        # nothing but the outputs was written
        for p, w0 in zip(params, ref["w"]):
            assert torch.equal(p.detach().cpu(), w0)


def test_clip_off_below_threshold_is_exactly_one(ref):
    params, opt = _setup(ref, "sgd", clip_global_norm=1e6)
    _load_grads(params, ref["grads"][0])
    opt.set_dynamic(LR, GRAD_SCALE)
    opt.launch_norms()
    assert float(opt._gclip) == 1.0


def _oracle_run(ref, kind, clip=0.0):
    """STEPS steps in fp64 from the fp32 start: LARS, or momentum with the clip by global norm."""
    w = [t.double() for t in ref["w"]]
    acc = [torch.zeros_like(t) for t in w]
    for s in range(STEPS):
        gs = [g.double() * GRAD_SCALE for g in ref["grads"][s]]
        ge = [a + WDS[i] * w[i] for i, a in enumerate(gs)]
        gclip = 1.0
        if clip > 0:
            gclip = clip / max(math.sqrt(sum(float(e.square().sum()) for e in ge)), clip)
        for i in range(len(w)):
            r = 1.0
            pn, gn = float(w[i].norm()), float(gs[i].norm())
            if kind == "lars" and i not in NOT_ADAPTED and pn > 0 and gn > 0:
                r = EETA * pn / (gn + WDS[i] * pn + EPS)
            acc[i] = MU * acc[i] + ge[i] * gclip
            w[i] = w[i] - LR * r * acc[i]
    return w, acc


@pytest.mark.parametrize("kind", ["lars", "clip"])
def test_lars_and_clipped_updates_match_fp64_oracle(ref, kind):
    clip = 0.0
    if kind == "lars":
        params, opt = _setup(ref, "lars", lars_eeta=EETA, lars_epsilon=EPS)
    else:
        sq = _oracle_norms(ref["w"], ref["grads"][0])
        clip = math.sqrt(float(sq[:, 2].sum())) / 3.0  # active on every step (the gradients have one scale)
        params, opt = _setup(ref, "momentum", clip_global_norm=clip)
    for s in range(STEPS):
        _load_grads(params, ref["grads"][s])
        opt.step(LR, grad_scale=GRAD_SCALE)
        if kind == "clip":
            assert float(opt._gclip) < 0.6
    torch.cuda.synchronize()
    w, acc = _oracle_run(ref, "lars" if kind == "lars" else "momentum", clip)
    for i, p in enumerate(params):
        torch.testing.assert_close(p.detach().cpu().double(), w[i], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(opt.state[p]["s1"].cpu().double(), acc[i], rtol=1e-5, atol=1e-6)
    # the factors mattered: the plain momentum trajectory is elsewhere
    plain, _ = _oracle_run(ref, "momentum", 0.0)
    assert float((plain[9] - w[9]).abs().max()) > 1e-3


@pytest.mark.parametrize("kind", ["sgd", "momentum", "rmsprop"])
def test_scaled_entry_with_null_pointers_is_bit_identical(ref, kind):
    L = _lib.lib()
    out = []
    for scaled in (False, True):
        params, opt = _setup(ref, kind)
        assert not opt.scaled and opt.last_norms() is None
        for s in range(2):
            _load_grads(params, ref["grads"][s])
            if not scaled:
                opt.step(LR, grad_scale=GRAD_SCALE)
                continue
            opt.set_dynamic(LR, GRAD_SCALE)
            L.dtm_multi_tensor_opt_scaled(_lib.ptr(opt._tens_dev), _lib.ptr(opt._chunks_dev), opt._nchunks,
                                          KINDS[kind], 0.0, float(opt.mu), float(opt.rho), float(opt.eps), 1.0, 0.0,
                                          1, None, _lib.ptr(opt._dyn), None, None, _lib.stream_ptr())
            opt.num_updates += 1
        torch.cuda.synchronize()
        st = [opt.state[p] for p in params]
        out.append([p.detach().clone() for p in params] + [s_[k] for s_ in st for k in ("s1", "s2", "ema") if k in s_]
                   + [opt.buffer_ema[id(b)] for b in opt.ema_buffers])
    assert len(out[0]) == len(out[1]) > len(SHAPES)
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][0].cpu(), ref["w"][0])


def _run_steps(name, use_graph, steps, size, ncls, sched):
    """tests/test_engine.py's helper, for the LARS step."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    from distributed_tensorflow_models_amd.ops import elementwise as E
    E.seed_offset(dev).zero_()
    E.set_base_seed(1234)
    model = nets_factory.build(name, num_classes=ncls).to(dev)
    init = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
    step = TrainStep(model, optimizer="lars", lr=0.5, momentum=0.9, use_graph=use_graph, ema_decay=0.99,
                     lr_schedule=sched, lars_eeta=0.02, weight_decay=1e-4)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(4, size, size, 3, generator=g).to(dev, torch.bfloat16) for _ in range(2)]
    ys = [torch.randint(0, ncls, (4,), generator=g).to(dev) for _ in range(2)]
    losses = [float(step(xs[i % 2], ys[i % 2])) for i in range(steps)]
    torch.cuda.synchronize()
    params = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
    emas = torch.cat([step.opt.state[p]["ema"].reshape(-1) for p in step.opt.params])
    step.dp.close()
    return losses, params, emas, step, init


def test_hipgraph_lars_step_matches_eager():
    sched = LinearWarmup(lambda s: 0.5 * (0.5 ** (s // 4)), 3)
    le, pe, ee, se, init = _run_steps("cifar10_cnn", False, 6, 24, 10, sched)
    lg, pg_, eg, sg, _ = _run_steps("cifar10_cnn", True, 6, 24, 10, sched)
    assert sg._graph is not None and sg.global_step == 6 and sg.opt.num_updates == 6
    assert all(math.isfinite(v) for v in le)
    assert lg == pytest.approx(le, rel=2e-2, abs=2e-3)
    for a, b in ((pg_, pe), (eg, ee)):
        assert ((a - b).norm() / b.norm()).item() < 1e-3
    assert ((pe - init).norm() / init.norm()).item() > 1e-2  # LARS moved the weights (warm-up included)
    ne, ng = se.opt.last_norms().cpu(), sg.opt.last_norms().cpu()  # the captured norm pass wrote its outputs
    assert bool((ng[:len(sg.opt.params), 0] > 0).all()) and bool(torch.isfinite(ng).all())
    torch.testing.assert_close(ng[:, 0], ne[:, 0], rtol=1e-3, atol=1e-6)  # |p| of the step before: as the parameters
    rg = sg.opt.last_lr_scale().cpu()
    assert bool((rg != 1.0).any()) and bool((rg == 1.0).any())  # weights adapted, biases not


def test_nan_guard_under_lars():
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = nets_factory.build("cifar10_cnn", 10).to(dev)
    step = TrainStep(m, optimizer="lars", lr=0.5, lars_eeta=0.02, weight_decay=1e-4)
    x = torch.randn(4, 24, 24, 3, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 10, (4,), device=dev)
    step(x, y)
    assert not step.poll_skipped()
    before = [p.detach().clone() for p in m.parameters()]
    mom = [step.opt.state[p]["s1"].clone() for p in step.opt.params]
    x_bad = x.clone()
    x_bad[0, 5, 5, 0] = float("inf")
    step(x_bad, y)
    torch.cuda.synchronize()
    assert step.poll_skipped() and step.skipped == 1
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert all(torch.equal(a, step.opt.state[p]["s1"]) for a, p in zip(mom, step.opt.params))
    loss = float(step(x, y))  # the next finite step proceeds
    assert math.isfinite(loss) and not step.poll_skipped()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert bool(torch.isfinite(step.opt.last_norms()).all())
    step.dp.close()
