"""The LAMB cases shared by tests/test_lamb_cpu.py and tests/test_lamb_gpu.py: the tensor set and drivers of
tests/test_adam_cpu.py (chunk and 256-lane edges, EMA 0.9 with a drifting EMA-only buffer, seed 11) with one more row
of 65 * 8192 + 3 elements (more than 64 chunk rows: the finalize's lane stride wraps), rows 1 and 6 not adapted, row 4
with a zero gradient and no decay, row 10 an all-zero weight; and the fp64 oracle, which is the definition itself over
the fp32 inputs with t counted here:

    gs = g * grad_scale;  m = b1*m + (1-b1)*gs;  v = b2*v + (1-b2)*gs*gs
    r = (m / (1-b1^t)) / (sqrt(v) / sqrt(1-b2^t) + eps) + wd*p
    phi = |p| / |r| if the tensor is adapted and |p| > 0 and |r| > 0 else 1;   p -= lr * lr_mult * phi * r

Tolerances: p, m and the EMA shadows rtol=1e-5, atol=1e-6; v rtol=1e-5, atol=1e-12 (the Adam tests' own: a plain fp32
evaluation of the definition stays within a few per cent of them over the 5 steps); phi rtol=1e-5 (an fp32 evaluation
is within 4e-7 relative of the fp64 one)."""
import math

import torch

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops.optim import FusedOptimizer

SHAPES = [(1,), (7,), (255,), (256,), (257,), (8191,), (8192,), (8193,), (3 * 8192 + 5,), (64, 37), (5, 3),
          (65 * 8192 + 3,)]
WDS = [0.0, 1e-4, 0.0, 1e-4, 0.0, 0.0, 1e-4, 0.0, 1e-4, 1e-4, 1e-4, 1e-2]
LR_MULTS = {2: 0.5, 9: 2.0}
NOT_ADAPTED = (1, 6)
ZERO_GRAD, ZERO_WEIGHT = 4, 10
# rows whose trust ratio is a genuine |p| / |r|: adapted, non-zero weight, non-zero direction
RATIO_ROWS = [i for i in range(len(SHAPES)) if i not in NOT_ADAPTED + (ZERO_GRAD, ZERO_WEIGHT)]
GRAD_SCALE, STEPS, EMA = 0.5, 5, 0.9
LRS = [0.010, 0.012, 0.015, 0.011, 0.013]
BUF_DRIFT = 0.25  # the EMA-only buffer moves by this much before every step
CONFIGS = [(0.9, 0.999, 1e-6), (0.5, 0.9, 1e-3), (0.0, 0.999, 1e-6)]  # (beta1, beta2, epsilon)
CONFIG_IDS = ["default", "b.5_.9_eps1e-3", "b1_0"]
P_TOL = dict(rtol=1e-5, atol=1e-6)
V_TOL = dict(rtol=1e-5, atol=1e-12)
PHI_RTOL = 1e-5

_REF = {}


def make_ref():
    """Initial weights and STEPS gradients (fp32, CPU): made once, shared and never modified."""
    if not _REF:
        g = torch.Generator().manual_seed(11)
        w = [torch.randn(s, generator=g) * 0.3 for s in SHAPES]
        w[ZERO_WEIGHT] = torch.zeros(SHAPES[ZERO_WEIGHT])
        grads = []
        for _ in range(STEPS):
            gr = [torch.randn(s, generator=g) for s in SHAPES]
            gr[ZERO_GRAD] = torch.zeros(SHAPES[ZERO_GRAD])
            grads.append(gr)
        _REF.update(w=w, grads=grads, buf=torch.randn(300, generator=g))
    return _REF


_ORACLES = {}


def oracle(ref, cfg, steps, skipped=(), adapted=None, wds=None):
    """The definition in fp64.  ``steps`` host steps; those in ``skipped`` apply nothing and do not advance t.
    ``adapted``: the adapted rows (default: all but NOT_ADAPTED; () is AdamW).  The EMA decay follows the host's update
    count, as for every kind.  Also returns, per applied step, phi and the norms (|p|, |r|, |gs|) of every row."""
    key = (cfg, steps, tuple(skipped), None if adapted is None else tuple(adapted), None if wds is None else tuple(wds))
    if key in _ORACLES:
        return _ORACLES[key]
    b1, b2, eps = cfg
    wds = WDS if wds is None else wds
    if adapted is None:
        adapted = [i for i in range(len(SHAPES)) if i not in NOT_ADAPTED]
    w = [x.double() for x in ref["w"]]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    ema = [x.clone() for x in w]
    buf = ref["buf"].double().clone()
    buf_ema = buf.clone()
    t, phis, norms = 0, [], []
    for n in range(steps):
        buf = buf + BUF_DRIFT
        if n in skipped:
            continue
        t += 1
        d = min(EMA, (1.0 + n) / (10.0 + n))
        bc1, bc2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
        phi, nrm = [], []
        for i in range(len(w)):
            gs = ref["grads"][n][i].double() * GRAD_SCALE
            m[i] = b1 * m[i] + (1 - b1) * gs
            v[i] = b2 * v[i] + (1 - b2) * gs * gs
            r = (m[i] / bc1) / (v[i].sqrt() / bc2 + eps) + wds[i] * w[i]
            pn, rn = float(w[i].norm()), float(r.norm())
            f = pn / rn if (i in adapted and pn > 0.0 and rn > 0.0) else 1.0
            phi.append(f)
            nrm.append((pn, rn, float(gs.norm())))
            w[i] = w[i] - LRS[n] * LR_MULTS.get(i, 1.0) * f * r
            ema[i] = ema[i] - (1 - d) * (ema[i] - w[i])
        phis.append(phi)
        norms.append(nrm)
        buf_ema = buf_ema - (1 - d) * (buf_ema - buf)
    out = {"w": w, "m": m, "v": v, "ema": ema, "buf_ema": buf_ema, "t": t, "phi": phis, "norms": norms}
    _ORACLES[key] = out
    return out


def make_optimizer(params, buf, cfg, lars_skip=None, **kw):
    b1, b2, eps = cfg
    for i, p in enumerate(params):
        p.row = i
    if lars_skip is None:
        lars_skip = lambda p: p.row in NOT_ADAPTED  # noqa: E731
    return FusedOptimizer(params, "lamb", lr=LRS[0], beta1=b1, beta2=b2, epsilon=eps, ema_decay=EMA,
                          ema_buffers=[buf], lr_mults={params[i]: mult for i, mult in LR_MULTS.items()},
                          lars_skip=lars_skip, **kw)


def setup_cpu(ref, cfg, lars_skip=None, wds=None, **kw):
    params = []
    for i, w in enumerate(ref["w"]):
        p = torch.nn.Parameter(w.clone())
        p.weight_decay = (WDS if wds is None else wds)[i]
        p.main_grad = torch.zeros_like(w)
        p.bf16 = w.to(torch.bfloat16)
        params.append(p)
    buf = ref["buf"].clone()
    return params, buf, make_optimizer(params, buf, cfg, lars_skip, **kw)


def drive(params, buf, opt, ref, steps, skip_flags=None, first=0, after=None):
    """Optimizer steps ``first`` .. ``steps - 1`` on either device; skip_flags[n]: the step's skip flag tensor (or
    None).  Returns the per-step copies of ``last_lr_scale()`` (taken in stream order; no synchronisation)."""
    phis = []
    for n in range(first, steps):
        for p, g in zip(params, ref["grads"][n]):
            p.main_grad.copy_(g)
        buf.add_(BUF_DRIFT)
        opt.step(LRS[n], grad_scale=GRAD_SCALE, skip_flag=skip_flags[n] if skip_flags else None)
        phis.append(opt.last_lr_scale().clone())
        if after is not None:
            after(n)
    return phis


def check(params, buf, opt, want, ref, phis=None, bf16=True, fixed_rows=True):
    """State against the oracle; ``phis``: drive()'s copies of the APPLIED steps, against the oracle's per step."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0, "ema": 0.0, "phi": 0.0}
    for i, p in enumerate(params):
        st = opt.state[p]
        got = {"p": p.detach().cpu().double(), "m": st["s1"].cpu().double(), "v": st["s2"].cpu().double(),
               "ema": st["ema"].cpu().double()}
        for k, e in (("p", want["w"][i]), ("m", want["m"][i]), ("v", want["v"][i]), ("ema", want["ema"][i])):
            tol = V_TOL if k == "v" else P_TOL
            err = ((got[k] - e).abs() / (tol["atol"] + tol["rtol"] * e.abs())).max()
            worst[k] = max(worst[k], float(err))
    if phis is not None:
        assert len(phis) == len(want["phi"])
        for got, exp in zip(phis, want["phi"]):
            got, exp = got.cpu().double()[:len(params)], torch.tensor(exp, dtype=torch.float64)
            worst["phi"] = max(worst["phi"], float(((got - exp).abs() / (PHI_RTOL * exp.abs())).max()))
    print("worst error as a fraction of the tolerance:", worst)
    for i, p in enumerate(params):
        st = opt.state[p]
        torch.testing.assert_close(p.detach().cpu().double(), want["w"][i], **P_TOL)
        torch.testing.assert_close(st["s1"].cpu().double(), want["m"][i], **P_TOL)
        torch.testing.assert_close(st["s2"].cpu().double(), want["v"][i], **V_TOL)
        torch.testing.assert_close(st["ema"].cpu().double(), want["ema"][i], **P_TOL)
        if bf16:
            assert torch.equal(p.bf16.cpu().view(torch.int16), p.detach().cpu().bfloat16().view(torch.int16))
    torch.testing.assert_close(opt.buffer_ema[id(buf)].cpu().double(), want["buf_ema"], **P_TOL)
    if phis is not None:
        for got, exp in zip(phis, want["phi"]):
            torch.testing.assert_close(got.cpu().double()[:len(params)], torch.tensor(exp, dtype=torch.float64),
                                       rtol=PHI_RTOL, atol=0.0)
            assert float(got[len(params):].cpu().sub(1.0).abs().max()) == 0.0  # the EMA-only row
    if fixed_rows:
        # zero gradient, zero decay: bit-unchanged; the all-zero weight moved
        assert torch.equal(params[ZERO_GRAD].detach().cpu(), ref["w"][ZERO_GRAD])
        assert float(params[ZERO_WEIGHT].detach().abs().min()) > 0.0


# ---- the step on LeNet ---------------------------------------------------------------------------------------------
def lenet_batches(dev, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 28, 28, 1, generator=g).to(dev, dtype)
    y = torch.randint(0, 10, (4,), generator=g).to(dev)
    return x, y


def nan_guard_through_train_step(dev, dtype=torch.float32):
    """A NaN batch on the second of three steps: nothing moves, and adam_step() lags global_step by one."""
    torch.manual_seed(0)
    m = nets_factory.build("lenet", 10).to(dev)
    step = TrainStep(m, optimizer="lamb", lr=0.002, ema_decay=0.99, weight_decay=1e-4)
    keys = [(p, k) for p in step.opt.params for k in ("s1", "s2", "ema")]
    x, y = lenet_batches(dev, dtype)
    step(x, y)
    assert not step.poll_skipped() and step.opt.adam_step() == 1
    before = [p.detach().clone() for p in m.parameters()]
    slots = [step.opt.state[p][k].clone() for p, k in keys]
    phi = step.opt.last_lr_scale().clone()
    assert float(phi.sub(1.0).abs().max()) > 0.0
    x_bad = x.clone()
    x_bad[0, 5, 5, 0] = float("nan")
    step(x_bad, y)
    assert step.poll_skipped() and step.skipped == 1
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert all(torch.equal(a, step.opt.state[p][k]) for a, (p, k) in zip(slots, keys))
    assert torch.equal(phi, step.opt.last_lr_scale())
    assert step.global_step == 2 and step.opt.adam_step() == 1
    loss = float(step(x, y))
    assert math.isfinite(loss) and not step.poll_skipped()
    assert step.global_step == 3 and step.opt.adam_step() == 2
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    step.dp.close()
