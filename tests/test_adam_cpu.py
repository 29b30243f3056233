"""Fused Adam on CPU against an fp64 oracle written here (the three lines of the definition over the fp32 gradient
values, with t counted by the test): the update, skipped updates that do not count, the checkpoint round trip with
beta1_power / beta2_power, the tf.train facade and the trainer's flags.  tests/test_adam_gpu.py runs the same tensor
set, oracle and drivers on the GPU.

Tolerances: p, m (and the EMA shadows, which are averages of p) rtol=1e-5, atol=1e-6; v rtol=1e-5, atol=1e-12.  A
plain fp32 evaluation of the formula stays within a few per cent of them over 5 steps at these settings; a t off by
one moves p by about 1e-3."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.ckpt.saver import AdamPowerVar, Saver, model_variables
from distributed_tensorflow_models_amd.compat import train as T
from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops.optim import KINDS, FusedOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."

# The tensor set of tests/test_large_batch_gpu.py (chunk and 256-lane edges): 11 parameters + one EMA-only row.  Row 4
# has a zero gradient and, here, no decay (the update must leave it bit-unchanged); row 10 is an all-zero weight.
SHAPES = [(1,), (7,), (255,), (256,), (257,), (8191,), (8192,), (8193,), (3 * 8192 + 5,), (64, 37), (5, 3)]
WDS = [0.0, 1e-4, 0.0, 1e-4, 0.0, 0.0, 1e-4, 0.0, 1e-4, 1e-4, 1e-4]
LR_MULTS = {2: 0.5, 9: 2.0}
ZERO_GRAD, ZERO_WEIGHT = 4, 10
GRAD_SCALE, STEPS, EMA = 0.5, 5, 0.9
LRS = [0.010, 0.012, 0.015, 0.011, 0.013]
BUF_DRIFT = 0.25  # the EMA-only buffer moves by this much before every step
CONFIGS = [(0.9, 0.999, 1e-8), (0.5, 0.9, 1e-3), (0.0, 0.999, 1e-8)]  # (beta1, beta2, epsilon)
P_TOL = dict(rtol=1e-5, atol=1e-6)
V_TOL = dict(rtol=1e-5, atol=1e-12)


def make_ref():
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


@pytest.fixture(scope="module")
def ref():
    return make_ref()


def first_step_norm(ref):
    """Global norm of the first step's effective gradient (fp64 sums of the fp32 terms)."""
    tot = 0.0
    for i, (p, g) in enumerate(zip(ref["w"], ref["grads"][0])):
        tot += float((g * GRAD_SCALE + WDS[i] * p).double().square().sum())
    return math.sqrt(tot)


def oracle(ref, cfg, clip, steps, skipped=()):
    """The definition in fp64.  ``steps`` host steps; those in ``skipped`` apply nothing and do not advance t.  The
    EMA decay follows the host's update count (min(EMA, (1+n)/(10+n)) with n = host steps so far), as for every kind."""
    b1, b2, eps = cfg
    w = [x.double() for x in ref["w"]]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    ema = [x.clone() for x in w]
    buf = ref["buf"].double().clone()
    buf_ema = buf.clone()
    t = 0
    for n in range(steps):
        buf = buf + BUF_DRIFT
        if n in skipped:
            continue
        t += 1
        d = min(EMA, (1.0 + n) / (10.0 + n))
        g = [ref["grads"][n][i].double() * GRAD_SCALE + WDS[i] * w[i] for i in range(len(w))]
        if clip:
            f = clip / max(math.sqrt(sum(float(x.square().sum()) for x in g)), clip)
            g = [x * f for x in g]
        for i in range(len(w)):
            m[i] = b1 * m[i] + (1 - b1) * g[i]
            v[i] = b2 * v[i] + (1 - b2) * g[i] * g[i]
            lr = LRS[n] * LR_MULTS.get(i, 1.0)
            w[i] = w[i] - lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m[i] / (v[i].sqrt() + eps)
            ema[i] = ema[i] - (1 - d) * (ema[i] - w[i])
        buf_ema = buf_ema - (1 - d) * (buf_ema - buf)
    return {"w": w, "m": m, "v": v, "ema": ema, "buf_ema": buf_ema, "t": t}


def make_optimizer(params, buf, cfg, clip):
    b1, b2, eps = cfg
    return FusedOptimizer(params, "adam", lr=LRS[0], beta1=b1, beta2=b2, epsilon=eps, ema_decay=EMA,
                          ema_buffers=[buf], lr_mults={params[i]: mult for i, mult in LR_MULTS.items()},
                          clip_global_norm=clip)


def setup_cpu(ref, cfg, clip=None):
    params = []
    for i, w in enumerate(ref["w"]):
        p = torch.nn.Parameter(w.clone())
        p.weight_decay = WDS[i]
        p.main_grad = torch.zeros_like(w)
        p.bf16 = w.to(torch.bfloat16)
        params.append(p)
    buf = ref["buf"].clone()
    return params, buf, make_optimizer(params, buf, cfg, clip)


def drive(params, buf, opt, ref, steps, skip_flags=None):
    """``steps`` optimizer steps on either device; skip_flags[n]: the step's skip flag tensor (or None)."""
    for n in range(steps):
        for p, g in zip(params, ref["grads"][n]):
            p.main_grad.copy_(g)
        buf.add_(BUF_DRIFT)
        opt.step(LRS[n], grad_scale=GRAD_SCALE, skip_flag=skip_flags[n] if skip_flags else None)


def check(params, buf, opt, want, ref):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, p in enumerate(params):
        st = opt.state[p]
        got = {"p": p.detach().cpu().double(), "m": st["s1"].cpu().double(), "v": st["s2"].cpu().double()}
        for k, e in (("p", want["w"][i]), ("m", want["m"][i]), ("v", want["v"][i])):
            tol = V_TOL if k == "v" else P_TOL
            err = ((got[k] - e).abs() / (tol["atol"] + tol["rtol"] * e.abs())).max()
            worst[k] = max(worst[k], float(err))
    print("worst error as a fraction of the tolerance:", worst)
    for i, p in enumerate(params):
        st = opt.state[p]
        torch.testing.assert_close(p.detach().cpu().double(), want["w"][i], **P_TOL)
        torch.testing.assert_close(st["s1"].cpu().double(), want["m"][i], **P_TOL)
        torch.testing.assert_close(st["s2"].cpu().double(), want["v"][i], **V_TOL)
        torch.testing.assert_close(st["ema"].cpu().double(), want["ema"][i], **P_TOL)
        assert torch.equal(p.bf16.cpu().view(torch.int16), p.detach().cpu().bfloat16().view(torch.int16))
    torch.testing.assert_close(opt.buffer_ema[id(buf)].cpu().double(), want["buf_ema"], **P_TOL)
    # zero gradient, zero decay: bit-unchanged; the all-zero weight moved
    assert torch.equal(params[ZERO_GRAD].detach().cpu(), ref["w"][ZERO_GRAD])
    assert float(params[ZERO_WEIGHT].detach().abs().min()) > 0.0


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "b.5_.9_eps1e-3", "b1_0"])
def test_update_matches_fp64_oracle(ref, cfg, clip):
    clip = first_step_norm(ref) / 3.0 if clip else None
    params, buf, opt = setup_cpu(ref, cfg, clip)
    drive(params, buf, opt, ref, STEPS)
    if clip:
        assert float(opt._gclip) < 0.6  # the clip was active
    assert opt.adam_step() == STEPS == opt.num_updates
    check(params, buf, opt, oracle(ref, cfg, clip, STEPS), ref)


def test_kind_and_epsilon_defaults(ref):
    assert KINDS["adam"] == 3
    params, buf, opt = setup_cpu(ref, (0.9, 0.999, None))
    assert opt.eps == 1e-8 and opt.b1 == 0.9 and opt.b2 == 0.999
    assert all(float(opt.state[p]["s1"].abs().max()) == 0.0 == float(opt.state[p]["s2"].abs().max()) for p in params)
    p = torch.nn.Parameter(torch.zeros(3))
    assert FusedOptimizer([p], "rmsprop").eps == 1e-10 and FusedOptimizer([p], "momentum").eps == 1e-10
    FusedOptimizer([p], "adam", lars_eeta=0.5, lars_epsilon=0.1)  # LARS-only arguments: no effect, as for momentum
    with pytest.raises(ValueError):
        FusedOptimizer([p], "adam", beta2=1.0)
    with pytest.raises(ValueError):
        FusedOptimizer([p], "adamw")


def test_skipped_update_does_not_count(ref):
    cfg = CONFIGS[0]
    params, buf, opt = setup_cpu(ref, cfg)
    flags = [torch.tensor([1 if n == 1 else 0], dtype=torch.int32) for n in range(4)]
    drive(params, buf, opt, ref, 4, flags)
    assert opt.adam_step() == 3 and opt.num_updates == 4
    want = oracle(ref, cfg, None, 4, skipped=(1,))
    assert want["t"] == 3
    check(params, buf, opt, want, ref)
    # counting the skipped step would have been seen: t = 2, 3, 4 on the last three steps
    counted = oracle(ref, cfg, None, 4, skipped=())
    assert float((counted["w"][9] - want["w"][9]).abs().max()) > 1e-3


def lenet_batches(dev, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 28, 28, 1, generator=g).to(dev, dtype)
    y = torch.randint(0, 10, (4,), generator=g).to(dev)
    return x, y


def nan_guard_through_train_step(dev, dtype=torch.float32):
    """A NaN batch on the second of three steps: nothing moves, and adam_step() lags global_step by one."""
    torch.manual_seed(0)
    m = nets_factory.build("lenet", 10).to(dev)
    step = TrainStep(m, optimizer="adam", lr=0.002, ema_decay=0.99)
    x, y = lenet_batches(dev, dtype)
    step(x, y)
    assert not step.poll_skipped() and step.opt.adam_step() == 1
    before = [p.detach().clone() for p in m.parameters()]
    slots = [step.opt.state[p][k].clone() for p in step.opt.params for k in ("s1", "s2", "ema")]
    x_bad = x.clone()
    x_bad[0, 5, 5, 0] = float("nan")
    step(x_bad, y)
    assert step.poll_skipped() and step.skipped == 1
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert all(torch.equal(a, step.opt.state[p][k]) for a, (p, k) in
               zip(slots, [(p, k) for p in step.opt.params for k in ("s1", "s2", "ema")]))
    assert step.global_step == 2 and step.opt.adam_step() == 1
    loss = float(step(x, y))
    assert math.isfinite(loss) and not step.poll_skipped()
    assert step.global_step == 3 and step.opt.adam_step() == 2
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    step.dp.close()


def test_nan_guard_under_adam():
    nan_guard_through_train_step(torch.device("cpu"))


# ---- checkpoints -------------------------------------------------------------------------------------------------
def _lenet_step(seed=0):
    torch.manual_seed(seed)
    model = nets_factory.build("lenet", 10, dropout_keep_prob=1.0)
    step = TrainStep(model, optimizer="adam", lr=0.002, ema_decay=0.99, weight_decay=1e-4)
    gstep = torch.zeros((), dtype=torch.int64)
    return model, step, gstep, model_variables(model, step.opt, gstep)


def _state(model, step):
    return [p.detach().clone() for p in model.parameters()] + \
        [step.opt.state[p][k].clone() for p in step.opt.params for k in ("s1", "s2", "ema")]


def test_checkpoint_round_trip(tmp_path):
    from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
    x, y = lenet_batches(torch.device("cpu"))
    model, step, gstep, vars_ = _lenet_step()
    for _ in range(3):
        step(x, y)
    gstep.fill_(step.global_step)
    ck = Saver(vars_).save(str(tmp_path / "model.ckpt"), global_step=gstep)
    step(x, y)  # the uninterrupted 4th step
    want = _state(model, step)
    step.dp.close()

    r = BundleReader(ck)
    names = set(r.names())
    weights = [v.name for v in model_variables(model)]
    assert len(weights) == 8
    assert all(w + "/Adam" in names and w + "/Adam_1" in names for w in weights)
    b1p, b2p = np.asarray(r.get_tensor("beta1_power")), np.asarray(r.get_tensor("beta2_power"))
    assert b1p.dtype == np.float32 and b1p.shape == () and b1p == np.float32(0.9 ** 4)
    assert b2p.dtype == np.float32 and b2p.shape == () and b2p == np.float32(0.999 ** 4)
    assert np.abs(np.asarray(r.get_tensor(weights[0] + "/Adam_1"))).max() > 0
    r.close()

    def resume(drop=(), gs_override=None):
        model2, step2, gstep2, vars2 = _lenet_step(seed=1)  # other initial values: everything comes from the file
        vars2 = [v for v in vars2 if not (isinstance(v, AdamPowerVar) and v.name in drop)]
        Saver(vars2).restore(ck)
        step2.global_step = int(gstep2)
        step2.opt.restored(int(gstep2) if gs_override is None else gs_override)
        return model2, step2

    model2, step2 = resume()
    assert step2.opt.adam_step() == 3 and step2.opt.num_updates == 3
    step2(x, y)
    assert all(torch.equal(a, b) for a, b in zip(want, _state(model2, step2)))  # bit for bit the 4th step
    step2.dp.close()
    # t comes from beta2_power, then beta1_power, then global_step
    for drop, gs, t in (((), 7, 3), (("beta2_power",), 7, 3), (("beta1_power", "beta2_power"), 3, 3),
                        (("beta1_power", "beta2_power"), 7, 7)):
        _, s = resume(drop, gs)
        assert s.opt.adam_step() == t, (drop, gs)
        s.dp.close()


def test_slot_variable_names(ref):
    params, buf, opt = setup_cpu(ref, CONFIGS[0])
    for i, p in enumerate(params[:2]):
        p.tf_name = "v%d" % i
    drive(params, buf, opt, ref, 2)
    slots = opt.slot_variables()
    assert [n for n, _ in slots] == ["v0/Adam", "v0/Adam_1", "v0/ExponentialMovingAverage", "v1/Adam", "v1/Adam_1",
                                     "v1/ExponentialMovingAverage", "beta1_power", "beta2_power"]
    assert slots[0][1] is opt.state[params[0]]["s1"] and slots[1][1] is opt.state[params[0]]["s2"]
    assert float(slots[-2][1]) == np.float32(0.9 ** 3) and float(slots[-1][1]) == np.float32(0.999 ** 3)


# ---- facade and flags ----------------------------------------------------------------------------------------------
def test_adam_optimizer_record():
    assert T.AdamOptimizer().config() == dict(optimizer="adam", lr=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8)
    o = T.AdamOptimizer(0.002, beta1=0.8, beta2=0.99, epsilon=1e-6)
    assert o.kind == "adam"
    torch.manual_seed(0)
    model = nets_factory.build("lenet", 10)
    op = o.minimize(lambda out, y: None, model, T.get_or_create_global_step())
    opt = op.step.opt
    assert isinstance(opt, FusedOptimizer) and opt.kind == "adam"
    assert (opt.b1, opt.b2, opt.eps, op.step.lr) == (0.8, 0.99, 1e-6, 0.002)
    assert {v.name for v in op.variables()} >= {"beta1_power", "beta2_power", "LeNet/conv1/weights/Adam",
                                                 "LeNet/conv1/weights/Adam_1"}
    op.close()


def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--synthetic_data", "--batch_size=8", "--data_dir=/nonexistent", "--seed=3"]


def test_trainer_adam_run_writes_the_slots(tmp_path):
    from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
    from distributed_tensorflow_models_amd.ckpt.saver import latest_checkpoint
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + d, "--max_steps=3", "--optimizer=adam", "--adam_beta1=0.8",
                 "--initial_learning_rate=0.002", "--metrics_file=" + mf, *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    rows = [json.loads(l) for l in open(mf)]
    assert [(r["global_step"], r["adam_step"]) for r in rows] == [(1, 1), (2, 2), (3, 3)]
    assert all(math.isfinite(r["loss"]) for r in rows)
    ck = latest_checkpoint(d)
    assert ck.endswith("-3")
    r = BundleReader(ck)
    names = r.names()
    assert len([n for n in names if n.endswith("/Adam")]) == 8 == len([n for n in names if n.endswith("/Adam_1")])
    assert all(np.abs(np.asarray(r.get_tensor(n))).max() > 0 for n in names if n.endswith(("/Adam", "/Adam_1")))
    assert np.asarray(r.get_tensor("beta1_power")) == np.float32(0.8 ** 4)
    assert np.asarray(r.get_tensor("beta2_power")) == np.float32(0.999 ** 4)
    r.close()


def test_trainer_refuses_adam_under_asp_and_unknown_optimizers(tmp_path):
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "asp"), "--sync_mode=asp", "--max_steps=2",
                 "--optimizer=adam", *COMMON)
    assert p.returncode != 0
    assert "ValueError" in p.stderr and "--optimizer adam needs --sync_mode bsp" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "asp").exists()  # refused at start-up, before anything was set up
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "w"), "--max_steps=2", "--optimizer=adamw", *COMMON)
    assert p.returncode != 0
    assert "--optimizer must be sgd, momentum, rmsprop, lars or adam, got 'adamw'" in p.stderr, p.stderr[-2000:]
