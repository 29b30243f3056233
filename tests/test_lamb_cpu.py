"""Fused LAMB on CPU against the fp64 oracle of tests/lamb_cases.py (tensor set, drivers and tolerances are explained
there): the update and the per-step trust ratios, the defaults and refusals, the rows with a known outcome, the
decoupled decay, the AdamW limit, skipped updates that do not count, the checkpoint round trip (also from an Adam run),
the tf.train facade and the trainer's flags.  tests/test_lamb_gpu.py runs the same cases on the GPU."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.ckpt.saver import Saver, model_variables
from distributed_tensorflow_models_amd.compat import train as T
from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops.optim import KINDS, FusedOptimizer
from lamb_cases import (CONFIG_IDS, CONFIGS, NOT_ADAPTED, RATIO_ROWS, SHAPES, STEPS, WDS, ZERO_GRAD, ZERO_WEIGHT, check,
                        drive, lenet_batches, make_ref, nan_guard_through_train_step, oracle, setup_cpu)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."


@pytest.fixture(scope="module")
def ref():
    return make_ref()


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_update_matches_fp64_oracle(ref, cfg):
    params, buf, opt = setup_cpu(ref, cfg)
    phis = drive(params, buf, opt, ref, STEPS)
    assert opt.adam_step() == STEPS == opt.num_updates
    check(params, buf, opt, oracle(ref, cfg, STEPS), ref, phis)


def test_kind_defaults_and_refusals(ref):
    assert KINDS["lamb"] == 4 and KINDS["adam"] == 3
    params, buf, opt = setup_cpu(ref, (0.9, 0.999, None))
    assert opt.eps == 1e-6 and opt.b1 == 0.9 and opt.b2 == 0.999
    assert all(float(opt.state[p]["s1"].abs().max()) == 0.0 == float(opt.state[p]["s2"].abs().max()) for p in params)
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError):
        FusedOptimizer([p], "lamb", beta2=1.0)
    with pytest.raises(ValueError):
        FusedOptimizer([p], "lamb", clip_global_norm=1.0)
    # the default predicate: tensors of rank <= 1 are not adapted
    q = torch.nn.Parameter(torch.ones(3, 2))
    o = FusedOptimizer([p, q], "lamb")
    assert [o.state[x]["adapt"] for x in (p, q)] == [False, True]


def test_fixed_rows(ref):
    params, buf, opt = setup_cpu(ref, CONFIGS[0])
    phis = drive(params, buf, opt, ref, 2)
    assert torch.equal(params[ZERO_GRAD].detach(), ref["w"][ZERO_GRAD])  # bit-unchanged
    assert float(params[ZERO_WEIGHT].detach().abs().min()) > 0.0  # moved ...
    assert float(phis[0][ZERO_WEIGHT]) == 1.0  # ... at phi = 1 on its first step (|p| = 0)
    for phi in phis:
        assert all(float(phi[i]) == 1.0 for i in NOT_ADAPTED + (ZERO_GRAD,))
        # every adapted row with a weight and a direction has a ratio of its own
        assert all(float(phi[i]) != 1.0 for i in RATIO_ROWS)
    assert float(phis[1][ZERO_WEIGHT]) != 1.0  # the weight is no longer zero on the second step
    ns = opt.norm_stats()
    assert set(ns) == {"grad_norm", "update_norm", "lamb/min_trust_ratio", "lamb/max_trust_ratio"}
    adapted = [i for i in range(len(SHAPES)) if i not in NOT_ADAPTED]
    assert ns["lamb/min_trust_ratio"] == float(phis[1][adapted].min())
    assert ns["lamb/max_trust_ratio"] == float(phis[1][adapted].max())
    want = oracle(ref, CONFIGS[0], 2)["norms"][1]
    assert ns["grad_norm"] == pytest.approx(math.sqrt(sum(g * g for _, _, g in want)), rel=1e-5)
    assert ns["update_norm"] == pytest.approx(math.sqrt(sum(r * r for _, r, _ in want)), rel=1e-5)


def test_decay_is_decoupled(ref):
    params, buf, opt = setup_cpu(ref, CONFIGS[0])
    drive(params, buf, opt, ref, 3)
    params0, buf0, opt0 = setup_cpu(ref, CONFIGS[0], wds=[0.0] * len(WDS))
    drive(params0, buf0, opt0, ref, 3)
    for i, (p, p0) in enumerate(zip(params, params0)):
        assert torch.equal(opt.state[p]["s1"], opt0.state[p0]["s1"])  # m and v never see the decay
        assert torch.equal(opt.state[p]["s2"], opt0.state[p0]["s2"])
        if WDS[i] > 0.0 and i != ZERO_WEIGHT:
            assert not torch.equal(p.detach(), p0.detach())


def test_no_adapted_tensor_is_adamw(ref):
    cfg = CONFIGS[0]
    params, buf, opt = setup_cpu(ref, cfg, lars_skip=lambda p: True)
    phis = drive(params, buf, opt, ref, STEPS)
    assert all(float(phi.sub(1.0).abs().max()) == 0.0 for phi in phis)
    want = oracle(ref, cfg, STEPS, adapted=())  # AdamW in fp64: decoupled decay, no trust ratio
    assert all(f == 1.0 for phi in want["phi"] for f in phi)
    check(params, buf, opt, want, ref, phis)
    assert "lamb/min_trust_ratio" not in opt.norm_stats()


def test_skipped_update_does_not_count(ref):
    cfg = CONFIGS[0]
    params, buf, opt = setup_cpu(ref, cfg)
    flags = [torch.tensor([1 if n == 1 else 0], dtype=torch.int32) for n in range(4)]
    phis = drive(params, buf, opt, ref, 4, flags)
    assert opt.adam_step() == 3 and opt.num_updates == 4
    assert torch.equal(phis[1], phis[0])  # the skipped step left the ratios alone
    want = oracle(ref, cfg, 4, skipped=(1,))
    assert want["t"] == 3
    check(params, buf, opt, want, ref, [phis[0], phis[2], phis[3]])
    # counting the skipped step would have been seen: t = 2, 3, 4 on the last three steps
    counted = oracle(ref, cfg, 4, skipped=())
    assert max(float((a - b).abs().max()) for a, b in zip(counted["w"], want["w"])) > 1e-3


def test_nan_guard_under_lamb():
    nan_guard_through_train_step(torch.device("cpu"))


# ---- checkpoints -------------------------------------------------------------------------------------------------
def _lenet_step(seed=0, optimizer="lamb"):
    torch.manual_seed(seed)
    model = nets_factory.build("lenet", 10, dropout_keep_prob=1.0)
    step = TrainStep(model, optimizer=optimizer, lr=0.002, ema_decay=0.99, weight_decay=1e-4)
    gstep = torch.zeros((), dtype=torch.int64)
    return model, step, gstep, model_variables(model, step.opt, gstep)


def _state(model, step):
    return [p.detach().clone() for p in model.parameters()] + \
        [step.opt.state[p][k].clone() for p in step.opt.params for k in ("s1", "s2", "ema")]


def _resume(ck, optimizer="lamb"):
    model2, step2, gstep2, vars2 = _lenet_step(seed=1, optimizer=optimizer)  # everything comes from the file
    Saver(vars2).restore(ck)
    step2.global_step = int(gstep2)
    step2.opt.restored(int(gstep2))
    return model2, step2


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

    model2, step2 = _resume(ck)
    assert step2.opt.adam_step() == 3 and step2.opt.num_updates == 3
    step2(x, y)
    assert all(torch.equal(a, b) for a, b in zip(want, _state(model2, step2)))  # bit for bit the 4th step
    step2.dp.close()


def test_adam_checkpoint_restores_into_lamb(tmp_path):
    x, y = lenet_batches(torch.device("cpu"))
    model, step, gstep, vars_ = _lenet_step(optimizer="adam")
    for _ in range(3):
        step(x, y)
    gstep.fill_(step.global_step)
    ck = Saver(vars_).save(str(tmp_path / "model.ckpt"), global_step=gstep)
    model2, step2 = _resume(ck)
    assert step2.opt.kind == "lamb" and step2.opt.adam_step() == 3 and step2.opt.num_updates == 3
    assert all(torch.equal(a, b) for a, b in zip(_state(model, step), _state(model2, step2)))
    assert math.isfinite(float(step2(x, y))) and step2.opt.adam_step() == 4
    step.dp.close()
    step2.dp.close()


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
def test_lamb_optimizer_record():
    assert T.LAMBOptimizer().config() == dict(optimizer="lamb", lr=0.001, beta1=0.9, beta2=0.999, epsilon=1e-6)
    o = T.LAMBOptimizer(0.002, beta1=0.8, beta2=0.99, epsilon=1e-5, weight_decay=0.01)
    assert o.kind == "lamb"
    torch.manual_seed(0)
    model = nets_factory.build("lenet", 10)
    op = o.minimize(lambda out, y: None, model, T.get_or_create_global_step())
    opt = op.step.opt
    assert isinstance(opt, FusedOptimizer) and opt.kind == "lamb"
    assert (opt.b1, opt.b2, opt.eps, op.step.lr) == (0.8, 0.99, 1e-5, 0.002)
    assert all(opt.state[p]["wd"] == 0.01 for p in opt.params)  # one coefficient for every variable, as LARSOptimizer
    assert {v.name for v in op.variables()} >= {"beta1_power", "beta2_power", "LeNet/conv1/weights/Adam",
                                                 "LeNet/conv1/weights/Adam_1"}
    op.close()


def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--synthetic_data", "--batch_size=8", "--data_dir=/nonexistent", "--seed=3"]


def test_trainer_lamb_run_logs_the_ratios_and_writes_the_slots(tmp_path):
    from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
    from distributed_tensorflow_models_amd.ckpt.saver import latest_checkpoint
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + d, "--max_steps=3", "--optimizer=lamb", "--adam_beta1=0.8",
                 "--lamb_epsilon=1e-5", "--initial_learning_rate=0.002", "--metrics_file=" + mf, *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    rows = [json.loads(l) for l in open(mf)]
    assert [(r["global_step"], r["adam_step"]) for r in rows] == [(1, 1), (2, 2), (3, 3)]
    for r in rows:
        assert all(math.isfinite(r[k]) for k in ("loss", "grad_norm", "update_norm", "lamb/min_trust_ratio",
                                                  "lamb/max_trust_ratio"))
        assert 0.0 < r["lamb/min_trust_ratio"] <= r["lamb/max_trust_ratio"] and r["update_norm"] > 0.0
    ck = latest_checkpoint(d)
    assert ck.endswith("-3")
    r = BundleReader(ck)
    names = r.names()
    assert len([n for n in names if n.endswith("/Adam")]) == 8 == len([n for n in names if n.endswith("/Adam_1")])
    assert all(np.abs(np.asarray(r.get_tensor(n))).max() > 0 for n in names if n.endswith(("/Adam", "/Adam_1")))
    assert np.asarray(r.get_tensor("beta1_power")) == np.float32(0.8 ** 4)
    assert np.asarray(r.get_tensor("beta2_power")) == np.float32(0.999 ** 4)
    r.close()


def test_trainer_refuses_lamb_under_asp_and_with_clipping(tmp_path):
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "asp"), "--sync_mode=asp", "--max_steps=2",
                 "--optimizer=lamb", *COMMON)
    assert p.returncode != 0
    assert "ValueError" in p.stderr and "--optimizer lamb needs --sync_mode bsp" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "asp").exists()  # refused at start-up, before anything was set up
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "clip"), "--max_steps=2", "--optimizer=lamb",
                 "--clip_global_norm=1", *COMMON)
    assert p.returncode != 0
    assert "ValueError" in p.stderr and "--optimizer lamb and --clip_global_norm are not combined" in p.stderr, \
        p.stderr[-2000:]
    assert not (tmp_path / "clip").exists()
