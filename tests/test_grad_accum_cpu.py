"""Gradient accumulation on the CPU path: TrainStep(accum_steps=N) sums the gradients of N micro-batches in order,
applies one update, counts one step; the three accumulate modes as torch ops; BN statistics and collective counts
over two gloo ranks; the trainer's --accum_steps."""
import copy
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as TF

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import accum
from distributed_tensorflow_models_amd.ops import elementwise as E
from distributed_tensorflow_models_amd.utils.testing import run_workers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."
N, MB = 4, 8  # micro-batches per step, rows per micro-batch


def lenet(keep=1.0, dev="cpu"):
    torch.manual_seed(0)
    return nets_factory.build("lenet", 10, dropout_keep_prob=keep).to(dev)


def rows(n=N * MB, dev="cpu", dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, 28, 28, 1, generator=g).to(dev, dtype), torch.randint(0, 10, (n,), generator=g).to(dev)


def params_of(model):
    return [p.detach().clone() for p in model.parameters()]


def micro_gradients(xs, ys, dev="cpu", **kw):
    """The flat gradient of every micro-batch from a separate zero-grad / forward / loss / backward pass on the
    initial weights (a twin model and a TrainStep without accumulation, closed afterwards)."""
    twin = lenet(dev=dev)
    st = TrainStep(twin, optimizer="sgd", lr=0.5, weight_decay=0.0, **kw)
    out = []
    for x, y in zip(xs, ys):
        st._forward_backward(x, y)
        out.append(st.dp.flat.clone())
    st.dp.close()
    return out


def ordered_sum(gs):
    s = gs[0].clone()
    for g in gs[1:]:
        s = s + g
    return s


def test_accum_modes_as_torch_ops():
    g0 = torch.randn(37)
    g0[5] = -0.0
    for mode in (accum.STORE, accum.ADD, accum.FOLD):
        acc, g, flag = torch.full((41,), 2.0), torch.zeros(41), torch.zeros(3, dtype=torch.int32)
        g[2:39] = g0
        accum.grad_accum(acc[2:39], g[2:39], mode, flag[1:2])
        assert flag.tolist() == [0, 0, 0]
        want_acc = {accum.STORE: g0, accum.ADD: 2.0 + g0, accum.FOLD: torch.full((37,), 2.0)}[mode]
        want_g = 2.0 + g0 if mode == accum.FOLD else torch.zeros(37)
        assert torch.equal(acc[2:39], want_acc) and torch.equal(g[2:39], want_g)
        assert torch.equal(acc[:2], torch.full((2,), 2.0)) and torch.equal(acc[39:], torch.full((2,), 2.0))
        assert not g[:2].any() and not g[39:].any()
        bad = torch.randn(9)
        bad[3] = float("inf")
        accum.grad_accum(torch.zeros(9), bad, mode, flag[1:2])
        assert flag.tolist() == [0, 1, 0]
        accum.grad_accum(torch.zeros(9), torch.ones(9), mode, None)
    with pytest.raises(ValueError):
        accum.grad_accum(torch.zeros(4), torch.zeros(4), 3)
    with pytest.raises(ValueError):
        accum.grad_accum(torch.zeros(4), torch.zeros(5), 0)


def test_step_applies_the_ordered_sum_of_the_micro_gradients():
    x, y = rows()
    xs, ys = list(x.split(MB)), list(y.split(MB))
    gs = micro_gradients(xs, ys)
    assert not torch.equal(gs[0], gs[1])
    model = lenet()
    before = params_of(model)
    lr = 0.5
    step = TrainStep(model, optimizer="sgd", lr=lr, weight_decay=0.0, accum_steps=N)
    loss = step(xs, ys)
    want = ordered_sum(gs)  # ((g0 + g1) + g2) + g3
    assert torch.equal(step.dp.flat, want)
    assert step.dp.grad_scale == 0.25 and step.nonfinite_micro() == [0] * N
    for p, p0 in zip(model.parameters(), before):
        off = step.dp.offsets[p]
        g = want[off:off + p.numel()].view(p.shape) * 0.25 + 0.0 * p0
        assert torch.equal(p.detach(), p0 - lr * g)
    # the loss is the fp32 mean of the micro-batch losses in order
    twin = lenet()
    ls = [step.loss_fn(twin(a, training=True), b).detach() for a, b in zip(xs, ys)]
    assert torch.equal(loss, (((ls[0] + ls[1]) + ls[2]) + ls[3]) / N) and loss.dtype == torch.float32
    step.dp.close()


def lenet_fp64_gradient(model, x, y):
    """LeNet's mean cross-entropy gradient in fp64 torch ops: {parameter name: gradient}, and the loss."""
    p = {n: v.detach().double().requires_grad_(True) for n, v in model.named_parameters()}
    layers = ("conv1", "conv2", "fc3", "fc4")
    assert sorted(p) == sorted("%s.%s" % (m, k) for m in layers for k in ("weights", "biases"))
    h = x.double().permute(0, 3, 1, 2)
    for c in ("conv1", "conv2"):  # weights [K][R][S][C], 5x5 SAME
        h = torch.relu(TF.conv2d(h, p[c + ".weights"].permute(0, 3, 1, 2), p[c + ".biases"], padding=2))
        h = TF.max_pool2d(h, 2)
    h = h.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    h = torch.relu(h @ p["fc3.weights"] + p["fc3.biases"])
    loss = TF.cross_entropy(h @ p["fc4.weights"] + p["fc4.biases"], y)
    loss.backward()
    return {n: v.grad for n, v in p.items()}, float(loss.detach())


def test_accumulated_step_tracks_the_big_batch_step():
    """One step at batch 32 against a step of 4 micro-batches of 8 on the same rows, both against p - lr * g64 with
    g64 the batch-32 gradient recomputed in fp64.  The bound is 4 x the error of the existing batch-32 step: each of
    the 3 extra partial sums adds at most one rounding of the running sum, the fourth unit covers the changed order
    of the row sum.  Measured (lr 1.0, max abs error over all parameters): batch-32 step 5.80e-06, accumulated step
    7.71e-06."""
    x, y = rows()
    lr = 1.0  # the update's error is then the gradient's error plus one rounding of the difference
    big_m, acc_m = lenet(), lenet()
    g64, loss64 = lenet_fp64_gradient(big_m, x, y)
    want = {n: v.detach().double() - lr * g64[n] for n, v in big_m.named_parameters()}
    big = TrainStep(big_m, optimizer="sgd", lr=lr, weight_decay=0.0)
    loss_big = float(big(x, y))
    big.dp.close()
    acc = TrainStep(acc_m, optimizer="sgd", lr=lr, weight_decay=0.0, accum_steps=N)
    loss_acc = float(acc(x, y))
    acc.dp.close()
    assert loss_big == pytest.approx(loss64, rel=1e-5) and loss_acc == pytest.approx(loss64, rel=1e-5)
    e_big = max(float((v.detach().double() - want[n]).abs().max()) for n, v in big_m.named_parameters())
    e_acc = max(float((v.detach().double() - want[n]).abs().max()) for n, v in acc_m.named_parameters())
    print("max abs error of the update: batch-32 step %.3e, accumulated step %.3e" % (e_big, e_acc))
    assert e_big > 0.0
    assert e_acc <= 4 * e_big


def test_counters_advance_once_per_step():
    x, y = rows()
    model = lenet()
    step = TrainStep(model, optimizer="adam", lr=0.002, ema_decay=0.99, accum_steps=N)
    for i in range(3):
        step(x, y)
        assert (step.global_step, step.opt.num_updates, step.opt.adam_step()) == (i + 1, i + 1, i + 1)
    step.dp.close()


def test_dropout_masks_differ_between_micro_batches():
    x, y = rows(MB)
    E.set_base_seed(7)
    twin = lenet(keep=0.5)
    st = TrainStep(twin, optimizer="sgd", lr=0.5)
    st._forward_backward(x, y)
    g0 = st.dp.flat.clone()
    st.dp.close()
    E.set_base_seed(7)
    model = lenet(keep=0.5)
    step = TrainStep(model, optimizer="sgd", lr=0.5, accum_steps=2)
    step([x, x], [y, y])
    assert torch.equal(step.dp.acc, g0)  # the first micro-batch drew the twin's mask ...
    assert not torch.equal(step.dp.flat, g0 + g0)  # ... and the second one another
    step.dp.close()


def test_nonfinite_micro_batch_skips_the_whole_step():
    x, y = rows(3 * MB)
    model = lenet()
    step = TrainStep(model, optimizer="adam", lr=0.002, ema_decay=0.99, accum_steps=3)
    step(x, y)
    assert not step.poll_skipped() and step.nonfinite_micro() == [0, 0, 0]
    before = params_of(model)
    keys = [(p, k) for p in step.opt.params for k in ("s1", "s2", "ema")]
    slots = [step.opt.state[p][k].clone() for p, k in keys]
    bad = x.clone()
    bad[MB + 2, 5, 5, 0] = float("nan")  # a row of micro-batch 1
    step(bad, y)
    assert step.nonfinite_micro() == [0, 1, 0]
    assert step.poll_skipped() and step.skipped == 1
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(torch.equal(a, step.opt.state[p][k]) for a, (p, k) in zip(slots, keys))
    assert step.global_step == 2 and step.opt.adam_step() == 1
    loss = float(step(x, y))  # mode 0 overwrites the accumulator: nothing lingers
    assert math.isfinite(loss) and not step.poll_skipped() and step.nonfinite_micro() == [0, 0, 0]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    step.dp.close()


def test_input_forms_and_errors():
    x, y = rows()
    runs = []
    for as_list in (False, True):
        model = lenet()
        step = TrainStep(model, optimizer="momentum", lr=0.05, accum_steps=N)
        with pytest.raises(ValueError):
            step(x[:30], y[:30])
        with pytest.raises(ValueError):
            step(list(x.split(MB))[:3], list(y.split(MB))[:3])
        losses = [float(step(list(x.split(MB)), tuple(y.split(MB))) if as_list else step(x, y)) for _ in range(2)]
        runs.append((losses, params_of(model)))
        step.dp.close()
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    with pytest.raises(ValueError):
        TrainStep(lenet(), accum_steps=0)
    # accum_steps=1 is today's step
    runs = []
    for kw in ({}, {"accum_steps": 1}):
        E.set_base_seed(3)
        model = lenet(keep=0.5)
        step = TrainStep(model, optimizer="momentum", lr=0.05, ema_decay=0.99, **kw)
        losses = [float(step(x, y)) for _ in range(3)]
        runs.append((losses, params_of(model), step.dp.acc, step.dp.grad_scale))
        step.dp.close()
    assert runs[0][0] == runs[1][0] and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert runs[1][2] is None and runs[1][3] == 1.0  # no accumulator was allocated


def _bn_accum_worker(rank, world, n):
    from distributed_tensorflow_models_amd.engine import moving_average_buffers, moving_average_decays
    torch.manual_seed(0)
    model = nets_factory.build("cifar10_resnet_v2", num_classes=10, resnet_size=8)
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, bucket_mb=0.05, accum_steps=n)
    g = torch.Generator().manual_seed(100 + rank)  # a different batch on every rank
    xs = [torch.randn(4, 32, 32, 3, generator=g) * (1 + rank) for _ in range(n)]
    ys = [torch.randint(0, 10, (4,), generator=g) for _ in range(n)]
    cat = lambda m: torch.cat([b.reshape(-1) for b in moving_average_buffers(m)]).clone()  # noqa: E731
    init = cat(model)
    shadow = copy.deepcopy(model)  # this replica's n local updates alone (the weights do not move inside a step)
    with torch.no_grad():
        for x in xs:
            shadow(x, training=True)
    step(xs, ys)
    decays = set(moving_average_decays(model, moving_average_buffers(model)))
    out = {"init": init, "local": cat(shadow), "synced": cat(model),
           "decay": decays.pop() if len(decays) == 1 else None,
           "params": torch.cat([p.detach().reshape(-1) for p in model.parameters()]),
           "works": len(step.dp._done_works), "buckets": len(step.dp.buckets), "scale": step.dp.grad_scale}
    step.dp.close()
    return out


def test_bn_statistics_and_collective_count_over_two_ranks():
    n = 3
    res = run_workers(_bn_accum_worker, 2, n)
    assert torch.equal(res[0]["synced"], res[1]["synced"]) and torch.equal(res[0]["params"], res[1]["params"])
    assert not torch.allclose(res[0]["local"], res[1]["local"])
    # BufferSync's formula with k = n local updates on each of W = 2 replicas
    d = res[0]["decay"]
    assert d is not None and 0.9 < d < 1.0
    prev = res[0]["init"].double()
    b = [(r["local"].double() - d ** n * prev) / (1 - d ** n) for r in res]
    want = d ** (2 * n) * prev + (1 - d ** (2 * n)) * (b[0] + b[1]) / 2
    torch.testing.assert_close(res[0]["synced"].double(), want, rtol=1e-5, atol=1e-6)
    assert not torch.allclose(res[0]["synced"].double(), d ** 2 * prev + (1 - d ** 2) * (b[0] + b[1]) / 2,
                              rtol=1e-5, atol=1e-6)  # (k = 1 would have been seen)
    # as many gradient collectives as a step of one micro-batch issues: one per bucket
    for r in res:
        assert r["works"] == r["buckets"] > 1 and r["scale"] == 1.0 / (2 * n)


def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--synthetic_data", "--batch_size=8", "--data_dir=/nonexistent", "--seed=3"]


def test_trainer_accum_steps(tmp_path):
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + d, "--max_steps=3", "--accum_steps=4", "--metrics_file=" + mf,
                 *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    recs = [json.loads(line) for line in open(mf)]
    assert [r["global_step"] for r in recs] == [1, 2, 3]
    for r in recs:
        assert r["accum_steps"] == 4 and math.isfinite(r["loss"]) and "nonfinite_micro_batches" not in r
        assert r["images_per_sec"] == pytest.approx(4 * 8 / (r["step_ms"] / 1e3), rel=1e-6)
        assert r["node_images_per_sec"] == pytest.approx(r["images_per_sec"], rel=1e-9)
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "asp"), "--sync_mode=asp", "--max_steps=2",
                 "--accum_steps=2", *COMMON)
    assert p.returncode != 0
    assert "ValueError" in p.stderr and "--accum_steps > 1 needs --sync_mode bsp" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "asp").exists()  # refused at start-up, before anything was set up
