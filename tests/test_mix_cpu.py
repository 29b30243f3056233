"""Mixup / CutMix on the CPU path: the plan sampler, mix_images and the two-label loss as torch ops,
TrainStep(mix=...) against a hand-composed run, the trainer's flags."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import mix
from distributed_tensorflow_models_amd.ops import nn as F
from distributed_tensorflow_models_amd.ops.mix import MixConfig, sample_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."
BOTH = dict(mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.8, switch_prob=0.5)


# ---- sampler ----------------------------------------------------------------------------------------------------
def test_plan_is_a_pure_function_of_its_arguments():
    cfg = MixConfig(**BOTH, seed=3)
    base = sample_plan(cfg, 1, 5, 0, 16, 12, 10)
    again = sample_plan(MixConfig(**BOTH, seed=3), 1, 5, 0, 16, 12, 10)
    assert base.rec.dtype == np.int32 and base.rec.shape == (16, 8) and np.array_equal(base.rec, again.rec)
    for other in (sample_plan(MixConfig(**BOTH, seed=4), 1, 5, 0, 16, 12, 10), sample_plan(cfg, 2, 5, 0, 16, 12, 10),
                  sample_plan(cfg, 1, 6, 0, 16, 12, 10), sample_plan(cfg, 1, 5, 1, 16, 12, 10)):
        assert not np.array_equal(base.rec, other.rec)
    dev = base.to("cpu").dev
    assert dev.dtype == torch.int32 and np.array_equal(dev.numpy(), base.rec)


@pytest.mark.parametrize("per_row", [False, True])
def test_sampled_records(per_row):
    H, W, B = 9, 13, 32
    seen = set()
    for step in range(40):
        cfg = MixConfig(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.75 if not per_row else 1.0, per_row=per_row, seed=1)
        p = sample_plan(cfg, 0, step, 0, B, H, W)
        p._checked = False
        p.validate()  # every sampled record passes the wrappers' validation
        if per_row or p.kinds()[0] != "identity":
            assert sorted(p.partner.tolist()) == list(range(B))
        assert not p.rec[:, 7].any()
        for r in range(B):
            y0, y1, x0, x1 = (int(v) for v in p.box[r])
            wp, wl = p.w_pix[r], p.w_lab[r]
            assert wp.dtype == np.float32 and wl.dtype == np.float32
            if y1 > y0 and x1 > x0:  # CutMix
                seen.add("cutmix")
                assert wp == 1.0
                assert wl == np.float32(1 - (y1 - y0) * (x1 - x0) / (H * W))
                seen.add("clipped" if (y0 == 0 or x0 == 0 or y1 == H or x1 == W) else "inner")
            elif wp != 1.0:  # mixup
                seen.add("mixup")
                assert y0 == y1 and wp == wl and 0.0 <= wp < 1.0
            else:  # the identity, or a CutMix row whose box came out empty (it keeps every pixel and the label)
                seen.add("identity")
                assert wl == 1.0 and (y0 == y1 or x0 == x1)
        if not per_row:  # one draw for the whole batch
            assert (p.rec[:, 1:] == p.rec[0, 1:]).all()
    assert seen == {"cutmix", "mixup", "identity", "clipped", "inner"}


def test_cutmix_box_follows_the_paper():
    """The batch-wise CutMix draw replayed by hand from the same generator."""
    cfg = MixConfig(cutmix_alpha=1.0, seed=9)
    B, H, W = 6, 11, 7
    for step in range(20):
        rng = np.random.default_rng([9, 0, step, 0])
        rng.random()
        rng.random()
        partner = rng.permutation(B)
        lam = rng.beta(1.0, 1.0)
        rat = np.sqrt(1 - lam)
        ch, cw = int(H * rat), int(W * rat)
        cy, cx = rng.integers(H), rng.integers(W)
        y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, H)
        x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, W)
        p = sample_plan(cfg, 0, step, 0, B, H, W)
        assert p.partner.tolist() == partner.tolist()
        assert p.box.tolist() == [[y0, y1, x0, x1]] * B
        assert (p.w_pix == 1.0).all() and (p.w_lab == np.float32(1 - (y1 - y0) * (x1 - x0) / (H * W))).all()


def test_prob_zero_is_the_identity_plan_and_bad_configs_raise():
    for per_row in (False, True):
        p = sample_plan(MixConfig(**dict(BOTH, prob=0.0), per_row=per_row), 0, 0, 0, 8, 5, 5)
        assert np.array_equal(p.rec, mix.identity_plan(8, 5, 5).rec)
        assert p.partner.tolist() == list(range(8)) and (p.w_pix == 1).all() and (p.w_lab == 1).all()
        assert not p.box.any() and p.kinds() == ["identity"] * 8
    for kw in (dict(), dict(mixup_alpha=-0.1), dict(mixup_alpha=0.2, cutmix_alpha=-1.0), dict(mixup_alpha=0.2, prob=1.5),
               dict(mixup_alpha=0.2, prob=-0.1), dict(cutmix_alpha=1.0, switch_prob=2.0),
               dict(cutmix_alpha=1.0, switch_prob=float("nan"))):
        with pytest.raises(ValueError):
            MixConfig(**kw)
    with pytest.raises(ValueError):
        TrainStep(torch.nn.Linear(2, 2), mix="cutmix")


def test_per_row_mixup_weights_are_uniform_for_alpha_one():
    """Beta(1, 1) is uniform: the mean of 4096 draws has sigma 0.0045, the bound is 0.03."""
    p = sample_plan(MixConfig(mixup_alpha=1.0, cutmix_alpha=0.0, prob=1.0, per_row=True), 0, 0, 0, 4096, 8, 8)
    m = float(p.w_lab.mean())
    print("mean w_lab %.4f" % m)
    assert abs(m - 0.5) <= 0.03
    assert len(set(p.w_lab.tolist())) > 4000 and sorted(p.partner.tolist()) == list(range(4096))


def test_validation_of_the_host_copy():
    x = torch.zeros(3, 4, 5, 3)
    ok = dict(partner=[1, 2, 0], w_pix=[1.0, 0.5, 1.0], w_lab=[1.0, 0.5, 0.7], box=[[0, 0, 0, 0]] * 2 + [[1, 4, 2, 5]])
    mix.mix_images(x, mix.make_plan(H=4, W=5, **ok))
    for key, bad in (("partner", [1, 3, 0]), ("partner", [-1, 2, 0]), ("w_pix", [1.0, 1.5, 1.0]),
                     ("w_pix", [1.0, float("nan"), 1.0]), ("w_lab", [1.0, 0.5, -0.1]),
                     ("box", [[0, 0, 0, 0]] * 2 + [[1, 5, 2, 5]]), ("box", [[0, 0, 0, 0]] * 2 + [[1, 4, 2, 6]]),
                     ("box", [[0, 0, 0, 0]] * 2 + [[3, 2, 2, 5]]), ("box", [[0, 0, 0, 0]] * 2 + [[-1, 2, 2, 5]])):
        plan = mix.make_plan(H=4, W=5, **dict(ok, **{key: bad}))
        with pytest.raises(ValueError):
            mix.mix_images(x, plan)
        if key != "box":  # (the loss checks what it reads: partners and weights)
            with pytest.raises(ValueError):
                F.mean_xent_loss([(torch.zeros(3, 4), 1.0)], torch.zeros(3, dtype=torch.long), mix=plan)
    plan = mix.make_plan(H=4, W=5, **ok)
    for bad_x in (x.to(torch.float16), x[0], x.double(), x[:, :, :, :2], x[:2]):
        with pytest.raises(ValueError):
            mix.mix_images(bad_x, plan)
    with pytest.raises(ValueError):
        mix.mix_images(x, plan, out=x)  # in place: partners are read after other rows were written
    buf = torch.zeros(2 * x.numel() - 7)
    with pytest.raises(ValueError):
        mix.mix_images(buf[:x.numel()].view(x.shape), plan, out=buf[x.numel() - 7:].view(x.shape))


# ---- mix_images -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mix_images_against_a_python_loop(dtype):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 4, 5, 3, generator=g).to(dtype)
    lam = np.float32(0.3)
    plan = mix.make_plan([0, 2, 0], [1.0, lam, 1.0], [1.0, lam, 0.55], [[0, 0, 0, 0], [0, 0, 0, 0], [1, 4, 2, 4]], 4, 5)
    assert plan.kinds() == ["identity", "mixup", "cutmix"]
    sent = torch.full((x.numel() + 10,), 7.0, dtype=dtype)
    out = sent[5:5 + x.numel()].view(x.shape)
    got = mix.mix_images(x, plan, out=out)
    assert got is out and bool((sent[:5] == 7).all()) and bool((sent[-5:] == 7).all())
    assert torch.equal(mix.mix_images(x, plan), out)
    want = torch.empty_like(x)
    for r in range(3):
        p, w = int(plan.partner[r]), plan.w_pix[r]
        y0, y1, x0, x1 = plan.box[r]
        for y in range(4):
            for xx in range(5):
                for c in range(3):
                    a, b = np.float32(float(x[r, y, xx, c])), np.float32(float(x[p, y, xx, c]))
                    if y0 <= y < y1 and x0 <= xx < x1:
                        v = b
                    elif w == 1.0:
                        v = a
                    else:
                        v = np.float32(np.float32(w * a) + np.float32(np.float32(np.float32(1) - w) * b))
                    want[r, y, xx, c] = torch.tensor(float(v)).to(dtype)
    assert torch.equal(out, want)
    assert torch.equal(out[0], x[0]) and not torch.equal(out[1], x[1]) and torch.equal(out[2, 1:4, 2:4], x[0, 1:4, 2:4])


def test_mix_images_copies_are_bit_copies():
    x = torch.randn(2, 3, 3, 1)
    x[0, 0, 0, 0] = -0.0
    x[1, 2, 2, 0] = float("nan")  # the partner's pixel outside the box: must not leak (0 * NaN would)
    x[0, 1, 1, 0] = float("inf")  # the row's own pixel inside the box: replaced
    plan = mix.make_plan([1, 0], [1.0, 1.0], [0.8, 1.0], [[1, 2, 1, 2], [0, 0, 0, 0]], 3, 3)
    out = mix.mix_images(x, plan)
    assert bool(torch.isfinite(out[0]).all()) and out[0, 1, 1, 0] == x[1, 1, 1, 0]
    assert torch.equal(out[0].view(torch.int32)[0, 0], x[0].view(torch.int32)[0, 0])  # -0.0 kept
    assert torch.equal(out[1].view(torch.int32), x[1].view(torch.int32))


# ---- the two-label loss ---------------------------------------------------------------------------------------
def soft_target_loss_fp64(logits, labels, plan, smoothing):
    """mean_r -sum_k t_k log p_k with t the mix of the two labels' smoothed one-hot targets, in fp64."""
    B, K = logits.shape
    on, off = 1.0 - smoothing + smoothing / K, smoothing / K
    w = torch.from_numpy(plan.w_lab.astype(np.float64)).view(B, 1)
    la, lb = labels.long(), labels.long()[torch.from_numpy(plan.partner.astype(np.int64))]
    hot = w * torch.nn.functional.one_hot(la, K).double() + (1 - w) * torch.nn.functional.one_hot(lb, K).double()
    t = off + (on - off) * hot
    return -(t * torch.log_softmax(logits.double(), -1)).sum(-1).mean()


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_mixed_loss_against_fp64_soft_targets(smoothing):
    g = torch.Generator().manual_seed(4)
    B, K = 16, 37
    main, aux = torch.randn(B, K, generator=g) * 3, torch.randn(B, K, generator=g)
    labels = torch.randint(0, K, (B,), generator=g)
    for per_row in (False, True):
        for step in range(4):
            plan = sample_plan(MixConfig(**BOTH, per_row=per_row), 0, step, 0, B, 8, 8)
            got = float(F.mean_xent_loss([(main, 1.0), (aux, 0.4)], labels, smoothing, mix=plan))
            ref = float(soft_target_loss_fp64(main, labels, plan, smoothing)
                        + 0.4 * soft_target_loss_fp64(aux, labels, plan, smoothing))
            assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    ident = mix.identity_plan(B, 8, 8)
    assert torch.equal(F.mean_xent_loss([(main, 1.0), (aux, 0.4)], labels, smoothing, mix=ident),
                       F.mean_xent_loss([(main, 1.0), (aux, 0.4)], labels, smoothing))
    with pytest.raises(ValueError):
        F.mean_xent_loss([(main[:8], 1.0)], labels[:8], smoothing, mix=ident)


# ---- the step -------------------------------------------------------------------------------------------------
MB = 16


def lenet():
    torch.manual_seed(0)
    return nets_factory.build("lenet", 10, dropout_keep_prob=1.0)


def batches(n):
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(MB, 28, 28, 1, generator=g), torch.randint(0, 10, (MB,), generator=g)) for _ in range(n)]


def params_of(model):
    return [p.detach().clone() for p in model.parameters()]


def run(accum, mix_cfg, steps=3):
    model = lenet()
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, label_smoothing=0.1, accum_steps=accum,
                     mix=mix_cfg)
    data = batches(steps * accum)
    losses, lams = [], []
    for s in range(steps):
        xs, ys = zip(*data[s * accum:(s + 1) * accum])
        keep = [x.clone() for x in xs]
        losses.append(step(list(xs), list(ys)) if accum > 1 else step(xs[0], ys[0]))
        assert all(torch.equal(a, b) for a, b in zip(keep, xs))  # the caller's batch is never written
        lams.append(step.last_mix_lambda())
    step.dp.close()
    return losses, params_of(model), lams


@pytest.mark.parametrize("accum", [1, 2])
def test_step_with_prob_zero_is_the_plain_step(accum):
    l0, p0, lam0 = run(accum, None)
    l1, p1, lam1 = run(accum, MixConfig(**dict(BOTH, prob=0.0)))
    assert lam0 == [None] * 3 and lam1 == [1.0] * 3
    assert all(torch.equal(a, b) for a, b in zip(l0, l1)) and all(torch.equal(a, b) for a, b in zip(p0, p1))


@pytest.mark.parametrize("accum", [1, 2])
def test_step_equals_the_hand_composed_run(accum):
    cfg = MixConfig(**BOTH, seed=0 if accum == 2 else 4)
    losses, params, lams = run(accum, cfg)
    # by hand: mix every micro-batch with sample_plan(cfg, 0, step, micro, ...), the composed two-label loss, and a
    # plain step's machinery (a TrainStep without mixing whose loss is swapped for the composed one)
    model = lenet()
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, label_smoothing=0.1, accum_steps=accum)
    data = batches(3 * accum)
    kinds, want_losses, want_lams = set(), [], []
    for s in range(3):
        plans = [sample_plan(cfg, 0, s, i, MB, 28, 28) for i in range(accum)]
        kinds.update(p.kinds()[0] for p in plans)
        xs = [mix.mix_images(data[s * accum + i][0], plans[i]) for i in range(accum)]
        ys = [data[s * accum + i][1] for i in range(accum)]
        queue = list(plans)

        def composed(out, labels, _queue=queue):
            p = _queue.pop(0)
            wl = torch.from_numpy(p.w_lab.copy())
            la = F.softmax_cross_entropy(out, labels, 0.1)
            lb = F.softmax_cross_entropy(out, labels[torch.from_numpy(p.partner.astype(np.int64))], 0.1)
            return (wl * la + (1.0 - wl) * lb).mean()
        step.loss_fn = composed
        want_losses.append(step(xs, ys) if accum > 1 else step(xs[0], ys[0]))
        assert not queue
        want_lams.append(float(np.mean([p.w_lab.astype(np.float64).mean() for p in plans])))
    step.dp.close()
    assert len(kinds) >= 2 and kinds != {"identity"}  # the three steps did mix
    assert all(torch.equal(a, b) for a, b in zip(losses, want_losses))
    assert all(torch.equal(a, b) for a, b in zip(params, params_of(model)))
    assert lams == pytest.approx(want_lams, rel=1e-12)
    plain = run(accum, None)[1]
    assert not all(torch.equal(a, b) for a, b in zip(params, plain))


# ---- trainer ----------------------------------------------------------------------------------------------------
def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--synthetic_data", "--batch_size=8", "--data_dir=/nonexistent", "--seed=3"]


def test_trainer_refuses_mixing_under_asp(tmp_path):
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % (tmp_path / "asp"), "--sync_mode=asp", "--max_steps=2",
                 "--mixup_alpha=0.2", *COMMON)
    assert p.returncode != 0
    assert "ValueError" in p.stderr and "need --sync_mode bsp" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "asp").exists()  # refused at start-up, before anything was set up


def test_trainer_cutmix_run_logs_mix_lambda(tmp_path):
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + d, "--max_steps=3", "--cutmix_alpha=1.0", "--metrics_file=" + mf,
                 *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    recs = [json.loads(line) for line in open(mf)]
    assert [r["global_step"] for r in recs] == [1, 2, 3]
    want = [float(sample_plan(MixConfig(cutmix_alpha=1.0, seed=3), 0, s, 0, 8, 28, 28).w_lab.mean()) for s in range(3)]
    for r, w in zip(recs, want):
        assert 0.0 <= r["mix_lambda"] <= 1.0 and np.isfinite(r["loss"])
        assert r["mix_lambda"] == pytest.approx(w, rel=1e-6)
    assert len(set(r["mix_lambda"] for r in recs)) > 1
