"""Fused LAMB on the GPU: the four launches against the fp64 oracle of tests/lamb_cases.py (same tensor set, drivers
and tolerances as tests/test_lamb_cpu.py), the 16-byte and 4-byte access paths of the moments and apply kernels
against each other, the fixed-order reductions, the apply pass's recomputed direction, the skip flag, the NaN guard and
the captured step against the eager one."""
import math

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops.optim import _bias_corrections
from lamb_cases import (CONFIG_IDS, CONFIGS, GRAD_SCALE, LR_MULTS, LRS, SHAPES, STEPS, WDS, check, drive, make_optimizer,
                        make_ref, nan_guard_through_train_step, oracle)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return make_ref()


def _setup(ref, cfg, packed=True):
    """``packed``: the gradients are views packed back to back into ONE flat buffer starting at element 1 (bases at any
    element offset).  Even rows live in a packed weight buffer the same way, with their bf16 copies in a packed bf16
    buffer (weight, gradient and slots misaligned alike: the 16-byte paths with a scalar head); odd rows are in
    allocations of their own (offset against the gradient: the moments pass's 4-byte path, unless the gradient's base
    happens to be aligned), and of those rows 3, 7 and 11 have a bf16 copy that starts one element into its
    allocation (the apply pass's 4-byte path: its 8-byte stores cannot be used).  Not ``packed``: every tensor in an
    aligned allocation of its own (the 16-byte paths throughout)."""
    dev = torch.device("cuda", 0)
    n = [int(np.prod(s)) for s in SHAPES]
    flat_g = torch.zeros(sum(n) + 3, device=dev)
    flat_w = torch.zeros(sum(n) + 3, device=dev)
    flat_c = torch.zeros(sum(n) + 3, device=dev, dtype=torch.bfloat16)
    params, off = [], 1
    for i, s in enumerate(SHAPES):
        if packed and i % 2 == 0:
            flat_w[off:off + n[i]].copy_(ref["w"][i].reshape(-1))
            p = torch.nn.Parameter(flat_w[off:off + n[i]].view(s))
            p.bf16 = flat_c[off:off + n[i]].view(s)
        else:
            p = torch.nn.Parameter(ref["w"][i].to(dev))
            shift = 1 if (packed and i % 4 == 3) else 0
            p.bf16 = torch.zeros(n[i] + shift, device=dev, dtype=torch.bfloat16)[shift:].view(s)
        p.weight_decay = WDS[i]
        p.main_grad = flat_g[off:off + n[i]].view(s) if packed else torch.zeros(s, device=dev)
        params.append(p)
        off += n[i]
    buf = ref["buf"].to(dev)
    opt = make_optimizer(params, buf, cfg)
    opt._hold = (flat_g, flat_w, flat_c)
    return params, buf, opt


def _paths(p, opt):
    """The kernels' own choices for this tensor: (moments pass, apply pass), each ('vec', head elements) or
    ('scalar', None)."""
    st = opt.state[p]
    a = p.data_ptr()
    head = ((16 - a % 16) % 16) // 4
    off = 0
    for t in (p.main_grad, st["s1"], st["s2"]):
        off |= a ^ t.data_ptr()
    moments = ("vec", head) if off % 16 == 0 else ("scalar", None)
    off = 0
    for t in (st["s1"], st["s2"], st["ema"]):
        off |= a ^ t.data_ptr()
    apply_ = ("vec", head) if off % 16 == 0 and (p.bf16.data_ptr() + 2 * head) % 8 == 0 else ("scalar", None)
    return moments, apply_


def test_layouts_reach_both_paths(ref):
    params, _, opt = _setup(ref, CONFIGS[0])
    paths = [_paths(p, opt) for p in params]
    for k in (0, 1):  # packed rows: slots follow the weight's misalignment, both passes vectorised with a scalar head
        assert all(pp[k][0] == "vec" for pp in paths[0::2])
        assert sum(pp[k][1] != 0 for pp in paths[0::2]) >= 3
    assert sum(pp[0][0] == "scalar" for pp in paths[1::2]) >= 3  # own allocations against a shifted gradient
    assert [pp[1][0] for pp in paths[3::4]] == ["scalar"] * 3      # the shifted bf16 copies
    assert paths[11][0][0] == "scalar"                             # the row of more than 64 chunks, 4-byte path here
    params, _, opt = _setup(ref, CONFIGS[0], packed=False)
    assert all(_paths(p, opt) == (("vec", 0), ("vec", 0)) for p in params)  # ... and the 16-byte path here


@pytest.mark.parametrize("cfg", CONFIGS, ids=CONFIG_IDS)
def test_update_matches_fp64_oracle(ref, cfg):
    params, buf, opt = _setup(ref, cfg)
    phis = drive(params, buf, opt, ref, STEPS)
    torch.cuda.synchronize()
    assert opt.adam_step() == STEPS == opt.num_updates
    check(params, buf, opt, oracle(ref, cfg, STEPS), ref, phis)


def _ordered(x):
    """fp32 bit patterns as integers that are monotonic in the value: differences are distances in ulps."""
    i = x.detach().cpu().contiguous().view(torch.int32).to(torch.int64).reshape(-1)
    return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))


def test_layouts_agree(ref):
    cfg, out = CONFIGS[0], []
    for packed in (True, False):
        params, buf, opt = _setup(ref, cfg, packed=packed)
        phis = drive(params, buf, opt, ref, 3)
        torch.cuda.synchronize()
        check(params, buf, opt, oracle(ref, cfg, 3), ref, phis)  # p of either layout within the oracle's tolerance
        out.append(([opt.state[p][k].detach().clone().reshape(-1) for p in params for k in ("s1", "s2")], phis))
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b)  # m and v depend neither on p nor on a reduction
    # the fp64 sums of the two layouts differ in their order only (about 1e-16 relative), so the once-rounded fp32
    # ratio moves by one step at the most
    worst = max(int((_ordered(a) - _ordered(b)).abs().max()) for a, b in zip(out[0][1], out[1][1]))
    print("largest distance between the layouts' trust ratios: %d ulp" % worst)
    assert worst <= 1


def test_same_layout_twice_is_bit_identical(ref):
    out = []
    for _ in range(2):
        params, buf, opt = _setup(ref, CONFIGS[0])
        drive(params, buf, opt, ref, 3)
        torch.cuda.synchronize()
        out.append([t.detach().clone().reshape(-1) for p in params
                    for t in (p, opt.state[p]["s1"], opt.state[p]["s2"], opt.state[p]["ema"],
                              p.bf16.view(torch.int16))] + [opt.last_norms().clone(), opt.last_lr_scale().clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_apply_pass_recomputes_the_direction(ref):
    """p after one step from the pre-step p, the device's m, v and phi and the kernel's own fp32 operations on the host.
    Quotients, the root and the products are correctly rounded on both sides (the root is taken in fp64 and rounded to
    fp32 here, which is the correctly rounded fp32 root; torch's fp32 sqrt on the CPU may come from a vector library
    that is not); the two fused multiply-adds are formed here in fp64 (the product of two fp32 values is exact there)
    and rounded to fp32, which is the fused result except where the fp64 sum lands within its own rounding error of an
    fp32 tie - so the comparison allows 1 ulp, and the count of elements that are not bit-equal is printed."""
    b1, b2, eps = cfg = CONFIGS[0]
    params, buf, opt = _setup(ref, cfg)
    drive(params, buf, opt, ref, 1)
    torch.cuda.synchronize()
    rec = opt._adam_state.cpu()  # {t, 1 - b1^t, sqrt(1 - b2^t), pad}: the corrections as the device rounded them
    assert int(rec[0]) == 1
    bc1, bc2 = rec[1:3].view(torch.float32)
    assert (float(bc1), float(bc2)) == pytest.approx([float(x) for x in _bias_corrections(b1, b2, 1)], rel=1e-6)
    eps32, lr32 = torch.tensor(eps, dtype=torch.float32), torch.tensor(LRS[0], dtype=torch.float32)
    phi = opt.last_lr_scale().cpu()
    off_by_one = total = 0
    for i, p in enumerate(params):
        p0 = ref["w"][i]
        m, v = opt.state[p]["s1"].cpu(), opt.state[p]["s2"].cpu()
        wd = torch.tensor(WDS[i], dtype=torch.float32)
        q = (m / bc1) / (v.double().sqrt().float() / bc2 + eps32)
        r = (wd.double() * p0.double() + q.double()).float()
        step = (lr32 * torch.tensor(LR_MULTS.get(i, 1.0), dtype=torch.float32)) * phi[i]
        want = (p0.double() - step.double() * r.double()).float()
        dist = (_ordered(want) - _ordered(p)).abs()
        assert int(dist.max()) <= 1, (i, int(dist.max()))
        off_by_one += int((dist != 0).sum())
        total += dist.numel()
    print("elements not bit-equal to the host's evaluation: %d of %d" % (off_by_one, total))
    assert not torch.equal(params[0].detach().cpu(), ref["w"][0])


def test_last_norms_columns(ref):
    cfg = CONFIGS[0]
    params, buf, opt = _setup(ref, cfg)
    drive(params, buf, opt, ref, 2)
    torch.cuda.synchronize()
    got = opt.last_norms().cpu().double()
    want = torch.tensor(oracle(ref, cfg, 2)["norms"][1], dtype=torch.float64)  # (|p|, |r|, |gs|) before the 2nd apply
    assert got.shape == (len(params) + 1, 3)
    torch.testing.assert_close(got[:len(params)], want, rtol=1e-5, atol=0.0)
    assert float(got[len(params)].abs().max()) == 0.0  # the EMA-only row
    ns = opt.norm_stats()
    assert ns["grad_norm"] == pytest.approx(float(want[:, 2].square().sum().sqrt()), rel=1e-5)
    assert ns["update_norm"] == pytest.approx(float(want[:, 1].square().sum().sqrt()), rel=1e-5)


def test_skip_flag_leaves_everything_alone(ref):
    cfg = CONFIGS[0]
    params, buf, opt = _setup(ref, cfg)
    flags = [torch.tensor([1 if n == 1 else 0], dtype=torch.int32, device=params[0].device) for n in range(4)]
    snaps = {}

    def snapshot(n):
        snaps[n] = [t.detach().clone() for p in params
                    for t in (p, opt.state[p]["s1"], opt.state[p]["s2"], opt.state[p]["ema"], p.bf16)] + \
                   [opt.last_lr_scale().clone(), opt.last_norms().clone()]

    phis = drive(params, buf, opt, ref, 4, flags, after=snapshot)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(snaps[0], snaps[1]))  # the skipped step wrote nothing
    assert any(not torch.equal(a, b) for a, b in zip(snaps[1], snaps[2]))
    assert opt.adam_step() == 3 and opt.num_updates == 4
    check(params, buf, opt, oracle(ref, cfg, 4, skipped=(1,)), ref, [phis[0], phis[2], phis[3]])


def test_nan_guard_under_lamb():
    nan_guard_through_train_step(torch.device("cuda", 0), torch.bfloat16)


def _run_steps(use_graph, steps, sched):
    """tests/test_adam_gpu.py's helper, for the LAMB step on LeNet (no dropout: an eager step draws a new host seed per
    step, a replayed graph keeps the captured one)."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = nets_factory.build("lenet", num_classes=10, dropout_keep_prob=1.0).to(dev)
    init = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
    step = TrainStep(model, optimizer="lamb", lr=0.002, use_graph=use_graph, ema_decay=0.99, lr_schedule=sched,
                     weight_decay=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-6)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(4, 28, 28, 1, generator=g).to(dev, torch.bfloat16) for _ in range(2)]
    ys = [torch.randint(0, 10, (4,), generator=g).to(dev) for _ in range(2)]
    losses = [float(step(xs[i % 2], ys[i % 2])) for i in range(steps)]
    torch.cuda.synchronize()
    params = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
    emas = torch.cat([step.opt.state[p]["ema"].reshape(-1) for p in step.opt.params])
    step.dp.close()
    return losses, params, emas, step, init


def test_hipgraph_lamb_step_matches_eager():
    sched = lambda s: 0.002 * (0.5 ** (s // 4))  # noqa: E731
    was = _lib.lib().dtm_get_deterministic()
    _lib.set_deterministic(True)  # the first steps move every weight by about lr * phi * sign(g): fixed-order sums
    try:
        le, pe, ee, se, init = _run_steps(False, 6, sched)
        lg, pg_, eg, sg, _ = _run_steps(True, 6, sched)
    finally:
        _lib.set_deterministic(bool(was))
    assert sg._graph is not None and sg.global_step == 6 and sg.opt.num_updates == 6
    assert se.opt.adam_step() == 6 and sg.opt.adam_step() == 6  # t advanced inside the four replays
    assert all(math.isfinite(v) for v in le)
    assert lg == pytest.approx(le, rel=2e-2, abs=2e-3)
    for a, b in ((pg_, pe), (eg, ee)):
        assert ((a - b).norm() / b.norm()).item() < 1e-3
    assert ((pe - init).norm() / init.norm()).item() > 1e-3  # LAMB moved the weights


@pytest.mark.parametrize("b2,eps", [(1.0, 1e-6), (0.999, -1e-6)], ids=["beta2_1", "negative_eps"])
def test_entry_point_refuses_bad_arguments(ref, b2, eps):
    params, buf, opt = _setup(ref, CONFIGS[0], packed=False)
    for p, g in zip(params, ref["grads"][0]):
        p.main_grad.copy_(g)
    opt.set_dynamic(LRS[0], GRAD_SCALE)
    rc = _lib.lib().dtm_multi_tensor_lamb(
        _lib.ptr(opt._tens_dev), _lib.ptr(opt._chunks_dev), opt._nchunks, _lib.ptr(opt._meta_dev), opt._ntens, 0.9,
        b2, eps, 1, None, _lib.ptr(opt._dyn), _lib.ptr(opt._adam_state), _lib.ptr(opt._norm_scratch),
        _lib.ptr(opt._norms), _lib.ptr(opt._lr_scale), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc < 0
    assert opt.adam_step() == 0  # nothing was launched: not even the state advance
    assert all(torch.equal(p.detach().cpu(), w) for p, w in zip(params, ref["w"]))
    assert all(float(opt.state[p]["s1"].abs().max()) == 0.0 for p in params)
