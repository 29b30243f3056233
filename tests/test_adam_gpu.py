"""Fused Adam on the GPU: the kernel against the fp64 oracle of tests/test_adam_cpu.py (same tensor set, drivers and
tolerances), its 16-byte and 4-byte load paths against each other, the device-side count of applied updates under the
NaN guard, and the captured step against the eager one."""
import math

import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib
from test_adam_cpu import (CONFIGS, SHAPES, STEPS, WDS, check, drive, first_step_norm, make_optimizer, make_ref,
                           nan_guard_through_train_step, oracle)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return make_ref()


def _setup(ref, cfg, clip=None, packed=True):
    """``packed``: the gradients are views packed back to back into ONE flat buffer starting at element 1 (bases at any
    element offset).  Even rows live in a packed weight buffer the same way, with their bf16 copies in a packed bf16
    buffer (weight, gradient and slots misaligned alike: the 16-byte path with a scalar head); odd rows are in
    allocations of their own (offset against the gradient: the 4-byte path, unless the gradient's base happens to be
    aligned).  Not ``packed``: every tensor in an aligned allocation of its own (the 16-byte path throughout)."""
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
            p.bf16 = torch.zeros(s, device=dev, dtype=torch.bfloat16)
        p.weight_decay = WDS[i]
        p.main_grad = flat_g[off:off + n[i]].view(s) if packed else torch.zeros(s, device=dev)
        params.append(p)
        off += n[i]
    buf = ref["buf"].to(dev)
    opt = make_optimizer(params, buf, cfg, clip)
    opt._hold = (flat_g, flat_w, flat_c)
    return params, buf, opt


def _path(p, opt):
    """The kernel's own choice for this tensor: ('vec', head elements) or ('scalar', None)."""
    st = opt.state[p]
    a = p.data_ptr()
    off = 0
    for t in (p.main_grad, st["s1"], st["s2"], st["ema"]):
        off |= a ^ t.data_ptr()
    head = ((16 - a % 16) % 16) // 4
    if off % 16 == 0 and (p.bf16.data_ptr() + 2 * head) % 8 == 0:
        return "vec", head
    return "scalar", None


def test_layouts_reach_both_paths(ref):
    params, _, opt = _setup(ref, CONFIGS[0])
    paths = [_path(p, opt) for p in params]
    assert all(k == "vec" for k, _ in paths[0::2])            # packed rows: slots follow the weight's misalignment
    assert sum(h != 0 for _, h in paths[0::2]) >= 3            # ... with a scalar head
    assert sum(k == "scalar" for k, _ in paths[1::2]) >= 3     # own allocations against a shifted gradient
    params, _, opt = _setup(ref, CONFIGS[0], packed=False)
    assert all(_path(p, opt) == ("vec", 0) for p in params)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "b.5_.9_eps1e-3", "b1_0"])
def test_update_matches_fp64_oracle(ref, cfg, clip):
    clip = first_step_norm(ref) / 3.0 if clip else None
    params, buf, opt = _setup(ref, cfg, clip)
    drive(params, buf, opt, ref, STEPS)
    torch.cuda.synchronize()
    if clip:
        assert float(opt._gclip) < 0.6  # the clip was active
    assert opt.adam_step() == STEPS == opt.num_updates
    check(params, buf, opt, oracle(ref, cfg, clip, STEPS), ref)


def test_both_load_paths_agree(ref):
    out = []
    for packed in (True, False):
        params, buf, opt = _setup(ref, CONFIGS[0], packed=packed)
        drive(params, buf, opt, ref, 3)
        torch.cuda.synchronize()
        out.append([t.detach().clone().reshape(-1) for p in params
                    for t in (p, opt.state[p]["s1"], opt.state[p]["s2"], opt.state[p]["ema"],
                              p.bf16.view(torch.int16))] + [opt.buffer_ema[id(buf)].clone()])
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert not torch.equal(out[0][0].cpu(), ref["w"][0].reshape(-1))


def test_skipped_update_does_not_count(ref):
    cfg = CONFIGS[0]
    params, buf, opt = _setup(ref, cfg)
    flags = [torch.tensor([1 if n == 1 else 0], dtype=torch.int32, device=params[0].device) for n in range(4)]
    drive(params, buf, opt, ref, 4, flags)
    torch.cuda.synchronize()
    assert opt.adam_step() == 3 and opt.num_updates == 4
    check(params, buf, opt, oracle(ref, cfg, None, 4, skipped=(1,)), ref)


def test_nan_guard_under_adam():
    nan_guard_through_train_step(torch.device("cuda", 0), torch.bfloat16)


def _run_steps(use_graph, steps, sched):
    """tests/test_large_batch_gpu.py's helper, for the Adam step on LeNet (no dropout: an eager step draws a new host
    seed per step, a replayed graph keeps the captured one)."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = nets_factory.build("lenet", num_classes=10, dropout_keep_prob=1.0).to(dev)
    init = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
    step = TrainStep(model, optimizer="adam", lr=0.002, use_graph=use_graph, ema_decay=0.99, lr_schedule=sched,
                     weight_decay=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-8)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(4, 28, 28, 1, generator=g).to(dev, torch.bfloat16) for _ in range(2)]
    ys = [torch.randint(0, 10, (4,), generator=g).to(dev) for _ in range(2)]
    losses = [float(step(xs[i % 2], ys[i % 2])) for i in range(steps)]
    torch.cuda.synchronize()
    params = torch.cat([p.detach().float().reshape(-1) for p in model.parameters()])
    emas = torch.cat([step.opt.state[p]["ema"].reshape(-1) for p in step.opt.params])
    step.dp.close()
    return losses, params, emas, step, init


def test_hipgraph_adam_step_matches_eager():
    sched = lambda s: 0.002 * (0.5 ** (s // 4))  # noqa: E731
    was = _lib.lib().dtm_get_deterministic()
    _lib.set_deterministic(True)  # Adam's first steps move every weight by ~lr * sign(g): fixed-order reductions
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
    assert ((pe - init).norm() / init.norm()).item() > 1e-3  # Adam moved the weights
