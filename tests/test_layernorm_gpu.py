"""The channel LayerNorm, layer scale + residual and GELU kernels (csrc/kernels/layernorm.hip, activation.hip) against
the float64 definition on the same stored inputs.

Per output, e = |got - want64|_2 / |want64|_2 of the kernels is at most max(2 e_torch, 2^-20), e_torch the error of the
op's own torch form on the device in the same storage type: 2 for a different summation order, 2^-20 (16 fp32
roundoffs) where both errors are a few ulps and their ratio is noise.  The bf16 LayerNorm forward also holds
element-wise: |y - y64| <= 2^-8 |y64| + 2^-16 (|gamma xh| + |beta|), one bf16 rounding with a margin of 2 plus fp32
statistics over at most 2048 terms."""
import copy

import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import slim_nets
from distributed_tensorflow_models_amd.models.slim_model import SlimModel
from distributed_tensorflow_models_amd.ops.activation import _torch_act, activation
from distributed_tensorflow_models_amd.ops.layernorm import (channel_layer_norm, channel_layer_norm_torch,
                                                             scale_residual, scale_residual_torch)
from test_convnext_cpu import gelu64, ln64, scale_residual64

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def _rel(got, want):
    return ((got.double().cpu() - want).norm() / want.norm()).item()


def _grads(fn, tensors, dy, cast=lambda t: t.to(DEV)):
    """fn's output and its gradients for the tensors that are not None, as (y, *grads)."""
    leaves = [None if t is None else cast(t).requires_grad_() for t in tensors]
    y = fn(*leaves)
    y.backward(cast(dy).to(y.dtype))
    return [y.detach()] + [t.grad for t in leaves if t is not None]


def _compare(tag, names, fn, fn_torch, fn64, tensors, dy, keep=slice(None), nan_ok=()):
    """The e of fn and of fn_torch against fn64 on the CPU; keep: the rows of [M, C] outputs that are compared."""
    got = _grads(fn, tensors, dy)
    yard = _grads(fn_torch, tensors, dy)
    want = _grads(fn64, tensors, dy, cast=lambda t: t.double())
    for name, g, t, w in zip(names, got, yard, want):
        if name in nan_ok:
            continue
        if g.dim() > 1:
            g, t, w = g[keep], t[keep], w[keep]
        assert torch.isfinite(g).all(), name
        e, limit = _rel(g, w), max(2 * _rel(t, w), 2.0 ** -20)
        print(tag, name, "e %.3e, limit %.3e" % (e, limit))
        assert e <= limit, (name, e, limit)
    return got, want


def _ln_inputs(shape, dtype, variant):
    g = torch.Generator().manual_seed(5)
    C = shape[-1]
    x, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    gamma, beta = 1 + 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    if variant == "offset":
        x = x + 100
    if variant == "noparams":
        gamma = beta = None
    if variant == "nan":
        x.reshape(-1, C)[1] = float("nan")
    return x.to(dtype), gamma, beta, dy.to(dtype)


LN_CASES = [
    pytest.param((1, 8), None, None, id="one-row-smallest-C"),
    pytest.param((7, 96), None, None, id="fewer-rows-than-a-wave"),
    pytest.param((2, 5, 3, 136), None, None, id="idle-vector-slots"),
    pytest.param((300, 768), 37, None, id="ragged-slabs-many-records"),
    pytest.param((33, 1024), None, None, id="four-vectors-a-lane"),
    pytest.param((5, 2048), None, None, id="largest-C"),
    pytest.param((64, 96), None, "offset", id="mean-100"),  # a one-pass variance fails this
    pytest.param((7, 96), None, "noparams", id="no-gamma-beta"),
    pytest.param((9, 136), 4, "nan", id="nan-row"),
]


@pytest.mark.parametrize("shape,slab,variant,dtype", [
    pytest.param(*c.values, d, id="%s-%s" % (c.id, n)) for c in LN_CASES for n, d in (("bf16", BF), ("fp32", F32))
    if not (c.values[2] == "offset" and d is BF)])  # bf16 keeps two digits of 100 + randn: the case is fp32's
def test_channel_layer_norm_against_float64(shape, slab, variant, dtype):
    x, gamma, beta, dy = _ln_inputs(shape, dtype, variant)
    C = shape[-1]
    keep = torch.arange(x.numel() // C) != 1 if variant == "nan" else slice(None)
    flat = [t.reshape(-1, C) for t in (x, dy)]
    got, want = _compare((shape, variant, dtype), ["y", "dx"] + ["dgamma", "dbeta"] * (gamma is not None),
                         lambda a, g, b: channel_layer_norm(a, g, b, 1e-6, slab_rows=slab),
                         lambda a, g, b: channel_layer_norm_torch(a, g, b, 1e-6), ln64, (flat[0], gamma, beta),
                         flat[1], keep, nan_ok=("dgamma", "dbeta") if variant == "nan" else ())
    if dtype == BF:
        xd = flat[0].double()[keep]
        xh = (xd - xd.mean(-1, keepdim=True)) * torch.rsqrt(xd.var(-1, keepdim=True, unbiased=False) + 1e-6)
        gx = xh if gamma is None else xh * gamma.double()
        bound = 2.0 ** -8 * want[0][keep].abs() + 2.0 ** -16 * (gx.abs() + (0 if beta is None else beta.double().abs()))
        assert ((got[0].double().cpu()[keep] - want[0][keep]).abs() <= bound).all()


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,rows,C,scaled", [(2, 15, 136, True), (2, 15, 136, False), (1, 300, 768, False)])
def test_scale_residual_against_float64(N, rows, C, scaled, dtype):
    g = torch.Generator().manual_seed(6)
    x, r, dy = (torch.randn(N, rows, C, generator=g).to(dtype) for _ in range(3))
    gamma = torch.randn(C, generator=g)
    s = torch.tensor([0.0, 1.25]) if scaled else None
    _compare((N, rows, C, scaled, dtype), ["y", "dx", "dr", "dgamma"],
             lambda a, b, c: scale_residual(a, b, c, None if s is None else s.to(DEV), slab_rows=7),
             lambda a, b, c: scale_residual_torch(a, b, c, None if s is None else s.to(DEV)),
             lambda a, b, c: scale_residual64(a, b, c, s), (x, r, gamma), dy)


@pytest.mark.parametrize("n,dtype", [(8 * 4099 + 3, BF), (100003, F32), (5, BF)])
def test_gelu_against_float64(n, dtype):
    g = torch.Generator().manual_seed(7)
    x = torch.linspace(-12, 12, n)[torch.randperm(n, generator=g)].to(dtype)
    dy = torch.randn(n, generator=g).to(dtype)
    _compare((n, dtype), ["y", "dx"], lambda a: activation(a, "gelu"), lambda a: _torch_act(a, "gelu", 0.2), gelu64,
             (x,), dy)


def test_bit_identical_runs():
    x, gamma, beta, dy = _ln_inputs((300, 768), BF, None)
    ln = lambda: _grads(lambda a, g, b: channel_layer_norm(a, g, b, slab_rows=37), (x, gamma, beta), dy)  # noqa: E731
    sr = lambda: _grads(lambda a, b, c: scale_residual(a, b, c, slab_rows=7), (x, dy, gamma), dy)  # noqa: E731
    for run in (ln, sr):
        assert all(torch.equal(a, b) for a, b in zip(run(), run()))


def test_tiny_convnext_matches_the_cpu_path_and_trains():
    torch.manual_seed(0)
    cpu = SlimModel(slim_nets.convnext, 64, num_classes=10, name="convnext", depths=(1, 1, 2, 1),
                    dims=(16, 32, 64, 128), layer_scale_init=0.5)  # a layer scale at which the branches count
    gpu = copy.deepcopy(cpu).to(DEV)
    x = torch.randn(2, 64, 64, 3)
    with torch.no_grad():
        want = cpu(x, training=False).double()
        got = gpu(x.to(DEV, BF), training=False)
        # the bound of tests/test_se_gpu.py: the oracle's own sensitivity to a bf16-sized input perturbation
        g = torch.Generator().manual_seed(1)
        sens = _rel(cpu(x * (1 + 0.004 * torch.randn(x.shape, generator=g)), training=False), want)
    print("tiny convnext e %.3e, sensitivity %.3e" % (_rel(got, want), sens))
    assert _rel(got, want) < max(6e-2, 3 * sens)
    watched = {n: p.detach().clone() for n, p in gpu.named_parameters()
               if n.endswith(("LayerNorm_gamma", "LayerScale_gamma", "pwconv1_weights", "pwconv2_weights"))}
    assert len(watched) == 10 + 5 + 10
    step = TrainStep(gpu, optimizer="momentum", lr=0.05, momentum=0.9)
    for _ in range(2):
        loss = float(step(x.to(DEV, BF), torch.tensor([3, 7], device=DEV)))
    assert loss == loss and abs(loss) < 1e3
    now = dict(gpu.named_parameters())
    assert all(not torch.equal(now[n].detach(), old) for n, old in watched.items())
