"""ConvNeXt on the CPU path: parameter counts (stem + blocks of 8 C^2 + 58 C + downsamplers + head, worked out by hand
from the published architecture), end points, the torch definitions of ops/layernorm.py and GELU against float64, and
stochastic depth's and layer scale's start."""
import math

import pytest
import torch

from distributed_tensorflow_models_amd.models import nets_factory, slim_nets
from distributed_tensorflow_models_amd.models.slim_model import SlimModel
from distributed_tensorflow_models_amd.ops.activation import gelu
from distributed_tensorflow_models_amd.ops.layernorm import channel_layer_norm, scale_residual


def ln64(x, gamma, beta, eps=1e-6):
    x = x.double()
    y = (x - x.mean(-1, keepdim=True)) / torch.sqrt(((x - x.mean(-1, keepdim=True)) ** 2).mean(-1, keepdim=True) + eps)
    y = y if gamma is None else y * gamma.double()
    return y if beta is None else y + beta.double()


def scale_residual64(x, r, gamma, s=None):
    g = gamma.double() if s is None else s.double().reshape((-1,) + (1,) * (x.dim() - 1)) * gamma.double()
    return x.double() + g * r.double()


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


@pytest.mark.parametrize("name,count", [("convnext_tiny", 28589128), ("convnext_small", 50223688),
                                        ("convnext_base", 88591464)])
def test_parameter_counts(name, count):
    assert sum(p.numel() for p in nets_factory.build(name, 1000).parameters() if p.requires_grad) == count


def test_end_points_and_layer_scale_start():
    net = nets_factory.build("convnext_tiny", 1000, layer_scale_init=0.25)
    ep = {}
    with torch.no_grad():
        logits = net(torch.zeros(1, 224, 224, 3), training=False, end_points=ep)
    assert tuple(logits.shape) == (1, 1000) and tuple(ep["convnext_tiny/stem"].shape) == (1, 56, 56, 96)
    assert [tuple(ep["convnext_tiny/stage%d" % i].shape) for i in (1, 2, 3, 4)] == [
        (1, 56, 56, 96), (1, 28, 28, 192), (1, 14, 14, 384), (1, 7, 7, 768)]
    scales = [v for n, v in net.store.vars.items() if n.endswith("LayerScale/gamma")]
    assert len(scales) == 18 and all(bool((v == 0.25).all()) and v.weight_decay == 0 for v in scales)
    assert all(v.weight_decay == (0.05 if n.endswith("weights") else 0) for n, v in net.store.vars.items())


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2.0 ** -20), (torch.bfloat16, 2.0 ** -8)])
def test_torch_definitions_against_float64(dtype, tol):
    g = torch.Generator().manual_seed(3)
    x, r = (torch.randn(2, 5, 3, 136, generator=g).to(dtype) for _ in range(2))
    gamma, beta, s = torch.randn(136, generator=g), torch.randn(136, generator=g), torch.tensor([0.0, 1.25])
    for got, want in ((channel_layer_norm(x, gamma, beta), ln64(x, gamma, beta)),
                      (channel_layer_norm(x), ln64(x, None, None)),
                      (scale_residual(x, r, gamma, s), scale_residual64(x, r, gamma, s)),
                      (gelu(6 * x), gelu64(6 * x))):
        assert got.dtype == dtype
        assert ((got.double() - want).norm() / want.norm()).item() <= tol


def test_drop_path_rate_0_draws_nothing(monkeypatch):
    net = SlimModel(slim_nets.convnext, 32, num_classes=10, name="convnext", depths=(1, 1, 1, 1), dims=(8, 16, 24, 32),
                    layer_scale_init=0.5)
    x = torch.randn(2, 32, 32, 3)
    monkeypatch.setattr(torch, "rand", None)  # a draw would raise
    with torch.no_grad():
        assert torch.equal(net(x, training=True), net(x, training=False))
    monkeypatch.undo()
    net.kw["drop_path_rate"] = 0.9
    with torch.no_grad():
        assert not torch.equal(net(x, training=True), net(x, training=False))
        assert torch.equal(net(x, training=False), net(x, training=False))
