"""Self-attention without a GPU: the torch composition against the float64 definition, the layer's variables and their
checkpoint layout, the botnet_50 zoo entry, and the fallback of an ineligible call."""
import pytest
import torch

from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
from distributed_tensorflow_models_amd.ckpt.saver import Saver, TFVar
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops.attention import mhsa, mhsa_torch


def definition(q, k, v, heads, scale):
    """The issue's four lines as einsums; q, k, v [N, L, heads * d].  Returns o, lse, p."""
    N, L, C = q.shape
    qh, kh, vh = (t.reshape(N, L, heads, C // heads) for t in (q, k, v))
    s = scale * torch.einsum("nihc,njhc->nhij", qh, kh)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("nhij,njhc->nihc", p / l, vh).reshape(N, L, C)
    return o, (m + torch.log(l)).squeeze(-1), p / l


@pytest.mark.parametrize("shape", [(2, 5, 2, 4), (1, 3, 7, 3, 48)])  # [N, L] or [N, H, W], heads, d (48: no kernel)
def test_torch_composition_against_the_definition(shape):
    *lead, heads, d = shape
    g = torch.Generator().manual_seed(3)
    q, k, v, do = (torch.randn(*lead, heads * d, generator=g) for _ in range(4))
    a = [t.clone().requires_grad_() for t in (q, k, v)]
    b = [t.double().reshape(lead[0], -1, heads * d).requires_grad_() for t in (q, k, v)]
    oa = mhsa(*a, heads)  # CPU tensors: the composition
    assert torch.equal(oa, mhsa_torch(q, k, v, heads)) and oa.shape == q.shape
    ob = definition(*b, heads, d ** -0.5)[0]
    oa.backward(do)
    ob.backward(do.double().reshape(ob.shape))
    torch.testing.assert_close(oa.double().reshape(ob.shape), ob, rtol=1e-5, atol=1e-6)
    for ta, tb in zip(a, b):
        torch.testing.assert_close(ta.grad.double().reshape(tb.shape), tb.grad, rtol=1e-4, atol=1e-5)


def test_ineligible_head_size_falls_back():
    q, k, v = (torch.randn(1, 4, 96).to(torch.bfloat16) for _ in range(3))
    assert torch.equal(mhsa(q, k, v, 2), mhsa_torch(q, k, v, 2))  # d = 48
    with pytest.raises(ValueError, match="heads"):
        mhsa(q, k, v, 5)


@pytest.fixture(scope="module")
def botnet50():
    return nets_factory.build("botnet_50", 1000)


def test_botnet50_parameters_and_end_points(botnet50):
    assert sum(p.numel() for p in botnet50.parameters() if p.requires_grad) == 20867112
    ep = {}
    with torch.no_grad():
        logits = botnet50(torch.zeros(1, 224, 224, 3), training=False, end_points=ep)
    assert tuple(logits.shape) == (1, 1000)
    assert tuple(ep["botnet_50/block4/unit_1/bottleneck/mhsa"].shape) == (1, 14, 14, 512)  # before the pool
    assert tuple(ep["botnet_50/block4/unit_2/bottleneck/mhsa"].shape) == (1, 7, 7, 512)
    unit = "botnet_50/block4/unit_%d/bottleneck/mhsa/"
    shapes = {n: tuple(botnet50.store.vars[n].shape) for n in botnet50.store.vars if "/mhsa/" in n}
    assert shapes[unit % 1 + "pos_h"] == shapes[unit % 1 + "pos_w"] == (14, 512)
    assert shapes[unit % 2 + "pos_h"] == shapes[unit % 3 + "pos_w"] == (7, 512)
    assert shapes[unit % 1 + "qkv/weights"] == (1536, 1, 1, 512) and unit % 1 + "qkv/biases" not in shapes
    assert unit % 1 + "BatchNorm/gamma" in shapes and len(shapes) == 3 * 7
    with pytest.raises(ValueError, match="position variables"):
        botnet50(torch.zeros(1, 256, 256, 3), training=False)


def test_mhsa_heads_0_is_todays_resnext(botnet50):
    kw = dict(cardinality=1, base_width=64)
    plain = set(nets_factory.build("resnext_50_32x4d", 10, **kw).store.vars)
    assert set(nets_factory.build("resnext_50_32x4d", 10, mhsa_heads=0, **kw).store.vars) == plain
    bot = {n.replace("botnet_50", "resnext_50_1x64d") for n in botnet50.store.vars}
    assert all("/block4/" in n and ("/mhsa/" in n or "/conv2/" in n) for n in bot ^ plain)


def test_qkv_weights_checkpoint_layout(botnet50, tmp_path):
    name = "botnet_50/block4/unit_2/bottleneck/mhsa/qkv/weights"
    v = botnet50.store.vars[name]
    assert v.tf_layout == "KRSC->HWIO" and v.weight_decay > 0
    assert botnet50.store.vars[name.replace("qkv/weights", "pos_h")].weight_decay == 0
    prefix = Saver([TFVar(name, v, v.tf_layout)]).save(str(tmp_path / "m.ckpt"), 1)
    assert tuple(BundleReader(prefix).get_tensor(name).shape) == (1, 1, 512, 1536)
