"""Grouped conv without a GPU: the eligibility table and its errors, the CPU reference against a per-group loop, the
ResNeXt zoo entries (parameter counts, end-point shapes) and the checkpoint layout of a grouped filter."""
import pytest
import torch

from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
from distributed_tensorflow_models_amd.ckpt.saver import Saver, TFVar
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import reference as ref
from distributed_tensorflow_models_amd.ops.groupconv import GcArgs, eligible, grouped_conv2d


def _args(**kw):
    d = dict(N=2, H=14, W=14, C=64, D=8, P=14, Q=14, stride=1, ph=1, pw=1)
    d.update(kw)
    return GcArgs(*(d[n] for n, _ in GcArgs._fields_))


@pytest.mark.parametrize("kw,ok", [
    ({}, True), ({"D": 4}, True), ({"D": 16, "stride": 2, "P": 7, "Q": 7, "ph": 0, "pw": 0}, True),
    ({"D": 32, "C": 96}, True), ({"C": 48}, True),
    ({"D": 64}, False), ({"D": 2}, False), ({"D": 12, "C": 48}, False), ({"C": 40}, False), ({"D": 32, "C": 48}, False),
    ({"stride": 3}, False), ({"ph": 2}, False), ({"pw": -1}, False), ({"N": 0}, False), ({"N": 65536}, False)])
def test_eligible(kw, ok):
    assert eligible(_args(**kw)) is ok


@pytest.mark.parametrize("C,D,taps,kw,word", [
    (128, 64, 3, {}, "D=64"), (32, 2, 3, {}, "D=2"), (64, 8, 3, {"stride": 3}, "stride 3"),
    (64, 8, 5, {}, "5x5"), (64, 8, 1, {}, "1x1"), (64, 8, 3, {"rate": 2}, "rate 2"),
    (64, 8, 3, {"padding": (2, 2)}, "pad"), (24, 8, 3, {}, "C=24")])
def test_ineligible_raises_and_names_it(C, D, taps, kw, word):
    with pytest.raises(ValueError, match=word):
        grouped_conv2d(torch.zeros(1, 9, 9, C), torch.zeros(C, taps, taps, D), C // D, **kw)


@pytest.mark.parametrize("stride,padding", [(1, "SAME"), (2, "SAME"), (2, "VALID"), (1, ((1, 0), (0, 1)))])
def test_reference_is_a_per_group_loop(stride, padding):
    g = torch.Generator().manual_seed(3)
    C, D = 48, 8
    x = torch.randn(2, 9, 10, C, generator=g, dtype=torch.float64)
    w = torch.randn(C, 3, 3, D, generator=g, dtype=torch.float64)
    parts = [ref.conv2d(x[..., i:i + D], w[i:i + D], None, stride, padding) for i in range(0, C, D)]
    y = grouped_conv2d(x, w, C // D, stride, padding)  # CPU tensors: the reference, through the public op
    assert torch.equal(y, ref.grouped_conv2d(x, w, C // D, stride, padding))
    torch.testing.assert_close(y, torch.cat(parts, -1), rtol=1e-12, atol=1e-12)


@pytest.fixture(scope="module")
def resnext50():
    return nets_factory.build("resnext_50_32x4d", 1000)


def _count(m):
    return sum(p.numel() for p in m.parameters() if p.requires_grad)


def test_resnext50_parameters_and_end_points(resnext50):
    assert _count(resnext50) == 25028904
    ep = {}
    with torch.no_grad():
        logits = resnext50(torch.zeros(1, 224, 224, 3), training=False, end_points=ep)
    assert tuple(logits.shape) == (1, 1000)
    for i, (hw, depth) in enumerate([(56, 256), (28, 512), (14, 1024), (7, 2048)]):
        assert tuple(ep["resnext_50_32x4d/block%d" % (i + 1)].shape) == (1, hw, hw, depth)
    conv2 = ep["resnext_50_32x4d/block2/unit_1/bottleneck/conv2"]
    assert tuple(conv2.shape) == (1, 28, 28, 256)  # stride 2 on the grouped 3x3 of the first unit


@pytest.mark.parametrize("name,count", [("resnext_101_32x4d", 44177704), ("resnext_101_64x4d", 83455272)])
def test_resnext101_parameters(name, count):
    assert _count(nets_factory.build(name, 1000)) == count


def test_grouped_weights_checkpoint_layout(resnext50, tmp_path):
    name = "resnext_50_32x4d/block3/unit_1/bottleneck/conv2/weights"
    v = resnext50.store.vars[name]
    assert tuple(v.shape) == (512, 3, 3, 16) and v.tf_layout == "KRSC->HWIO"
    prefix = Saver([TFVar(name, v, v.tf_layout)]).save(str(tmp_path / "m.ckpt"), 1)
    assert tuple(BundleReader(prefix).get_tensor(name).shape) == (3, 3, 16, 512)
    want = v.detach().clone()
    with torch.no_grad():
        v.zero_()
    assert Saver([TFVar(name, v, v.tf_layout)]).restore(prefix) == [] and torch.equal(v, want)
