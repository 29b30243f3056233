"""Which depthwise family a call runs: tile_eligible and the "auto" choice as a table, no GPU."""
import pytest
import torch

from distributed_tensorflow_models_amd.ops.depthwise import DwArgs, depthwise_conv2d, resolve_impl, tile_eligible
from distributed_tensorflow_models_amd.ops.geometry import conv_geom


def _args(C, M=1, R=3, stride=1, rate=1, H=14):
    g = conv_geom((2, H, H, C), (C, R, R, C), stride, "SAME", rate)
    return DwArgs(g.N, g.H, g.W, g.C, M, R, R, g.P, g.Q, g.stride, g.pad_h, g.pad_w, rate)


@pytest.mark.parametrize("C", [96, 144, 192, 384, 576, 960, 24, 48, 768])
@pytest.mark.parametrize("stride", [1, 2])
def test_auto_moves_the_scalar_shapes(C, stride):
    a = _args(C, stride=stride)
    assert tile_eligible(a) and resolve_impl(a, "auto") == "tile" and resolve_impl(a, "legacy") == "legacy"


@pytest.mark.parametrize("C", [32, 64, 128, 256, 512, 1024])
def test_auto_keeps_the_vector_shapes(C, monkeypatch):
    a = _args(C)
    assert tile_eligible(a) and resolve_impl(a, "auto") == "legacy" and resolve_impl(a, "tile") == "tile"
    monkeypatch.delenv("DTM_DW_IMPL", raising=False)
    assert resolve_impl(a) == "legacy"
    monkeypatch.setenv("DTM_DW_IMPL", "tile")  # read at each call
    assert resolve_impl(a) == "tile"


@pytest.mark.parametrize("kw", [dict(C=96, M=2), dict(C=96, rate=2), dict(C=44), dict(C=96, R=9)],
                         ids=["M2", "rate2", "C44", "R9"])
def test_ineligible(kw):
    a = _args(**kw)
    assert not tile_eligible(a) and resolve_impl(a, "auto") == "legacy"
    x, w = torch.zeros(2, 14, 14, a.C), torch.zeros(a.R, a.S, a.C, a.M)
    with pytest.raises(ValueError):
        depthwise_conv2d(x, w, 1, "SAME", a.dil, impl="tile")
    assert depthwise_conv2d(x, w, 1, "SAME", a.dil).shape == (2, 14, 14, a.C * a.M)  # CPU tensors: the reference


def test_unknown_impl():
    with pytest.raises(ValueError):
        depthwise_conv2d(torch.zeros(1, 5, 5, 8), torch.zeros(3, 3, 8, 1), impl="fast")
