"""Shared inputs of the int8 tests: quantiser records, one random integer layer, and a 3-layer slim net."""
import math

import torch

from distributed_tensorflow_models_amd.compat import quantize as Q
from distributed_tensorflow_models_amd.compat import slim
from distributed_tensorflow_models_amd.models.slim_model import SlimModel
from distributed_tensorflow_models_amd.ops import fakequant as FQ
from distributed_tensorflow_models_amd.ops.nn import invalidate_weight_copies


def rec(scale, zp, qmin=0, qmax=255):
    """A quantiser record (ops/fakequant.py) written by hand."""
    r = torch.zeros(8, dtype=torch.int32)
    f = r.view(torch.float32)
    f[0] = scale
    f[1:2] = 1.0 / f[0:1]
    f[2], f[3], f[4] = float(zp), float(qmin), float(qmax)
    r[5] = 1
    return r


def layer(seed, N, H, W, C, K, R, S, za, zw, depthwise=False):
    """Random codes of one layer: a [N,H,W,C] uint8, the fp32 weights whose codes are uniform in [1, 255] ([K,R,S,C],
    depthwise [R,S,C]), a bias that centres the accumulator's mean plus a few output steps, and the three records (scales
    that spread r over a few units around 0, so relu and relu6 both cut and the codes spread)."""
    g = torch.Generator().manual_seed(seed)
    n = R * S * (1 if depthwise else C)
    sa, so = 0.0235, 0.1
    sw = 5.0 / (sa * math.sqrt(n) * 1e4)  # (sigma of one product: 5e3 .. 1.4e4 with the zero points; of r: 3 .. 7)
    a = torch.randint(0, 256, (N, H, W, C), generator=g, dtype=torch.uint8)
    wshape = (R, S, C) if depthwise else (K, R, S, C)
    w = (torch.randint(1, 256, wshape, generator=g).float() - zw) * sw
    bias = torch.randn(C if depthwise else K, generator=g) * 2.0 - n * (127.5 - za) * (128 - zw) * sa * sw
    return a, w, bias, rec(sa, za), rec(sw, zw, 1, 255), rec(so, 100)


def tiny_net(x, is_training=False):
    """Two depthwise layers (stride 2, stride 1) and a 1x1 conv, each with folded BatchNorm and relu6."""
    with slim.arg_scope([slim.conv2d, slim.separable_conv2d], activation_fn=slim.relu6,
                        normalizer_fn=slim.batch_norm, normalizer_params=dict(scale=True, is_training=is_training)):
        with slim.variable_scope("t"):
            net = slim.separable_conv2d(x, None, 3, stride=2, scope="dw1")
            net = slim.separable_conv2d(net, None, 3, stride=1, scope="dw2")
            return slim.conv2d(net, 24, 1, scope="pw")


def tiny_model(C=40, size=9):
    """``tiny_net`` under QuantConfig(integer=True) with seeded BatchNorm statistics and quantiser ranges."""
    torch.manual_seed(3)
    m = SlimModel(tiny_net, size, in_channels=C, quantize=Q.QuantConfig(is_training=False, fused=True, integer=True))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, v in m.store.vars.items():
            if n.endswith(("moving_mean", "beta")):
                v.copy_(torch.randn(v.shape, generator=g) * 0.5)
            elif n.endswith(("moving_variance", "gamma")):
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            elif n.endswith("weights_quant/min"):
                v.fill_(-0.9)
            elif n.endswith("weights_quant/max"):
                v.fill_(1.3)
    invalidate_weight_copies(m.parameters())
    return m


def tiny_input(m, C=40, size=9, device="cpu"):
    """The net's input handed over as codes: the dequantised values with ``.q8`` attached."""
    g = torch.Generator().manual_seed(6)
    codes = torch.randint(0, 256, (2, size, size, C), generator=g, dtype=torch.uint8).to(device)
    st = FQ.QuantizerState(torch.device(device))
    st.rec.copy_(rec(0.0235, 3))
    from distributed_tensorflow_models_amd.ops import int8
    x = int8.dequantize_u8(codes, st.rec, torch.bfloat16 if codes.is_cuda else torch.float32)
    x.q8 = (codes, st)
    return x
