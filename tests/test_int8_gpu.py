"""The int8 kernels (csrc/kernels/int8.hip) against the torch integer form of ops/int8.py on the CPU: codes and the
dequantised copy bit for bit, no tolerance anywhere."""
import itertools

import pytest
import torch

from distributed_tensorflow_models_amd.ops import int8
from distributed_tensorflow_models_amd.ops.nn import invalidate_weight_copies
from int8_cases import layer, rec, tiny_input, tiny_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ACTS = (None, "relu", "relu6")
DEQS = (torch.bfloat16, torch.float32)
ZS = (0, 37, 255)
ZWS = (1, 128, 255)


def _both(fn, a, w, bias, ra, rw, ro, depthwise, stride, act, deq):
    """The layer on the CPU and on the GPU; both results must be the same bits."""
    out = []
    for dev in ("cpu", DEV):
        ra_, rw_, ro_ = (r.to(dev) for r in (ra, rw, ro))
        qw = int8.prepare_weights(w.to(dev), rw_, depthwise)
        out.append(fn(a.to(dev), ra_, qw, bias.to(dev), ro_, stride, "SAME", act, deq))
    (c0, d0), (c1, d1) = out
    assert c1.dtype == torch.uint8 and d1.dtype == deq and c1.shape == c0.shape
    assert torch.equal(c0, c1.cpu()), "codes differ at %d of %d" % (int((c0 != c1.cpu()).sum()), c0.numel())
    assert torch.equal(d0, d1.cpu())
    return c0


# M = N*H*W: 25 (inside one 32-pixel wave tile) and 130 (across 64-pixel block tiles); K: one channel tile, a partial
# one, more than one 128-channel block; reduction 16, 80 (no multiple of 64) and 3*3*48
@pytest.mark.parametrize("i,case", list(enumerate(itertools.product(
    ((1, 5, 5), (2, 5, 13)), (16, 24, 136), ((1, 16), (1, 80), (3, 48))))))
def test_conv(i, case):
    (N, H, W), K, (R, C) = case
    a, w, bias, ra, rw, ro = layer(i, N, H, W, C, K, R, R, ZS[i % 3], ZWS[(i // 3) % 3])
    codes = _both(int8.conv2d_q8, a, w, bias, ra, rw, ro, False, 1, ACTS[i % 3], DEQS[i % 2])
    assert len(torch.unique(codes)) > 8


@pytest.mark.parametrize("H", (5, 6))
@pytest.mark.parametrize("za", ZS)
def test_conv_3x3_stride2_border(H, za):
    """SAME padding of both asymmetries; the border taps are filled with z_a on load."""
    a, w, bias, ra, rw, ro = layer(40 + H, 2, H, H, 16, 16, 3, 3, za, 128)
    _both(int8.conv2d_q8, a, w, bias, ra, rw, ro, False, 2, "relu", torch.bfloat16)


def test_conv_largest_accumulator_and_refusal():
    """All-255 codes on both sides with zero points 0 at R*S*C = 32768: acc = 255 * 255 * 32768 in every output; the
    bias spreads the codes.  One 16-channel chunk more is refused with -2."""
    C, K = 32768, 16
    a = torch.full((1, 5, 5, C), 255, dtype=torch.uint8)
    w = torch.full((K, 1, 1, C), 255.0)
    bias = -torch.arange(K, dtype=torch.float32) * 2.0 ** 23
    codes = _both(int8.conv2d_q8, a, w, bias, rec(1.0, 0), rec(1.0, 0), rec(2.0 ** 23, 0), False, 1, None,
                  torch.float32)
    assert codes[0, 0, 0].tolist() == [254 - k for k in range(K)]
    with pytest.raises(RuntimeError, match=r"dtm_q8_prepare_weights failed \(-2\)"):
        int8.prepare_weights(torch.zeros(K, 1, 1, C + 16, device=DEV), rec(1.0, 0).to(DEV))
    qw = int8.prepare_weights(w.to(DEV), rec(1.0, 0).to(DEV))
    qw.shape = (K, 1, 1, C + 16)
    with pytest.raises(RuntimeError, match=r"dtm_q8_conv failed \(-2\)"):
        int8.conv2d_q8(torch.zeros(1, 1, 1, C + 16, dtype=torch.uint8, device=DEV), rec(1.0, 0).to(DEV), qw,
                       bias.to(DEV), rec(1.0, 0).to(DEV))


@pytest.mark.parametrize("i,case", list(enumerate(itertools.product((16, 40), (1, 2), (5, 6)))))
def test_depthwise(i, case):
    C, stride, H = case
    a, w, bias, ra, rw, ro = layer(60 + i, 2, H, H, C, C, 3, 3, ZS[i % 3], ZWS[(i // 2) % 3], depthwise=True)
    codes = _both(int8.depthwise_q8, a, w, bias, ra, rw, ro, True, stride, ACTS[i % 3], DEQS[i % 2])
    assert len(torch.unique(codes)) > 8


@pytest.mark.parametrize("n", (1, 15, 4099))
@pytest.mark.parametrize("dtype", DEQS)
def test_quantize_dequantize_misaligned(n, dtype):
    """Both buffers start one element past a 16-byte boundary."""
    g = torch.Generator().manual_seed(n)
    r = rec(0.0235, 37)
    x = (torch.rand(n, generator=g) * 8.0 - 1.5).to(dtype)
    xb = torch.zeros(n + 17, dtype=dtype, device=DEV)
    cb = torch.full((n + 17,), 7, dtype=torch.uint8, device=DEV)
    assert xb.data_ptr() % 16 == 0 and cb.data_ptr() % 16 == 0
    xb[1:n + 1].copy_(x)
    int8.quantize_u8_into(xb[1:n + 1], cb[1:n + 1], r.to(DEV))
    want = int8.quantize_u8(x, r)
    assert torch.equal(cb[1:n + 1].cpu(), want) and int(cb[0]) == 7 and bool((cb[n + 1:] == 7).all())
    yb = torch.full((n + 17,), 3.0, dtype=dtype, device=DEV)
    int8.dequantize_u8(cb[1:n + 1], r.to(DEV), out=yb[1:n + 1])
    assert torch.equal(yb[1:n + 1].cpu(), int8.dequantize_u8(want, r, dtype))
    assert float(yb[0]) == 3.0 and bool((yb[n + 1:] == 3.0).all())
    assert torch.equal(int8.quantize_u8(x.to(DEV), r.to(DEV)).cpu(), want)  # (an aligned result: element-wise path)


def test_weight_cache_follows_weights_version():
    a, w, bias, ra, rw, ro = (t.to(DEV) for t in layer(80, 1, 5, 5, 16, 16, 1, 1, 37, 128))
    p = torch.nn.Parameter(w)
    run = lambda: int8.conv2d_q8(a, ra, int8.prepare_weights(p, rw), bias, ro)  # noqa: E731
    c0 = run()
    with torch.no_grad():
        p.neg_()
    assert torch.equal(run(), c0)  # (the prepared copy of the old version)
    invalidate_weight_copies([p])
    c1 = run()
    assert not torch.equal(c1, c0)
    assert torch.equal(c1, int8.conv2d_q8(a, ra, int8.prepare_weights(p.detach(), rw), bias, ro))


def test_slim_net_equals_cpu_run():
    outs = []
    for dev in ("cpu", DEV):
        m = tiny_model().to(dev)
        invalidate_weight_copies(m.parameters())
        int8.reset_layers()
        with torch.no_grad():
            y = m(tiny_input(m, device=dev), training=False)
        assert int8.layers_run() == 3
        outs.append((y.q8[0].cpu(), y.float().cpu()))
    assert torch.equal(outs[0][0], outs[1][0])
    # (the CPU run's dequantised copy is fp32, the GPU's bf16: the same values once rounded)
    assert torch.equal(outs[0][1].to(torch.bfloat16).float(), outs[1][1])
