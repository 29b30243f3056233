"""The LDS-tiled depthwise kernels (impl="tile") against the float64 CPU reference: forward, dgrad and wgrad bit for
bit on ternary inputs, arithmetic bounds on random ones, and the public slim layer reaching them under "auto"."""
import pytest
import torch

from distributed_tensorflow_models_amd.compat import slim
from distributed_tensorflow_models_amd.ops import reference as ref
from distributed_tensorflow_models_amd.ops.depthwise import depthwise_conv2d
from distributed_tensorflow_models_amd.ops.lazy import as_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (N, H, W, C, (R, S), stride, padding)
EXACT = [
    (1, 5, 5, 8, (3, 3), 1, "SAME"),       # smaller than any tile, one channel column
    (2, 9, 11, 24, (3, 3), 1, "SAME"),     # three columns, H != W
    (3, 15, 15, 96, (3, 3), 2, "SAME"),    # odd extent, symmetric SAME pad at stride 2, slab tail
    (2, 16, 16, 144, (3, 3), 2, "SAME"),   # even extent: pad on the bottom / right only
    (2, 19, 21, 40, (5, 5), 1, "SAME"),    # 5x5 taps
    (1, 18, 18, 16, (7, 7), 2, "VALID"),   # row and column 17 are touched by no output: dx there is +0
    (2, 9, 9, 264, (3, 3), 1, "VALID"),    # 33 columns
    (4, 33, 35, 32, (3, 3), 1, "SAME"),    # a fast8 shape forced onto the tile; 60 wgrad tiles = 60 blocks
]
RANDOM = (2, 13, 13, 96, (3, 3), 1, "SAME")


def _run(x, w, dy, st, pad, **kw):
    """One forward + backward: (y, dx, dw).  CPU float64 tensors run the reference, the others the op under test."""
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = (ref.depthwise_conv2d if x.dtype == torch.float64 else depthwise_conv2d)(x, w, st, pad, **kw)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


def _case(case, ternary):
    N, H, W, C, (R, S), st, pad = case
    g = torch.Generator().manual_seed(C * 131 + H)
    draw = (lambda s: torch.randint(-1, 2, s, generator=g).double()) if ternary else \
        (lambda s: torch.randn(s, generator=g).to(BF).double())
    x, w = draw((N, H, W, C)), draw((R, S, C, 1))
    dy = draw(tuple(ref.depthwise_conv2d(x, w, st, pad).shape))
    return x, w, dy, st, pad


def _gpu(x, w, dy, st, pad, **kw):
    out = _run(x.to(DEV, BF), w.float().to(DEV), dy.to(DEV, BF), st, pad, **kw)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "%dx%dx%dx%d-%dx%d-s%d-%s" % (c[:4] + c[4] + c[5:]))
def test_tile_exact(case):
    x, w, dy, st, pad = _case(case, ternary=True)
    yr, dxr, dwr = _run(x, w, dy, st, pad)
    assert max(yr.abs().max(), dxr.abs().max()) <= 49 and dwr.abs().max() < 2 ** 24
    y, dx, dw = _gpu(x, w, dy, st, pad, impl="tile")
    assert torch.equal(y, yr.to(BF)) and torch.equal(dx, dxr.to(BF)) and torch.equal(dw, dwr.float())
    if pad == "VALID" and st == 2:  # the leftover row and column: +0, not -0
        assert not torch.signbit(dx[:, -1]).any() and not torch.signbit(dx[:, :, -1]).any()
        assert dx[:, -1].count_nonzero() == 0 and dx[:, :, -1].count_nonzero() == 0


def test_tile_random_bounds_and_repeatable():
    x, w, dy, st, pad = _case(RANDOM, ternary=False)
    yr, dxr, dwr = _run(x, w, dy, st, pad)
    ya, dxa, dwa = _run(x.abs(), w.abs(), dy.abs(), st, pad)  # sum |x||w|, sum |dy||w|, sum |x||dy|
    y, dx, dw = _gpu(x, w, dy, st, pad, impl="tile")
    npq = yr.shape[0] * yr.shape[1] * yr.shape[2]
    # one bf16 rounding + fp32 accumulation over <= 9 taps; any-order fp32 summation over N*P*Q products
    assert ((y.double() - yr).abs() <= 2.0 ** -8 * ya).all()
    assert ((dx.double() - dxr).abs() <= 2.0 ** -8 * dxa).all()
    assert ((dw.double() - dwr).abs() <= npq * 2.0 ** -24 * dwa).all()
    assert torch.equal(_gpu(x, w, dy, st, pad, impl="tile")[2], dw)


def test_slim_auto_reaches_tile():
    x, w, dy, st, pad = _case((2, 14, 14, 96, (3, 3), 1, "SAME"), ternary=False)
    store = slim.VariableStore()
    store.device = DEV
    with slim.use_store(store):
        slim.begin_pass()
        xs = x.to(DEV, BF).requires_grad_()
        ys = as_tensor(slim.separable_conv2d(xs, None, 3, activation_fn=None, biases_initializer=None, scope="dw"))
    (ws,) = store.vars.values()
    ys.backward(dy.to(DEV, BF))
    y, dx, dw = _gpu(x, ws.detach().double().cpu(), dy, st, pad, impl="tile")
    assert torch.equal(ys.detach().cpu(), y) and torch.equal(xs.grad.cpu(), dx) and torch.equal(ws.grad.cpu(), dw)
