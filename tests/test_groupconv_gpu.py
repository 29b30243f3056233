"""The grouped 3x3 MFMA kernels against the float64 CPU reference: forward, dgrad and wgrad bit for bit on ternary
inputs, arithmetic bounds and repeatability on random ones, the slim layer reaching them, and a tiny ResNeXt step."""
import pytest
import torch

from distributed_tensorflow_models_amd.compat import slim
from distributed_tensorflow_models_amd.models import slim_nets
from distributed_tensorflow_models_amd.models.slim_model import SlimModel
from distributed_tensorflow_models_amd.ops import reference as ref
from distributed_tensorflow_models_amd.ops.groupconv import grouped_conv2d
from distributed_tensorflow_models_amd.ops.lazy import as_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# (N, H, W, C, D, stride, padding)
EXACT = [
    (1, 5, 5, 16, 4, 1, "SAME"),       # smaller than any tile, one column of four groups
    (2, 9, 11, 48, 8, 1, "SAME"),      # a 48-channel tail chunk, H != W
    (2, 15, 15, 64, 16, 2, "SAME"),    # odd extent at stride 2
    (2, 16, 16, 96, 32, 2, "SAME"),    # even extent: pad on the bottom / right only; 3 groups over a 64 + 32 split
    (1, 18, 18, 32, 4, 2, "VALID"),    # row and column 17 reach no output: dx there is +0
    (3, 33, 35, 160, 8, 1, "SAME"),    # many tiles, three chunks, several wgrad partial rows
    (2, 7, 7, 192, 32, 1, "SAME"),     # a map smaller than a tile at D = 32
    (2, 12, 10, 80, 16, 1, "VALID"),   # no padding
]
RANDOM = [(2, 13, 13, 96, 8, 1, "SAME"), (2, 13, 13, 96, 32, 2, "SAME")]
_ID = lambda c: "%dx%dx%dx%d-D%d-s%d-%s" % c  # noqa: E731


def _run(x, w, dy, groups, st, pad):
    """One forward + backward: (y, dx, dw).  CPU float64 tensors run the reference, the others the op under test."""
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = (ref.grouped_conv2d if x.dtype == torch.float64 else grouped_conv2d)(x, w, groups, st, pad)
    y.backward(dy)
    return y.detach(), x.grad, w.grad


def _case(case, ternary):
    N, H, W, C, D, st, pad = case
    g = torch.Generator().manual_seed(C * 131 + H)
    draw = (lambda s: torch.randint(-1, 2, s, generator=g).double()) if ternary else \
        (lambda s: torch.randn(s, generator=g).to(BF).double())
    x, w = draw((N, H, W, C)), draw((C, 3, 3, D))
    dy = draw(tuple(ref.grouped_conv2d(x, w, C // D, st, pad).shape))
    return x, w, dy, C // D, st, pad


def _gpu(x, w, dy, groups, st, pad):
    out = _run(x.to(DEV, BF), w.float().to(DEV), dy.to(DEV, BF), groups, st, pad)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@pytest.mark.parametrize("case", EXACT, ids=_ID)
def test_exact(case):
    args = _case(case, ternary=True)
    yr, dxr, dwr = _run(*args)
    assert max(yr.abs().max(), dxr.abs().max()) <= 256 and dwr.abs().max() < 2 ** 24
    y, dx, dw = _gpu(*args)
    assert torch.equal(y, yr.to(BF)) and torch.equal(dx, dxr.to(BF)) and torch.equal(dw, dwr.float())
    if case[6] == "VALID" and case[5] == 2:  # the leftover row and column: +0, not -0
        assert not torch.signbit(dx[:, -1]).any() and not torch.signbit(dx[:, :, -1]).any()
        assert dx[:, -1].count_nonzero() == 0 and dx[:, :, -1].count_nonzero() == 0


@pytest.mark.parametrize("case", RANDOM, ids=_ID)
def test_random_bounds_and_repeatable(case):
    args = _case(case, ternary=False)
    yr, dxr, dwr = _run(*args)
    ya, dxa, dwa = _run(*(t.abs() for t in args[:3]), *args[3:])  # sum |x||w|, sum |dy||w|, sum |x||dy|
    y, dx, dw = _gpu(*args)
    npq = yr.shape[0] * yr.shape[1] * yr.shape[2]
    # one bf16 rounding + fp32 accumulation over <= 288 exact products; any-order fp32 summation over N*P*Q
    # products, doubled for the MFMA's undocumented internal summation order
    assert ((y.double() - yr).abs() <= 2.0 ** -8 * ya).all()
    assert ((dx.double() - dxr).abs() <= 2.0 ** -8 * dxa).all()
    assert ((dw.double() - dwr).abs() <= npq * 2.0 ** -23 * dwa).all()
    assert torch.equal(_gpu(*args)[2], dw)


def test_slim_layer_reaches_the_kernels():
    x, w, dy, groups, st, pad = _case((2, 14, 14, 96, 8, 1, "SAME"), ternary=False)
    store = slim.VariableStore()
    store.device = DEV
    with slim.use_store(store):
        slim.begin_pass()
        xs = x.to(DEV, BF).requires_grad_()
        ys = as_tensor(slim.grouped_conv2d(xs, 96, 3, groups, activation_fn=None, biases_initializer=None, scope="g"))
    (ws,) = store.vars.values()
    ys.backward(dy.to(DEV, BF))
    y, dx, dw = _gpu(x, ws.detach().double().cpu(), dy, groups, st, pad)
    assert torch.equal(ys.detach().cpu(), y) and torch.equal(xs.grad.cpu(), dx) and torch.equal(ws.grad.cpu(), dw)


def test_tiny_resnext_step():
    torch.manual_seed(0)
    model = SlimModel(slim_nets.resnext, 64, num_classes=10, name="resnext", blocks=(1, 1, 1, 1), cardinality=4,
                      base_width=4).to(DEV)
    logits = as_tensor(model(torch.randn(2, 64, 64, 3, device=DEV), training=True))
    loss = torch.nn.functional.cross_entropy(logits.float(), torch.tensor([3, 7], device=DEV))
    loss.backward()
    assert torch.isfinite(loss)
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.count_nonzero() > 0, n
