"""Block-output BN-apply formed inside the next unit's conv1 forward (feature blockout_conv_fuse,
conv_nt_kernel's block-output prologue, dtm_conv_fwd_bn_blockout).

The fused call must reproduce the two-kernel path (dtm_bn_apply2, then dtm_conv_fwd_bn on the same tile) bit for bit
under deterministic reductions: it computes y in bn_apply_fast's operation order and convolves the same bf16 y.
Against the fp32 reference the bound is the conv tests' (tests/test_kernels_gpu.py: relative L2 error < 1e-2)."""
import ctypes

import pytest
import torch

from distributed_tensorflow_models_amd.ops import _lib, features, fused
from distributed_tensorflow_models_amd.ops import reference as ref
from distributed_tensorflow_models_amd.ops.lazy import DeferredBlockOut, as_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, DECAY = 1e-5, 0.997


def _rel(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.fixture
def deterministic():
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(False)
        _lib.lib().dtm_conv_set_tile(-1)
        _lib.lib().dtm_conv_set_blockout(-1, 1)


def _inputs(N, H, C, K, res_mode, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {
        "raw3": (r(N, H, H, C) * 1.5).to(DEV, torch.bfloat16),
        "res": r(N, H, H, C).to(DEV, torch.bfloat16),
        "w": (r(K, 1, 1, C) * (2.0 / C) ** 0.5).to(DEV, torch.bfloat16),
        "gamma": (torch.rand(K, generator=g) + 0.5).to(DEV),
        "beta": (r(K) * 0.1).to(DEV),
    }
    ss3 = torch.zeros(4, C)
    ss3[0] = torch.rand(C, generator=g) + 0.5
    ss3[1] = r(C) * 0.3
    t["ss3"] = ss3.to(DEV)
    if res_mode == 2:
        rss = torch.zeros(4, C)
        rss[0] = torch.rand(C, generator=g) + 0.5
        rss[1] = r(C) * 0.3
        t["rss"] = rss.to(DEV)
    else:
        t["rss"] = None
    return t


def _run(t, N, H, C, K, res_mode, fusedcall):
    """-> (rc, y, mask, raw1, ss, moving_mean, moving_var); y / mask start as a sentinel."""
    L = _lib.lib()
    s = _lib.stream_ptr()
    M = N * H * H
    y = torch.full((N, H, H, C), -7.0, device=DEV, dtype=torch.bfloat16)
    mask = torch.full((M * C // 8,), 0xA5, device=DEV, dtype=torch.uint8)
    raw1 = torch.full((N, H, H, K), -7.0, device=DEV, dtype=torch.bfloat16)
    ss = torch.zeros(4, K, device=DEV)
    mm, mv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
    d = _lib.ConvDesc(N, H, H, C, K, 1, 1, H, H, 1, 0, 0, 0, 0)
    P = _lib.ptr
    if fusedcall:
        rc = L.dtm_conv_fwd_bn_blockout(P(t["raw3"]), P(t["ss3"]), P(t["res"]), P(t["rss"]), P(y), P(mask), P(t["w"]),
                                        P(raw1), P(t["gamma"]), P(t["beta"]), P(mm), P(mv), P(ss), float(M), EPS, DECAY,
                                        1, 1, ctypes.byref(d), s)
    else:
        rc = L.dtm_bn_apply2(P(t["raw3"]), P(t["ss3"]), P(t["res"]), P(t["rss"]), P(y), P(mask), M, C, res_mode, 1, s)
        assert rc == 0
        rc = L.dtm_conv_fwd_bn(P(y), P(t["w"]), P(raw1), None, None, P(t["gamma"]), P(t["beta"]), P(mm), P(mv), P(ss),
                               float(M), EPS, DECAY, 1, 1, ctypes.byref(d), s)
    torch.cuda.synchronize()
    return rc, y, mask, raw1, ss, mm, mv


def _reference(t, res_mode, ss):
    """fp32: y, its ReLU bits, the conv of the bf16-rounded y, and the BN scale / shift of that conv's output."""
    C = t["raw3"].shape[-1]
    f = t["raw3"].float() * t["ss3"][0] + t["ss3"][1]
    r = t["res"].float()
    f = f + (r * t["rss"][0] + t["rss"][1] if res_mode == 2 else r)
    y = torch.relu(f)
    raw1 = ref.conv2d(y.to(torch.bfloat16).float(), t["w"].float(), None, 1, "SAME")
    q = raw1.to(torch.bfloat16).float().reshape(-1, raw1.shape[-1])
    mean, var = q.mean(0), q.var(0, unbiased=False)
    scale = t["gamma"] * torch.rsqrt(var + EPS)
    shift = t["beta"] - mean * scale
    assert C % 8 == 0
    return y, f > 0, raw1, scale, shift


def _unpack_bits(mask, shape):
    b = (mask.view(-1, 1).to(torch.int32) >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return b.reshape(shape).bool()


# ragged single tile (M = 98), ragged multi-tile (M = 243: 2 tiles of 128 rows / 4 of 64), last rows partial (M = 1)
SHAPES = [(2, 7), (3, 9), (1, 1)]


@pytest.mark.parametrize("res_mode", [1, 2])
@pytest.mark.parametrize("N,H", SHAPES)
def test_kernel_bit_identical_to_two_kernel_path(deterministic, N, H, res_mode):
    L = _lib.lib()
    for C in (64, 256, 512):  # 1 / 4 / 8 k-tiles; 512 is the LDS limit of the prologue parameters
        for K in (64, 128):
            for nt in (1, 0):
                t = _inputs(N, H, C, K, res_mode, seed=C + K)
                L.dtm_conv_set_tile(3 if K <= 64 else 4)  # the same register-staged tile on both paths
                L.dtm_conv_set_blockout(1, nt)
                rc, y, mask, raw1, ss, mm, mv = _run(t, N, H, C, K, res_mode, True)
                assert rc == 0, (C, K, rc)
                rc2, y2, mask2, raw12, ss2, mm2, mv2 = _run(t, N, H, C, K, res_mode, False)
                assert rc2 == 0
                for a, b, what in ((y, y2, "y"), (mask, mask2, "mask"), (raw1, raw12, "raw1"), (ss, ss2, "ss"),
                                   (mm, mm2, "moving_mean"), (mv, mv2, "moving_variance")):
                    assert torch.equal(a, b), (what, C, K, nt)
            yr, bits, raw1r, scale, shift = _reference(t, res_mode, ss)
            assert _rel(y, yr) < 1e-2
            assert _rel(raw1, raw1r) < 1e-2
            assert _rel(ss[0], scale) < 1e-2 and _rel(ss[1], shift) < 1e-2
            # bit e of byte (row*C + c)/8 = [y > 0] of channel c + e (a positive fp32 value stays positive in bf16),
            # and it is the sign of the fp32 reference pre-activation except within rounding of zero
            got = _unpack_bits(mask, bits.shape)
            assert torch.equal(got, y > 0)
            assert (got != bits).float().mean().item() < 1e-3


@pytest.mark.parametrize("C,K,tile,why", [(520, 64, 3, "C over the LDS limit"), (256, 256, 4, "two channel tiles"),
                                          (256, 128, 3, "two channel tiles of the 64-channel tile")])
def test_kernel_declines_and_launches_nothing(deterministic, C, K, tile, why):
    L = _lib.lib()
    N, H = 2, 7
    t = _inputs(N, H, C, K, 1)
    L.dtm_conv_set_tile(tile)
    L.dtm_conv_set_blockout(1, 1)
    rc, y, mask, raw1, ss, _, _ = _run(t, N, H, C, K, 1, True)
    assert rc == 1, why
    assert bool((y == -7).all()) and bool((mask == 0xA5).all()) and bool((raw1 == -7).all())
    # ... and the two-kernel path the caller then runs is right
    rc, y, mask, raw1, ss, _, _ = _run(t, N, H, C, K, 1, False)
    assert rc == 0
    yr, bits, raw1r, scale, shift = _reference(t, 1, ss)
    assert _rel(y, yr) < 1e-2 and _rel(raw1, raw1r) < 1e-2
    assert _rel(ss[0], scale) < 1e-2 and _rel(ss[1], shift) < 1e-2


def test_setter_off_declines(deterministic):
    L = _lib.lib()
    t = _inputs(2, 7, 256, 64, 1)
    L.dtm_conv_set_tile(3)
    L.dtm_conv_set_blockout(0, 1)
    assert _run(t, 2, 7, 256, 64, 1, True)[0] == 1


# ---- autograd: three bottleneck units, projection -> identity -> identity (BN'd and identity residuals) -------------
def _units():
    from distributed_tensorflow_models_amd.models.resnet_v1 import BottleneckV1, resnet_arg_scope
    torch.manual_seed(0)
    sc = resnet_arg_scope()
    us = [BottleneckV1("t/a", 32, 128, 32, 1, sc), BottleneckV1("t/b", 128, 128, 32, 1, sc),
          BottleneckV1("t/c", 128, 128, 32, 1, sc)]
    g = torch.Generator().manual_seed(5)
    for u in us:
        u.to(DEV)
        for n, p in u.named_parameters():
            if n.endswith("gamma") or n.endswith("beta"):
                with torch.no_grad():
                    p.add_((torch.randn(p.shape, generator=g) * 0.2).to(DEV))
    return us


def _chain(on, case):
    """One pass of the three units under ``case`` with the feature on / off -> (values, gradients, fused count)."""
    us = _units()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 5, 5, 32, generator=g).to(DEV, torch.bfloat16).requires_grad_(case != "no_grad")
    wgt = torch.randn(2, 5, 5, 128, generator=g).to(DEV)
    training = case != "eval"
    vals, grads = [], []
    with features.override(blockout_conv_fuse=on):
        c0 = fused.BLOCKOUT_FUSED[0]
        if case == "end_points":
            ep = {}
            a = us[0](x, training, ep, defer_out=True)
            assert not isinstance(a, DeferredBlockOut)
            out = us[2](us[1](a, training, ep, defer_out=True), training, ep)
            vals += [ep[k] for k in sorted(ep)]
        elif case == "no_grad":
            with torch.no_grad():
                a = us[0](x, training, defer_out=True)
                assert isinstance(a, DeferredBlockOut) == on
                out = as_tensor(us[2](us[1](a, training, defer_out=True), training))
        elif case == "other_first":
            # the deferred output is read first by a non-conv op: the ordinary BN-apply fills it, the conv reads it plainly
            a = us[0](x, training, defer_out=True)
            assert isinstance(a, DeferredBlockOut) == on
            side = as_tensor(a).float().sum()
            if on:
                assert a.filled
            out = us[2](us[1](as_tensor(a), training), training)
            vals.append(side.detach())
            out = out.float() + side * 1e-3
        else:  # "train" / "eval": read by the conv, then as the next unit's identity residual
            a = us[0](x, training, defer_out=True)
            assert isinstance(a, DeferredBlockOut) == (on and training)
            b = us[1](a, training, defer_out=True)
            if on and training:
                assert a.filled and isinstance(b, DeferredBlockOut) and not b.filled
            out = as_tensor(us[2](b, training))
        count = fused.BLOCKOUT_FUSED[0] - c0
        vals.append(out.detach())
        if case != "no_grad":
            (out.float() * wgt).sum().backward()
            grads.append(x.grad)
            for u in us:
                grads += [p.grad for _, p in sorted(u.named_parameters())]
        for u in us:
            vals += [b.detach().clone() for _, b in sorted(u.named_buffers())]
    torch.cuda.synchronize()
    return vals, grads, count


@pytest.mark.parametrize("case,want", [("train", 2), ("other_first", 0), ("no_grad", 2), ("eval", 0),
                                       ("end_points", 0)])
def test_autograd_pair_bit_identical_on_and_off(deterministic, case, want):
    v1, g1, c1 = _chain(True, case)
    v0, g0, c0 = _chain(False, case)
    assert c1 == want and c0 == 0
    assert len(v1) == len(v0) and len(g1) == len(g0)
    for a, b in zip(v1, v0):
        assert torch.equal(a, b)
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)
    if case == "train":
        assert all(g is not None for g in g1)


def test_autograd_values_against_fp32_reference(deterministic):
    """The fused pair (block-output apply -> conv1) against the fp32 reference, through the Python ops."""
    from distributed_tensorflow_models_amd.ops.lazy import LazyBN
    N, H, C, K = 3, 9, 256, 64
    t = _inputs(N, H, C, K, 1, seed=3)
    from distributed_tensorflow_models_amd.models.layers import Conv2d
    from distributed_tensorflow_models_amd.models.resnet_v1 import resnet_arg_scope
    sc = resnet_arg_scope()
    conv = Conv2d("t/conv1", C, K, 1, 1, "SAME", "relu", sc["normalizer"], None, 0.0, sc["init"]).to(DEV)
    t["w"] = conv.weights.detach().to(torch.bfloat16)
    t["gamma"], t["beta"] = conv.bn.gamma.detach(), conv.bn.beta.detach()
    c0 = fused.BLOCKOUT_FUSED[0]
    with features.override(blockout_conv_fuse=True):
        lz = LazyBN(t["raw3"].clone().requires_grad_(), t["ss3"], False, unscaled=True)
        y = lz.materialize(residual=t["res"].clone().requires_grad_(), residual_act="relu", defer=True)
        assert isinstance(y, DeferredBlockOut)
        out = conv(y, True)
    assert fused.BLOCKOUT_FUSED[0] - c0 == 1 and y.filled
    yr, bits, raw1r, scale, shift = _reference(t, 1, None)
    assert _rel(as_tensor(y), yr) < 1e-2
    assert _rel(out.raw, raw1r) < 1e-2
    assert _rel(out.ss[0], scale) < 1e-2 and _rel(out.ss[1], shift) < 1e-2


def test_declined_conv_fills_by_bn_apply(deterministic):
    """Two channel tiles (K = 256): the conv declines, the ordinary BN-apply fills y first; values right, count 0."""
    from distributed_tensorflow_models_amd.models.layers import Conv2d
    from distributed_tensorflow_models_amd.models.resnet_v1 import resnet_arg_scope
    from distributed_tensorflow_models_amd.ops.lazy import LazyBN
    N, H, C, K = 2, 7, 256, 256
    t = _inputs(N, H, C, K, 2, seed=4)
    sc = resnet_arg_scope()
    conv = Conv2d("t/conv1", C, K, 1, 1, "SAME", "relu", sc["normalizer"], None, 0.0, sc["init"]).to(DEV)
    t["w"] = conv.weights.detach().to(torch.bfloat16)
    t["gamma"], t["beta"] = conv.bn.gamma.detach(), conv.bn.beta.detach()
    c0 = fused.BLOCKOUT_FUSED[0]
    with features.override(blockout_conv_fuse=True):
        lz = LazyBN(t["raw3"].clone().requires_grad_(), t["ss3"], False, unscaled=True)
        res = LazyBN(t["res"].clone().requires_grad_(), t["rss"], False, unscaled=True)
        y = lz.materialize(residual=res, residual_act="relu", defer=True)
        assert isinstance(y, DeferredBlockOut)
        out = conv(y, True)
    assert fused.BLOCKOUT_FUSED[0] == c0 and y.filled
    yr, bits, raw1r, scale, shift = _reference(t, 2, None)
    assert _rel(as_tensor(y), yr) < 1e-2 and _rel(out.raw, raw1r) < 1e-2


# ---- model: one deterministic TrainStep of a small ResNet, feature on / off ---------------------------------------
def _train_once(on):
    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models.resnet_v1 import ResNetV1
    torch.manual_seed(0)
    net = ResNetV1(blocks=[(16, 3, 2), (32, 2, 1)], num_classes=10).to(DEV)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 32, 32, 3, generator=g).to(DEV, torch.bfloat16)
    y = torch.randint(0, 10, (2,), generator=g).to(DEV)
    with features.override(blockout_conv_fuse=on):
        step = TrainStep(net, optimizer="momentum", lr=0.05, momentum=0.9)
        c0 = fused.BLOCKOUT_FUSED[0]
        loss = float(step(x, y))
        torch.cuda.synchronize()
        count = fused.BLOCKOUT_FUSED[0] - c0
    state = [p.detach().clone() for p in net.parameters()] + [b.detach().clone() for b in net.buffers()]
    step.dp.close()
    return loss, state, count


def test_model_train_step_bit_identical_on_and_off(deterministic):
    l1, s1, c1 = _train_once(True)
    l0, s0, c0 = _train_once(False)
    assert c1 > 0 and c0 == 0
    assert l1 == l0
    assert len(s1) == len(s0)
    for a, b in zip(s1, s0):
        assert torch.equal(a, b)


def test_resnet50_fuses_five_transitions_per_forward():
    """ResNet-50: block 1 u1->u2, u2->u3 and block 2 u1->u2, u2->u3, u3->u4 (blocks 3 / 4 run LDS-DMA tiles)."""
    from distributed_tensorflow_models_amd.models import nets_factory
    torch.manual_seed(0)
    net = nets_factory.build("resnet_v1_50", num_classes=10).to(DEV)
    x = torch.randn(2, 64, 64, 3, device=DEV).to(torch.bfloat16)
    c0 = fused.BLOCKOUT_FUSED[0]
    out = net(x, True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    assert fused.BLOCKOUT_FUSED[0] - c0 == 5
