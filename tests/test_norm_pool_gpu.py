"""The BatchNorm, pooling and LRN kernels (csrc/kernels/batchnorm.hip, pool.hip, lrn.hip) against the float64
references of tests/norm_pool_cases.py: bit for bit where the exact answer is representable (integer statistics, max
pools, first-maximum gradients, power-of-two averages), per element inside the bounds derived there everywhere else.
Every assertion covers every element."""
import ctypes

import pytest
import torch

import norm_pool_cases as NP
from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops import lrn as dlrn
from distributed_tensorflow_models_amd.ops import nn as dnn
from distributed_tensorflow_models_amd.ops.geometry import pool_geom

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F64 = torch.bfloat16, torch.float64
BN_NAMES = list(NP.BN_CASES)


def _cpu64(t):
    torch.cuda.synchronize()
    return t.detach().cpu().to(F64)


def _inside(got, want, tol, what):
    err = (_cpu64(got) - want).abs()
    bad = ~(err <= tol)  # (a NaN is outside)
    assert not bad.any(), "%s: %d of %d elements outside the bound, worst |err| / bound = %.3g" % (
        what, int(bad.sum()), bad.numel(), float((err / tol.clamp(min=1e-300))[bad].max()))


# ---- BatchNorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BN_NAMES)
def test_bn_statistics_bit_exact(name):
    x64, sums = NP.bn_exact_input(name)
    assert sums.abs().max() < NP.SUM_LIMIT
    C = x64.shape[-1]
    M = x64.numel() // C
    L, s = _lib.lib(), _lib.stream_ptr()
    x = x64.to(DEV, BF).contiguous()
    stats = torch.zeros(2, C, device=DEV)
    L.dtm_bn_stats(_lib.ptr(x), _lib.ptr(stats), M, C, s)
    assert torch.equal(_cpu64(stats), sums)
    det = torch.zeros(2, C, device=DEV)
    rc = L.dtm_col_sums(_lib.ptr(x), _lib.ptr(det), M, C, s)
    assert rc == (0 if NP.fast_ok(M, C) else -1)
    if rc == 0:
        assert torch.equal(_cpu64(det), sums)
    # through the public op: decay 0 from a zero moving mean leaves exactly fl32(sum / M)
    mm, mv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    dnn.batch_norm(x, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), mm, mv, True, 0.0, NP.EPS)
    torch.cuda.synchronize()
    assert torch.equal(mm.cpu(), sums[0].float() / torch.tensor(float(M)))


def _bn_run(name, relu, res, bessel, backward):
    inp = NP.bn_random_input(name)
    r64 = inp.res if res else None
    f = NP.bn_forward64(inp.x, inp.gamma, inp.beta, r64, relu, inp.mm, inp.mv, bessel)
    x = inp.x.to(DEV, BF).requires_grad_(backward)
    gm, bt = (t.to(DEV, torch.float32).requires_grad_(backward) for t in (inp.gamma, inp.beta))
    r = inp.res.to(DEV, BF).requires_grad_(backward) if res else None
    mm, mv = inp.mm.to(DEV, torch.float32), inp.mv.to(DEV, torch.float32)
    y = dnn.batch_norm(x, gm, bt, mm, mv, True, NP.DECAY, NP.EPS, relu, r, bessel)
    return inp, f, x, gm, bt, r, mm, mv, y


@pytest.mark.parametrize("relu,res,bessel", [(False, False, True), (True, True, False), (True, False, True)],
                         ids=["plain-bessel", "relu-res", "relu-bessel"])
@pytest.mark.parametrize("name", BN_NAMES + [NP.BN_COND])
def test_bn_forward_per_element(name, relu, res, bessel):
    inp, f, _, _, _, _, mm, mv, y = _bn_run(name, relu, res, bessel, False)
    assert y.dtype == BF and tuple(y.shape) == tuple(inp.x.shape)
    _inside(y, f.y, f.tol, "y")
    _inside(mm, f.mm, f.mm_tol, "moving_mean")
    _inside(mv, f.mv, f.mv_tol, "moving_var")


@pytest.mark.parametrize("relu,res", [(False, False), (True, True)], ids=["plain", "relu-res"])
@pytest.mark.parametrize("name", BN_NAMES)
def test_bn_backward_per_element(name, relu, res):
    inp, f, x, gm, bt, r, _, _, y = _bn_run(name, relu, res, True, True)
    y.backward(inp.dy.to(DEV, BF))
    # the ReLU mask of the kernel's own output: a sign flip where |y64| is below the forward tolerance is the
    # forward's error (bounded above), not the backward's
    _inside(y, f.y, f.tol, "y")
    mask = (_cpu64(y) > 0).to(F64) if relu else None
    b = NP.bn_backward64(f, inp.x, inp.gamma, inp.dy, mask)
    _inside(x.grad, b.dx, b.dx_tol, "dx")
    _inside(bt.grad, b.dbeta, b.dbeta_tol, "dbeta")
    _inside(gm.grad, b.dgamma, b.dgamma_tol, "dgamma")
    if res:
        assert torch.equal(_cpu64(r.grad), b.g)  # the residual gradient is the masked dy itself


# ---- pooling --------------------------------------------------------------------------------------------------------
def _pool(fn, x64, dy64, *args):
    x = x64.to(DEV, BF).requires_grad_()
    y = fn(x, *args)
    y.backward(dy64.to(DEV, BF))
    return _cpu64(y), _cpu64(x.grad)


@pytest.mark.parametrize("kind", ["unique", "ties"])
@pytest.mark.parametrize("case", NP.POOL_CASES, ids=NP.pool_id)
def test_max_pool_bit_exact(case, kind):
    shape, k, s, pad = case
    x = NP.pool_input(shape, kind)
    dy = NP.pool_dy(case, -1, 1)
    yr, _, ties = NP.max_pool64(x, k, s, pad)
    assert ties == 0 if kind == "unique" else (ties > 0 or k == 1)
    dxr = NP.max_pool_bwd64(x, dy, k, s, pad)  # the whole of a window's dy to its first maximum
    assert dxr.abs().max() <= 9
    y, dx = _pool(dnn.max_pool, x, dy, k, s, pad)
    assert torch.equal(y, yr) and torch.equal(dx, dxr)


@pytest.mark.parametrize("case", NP.POOL_CASES, ids=NP.pool_id)
def test_max_pool_padding_is_minus_infinity(case):
    shape, k, s, pad = case
    x = NP.pool_input(shape, "negative")
    yr = NP.max_pool64(x, k, s, pad)[0]
    assert yr.max() <= -1
    y = dnn.max_pool(x.to(DEV, BF), k, s, pad)
    assert torch.equal(_cpu64(y), yr)


@pytest.mark.parametrize("case", [c for c in NP.POOL_CASES if c[1:3] == (3, 2) and c[0][3] % 8 == 0], ids=NP.pool_id)
def test_max_pool_backward_reads_a_channel_slice_in_place(case):
    shape, k, s, pad = case
    g = pool_geom(shape, k, s, pad)
    assert NP.pool_dispatch(g)["max_bwd"] == "k3s2"
    L, st = _lib.lib(), _lib.stream_ptr()
    a = g.as_args(_lib.PoolArgs)
    x64, dy64 = NP.pool_input(shape, "unique"), NP.pool_dy(case, -1, 1)
    x = x64.to(DEV, BF).contiguous()
    y = torch.empty((g.N, g.P, g.Q, g.C), device=DEV, dtype=BF)
    arg = torch.empty((g.N, g.P, g.Q, g.C), device=DEV, dtype=torch.uint8)
    L.dtm_maxpool_fwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(arg), ctypes.byref(a), st)
    ld = g.C + 24
    wide = torch.full((g.N, g.P, g.Q, ld), 7.0, device=DEV, dtype=BF)  # (a neighbour's gradient must not leak in)
    dy = wide[..., 8:8 + g.C]
    dy.copy_(dy64.to(DEV, BF))
    assert dnn._pixel_pitch(dy) == ld
    dx = torch.empty_like(x)
    assert L.dtm_maxpool_bwd_ld(_lib.ptr(dy), ld, _lib.ptr(arg), _lib.ptr(dx), ctypes.byref(a), st) == 0
    want = NP.max_pool_bwd64(x64, dy64, k, s, pad)
    assert torch.equal(_cpu64(dx), want)
    # and through autograd, which hands the slice to the same entry
    xg = x.clone().requires_grad_()
    dnn.max_pool(xg, k, s, pad).backward(dy)
    assert torch.equal(_cpu64(xg.grad), want)


@pytest.mark.parametrize("count_pad", [0, 1])
@pytest.mark.parametrize("case", NP.POOL_CASES, ids=NP.pool_id)
def test_avg_pool_per_element(case, count_pad):
    shape, k, s, pad = case
    x, dy = NP.pool_input(shape, "int"), NP.pool_dy(case, -3, 3, salt=1)
    yr, ytol = NP.avg_pool64(x, k, s, pad, count_pad)
    dxr, dtol = NP.avg_pool_bwd64(shape, dy, k, s, pad, count_pad)
    y, dx = _pool(dnn.avg_pool, x, dy, k, s, pad, bool(count_pad))
    _inside(y, yr, ytol, "y")
    _inside(dx, dxr, dtol, "dx")
    if k in (1, 2):  # a power-of-two divisor, one window per input pixel: exact
        assert torch.equal(y, yr) and torch.equal(dx, dxr)
    # the accumulating backward: dx += into an existing gradient, one rounding of the total
    g = pool_geom(shape, k, s, pad)
    L, st = _lib.lib(), _lib.stream_ptr()
    a = g.as_args(_lib.PoolArgs)
    main = NP.pool_input(shape, "ties")
    acc = main.to(DEV, BF).contiguous()
    dyk = dy.to(DEV, BF).contiguous()
    rc = L.dtm_avgpool_bwd_acc(_lib.ptr(dyk), _lib.ptr(acc), ctypes.byref(a), count_pad, st)
    assert rc == (-1 if NP.pool_dispatch(g)["avg_bwd_acc"] is None else 0)
    if rc == 0:
        tot, ttol = NP.avg_pool_bwd64(shape, dy, k, s, pad, count_pad, main)
        _inside(acc, tot, ttol, "main + dx")
    else:
        assert torch.equal(_cpu64(acc), main)  # refused: untouched


@pytest.mark.parametrize("C", [16, 20])
def test_avg_pool_same_divisor_excludes_padding(C):
    x = torch.full((1, 8, 8, C), 9.0, device=DEV, dtype=BF)
    y0 = _cpu64(dnn.avg_pool(x, 3, 1, "SAME", count_pad=False))
    assert torch.equal(y0, torch.full_like(y0, 9.0))  # corner / 4, edge / 6, interior / 9
    y1 = _cpu64(dnn.avg_pool(x, 3, 1, "SAME", count_pad=True))
    want = torch.full((8, 8), 9.0, dtype=F64)
    want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 6.0
    want[0, 0] = want[0, -1] = want[-1, 0] = want[-1, -1] = 4.0
    assert torch.equal(y1, want[None, :, :, None].expand(1, 8, 8, C))
    # stride 2 on 13 x 14: TF pads top 1 / left 0 / bottom 1 / right 1
    x = torch.full((2, 13, 14, C), 9.0, device=DEV, dtype=BF)
    y1 = _cpu64(dnn.avg_pool(x, 3, 2, "SAME", count_pad=True))
    assert y1[0, 0, 0, 0] == 6 and y1[1, 1, 0, 0] == 9 and y1[0, 0, 6, 0] == 4 and y1[1, 6, 6, C - 1] == 4
    y0 = _cpu64(dnn.avg_pool(x, 3, 2, "SAME", count_pad=False))
    assert torch.equal(y0, torch.full_like(y0, 9.0))


# ---- LRN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", NP.LRN_PARAMS, ids=["model", "r2-a1", "r5-a.5"])
@pytest.mark.parametrize("shape", NP.LRN_SHAPES + [NP.LRN_4D], ids=lambda s: "x".join(map(str, s)))
def test_lrn_per_element(shape, params):
    r, bias, alpha, beta = params
    x64, dy64 = NP.lrn_input(shape)
    want = NP.lrn64(x64, dy64, r, bias, alpha, beta)
    x = x64.to(DEV, BF).requires_grad_()
    y = dlrn.lrn(x, r, bias, alpha, beta)
    assert y.dtype == BF and tuple(y.shape) == tuple(shape)
    y.backward(dy64.to(DEV, BF))
    _inside(y, want.y, want.y_tol, "y")
    _inside(x.grad, want.dx, want.dx_tol, "dx")


def test_lrn_refuses_more_than_1024_channels():
    x = torch.zeros(2, 1032, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError):
        dlrn.lrn(x, *NP.LRN_MODEL)
