"""The float64 references and bounds of tests/norm_pool_cases.py checked on the CPU: they agree with ops.reference and
torch autograd, every case lands on the kernel path its comment names, the exactness conditions hold, the kernel's
BatchNorm formula evaluated in fp32 meets the bounds (margins printed), and deliberately wrong LRN references do not."""
import pytest
import torch

import norm_pool_cases as NP
from distributed_tensorflow_models_amd.ops import reference as ref
from distributed_tensorflow_models_amd.ops.geometry import pool_geom

F64 = torch.float64
BN_NAMES = list(NP.BN_CASES)
SMALL_POOL = [c for c in NP.POOL_CASES if c[0][:3] == (1, 8, 8) and c[0][3] in (16, 3)] + \
    [c for c in NP.POOL_CASES if c[0] == (2, 13, 14, 20)]


# ---- number formats -------------------------------------------------------------------------------------------------
def test_bf16_rounding_costs_up_to_2_pow_minus_8():
    v = torch.tensor([1 + 2.0 ** -8 - 2.0 ** -12], dtype=F64)
    err = (v.to(NP.BF).to(F64) - v).abs() / v
    assert 2.0 ** -9 < err.item() <= NP.BF16 / (1 + NP.BF16)
    # the correctly rounded reference itself breaks a 2^-9 bound and keeps the 2^-8 one
    f = NP.bn_forward64(NP.bn_random_input("fast-1blk").x, torch.ones(64, dtype=F64), torch.zeros(64, dtype=F64), None,
                        False)
    e = (f.y.to(NP.BF).to(F64) - f.y).abs()
    assert (e > 2.0 ** -9 * f.y.abs()).any() and (e <= NP.BF16 * f.y.abs()).all()


# ---- BatchNorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BN_NAMES)
def test_bn_case_reaches_its_path(name):
    shape, want = NP.BN_CASES[name]
    got = NP.bn_path(shape)
    assert {k: got.get(k) for k in want} == want, got
    assert shape[0] * shape[1] * shape[2] * shape[3] * 2 < 4 << 20


def test_bn_paths_cover_the_issue_list():
    p = {n: NP.bn_path(s) for n, (s, _) in NP.BN_CASES.items()}
    assert p["fast-ragged"]["blocks"] in (3, 4) and p["fast-cols5"]["blocks"] > 1 and 256 % p["fast-cols5"]["cols"]
    assert p["fast-33blk"]["blocks"] > 32 and p["fast-c2048"]["blocks"] > 32 and p["fast-c2048"]["cols"] == 256
    assert NP.bn_path((4, 46, 46, 64))["blocks"] == 30  # (why the 33-block case is not 4x46x46)
    for n in ("gen1-c3", "gen1-c36", "gen1-c300", "gen8-c2056"):
        assert p[n]["blocks"] >= 3 and p[n]["rpb"] >= 64
    assert NP.bn_path(NP.BN_COND_SHAPE)["kind"] == "fast"


@pytest.mark.parametrize("name", BN_NAMES)
def test_bn_exact_sums_fit_fp32(name):
    x, sums = NP.bn_exact_input(name)
    assert x.abs().max() <= 3 and torch.equal(x, x.to(NP.BF).to(F64))
    assert sums.abs().max() < NP.SUM_LIMIT and torch.equal(sums, sums.float().to(F64))
    assert sums[1].min() > 0


def _bn_autograd(inp, relu, res, bessel):
    x, gm, bt = (t.clone().requires_grad_() for t in (inp.x, inp.gamma, inp.beta))
    r = inp.res.clone().requires_grad_() if res else None
    mm, mv = inp.mm.clone(), inp.mv.clone()
    xf = x.reshape(-1, x.shape[-1])
    mean, var = xf.mean(0), xf.var(0, unbiased=False)
    y = ((xf - mean) * torch.rsqrt(var + NP.EPS) * gm + bt).reshape(x.shape)
    if res:
        y = y + r
    if relu:
        y = torch.relu(y)
    y.backward(inp.dy)
    return y.detach(), x.grad, gm.grad, bt.grad, (r.grad if res else None), mm, mv


@pytest.mark.parametrize("name,relu,res,bessel", [("fast-1blk", False, False, True), ("gen1-c36", True, True, False),
                                                  ("fast-cols5", True, False, True)])
def test_bn_reference_matches_autograd_and_ops_reference(name, relu, res, bessel):
    inp = NP.bn_random_input(name)
    r = inp.res if res else None
    f = NP.bn_forward64(inp.x, inp.gamma, inp.beta, r, relu, inp.mm, inp.mv, bessel)
    b = NP.bn_backward64(f, inp.x, inp.gamma, inp.dy, (f.y > 0).to(F64) if relu else None)
    y, dx, dg, db, dr, _, _ = _bn_autograd(inp, relu, res, bessel)
    for got, want in ((f.y, y), (b.dx, dx), (b.dgamma, dg), (b.dbeta, db)):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-10)
    if res:
        assert torch.equal(b.g, dr)
    # ops.reference (fp32 inside): the forward and the moving-average rules, Bessel on and off
    mm, mv = inp.mm.float(), inp.mv.float()
    yr = ref.batch_norm(inp.x.float(), inp.gamma.float(), inp.beta.float(), mm, mv, True, NP.DECAY, NP.EPS, relu,
                        r.float() if res else None, bessel)
    assert torch.allclose(yr.to(F64), f.y, rtol=1e-4, atol=1e-4)
    assert torch.allclose(mm.to(F64), f.mm, rtol=1e-5, atol=1e-6) and torch.allclose(mv.to(F64), f.mv, rtol=1e-5, atol=1e-6)
    assert (f.mm_tol > 0).all() and (f.mv_tol > 0).all() and (f.mm_tol < 1e-5).all() and (f.mv_tol < 1e-3).all()


@pytest.mark.parametrize("name", BN_NAMES + [NP.BN_COND])
def test_bn_fp32_emulation_meets_the_bounds(name):
    inp = NP.bn_random_input(name)
    worst = 0.0
    for relu, res in ((False, False), (True, True)):
        r = inp.res if res else None
        f = NP.bn_forward64(inp.x, inp.gamma, inp.beta, r, relu)
        yb, y32 = NP.bn_fp32_emulation(inp.x, inp.gamma, inp.beta, r, relu)
        err = (yb.to(F64) - f.y).abs()
        assert (err <= f.tol).all()
        margin = (err / f.tol).max().item()
        fp32_share = ((y32.to(F64) - f.y).abs() / (f.tol - NP.BF16 * f.y.abs())).max().item()
        print("bn %s relu=%d res=%d: max |err| / bound = %.3f; fp32 error / (bound - bf16 term) = %.3f; "
              "max kappa = %.1f" % (name, relu, res, margin, fp32_share, f.kappa.max().item()))
        worst = max(worst, margin, fp32_share)
    assert worst < 1.0
    if name == NP.BN_COND:
        assert f.kappa.min() > 500  # the mean really is far from zero against the spread


def test_bn_conditioning_term_is_needed():
    # without the kappa term the fp32 formula breaks the bound on the conditioning case: the term is what the case tests
    inp = NP.bn_random_input(NP.BN_COND)
    f = NP.bn_forward64(inp.x, inp.gamma, inp.beta, None, False)
    _, y32 = NP.bn_fp32_emulation(inp.x, inp.gamma, inp.beta, None, False)
    bare = f.tol - NP.BF16 * f.y.abs() - f.kappa * 2.0 ** -22 * (f.xhat * inp.gamma).abs()
    assert ((y32.to(F64) - f.y).abs() > bare).any()


# ---- pooling --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NP.POOL_CASES, ids=NP.pool_id)
def test_pool_case_dispatch(case):
    shape, k, s, pad = case
    C = shape[3]
    d = NP.pool_dispatch(pool_geom(shape, k, s, pad))
    eight = C % 8 == 0
    assert d["generic"] == ("V8-Idx32" if eight else "V1-Idx64")
    assert d["k3s2"] == (eight and (k, s) == (3, 2)) and d["k3s1"] == (eight and (k, s) == (3, 1))
    assert d["valid53"] == (eight and (k, s) == (5, 3))
    assert d["max_fwd"] == ("k3s2" if d["k3s2"] else d["generic"])
    assert d["avg_fwd"] == ("k3s1" if d["k3s1"] else "valid53" if d["valid53"] else d["generic"])
    assert (d["avg_bwd_acc"] is None) == (not eight)


def test_pool_cases_cover_every_kernel():
    seen = set()
    for shape, k, s, pad in NP.POOL_CASES:
        g = pool_geom(shape, k, s, pad)
        d = NP.pool_dispatch(g)
        seen |= {("max", d["max_fwd"]), ("avg", d["avg_fwd"]), ("acc", d["avg_bwd_acc"]), ("pad", g.PH, g.PW)}
    assert {("max", "k3s2"), ("max", "V8-Idx32"), ("max", "V1-Idx64"), ("avg", "k3s1"), ("avg", "valid53"),
            ("avg", "V8-Idx32"), ("avg", "V1-Idx64"), ("acc", "valid53"), ("acc", "V8-Idx32"),
            ("pad", 1, 0), ("pad", 0, 0), ("pad", 1, 1)} <= seen


@pytest.mark.parametrize("case", NP.POOL_CASES, ids=NP.pool_id)
def test_pool_unique_inputs_have_no_tied_window(case):
    shape, k, s, pad = case
    x = NP.pool_input(shape, "unique")
    assert torch.equal(x, x.to(NP.BF).to(F64)) and x.abs().max() <= 4
    y, _, ties = NP.max_pool64(x, k, s, pad)
    assert ties == 0 and torch.isfinite(y).all()
    dx = NP.max_pool_bwd64(x, NP.pool_dy(case, -1, 1), k, s, pad)
    assert dx.abs().max() <= 9 and torch.equal(dx, dx.round())
    if k > 1:
        assert NP.max_pool64(NP.pool_input(shape, "ties"), k, s, pad)[2] > 0


def _autograd(fn, x, dy):
    x = x.clone().requires_grad_()
    y = fn(x)
    y.backward(dy)
    return y.detach(), x.grad


@pytest.mark.parametrize("case", SMALL_POOL, ids=NP.pool_id)
def test_pool_references_match_ops_reference(case):
    shape, k, s, pad = case
    x = NP.pool_input(shape, "unique")
    dy = NP.pool_dy(case, -3, 3)
    yr, dxr = _autograd(lambda t: ref.max_pool(t, k, s, pad), x, dy)
    assert torch.equal(NP.max_pool64(x, k, s, pad)[0], yr) and torch.equal(NP.max_pool_bwd64(x, dy, k, s, pad), dxr)
    neg = NP.pool_input(shape, "negative")
    y = NP.max_pool64(neg, k, s, pad)[0]
    assert torch.equal(y, ref.max_pool(neg, k, s, pad)) and y.max() <= -1
    xi = NP.pool_input(shape, "int")
    for cp in (0, 1):
        yr, dxr = _autograd(lambda t: ref.avg_pool(t, k, s, pad, bool(cp)), xi, dy)
        y, ytol = NP.avg_pool64(xi, k, s, pad, cp)
        dx, dtol = NP.avg_pool_bwd64(shape, dy, k, s, pad, cp)
        assert torch.allclose(y, yr, rtol=1e-12, atol=1e-12) and torch.allclose(dx, dxr, rtol=1e-12, atol=1e-12)
        assert (ytol >= NP.BF16 * y.abs()).all() and (dtol >= NP.BF16 * dx.abs()).all()
        main = NP.pool_input(shape, "ties")
        tot, ttol = NP.avg_pool_bwd64(shape, dy, k, s, pad, cp, main)
        assert torch.allclose(tot, main + dx, rtol=1e-12, atol=1e-12) and (ttol >= NP.BF16 * tot.abs()).all()


def test_max_pool_tie_rule_is_first_maximum():
    # a hand-made window: all nine taps equal -> tap 0 takes the gradient; then a later strict maximum takes over
    x = torch.zeros(1, 3, 3, 1, dtype=F64)
    dy = torch.full((1, 1, 1, 1), 5.0, dtype=F64)
    want = torch.zeros_like(x)
    want[0, 0, 0, 0] = 5
    assert torch.equal(NP.max_pool_bwd64(x, dy, 3, 1, "VALID"), want)
    x[0, 1, 2, 0] = x[0, 2, 0, 0] = 1.0
    want.zero_()
    want[0, 1, 2, 0] = 5
    assert torch.equal(NP.max_pool_bwd64(x, dy, 3, 1, "VALID"), want)
    assert NP.max_pool64(x, 3, 1, "VALID")[2] == 1


def test_avg_pool_same_divisor_excludes_padding():
    cnt = NP.pool_counts(pool_geom((1, 8, 8, 16), 3, 1, "SAME"))
    assert cnt[0, 0] == 4 and cnt[0, 3] == 6 and cnt[3, 0] == 6 and cnt[3, 3] == 9 and cnt[7, 7] == 4
    cnt = NP.pool_counts(pool_geom((2, 13, 14, 16), 3, 2, "SAME"))  # pads: top 1, left 0, bottom 1, right 1
    assert cnt[0, 0] == 6 and cnt[1, 0] == 9 and cnt[0, 6] == 4 and cnt[6, 6] == 4 and cnt[6, 0] == 6
    x = torch.full((1, 8, 8, 16), 9.0, dtype=F64)
    assert torch.equal(NP.avg_pool64(x, 3, 1, "SAME", 0)[0], x)
    y = NP.avg_pool64(x, 3, 1, "SAME", 1)[0]
    assert y[0, 0, 0, 0] == 4 and y[0, 0, 3, 0] == 6 and y[0, 3, 3, 0] == 9


# ---- LRN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", NP.LRN_PARAMS)
@pytest.mark.parametrize("shape", [(1, 1, 7, 3), (1, 1, 9, 100), NP.LRN_4D])
def test_lrn_reference_matches_ops_reference_and_autograd(shape, params):
    r, bias, alpha, beta = params
    x, dy = NP.lrn_input(shape)
    got = NP.lrn64(x, dy, r, bias, alpha, beta)
    xr = x.clone().requires_grad_()
    # (ops.reference.lrn computes in fp32 whatever it is given: autograd in fp32, compared at fp32 accuracy)
    yr = ref.lrn(xr.float(), r, bias, alpha, beta)
    yr.backward(dy.float())
    assert torch.allclose(yr.detach().to(F64), got.y, rtol=1e-5, atol=1e-6)
    assert torch.allclose(xr.grad, got.dx, rtol=1e-4, atol=1e-5)
    # and the same formulas composed in float64 under autograd
    xd = x.clone().requires_grad_()
    C = shape[-1]
    sq = torch.nn.functional.pad(xd * xd, (r, r))
    s = bias + alpha * sum(sq[..., i:i + C] for i in range(2 * r + 1))
    y = xd * s ** -beta
    y.backward(dy)
    assert torch.allclose(y.detach(), got.y, rtol=1e-12, atol=1e-12) and torch.allclose(xd.grad, got.dx, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("shape", NP.LRN_SHAPES)
def test_lrn_shapes_reach_their_block_layouts(shape):
    npix, C = shape
    want = {3: 85, 64: 4, 96: 2, 100: 2, 256: 1, 384: 1, 1024: 1}[C]
    assert NP.lrn_pixels_per_block(C) == want and C <= 1024
    if C == 64:
        assert npix % want  # ragged last block
    if C == 3:
        assert all(C < 2 * r + 1 for r, *_ in NP.LRN_PARAMS)


@pytest.mark.parametrize("params", NP.LRN_SHARP)
@pytest.mark.parametrize("shape", [s for s in NP.LRN_SHAPES if s[1] > 16])
@pytest.mark.parametrize("wrong", ["r-1", "r+1", "lo+1", "hi-1", "no-clamp-lo", "no-clamp-hi"])
def test_wrong_lrn_references_violate_the_bound(shape, params, wrong):
    r, bias, alpha, beta = params
    x, dy = NP.lrn_input(shape)
    good = NP.lrn64(x, dy, r, bias, alpha, beta)
    kw = {"r-1": dict(r_lo=r - 1, r_hi=r - 1), "r+1": dict(r_lo=r + 1, r_hi=r + 1), "lo+1": dict(r_lo=r + 1),
          "hi-1": dict(r_hi=r - 1), "no-clamp-lo": dict(clamp_lo=False), "no-clamp-hi": dict(clamp_hi=False)}[wrong]
    bad = NP.lrn64(x, dy, r, bias, alpha, beta, **kw)
    # as a bf16 kernel would deliver it
    ybad, dxbad = bad.y.to(NP.BF).to(F64), bad.dx.to(NP.BF).to(F64)
    assert ((ybad - good.y).abs() > good.y_tol).any() and ((dxbad - good.dx).abs() > good.dx_tol).any()
    if wrong.startswith("no-clamp") and shape[0] > 1:
        # only channels within r of that end, and not the first / last pixel's outer side, can differ
        C = shape[1]
        far = slice(r, C) if wrong == "no-clamp-lo" else slice(0, C - r)
        assert torch.equal(bad.y[:, far], good.y[:, far])
    ygood, dxgood = good.y.to(NP.BF).to(F64), good.dx.to(NP.BF).to(F64)
    assert ((ygood - good.y).abs() <= good.y_tol).all() and ((dxgood - good.dx).abs() <= good.dx_tol).all()


def test_lrn_model_parameters_hide_the_window():
    # with alpha = 0.001 / 9 the normaliser is about 1: a wrong radius stays inside the bound - why the sharp
    # parameter sets exist
    r, bias, alpha, beta = NP.LRN_MODEL
    x, dy = NP.lrn_input((37, 64))
    good = NP.lrn64(x, dy, r, bias, alpha, beta)
    bad = NP.lrn64(x, dy, r, bias, alpha, beta, r_lo=r - 1, r_hi=r - 1)
    assert ((bad.y.to(NP.BF).to(F64) - good.y).abs() <= good.y_tol).all()
