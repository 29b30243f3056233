"""Mixup / CutMix on the GPU: dtm_mix_images against the torch form of ops/mix.py bit for bit, containment of
non-contributing NaN / Inf, dtm_softmax_xent_mix against the plain kernel and an fp64 oracle, the fused mixed loss,
and TrainStep(mix=...) eager and captured."""
import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib, mix
from distributed_tensorflow_models_amd.ops import nn as F
from distributed_tensorflow_models_amd.ops.mix import MixConfig, sample_plan

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64  # sentinel elements on each side of x and of out
BOTH = dict(mixup_alpha=0.2, cutmix_alpha=1.0, prob=0.8, switch_prob=0.5)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _bits(t):
    return t.cpu().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- plans --------------------------------------------------------------------------------------------------------
def sampled_plans(B, H, W):
    """Sampler output: one batch-wise plan of each kind, and two per-row plans."""
    cfg, found = MixConfig(**BOTH, seed=1), {}
    for step in range(200):
        p = sample_plan(cfg, 0, step, 0, B, H, W)
        k = "cutmix" if (p.w_pix[0] == 1.0 and p.w_lab[0] != 1.0) else "mixup" if p.w_pix[0] != 1.0 else "identity"
        found.setdefault(k, p)
        if len(found) == 3:
            break
    # (a 1 x 1 image has no room for a box: its CutMix draws keep every pixel)
    assert "identity" in found and "mixup" in found and ("cutmix" in found or H * W == 1)
    rows = [sample_plan(MixConfig(**dict(BOTH, prob=0.7), per_row=True, seed=2), 0, s, 0, B, H, W) for s in (0, 1)]
    return list(found.values()) + rows


def handmade_plans(B, H, W, C):
    """Hand-made rows, B per plan: (partner offset, w_pix, box)."""
    xmid = 1 if W > 1 else 0  # x0 * C = 3 elements with C = 3: inside a 16-byte vector
    rows = [
        (1, 0.3, (0, 0, 0, 0)),                      # an empty box, blended
        (1, 1.0, (0, H, 0, W)),                      # the full image from the partner
        (1, 1.0, (0, 1, 0, 1)), (1, 1.0, (0, 1, W - 1, W)), (1, 1.0, (H - 1, H, 0, 1)), (1, 1.0, (H - 1, H, W - 1, W)),
        (1, 1.0, (H // 2, H, W // 2, W)),            # flush with the right and bottom edges
        (1, 1.0, (0, H, xmid, W)),                   # x0 * C in the middle of a vector
        (1, 1.0, (H // 3, H - H // 3, xmid, max(xmid, W - 1))),
        (0, 0.5, (0, 0, 0, 0)), (0, 1.0, (0, H, 0, max(1, W // 2))),  # partner == r
        (1, 0.0, (0, 0, 0, 0)), (1, 1.0, (0, 0, 0, 0)),              # w_pix of 0 and of 1
        (1, 0.0, (0, max(1, H // 2), 0, W)),         # all of the partner, box or not
        (1, 0.25, (0, H, 0, max(1, W // 2))),        # a blend outside a box (no sampler draws it; the kernel takes it)
        (1, 1.0, (2 % H, 2 % H, 0, W)),              # rows empty, columns not
    ]
    plans = []
    for i in range(0, len(rows), B):
        chunk = [rows[(i + j) % len(rows)] for j in range(B)]
        plans.append(mix.make_plan([(r + d) % B for r, (d, _w, _b) in enumerate(chunk)], [w for _d, w, _b in chunk],
                                   [0.5] * B, [b for _d, _w, b in chunk], H, W))
    return plans


def run_kernel_case(x_cpu, plan, off_x, off_out):
    """x and out inside larger device buffers ([guard | offset | rows | guard], the guards and the offset hold 7);
    returns the whole out buffer and the slice of the rows."""
    n = x_cpu.numel()
    bx = torch.full((GUARD + off_x + n + GUARD,), 7.0, dtype=x_cpu.dtype)
    sx = slice(GUARD + off_x, GUARD + off_x + n)
    bx[sx] = x_cpu.reshape(-1)
    bx_d = bx.to(DEV)
    bo_d = torch.full((GUARD + off_out + n + GUARD,), 7.0, dtype=x_cpu.dtype, device=DEV)
    so = slice(GUARD + off_out, GUARD + off_out + n)
    assert bx_d.data_ptr() % 16 == 0 and bo_d.data_ptr() % 16 == 0
    out = mix.mix_images(bx_d[sx].view(x_cpu.shape), plan.to(DEV), out=bo_d[so].view(x_cpu.shape))
    torch.cuda.synchronize()
    assert out.data_ptr() == bo_d.data_ptr() + so.start * x_cpu.element_size()
    assert torch.equal(_bits(bx_d), _bits(bx))  # the source, its guards included, is only read
    return bo_d.cpu(), so


SHAPES = [((2, 1, 1, 3), torch.bfloat16), ((3, 4, 4, 1), torch.float32), ((4, 5, 7, 3), torch.bfloat16),
          ((4, 5, 7, 3), torch.float32), ((8, 8, 8, 3), torch.bfloat16), ((16, 32, 32, 3), torch.bfloat16),
          ((2, 299, 299, 3), torch.bfloat16)]


@pytest.mark.parametrize("shape,dtype", SHAPES, ids=["%s-%s" % ("x".join(map(str, s)), str(d)[6:]) for s, d in SHAPES])
def test_kernel_matches_the_cpu_form_bit_for_bit(shape, dtype):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(dtype)
    x.view(-1)[:: max(2, x.numel() // 7)] = -0.0
    plans = sampled_plans(B, H, W) + handmade_plans(B, H, W, C)
    wants = [mix.mix_images(x, p) for p in plans]  # the torch form, once per plan
    assert any(not torch.equal(w, x) for w in wants)
    # x 0, 1, 3 and 7 elements past a 16-byte boundary, out alike (16-byte path where the rows allow it), and once
    # out offset differently (element path whatever the rows)
    for off_x, off_out in ((0, 0), (1, 1), (3, 3), (7, 7), (1, 3)):
        for k, (plan, want) in enumerate(zip(plans, wants)):
            got, so = run_kernel_case(x, plan, off_x, off_out)
            what = "shape %s offsets %d/%d plan %d %s" % (shape, off_x, off_out, k, plan.rec.tolist()[:4])
            assert torch.equal(_bits(got[so]), _bits(want.reshape(-1))), what
            assert bool((got[:so.start] == 7.0).all()) and bool((got[so.stop:] == 7.0).all()), what


def test_kernel_refuses_bad_arguments():
    x = torch.zeros(2, 4, 4, 3, device=DEV)
    plan = mix.identity_plan(2, 4, 4).to(DEV)
    L, s = _lib.lib(), _lib.stream_ptr()
    out = torch.ones_like(x)
    assert L.dtm_mix_images(_lib.ptr(x), _lib.ptr(x), _lib.ptr(plan.dev), 2, 4, 4, 3, 0, s) == -2  # in place
    assert L.dtm_mix_images(_lib.ptr(x), _lib.ptr(out), None, 2, 4, 4, 3, 0, s) == -1
    assert L.dtm_mix_images(_lib.ptr(x), _lib.ptr(out), _lib.ptr(plan.dev), 0, 4, 4, 3, 0, s) == -1
    with pytest.raises(ValueError):
        mix.mix_images(x, mix.identity_plan(2, 4, 4))  # no device record
    with pytest.raises(ValueError):
        mix.mix_images(x.view(-1)[:-8], plan)
    torch.cuda.synchronize()
    assert bool((out == 1).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("off", [0, 1])
def test_non_contributing_nan_and_inf_stay_out(dtype, off):
    B, H, W, C = 2, 6, 6, 3
    g = torch.Generator().manual_seed(1)
    base = torch.randn(B, H, W, C, generator=g).to(dtype)
    # row 0: CutMix from row 1 with the box [2, 4) x [2, 4); row 1: itself
    plan = mix.make_plan([1, 1], [1.0, 1.0], [0.8, 1.0], [[2, 4, 2, 4], [0, 0, 0, 0]], H, W)
    quiet = base.clone()
    quiet[1, 0, 0, 1] = float("nan")    # partner pixels outside the box
    quiet[1, 5, 3, 2] = float("inf")
    quiet[0, 2, 2, 0] = float("nan")    # the row's own pixels inside the box
    quiet[0, 3, 3, 1] = float("-inf")
    got, so = run_kernel_case(quiet, plan, off, off)
    out = got[so].view(B, H, W, C)
    assert bool(torch.isfinite(out[0]).all())
    assert torch.equal(_bits(out), _bits(mix.mix_images(quiet, plan)))
    loud = base.clone()
    loud[1, 2, 3, 0] = float("nan")     # a partner pixel inside the box
    loud[1, 3, 2, 2] = float("inf")
    loud[0, 0, 0, 1] = float("inf")     # the row's own pixel outside it
    loud[0, 5, 5, 0] = float("nan")
    got, so = run_kernel_case(loud, plan, off, off)
    out = got[so].view(B, H, W, C)
    bad = ~torch.isfinite(out[0].float())
    assert sorted(map(tuple, bad.nonzero().tolist())) == [(0, 0, 1), (2, 3, 0), (3, 2, 2), (5, 5, 0)]
    assert bool(torch.isnan(out[0, 2, 3, 0])) and bool(torch.isinf(out[0, 0, 0, 1]))
    # mixup: both sources contribute everywhere
    blend = mix.make_plan([1, 0], [0.5, 0.5], [0.5, 0.5], [[0, 0, 0, 0]] * 2, H, W)
    got, so = run_kernel_case(loud, blend, off, off)
    out = got[so].view(B, H, W, C).float()
    for r in (0, 1):
        assert bool(torch.isnan(out[r, 2, 3, 0])) and bool(torch.isinf(out[r, 0, 0, 1]))
        assert int((~torch.isfinite(out[r])).sum()) == 4


# ---- the two-label loss kernel ------------------------------------------------------------------------------------
def xent_case(K, dtype, seed=0):
    """B = 8 rows at a padded pitch; identity rows (w_lab == 1) inside a mixed batch, la == lb, w of 0, one
    out-of-range label on each side."""
    B, ld = 8, K + 5
    g = torch.Generator().manual_seed(seed + K)
    buf = (torch.randn(B, ld, generator=g) * 3).to(dtype)
    labels = torch.randint(0, K, (B,), generator=g).to(torch.int32)
    partner = [0, 2, 1, 3, 6, 5, 7, 4]
    labels[2] = labels[1]                # rows 1 and 2: la == lb
    labels[6] = K                        # out of range: row 6's own label, row 4's partner label
    w_lab = [1.0, 0.3, 0.6, 1.0, 0.7, 1.0, 0.25, 0.0]  # rows 0, 3, 5 identity; row 7 takes all of row 4's label
    plan = mix.make_plan(partner, [1.0] * B, w_lab, [[0, 0, 0, 0]] * B, 4, 4)
    return buf, labels, plan, ld


def run_xent(buf, labels, plan, K, ld, smoothing, gscale, mixed):
    B = buf.shape[0]
    L, s = _lib.lib(), _lib.stream_ptr()
    lg, lab = buf.to(DEV), labels.to(DEV)
    loss = torch.full((B + 2,), 7.0, device=DEV)
    dl = torch.full((B * K + 16,), 7.0, device=DEV).to(buf.dtype)
    bf = int(buf.dtype == torch.bfloat16)
    if mixed:
        pd = plan.to(DEV)
        assert L.dtm_softmax_xent_mix(_lib.ptr(lg), bf, _lib.ptr(lab), _lib.ptr(pd.dev), _lib.ptr(loss[1:]),
                                      _lib.ptr(dl[8:]), B, K, smoothing, gscale, ld, s) == 0
    else:
        L.dtm_softmax_xent(_lib.ptr(lg), bf, _lib.ptr(lab), _lib.ptr(loss[1:]), _lib.ptr(dl[8:]), B, K, smoothing,
                           gscale, None, ld, s)
    torch.cuda.synchronize()
    assert float(loss[0]) == 7.0 and float(loss[-1]) == 7.0
    assert bool((dl[:8].float() == 7.0).all()) and bool((dl[8 + B * K:].float() == 7.0).all())
    return loss[1:1 + B].cpu(), dl[8:8 + B * K].view(B, K).cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K", [10, 257, 1001])
def test_xent_mix_kernel(K, dtype):
    smoothing, gscale = 0.1, 0.125
    buf, labels, plan, ld = xent_case(K, dtype)
    loss_m, dl_m = run_xent(buf, labels, plan, K, ld, smoothing, gscale, mixed=True)
    loss_p, dl_p = run_xent(buf, labels, plan, K, ld, smoothing, gscale, mixed=False)
    ident = [r for r in range(8) if plan.w_lab[r] == 1.0]
    assert ident == [0, 3, 5]
    for r in ident:  # the plain kernel's bits
        assert torch.equal(_bits(loss_m[r:r + 1]), _bits(loss_p[r:r + 1])), r
        assert torch.equal(_bits(dl_m[r]), _bits(dl_p[r])), r
    assert not torch.equal(dl_m[4], dl_p[4])  # (a mixed row does differ from the plain kernel's)
    # fp64 oracle: an out-of-range label contributes nothing
    x = buf[:, :K].double()
    on, off = 1.0 - smoothing + smoothing / K, smoothing / K
    la, lb = labels.long(), labels.long()[torch.from_numpy(plan.partner.astype(np.int64))]
    w = torch.from_numpy(plan.w_lab.astype(np.float64)).view(-1, 1)
    ks = torch.arange(K).view(1, K)
    hot = w * (ks == la.view(-1, 1)).double() + (1 - w) * (ks == lb.view(-1, 1)).double()
    assert float(hot[6].sum()) == pytest.approx(0.75) and float(hot[4].sum()) == pytest.approx(0.7)
    t = off + (on - off) * hot
    lse = torch.logsumexp(x, -1)
    want_loss = lse - (t * x).sum(-1)
    want_dl = (torch.softmax(x, -1) - t) * gscale
    assert _rel(loss_m, want_loss) < 1e-4
    assert _rel(dl_m, want_dl) < (1e-4 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("bw", [1.0, 0.5])
def test_mean_xent_loss_mixed_fused_matches_composition(bw):
    """As test_mean_xent_loss_fused_matches_composition, with a plan: the fused two-label op (the plan's device
    record) against the composition mean(w * L_a + (1 - w) * L_b) of per-row kernels (the same plan without one)."""
    torch.manual_seed(13)
    B, Kin, N = 64, 128, 1001
    x = torch.randn(B, Kin, device=DEV).to(torch.bfloat16)
    labels = torch.randint(0, N, (B,), device=DEV)
    ws = [torch.nn.Parameter(torch.randn(Kin, N, device=DEV) / Kin ** 0.5) for _ in range(2)]
    host = sample_plan(MixConfig(**dict(BOTH, prob=0.7), per_row=True, seed=5), 0, 0, 0, B, 8, 8)
    assert len(set(host.kinds())) == 3
    out = []
    for plan in (host.to(DEV), host):
        for w in ws:
            w.grad = None
        xi = x.clone().requires_grad_()
        la, lb = F.linear(xi, ws[0], None), F.linear(xi * 2, ws[1], None)
        loss = F.mean_xent_loss([(la, bw), (lb, 0.4 * bw)], labels, 0.1, mix=plan)
        loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.detach()), xi.grad.float(), [w.grad.clone() for w in ws]))
    (l1, gx1, gw1), (l2, gx2, gw2) = out
    assert abs(l1 - l2) <= 1e-5 * abs(l2), (l1, l2)
    assert _rel(gx1, gx2) < 1e-2
    for a, b in zip(gw1, gw2):
        assert _rel(a, b) < 1e-2
    plain = float(F.mean_xent_loss([(la.detach(), bw), (lb.detach(), 0.4 * bw)], labels, 0.1))
    assert abs(plain - l1) > 1e-3 * abs(l1)  # the plan did change the loss


# ---- the step -----------------------------------------------------------------------------------------------------
MB = 16


@pytest.fixture()
def deterministic():
    """Fixed-order reductions, weight gradients on the main stream (the side stream sizes its split-K otherwise)."""
    side_was = _lib.side_enabled()
    _lib.set_deterministic(True)
    _lib.set_side_enabled(False)
    try:
        yield
    finally:
        _lib.set_deterministic(False)
        _lib.set_side_enabled(side_was)


def lenet():
    torch.manual_seed(0)
    return nets_factory.build("lenet", 10, dropout_keep_prob=1.0).to(DEV)


def batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(MB, 28, 28, 1, generator=g).to(DEV, torch.bfloat16),
             torch.randint(0, 10, (MB,), generator=g).to(DEV)) for _ in range(n)]


def run_steps(accum, cfg, steps, graph=False):
    model = lenet()
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, label_smoothing=0.1, ema_decay=0.99,
                     accum_steps=accum, mix=cfg, use_graph=graph)
    data = batches(steps * accum)
    keep = [x.clone() for x, _y in data]
    losses, lams = [], []
    for s in range(steps):
        xs, ys = (list(v) for v in zip(*data[s * accum:(s + 1) * accum]))
        losses.append(float(step(xs, ys) if accum > 1 else step(xs[0], ys[0])))
        lams.append(step.last_mix_lambda())
    torch.cuda.synchronize()
    assert (step._graph is not None) == graph and step.global_step == steps
    assert all(torch.equal(a, x) for a, (x, _y) in zip(keep, data))  # the caller's batches are never written
    step.dp.close()
    return losses, [p.detach().clone() for p in model.parameters()], lams


def test_step_with_prob_zero_is_the_plain_step(deterministic):
    l0, p0, _ = run_steps(1, None, 3)
    l1, p1, lams = run_steps(1, MixConfig(**dict(BOTH, prob=0.0)), 3)
    assert l0 == l1 and lams == [1.0] * 3
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))


@pytest.mark.parametrize("accum,seed", [(1, 4), (2, 0)])
def test_captured_step_matches_eager(deterministic, accum, seed):
    """Two eager warm-up steps, the capture, three replays, against six eager steps.  The plans of those steps hold an
    unmixed batch, a mixup batch and a CutMix batch (asserted: a frozen plan could not pass)."""
    cfg = MixConfig(**BOTH, seed=seed)
    plans = [sample_plan(cfg, 0, s, i, MB, 28, 28) for s in range(6) for i in range(accum)]
    assert {p.kinds()[0] for p in plans} == {"identity", "mixup", "cutmix"}
    assert len({p.kinds()[0] for p in plans[2 * accum:]}) >= 2  # and the captured steps themselves differ in kind
    le, pe, lam_e = run_steps(accum, cfg, 6)
    lg, pg_, lam_g = run_steps(accum, cfg, 6, graph=True)
    want = [float(np.mean([p.w_lab.astype(np.float64).mean() for p in plans[s * accum:(s + 1) * accum]]))
            for s in range(6)]
    assert lam_e == pytest.approx(want, rel=1e-12) and lam_g == lam_e
    assert le == lg, (le, lg)
    assert all(torch.equal(a, b) for a, b in zip(pe, pg_))
    plain = run_steps(accum, None, 6)[1]
    assert not all(torch.equal(a, b) for a, b in zip(pe, plain))
