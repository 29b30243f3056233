"""The column tree of csrc/kernels/nhwc8.h, pinned bit for bit through its two slab-split users: the squeezed vector of
se.hip (one accumulator set) and the slab records and statistics of groupnorm.hip (two sets).

The host references repeat the documented order in fp32 on the stored inputs: the pixel lanes of a column fold past
the largest power of two first, then halve; slab records merge in slab order.  Every shape keeps a slab no longer
than the block's pixel lanes (256 // 3 = 85 for SE, 256 // 17 = 15 for group norm), so a lane's partial is one pixel,
exact in fp32, and every rounding of the result is one of the tree's, the channel fold's or the slab merge's.  With
slabs of 8 pixels only the lanes 0 .. 7 hold data and the fold past the largest power of two (64, 8) adds zeros; the
one-slab rows (81 and 15 pixels) fill lanes past it, so that the fold-first order shows in the bits."""
import numpy as np
import pytest
import torch

from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops.se import squeeze_excite

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _tree(lanes):
    """lanes [PL, ...] fp32 -> the totals col_tree8 leaves in lane 0."""
    L = lanes.copy()
    PL = L.shape[0]
    P = 1
    while P * 2 <= PL:
        P *= 2
    L[:PL - P] += L[P:PL]
    h = P // 2
    while h >= 1:
        L[:h] += L[h:2 * h]
        h //= 2
    return L[0]


def _lanes(vals, PL):
    """vals [pixels <= PL, ...] as the partials of PL pixel lanes: 0 + value, 0 for the idle lanes."""
    assert vals.shape[0] <= PL
    L = np.zeros((PL,) + vals.shape[1:], F)
    L[:vals.shape[0]] += vals
    return L


def _slabs(HW, SP):
    return [(p0, min(HW, p0 + SP)) for p0 in range(0, HW, SP)]


@pytest.mark.parametrize("H,SP", [(5, 8), (9, 81)], ids=["slabs-8-8-8-1", "one-slab-81-of-85-lanes"])
def test_se_squeeze_bits(H, SP):
    N, W, C, Cr = 2, H, 24, 4
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)
    w1, b1, w2, b2 = (torch.randn(*s, generator=g).to(DEV) for s in ((Cr, C), (Cr,), (C, Cr), (C,)))
    y = squeeze_excite(x.to(DEV).requires_grad_(), w1, b1, w2, b2, relu=False, slab_pixels=SP)
    s = y.grad_fn.saved_tensors[6]  # ops/se.py saves (x, y, w1, b1, w2, b2, s, z, g): s is the squeezed vector [N, C]
    assert s.shape == (N, C) and s.dtype == torch.float32 and y.grad_fn.saved_tensors[7].shape == (N, Cr)
    got = s.cpu().numpy()
    xs = x.float().numpy().reshape(N, H * W, C)
    want = np.zeros((N, C), F)
    for p0, p1 in _slabs(H * W, SP):  # se_gate_kernel: a = 0, a += record, in slab order
        want += _tree(_lanes(xs[:, p0:p1].transpose(1, 0, 2), 256 // (C // 8)))
    want *= F(1) / F(H * W)
    assert np.array_equal(got, want), np.abs(got - want).max()


def _merge_chan(u, v, na, ub, vb, nb):
    """merge2<true> of groupnorm.hip: (mean, M2) of na values absorbs (ub, vb) of nb values; every product rounded."""
    d, n = ub - u, F(na + nb)
    return u + d * (F(nb) / n), v + (vb + d * d * (F(na) * F(nb) / n))


@pytest.mark.parametrize("SP", [8, 15], ids=["slabs-8-7", "one-slab-15-of-15-lanes"])
def test_group_norm_stats_bits(SP):
    """dtm_groupnorm_fwd on a workspace the test owns: the per-slab records (mean, M2) of ws, which the two-set tree
    and the channel fold write before any reciprocal square root, and the merged mean of stats, bit for bit."""
    N, H, W, C, G = 2, 3, 5, 136, 17
    HW, Cg, eps = H * W, C // G, 1e-6
    assert Cg == 8  # a group is one 16-byte column: the fold across columns has a single term
    torch.manual_seed(12)
    x = torch.randn(N, H, W, C) + 3.0
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    L, slabs = _lib.lib(), _slabs(HW, SP)
    f32 = dict(device=DEV, dtype=torch.float32)
    y, stats = torch.empty_like(xd), torch.empty((N, G, 2), **f32)
    n_ws = L.dtm_groupnorm_ws_floats(N, HW, C, G, SP, 0)
    assert n_ws == N * len(slabs) * G * 2
    ws = torch.empty(n_ws, **f32)
    rc = L.dtm_groupnorm_fwd(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(y), _lib.ptr(stats), _lib.ptr(ws), n_ws,
                             N, HW, C, G, SP, eps, 1, 0, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got, got_ws = stats.cpu().numpy(), ws.cpu().numpy().reshape(N, len(slabs), G, 2)

    xs = x.numpy().reshape(N, HW, C)
    PL = 256 // (C // 8)
    recs = []
    for p0, p1 in slabs:
        np_ = F(p1 - p0)
        K = xs[:, p0]  # the shift: each channel at the slab's first pixel
        d = (xs[:, p0:p1] - K[:, None]).transpose(1, 0, 2)
        ts = _tree(_lanes(d, PL))
        tq = _tree(_lanes((d.astype(np.float64) ** 2).astype(F), PL))  # fmaf(d, d, 0): one rounding of the product
        dm = ts / np_
        m2 = np.maximum(tq - ts * dm, F(0))
        K, dm, m2 = (t.reshape(N, G, Cg) for t in (K, dm, m2))
        ref, u, v, na = K[..., 0], dm[..., 0], m2[..., 0], np_  # fold_to_groups: the channels of a column in order
        for e in range(1, Cg):
            u, v = _merge_chan(u, v, na, dm[..., e] + (K[..., e] - ref), m2[..., e], np_)
            na = F(na + np_)
        recs.append((ref + u, v, F(p1 - p0) * F(Cg)))
    for i, (ub, vb, _) in enumerate(recs):
        assert ub.dtype == F and vb.dtype == F
        assert np.array_equal(got_ws[:, i, :, 0], ub), (i, np.abs(got_ws[:, i, :, 0] - ub).max())
        assert np.array_equal(got_ws[:, i, :, 1], vb), (i, np.abs(got_ws[:, i, :, 1] - vb).max())
    ref, v, na = recs[0][0], recs[0][1], recs[0][2]  # fold_slabs: means relative to the first slab's
    u = ref - ref
    for ub, vb, nb in recs[1:]:
        u, v = _merge_chan(u, v, na, ub - ref, vb, nb)
        na = F(na + nb)
    mean = ref + u
    arg = v / (F(HW) * F(Cg)) + F(eps)
    assert all(t.dtype == F for t in (mean, arg))
    assert np.array_equal(got[..., 0], mean), np.abs(got[..., 0] - mean).max()
    # rstd = rsqrtf(arg) is one v_rsq_f32 of an argument whose terms are pinned above.  The instruction is accurate to
    # 1 ulp and not correctly rounded, so no host or torch function returns its bits (torch.rsqrt on the device
    # differed from it by one ulp in 2 of the 34 groups): this last step alone is held to that 1 ulp
    exact = 1.0 / np.sqrt(arg.astype(np.float64))
    ulps = np.abs(got[..., 1].astype(np.float64) - exact) / np.spacing(exact.astype(F))
    print("rstd error in ulp", ulps.max())
    assert ulps.max() <= 1.0, ulps.max()
