"""Exact-arithmetic tests of the 8-wave streaming 1x1 conv kernels (conv1x1_stream_kernel with 512 threads, tile ids
34: 64 pixels x 256 channels, reductions up to 128 deep, and 35: 64 x 128, up to 256 deep).

Inputs as in tests/conv_exact_cases.py (ternary operands, prologue scales in {1, 2} and shifts in {-1, 0, 1}): every
output and every BatchNorm sum is a small integer, so the kernel must equal the float64 reference bit for bit, and the
sum over its statistics rows (one per 256-pixel group, as the 256x256 tile writes them) must equal the float64 column
sums exactly.  Every launch asserts
dtm_conv_last_tiles against the requested id.  dtm_conv_set_stream_workers_cap makes each worker walk several pixel
tiles of these tiny inputs (ring wrap, both buffer parities, the tail of the tile walk)."""
import ctypes

import pytest
import torch

import conv_exact_cases as C
from distributed_tensorflow_models_amd.ops import _lib, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CT = {34: 256, 35: 128}


def _case(N, H, W, Cin, K):
    return (N, H, W, Cin, K, (1, 1), 1, "SAME")


# (tile id, case, worker cap: 0 = off).  A worker walks whole 256-pixel groups, four 64-pixel tiles each.
CASES = [
    (34, _case(1, 5, 5, 128, 256), 0),     # M = 25: one partial pixel tile; K = CT
    (34, _case(1, 9, 9, 128, 512), 0),     # M = 81: a full tile and a partial one; K = 2 CT
    (34, _case(1, 11, 41, 128, 264), 2),   # M = 64*7 + 3: 8 tiles, one group per worker; K = CT + 8 (partial channel tile)
    (34, _case(1, 11, 41, 128, 264), 1),   # ... two groups on one worker (even): the ring wraps, the walk crosses a group
    (34, _case(1, 23, 31, 128, 256), 1),   # M = 713: three groups (odd) on one worker, the last one partial
    (34, _case(1, 23, 31, 128, 256), 2),   # ... 2 + 1 groups: the tail of the walk
    (34, _case(1, 11, 41, 64, 256), 1),    # Kg = 64: the second k sub-tile is all zero fill
    (35, _case(1, 5, 5, 256, 128), 0),
    (35, _case(1, 9, 9, 192, 256), 0),     # Kg = 192: the k < Kg guard inside the last sub-tile pair
    (35, _case(1, 9, 9, 128, 128), 0),     # Kg = 128 on the 256-deep form
    (35, _case(1, 11, 41, 192, 136), 2),   # K = CT + 8
    (35, _case(1, 11, 41, 192, 136), 1),
    (35, _case(1, 23, 31, 256, 256), 1),
    (35, _case(1, 23, 31, 256, 256), 2),
]


def _last(L):
    nt = ctypes.c_int(-7)
    L.dtm_conv_last_tiles(ctypes.byref(nt), None)
    return nt.value


def _run(L, tid, case, opt, d):
    """One forced launch through dtm_conv_fwd: (y, stats or None)."""
    N, H, W, Cin, K, _, _, _ = case
    pro, stats_on = opt == "prologue_stats", opt != "plain"
    y = torch.full((N, H, W, K), float("nan"), device=DEV, dtype=BF)
    stats = torch.zeros(2, K, device=DEV) if stats_on else None
    desc = C.inputs(case).geom.as_desc(_lib.ConvDesc)
    rc = L.dtm_conv_fwd(_lib.ptr(d["x"]), _lib.ptr(d["w_pro"] if pro else d["w"]), _lib.ptr(y), _lib.ptr(stats), None,
                        _lib.ptr(d["sc"]) if pro else None, _lib.ptr(d["sh"]) if pro else None, 0, ctypes.byref(desc),
                        _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _last(L) == tid, "requested tile %d, dtm_conv_last_tiles says %d" % (tid, _last(L))
    return y, stats


@pytest.mark.parametrize("tid,case,cap", CASES, ids=["t%d-%s-cap%d" % (t, C.case_id(c), w) for t, c, w in CASES])
def test_stream8_exact(tid, case, cap):
    L = _lib.lib()
    t, r = C.inputs(case), C.reference(case)
    C.check_exact_conditions(r)
    d = {n: getattr(t, n).to(DEV, BF).contiguous() for n in ("x", "w", "w_pro")}
    d.update({n: getattr(t, n).to(DEV, torch.float32).contiguous() for n in ("sc", "sh")})
    errors = []
    try:
        L.dtm_conv_set_tile(tid)
        L.dtm_conv_set_stream_workers_cap(cap)
        for det in (0, 1):
            L.dtm_set_deterministic(det)
            for opt in ("plain", "stats", "prologue_stats"):
                what = "fwd tile %d %s cap %d %s det %d" % (tid, C.case_id(case), cap, opt, det)
                pro = opt == "prologue_stats"
                y, stats = _run(L, tid, case, opt, d)
                try:
                    C.assert_exact(y, r.y_pro if pro else r.y, (64, CT[tid]), what + " y")
                    if stats is not None:
                        C.assert_exact(stats, r.stats_pro if pro else r.stats, None, what + " stats [sum y; sum y^2]")
                    if det:  # bit-identical across two calls
                        y2, stats2 = _run(L, tid, case, opt, d)
                        assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), what + ": y differs between calls"
                        if stats is not None:
                            assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32)), what + ": stats differ"
                except AssertionError as e:
                    errors.append(str(e))
    finally:
        L.dtm_conv_set_tile(-1)
        L.dtm_conv_set_stream_workers_cap(0)
        L.dtm_set_deterministic(0)
    assert not errors, "\n".join(errors)


def test_side_inputs_fall_back():
    """The 8-wave forms have no dgrad post-ops: a forced id with a side input runs the 64x128 register-staged tile."""
    L = _lib.lib()
    case = _case(1, 9, 9, 256, 128)  # as a dgrad: dy has 128 channels (Kg = 128), dx 256
    t, r = C.inputs(case), C.reference(case)
    dy, add = t.dy.to(DEV, BF).contiguous(), t.add1.to(DEV, BF).contiguous()
    wt = t.w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(DEV, BF)
    desc = t.geom.as_desc(_lib.ConvDesc)
    try:
        for tid, src, want, ran in ((34, None, r.dgrad["plain"][0], 34), (34, add, r.dgrad["add1"][0], 4)):
            L.dtm_conv_set_tile(tid)
            dx = torch.full((1, 9, 9, 256), float("nan"), device=DEV, dtype=BF)
            rc = L.dtm_conv_dgrad_ex(_lib.ptr(dy), _lib.ptr(wt), _lib.ptr(dx), ctypes.byref(desc), _lib.ptr(src), 1,
                                     None, None, None, 0, _lib.stream_ptr())
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert _last(L) == ran, (tid, _last(L), ran)
            C.assert_exact(dx, want, None, "dgrad tile %d add %s" % (tid, src is not None))
    finally:
        L.dtm_conv_set_tile(-1)


def test_conv_fwd_bn_routed_by_the_policy():
    """dtm_conv_fwd_bn at a shape the policy sends to tile 34 (128 -> 512, 150 tiles of 256 x 256): y exact, ss
    against ops/reference.py.  Tolerances: the statistics sums are exact integers, so mean = sum / M and
    rstd = rsqrt(sumsq / M - mean^2 + eps) carry a handful of fp32 roundings (2^-24 each; the variance here is far
    larger than mean^2, so no cancellation): 1e-5 relative is two orders above that.  The normalised output has
    magnitude < 16, so those roundings move it by about 16 * 4 * 2^-24 = 4e-6, and the fp32 reference by as much:
    it is compared to 1e-4 absolute."""
    L = _lib.lib()
    N, H, W, Cin, K = 75, 16, 16, 128, 512
    M = N * H * W
    g = torch.Generator().manual_seed(7)
    x = (torch.randint(0, 8, (M, Cin), generator=g) == 0).double() - (torch.randint(0, 8, (M, Cin), generator=g) == 1).double()
    w = (torch.randint(0, 8, (K, Cin), generator=g) == 0).double() - (torch.randint(0, 8, (K, Cin), generator=g) == 1).double()
    y64 = x @ w.t()
    assert float(y64.abs().max()) <= C.LIMIT and float(y64.square().sum(0).max()) < C.SUM_LIMIT
    gamma = torch.rand(K, generator=g) + 0.5
    beta = torch.randn(K, generator=g)
    xd, wd = x.to(DEV, BF).reshape(N, H, W, Cin), w.to(DEV, BF).reshape(K, 1, 1, Cin)
    y = torch.full((N, H, W, K), float("nan"), device=DEV, dtype=BF)
    ss = torch.zeros(4, K, device=DEV)
    mm, mv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    from distributed_tensorflow_models_amd.ops.geometry import conv_geom
    desc = conv_geom((N, H, W, Cin), (K, 1, 1, Cin), 1, "SAME").as_desc(_lib.ConvDesc)
    eps = 1e-3
    outs = []
    try:
        for det in (0, 1, 1):
            L.dtm_set_deterministic(det)
            rc = L.dtm_conv_fwd_bn(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(y), None, None, _lib.ptr(gd), _lib.ptr(bd),
                                   _lib.ptr(mm), _lib.ptr(mv), _lib.ptr(ss), float(M), eps, 0.9, 0, 1,
                                   ctypes.byref(desc), _lib.stream_ptr())
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert _last(L) == 34, _last(L)
            outs.append((y.clone(), ss.clone()))
    finally:
        L.dtm_set_deterministic(0)
    for yy, _ in outs:
        C.assert_exact(yy.reshape(M, K), y64, (64, 256), "conv_fwd_bn y")
    assert torch.equal(outs[1][1].view(torch.int32), outs[2][1].view(torch.int32)), "ss differs between two calls"
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    ssc = outs[0][1].double().cpu()
    torch.testing.assert_close(ssc[2], mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ssc[3], torch.rsqrt(var + eps), rtol=1e-5, atol=0)
    want = reference.batch_norm(y64.float(), gamma, beta, None, None, training=True, eps=eps)
    got = y64 * ssc[0] + ssc[1]
    torch.testing.assert_close(got, want.double(), rtol=0, atol=1e-4)


@pytest.mark.parametrize("tid,Cin,K", [(34, 128, 512), (35, 256, 256)])
def test_same_bits_as_the_256x256_tile(tid, Cin, K):
    """On ordinary (non-integer) data the 8-wave streaming forms give the bits of the 256x256 tile they replace: the
    same y (the same k order) and the same BatchNorm sums (the same statistics rows, reduced alike) - with one
    worker (three 256-pixel groups, the last partial) and with the grid's own worker count."""
    L = _lib.lib()
    N, H, W = 1, 23, 31
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, H, W, Cin, generator=g).to(DEV, BF)
    w = (torch.randn(K, 1, 1, Cin, generator=g) * 0.1).to(DEV, BF)
    from distributed_tensorflow_models_amd.ops.geometry import conv_geom
    desc = conv_geom((N, H, W, Cin), (K, 1, 1, Cin), 1, "SAME").as_desc(_lib.ConvDesc)
    out = {}
    try:
        L.dtm_set_deterministic(1)
        for key, forced, cap in (("w8", 40, 0), ("one", tid, 1), ("all", tid, 0)):
            L.dtm_conv_set_tile(forced)
            L.dtm_conv_set_stream_workers_cap(cap)
            y = torch.full((N, H, W, K), float("nan"), device=DEV, dtype=BF)
            stats = torch.zeros(2, K, device=DEV)
            rc = L.dtm_conv_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(y), _lib.ptr(stats), None, None, None, 0,
                                ctypes.byref(desc), _lib.stream_ptr())
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert _last(L) == forced, (forced, _last(L))
            out[key] = (y, stats)
    finally:
        L.dtm_conv_set_tile(-1)
        L.dtm_conv_set_stream_workers_cap(0)
        L.dtm_set_deterministic(0)
    for key in ("one", "all"):
        assert torch.equal(out[key][0].view(torch.int16), out["w8"][0].view(torch.int16)), key + ": y bits differ"
        assert torch.equal(out[key][1].view(torch.int32), out["w8"][1].view(torch.int32)), key + ": statistics bits differ"
