"""Exact-arithmetic tests of the conv kernels (csrc/kernels/conv_igemm.hip) over every tile, direction and epilogue.

The inputs (tests/conv_exact_cases.py) make every exact answer a small integer, so each kernel must reproduce the
float64 reference bit for bit: there is no tolerance, any single wrong element fails.  The C API is driven directly
with a forced tile; after every launch dtm_conv_last_tiles must report the requested id, and the matrix holds only
combinations whose effective tile is the requested one (conv_exact_cases.effective_tile), apart from the explicit
FALLBACKS list, which asserts the documented fallback id."""
import contextlib
import ctypes
import functools
import types

import pytest
import torch

import conv_exact_cases as C
from distributed_tensorflow_models_amd.ops import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# A/B knobs the matrix flips: setter and the library's default, restored after every run
KNOBS = {"stream_act": ("dtm_conv_set_stream_act", 0), "ct32": ("dtm_conv_set_direct_ct32", 1),
         "act_occ": ("dtm_conv_set_act_occ", 2), "nt_occ": ("dtm_conv_set_nt_occ", 2),
         "dec_group": ("dtm_conv_set_dec_group", 1), "dec_lpt": ("dtm_conv_set_dec_lpt", 1),
         "dec_tile": ("dtm_conv_set_dec_tile", 1), "direct_kt": ("dtm_conv_set_wgrad_direct_kt", 64)}


@contextlib.contextmanager
def forced(L, nt=-1, wgrad=-1, knobs=None):
    try:
        L.dtm_conv_set_tile(int(nt))
        L.dtm_conv_set_wgrad_tile(int(wgrad), 0)
        for k, v in (knobs or {}).items():
            getattr(L, KNOBS[k][0])(ctypes.c_int(int(v)))
        yield
        torch.cuda.synchronize()
    finally:
        L.dtm_conv_set_tile(-1)
        L.dtm_conv_set_wgrad_tile(-1, 0)
        for name, default in KNOBS.values():
            getattr(L, name)(ctypes.c_int(default))


def last_tiles(L):
    nt, wg = ctypes.c_int(-7), ctypes.c_int(-7)
    L.dtm_conv_last_tiles(ctypes.byref(nt), ctypes.byref(wg))
    return nt.value, wg.value


@functools.lru_cache(maxsize=None)
def dev(case):
    """The case's inputs on the device, uploaded once (bf16 operands, fp32 per-channel vectors)."""
    t = C.inputs(case)
    N, H, W, Cc, K, (R, S), st, pad = case
    L = _lib.lib()
    d = types.SimpleNamespace()
    for name in ("x", "w", "w_pro", "dy", "add1", "add2", "act_x", "act_r"):
        setattr(d, name, getattr(t, name).to(DEV, BF).contiguous())
    for name in ("sc", "sh", "bias"):
        setattr(d, name, getattr(t, name).to(DEV, torch.float32).contiguous())
    d.ss4 = torch.stack([d.sc, d.sh, torch.zeros_like(d.sc), torch.zeros_like(d.sc)]).contiguous()
    d.mask = C.pack_bits(t.bits).to(DEV)
    # the flipped / transposed dgrad weight wt[c][R-1-r][S-1-s][k] = w[k][r][s][c], formed here and not by the kernel
    d.wt = t.w.flip(1, 2).permute(3, 1, 2, 0).contiguous().to(DEV, BF)
    d.wt_dec = None
    if st > 1:
        d.wt_dec = torch.zeros(Cc, R, S, K, device=DEV, dtype=BF)
        L.dtm_weight_flip_transpose_dec(_lib.ptr(d.w), _lib.ptr(d.wt_dec), K, R, S, Cc, st, t.geom.pad_h, t.geom.pad_w,
                                        _lib.stream_ptr())
        torch.cuda.synchronize()
    return d


def _desc(case, dec=0):
    d = C.inputs(case).geom.as_desc(_lib.ConvDesc)
    d.dec = dec
    return d


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)  # an element no kernel writes stays a mismatch


def _what(direction, tid, case, knobs, opt, extra=""):
    return "%s tile %d %s %s %s%s" % (direction, tid, C.case_id(case), opt, knobs or "", extra)


def _ran_shape(direction, requested, ran, case, flags, table):
    """(PT, CT) of what ran; a forced id must have run (the policy, -1, may pick any known tile)."""
    if requested != -1:
        want, shape = C.effective_tile(direction, requested, case, flags)
        assert ran == want, "requested tile %d, effective_tile says %d, dtm_conv_last_tiles says %d" % (
            requested, want, ran)
        return shape
    assert ran in table, "the policy ran an unknown tile %d" % ran
    return C.effective_tile(direction, ran, case, flags)[1]


def _params(matrix):
    """pytest params with readable ids: tile, case, mode and knobs (the option list is looped inside the test)."""
    out = []
    for m in matrix:
        parts = ["t%d" % m[0], C.case_id(m[1])]
        for v in m[2:-1]:
            parts += [v] if isinstance(v, str) else ["%s%d" % kv for kv in sorted(v.items())]
        out.append(pytest.param(*m, id="-".join(parts)))
    return out


def _collect(fn, items):
    errors = []
    for it in items:
        try:
            fn(it)
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, "\n".join(errors)


# ---- forward ---------------------------------------------------------------------------------------------------------
def run_fwd(tid, case, knobs, opt, want_tile=None):
    L = _lib.lib()
    r, g, d = C.reference(case), C.inputs(case).geom, dev(case)
    N, H, W, Cc, K, (R, S), st, pad = case
    pro, stats_on, br = opt == "prologue_stats", opt in ("stats", "prologue_stats"), opt == "bias_relu"
    y = _nan((N, g.P, g.Q, K), BF)
    stats = torch.zeros(2, K, device=DEV) if stats_on else None
    desc = _desc(case)
    what = _what("fwd", tid, case, knobs, opt)
    with forced(L, nt=tid, knobs=knobs):
        rc = L.dtm_conv_fwd(_lib.ptr(d.x), _lib.ptr(d.w_pro if pro else d.w), _lib.ptr(y), _lib.ptr(stats),
                            _lib.ptr(d.bias) if br else None, _lib.ptr(d.sc) if pro else None,
                            _lib.ptr(d.sh) if pro else None, int(br), ctypes.byref(desc), _lib.stream_ptr())
        assert rc == 0, "%s: rc %d" % (what, rc)
    ran = last_tiles(L)[0]
    flags = dict(C.FWD_OPTION_FLAGS[opt], **knobs)
    if want_tile is not None:
        assert ran == want_tile, "%s: documented fallback %d, ran %d" % (what, want_tile, ran)
        shape = C.NT_TILES[ran]
    else:
        shape = _ran_shape("fwd", tid, ran, case, flags, C.NT_TILES)
    C.assert_exact(y, r.y_pro if pro else (r.y_bias_relu if br else r.y), shape, what + " y")
    if stats_on:
        C.assert_exact(stats, r.stats_pro if pro else r.stats, None, what + " stats [sum y; sum y^2]")


@pytest.mark.parametrize("tid,case,knobs,opts", _params(C.fwd_matrix()))
def test_forward_exact(tid, case, knobs, opts):
    _collect(lambda o: run_fwd(tid, case, knobs, o), opts)


# ---- dgrad -----------------------------------------------------------------------------------------------------------
def run_dgrad(tid, case, mode, knobs, opt, want_tile=None):
    L = _lib.lib()
    r, d = C.reference(case), dev(case)
    N, H, W, Cc, K, (R, S), st, pad = case
    want_dx, want_sums = r.dgrad[opt]
    fl = C.DGRAD_OPTION_FLAGS[opt]
    dec = mode == "dec"
    add = {0: None, 1: d.add1, 2: d.add2}[fl.get("add", 0)]
    act = fl.get("act")
    dx = _nan((N, H, W, Cc), BF)
    sums = torch.zeros(8, Cc, device=DEV)
    desc = _desc(case, int(dec))
    wt = d.wt_dec if dec else d.wt
    what = _what("dgrad", tid, case, knobs, opt, " " + mode)
    with forced(L, nt=tid, knobs=knobs):
        if act in ("mask", "mask_r"):
            rc = L.dtm_conv_dgrad_bnout(_lib.ptr(d.dy), _lib.ptr(wt), _lib.ptr(dx), ctypes.byref(desc), _lib.ptr(add),
                                        max(1, fl.get("add", 0)), _lib.ptr(d.mask), _lib.ptr(d.act_x),
                                        _lib.ptr(d.act_r) if act == "mask_r" else None, _lib.ptr(sums),
                                        _lib.stream_ptr())
        else:
            rc = L.dtm_conv_dgrad_ex(_lib.ptr(d.dy), _lib.ptr(wt), _lib.ptr(dx), ctypes.byref(desc), _lib.ptr(add),
                                     max(1, fl.get("add", 0)), _lib.ptr(d.act_x) if act else None,
                                     _lib.ptr(d.ss4) if act else None, _lib.ptr(sums) if act else None,
                                     int(act == "unscaled"), _lib.stream_ptr())
        assert rc == 0, "%s: rc %d" % (what, rc)
    ran = last_tiles(L)[0]
    flags = dict(fl, dec=dec)
    if want_tile is not None:
        assert ran == want_tile, "%s: documented fallback %d, ran %d" % (what, want_tile, ran)
        shape = C.NT_TILES[ran]
    else:
        shape = _ran_shape("dgrad", tid, ran, case, flags, C.NT_TILES)
    C.assert_exact(dx, want_dx, shape, what + " dx", ostr=st if dec else 1)
    want8 = torch.zeros(8, Cc, dtype=torch.float64)
    if want_sums is not None:
        want8[:want_sums.shape[0]] = want_sums
    C.assert_exact(sums, want8, None, what + " sums [8][C]")


@pytest.mark.parametrize("tid,case,mode,knobs,opts", _params(C.dgrad_matrix()))
def test_dgrad_exact(tid, case, mode, knobs, opts):
    _collect(lambda o: run_dgrad(tid, case, mode, knobs, o), opts)


# ---- wgrad -----------------------------------------------------------------------------------------------------------
def run_wgrad(tid, case, knobs, opt, ncus, want_tile=None):
    L = _lib.lib()
    r, t, d = C.reference(case), C.inputs(case), dev(case)
    pro = opt == "prologue"
    dw = t.dw0.to(DEV, torch.float32).contiguous()  # a non-zero start: the kernel adds into dW
    desc = _desc(case)
    what = _what("wgrad", tid, case, knobs, opt, " num_cus %d" % ncus)
    with forced(L, wgrad=tid, knobs=knobs):
        rc = L.dtm_conv_wgrad(_lib.ptr(d.x), _lib.ptr(d.dy), _lib.ptr(dw), _lib.ptr(d.sc) if pro else None,
                              _lib.ptr(d.sh) if pro else None, ctypes.byref(desc), int(ncus), _lib.stream_ptr())
        assert rc == 0, "%s: rc %d" % (what, rc)
    ran = last_tiles(L)[1]
    flags = dict({"prologue": pro}, **knobs)
    if want_tile is not None:
        assert ran == want_tile, "%s: documented fallback %d, ran %d" % (what, want_tile, ran)
        shape = C.WGRAD_TILES[ran]
    else:
        shape = _ran_shape("wgrad", tid, ran, case, flags, C.WGRAD_TILES)
    C.assert_exact(dw, t.dw0 + (r.dw_pro if pro else r.dw), shape, what + " dw", ncol=3)


def _cus():
    return (_lib.num_cus(), 1, 1024)  # the split count through its policy value, 1 and its ksteps cap


@pytest.mark.parametrize("tid,case,knobs,opts", _params(C.wgrad_matrix()))
def test_wgrad_exact(tid, case, knobs, opts):
    _collect(lambda a: run_wgrad(tid, case, knobs, a[0], a[1]), [(o, n) for o in opts for n in _cus()])


@pytest.mark.parametrize("tid", [-1, 10, 12])
@pytest.mark.parametrize("case,rows", C.MULTI_CASES, ids=[C.case_id(c) for c, _ in C.MULTI_CASES])
def test_wgrad_multi_exact(tid, case, rows):
    """dtm_conv_wgrad_multi: one wgrad over the members' output gradients side by side, the slabs' row ranges reduced
    into each member's own dW."""
    L = _lib.lib()
    r, t, d = C.reference(case), C.inputs(case), dev(case)
    N, H, W, Cc, K, (R, S), st, pad = case
    assert sum(rows) == K
    desc = _desc(case)

    def one(ncus):
        dws, off = [], 0
        for k in rows:
            dws.append(t.dw0[off:off + k].to(DEV, torch.float32).contiguous())
            off += k
        ptrs = (ctypes.c_void_p * len(rows))(*[x.data_ptr() for x in dws])
        rws = (ctypes.c_int * len(rows))(*rows)
        what = _what("wgrad_multi", tid, case, {}, str(rows), " num_cus %d" % ncus)
        with forced(L, wgrad=tid):
            rc = L.dtm_conv_wgrad_multi(_lib.ptr(d.x), _lib.ptr(d.dy), ptrs, rws, len(rows), ctypes.byref(desc),
                                        int(ncus), _lib.stream_ptr())
            assert rc == 0, "%s: rc %d" % (what, rc)
        shape = _ran_shape("wgrad", tid, last_tiles(L)[1], case, {"multi": 1}, C.WGRAD_TILES)
        want, off = t.dw0 + r.dw, 0
        for i, k in enumerate(rows):
            C.assert_exact(dws[i], want[off:off + k], shape, "%s member %d (rows %d..%d)" % (what, i, off, off + k),
                           ncol=3)
            off += k

    _collect(one, _cus())


# ---- the documented fallbacks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction,tid,case,option,want", C.FALLBACKS,
                         ids=["%s-t%d-%s-%s-runs%d" % (f[0], f[1], C.case_id(f[2]), f[3], f[4]) for f in C.FALLBACKS])
def test_documented_fallbacks_exact(direction, tid, case, option, want):
    """Forced ids that do not run the requested kernel: the documented tile runs instead, and is exact."""
    if direction == "fwd":
        run_fwd(tid, case, {}, option, want_tile=want)
    elif direction == "dgrad":
        run_dgrad(tid, case, "s1", {}, option, want_tile=want)
    else:
        run_wgrad(tid, case, {}, option, _lib.num_cus(), want_tile=want)


def test_unsupported_channel_counts_are_refused():
    """The entry points take C % 8 == 0, K % 4 == 0 (forward), K % 8 == 0, C % 4 == 0 (dgrad; C % 8 == 0 with a side
    epilogue) and C % 8 == 0, K % 8 == 0 (wgrad); anything else returns an error and launches nothing."""
    L = _lib.lib()
    d = dev(C.FWD_K36)
    desc = _desc(C.FWD_K36)
    before = last_tiles(L)
    buf = _nan((2, 9, 9, 40), BF)
    assert L.dtm_conv_dgrad(_lib.ptr(buf), _lib.ptr(d.wt), _lib.ptr(buf), ctypes.byref(desc), _lib.stream_ptr()) == -1
    dw = torch.zeros(36, 3, 3, 24, device=DEV)
    assert L.dtm_conv_wgrad(_lib.ptr(d.x), _lib.ptr(buf), _lib.ptr(dw), None, None, ctypes.byref(desc), _lib.num_cus(),
                            _lib.stream_ptr()) == -1
    d2, desc2 = dev(C.DGRAD_C36), _desc(C.DGRAD_C36)
    assert L.dtm_conv_fwd(_lib.ptr(d2.x), _lib.ptr(d2.w), _lib.ptr(buf), None, None, None, None, 0, ctypes.byref(desc2),
                          _lib.stream_ptr()) == -1
    assert L.dtm_conv_dgrad_ex(_lib.ptr(d2.dy), _lib.ptr(d2.wt), _lib.ptr(buf), ctypes.byref(desc2), _lib.ptr(d2.add1), 1,
                               None, None, None, 0, _lib.stream_ptr()) == -5
    torch.cuda.synchronize()
    assert last_tiles(L) == before and not dw.any()
