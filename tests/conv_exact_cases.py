"""Shared pieces of the exact-arithmetic conv tests (tests/test_conv_exact_cpu.py, tests/test_conv_exact_gpu.py).

Inputs for which the exact answer is representable: x, w, dy and add_src from {-1, 0, +1}, prologue / activation
scales from {1, 2} and shifts from {-1, 0, 1}, small integer biases.  Every bf16 x bf16 product is then an integer, every
fp32 partial sum an integer below 2^24 and every output an integer of magnitude <= 256, which bf16 holds exactly: a
correct kernel reproduces the float64 reference bit for bit whatever its k-tile order, split-K count, MFMA shape or ring
depth.  No GPU and no ctypes in this module."""
import functools
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from distributed_tensorflow_models_amd.ops.geometry import conv_geom

LIMIT = 256          # integers of magnitude <= 256 are bf16 values
SUM_LIMIT = 2 ** 24  # integer sums below 2^24 are exact in fp32 in any order

# ---- cases: (N, H, W, C, K, (R, S), stride, padding) ----------------------------------------------------------------
SMALLEST = (1, 5, 5, 8, 8, (3, 3), 1, "SAME")            # M = 25 < any tile, Kg = 72 < one k-tile
KTAIL = (2, 9, 9, 24, 40, (3, 3), 1, "SAME")             # Kg = 216 (k-tail), K = 40 (channel tail), M = 162
RAGGED_1X1 = (3, 7, 7, 512, 200, (1, 1), 1, "SAME")      # M = 147 ragged, K = 200
ODD_S2 = (4, 15, 15, 64, 96, (3, 3), 2, "SAME")          # odd extent: ungrouped parity classes, asymmetric SAME
EVEN_S2 = (2, 28, 28, 128, 128, (3, 3), 2, "SAME")       # even extent: grouped parity-class launch
ONE_CT256 = (2, 14, 14, 128, 256, (3, 3), 1, "SAME")     # one whole 256-wide channel tile, M = 392
TWO_CT256 = (2, 16, 16, 256, 512, (3, 3), 1, "SAME")     # two 256-wide tiles, 36 k-tiles: the rings wrap
DEEPEST = (3, 7, 7, 512, 512, (3, 3), 1, "SAME")         # Kg = 4608
FACT_1X7 = (2, 17, 17, 128, 128, (1, 7), 1, "SAME")
FACT_7X1 = (2, 17, 17, 160, 192, (7, 1), 1, "SAME")
STREAM_K64 = (2, 9, 9, 64, 64, (1, 1), 1, "SAME")        # streaming 1x1, Kg 64 (NKT 1)
STREAM_K128 = (2, 30, 30, 128, 64, (1, 1), 1, "SAME")    # streaming 1x1, forward Kg 128 (NKT 2)
DIRECT_32 = (2, 19, 21, 32, 32, (3, 3), 1, "SAME")       # direct kernel, ragged 8 x 16 spatial tiles
DIRECT_64 = (2, 17, 23, 64, 64, (3, 3), 1, "SAME")
DIRECT_VALID = (2, 9, 30, 64, 32, (3, 3), 1, "VALID")
FWD_K36 = (2, 9, 9, 24, 36, (3, 3), 1, "SAME")           # forward only: K % 8 != 0 (direct stores, per-wave stat rows)
DGRAD_C36 = (2, 9, 9, 36, 40, (3, 3), 1, "SAME")         # dgrad only: C % 8 != 0, the same path
SAME_EXPLICIT = (2, 16, 16, 64, 64, (3, 3), 2, (1, 1))           # policy tile only
EVEN_KERNEL = (2, 9, 9, 64, 64, (4, 4), 2, ((1, 2), (1, 2)))     # policy tile only

GEMM_CASES = [SMALLEST, KTAIL, RAGGED_1X1, ODD_S2, EVEN_S2, ONE_CT256, TWO_CT256, DEEPEST, FACT_1X7, FACT_7X1,
              STREAM_K64, STREAM_K128, DIRECT_32, DIRECT_64, DIRECT_VALID]
STREAM_CASES = [STREAM_K64, STREAM_K128]
DIRECT_CASES = [DIRECT_32, DIRECT_64, DIRECT_VALID]
POLICY_CASES = [SAME_EXPLICIT, EVEN_KERNEL]
ALL_CASES = GEMM_CASES + [FWD_K36, DGRAD_C36] + POLICY_CASES


def case_id(case):
    N, H, W, C, K, (R, S), st, pad = case
    p = pad if isinstance(pad, str) else "p" + "".join(str(v) for v in np.ravel(pad))
    return "%dx%dx%dx%d-k%d-%dx%d-s%d-%s" % (N, H, W, C, K, R, S, st, p)


def fwd_ok(case):
    return case[3] % 8 == 0 and case[4] % 4 == 0


def dgrad_ok(case):
    return case[4] % 8 == 0 and case[3] % 4 == 0


def wgrad_ok(case):
    return case[3] % 8 == 0 and case[4] % 8 == 0


# ---- the ternary inputs ---------------------------------------------------------------------------------------------
def _ternary(rs, shape, p):
    """-1 / +1 with probability p each, else 0 (float64)."""
    u = rs.random_sample(shape)
    return torch.from_numpy((u < p).astype(np.float64) - (u > 1.0 - p).astype(np.float64))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Seeded inputs of a case (float64 CPU tensors holding small integers)."""
    N, H, W, C, K, (R, S), st, pad = case
    g = conv_geom((N, H, W, C), (K, R, S, C), st, pad)
    rs = np.random.RandomState(zlib.crc32(case_id(case).encode()) & 0x7FFFFFFF)
    pw = 0.25 * (0.5 if R * S * C > 1200 else 1.0)
    t = types.SimpleNamespace(case=case, geom=g)
    t.x = _ternary(rs, (N, H, W, C), 0.25)
    t.w = _ternary(rs, (K, R, S, C), pw)
    # under the prologue the operand is relu(x*sc + sh) in {0 .. 3}: half the weight density again
    t.w_pro = t.w * torch.from_numpy((rs.random_sample((K, R, S, C)) < 0.5).astype(np.float64))
    t.dy = _ternary(rs, (N, g.P, g.Q, K), 0.25)
    t.sc = torch.from_numpy(rs.randint(1, 3, C).astype(np.float64))       # {1, 2}
    t.sh = torch.from_numpy(rs.randint(-1, 2, C).astype(np.float64))      # {-1, 0, 1}
    t.bias = torch.from_numpy(rs.randint(-3, 4, K).astype(np.float64))
    t.add1 = _ternary(rs, (N, H, W, C), 0.25)
    t.add2 = _ternary(rs, (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), 0.25)
    t.act_x = _ternary(rs, (N, H, W, C), 0.3)   # x*sc + sh hits 0 exactly on a large share of the elements
    t.act_r = _ternary(rs, (N, H, W, C), 0.3)
    t.bits = torch.from_numpy((rs.random_sample((N, H, W, C)) > 0.4).astype(np.float64))
    t.dw0 = torch.from_numpy(rs.randint(-4, 5, (K, R, S, C)).astype(np.float64))
    return t


def pack_bits(bits):
    """ReLU bitmask of the block-output dgrad: bit e of byte (row*C + c) / 8 is channel c + e (uint8 tensor)."""
    return torch.from_numpy(np.packbits(bits.numpy().astype(bool).reshape(-1), bitorder="little"))


# ---- the float64 reference ------------------------------------------------------------------------------------------
def conv_fwd64(x, w, g):
    """float64 NHWC conv with the project's own pads (geometry.conv_geom): x [N,H,W,C], w [K,R,S,C]."""
    xp = F.pad(x.permute(0, 3, 1, 2), (g.pad_w, g.pad_r, g.pad_h, g.pad_b))
    y = F.conv2d(xp, w.permute(0, 3, 1, 2), None, g.stride, 0)
    return y[:, :, :g.P, :g.Q].permute(0, 2, 3, 1).contiguous()


def prologue64(x, sc, sh):
    """The forward / wgrad prologue relu(x*sc + sh); the conv pads the result with zeros (padding stays zero)."""
    return torch.relu(x * sc + sh)


def _grads(x, w, dy, g):
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    conv_fwd64(xr, wr, g).backward(dy)
    return xr.grad, wr.grad


def stats64(y):
    K = y.shape[-1]
    y2 = y.reshape(-1, K)
    return torch.stack([y2.sum(0), y2.square().sum(0)])


def add_strided(dx, add, stride):
    """dx + add_src: stride 1 element-wise; stride s: add_src is the gradient of x[:, ::s, ::s]."""
    out = dx.clone()
    if stride == 1:
        out += add
    else:
        out[:, ::stride, ::stride] += add
    return out


def act64(total, act_x, sc, sh, unscaled):
    """Activation-backward epilogue: g = [act_x*sc + sh > 0] * total, out = g (unscaled) or g*sc,
    sums = (sum g*act_x, sum g) per channel.  Returns (out, g, sums [2][C])."""
    C = total.shape[-1]
    g = total * ((act_x * sc + sh) > 0).to(total.dtype)
    sums = torch.stack([(g * act_x).reshape(-1, C).sum(0), g.reshape(-1, C).sum(0)])
    return (g if unscaled else g * sc), g, sums


def bnout64(total, bits, x_raw, r_raw):
    """Block-output epilogue: g = total * bit; the [8][C] sums table: rows 0-1 = (sum g*x_raw, sum g), rows 4-5 =
    (sum g*r_raw, sum g) with a BN'd residual, every other row untouched (zero)."""
    C = total.shape[-1]
    g = total * bits
    sums = torch.zeros(8, C, dtype=total.dtype)
    sums[0] = (g * x_raw).reshape(-1, C).sum(0)
    sums[1] = g.reshape(-1, C).sum(0)
    if r_raw is not None:
        sums[4] = (g * r_raw).reshape(-1, C).sum(0)
        sums[5] = sums[1]
    return g, sums


DGRAD_OPTIONS = ("plain", "add1", "add2", "act_unscaled", "act_scaled", "add1_act", "mask", "mask_r_add1")
FWD_OPTIONS = ("plain", "stats", "prologue_stats", "bias_relu")


def dgrad_option(t, dx, option):
    """(dx_out, sums or None) of one dgrad option from the plain dgrad dx."""
    if option == "plain":
        return dx, None
    if option == "add1":
        return add_strided(dx, t.add1, 1), None
    if option == "add2":
        return add_strided(dx, t.add2, 2), None
    if option == "act_unscaled":
        out, _, sums = act64(dx, t.act_x, t.sc, t.sh, True)
        return out, sums
    if option == "act_scaled":
        out, _, sums = act64(dx, t.act_x, t.sc, t.sh, False)
        return out, sums
    if option == "add1_act":
        out, _, sums = act64(add_strided(dx, t.add1, 1), t.act_x, t.sc, t.sh, False)
        return out, sums
    if option == "mask":
        return bnout64(dx, t.bits, t.act_x, None)
    if option == "mask_r_add1":
        return bnout64(add_strided(dx, t.add1, 1), t.bits, t.act_x, t.act_r)
    raise ValueError(option)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 reference of everything the tests compare, computed once per case and never modified."""
    t = inputs(case)
    g = t.geom
    r = types.SimpleNamespace(case=case, inputs=t, geom=g)
    r.y = conv_fwd64(t.x, t.w, g)
    r.xin = prologue64(t.x, t.sc, t.sh)
    r.y_pro = conv_fwd64(r.xin, t.w_pro, g)
    r.y_pre_relu = r.y + t.bias
    r.y_bias_relu = torch.relu(r.y_pre_relu)
    r.stats = stats64(r.y)
    r.stats_pro = stats64(r.y_pro)
    r.dx, r.dw = _grads(t.x, t.w, t.dy, g)
    _, r.dw_pro = _grads(r.xin, t.w, t.dy, g)
    r.dgrad = {}
    for opt in DGRAD_OPTIONS:
        if opt != "plain" and case[3] % 8:
            continue  # the side epilogues need C % 8 == 0
        r.dgrad[opt] = dgrad_option(t, r.dx, opt)
    return r


def _is_int(v):
    return bool(torch.equal(v, v.round()))


def check_exact_conditions(ref):
    """The conditions under which a correct kernel must equal the reference bit for bit (conditions on the inputs,
    asserted on the float64 reference): every element an integer of magnitude <= 256 (the dgrad before and after the
    add included), every per-channel sum of magnitudes below 2^24."""
    t, g = ref.inputs, ref.geom
    N, H, W, C, K, (R, S), st, pad = ref.case
    what = case_id(ref.case)
    outs = {"y": ref.y, "y_pro": ref.y_pro, "y+bias": ref.y_pre_relu, "relu(y+bias)": ref.y_bias_relu,
            "dx": ref.dx, "dx+add1": add_strided(ref.dx, t.add1, 1), "dx+add2": add_strided(ref.dx, t.add2, 2),
            "dw": ref.dw, "dw_pro": ref.dw_pro, "dw0+dw": t.dw0 + ref.dw, "dw0+dw_pro": t.dw0 + ref.dw_pro}
    for opt, (out, sums) in ref.dgrad.items():
        outs["dgrad[%s]" % opt] = out
    for name, v in outs.items():
        assert _is_int(v), "%s: %s is not integral" % (what, name)
        if not name.startswith("dw"):  # (dW is fp32: the sum bound below covers it)
            assert float(v.abs().max()) <= LIMIT, "%s: max|%s| = %g > %d" % (what, name, float(v.abs().max()), LIMIT)
    # fp32 accumulators: the sum of magnitudes bounds every partial sum in any order
    xmax = float(max(t.x.abs().max(), ref.xin.abs().max()))
    assert R * S * C * xmax < SUM_LIMIT and R * S * K < SUM_LIMIT, what      # forward / dgrad reductions
    M = N * g.P * g.Q
    assert M * xmax + float(t.dw0.abs().max()) < SUM_LIMIT, what              # every dW term sum (|dy| <= 1)
    for name, y in (("y", ref.y), ("y_pro", ref.y_pro)):
        y2 = y.reshape(-1, K)
        assert float(y2.abs().sum(0).max()) < SUM_LIMIT, "%s: sum|%s|" % (what, name)
        assert float(y2.square().sum(0).max()) < SUM_LIMIT, "%s: sum %s^2" % (what, name)
    for tot in (ref.dx, outs["dx+add1"]):
        assert float(tot.abs().reshape(-1, C).sum(0).max()) < SUM_LIMIT, "%s: sum|g|, sum|g*x|, sum|g*r|" % what
    for opt, (out, sums) in ref.dgrad.items():
        if sums is not None:
            assert _is_int(sums) and float(sums.abs().max()) < SUM_LIMIT, "%s: sums of %s" % (what, opt)
    assert _is_int(ref.stats) and _is_int(ref.stats_pro), what


# ---- the comparison -------------------------------------------------------------------------------------------------
def _locate(coord, shape, ncol, tile_shape, ostr):
    """Tile coordinates of one element: rows = the leading dims (pixels n, h, w; dW: k), columns = the last ncol dims."""
    PT, CT = tile_shape
    rows, cols = shape[:len(shape) - ncol], shape[len(shape) - ncol:]
    col = int(np.ravel_multi_index(coord[len(rows):], cols))
    s = "ctile %d+%d" % (col // CT, col % CT)
    if isinstance(PT, (tuple, list)):  # spatial pixel tiles (TH, TW) of the direct kernel
        n, h, w = coord[:3]
        return "ptile (n %d, th %d, tw %d)+(%d, %d) %s" % (n, h // PT[0], w // PT[1], h % PT[0], w % PT[1], s)
    if ostr > 1:  # stride-decomposed dgrad: one launch (or z-slice) per output parity class
        n, h, w = coord[:3]
        a, b = h % ostr, w % ostr
        Hc, Wc = (shape[1] - a + ostr - 1) // ostr, (shape[2] - b + ostr - 1) // ostr
        m = (n * Hc + h // ostr) * Wc + w // ostr
        return "class (%d, %d) ptile %d+%d %s" % (a, b, m // PT, m % PT, s)
    m = int(np.ravel_multi_index(coord[:len(rows)], rows))
    return "ptile %d+%d %s" % (m // PT, m % PT, s)


def assert_exact(got, ref, tile_shape=None, what="", ncol=1, ostr=1):
    """got == ref.to(got.dtype) by value (-0.0 == 0.0; no bit views).  On mismatch: the count and the first eight
    coordinates with got / want and, with tile_shape = (PT, CT), each element's pixel-tile and channel-tile index and
    its offset inside the tile (PT = (TH, TW): spatial tiles; ncol: trailing dims that form the column index, 3 for
    dW [K][R][S][C]; ostr: the parity classes of a stride-decomposed dgrad)."""
    got = got.detach().cpu()
    want = ref.detach().cpu().to(got.dtype)
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = torch.nonzero(~(got == want))  # (a NaN in got is a mismatch too)
    lines = ["%s: %d of %d elements differ from the exact reference" % (what, bad.shape[0], got.numel())]
    for c in bad[:8].tolist():
        c = tuple(c)
        s = "  %s got %r want %r" % (c, float(got[c]), float(want[c]))
        if tile_shape is not None:
            s += "  [" + _locate(c, tuple(got.shape), ncol, tile_shape, ostr) + "]"
        lines.append(s)
    raise AssertionError("\n".join(lines))


# ---- which kernel a forced tile id really runs ------------------------------------------------------------------------
# (PT, CT) of the conv_nt tile ids (forward / dgrad): pixels x output channels per block
NT_TILES = {0: (128, 128), 3: (128, 64), 4: (64, 128), 21: (128, 128), 24: (256, 64), 26: (128, 64), 32: (256, 32),
            30: (64, 128), 31: (64, 64), 40: (256, 256), 41: (256, 256), 60: ((8, 16), 32)}
# (MT, NT) of the wgrad tile ids: dW rows (K) x columns (R*S*C) per block; 20 = the direct 3x3 kernel (all columns)
WGRAD_TILES = {0: (128, 128), 1: (64, 128), 6: (32, 128), 7: (64, 256), 8: (64, 256), 10: (128, 128), 11: (64, 256),
               12: (256, 256), 13: (256, 256), 14: (64, 256), 15: (64, 256), 16: (64, 256), 20: (64, 1 << 30)}
GEMM_IDS = (0, 3, 4, 21, 24, 26, 32, 40, 41)
WGRAD_IDS = (0, 1, 6, 7, 8, 10, 11, 12, 13)


def _nt_args(direction, case, options):
    """The fields of the kernel's launch arguments that the fallback rules read (conv_fwd_impl / conv_dgrad_impl)."""
    N, H, W, C, K, (R, S), st, pad = case
    g = conv_geom((N, H, W, C), (K, R, S, C), st, pad)
    a = types.SimpleNamespace(R=R, S=S, stride=st, bias=bool(options.get("bias")), relu=bool(options.get("relu")),
                              pro=bool(options.get("prologue")), add=options.get("add", 0), act=options.get("act"),
                              ostr=1)
    if direction == "fwd":
        a.C, a.K, a.Hin, a.Win, a.Hv, a.Wv, a.P, a.Q = C, K, H, W, H, W, g.P, g.Q
        a.pad_h, a.pad_w = g.pad_h, g.pad_w
    else:  # the dilated dgrad: a stride-1 conv over dy (zero-dilated when the forward stride is 2)
        a.C, a.K, a.Hin, a.Win, a.P, a.Q = K, C, g.P, g.Q, H, W
        a.Hv, a.Wv = (g.P - 1) * st + 1, (g.Q - 1) * st + 1
        a.pad_h, a.pad_w = R - 1 - g.pad_h, S - 1 - g.pad_w
        a.stride = 1
        a.pro = False
    a.Kg = R * S * a.C
    return a


def _stream_ok(a):
    return (not a.bias and not a.relu and a.R == 1 and a.S == 1 and a.stride == 1 and a.pad_h == 0 and a.pad_w == 0 and
            a.Hv == a.Hin and a.Wv == a.Win and a.P == a.Hin and a.Q == a.Win and a.Kg % 64 == 0 and a.Kg <= 128 and
            a.K % 8 == 0 and (not a.pro or a.C <= 512) and a.ostr == 1)


def _direct_ok(a):
    return (a.R == 3 and a.S == 3 and a.stride == 1 and a.Hv == a.Hin and a.Wv == a.Win and a.C in (32, 64) and
            a.K % 32 == 0 and not a.pro and not a.bias and not a.relu and a.ostr == 1 and a.pad_h <= 2 and
            a.pad_w <= 2 and a.act not in ("mask", "mask_r") and (not a.add or a.add == 1))


def effective_tile(direction, forced_id, case, options=None):
    """(id, (PT, CT)) of the kernel that a forced tile id really runs: the fallback rules of pick_tile_impl (fwd, dgrad)
    and of the wgrad remap in conv_wgrad_impl, with every A/B knob at its default.  The single table of tile ids of
    the tests.  options: prologue, bias, relu, add (0 / 1 / 2 = add_src stride), act (None, "scaled", "unscaled",
    "mask", "mask_r"), dec (stride-decomposed dgrad), ct32 (dtm_conv_set_direct_ct32, default 1), multi (row-split
    wgrad), direct_kt (dtm_conv_set_wgrad_direct_kt, default 64).  forced_id -1 (the shape policy) returns
    (-1, None): the policy depends on the device's CU count, the tests read what ran."""
    options = dict(options or {})
    N, H, W, C, K, (R, S), st, pad = case
    if forced_id == -1:
        return -1, None
    if direction == "wgrad":
        g = conv_geom((N, H, W, C), (K, R, S, C), st, pad)
        pro = bool(options.get("prologue"))
        if (forced_id == 20 and not options.get("multi") and R == 3 and S == 3 and st == 1 and C in (32, 64) and
                K % 32 == 0 and g.pad_h <= 2 and g.pad_w <= 2 and g.P == H + 2 * g.pad_h - 2 and
                g.Q == W + 2 * g.pad_w - 2):
            return 20, (64 if K % 64 == 0 and options.get("direct_kt", 64) == 64 else 32, 1 << 30)
        wt = forced_id
        if 10 <= wt <= 13 and pro:
            wt = 1 if K <= 64 else 0  # no x prologue in the pipelined kernels
        if 14 <= wt <= 16:
            wt = 1 if K <= 64 else 0  # the BN-fused stem tiles: dtm_conv_wgrad_bnbwd only
        if wt not in WGRAD_IDS:
            wt = 0
        return wt, WGRAD_TILES[wt]
    a = _nt_args(direction, case, options)
    dec = direction == "dgrad" and options.get("dec") and st > 1
    if dec:  # per parity class: a stride-1 conv with the class's taps and a strided output (ostr = st)
        a.ostr, a.Hv, a.Wv, a.R, a.S = st, a.Hin, a.Win, 0, 0
    fid = forced_id
    if fid == 60 and _direct_ok(a):
        ct = 32 if (a.add or a.act or options.get("ct32", 1) or a.K % 64) else 64
        return 60, ((8, 16), ct)
    if fid in (21, 24, 26, 32) and a.pro and a.C > 512:
        fid = 0
    if fid in (40, 41) and a.pro:
        fid = 0
    if fid == 41 and a.K % 8:
        fid = 40  # the ping-pong tile has only the LDS-staged epilogue
    if fid in (30, 31) and not _stream_ok(a):
        fid = 3 if a.K <= 64 else 4
    if fid not in NT_TILES or fid == 60:
        fid = 0
    return fid, NT_TILES[fid]


# ---- the GPU matrix (tests/test_conv_exact_gpu.py runs it; tests/test_conv_exact_cpu.py checks its conditions) ----------
FWD_IDS = (-1,) + GEMM_IDS
FWD_OPTION_FLAGS = {"plain": {}, "stats": {}, "prologue_stats": {"prologue": 1}, "bias_relu": {"bias": 1, "relu": 1}}
DGRAD_OPTION_FLAGS = {"plain": {}, "add1": {"add": 1}, "add2": {"add": 2}, "act_unscaled": {"act": "unscaled"},
                      "act_scaled": {"act": "scaled"}, "add1_act": {"add": 1, "act": "scaled"}, "mask": {"act": "mask"},
                      "mask_r_add1": {"add": 1, "act": "mask_r"}}
# row-split weight gradients (dtm_conv_wgrad_multi): (case, rows)
MULTI_CASES = [((2, 9, 9, 288, 208, (1, 1), 1, "SAME"), (64, 48, 64, 32)),
               ((2, 9, 9, 256, 256, (1, 1), 1, "SAME"), (192, 64))]
# forced ids that do NOT run the requested kernel, kept on purpose: (direction, forced id, case, option, documented id)
FALLBACKS = [("fwd", 40, ONE_CT256, "prologue_stats", 0), ("fwd", 41, ONE_CT256, "prologue_stats", 0),
             ("fwd", 30, KTAIL, "stats", 3), ("fwd", 31, ONE_CT256, "stats", 4), ("fwd", 60, EVEN_S2, "plain", 0),
             ("fwd", 60, ONE_CT256, "plain", 0), ("fwd", 41, FWD_K36, "stats", 40), ("fwd", 27, KTAIL, "stats", 0),
             ("fwd", 30, STREAM_K64, "bias_relu", 3), ("dgrad", 60, DIRECT_64, "mask", 0),
             ("dgrad", 30, ONE_CT256, "plain", 4), ("dgrad", 22, KTAIL, "plain", 0),
             ("wgrad", 10, ONE_CT256, "prologue", 0), ("wgrad", 12, STREAM_K64, "prologue", 1),
             ("wgrad", 20, ONE_CT256, "plain", 0), ("wgrad", 9, KTAIL, "plain", 0), ("wgrad", 15, KTAIL, "plain", 1)]


def _runs(direction, tid, case, flags):
    return tid == -1 or effective_tile(direction, tid, case, flags)[0] == tid


def fwd_matrix():
    """[(tile id, case, knobs, [options])]: only combinations that run the requested kernel."""
    out = []
    for case in GEMM_CASES + [FWD_K36] + POLICY_CASES:
        ids = (-1,) if case in POLICY_CASES else FWD_IDS + (30, 31, 60)
        for tid in ids:
            for knobs in (({"ct32": 0}, {"ct32": 1}) if tid == 60 else ({},)):
                opts = [o for o in FWD_OPTIONS if _runs("fwd", tid, case, dict(FWD_OPTION_FLAGS[o], **knobs))]
                if opts:
                    out.append((tid, case, knobs, opts))
    return out


def dgrad_matrix():
    """[(tile id, case, mode, knobs, [options])]; mode: "s1" (stride 1), "dilated" (stride 2, d.dec = 0), "dec"
    (stride-decomposed, d.dec = 1); knobs: the A/B setters to flip for this run."""
    out = []
    for case in GEMM_CASES + [DGRAD_C36] + POLICY_CASES:
        st = case[6]
        ids = (-1,) if case in POLICY_CASES else FWD_IDS + (30, 31, 60)
        for tid in ids:
            for mode in (("s1",) if st == 1 else ("dilated", "dec")):
                variants = [{}]
                if mode == "dec" and case == EVEN_S2:
                    variants += [{"dec_group": 0}, {"dec_lpt": 0}] + ([{"dec_tile": 0}] if tid == -1 else [])
                if tid in (30, 31):
                    variants = [{"stream_act": 1}]
                for knobs in variants:
                    opts = []
                    for o in DGRAD_OPTIONS:
                        if o != "plain" and case[3] % 8:
                            continue
                        flags = dict(DGRAD_OPTION_FLAGS[o], dec=mode == "dec")
                        if _runs("dgrad", tid, case, flags):
                            opts.append(o)
                    if opts:
                        out.append((tid, case, mode, knobs, opts))
    # the occupancy variants of the register-staged tiles 3 / 4: side epilogue (act_occ) and plain (nt_occ)
    for tid in (3, 4):
        for v in (0, 1, 2, 3):
            out.append((tid, ONE_CT256, "s1", {"act_occ": v}, ["add1_act", "mask_r_add1", "add2"]))
            out.append((tid, FACT_1X7, "s1", {"nt_occ": v}, ["plain"]))
    return out


def wgrad_matrix():
    """[(tile id, case, knobs, [options])]; options: "plain", "prologue"."""
    out = []
    for case in GEMM_CASES + POLICY_CASES:
        ids = (-1,) if case in POLICY_CASES else (-1,) + WGRAD_IDS + (20,)
        for tid in ids:
            for knobs in (({"direct_kt": 32}, {"direct_kt": 64}) if tid == 20 else ({},)):
                opts = [o for o in ("plain", "prologue")
                        if _runs("wgrad", tid, case, dict({"prologue": o == "prologue"}, **knobs))]
                if opts:
                    out.append((tid, case, knobs, opts))
    return out


def matrix_cases():
    """Every case the GPU matrix touches (the row-split and the fallback cases included)."""
    cs = [m[1] for m in fwd_matrix()] + [m[1] for m in dgrad_matrix()] + [m[1] for m in wgrad_matrix()]
    cs += [c for c, _ in MULTI_CASES] + [f[2] for f in FALLBACKS]
    seen = []
    for c in cs:
        if c not in seen:
            seen.append(c)
    return seen
