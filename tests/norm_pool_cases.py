"""Shared pieces of the per-element BatchNorm / pooling / LRN tests (tests/test_norm_pool_cpu.py and
tests/test_norm_pool_gpu.py): seeded inputs, plain float64 references of the operations and the tolerance formulas,
each derived from the arithmetic the kernels do.  No GPU and no ctypes in this module.

Number formats.  bf16 keeps 8 significant bits, so one round-to-nearest costs at most 2^-8 / (1 + 2^-8) of the value
(attained just above a power of two); the tests charge BF16 = 2^-8 per output rounding.  (2^-9 is the AVERAGE relative
half ulp, not a bound: fp64 1 + 2^-8 - 2^-12 rounds to 1.0, an error of 0.94 * 2^-8; tests/test_norm_pool_cpu.py
shows the correctly rounded float64 reference itself violating a 2^-9 bound.)  fp32: u = 2^-24 per rounded operation.

BatchNorm forward bound, per element (a = |x sc|, m = |mean sc|, B = |beta|, R = |res|):

    |y - y64| <= BF16 |y64| + BN_K 2^-23 (a + m + B + R) + kappa 2^-22 |xhat gamma|,  kappa = E[x^2] / (var + eps)

  The kernels compute (bn_finalize_kernel, bn_apply_*):
    mean = S / M;  var = max(Q / M - mean mean, 0);  rstd = rsqrtf(var + eps);  sc = g rstd;  sh = b - mean sc;
    y = bf16(max(fma(x, sc, sh) + res, 0)).
  The per-channel sums S = sum x and Q = sum x^2 are charged ONE rounding each, relative to their own value: the
  accumulation is taken to be no worse than a correctly rounded fp32 sum ("fp32-naive").  First-order count, in u:
    var + eps:  Q 1 + Q/M 1 -> 2 E[x^2];  mean (S 1 + S/M 1) twice + the product 1 -> 5 mean^2;  the subtraction 1 var;
                + eps 1 (var + eps)   =>  <= 7 E[x^2] + 2 (var + eps)      [mean^2, var <= E[x^2]]
    rstd:       half of that relative to var + eps, plus rsqrtf (1 ulp = 2 u, HIP math API)  =>  3.5 kappa + 3
    sc:         + 1 for g * rstd  =>  3.5 kappa + 4
  The kappa part scales x sc - mean sc = xhat gamma: 3.5 kappa u <= kappa 2^-22, the conditioning term - what
  E[x^2] - mean^2 costs in fp32.  The rest, per magnitude:
    a:  sc 4 + fma 1 + residual add 1                                              = 6
    m:  sc 4 + mean 2 + mean * sc 1 + b - (.) 1 + fma 1 + residual add 1           = 10
    B:  b - (.) 1 + fma 1 + residual add 1                                         = 3
    R:  residual add 1                                                             = 1
  so BN_K 2^-23 = 10 u covers every coefficient: BN_K = 5.  ReLU is exact.

Margins of the kernel's formula evaluated in torch fp32 on the CPU (max over all elements of |error| / bound, printed
by tests/test_norm_pool_cpu.py::test_bn_fp32_emulation_meets_the_bounds): 0.97 - 0.996 on every case (0.92 and 0.98 on the
conditioning case, x = 8 + 0.25 randn, kappa up to 1141): that figure is the bf16 rounding alone, some element always
sits just above a power of two.  The error BEFORE the bf16 rounding against the bound without its BF16 term - the
share the fp32 arithmetic uses of its own part - is 0.16 - 0.28 on the ordinary cases and 0.43 on the conditioning
case; without the kappa term the conditioning case fails (test_bn_conditioning_term_is_needed)."""
import functools
import types

import torch

from distributed_tensorflow_models_amd.ops.geometry import pool_geom

BF = torch.bfloat16
F64 = torch.float64
BF16 = 2.0 ** -8     # one bf16 rounding, relative
U = 2.0 ** -24       # one fp32 rounding, relative
SUM_LIMIT = 2 ** 24  # integer sums below 2^24 are exact in fp32 in any order
BN_K = 5
EPS = 1e-3
DECAY = 0.9


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# =====================================================================================================================
# BatchNorm
# =====================================================================================================================
# ---- the launch arithmetic of csrc/kernels/batchnorm.hip, re-stated ----
FU = 4


def fast_ok(M, C):
    return C % 8 == 0 and C // 8 <= 256 and M < 2 ** 31 and M * C < 2 ** 40


def fast_grid(M, C):
    cols = C // 8
    RP = 256 // cols
    b = min(max(M * cols // (256 * 8), 1), 2048)
    r = -(-M // b)
    r = -(-r // RP) * RP
    return -(-M // r), r


def rows_per_block_for(M, C):
    return max(-(-M // 1024), 64)


def bn_path(shape):
    """Where ops.nn.batch_norm's kernels land for an NHWC shape: the kernel family, its grid and what follows from it."""
    C = shape[-1]
    M = 1
    for d in shape[:-1]:
        M *= d
    if fast_ok(M, C):
        blocks, rpb = fast_grid(M, C)
        cols = C // 8
        RP = 256 // cols
        last = M - (blocks - 1) * rpb
        return dict(kind="fast", blocks=blocks, rpb=rpb, cols=cols, RP=RP, idle_lanes=256 - RP * cols,
                    last_rows=last, ragged_rp=last % RP != 0, ragged_fu=last % (RP * FU) != 0,
                    reduce="few" if blocks <= 32 else "rows4")
    rpb = rows_per_block_for(M, C)
    V = 8 if C % 8 == 0 else 1
    cols = C // V
    return dict(kind="gen%d" % V, blocks=-(-M // rpb), rpb=rpb, cols=cols, atomic_cols=cols >= 256,
                cb_rounds=-(-cols // 256))


# name -> (NHWC shape, the properties of bn_path the case is there for)
BN_CASES = {
    # fast path, one block: the shape tests/test_kernels_gpu.py::test_batch_norm uses
    "fast-1blk": ((4, 7, 7, 64), dict(kind="fast", blocks=1, reduce="few")),
    # fast path, 3 blocks of 288 rows, the last one (201 rows) ragged against RP = 32 and RP * FU = 128
    "fast-ragged": ((3, 7, 37, 64), dict(kind="fast", blocks=3, ragged_rp=True, ragged_fu=True, reduce="few")),
    # cols = 5 does not divide 256: RP = 51, one idle lane per block; 3 blocks, ragged last
    "fast-cols5": ((3, 21, 21, 40), dict(kind="fast", blocks=3, idle_lanes=1, ragged_rp=True, reduce="few")),
    # 33 partial rows: dtm_reduce_rows leaves the few-row kernel (4x46x46 would give 30 blocks: rpb rounds up to 288)
    "fast-33blk": ((4, 47, 50, 64), dict(kind="fast", blocks=33, ragged_rp=True, ragged_fu=True, reduce="rows4")),
    # cols = 256, RP = 1 (no LDS tree), 34 blocks of 9 rows, the last with 3
    "fast-c2048": ((3, 10, 10, 2048), dict(kind="fast", blocks=34, RP=1, ragged_fu=True, reduce="rows4")),
    # generic <1>: 4 blocks of 64 rows (the last with 8); rpi = 85 / 7 row lanes
    "gen1-c3": ((2, 10, 10, 3), dict(kind="gen1", blocks=4, atomic_cols=False)),
    "gen1-c36": ((2, 10, 10, 36), dict(kind="gen1", blocks=4, atomic_cols=False)),
    # generic <1>, cols >= 256: the per-lane atomic branch, two cb rounds
    "gen1-c300": ((2, 10, 10, 300), dict(kind="gen1", blocks=4, atomic_cols=True, cb_rounds=2)),
    # generic <8>: C / 8 = 257 > 256
    "gen8-c2056": ((2, 10, 10, 2056), dict(kind="gen8", blocks=4, atomic_cols=True, cb_rounds=2)),
}
BN_COND = "cond"  # the conditioning case: x = 8 + 0.25 randn on the fast-ragged shape
BN_COND_SHAPE = BN_CASES["fast-ragged"][0]


def bn_shape(name):
    return BN_COND_SHAPE if name == BN_COND else BN_CASES[name][0]


@functools.lru_cache(maxsize=None)
def bn_exact_input(name):
    """Integers |x| <= 3 (bf16 values) and their float64 per-channel sums [2][C]: exact in fp32 in any order."""
    shape = bn_shape(name)
    x = torch.randint(-3, 4, shape, generator=_gen(1, *shape)).to(F64)
    x2 = x.reshape(-1, shape[-1])
    sums = torch.stack([x2.sum(0), (x2 * x2).sum(0)])
    return x, sums


@functools.lru_cache(maxsize=None)
def bn_random_input(name):
    """bf16-valued float64 x, res, dy; fp32-valued float64 gamma, beta, moving statistics."""
    shape = bn_shape(name)
    C = shape[-1]
    g = _gen(2, *shape, name == BN_COND)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x = (8 + 0.25 * rn(shape)) if name == BN_COND else (1.5 * rn(shape) + 0.5)
    return types.SimpleNamespace(
        x=x.to(BF).to(F64), res=rn(shape).to(BF).to(F64), dy=rn(shape).to(BF).to(F64),
        gamma=(torch.rand(C, generator=g) + 0.5).to(F64), beta=rn(C).to(F64),
        mm=(0.5 * rn(C)).to(F64), mv=(torch.rand(C, generator=g) + 0.5).to(F64))


def bn_forward64(x, gamma, beta, res, relu, mm=None, mv=None, bessel=True, eps=EPS, decay=DECAY):
    """Training-mode batch norm in float64 with everything the bounds need."""
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    M = x2.shape[0]
    mean = x2.mean(0)
    ex2 = (x2 * x2).mean(0)
    var = ((x2 - mean) ** 2).mean(0)
    rstd = (var + eps) ** -0.5
    sc = gamma * rstd
    xhat = ((x2 - mean) * rstd).reshape(x.shape)
    pre = xhat * gamma + beta
    if res is not None:
        pre = pre + res
    y = pre.clamp(min=0) if relu else pre
    o = types.SimpleNamespace(M=M, mean=mean, ex2=ex2, var=var, rstd=rstd, sc=sc, xhat=xhat, pre=pre, y=y,
                              kappa=ex2 / (var + eps))
    o.tol = (BF16 * y.abs() + BN_K * 2.0 ** -23 * ((x * sc).abs() + (mean * sc).abs() + beta.abs()
                                                    + (res.abs() if res is not None else 0.0))
             + o.kappa * 2.0 ** -22 * (xhat * gamma).abs())
    if mm is not None:
        # moving_x -= (moving_x - batch_x) * (1 - decay) in fp32.  decay reaches the kernel rounded to fp32 (u |d|) and
        # 1 - d rounds once more; the difference, the product and the final subtraction round once each; the batch
        # mean carries 2 u (sum, division); the batch variance u (7 E[x^2] + var) (the count above without eps), and
        # Bessel's var * M / (M - 1) two more roundings.
        od = 1.0 - decay
        dd = U * (abs(decay) + abs(od))
        bess = M / (M - 1.0) if (bessel and M > 1) else 1.0
        uvar = var * bess
        dvar = bess * (U * (7 * ex2 + var) + (2 * U * var if bess != 1.0 else 0.0))
        for name, mov, batch, dbatch in (("mm", mm, mean, 2 * U * mean.abs()), ("mv", mv, uvar, dvar)):
            diff = mov - batch
            new = mov - diff * od
            setattr(o, name, new)
            setattr(o, name + "_tol", U * (new.abs() + 2 * (diff * od).abs()) + diff.abs() * dd + dbatch * abs(od))
    return o


def bn_backward64(f, x, gamma, dy, mask):
    """Gradients of bn_forward64's output f for the incoming dy, the ReLU mask given (None: no ReLU), with bounds.

    g = dy mask;  dbeta = sum g;  dgamma = sum g xhat;  dx = sc (g - sum g / M - xhat sum(g xhat) / M);  dres = g.
    dbeta / dgamma: any-order fp32 summation over M terms, M 2^-23 sum|.|.  dgamma adds the fp32 error of the kernel's
    xhat = (x - mean) rstd: |xhat| (rstd's 3.5 kappa + 3, the subtraction and the product: (3.5 kappa + 5) u) +
    rstd 2 u |mean| (the mean's two roundings).  dx: one bf16 rounding of a sum of three terms, bounded through their
    magnitudes: 2^-8 |sc| (|g| + sum|g| / M + |xhat| sum|g xhat| / M); the fp32 roundings are four orders below it."""
    M, C = f.M, x.shape[-1]
    g = dy if mask is None else dy * mask
    g2, xh2 = g.reshape(-1, C), f.xhat.reshape(-1, C)
    sg, sgx = g2.sum(0), (g2 * xh2).sum(0)
    ag, agx = g2.abs().sum(0), (g2 * xh2).abs().sum(0)
    o = types.SimpleNamespace(g=g, dbeta=sg, dgamma=sgx)
    o.dx = f.sc * (g - sg / M - f.xhat * sgx / M)
    o.dx_tol = BF16 * f.sc.abs() * (g.abs() + ag / M + f.xhat.abs() * agx / M)
    o.dbeta_tol = M * 2.0 ** -23 * ag
    dxhat = xh2.abs() * ((3.5 * f.kappa + 5) * U) + f.rstd * 2 * U * f.mean.abs()
    o.dgamma_tol = M * 2.0 ** -23 * agx + (g2.abs() * dxhat).sum(0)
    return o


def bn_fp32_emulation(x, gamma, beta, res, relu, eps=EPS):
    """The kernel's own formula, E[x^2] - mean^2 included, in torch fp32 (inputs float64 holding bf16 / fp32 values):
    (y as bf16, y before the bf16 rounding)."""
    C = x.shape[-1]
    xf = x.float().reshape(-1, C)
    M = torch.tensor(float(xf.shape[0]))
    mean = xf.sum(0) / M
    var = ((xf * xf).sum(0) / M - mean * mean).clamp(min=0)
    sc = gamma.float() * torch.rsqrt(var + torch.tensor(eps))
    sh = beta.float() - mean * sc
    y = (xf * sc + sh).reshape(x.shape)
    if res is not None:
        y = y + res.float()
    if relu:
        y = y.clamp(min=0)
    return y.to(BF), y


# =====================================================================================================================
# pooling
# =====================================================================================================================
POOL_KSP = [(3, 2, "SAME"), (3, 2, "VALID"), (2, 2, "VALID"), (3, 1, "SAME"), (1, 2, "VALID"), (5, 3, "VALID")]
POOL_NHW = [(2, 13, 14), (1, 8, 8)]
POOL_C = [64, 16, 3, 20]
POOL_CASES = [(nhw + (C,), k, s, pad) for (k, s, pad) in POOL_KSP for nhw in POOL_NHW for C in POOL_C]


def pool_id(case):
    shape, k, s, pad = case
    return "%dx%dx%dx%d-k%ds%d-%s" % (shape + (k, s, pad))


def pool_dispatch(g):
    """The dispatch predicates of csrc/kernels/pool.hip (fits32, k3pad01, k3s2_ok, k3s1_ok, valid53, POOL_GENERIC)."""
    fits32 = g.N * g.H * g.W * g.C < 2 ** 31 and g.N * g.P * g.Q * g.C < 2 ** 31

    def k3(stride):
        return (g.KH == 3 and g.KW == 3 and g.SH == stride and g.SW == stride and 0 <= g.PH <= 1 and 0 <= g.PW <= 1
                and g.C % 8 == 0 and fits32)
    valid53 = (g.KH == 5 and g.KW == 5 and g.SH == 3 and g.SW == 3 and g.PH == 0 and g.PW == 0
               and (g.P - 1) * 3 + 5 <= g.H and (g.Q - 1) * 3 + 5 <= g.W and g.C % 8 == 0 and fits32)
    generic = "V1-Idx64" if g.C % 8 else ("V8-Idx32" if fits32 else "V8-Idx64")
    d = dict(k3s2=k3(2), k3s1=k3(1), valid53=valid53, generic=generic)
    d["max_fwd"] = d["max_bwd"] = "k3s2" if d["k3s2"] and g.C // 8 <= 256 else generic
    d["avg_fwd"] = "k3s1" if d["k3s1"] else "valid53" if valid53 else generic
    d["avg_bwd"] = "k3s1" if d["k3s1"] else "valid53" if valid53 else generic
    d["avg_bwd_acc"] = None if (g.C % 8 or not fits32) else ("valid53" if valid53 else generic)
    return d


def _padded(g, t, fill):
    """t [N][H][W][C] padded with `fill` so that every window of every output pixel is in range."""
    hp = max((g.P - 1) * g.SH + g.KH, g.PH + g.H)
    wp = max((g.Q - 1) * g.SW + g.KW, g.PW + g.W)
    out = torch.full((g.N, hp, wp, g.C), fill, dtype=t.dtype)
    out[:, g.PH:g.PH + g.H, g.PW:g.PW + g.W] = t
    return out


def _tap(g, tp, r, s):
    """The view of padded tp that tap (r, s) of every window reads: [N][P][Q][C]."""
    return tp[:, r:r + (g.P - 1) * g.SH + 1:g.SH, s:s + (g.Q - 1) * g.SW + 1:g.SW]


def _unpad(g, tp):
    return tp[:, g.PH:g.PH + g.H, g.PW:g.PW + g.W].contiguous()


def pool_counts(g):
    """In-bounds taps per output pixel [P][Q] (the TF SAME divisor)."""
    ones = _padded(g, torch.ones((g.N, g.H, g.W, g.C), dtype=F64), 0.0)
    return sum(_tap(g, ones, r, s) for r in range(g.KH) for s in range(g.KW))[0, :, :, 0]


def max_pool64(x, k, s, pad):
    """(y, argmax, ties): padding acts as -inf; argmax is the FIRST maximum in (kh, kw) scan order (strict >), as
    TF's MaxPoolGrad and the kernels' uint8 argmax; ties = number of windows whose maximum occurs more than once."""
    g = pool_geom(tuple(x.shape), k, s, pad)
    xp = _padded(g, x, float("-inf"))
    best = torch.full((g.N, g.P, g.Q, g.C), float("-inf"), dtype=x.dtype)
    arg = torch.zeros((g.N, g.P, g.Q, g.C), dtype=torch.long)
    hits = torch.zeros_like(arg)
    for r in range(g.KH):
        for c in range(g.KW):
            v = _tap(g, xp, r, c)
            gt = v > best
            hits = torch.where(gt, torch.ones_like(hits), hits + (v == best).long())
            arg = torch.where(gt, torch.full_like(arg, r * g.KW + c), arg)
            best = torch.where(gt, v, best)
    return best, arg, int((hits > 1).sum())


def max_pool_bwd64(x, dy, k, s, pad):
    """The whole of each window's dy goes to its first maximum."""
    g = pool_geom(tuple(x.shape), k, s, pad)
    _, arg, _ = max_pool64(x, k, s, pad)
    dxp = _padded(g, torch.zeros_like(x), 0.0)
    for r in range(g.KH):
        for c in range(g.KW):
            _tap(g, dxp, r, c).add_(dy * (arg == r * g.KW + c))
    return _unpad(g, dxp)


def avg_pool64(x, k, s, pad, count_pad):
    """(y, tol): tol = one bf16 rounding + the fp32 accumulation and the multiplication by fl(1 / count):
    2^-8 |y64| + 2^-22 sum_window|x| / count (<= 25 additions of small integers are exact; 2^-22 = 4 u covers the
    reciprocal, the product and any rounding a non-integer input would add)."""
    g = pool_geom(tuple(x.shape), k, s, pad)
    xp = _padded(g, x, 0.0)
    taps = [_tap(g, xp, r, c) for r in range(g.KH) for c in range(g.KW)]
    div = torch.full((g.P, g.Q), float(g.KH * g.KW), dtype=F64) if count_pad else pool_counts(g)
    div = div[None, :, :, None]
    y = sum(taps) / div
    return y, BF16 * y.abs() + 2.0 ** -22 * sum(t.abs() for t in taps) / div


def avg_pool_bwd64(shape, dy, k, s, pad, count_pad, main=None):
    """(dx, tol) of the avg-pool input gradient; main: the accumulating backward's dx += (one rounding of the total;
    the fp32 addition of main rounds relative to the total, inside the 2^-22 term)."""
    g = pool_geom(tuple(shape), k, s, pad)
    div = torch.full((g.P, g.Q), float(g.KH * g.KW), dtype=F64) if count_pad else pool_counts(g)
    q = dy / div[None, :, :, None]
    dxp, axp = _padded(g, torch.zeros(shape, dtype=F64), 0.0), _padded(g, torch.zeros(shape, dtype=F64), 0.0)
    for r in range(g.KH):
        for c in range(g.KW):
            _tap(g, dxp, r, c).add_(q)
            _tap(g, axp, r, c).add_(q.abs())
    dx, adx = _unpad(g, dxp), _unpad(g, axp)
    if main is not None:
        dx, adx = dx + main, adx + main.abs()
    return dx, BF16 * dx.abs() + 2.0 ** -22 * adx


@functools.lru_cache(maxsize=None)
def _bf16_pool_values():
    """Every finite bf16 value in [-4, 4], once (-0 left out: it ties with +0)."""
    bits = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF).to(F64)
    keep = torch.isfinite(v) & (v.abs() <= 4) & ~((v == 0) & (bits != 0))
    v = v[keep]
    assert v.unique().numel() == v.numel()
    return v


@functools.lru_cache(maxsize=None)
def pool_input(shape, kind):
    """kind: 'unique' - every (n, c) plane drawn without replacement from the bf16 values in [-4, 4] (no window can
    tie); 'ties' - {-1, 0, 1}; 'negative' - -|randn| - 1 (bf16); 'int' - integers in [-3, 3]."""
    N, H, W, C = shape
    g = _gen(3, *shape, len(kind))
    if kind == "unique":
        vals = _bf16_pool_values()
        idx = torch.multinomial(torch.ones(N * C, vals.numel()), H * W, replacement=False, generator=g)
        return vals[idx].reshape(N, C, H, W).permute(0, 2, 3, 1).contiguous()
    if kind == "ties":
        return torch.randint(-1, 2, shape, generator=g).to(F64)
    if kind == "negative":
        return (-torch.randn(shape, generator=g).abs() - 1).to(BF).to(F64)
    if kind == "int":
        return torch.randint(-3, 4, shape, generator=g).to(F64)
    raise ValueError(kind)


def pool_dy(case, lo, hi, salt=0):
    """Integer dy in [lo, hi] for a pool case's output shape."""
    shape, k, s, pad = case
    g = pool_geom(shape, k, s, pad)
    return torch.randint(lo, hi + 1, (g.N, g.P, g.Q, g.C), generator=_gen(4, *shape, k, s, len(pad), salt)).to(F64)


# =====================================================================================================================
# LRN
# =====================================================================================================================
LRN_MODEL = (4, 1.0, 0.001 / 9, 0.75)   # the classic.py CIFAR-10 / AlexNet parameters: the normaliser is about 1
LRN_SHARP = [(2, 1.0, 1.0, 0.75), (5, 2.0, 0.5, 0.5)]  # the window term dominates
LRN_PARAMS = [LRN_MODEL] + LRN_SHARP
# (npix, C): C < 2r + 1 with 85 pixels per block; 4 pixels per block with a ragged last block; 2 per block on 192 of
# 256 lanes; C no divisor of anything; one pixel per block; C > 256 (strided loop); the limit C = 1024
LRN_SHAPES = [(7, 3), (37, 64), (10, 96), (9, 100), (5, 256), (3, 384), (2, 1024)]
LRN_4D = (2, 3, 5, 64)


def lrn_pixels_per_block(C):
    return 1 if C >= 256 else 256 // C


@functools.lru_cache(maxsize=None)
def lrn_input(shape):
    g = _gen(5, *shape)
    return torch.randn(shape, generator=g).to(BF).to(F64), torch.randn(shape, generator=g).to(BF).to(F64)


def _window(v, r_lo, r_hi, clamp_lo=True, clamp_hi=True):
    """sum_{-r_lo <= d <= r_hi} v[p][c + d] over [npix][C] rows; a clamp switched off lets the window run into the
    neighbouring pixel's channels (what a kernel without that clamp reads from its staged rows), zero outside."""
    npix, C = v.shape
    flat = v.reshape(-1)
    c = torch.arange(npix * C) % C
    i = torch.arange(npix * C)
    out = torch.zeros_like(flat)
    for d in range(-r_lo, r_hi + 1):
        j = i + d
        ok = (j >= 0) & (j < npix * C)
        if clamp_lo:
            ok &= c + d >= 0
        if clamp_hi:
            ok &= c + d < C
        out += torch.where(ok, flat[j.clamp(0, npix * C - 1)], torch.zeros_like(flat))
    return out.reshape(npix, C)


def lrn64(x, dy, r, bias, alpha, beta, r_lo=None, r_hi=None, clamp_lo=True, clamp_hi=True):
    """The formulas of csrc/kernels/lrn.hip in float64 over the last dimension, with the per-element bounds:
      s_c = bias + alpha sum_{|c'-c|<=r} x_c'^2;  y = x s^-beta;
      dx_i = dy_i s_i^-beta - 2 alpha beta x_i sum_{|j-i|<=r} dy_j y_j / s_j.
    Forward 2^-8 |y64|: the bf16 rounding reaches at most 2^-8 / (1 + 2^-8), which leaves 2^-16 |y64| for the fp32
    window sum and the fast-math __powf (a few ulp of fp32, 2^-21).  Backward: the same rounding of a sum of two
    terms, bounded through their magnitudes.  r_lo / r_hi / clamp_*: deliberately wrong variants for the CPU test."""
    shape = x.shape
    x2, dy2 = x.reshape(-1, shape[-1]), dy.reshape(-1, shape[-1])
    w = functools.partial(_window, r_lo=r if r_lo is None else r_lo, r_hi=r if r_hi is None else r_hi,
                          clamp_lo=clamp_lo, clamp_hi=clamp_hi)
    s = bias + alpha * w(x2 * x2)
    p = s ** -beta
    y = x2 * p
    dx = dy2 * p - 2 * alpha * beta * x2 * w(dy2 * y / s)
    dx_tol = BF16 * (dy2.abs() * p + 2 * alpha * beta * x2.abs() * w((dy2 * y).abs() / s))
    return types.SimpleNamespace(y=y.reshape(shape), y_tol=(BF16 * y.abs()).reshape(shape), dx=dx.reshape(shape),
                                 dx_tol=dx_tol.reshape(shape))
