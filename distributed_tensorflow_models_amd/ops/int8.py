"""8-bit integer inference for fake-quantised models (csrc/kernels/int8.hip): the arithmetic a ``--quantize``
checkpoint describes, run on integer codes.  ``compat.quantize.QuantConfig(integer=True)`` routes the slim layers here.

One integer layer, for activation codes ``a`` (uint8 NHWC, record ``rec_a``), weight codes ``w`` (record ``rec_w``,
TF's narrow range), a per-channel fp32 ``bias`` and an output record ``rec_o``::

    acc  = sum over the in-bounds taps (r, s) and c of (a - z_a) * (w - z_w)         int32, exact; padding adds 0
    t    = s_a * s_w                                                                  fp32
    r    = act(fma(float(acc), t, bias[k]))                                           one rounding; none / relu / relu6
    code = clamp(rint(r * inv_o) + z_o, 0, 255)                                       the arithmetic of fakequant apply

and on request the dequantised ``(code - z_o) * s_o`` in bf16 or fp32 -- the bits ``fakequant.apply`` gives ``r``.
``R * S * C`` is at most 32768, so int32 cannot overflow.  Records are the int32[8] tensors of ``ops.fakequant``.

On a CPU tensor the definitions run as torch integer ops (the fallback and the tests' oracle); on the GPU a missing
kernel library is an error.  ``layers_run()`` counts the integer layers executed (tests, the evaluator's result line).
"""
import ctypes

import torch

from . import _lib
from .geometry import conv_geom

MAX_REDUCE = 32768
_DTYPES = {torch.float32: 0, torch.bfloat16: 1}
_DEQ = {None: 0, torch.bfloat16: 1, torch.float32: 2}
_ACTS = {None: 0, "none": 0, "relu": 1, "relu6": 2}
_layers = [0]


def layers_run():
    """Integer layers (``conv2d_q8`` / ``depthwise_q8`` calls) executed since the last ``reset_layers``."""
    return _layers[0]


def reset_layers():
    _layers[0] = 0


class Q8Desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("N", "H", "W", "C", "K", "R", "S", "P", "Q", "stride", "pad_h", "pad_w")]


class Q8Dw(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("N", "H", "W", "C", "Cp", "R", "S", "P", "Q", "stride", "pad_h", "pad_w")]


class Q8Weights:
    """Weight codes of one layer: ``codes`` uint8 [K,R,S,C] (depthwise: [R,S,C]) and their record; on the GPU the
    kernels' form instead -- ``w8`` int8 [rows, row bytes] of ``code - 128`` and ``wsum`` int32 [rows]."""

    def __init__(self, shape, rec, depthwise, codes=None, w8=None, wsum=None):
        self.shape, self.rec, self.depthwise = tuple(shape), rec, depthwise
        self.codes, self.w8, self.wsum = codes, w8, wsum


def _rc(name, rc):
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (name, rc))


def _codes_cpu(x, rec):
    f = rec.view(torch.float32)
    return torch.clamp(torch.round(x.float() * f[1]) + f[2], f[3], f[4]).to(torch.uint8)


def quantize_u8(x, rec):
    """bf16 / fp32 ``x`` -> uint8 codes ``clamp(rint(x * inv_scale) + zp, qmin, qmax)`` of the record ``rec``."""
    if x.dtype not in _DTYPES:
        raise TypeError("int8: fp32 or bf16 expected, got %s" % x.dtype)
    if not x.is_cuda:
        return _codes_cpu(x, rec)
    if not x.is_contiguous():
        x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel():
        _rc("dtm_q8_quantize", _lib.lib().dtm_q8_quantize(_lib.ptr(x), _DTYPES[x.dtype], _lib.ptr(y), x.numel(),
                                                          _lib.ptr(rec), _lib.stream_ptr()))
    return y


def quantize_u8_into(x, y, rec):
    """``quantize_u8`` into the contiguous uint8 tensor ``y`` (x, y starting at any element)."""
    if not x.is_cuda:
        return y.copy_(_codes_cpu(x, rec))
    _rc("dtm_q8_quantize", _lib.lib().dtm_q8_quantize(_lib.ptr(x), _DTYPES[x.dtype], _lib.ptr(y), x.numel(),
                                                      _lib.ptr(rec), _lib.stream_ptr()))
    return y


def _deq_cpu(codes, rec, dtype):
    f = rec.view(torch.float32)
    return ((codes.float() - f[2]) * f[0]).to(dtype)


def dequantize_u8(codes, rec, dtype=torch.float32, out=None):
    """uint8 codes -> ``(code - zp) * scale`` in bf16 or fp32 (``out``: a contiguous tensor to fill)."""
    y = out if out is not None else torch.empty(codes.shape, dtype=dtype, device=codes.device)
    if not codes.is_cuda:
        return y.copy_(_deq_cpu(codes, rec, y.dtype))
    if not codes.is_contiguous():
        codes = codes.contiguous()
    if codes.numel():
        _rc("dtm_q8_dequantize", _lib.lib().dtm_q8_dequantize(_lib.ptr(codes), _lib.ptr(y), _DTYPES[y.dtype],
                                                              codes.numel(), _lib.ptr(rec), _lib.stream_ptr()))
    return y


def cached(param, build):
    """``build()`` once per weights version, kept on ``param`` (``ops.nn.WEIGHT_VERSION``: the optimizer's update and
    ``invalidate_weight_copies`` retire it)."""
    from .nn import WEIGHT_VERSION
    c = getattr(param, "_q8w", None)
    if c is not None and c[0] == WEIGHT_VERSION[0]:
        return c[1]
    val = build()
    try:
        param._q8w = (WEIGHT_VERSION[0], val)
    except Exception:
        pass
    return val


def prepare_weights(w, rec_w, depthwise=False):
    """Folded fp32 weights ``w`` ([K,R,S,C]; depthwise [R,S,C] or TF's [R,S,C,1]) -> ``Q8Weights`` through the weight
    record.  A ``torch.nn.Parameter`` is prepared once per weights version."""
    if isinstance(w, torch.nn.Parameter):
        return cached(w, lambda: prepare_weights(w.detach(), rec_w, depthwise))
    if depthwise and w.dim() == 4:
        if w.shape[3] != 1:
            raise ValueError("int8: depthwise multiplier 1 only")
        w = w[..., 0]
    if w.dim() != (3 if depthwise else 4):
        raise ValueError("int8: weights of shape %s" % (tuple(w.shape),))
    K, (R, S, C) = (1 if depthwise else w.shape[0]), w.shape[-3:]
    w = w.detach().float().contiguous()
    if not w.is_cuda:
        if R * S * C > MAX_REDUCE:  # (on the GPU the entry points refuse it with -2)
            raise ValueError("int8: R*S*C = %d above %d" % (R * S * C, MAX_REDUCE))
        return Q8Weights(w.shape, rec_w, depthwise, codes=_codes_cpu(w, rec_w))
    L = _lib.lib()
    rows, rb = L.dtm_q8_weight_rows(K), L.dtm_q8_weight_row_bytes(R, S, C)
    w8 = torch.empty((rows, rb), dtype=torch.int8, device=w.device)
    wsum = torch.empty(rows, dtype=torch.int32, device=w.device)
    _rc("dtm_q8_prepare_weights", L.dtm_q8_prepare_weights(_lib.ptr(w), _lib.ptr(rec_w), _lib.ptr(w8), _lib.ptr(wsum),
                                                           K, R, S, C, _lib.stream_ptr()))
    return Q8Weights(w.shape, rec_w, depthwise, w8=w8, wsum=wsum)


# ---- the definition in torch integer ops (CPU) -----------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma(a, b, c) with ONE rounding: the product is exact in fp64; the fp64 sum is rounded to odd (TwoSum gives
    its error), after which the rounding to fp32 is the rounding of the exact value."""
    p = a.double() * b.double()
    c = c.double()
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    odd = (s.view(torch.int64) & 1) == 1
    toward = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    return torch.where((e != 0) & ~odd, torch.nextafter(s, toward), s).float()


def _requant_cpu(acc, rec_a, rec_w, bias, act, rec_o, out_dtype):
    fa, fw, fo = (r.view(torch.float32) for r in (rec_a, rec_w, rec_o))
    r = _fma(acc.to(torch.float32), fa[0] * fw[0], bias.float())
    if act >= 1:
        r = torch.clamp(r, min=0.0)
    if act == 2:
        r = torch.clamp(r, max=6.0)
    q = torch.clamp(torch.round(r * fo[1]) + fo[2], 0.0, 255.0)
    codes = q.to(torch.uint8)
    if out_dtype is None:
        return codes
    return codes, ((q - fo[2]) * fo[0]).to(out_dtype)


def _windows(a, rec_a, g):
    """(a - z_a) as int64 windows [N,P,Q,C,R,S]; padding taps are 0."""
    za = int(rec_a.view(torch.float32)[2])
    x = a.to(torch.int64) - za
    x = torch.nn.functional.pad(x, (0, 0, g.pad_w, max(g.pad_r, 0) + g.stride, g.pad_h, max(g.pad_b, 0) + g.stride))
    x = x.unfold(1, g.R, g.stride).unfold(2, g.S, g.stride)
    return x[:, :g.P, :g.Q]


def _check(a, qw, bias, act, out_dtype, depthwise):
    if a.dtype != torch.uint8 or a.dim() != 4:
        raise TypeError("int8: uint8 NHWC activation codes expected")
    if qw.depthwise != depthwise:
        raise ValueError("int8: weights prepared for the other layer kind")
    if act not in _ACTS or out_dtype not in _DEQ:
        raise ValueError("int8: act none / relu / relu6, out_dtype None / bf16 / fp32")
    K = a.shape[-1] if depthwise else qw.shape[0]
    if bias.numel() != K or a.shape[-1] != qw.shape[-1]:
        raise ValueError("int8: bias or channel count does not match the weights")
    return _ACTS[act]


def _pad16(a):
    """Channels padded to a multiple of 16 (with code 0: the prepared weights hold z_w there, so they add 0)."""
    C = a.shape[-1]
    return a if C % 16 == 0 else torch.nn.functional.pad(a, (0, -C % 16))


def _outputs(a, shape, out_dtype):
    codes = torch.empty(shape, dtype=torch.uint8, device=a.device)
    deq = torch.empty(shape, dtype=out_dtype, device=a.device) if out_dtype is not None else None
    return codes, deq


def conv2d_q8(a, rec_a, qw, bias, rec_o, stride=1, padding="SAME", act=None, out_dtype=None):
    """One integer conv layer.  ``a``: uint8 [N,H,W,C]; ``qw``: ``prepare_weights`` of [K,R,S,C]; ``bias``: fp32 [K].
    Returns the uint8 codes [N,P,Q,K], or ``(codes, dequantised)`` with ``out_dtype`` bf16 / fp32."""
    iact = _check(a, qw, bias, act, out_dtype, False)
    K, R, S, C = qw.shape
    g = conv_geom(tuple(a.shape), (K, R, S, C), stride, padding)
    _layers[0] += 1
    if not a.is_cuda:
        acc = torch.einsum("npqcrs,krsc->npqk", _windows(a, rec_a, g),
                           qw.codes.to(torch.int64) - int(qw.rec.view(torch.float32)[2]))
        return _requant_cpu(acc, rec_a, qw.rec, bias, iact, rec_o, out_dtype)
    ap = _pad16(a.contiguous())
    codes, deq = _outputs(a, (g.N, g.P, g.Q, K), out_dtype)
    d = Q8Desc(g.N, g.H, g.W, ap.shape[-1], K, R, S, g.P, g.Q, g.stride, g.pad_h, g.pad_w)
    _rc("dtm_q8_conv", _lib.lib().dtm_q8_conv(
        _lib.ptr(ap), _lib.ptr(qw.w8), _lib.ptr(qw.wsum), _lib.ptr(bias.float().contiguous()), _lib.ptr(rec_a),
        _lib.ptr(qw.rec), _lib.ptr(rec_o), _lib.ptr(codes), _lib.ptr(deq), _DEQ[out_dtype], iact, ctypes.byref(d),
        _lib.stream_ptr()))
    return codes if deq is None else (codes, deq)


def depthwise_q8(a, rec_a, qw, bias, rec_o, stride=1, padding="SAME", act=None, out_dtype=None):
    """One integer depthwise layer (multiplier 1, stride 1 or 2).  ``qw``: ``prepare_weights(..., depthwise=True)`` of
    [R,S,C]; ``bias``: fp32 [C].  Returns like ``conv2d_q8``, [N,P,Q,C]."""
    iact = _check(a, qw, bias, act, out_dtype, True)
    R, S, C = qw.shape
    g = conv_geom(tuple(a.shape), (C, R, S, C), stride, padding)
    if g.stride not in (1, 2):
        raise ValueError("int8: depthwise stride 1 or 2")
    _layers[0] += 1
    if not a.is_cuda:
        wz = qw.codes.to(torch.int64) - int(qw.rec.view(torch.float32)[2])
        acc = (_windows(a, rec_a, g) * wz.permute(2, 0, 1)).sum((-1, -2))
        return _requant_cpu(acc, rec_a, qw.rec, bias, iact, rec_o, out_dtype)
    ap = _pad16(a.contiguous())
    codes, deq = _outputs(a, (g.N, g.P, g.Q, C), out_dtype)
    d = Q8Dw(g.N, g.H, g.W, C, ap.shape[-1], R, S, g.P, g.Q, g.stride, g.pad_h, g.pad_w)
    _rc("dtm_q8_depthwise", _lib.lib().dtm_q8_depthwise(
        _lib.ptr(ap), _lib.ptr(qw.w8), _lib.ptr(bias.float().contiguous()), _lib.ptr(rec_a), _lib.ptr(qw.rec),
        _lib.ptr(rec_o), _lib.ptr(codes), _lib.ptr(deq), _DEQ[out_dtype], iact, ctypes.byref(d), _lib.stream_ptr()))
    return codes if deq is None else (codes, deq)
