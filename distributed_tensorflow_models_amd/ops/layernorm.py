"""Channel LayerNorm and layer scale + residual on rows of C channels (``csrc/kernels/layernorm.hip``).

``channel_layer_norm`` normalises every run of C contiguous channels of ``[..., C]`` on its own (one set of statistics
per NHWC pixel or ``[N, L, C]`` token: ConvNeXt's and a transformer block's LayerNorm; ``slim.layer_norm`` keeps
TF-contrib's per-sample meaning).  ``scale_residual`` is ``x + (row_scale[n] * gamma[c]) * r``: ConvNeXt's layer scale
and residual add, with stochastic depth's per-sample factor.

CUDA bf16 / fp32 tensors with ``C % 8 == 0``, ``8 <= C <= 2048`` and fewer than 2^31 rows run the kernels (hard error
if the library is missing, via ``_lib.lib()``); CPU tensors and every other shape run the same definition as a torch
composition.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib

# the automatic slab rule sizes grids for this part whatever device runs them: results keep their bits across machines
_RULE_CUS, _RULE_BLOCKS_PER_CU, _MIN_TRIPS, _MAX_RECORDS = 256, 4, 2, 4096


def eligible(M, C):
    return C % 8 == 0 and 8 <= C <= 2048 and 1 <= M < 2 ** 31


def lanes_per_row(C):
    """G: the smallest power of two for which a lane holds at most four 16-byte vectors of a row."""
    G = 1
    while -(-(C // 8) // G) > 4:
        G *= 2
    return G


def auto_slab_rows(M, C):
    """Rows per block from the shape alone: a few blocks per CU where the tensor allows it, no block below two trips
    of its 256 / G rows, whole trips."""
    rt = 256 // lanes_per_row(C)
    want = -(-M // (_RULE_CUS * _RULE_BLOCKS_PER_CU))
    return max(_MIN_TRIPS * rt, -(-want // rt) * rt)


def _slab(M, C, slab_rows):
    if slab_rows is None:
        return auto_slab_rows(M, C)
    return max(1, int(slab_rows), -(-M // _MAX_RECORDS))  # every record is read again by col_records_sum


def _param_ok(p, x, C):
    return p is None or (p.device == x.device and p.dtype == torch.float32 and tuple(p.shape) == (C,))


def _kernel_path(x, *params):
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and x.dim() >= 1 and x.numel() > 0):
        return False
    C = x.shape[-1]
    return eligible(x.numel() // C, C) and all(_param_ok(p, x, C) for p in params)


def _check(rc):
    if rc != 0:
        raise RuntimeError("layernorm kernel launch refused: code %d" % rc)


def _ws(L, M, C, slab, sets, device):
    return torch.empty(L.dtm_cln_ws_floats(M, C, slab, sets), device=device, dtype=torch.float32)


class _ChannelLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, slab):
        x = x.contiguous()
        gamma = None if gamma is None else gamma.contiguous()
        beta = None if beta is None else beta.contiguous()
        C = x.shape[-1]
        M = x.numel() // C
        y = torch.empty_like(x)
        stats = torch.empty((M, 2), device=x.device, dtype=torch.float32)
        _check(_lib.lib().dtm_cln_fwd(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(y), _lib.ptr(stats), M, C,
                                      slab, float(eps), int(x.dtype == torch.bfloat16), _lib.stream_ptr()))
        ctx.save_for_backward(x, gamma, stats)
        ctx.slab, ctx.has_beta = slab, beta is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, stats = ctx.saved_tensors
        C = x.shape[-1]
        M = x.numel() // C
        L = _lib.lib()
        dy = dy.contiguous().to(x.dtype)
        dx = torch.empty_like(x)
        f32 = dict(device=x.device, dtype=torch.float32)
        dgamma = torch.empty(C, **f32) if gamma is not None and ctx.needs_input_grad[1] else None
        dbeta = torch.empty(C, **f32) if ctx.has_beta and ctx.needs_input_grad[2] else None
        ws = _ws(L, M, C, ctx.slab, 2, x.device) if dgamma is not None or dbeta is not None else None
        _check(L.dtm_cln_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(gamma), _lib.ptr(stats), _lib.ptr(dx),
                             _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), 0 if ws is None else ws.numel(), M, C,
                             ctx.slab, int(x.dtype == torch.bfloat16), _lib.stream_ptr()))
        return dx, dgamma, dbeta, None, None


def channel_layer_norm_torch(x, gamma=None, beta=None, eps=1e-6):
    """The definition as torch ops: fp32 moments over the last dimension, affine, one rounding to x's type."""
    xf = x.float()
    mean = xf.mean(dim=-1, keepdim=True)
    var = xf.var(dim=-1, keepdim=True, unbiased=False)
    y = (xf - mean) * torch.rsqrt(var + eps)
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    return y.to(x.dtype)


def channel_layer_norm(x, gamma=None, beta=None, eps=1e-6, slab_rows=None):
    """y = (x - mean_r) * rsqrt(var_r + eps) * gamma + beta over every row r of ``x.shape[-1]`` channels; ``gamma`` /
    ``beta`` fp32 [C] or None.  ``slab_rows``: rows per block of the kernels' work split (None = ``auto_slab_rows``)."""
    if _kernel_path(x, gamma, beta):
        C = x.shape[-1]
        return _ChannelLayerNormFn.apply(x, gamma, beta, eps, _slab(x.numel() // C, C, slab_rows))
    return channel_layer_norm_torch(x, gamma, beta, eps)


class _ScaleResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, gamma, row_scale, slab):
        x, r, gamma = x.contiguous(), r.contiguous(), gamma.contiguous()
        s = None if row_scale is None else row_scale.contiguous()
        C = x.shape[-1]
        M = x.numel() // C
        ns = 0 if s is None else s.numel()
        y = torch.empty_like(x)
        _check(_lib.lib().dtm_scale_residual_fwd(_lib.ptr(x), _lib.ptr(r), _lib.ptr(gamma), _lib.ptr(s), _lib.ptr(y),
                                                 M, C, ns, M // max(ns, 1), slab, int(x.dtype == torch.bfloat16),
                                                 _lib.stream_ptr()))
        ctx.save_for_backward(r, gamma, s)
        ctx.slab = slab
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        r, gamma, s = ctx.saved_tensors
        C = r.shape[-1]
        M = r.numel() // C
        ns = 0 if s is None else s.numel()
        L = _lib.lib()
        dy = dy.contiguous().to(r.dtype)
        dr = dgamma = ws = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dr = torch.empty_like(r)
            if ctx.needs_input_grad[2]:
                dgamma = torch.empty(C, device=r.device, dtype=torch.float32)
                ws = _ws(L, M, C, ctx.slab, 1, r.device)
            _check(L.dtm_scale_residual_bwd(_lib.ptr(dy), _lib.ptr(r), _lib.ptr(gamma), _lib.ptr(s), _lib.ptr(dr),
                                            _lib.ptr(dgamma), _lib.ptr(ws), 0 if ws is None else ws.numel(), M, C, ns,
                                            M // max(ns, 1), ctx.slab, int(r.dtype == torch.bfloat16),
                                            _lib.stream_ptr()))
        return dy, dr, dgamma, None, None


def scale_residual_torch(x, r, gamma, row_scale=None):
    """The definition as torch ops: fp32, one rounding to x's type; row_scale [N] scales the samples of ``r``."""
    g = gamma.float()
    if row_scale is not None:
        g = row_scale.float().reshape((-1,) + (1,) * (x.dim() - 1)) * g
    return (x.float() + g * r.float()).to(x.dtype)


def scale_residual(x, r, gamma, row_scale=None, slab_rows=None):
    """y = x + (row_scale[n] * gamma[c]) * r on ``[N, ..., C]`` tensors of one shape and type; ``gamma`` fp32 [C],
    ``row_scale`` fp32 [N] or None (stochastic depth: 0 or 1 / (1 - p) per sample)."""
    if x.shape != r.shape or x.dtype != r.dtype:
        raise ValueError("scale_residual: x %s %s and r %s %s differ" % (tuple(x.shape), x.dtype, tuple(r.shape),
                                                                      r.dtype))
    if row_scale is not None and tuple(row_scale.shape) != (x.shape[0],):
        raise ValueError("scale_residual: row_scale %s for %d samples" % (tuple(row_scale.shape), x.shape[0]))
    s_ok = row_scale is None or (row_scale.device == x.device and row_scale.dtype == torch.float32)
    if gamma is not None and r.device == x.device and s_ok and _kernel_path(x, gamma):
        C = x.shape[-1]
        return _ScaleResidualFn.apply(x, r, gamma, row_scale, _slab(x.numel() // C, C, slab_rows))
    return scale_residual_torch(x, r, gamma, row_scale)
