"""Squeeze-and-excitation on NHWC (``csrc/kernels/se.hip``): a per-sample channel gate from the global average through
a two-layer MLP and a sigmoid, applied to ``x`` with an optional residual add and ReLU in the same pass.

CUDA bf16 tensors of an eligible shape (``C % 8 == 0``, ``8 <= C <= 4096``, ``1 <= Cr <= 256``, fp32 parameters on
``x``'s device) run the slab-split kernels (hard error if the library is missing, via ``_lib.lib()``); CPU tensors and
everything else run the same definition as a torch composition.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .groupnorm import _MAX_SLABS, auto_slab_pixels
from .nn import _accum_param_grad

C_MAX, CR_MAX = 4096, 256
GATE_GROUP = 4  # samples per block of the gate kernels (SE_G in se.hip)


def eligible(C, Cr):
    return C % 8 == 0 and 8 <= C <= C_MAX and 1 <= Cr <= CR_MAX


def _fc(w, rows, cols):
    """The [rows, cols] matrix of an FC master stored as it is or as a 1x1 conv [rows, 1, 1, cols]."""
    if tuple(w.shape) not in ((rows, cols), (rows, 1, 1, cols)):
        raise ValueError("squeeze_excite: weights of shape %r where [%d, %d] or [%d, 1, 1, %d] is needed"
                         % (tuple(w.shape), rows, cols, rows, cols))
    return w.reshape(rows, cols)


def _kernel_path(x, residual, params):
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.numel() > 0 and x.shape[0] <= 65535):
        return False
    if residual is not None and not (residual.is_cuda and residual.dtype == torch.bfloat16
                                     and residual.shape == x.shape):
        return False
    return eligible(x.shape[-1], params[0].shape[0]) and all(
        p.device == x.device and p.dtype == torch.float32 for p in params)


def _check(rc):
    if rc != 0:
        raise RuntimeError("squeeze-excite kernel launch refused: code %d" % rc)


class _SqueezeExciteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, w1, b1, w2, b2, relu, slab_pixels):
        x = x.contiguous()
        res = None if residual is None else residual.contiguous()
        N, H, W, C = x.shape
        Cr = w1.shape[0]
        w1m, w2m = w1.detach().reshape(Cr, C).contiguous(), w2.detach().reshape(C, Cr).contiguous()
        L, f32 = _lib.lib(), dict(device=x.device, dtype=torch.float32)
        y = torch.empty_like(x)
        s, z, g = torch.empty((N, C), **f32), torch.empty((N, Cr), **f32), torch.empty((N, C), **f32)
        ws = torch.empty(L.dtm_se_ws_floats(N, H * W, C, Cr, slab_pixels, 0), **f32)
        _check(L.dtm_se_fwd(_lib.ptr(x), _lib.ptr(res), _lib.ptr(w1m), _lib.ptr(b1.detach().contiguous()),
                            _lib.ptr(w2m), _lib.ptr(b2.detach().contiguous()), _lib.ptr(y), _lib.ptr(s), _lib.ptr(z),
                            _lib.ptr(g), _lib.ptr(ws), ws.numel(), N, H * W, C, Cr, slab_pixels, int(relu),
                            _lib.stream_ptr()))
        ctx.save_for_backward(x, y if relu else None, w1, b1, w2, b2, s, z, g)
        ctx.cfg = (relu, slab_pixels, residual is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, y, w1, b1, w2, b2, s, z, g = ctx.saved_tensors
        relu, slab_pixels, has_res = ctx.cfg
        N, H, W, C = x.shape
        Cr = w1.shape[0]
        L, f32 = _lib.lib(), dict(device=x.device, dtype=torch.float32)
        dy = dy.contiguous().to(x.dtype)
        dx = torch.empty_like(x)
        want_res = has_res and ctx.needs_input_grad[1]
        dres = torch.empty_like(x) if want_res and relu else None  # without ReLU dresidual is dy itself
        params = (w1, b1, w2, b2)
        grads = [torch.empty(p.shape, **f32) for p in params] if any(ctx.needs_input_grad[2:6]) else [None] * 4
        ws = torch.empty(L.dtm_se_ws_floats(N, H * W, C, Cr, slab_pixels, 1), **f32)
        _check(L.dtm_se_bwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(dy), _lib.ptr(w1.detach().reshape(Cr, C).contiguous()),
                            _lib.ptr(w2.detach().reshape(C, Cr).contiguous()), _lib.ptr(s), _lib.ptr(z), _lib.ptr(g),
                            _lib.ptr(dx), _lib.ptr(dres), *(_lib.ptr(t) for t in grads), _lib.ptr(ws), ws.numel(), N,
                            H * W, C, Cr, slab_pixels, int(relu), _lib.stream_ptr()))
        out = [_accum_param_grad(p, t) if t is not None and need else None
               for p, t, need in zip(params, grads, ctx.needs_input_grad[2:6])]
        return (dx, (dres if relu else dy) if want_res else None, *out, None, None)


def squeeze_excite_torch(x, w1, b1, w2, b2, residual=None, relu=False):
    """The definition as torch ops: fp32 mean, two FCs, sigmoid, gate, residual, ReLU, one rounding to x's type."""
    N, C = x.shape[0], x.shape[-1]
    Cr = w1.shape[0]
    cd = torch.float64 if x.dtype == torch.float64 else torch.float32
    xf = x.to(cd)
    s = xf.reshape(N, -1, C).mean(dim=1)
    z = torch.relu(s @ _fc(w1, Cr, C).to(cd).t() + b1.to(cd))
    g = torch.sigmoid(z @ _fc(w2, C, Cr).to(cd).t() + b2.to(cd))
    y = xf * g.reshape(N, 1, 1, C)
    if residual is not None:
        y = y + residual.to(cd)
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


def squeeze_excite(x, w1, b1, w2, b2, residual=None, relu=False, slab_pixels=None):
    """y = act(x * sigmoid(w2 relu(w1 mean_hw(x) + b1) + b2) + residual) on NHWC ``x``.  ``w1`` [Cr, C] or
    [Cr, 1, 1, C], ``w2`` [C, Cr] or [C, 1, 1, Cr], fp32 masters.  ``slab_pixels``: pixels per block of the kernels'
    work split (None = ``groupnorm.auto_slab_pixels``); it is raised where it would cut a sample into more than 128
    slabs, since the gate kernel merges a sample's slab records serially."""
    C, Cr = x.shape[-1], w1.shape[0]
    _fc(w1, Cr, C), _fc(w2, C, Cr)
    if tuple(b1.shape) != (Cr,) or tuple(b2.shape) != (C,):
        raise ValueError("squeeze_excite: biases of shape %r, %r where [%d], [%d] are needed"
                         % (tuple(b1.shape), tuple(b2.shape), Cr, C))
    if residual is not None and residual.shape != x.shape:
        raise ValueError("squeeze_excite: residual of shape %r against x of shape %r"
                         % (tuple(residual.shape), tuple(x.shape)))
    if _kernel_path(x, residual, (w1, b1, w2, b2)):
        N, H, W, _ = x.shape
        if slab_pixels is None:
            sp = auto_slab_pixels(N, H * W, C)
        else:
            sp = max(1, int(slab_pixels), -(-H * W // _MAX_SLABS))
        return _SqueezeExciteFn.apply(x, residual, w1, b1, w2, b2, relu, sp)
    return squeeze_excite_torch(x, w1, b1, w2, b2, residual, relu)
