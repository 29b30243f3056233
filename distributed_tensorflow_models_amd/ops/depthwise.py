"""Depthwise conv (TF ``depthwise_conv2d`` / slim.separable_conv2d(num_outputs=None)); HIP on GPU.

Two kernel families: ``legacy`` (csrc/kernels/depthwise.hip: the 8-channel vector kernels where 256 % (C/8) == 0, scalar
kernels elsewhere) and ``tile`` (csrc/kernels/depthwise_tile.hip: LDS-tiled, any C % 8 == 0 at multiplier 1).  ``impl``
/ the environment variable ``DTM_DW_IMPL`` picks one; ``auto`` takes the tile where the legacy dispatch would run its
scalar kernels.
"""
import ctypes
import os

import torch

from . import _lib
from . import reference as ref
from .geometry import conv_geom
from .lazy import as_tensor
from .nn import _accum_param_grad


class DwArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("N", "H", "W", "C", "M", "R", "S", "P", "Q", "stride", "ph", "pw", "dil")]


IMPLS = ("auto", "tile", "legacy")


def fast8(a):
    """The legacy dispatch runs its 8-channel vector kernels (dw_*8) for this geometry."""
    return a.M == 1 and a.C % 8 == 0 and a.C // 8 <= 256 and 256 % (a.C // 8) == 0


def tile_eligible(a):
    """The tiled kernels serve this geometry (tile_ok in depthwise_tile.hip)."""
    return (a.M == 1 and a.C >= 8 and a.C % 8 == 0 and 1 <= a.R <= 7 and 1 <= a.S <= 7 and a.stride in (1, 2)
            and a.dil == 1 and 1 <= a.N <= 65535 and min(a.H, a.W, a.P, a.Q) >= 1 and a.ph >= 0 and a.pw >= 0)


def resolve_impl(a, impl=None):
    """``impl`` (None: $DTM_DW_IMPL, default "auto") -> the family this call runs, "tile" or "legacy"."""
    if impl is None:
        impl = os.environ.get("DTM_DW_IMPL") or "auto"
    if impl not in IMPLS:
        raise ValueError("depthwise impl %r: one of %s" % (impl, ", ".join(IMPLS)))
    if impl == "tile" and not tile_eligible(a):
        raise ValueError("depthwise impl 'tile' needs multiplier 1, C %% 8 == 0, R, S <= 7, stride 1 or 2 and rate 1; "
                         "got C=%d M=%d %dx%d stride %d rate %d" % (a.C, a.M, a.R, a.S, a.stride, a.dil))
    if impl == "auto":
        return "tile" if tile_eligible(a) and not fast8(a) else "legacy"
    return impl


def _entry(L, tile, name):
    fn = getattr(L, "dtm_depthwise_" + ("tile_" if tile else "") + name)

    def call(*args):
        rc = fn(*args)
        if rc:
            raise RuntimeError("%s failed: %d" % (fn.__name__, rc))
    return call


class _DepthwiseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, a, tile):
        L = _lib.lib()
        x = x.contiguous()
        wf = w.detach().float().contiguous()
        y = torch.empty((a.N, a.P, a.Q, a.C * a.M), device=x.device, dtype=torch.bfloat16)
        _entry(L, tile, "fwd")(_lib.ptr(x), _lib.ptr(wf), _lib.ptr(y), ctypes.byref(a), _lib.stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.a, ctx.tile = a, tile
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _lib.lib()
        x, w = ctx.saved_tensors
        a = ctx.a
        dy = dy.contiguous()
        s = _lib.stream_ptr()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _entry(L, ctx.tile, "dgrad")(_lib.ptr(dy), _lib.ptr(w.detach().float().contiguous()), _lib.ptr(dx),
                                         ctypes.byref(a), s)
        dw = None
        if ctx.needs_input_grad[1]:
            g = torch.zeros(w.shape, device=x.device, dtype=torch.float32)
            _entry(L, ctx.tile, "wgrad")(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(g), ctypes.byref(a), s)
            dw = _accum_param_grad(w, g)
        return dx, dw, None, None


def depthwise_conv2d(x, w, stride=1, padding="SAME", rate=1, impl=None):
    """x [N,H,W,C]; w [R,S,C,M] (TF layout, fp32 master) -> [N,P,Q,C*M].  impl: "auto" | "tile" | "legacy"; None
    reads $DTM_DW_IMPL at each call (default "auto").  Forward and backward of one call run the same family."""
    x = as_tensor(x)
    R, S, C, M = w.shape
    g = conv_geom(tuple(x.shape), (C, R, S, C), stride, padding, rate)
    a = DwArgs(g.N, g.H, g.W, g.C, M, R, S, g.P, g.Q, g.stride, g.pad_h, g.pad_w, rate)
    family = resolve_impl(a, impl)
    if not x.is_cuda:
        return ref.depthwise_conv2d(x, w, stride, padding, rate)
    return _DepthwiseFn.apply(x.to(torch.bfloat16), w, a, family == "tile")
