"""Grouped 3x3 convolution (ResNeXt's bottleneck conv): equal input and output width C, ``groups`` groups of
D = C / groups channels, group g owning channels [gD, (g+1)D) of both.  HIP on the GPU (csrc/kernels/groupconv.hip:
MFMA kernels over block-diagonal weight fragments built in registers from the fp32 master), the composed reference
on CPU tensors.  Served: D in {4, 8, 16, 32}, C % 16 == 0, 3x3 taps, stride 1 or 2, rate 1, top / left pad 0 or 1;
anything else is a ValueError - there is no other grouped path.
"""
import ctypes

import torch

from . import _lib
from . import nn
from . import reference as ref
from .geometry import conv_geom
from .lazy import as_tensor
from .nn import _accum_param_grad


class GcArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("N", "H", "W", "C", "D", "P", "Q", "stride", "ph", "pw")]


DEPTHS = (4, 8, 16, 32)


def eligible(a):
    """The kernels serve this geometry (gc_ok in groupconv.hip)."""
    return (a.D in DEPTHS and a.C >= 16 and a.C % 16 == 0 and a.C % a.D == 0 and a.stride in (1, 2)
            and 1 <= a.N <= 65535 and min(a.H, a.W, a.P, a.Q) >= 1 and a.ph in (0, 1) and a.pw in (0, 1)
            and a.C * 9 * a.D < 2 ** 31 - 1)


def _entry(name):
    fn = getattr(_lib.lib(), "dtm_groupconv_" + name)

    def call(*args):
        nn._check(fn(*args), fn.__name__)
    return call


class _GroupConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, a):
        x = x.contiguous()
        wf = w.detach().float().contiguous()
        y = torch.empty((a.N, a.P, a.Q, a.C), device=x.device, dtype=torch.bfloat16)
        _entry("fwd")(_lib.ptr(x), _lib.ptr(wf), _lib.ptr(y), ctypes.byref(a), _lib.stream_ptr())
        ctx.save_for_backward(x, w)
        ctx.a = a
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        a = ctx.a
        dy = dy.contiguous()
        s = _lib.stream_ptr()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)  # the kernel writes every pixel
            _entry("dgrad")(_lib.ptr(dy), _lib.ptr(w.detach().float().contiguous()), _lib.ptr(dx), ctypes.byref(a), s)
        dw = None
        if ctx.needs_input_grad[1]:
            g = torch.zeros(w.shape, device=x.device, dtype=torch.float32)
            _entry("wgrad")(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(g), ctypes.byref(a), s)
            dw = _accum_param_grad(w, g)
        return dx, dw, None


def grouped_conv2d(x, w, groups, stride=1, padding="SAME", rate=1):
    """x [N,H,W,C]; w [C,3,3,C/groups] (KRSC per group, fp32 master) -> [N,P,Q,C]."""
    x = as_tensor(x)
    if rate != 1:
        raise ValueError("grouped_conv2d: rate 1 only, got rate %d" % rate)
    if groups == 1:
        return nn.conv2d(x, w, None, stride, padding)
    K, R, S, D = w.shape
    C = x.shape[-1]
    if groups < 1 or C % groups or C // groups != D:
        raise ValueError("grouped_conv2d: groups=%d over %d input channels needs filters of C / groups channels, got %d"
                         % (groups, C, D))
    if K != C:
        raise ValueError("grouped_conv2d: output width %d must equal the input width %d" % (K, C))
    if (R, S) != (3, 3):
        raise ValueError("grouped_conv2d: 3x3 taps only, got %dx%d" % (R, S))
    if isinstance(stride, (tuple, list)):
        if stride[0] != stride[1]:
            raise ValueError("grouped_conv2d: square strides only, got %r" % (stride,))
        stride = stride[0]
    if stride not in (1, 2):
        raise ValueError("grouped_conv2d: stride 1 or 2, got stride %d" % stride)
    if D not in DEPTHS:
        raise ValueError("grouped_conv2d: D = C / groups must be one of %s, got D=%d" % (DEPTHS, D))
    if C % 16:
        raise ValueError("grouped_conv2d: C %% 16 == 0 required, got C=%d" % C)
    g = conv_geom(tuple(x.shape), (C, 3, 3, C), stride, padding)
    a = GcArgs(g.N, g.H, g.W, C, D, g.P, g.Q, g.stride, g.pad_h, g.pad_w)
    if a.ph not in (0, 1) or a.pw not in (0, 1):
        raise ValueError("grouped_conv2d: top / left pad 0 or 1, got padding %r" % (padding,))
    if not eligible(a):
        raise ValueError("grouped_conv2d: geometry N=%d %dx%dx%d D=%d is outside the kernels' range"
                         % (a.N, a.H, a.W, C, D))
    if not x.is_cuda:
        return ref.grouped_conv2d(x, w, groups, stride, padding)
    return _GroupConvFn.apply(x.to(torch.bfloat16), w, a)
