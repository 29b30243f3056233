"""Multi-head self-attention over the rows of ``[N, L, heads * d]`` (or NHWC ``[N, H, W, heads * d]``, ``L = H * W``)
on the fused kernels of ``csrc/kernels/attention.hip``: online-softmax forward, recomputing deterministic backward.

CUDA bf16 tensors on one device with ``d`` in {32, 64, 128}, ``1 <= L <= 4096`` and ``N * heads <= 65535`` run the
kernels (hard error if the library is missing, via ``_lib.lib()``); CPU tensors and everything else run the same
definition as a torch composition.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib

HEAD_SIZES = (32, 64, 128)
L_MAX = 4096
GRID_MAX = 65535


def _split(q, k, v, heads):
    if q.dim() not in (3, 4) or q.shape != k.shape or q.shape != v.shape:
        raise ValueError("mhsa: q, k, v of shapes %r, %r, %r where one [N, L, C] or [N, H, W, C] shape is needed"
                         % (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    C = q.shape[-1]
    if heads < 1 or C % heads != 0:
        raise ValueError("mhsa: %d channels do not divide into %d heads" % (C, heads))
    return q.shape[0], q.numel() // (q.shape[0] * C) if q.numel() else 0, C // heads


def eligible(N, L, heads, d):
    return d in HEAD_SIZES and 1 <= L <= L_MAX and heads >= 1 and N >= 1 and N * heads <= GRID_MAX


def _kernel_path(q, k, v, heads):
    N, L, d = _split(q, k, v, heads)
    return (all(t.is_cuda and t.dtype == torch.bfloat16 and t.device == q.device for t in (q, k, v))
            and eligible(N, L, heads, d))


def _rows(t):
    """(tensor, row pitch in elements) with the kernels' layout: contiguous rows, samples L rows apart, the pitch a
    multiple of 8, a 16-byte aligned base.  A last-dimension slice of a contiguous tensor at a multiple of 8 channels
    is taken as it is, anything else is copied."""
    lead, st = t.shape[:-1], t.stride()
    pitch, ok = st[-2], st[-1] == 1
    for i in range(t.dim() - 3, -1, -1):  # every leading stride is the next one times the next extent
        ok = ok and (lead[i] == 1 or st[i] == st[i + 1] * lead[i + 1])
    if ok and pitch >= t.shape[-1] and pitch % 8 == 0 and t.data_ptr() % 16 == 0:
        return t, pitch
    t = t.contiguous()
    return t, t.shape[-1]


def _check(rc):
    if rc != 0:
        raise RuntimeError("attention kernel launch refused: code %d" % rc)


class _MhsaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, scale):
        N, L, d = _split(q, k, v, heads)
        (q, pq), (k, pk), (v, pv) = _rows(q.detach()), _rows(k.detach()), _rows(v.detach())
        o = torch.empty(q.shape, device=q.device, dtype=q.dtype)
        lse = torch.empty((N, heads, L), device=q.device, dtype=torch.float32)
        _check(_lib.lib().dtm_mhsa_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), _lib.ptr(lse), pq, pk, pv,
                                       N, L, heads, d, scale, _lib.stream_ptr()))
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.cfg = (heads, scale, pq, pk, pv)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        heads, scale, pq, pk, pv = ctx.cfg
        N, _, L = lse.shape
        do = do.to(o.dtype).contiguous()
        dq, dk, dv = (torch.empty_like(o) for _ in range(3))
        delta = torch.empty_like(lse)
        _check(_lib.lib().dtm_mhsa_bwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), _lib.ptr(do), _lib.ptr(lse),
                                       _lib.ptr(delta), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), pq, pk, pv, N, L,
                                       heads, o.shape[-1] // heads, scale, _lib.stream_ptr()))
        return dq, dk, dv, None, None


def mhsa_torch(q, k, v, heads, scale=None):
    """The definition as torch ops in the inputs' own type (two batched matrix products and a softmax, autograd's own
    backward): the CPU path and the fallback."""
    N, L, d = _split(q, k, v, heads)
    scale = d ** -0.5 if scale is None else float(scale)
    qh, kh, vh = (t.reshape(N, L, heads, d).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(torch.matmul(qh, kh.transpose(2, 3)) * scale, dim=-1)
    return torch.matmul(p, vh).transpose(1, 2).reshape(q.shape)


def mhsa(q, k, v, heads, scale=None):
    """softmax(scale q k^T) v per sample and head over bf16 ``[N, L, heads * d]`` or NHWC ``[N, H, W, heads * d]``
    (``L = H * W``); channel ``h * d + c`` is component ``c`` of head ``h``; ``scale`` defaults to ``d ** -0.5``.
    Returns a contiguous tensor of q's shape.  Each argument may be a last-dimension slice of a wider tensor (the
    thirds of a fused qkv row): the kernels take a row pitch per tensor.

    Kernel path: logits, softmax statistics (row max, row sum, ``lse``) and ``delta = sum_c dO * O`` are fp32 from the
    stored bf16 inputs, and the result is rounded once; the probabilities ``P`` (forward and ``dV = P^T dO``) and
    ``dS = P * (dP - delta)`` (``dQ``, ``dK``) are multiplied as bf16 MFMA operands - that rounding is part of the
    definition of the kernel path.  The row sum is taken from the unrounded ``P``."""
    N, L, d = _split(q, k, v, heads)
    if _kernel_path(q, k, v, heads):
        return _MhsaFn.apply(q, k, v, heads, d ** -0.5 if scale is None else float(scale))
    return mhsa_torch(q, k, v, heads, scale)
