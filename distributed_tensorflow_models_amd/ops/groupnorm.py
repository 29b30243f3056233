"""Group normalisation on NHWC (``csrc/kernels/groupnorm.hip``): per sample and group of ``C / groups`` channels,
statistics over H, W and the group's channels; ``groups == C`` is instance norm, ``groups == 1`` layer norm.

CUDA bf16 / fp32 tensors of an eligible shape (``C % 8 == 0`` and ``C / groups`` in {1, 2, 4} or a multiple of 8) run
the slab-split kernels (hard error if the library is missing, via ``_lib.lib()``); CPU tensors and every other shape
run the same definition as a torch composition.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib

# the automatic slab rule sizes grids for this part whatever device runs them: results keep their bits across machines
_RULE_CUS, _RULE_BLOCKS_PER_CU, _MIN_SLAB, _MAX_SLABS = 256, 4, 32, 128


def eligible(C, groups):
    cg = C // groups
    return C % 8 == 0 and C % groups == 0 and (cg in (1, 2, 4) or cg % 8 == 0)


def auto_slab_pixels(N, HW, C):
    """Pixels per slab from the shape alone: enough slabs for a few blocks per CU where the tensor allows it, no slab
    below 32 pixels or below one pixel per pixel lane, and at most 128 slabs a sample (every block of a sample merges
    all of its slab records again)."""
    floor = max(_MIN_SLAB, 256 // min(C // 8, 256))
    want = -(-_RULE_CUS * _RULE_BLOCKS_PER_CU // N)
    slabs = max(1, min(want, HW // floor, _MAX_SLABS))
    return -(-HW // slabs)


def _kernel_path(x, groups, gamma, beta):
    """The kernels read x as bf16 / fp32 NHWC and the parameters as fp32 [C] on x's device; N rides the grid's y."""
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and x.dim() == 4 and x.numel() > 0
            and x.shape[0] <= 65535 and eligible(x.shape[-1], groups)):
        return False
    return all(p is None or (p.device == x.device and p.dtype == torch.float32 and p.shape == x.shape[-1:])
               for p in (gamma, beta))


def _check(rc):
    if rc != 0:
        raise RuntimeError("groupnorm kernel launch refused: code %d" % rc)


class _GroupNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu, slab_pixels):
        x = x.contiguous()
        gamma = None if gamma is None else gamma.contiguous()
        beta = None if beta is None else beta.contiguous()
        N, H, W, C = x.shape
        L, bf16 = _lib.lib(), int(x.dtype == torch.bfloat16)
        y = torch.empty_like(x)
        stats = torch.empty((N, groups, 2), device=x.device, dtype=torch.float32)
        ws = torch.empty(L.dtm_groupnorm_ws_floats(N, H * W, C, groups, slab_pixels, 0), device=x.device,
                         dtype=torch.float32)
        _check(L.dtm_groupnorm_fwd(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(y), _lib.ptr(stats),
                                   _lib.ptr(ws), ws.numel(), N, H * W, C, groups, slab_pixels, float(eps), int(relu),
                                   bf16, _lib.stream_ptr()))
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.cfg = (groups, relu, slab_pixels)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, beta, stats = ctx.saved_tensors
        groups, relu, slab_pixels = ctx.cfg
        N, H, W, C = x.shape
        L, bf16 = _lib.lib(), int(x.dtype == torch.bfloat16)
        dy = dy.contiguous().to(x.dtype)
        dx = torch.empty_like(x)
        f32 = dict(device=x.device, dtype=torch.float32)
        dgamma = torch.empty(C, **f32) if gamma is not None and ctx.needs_input_grad[1] else None
        dbeta = torch.empty(C, **f32) if beta is not None and ctx.needs_input_grad[2] else None
        ws = torch.empty(L.dtm_groupnorm_ws_floats(N, H * W, C, groups, slab_pixels, 1), **f32)
        sums = torch.empty((N, C, 2), **f32)
        _check(L.dtm_groupnorm_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(stats),
                                   _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), ws.numel(),
                                   _lib.ptr(sums), N, H * W, C, groups, slab_pixels, int(relu), bf16,
                                   _lib.stream_ptr()))
        return dx, dgamma, dbeta, None, None, None, None


def group_norm_torch(x, groups, gamma=None, beta=None, eps=1e-6, relu=False):
    """The definition as torch ops: [N, HW, G, Cg], fp32 moments, affine, ReLU, one rounding to x's type."""
    N, C = x.shape[0], x.shape[-1]
    xf = x.float().reshape(N, -1, groups, C // groups)
    mean = xf.mean(dim=(1, 3), keepdim=True)
    var = xf.var(dim=(1, 3), keepdim=True, unbiased=False)
    y = ((xf - mean) * torch.rsqrt(var + eps)).reshape(x.shape)
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype)


def group_norm(x, groups, gamma=None, beta=None, eps=1e-6, relu=False, slab_pixels=None):
    """y = act((x - mean_ng) * rsqrt(var_ng + eps) * gamma + beta) on NHWC ``x``; ``gamma`` / ``beta`` fp32 [C] or
    None.  ``slab_pixels``: pixels per block of the kernels' work split (None = ``auto_slab_pixels``); it is raised
    where it would cut a sample into more than 128 slabs, since every block merges all of its sample's slab records."""
    C = x.shape[-1]
    if groups < 1 or C % groups != 0:
        raise ValueError("group_norm: %d channels do not divide into %d groups" % (C, groups))
    if _kernel_path(x, groups, gamma, beta):
        N, H, W, _ = x.shape
        if slab_pixels is None:
            sp = auto_slab_pixels(N, H * W, C)
        else:
            sp = max(1, int(slab_pixels), -(-H * W // _MAX_SLABS))
        return _GroupNormFn.apply(x, gamma, beta, groups, eps, relu, sp)
    return group_norm_torch(x, groups, gamma, beta, eps, relu)
