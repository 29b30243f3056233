"""Gradient accumulation over a range of the flat gradient buffer (csrc/kernels/grad_accum.hip).

``g`` is a range of the flat fp32 gradient buffer, ``acc`` the same range of the accumulator (parallel/bsp.py):
  STORE  acc = g;        g = 0    after the backward of micro-batch 0 (a bit copy)
  ADD    acc = acc + g;  g = 0    after the backward of micro-batches 1 .. N-2
  FOLD   g = acc + g              micro-batch N-1, before the range's all-reduce
``flag``: a one-element int32 tensor or None; set to 1 when the incoming ``g`` holds an Inf or a NaN, never cleared.
On CPU tensors the same three modes run as torch ops (the CPU path of the feature and the kernel's oracle).
"""
import torch

from . import _lib

STORE, ADD, FOLD = 0, 1, 2


@torch.no_grad()
def grad_accum(acc, g, mode, flag=None):
    if mode not in (STORE, ADD, FOLD):
        raise ValueError("grad_accum mode must be 0 (store), 1 (add) or 2 (fold), got %r" % (mode,))
    if acc.dtype != torch.float32 or g.dtype != torch.float32 or acc.numel() != g.numel():
        raise ValueError("grad_accum needs two fp32 ranges of one length")
    if not (acc.is_contiguous() and g.is_contiguous()) or acc.device != g.device:
        raise ValueError("grad_accum needs two contiguous ranges on one device")
    if flag is not None and (flag.dtype != torch.int32 or flag.numel() != 1 or flag.device != g.device):
        raise ValueError("grad_accum flag must be one int32 on the gradients' device")
    if g.is_cuda:
        rc = _lib.lib().dtm_grad_accum(_lib.ptr(acc), _lib.ptr(g), g.numel(), int(mode), _lib.ptr(flag),
                                       _lib.stream_ptr())
        if rc != 0:
            raise RuntimeError("dtm_grad_accum failed (%d)" % rc)
        return
    if flag is not None and not bool(torch.isfinite(g).all()):
        flag.fill_(1)
    if mode == STORE:
        acc.copy_(g)
        g.zero_()
    elif mode == ADD:
        acc.add_(g)
        g.zero_()
    else:
        torch.add(acc, g, out=g)
