"""Top-k gradient sparsification with error feedback over one bucket (csrc/kernels/grad_compress.hip).

``g`` is a plain bucket's range of the flat fp32 gradient buffer (this rank's summed gradient, not yet scaled),
``res`` the same range of the rank-local residual, ``n`` their length and ``k = bucket_k(n, ratio)``:

  compress_bucket(res, g, k, packet, scratch)
      u[i]   = res[i] + g[i]                            (fp32, round to nearest)
      key(i) = bits(u[i]) & 0x7fffffff as an unsigned   (-0 == +0, denormals order, Inf / NaN largest)
      S      = the first k elements by (key descending, index ascending): exactly k, whatever the ties
      packet = int32[2k]: packet[:k] the indices of S ascending, packet[k:] the bit patterns of u there
      res[i] = +0 where i is in S or u[i] is not finite, else u[i]
      (g is only read)
  decompress_bucket(g, packets, k)        packets: int32[W, 2k], the ranks' packets in rank order
      g = +0; for w = 0 .. W-1 in order: g[idx_w[j]] = g[idx_w[j]] + val_w[j]

On CPU tensors both run as torch / numpy ops with ``numpy.lexsort((index, 0x7fffffff - key))`` for the order: the CPU
path of the feature (gloo ranks) and the kernels' oracle.  A device call allocates nothing and reads nothing back.
"""
import math

import numpy as np
import torch

from . import _lib

KEY_MASK = 0x7fffffff
CHUNK = 8192  # elements per chunk row of the kernels (dtm_gc_chunk_size)

# test-only: device tensors take the CPU forms on host copies (tests/test_grad_compress_gpu.py compares a whole
# training step against them)
FORCE_CPU = False


class GradCompress:
    """Top-k sparsification of the BSP gradient exchange (parallel/bsp.py): every plain bucket sends its
    ``bucket_k(n, ratio)`` largest-magnitude entries of residual + gradient and keeps the rest as the next step's
    residual.  Steps before ``begin_step`` use the dense all-reduce and leave the residual at zero."""
    __slots__ = ("ratio", "begin_step")

    def __init__(self, ratio, begin_step=0):
        try:
            r = float(ratio)
        except (TypeError, ValueError):
            raise ValueError("GradCompress ratio must be a number in (0, 1], got %r" % (ratio,))
        if not (0.0 < r <= 1.0):
            raise ValueError("GradCompress ratio must lie in (0, 1], got %r" % (ratio,))
        if isinstance(begin_step, bool) or int(begin_step) != begin_step or begin_step < 0:
            raise ValueError("GradCompress begin_step must be an integer, at least 0, got %r" % (begin_step,))
        self.ratio, self.begin_step = r, int(begin_step)

    def __repr__(self):
        return "GradCompress(ratio=%r, begin_step=%d)" % (self.ratio, self.begin_step)


def bucket_k(n, ratio):
    """k = min(n, max(1, ceil(ratio * n)))."""
    return min(int(n), max(1, int(math.ceil(float(ratio) * int(n)))))


def check(n, k):
    """The entry points' codes: -2 for n outside [1, 2^31), -3 for k outside [1, n], else 0."""
    if n < 1 or n >= (1 << 31):
        return -2
    if k < 1 or k > n:
        return -3
    return 0


def scratch_words(n):
    """int32 words of device scratch a bucket of n elements needs."""
    if check(n, 1) != 0:
        raise ValueError("a bucket holds 1 .. 2^31 - 1 elements, got %d" % n)
    return 2048 + 8 + 2 * (n // CHUNK + 2)


def _ranges(res, g):
    if res.dtype != torch.float32 or g.dtype != torch.float32 or res.numel() != g.numel():
        raise ValueError("grad compression needs two fp32 ranges of one length")
    if not (res.is_contiguous() and g.is_contiguous()) or res.device != g.device or res.dim() != 1 or g.dim() != 1:
        raise ValueError("grad compression needs two contiguous 1-d ranges on one device")


def _packet(packet, words, dev, what):
    if packet.dtype != torch.int32 or not packet.is_contiguous() or packet.numel() != words or packet.device != dev:
        raise ValueError("%s must be a contiguous int32 tensor of %d words on the gradients' device" % (what, words))


def _raise(rc, n, k):
    if rc == -2:
        raise ValueError("a bucket holds 1 .. 2^31 - 1 elements, got %d" % n)
    if rc == -3:
        raise ValueError("k must lie in [1, n = %d], got %d" % (n, k))
    raise RuntimeError("grad compression kernel launch failed (%d)" % rc)


def compress_cpu(res, g, k, packet):
    """The torch / numpy form on CPU tensors (the documented oracle and the gloo path)."""
    n = g.numel()
    u = res + g
    bits = u.view(torch.int32).numpy()
    key = (bits & KEY_MASK).astype(np.int64)
    index = np.arange(n, dtype=np.int64)
    sel = np.sort(np.lexsort((index, KEY_MASK - key))[:k])
    out = packet.numpy()
    out[:k] = sel
    out[k:] = bits[sel]
    keep = np.isfinite(u.numpy())
    keep[sel] = False
    res.copy_(torch.where(torch.from_numpy(keep), u, torch.zeros_like(u)))


def decompress_cpu(g, packets, k):
    gv = g.numpy()
    gv[:] = 0.0
    pk = packets.numpy()
    for w in range(pk.shape[0]):
        idx = pk[w, :k].astype(np.int64)
        gv[idx] = gv[idx] + pk[w, k:].view(np.float32)  # unique within a packet: a plain gather, add, scatter


@torch.no_grad()
def compress_bucket(res, g, k, packet, scratch=None):
    _ranges(res, g)
    n, k = g.numel(), int(k)
    rc = check(n, k)
    if rc != 0:
        _raise(rc, n, k)
    _packet(packet, 2 * k, g.device, "packet")
    if not g.is_cuda:
        compress_cpu(res, g, k, packet)
        return
    if FORCE_CPU:
        r, p = res.cpu(), packet.cpu()
        compress_cpu(r, g.cpu(), k, p)
        res.copy_(r)
        packet.copy_(p)
        return
    if scratch is None or scratch.dtype != torch.int32 or scratch.device != g.device \
            or scratch.numel() < scratch_words(n) or not scratch.is_contiguous():
        raise ValueError("scratch must be a contiguous int32 device tensor of at least scratch_words(n) words")
    rc = _lib.lib().dtm_grad_compress(_lib.ptr(res), _lib.ptr(g), n, k, _lib.ptr(packet), _lib.ptr(scratch),
                                      _lib.stream_ptr())
    if rc != 0:
        _raise(rc, n, k)


@torch.no_grad()
def decompress_bucket(g, packets, k):
    if g.dtype != torch.float32 or not g.is_contiguous() or g.dim() != 1:
        raise ValueError("grad decompression needs a contiguous 1-d fp32 range")
    n, k = g.numel(), int(k)
    rc = check(n, k)
    if rc != 0:
        _raise(rc, n, k)
    if packets.dim() != 2 or packets.shape[0] < 1:
        raise ValueError("packets must be int32[W, 2k] with W >= 1")
    _packet(packets, packets.shape[0] * 2 * k, g.device, "packets")
    if not g.is_cuda:
        decompress_cpu(g, packets, k)
        return
    if FORCE_CPU:
        h = g.cpu()
        decompress_cpu(h, packets.cpu(), k)
        g.copy_(h)
        return
    rc = _lib.lib().dtm_grad_decompress(_lib.ptr(g), n, _lib.ptr(packets), int(packets.shape[0]), k,
                                        _lib.stream_ptr())
    if rc != 0:
        _raise(rc, n, k)
