"""Summary statistics of many tensors at once: the data behind tf.summary.histogram / tf.nn.zero_fraction.

``TensorStats`` computes, for every tensor of a list, TensorFlow's default-limit histogram (1551 buckets), num,
min, max, sum, sum of squares (fp64), the zero count and the non-finite count.  On the GPU that is TWO launches
for the whole list (csrc/kernels/summary.hip: one block per (tensor, chunk) row of a table built once here, then
one block per tensor), whatever the number of tensors; on the CPU the same quantities come from numpy.

Semantics: each row is a contiguous fp32 or bf16 tensor with its own fp32 ``scale``; the value seen is
``v = float(x) * scale`` (one fp32 multiply).  Non-finite values are counted only: they enter no bucket, min, max,
sum or sum of squares, and ``num`` counts the finite elements.  The bucket of ``v`` is the index of the first limit
strictly greater than ``v``; +-0 land in bucket 776.  With no finite element min = +inf and max = -inf.

A record (one per tensor, from ``fetch()``) is a dict: ``counts`` (uint32 [1551]), ``n``, ``num``, ``min``, ``max``,
``sum``, ``sum_squares``, ``zeros``, ``nonfinite``.
"""
import sys

import numpy as np
import torch

from . import _lib
from ._tables import chunk_rows, to_device_bytes

NUM_BUCKETS = 1551
_limits = None


def limits():
    """TensorFlow's default histogram bucket limits (histogram.cc InitDefaultBucketsInner): the positive limits by
    repeated fp64 multiplication (not pow: the two differ in the last bits), DBL_MAX appended, mirrored around 0."""
    global _limits
    if _limits is None:
        pos = []
        v = 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        pos.append(sys.float_info.max)
        lim = np.array([-p for p in reversed(pos)] + [0.0] + pos, dtype=np.float64)
        assert lim.shape[0] == NUM_BUCKETS
        lim.setflags(write=False)
        _limits = lim
    return _limits


def _values(x, scale):
    """The fp32 values a row stands for: float(x) * scale in fp32."""
    return x.detach().reshape(-1).float().cpu().numpy() * np.float32(scale)


def _stats_numpy(v):
    """Record of a fp32 numpy vector (the CPU path)."""
    fin = np.isfinite(v)
    f = v[fin]
    d = f.astype(np.float64)
    counts = np.bincount(np.searchsorted(limits(), d, side="right"), minlength=NUM_BUCKETS).astype(np.uint32)
    return dict(counts=counts, n=int(v.size), num=int(f.size),
                min=float(f.min()) if f.size else float("inf"), max=float(f.max()) if f.size else float("-inf"),
                sum=float(d.sum()), sum_squares=float((d * d).sum()), zeros=int((f == 0).sum()),
                nonfinite=int(v.size - f.size))


_RESULT_DTYPE = np.dtype([("sum", "<f8"), ("sum_squares", "<f8"), ("min", "<f4"), ("max", "<f4"), ("num", "<u8"),
                          ("zeros", "<u8"), ("nonfinite", "<u8")])


class TensorStats:
    def __init__(self, tensors, scales=None, pinned_from=None):
        """``pinned_from``: an earlier TensorStats over as many tensors whose records have been fetched; its pinned
        host buffers are taken over instead of pinning new ones (tables rebuilt every summary step)."""
        self.tensors = list(tensors)
        if not self.tensors:
            raise ValueError("TensorStats needs at least one tensor")
        self.scales = [1.0] * len(self.tensors) if scales is None else [float(s) for s in scales]
        if len(self.scales) != len(self.tensors):
            raise ValueError("one scale per tensor")
        dev = self.tensors[0].device
        for i, t in enumerate(self.tensors):
            if t.dtype not in (torch.float32, torch.bfloat16):
                raise TypeError("tensor %d: fp32 or bf16 expected, got %s" % (i, t.dtype))
            if not t.is_contiguous():
                raise ValueError("tensor %d is not contiguous" % i)
            if t.numel() == 0:
                raise ValueError("tensor %d is empty" % i)
            if t.numel() >= 2 ** 32:
                raise ValueError("tensor %d has %d elements (limit 2^32 - 1)" % (i, t.numel()))
            if t.device != dev:
                raise ValueError("tensor %d is on %s, the first on %s" % (i, t.device, dev))
        self.device = dev
        self._launched = False
        self._cpu_records = None
        if dev.type == "cuda":
            self._build_tables(pinned_from)

    # ---- device tables (built once, like FusedOptimizer._build_tables) ---------------------------------------
    def _build_tables(self, pinned_from=None):
        L = _lib.lib()
        tb, cb, chunk = L.dtm_stats_tensor_bytes(), L.dtm_stats_chunk_bytes(), L.dtm_stats_chunk_size()
        assert tb == 32 and cb == 16 and L.dtm_stats_num_buckets() == NUM_BUCKETS, (tb, cb)
        assert L.dtm_stats_result_bytes() == _RESULT_DTYPE.itemsize
        T = len(self.tensors)
        tens = np.zeros(T, dtype=np.dtype([("x", "<u8"), ("n", "<u8"), ("scale", "<f4"), ("bf16", "<i4"),
                                           ("chunk0", "<u4"), ("nchunks", "<u4")]))
        ct, chunk0, nchunks = chunk_rows([t.numel() for t in self.tensors], chunk)
        for i, t in enumerate(self.tensors):
            assert t.data_ptr() % t.element_size() == 0
            tens[i] = (t.data_ptr(), t.numel(), self.scales[i], int(t.dtype == torch.bfloat16), chunk0[i], nchunks[i])
        dev = self.device
        self._tens_dev = to_device_bytes(tens, dev)
        self._chunks_dev = to_device_bytes(ct, dev)
        self._nchunks = len(ct)
        self._bins = torch.empty((T, NUM_BUCKETS), dtype=torch.int32, device=dev)  # zeroed by every launch
        self._partials = torch.empty(self._nchunks * L.dtm_stats_partial_bytes(), dtype=torch.uint8, device=dev)
        self._results = torch.empty(T * _RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        old = getattr(pinned_from, "_bins_host", None)
        if old is not None and old.shape[0] == T:
            self._bins_host, self._results_host = pinned_from._bins_host, pinned_from._results_host
        else:
            self._bins_host = torch.empty((T, NUM_BUCKETS), dtype=torch.int32).pin_memory()
            self._results_host = torch.empty(T * _RESULT_DTYPE.itemsize, dtype=torch.uint8).pin_memory()

    def release(self):
        """Drop the tensors and device tables of a fetched pass; only the pinned host buffers stay (``pinned_from``)."""
        self.tensors, self._launched = [], False
        self._tens_dev = self._chunks_dev = self._bins = self._partials = self._results = None

    def launch(self):
        """Enqueue the pass on the current stream (two kernels, then a non-blocking copy of the bins and results
        into pinned host memory).  Not capturable into a hipGraph; synchronise before ``fetch()``.  The pinned
        buffers are reused: fetch one launch's records before launching again."""
        if self.device.type == "cuda":
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TensorStats.launch() inside a hipGraph capture")
            rc = _lib.lib().dtm_tensor_stats(_lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks,
                                             len(self.tensors), _lib.ptr(self._bins), _lib.ptr(self._partials),
                                             _lib.ptr(self._results), _lib.stream_ptr())
            if rc != 0:
                raise RuntimeError("dtm_tensor_stats failed (%d)" % rc)
            self._bins_host.copy_(self._bins, non_blocking=True)
            self._results_host.copy_(self._results, non_blocking=True)
        else:
            self._cpu_records = [_stats_numpy(_values(t, s)) for t, s in zip(self.tensors, self.scales)]
        self._launched = True

    def fetch(self):
        """One record per tensor of the last ``launch()``; the caller has synchronised the stream since."""
        if not self._launched:
            raise RuntimeError("TensorStats.fetch() before launch()")
        if self.device.type != "cuda":
            return self._cpu_records
        bins = self._bins_host.numpy().view(np.uint32)
        res = self._results_host.numpy().view(_RESULT_DTYPE)
        out = []
        for i, t in enumerate(self.tensors):
            r = res[i]
            out.append(dict(counts=bins[i].copy(), n=t.numel(), num=int(r["num"]), min=float(r["min"]),
                            max=float(r["max"]), sum=float(r["sum"]), sum_squares=float(r["sum_squares"]),
                            zeros=int(r["zeros"]), nonfinite=int(r["nonfinite"])))
        return out
