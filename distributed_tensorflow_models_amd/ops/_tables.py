"""The chunk table of the multi-tensor kernels (csrc/kernels/chunk_walk.h: ``ChunkRow`` / ``ChunkSpan``) and the
upload of a host-packed table.  The per-tensor rows differ per kernel family and are packed by their owners."""
import numpy as np
import torch


def chunk_rows(numels, chunk):
    """One row per ``chunk`` elements of every tensor, the rows of a tensor contiguous and in order.

    Returns ``(table, chunk0, nchunks)``: ``table`` is int64 ``[rows, 2]`` = (tensor index, first element), which
    views as ``{int t, int pad, long start}`` (little-endian, t >= 0); ``chunk0[t]`` / ``nchunks[t]`` are tensor t's
    first row and row count (both 0 for a tensor without elements)."""
    rows, chunk0, nchunks = [], [], []
    for t, n in enumerate(numels):
        starts = range(0, int(n), chunk)
        chunk0.append(len(rows) if len(starts) else 0)
        nchunks.append(len(starts))
        rows.extend((t, s) for s in starts)
    table = np.array(rows, dtype=np.int64).reshape(len(rows), 2)
    return table, np.array(chunk0, dtype=np.int64), np.array(nchunks, dtype=np.int64)


def to_device_bytes(array, dev):
    """The bytes of a host-packed numpy table as a uint8 tensor on ``dev``."""
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1).copy()).to(dev)
