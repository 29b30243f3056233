"""The row walk shared by the multi-tensor kernels (csrc/kernels/chunk_walk.h) and the chunk table they walk
(ops/_tables.py), without a GPU.

The index plan and the walker are plain C++: csrc/kernels/tests/chunk_walk_test.cpp compiles them with the host
compiler and lets every thread of a simulated block walk rows of every element size (2, 4), offset from a 16-byte
boundary, length 0..70, stride (64, 256) and value of the "vector allowed" flag: every element exactly once, every
16-byte group on a boundary and inside the row, each thread's visits in increasing order (head, body, tail)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from distributed_tensorflow_models_amd.ops._tables import chunk_rows, to_device_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "csrc", "kernels")


def test_walk_plan_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "chunk_walk_test")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", KDIR, os.path.join(KDIR, "tests", "chunk_walk_test.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "chunk_walk test OK" in out.stdout, (out.stdout + out.stderr)[-4000:]


def _tables_by_loop(numels, chunk):
    """The loops the four table builders carried before ops/_tables.py (optim.py's form, with its side table)."""
    chunks = []
    for i, n in enumerate(numels):
        for s in range(0, n, chunk):
            chunks.append((i, 0, s))
    ct = np.zeros((len(chunks), 2), dtype=np.int64)
    for j, (i, _, s) in enumerate(chunks):
        ct[j, 0] = i  # int t, int pad packed little-endian into first 8 bytes
        ct[j, 1] = s
    meta = np.zeros((len(numels), 4), dtype=np.int32)
    for j, (i, _, _s) in enumerate(chunks):
        if meta[i, 1] == 0:
            meta[i, 0] = j
        assert meta[i, 0] + meta[i, 1] == j, "chunk rows of a tensor must be contiguous"
        meta[i, 1] += 1
    return ct.view(np.uint8).reshape(-1).copy(), meta


def _numels(c):
    return [[0, 1, c - 1, c, c + 1, 65 * c + 3], [65 * c + 3, 0, 0, c, 1], [1], [0], [], [c + 1, 0, c - 1, 0]]


@pytest.mark.parametrize("case", range(len(_numels(1))))
@pytest.mark.parametrize("chunk", [8192, 32768])  # the optimizer's / SAM's rows and the summary pass's
def test_chunk_rows_match_the_loops(case, chunk):
    numels = _numels(chunk)[case]
    ref_bytes, ref_meta = _tables_by_loop(numels, chunk)
    ct, chunk0, nchunks = chunk_rows(numels, chunk)
    assert ct.dtype == np.int64 and ct.shape == (len(ref_bytes) // 16, 2)
    got = to_device_bytes(ct, "cpu")
    assert got.dtype.is_floating_point is False and got.element_size() == 1 and got.dim() == 1
    assert got.numpy().tobytes() == ref_bytes.tobytes()
    # the {int t, int pad, long start} view of a row
    rows = ct.view(np.dtype([("t", "<i4"), ("pad", "<i4"), ("start", "<i8")])).reshape(-1)
    assert (rows["pad"] == 0).all()
    assert [(int(r["t"]), int(r["start"])) for r in rows] == [(i, s) for i, n in enumerate(numels)
                                                              for s in range(0, n, chunk)]
    # the side table: first row and row count per tensor, 0 / 0 for an empty tensor
    meta = np.zeros((len(numels), 4), dtype=np.int32)
    meta[:, 0], meta[:, 1] = chunk0, nchunks
    assert meta.tobytes() == ref_meta.tobytes()
    assert to_device_bytes(meta, "cpu").numpy().tobytes() == ref_meta.tobytes()


def test_to_device_bytes_structured():
    rec = np.zeros(3, dtype=np.dtype([("x", "<u8"), ("n", "<u8"), ("scale", "<f4"), ("bf16", "<i4"),
                                      ("chunk0", "<u4"), ("nchunks", "<u4")]))
    rec["x"], rec["scale"], rec["nchunks"] = [1, 2, 3], [0.5, 1.0, 2.0], [7, 8, 9]
    got = to_device_bytes(rec, "cpu")
    assert got.shape == (3 * 32,) and got.numpy().tobytes() == rec.tobytes()
    rec["x"][0] = 99  # a copy, not a view of the host table
    assert got.numpy().tobytes() != rec.tobytes()
