"""The two-launch multi-tensor summary pass (csrc/kernels/summary.hip) against the plain oracle and the CPU path,
its run-to-run reproducibility, and the trainer's summary flags on the GPU (captured and eager step)."""
import os

import numpy as np
import pytest
import torch

from test_summary import (EXACT, SCALES, adversarial_values, as_dtype, assert_checkpoints_bit_equal, check_record,
                          event_values, run_trainer, seen_values)

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def _chunk():
    from distributed_tensorflow_models_amd.ops import _lib
    return _lib.lib().dtm_stats_chunk_size()


def _sizes():
    c = _chunk()
    return [1, 255, 256, 257, c - 1, c, c + 1, 3 * c + 17]


_base = {}


def _base_values():
    """The adversarial set in a fixed shuffled order (so short tensors get special values too), repeated to the
    largest size."""
    if "v" not in _base:
        adv = adversarial_values()
        _base["v"] = np.resize(np.random.RandomState(7).permutation(adv), 3 * _chunk() + 18)
    return _base["v"]


def _run(tensors, scales):
    from distributed_tensorflow_models_amd.ops.summary import TensorStats
    st = TensorStats(tensors, scales)
    st.launch()
    torch.cuda.synchronize()
    return st.fetch()


def _check_all(tensors, scales, recs):
    from distributed_tensorflow_models_amd.ops import reference
    assert len(recs) == len(tensors)
    for i, (x, s, rec) in enumerate(zip(tensors, scales, recs)):
        check_record(rec, reference.tensor_stats(x, s), seen_values(x, s),
                     "row %d n %d scale %g %s" % (i, x.numel(), s, x.dtype))


def _flat_table(dtype, dev):
    """Every size back to back in ONE flat buffer that itself starts one element into its allocation: tensor
    boundaries fall anywhere relative to the 16-byte boundaries and chunk boundaries meet tensor boundaries."""
    sizes = _sizes()
    total = sum(sizes)
    flat = as_dtype(np.resize(_base_values(), total + 1), dtype).to(dev)
    tensors, scales, off = [], [], 1
    for i, n in enumerate(sizes):
        tensors.append(flat[off:off + n])
        scales.append(SCALES[i % len(SCALES)])
        off += n
    return flat, tensors, scales


def test_abi_limits_match():
    from distributed_tensorflow_models_amd.ops import _lib
    from distributed_tensorflow_models_amd.ops.summary import NUM_BUCKETS, limits
    L = _lib.lib()
    assert L.dtm_stats_num_buckets() == NUM_BUCKETS
    out = np.zeros(NUM_BUCKETS, dtype=np.float64)
    L.dtm_stats_limits(out.ctypes.data)
    assert out.tobytes() == limits().tobytes()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel_matches_oracle_sizes(dtype):
    dev = torch.device("cuda", 0)
    base = _base_values()
    tensors = [as_dtype(base[:n], dtype).to(dev) for n in _sizes()]
    scales = [1.0] * len(tensors)
    # a tensor that starts one element into its buffer (misaligned head), at the other two scales
    for n, s in ((257, 0.125), (_chunk() + 1, 0.37)):
        buf = as_dtype(base[:n + 1], dtype).to(dev)
        tensors.append(buf[1:])
        scales.append(s)
    _check_all(tensors, scales, _run(tensors, scales))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_contention_rows_unshuffled(dtype):
    """The contention case: rows in which every lane of every wave hits ONE LDS bin (more than a chunk of a single
    value, so also across a chunk boundary; a block of zeros), and the adversarial vector in its own order - its
    4096 equal values and 512 zeros are contiguous there, and its limit neighbours come in bucket order."""
    dev = torch.device("cuda", 0)
    c = _chunk()
    rows = [np.full(c + 300, 0.5, np.float32), np.zeros(2 * c, np.float32), np.full(4099, -3.0e-7, np.float32),
            adversarial_values()]
    tensors = [as_dtype(r, dtype).to(dev) for r in rows]
    scales = [1.0, 1.0, 0.37, 1.0]
    recs = _run(tensors, scales)
    _check_all(tensors, scales, recs)
    assert int(recs[0]["counts"].max()) == c + 300 and int(recs[1]["counts"][776]) == 2 * c == recs[1]["zeros"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mixed_table_oracle_cpu_and_reproducible(dtype):
    from distributed_tensorflow_models_amd.ops.summary import TensorStats
    dev = torch.device("cuda", 0)
    flat, tensors, scales = _flat_table(dtype, dev)
    recs = _run(tensors, scales)
    _check_all(tensors, scales, recs)
    # GPU against the CPU path on the same data
    cpu = TensorStats([t.cpu().contiguous() for t in tensors], scales)
    cpu.launch()
    for g, c in zip(recs, cpu.fetch()):
        np.testing.assert_array_equal(g["counts"], c["counts"])
        for k in EXACT:
            assert g[k] == c[k], (k, g[k], c[k])
    # a second launch after a dummy allocation, over a freshly allocated copy: bit-identical in every field
    dummy = torch.empty(12345, dtype=torch.uint8, device=dev)
    flat2 = torch.empty_like(flat)
    flat2.copy_(flat)
    off, t2 = 1, []
    for t in tensors:
        t2.append(flat2[off:off + t.numel()])
        off += t.numel()
    again = _run(t2, scales)
    del dummy
    for a, b in zip(recs, again):
        assert a["counts"].tobytes() == b["counts"].tobytes()
        for k in EXACT:
            assert a[k] == b[k], k
        for k in ("sum", "sum_squares", "min", "max"):
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), k


def test_fp32_and_bf16_rows_in_one_table():
    dev = torch.device("cuda", 0)
    base = _base_values()
    tensors = [as_dtype(base[:1000], torch.float32).to(dev), as_dtype(base[:1000], torch.bfloat16).to(dev),
               as_dtype(base[3:260], torch.float32).to(dev)]
    scales = [0.37, 0.125, 1.0]
    _check_all(tensors, scales, _run(tensors, scales))


@pytest.mark.parametrize("mod,model,extra", [
    ("mnist_lenet_bsp", "lenet", ["--use_hipgraph"]),
    ("mnist_lenet_bsp", "lenet", []),
    # BatchNorm moving statistics and EMA slots: the extra activation forward must leave them alone on the GPU too
    ("cifar10_resnet_bsp", None, ["--resnet_size=8", "--train_accuracy_every=0"]),
], ids=["lenet-hipgraph", "lenet-eager", "resnet-eager"])
def test_trainer_gpu_summaries(tmp_path, mod, model, extra):
    from distributed_tensorflow_models_amd.models import nets_factory
    common = ["--synthetic_data", "--max_steps=4", "--batch_size=8", "--data_dir=/nonexistent", "--deterministic",
              "--seed=5"] + extra
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    run_trainer(mod, "--train_dir=" + on, "--save_summaries_steps=1", "--summary_histograms",
                "--summary_activations", *common)
    run_trainer(mod, "--train_dir=" + off, *common)
    ev = event_values(on)
    assert sorted(ev) == [1, 2, 3, 4]
    for step, tags in ev.items():
        grads = [t for t in tags if t.endswith("/gradients")]
        assert grads
        for t in grads:  # live gradients: not a zeroed buffer (all of it in bucket 776, sum of squares 0)
            assert tags[t]["histo"]["sum_squares"] > 0.0, (step, t)
            assert tags[t]["histo"]["num"] == tags[t[:-len("/gradients")]]["histo"]["num"]
    if model is not None:
        params = {p.tf_name: p.numel() for p in nets_factory.build(model, num_classes=10).parameters()
                  if p.requires_grad}
        for step, tags in ev.items():
            for name, n in params.items():
                assert tags[name]["histo"]["num"] == n, (step, name)
                assert tags[name + "/gradients"]["histo"]["num"] == n, (step, name)
            for e in ("LeNet/conv1", "LeNet/pool2", "LeNet/fc3", "LeNet/Logits"):
                assert "histo" in tags[e + "/activations"] and "simple_value" in tags[e + "/sparsity"], (step, e)
    else:
        assert any("batch_normalization" in t for t in ev[4])
    assert_checkpoints_bit_equal(os.path.join(on, "model.ckpt-4"), os.path.join(off, "model.ckpt-4"))
