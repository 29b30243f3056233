"""Histogram / sparsity / image summaries on the CPU: TensorFlow's default bucket limits, the numpy path of
ops.summary.TensorStats against the plain oracle ops.reference.tensor_stats, the event encoding against a
hand-checked golden and an independent protobuf decoder, and the trainer flags end to end."""
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."
FLT_MAX = float(np.finfo(np.float32).max)
SCALES = (1.0, 0.125, 0.37)
EXACT = ("n", "num", "min", "max", "zeros", "nonfinite")


# ---- shared with tests/test_summary_gpu.py ---------------------------------------------------------------------
def adversarial_values():
    """fp32 vector: for every limit float32(limit) and its two fp32 neighbours, +-0, the smallest and largest
    denormals, +-FLT_MAX, NaN, +-Inf, a block of equal values (every lane on one bin) and random normals at
    scales 1e-8, 1 and 1e8."""
    from distributed_tensorflow_models_amd.ops.summary import limits
    with np.errstate(over="ignore"):
        f = limits().astype(np.float32)  # +-DBL_MAX -> +-inf: its inner neighbour is +-FLT_MAX
    inf = np.float32(np.inf)
    tiny = np.float32(1.401298464324817e-45)
    maxden = np.float32(1.1754942106924411e-38)
    special = np.array([0.0, -0.0, tiny, -tiny, maxden, -maxden, FLT_MAX, -FLT_MAX, np.nan, np.inf, -np.inf],
                       dtype=np.float32)
    rng = np.random.RandomState(1234)
    rnd = [rng.standard_normal(2048).astype(np.float32) * np.float32(s) for s in (1e-8, 1.0, 1e8)]
    return np.concatenate([np.nextafter(f, -inf), f, np.nextafter(f, inf), special,
                           np.full(4096, 0.5, np.float32), np.zeros(512, np.float32)] + rnd).astype(np.float32)


def as_dtype(v, dtype):
    """torch tensor of dtype; for bf16 the values become those after rounding to bf16."""
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype)


def check_record(got, ref, values, label=""):
    """The exact fields are equal; sum and sum_squares are within the fp64 reordering bound n * 2^-52 * sum|v|
    (resp. sum v^2) of the oracle's correctly rounded sums - derived, not measured."""
    np.testing.assert_array_equal(np.asarray(got["counts"], dtype=np.int64), np.asarray(ref["counts"], dtype=np.int64),
                                  err_msg=label)
    for k in EXACT:
        assert got[k] == ref[k], (label, k, got[k], ref[k])
    assert int(np.asarray(got["counts"], dtype=np.int64).sum()) == got["num"], label
    d = values[np.isfinite(values)].astype(np.float64)
    n = max(d.size, 1)
    b1 = n * 2.0 ** -52 * math.fsum(np.abs(d).tolist())
    b2 = n * 2.0 ** -52 * math.fsum((d * d).tolist())
    assert abs(got["sum"] - ref["sum"]) <= b1, (label, got["sum"], ref["sum"], b1)
    assert abs(got["sum_squares"] - ref["sum_squares"]) <= b2, (label, got["sum_squares"], ref["sum_squares"], b2)


def seen_values(t, scale):
    """The fp32 values a row stands for (float(x) * scale, one fp32 multiply), as numpy."""
    return t.detach().reshape(-1).float().cpu().numpy() * np.float32(scale)


# ---- limits -------------------------------------------------------------------------------------------------------
def test_limits_table():
    from distributed_tensorflow_models_amd.ops.summary import NUM_BUCKETS, limits
    lim = limits()
    assert NUM_BUCKETS == 1551 and lim.shape == (1551,) and lim.dtype == np.float64
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[-1] == sys.float_info.max and lim[0] == -sys.float_info.max
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    assert len(pos) == 774
    assert lim[776:1550].tobytes() == np.array(pos, dtype=np.float64).tobytes()  # bit for bit
    assert lim[:775].tobytes() == (-lim[776:][::-1]).tobytes()
    assert np.all(np.diff(lim) > 0)
    # no fp32 value other than 0 equals a limit: the strict / non-strict side of the comparison is unobservable
    with np.errstate(over="ignore"):
        f = lim.astype(np.float32).astype(np.float64)
    assert np.flatnonzero(f == lim).tolist() == [775]


def test_oracle_hand_values():
    from distributed_tensorflow_models_amd.ops import reference
    r = reference.tensor_stats(np.array([-1.0, 0.0, -0.0, 2.5, np.nan, np.inf], dtype=np.float32))
    assert (r["n"], r["num"], r["zeros"], r["nonfinite"]) == (6, 4, 2, 2)
    assert (r["min"], r["max"], r["sum"], r["sum_squares"]) == (-1.0, 2.5, 1.5, 7.25)
    assert r["counts"][776] == 2 and int(r["counts"].sum()) == 4
    r = reference.tensor_stats(np.array([8.0], dtype=np.float32), 0.125)
    assert r["sum"] == 1.0 and r["min"] == 1.0


# ---- CPU path against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_cpu_path_matches_oracle(dtype):
    from distributed_tensorflow_models_amd.ops import reference
    from distributed_tensorflow_models_amd.ops.summary import TensorStats
    t = as_dtype(adversarial_values(), dtype)
    rows = [t, t[1:257].clone(), t[:1].clone()]
    tensors = [r for r in rows for _ in SCALES]
    scales = [s for _ in rows for s in SCALES]
    st = TensorStats(tensors, scales)
    with pytest.raises(RuntimeError):
        st.fetch()
    st.launch()
    recs = st.fetch()
    assert len(recs) == len(tensors)
    for i, (x, s, rec) in enumerate(zip(tensors, scales, recs)):
        check_record(rec, reference.tensor_stats(x, s), seen_values(x, s), "row %d scale %g" % (i, s))


def test_table_rejects_bad_rows():
    from distributed_tensorflow_models_amd.ops.summary import TensorStats
    with pytest.raises(ValueError):
        TensorStats([torch.zeros(0)])
    with pytest.raises(TypeError):
        TensorStats([torch.zeros(4, dtype=torch.float64)])
    with pytest.raises(ValueError):
        TensorStats([torch.zeros(4, 4).t()])


# ---- event encoding ---------------------------------------------------------------------------------------------
GOLDEN_LIMITS = [-1.0089710279437536, -0.917246389039776, 0.0, 1e-12, 2.379100905625872, 2.6170109961884593,
                 1.7976931348623157e+308]
GOLDEN_BUCKETS = [0, 1, 0, 2, 0, 1, 0]


def _golden_record():
    from distributed_tensorflow_models_amd.ops.summary import TensorStats
    st = TensorStats([torch.tensor([-1.0, 0.0, 0.0, 2.5])])
    st.launch()
    return st.fetch()[0]


def test_histogram_golden(tmp_path):
    from distributed_tensorflow_models_amd.utils import tb
    rec = _golden_record()
    bl, bc = tb.histogram_buckets(rec)
    assert bl == GOLDEN_LIMITS and bc == GOLDEN_BUCKETS
    w = tb.SummaryWriter(str(tmp_path))
    w.add_histogram("h", rec, 7)
    w.close()
    ev = tb.read_events(w.path)
    assert ev[0]["file_version"] == "brain.Event:2" and ev[1]["step"] == 7
    (val,) = ev[1]["values"]
    h = val["histo"]
    assert val["tag"] == "h"
    assert h["bucket_limit"] == GOLDEN_LIMITS and h["bucket"] == GOLDEN_BUCKETS
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (-1.0, 2.5, 4.0, 1.5, 7.25)


def _proto_classes():
    """Event / Summary / HistogramProto message classes built at run time from the field numbers of the TensorFlow
    protos (an implementation independent of utils/tb.py's hand-written wire code)."""
    from google.protobuf import descriptor_pb2, descriptor_pool
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="dtm_test_event.proto", package="dtmtest", syntax="proto3")

    def msg(name, fields):
        m = fd.message_type.add(name=name)
        for fname, num, typ, rep, tname in fields:
            f = m.field.add(name=fname, number=num, type=typ,
                            label=F.LABEL_REPEATED if rep else F.LABEL_OPTIONAL)
            if tname:
                f.type_name = ".dtmtest." + tname
    msg("HistogramProto", [("min", 1, F.TYPE_DOUBLE, 0, None), ("max", 2, F.TYPE_DOUBLE, 0, None),
                           ("num", 3, F.TYPE_DOUBLE, 0, None), ("sum", 4, F.TYPE_DOUBLE, 0, None),
                           ("sum_squares", 5, F.TYPE_DOUBLE, 0, None), ("bucket_limit", 6, F.TYPE_DOUBLE, 1, None),
                           ("bucket", 7, F.TYPE_DOUBLE, 1, None)])
    msg("Image", [("height", 1, F.TYPE_INT32, 0, None), ("width", 2, F.TYPE_INT32, 0, None),
                  ("colorspace", 3, F.TYPE_INT32, 0, None), ("encoded_image_string", 4, F.TYPE_BYTES, 0, None)])
    msg("Value", [("tag", 1, F.TYPE_STRING, 0, None), ("simple_value", 2, F.TYPE_FLOAT, 0, None),
                  ("image", 4, F.TYPE_MESSAGE, 0, "Image"), ("histo", 5, F.TYPE_MESSAGE, 0, "HistogramProto")])
    msg("Summary", [("value", 1, F.TYPE_MESSAGE, 1, "Value")])
    msg("Event", [("wall_time", 1, F.TYPE_DOUBLE, 0, None), ("step", 2, F.TYPE_INT64, 0, None),
                  ("file_version", 3, F.TYPE_STRING, 0, None), ("summary", 5, F.TYPE_MESSAGE, 0, "Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    desc = pool.FindMessageTypeByName("dtmtest.Event")
    try:
        from google.protobuf import message_factory
        return message_factory.GetMessageClass(desc)
    except (ImportError, AttributeError):
        from google.protobuf import message_factory
        return message_factory.MessageFactory(pool).GetPrototype(desc)


def _decode_independent(path):
    from distributed_tensorflow_models_amd.data.tfrecord import tf_record_iterator
    Event = _proto_classes()
    out = []
    for rec in tf_record_iterator(path):
        e = Event()
        e.ParseFromString(rec)
        out.append(e)
    return out


def test_events_decode_with_protobuf(tmp_path):
    from PIL import Image
    from distributed_tensorflow_models_amd.utils import tb
    rec = _golden_record()
    rng = np.random.RandomState(0)
    rgb = rng.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    grey = rng.randint(0, 256, (4, 3, 1)).astype(np.uint8)
    w = tb.SummaryWriter(str(tmp_path))
    w.add_scalar("s", 0.25, 1)
    w.add_histogram("h", rec, 2)
    w.add_image("rgb", rgb, 3)
    w.add_summaries([tb.scalar_value("a/sparsity", 0.5), tb.histogram_value("a/activations", rec),
                     tb.image_value("grey", grey)], 4)
    w.close()
    evs = _decode_independent(w.path)
    assert evs[0].file_version == "brain.Event:2"
    assert [e.step for e in evs[1:]] == [1, 2, 3, 4]
    assert [[v.tag for v in e.summary.value] for e in evs[1:]] == [["s"], ["h"], ["rgb"],
                                                                   ["a/sparsity", "a/activations", "grey"]]
    assert evs[1].summary.value[0].simple_value == 0.25
    for h in (evs[2].summary.value[0].histo, evs[4].summary.value[1].histo):
        assert list(h.bucket_limit) == GOLDEN_LIMITS and list(h.bucket) == GOLDEN_BUCKETS
        assert (h.min, h.max, h.num, h.sum, h.sum_squares) == (-1.0, 2.5, 4.0, 1.5, 7.25)
    for im, src in ((evs[3].summary.value[0].image, rgb), (evs[4].summary.value[2].image, grey)):
        assert (im.height, im.width, im.colorspace) == src.shape
        px = np.asarray(Image.open(io.BytesIO(im.encoded_image_string)))
        np.testing.assert_array_equal(px.reshape(src.shape), src)
    # the project's own reader agrees with the protobuf decoder
    mine = tb.read_events(w.path)
    assert len(mine) == len(evs)
    for a, b in zip(mine, evs):
        assert a["step"] == b.step and a["wall_time"] == b.wall_time
        assert [v["tag"] for v in a["values"]] == [v.tag for v in b.summary.value]
        for va, vb in zip(a["values"], b.summary.value):
            if "simple_value" in va:
                assert va["simple_value"] == vb.simple_value
            if "histo" in va:
                assert va["histo"]["bucket_limit"] == list(vb.histo.bucket_limit)
                assert va["histo"]["bucket"] == list(vb.histo.bucket)
                assert va["histo"]["sum_squares"] == vb.histo.sum_squares and va["histo"]["min"] == vb.histo.min
            if "image" in va:
                assert va["image"]["encoded_image_string"] == vb.image.encoded_image_string
                assert (va["image"]["height"], va["image"]["width"]) == (vb.image.height, vb.image.width)


def test_images_to_uint8_rule():
    from distributed_tensorflow_models_amd.utils.summaries import images_to_uint8
    x = torch.zeros(4, 3, 3, 1)  # N, H, W, C = 1
    x[0, :, :, 0] = torch.tensor([[-2.0, 0.0, 1.0], [0.5, 0.5, 0.5], [2.0, 2.0, -1.0]])  # signed: 128 + x * 127 / 2
    x[1, :, :, 0] = torch.tensor([[0.0, 1.0, 4.0], [2.0, 2.0, 2.0], [float("nan"), 0.0, 0.0]])  # x * 255 / 4, NaN -> red
    x[3, :, :, 0] = torch.tensor([[0.0, 0.0, 0.0], [float("inf"), 1.0, 1.0], [-1.0, 0.0, 1.0]])
    y = images_to_uint8(x).numpy()
    assert y.dtype == np.uint8 and y.shape == (4, 3, 3, 1)
    assert y[0, :, :, 0].tolist() == [[1, 128, 191], [159, 159, 159], [255, 255, 64]]
    assert y[1, :, :, 0].tolist() == [[0, 63, 255], [127, 127, 127], [255, 0, 0]]
    assert y[2].max() == 0  # all zero: scale 0
    assert y[3, :, :, 0].tolist() == [[128, 128, 128], [255, 255, 255], [1, 128, 255]]  # Inf -> red (255 at C = 1)
    z = torch.tensor([[[[0.0, float("nan"), 1.0], [1.0, 1.0, 1.0]]]])  # C = 3: a pixel with a NaN channel is red
    assert images_to_uint8(z)[0, 0].tolist() == [[255, 0, 0], [255, 255, 255]]
    u = torch.arange(12, dtype=torch.uint8).reshape(1, 2, 2, 3)
    assert images_to_uint8(u) is u


# ---- trainer -----------------------------------------------------------------------------------------------------
SCALARS = ["learning_rate", "total_loss (raw)", "total_loss", "images_per_sec"]
SUMMARY_FLAGS = ["--save_summaries_steps=1", "--summary_histograms", "--summary_activations", "--summary_images=2"]


def run_trainer(mod, *args, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    return p.stdout + p.stderr


def event_values(train_dir):
    """{step: {tag: value dict}} of the single event file of a train_dir."""
    from distributed_tensorflow_models_amd.utils import tb
    files = [f for f in os.listdir(train_dir) if f.startswith("events.out.tfevents")]
    assert len(files) == 1, files
    out = {}
    for ev in tb.read_events(os.path.join(train_dir, files[0])):
        for v in ev["values"]:
            assert v["tag"] not in out.setdefault(ev["step"], {}), (ev["step"], v["tag"])
            out[ev["step"]][v["tag"]] = v
    return out


def checkpoint_tensors(prefix):
    from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
    r = BundleReader(prefix)
    return {n: np.asarray(r.get_tensor(n)) for n in r.names()}


def assert_checkpoints_bit_equal(a, b):
    ta, tb_ = checkpoint_tensors(a), checkpoint_tensors(b)
    assert sorted(ta) == sorted(tb_) and len(ta) > 4
    for n in ta:
        assert ta[n].dtype == tb_[n].dtype and ta[n].tobytes() == tb_[n].tobytes(), n


@pytest.fixture(scope="module")
def lenet_runs(tmp_path_factory):
    """LeNet, synthetic data, 3 steps, same seed: once with every summary flag, once with none."""
    base = tmp_path_factory.mktemp("summary_trainer")
    common = ["--synthetic_data", "--max_steps=3", "--batch_size=8", "--data_dir=/nonexistent", "--deterministic",
              "--seed=3"]
    on, off = str(base / "on"), str(base / "off")
    out = run_trainer("mnist_lenet_bsp", "--train_dir=" + on, *(common + SUMMARY_FLAGS))
    run_trainer("mnist_lenet_bsp", "--train_dir=" + off, *common)
    return on, off, out


def test_trainer_writes_summaries(lenet_runs):
    from distributed_tensorflow_models_amd.models import nets_factory
    on, _, out = lenet_runs
    ev = event_values(on)
    assert sorted(ev) == [1, 2, 3]
    model = nets_factory.build("lenet", num_classes=10)
    params = {p.tf_name: p.numel() for p in model.parameters() if p.requires_grad}
    assert len(params) == 8
    for step in (1, 2, 3):
        tags = ev[step]
        for name, n in params.items():
            assert tags[name]["histo"]["num"] == n, (step, name)
            assert tags[name + "/gradients"]["histo"]["num"] == n, (step, name)
            assert tags[name + "/gradients"]["histo"]["sum_squares"] > 0.0, (step, name)  # live, not zeroed
            assert sum(tags[name]["histo"]["bucket"]) == n
        for e in ("LeNet/conv1", "LeNet/pool1", "LeNet/conv2", "LeNet/pool2", "LeNet/fc3", "LeNet/Logits"):
            assert "histo" in tags[e + "/activations"], (step, e)
            assert 0.0 <= tags[e + "/sparsity"]["simple_value"] <= 1.0
        assert tags["LeNet/conv1/sparsity"]["simple_value"] > 0.0  # a ReLU output has zeros
        for i in (0, 1):
            im = tags["images/image/%d" % i]["image"]
            assert (im["height"], im["width"], im["colorspace"]) == (28, 28, 1)
            assert im["encoded_image_string"][:8] == b"\x89PNG\r\n\x1a\n"
        for s in SCALARS:
            assert "simple_value" in tags[s], (step, s)
        assert len(tags) == 2 * len(params) + 2 * 6 + 2 + 4
    assert "non-finite" not in out


def test_trainer_flags_off_scalars_only(lenet_runs):
    _, off, _ = lenet_runs
    ev = event_values(off)
    assert ev and all(sorted(tags) == sorted(SCALARS) for tags in ev.values())


def test_summaries_do_not_change_training(lenet_runs):
    on, off, _ = lenet_runs
    tags = event_values(on)[3]  # the compared run did write histograms, activations and images
    assert "histo" in tags["LeNet/conv1/weights/gradients"] and "histo" in tags["LeNet/fc3/activations"]
    assert "image" in tags["images/image/1"]
    assert_checkpoints_bit_equal(os.path.join(on, "model.ckpt-3"), os.path.join(off, "model.ckpt-3"))


@pytest.fixture(scope="module")
def resnet_runs(tmp_path_factory):
    """The smallest CIFAR ResNet (BatchNorm moving statistics, EMA slot variables), 3 steps, same seed, with and
    without the summary flags: the activation pass runs an extra training-mode forward, which must leave the moving
    statistics alone."""
    base = tmp_path_factory.mktemp("summary_resnet")
    common = ["--synthetic_data", "--max_steps=3", "--batch_size=4", "--data_dir=/nonexistent", "--deterministic",
              "--seed=3", "--resnet_size=8", "--train_accuracy_every=0"]
    on, off = str(base / "on"), str(base / "off")
    run_trainer("cifar10_resnet_bsp", "--train_dir=" + on, *(common + SUMMARY_FLAGS))
    run_trainer("cifar10_resnet_bsp", "--train_dir=" + off, *common)
    return on, off


def test_summaries_do_not_change_training_bn_and_slots(resnet_runs):
    on, off = resnet_runs
    names = checkpoint_tensors(os.path.join(on, "model.ckpt-3"))
    assert any(n.endswith("/ExponentialMovingAverage") for n in names)
    assert any(n.endswith("moving_variance") for n in names)
    assert any(n.endswith("global_step") or n.endswith("Variable") for n in names)
    assert_checkpoints_bit_equal(os.path.join(on, "model.ckpt-3"), os.path.join(off, "model.ckpt-3"))
    ev = event_values(on)
    assert sorted(ev) == [1, 2, 3]
    grads = [t for t in ev[3] if t.endswith("/gradients")]
    assert grads and all(t[:-len("/gradients")] in ev[3] for t in grads)
    assert any("batch_normalization" in t for t in grads)
    assert "images/image/0" in ev[3] and "images/image/1" in ev[3]
