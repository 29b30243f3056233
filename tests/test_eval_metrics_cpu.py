"""StreamingMetrics on the CPU (the torch form of csrc/kernels/metrics.hip) against the numpy oracle, the evaluator's
unchanged numbers and new outputs, and merge() over gloo."""
import json
import math
import os

import numpy as np
import pytest
import torch

import eval_metrics_cases as cases
from distributed_tensorflow_models_amd.ops import elementwise as E
from distributed_tensorflow_models_amd.ops.metrics import StreamingMetrics
from test_distributed import run_workers

ROWS = 40


def _run(x, t, k, batch, confusion=True):
    m = StreamingMetrics(x.shape[1], k=k, confusion=confusion)
    for s in range(0, x.shape[0], batch):
        m.update(x[s:s + batch], t[s:s + batch])
    return m.fetch()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 10, 65])
def test_cpu_path_matches_oracle(C, dtype):
    x, t, _ = cases.pool(C, dtype, ROWS)
    for k in cases.ks(C):
        got = _run(x, t, k, x.shape[0])
        cases.check(got, cases.oracle(C, dtype, ROWS, k), x, t)
        assert got["skipped"] == 2 and got["nonfinite"] == (4 if C == 1 else 6)
    # the random rows alone: a bound not swamped by the 3e38 rows
    n_adv = cases.pool(C, dtype, ROWS)[2]
    cases.check(_run(x[n_adv:], t[n_adv:], 1, 7), cases.oracle(C, dtype, ROWS, 1, n_adv), x[n_adv:], t[n_adv:])


def test_counters_do_not_depend_on_the_batching():
    x, t, _ = cases.pool(10, torch.float32, ROWS)
    whole = _run(x, t.int(), 5, x.shape[0])
    for batch in (1, 3):
        part = _run(x, t, 5, batch)
        for n in cases.INT_KEYS:
            assert part[n] == whole[n], n
        for n in cases.ARRAY_KEYS + ("confusion",):
            assert np.array_equal(part[n], whole[n]), n


@pytest.mark.parametrize("C", [2, 10, 65])
def test_top1_topk_equal_in_top_k(C):
    x, t, _ = cases.pool(C, torch.float32, ROWS)
    for k in cases.ks(C):
        got = _run(x, t, k, 16, confusion=False)
        assert got["top1"] == int(E.in_top_k(x, t, 1).sum())
        assert got["topk"] == int(E.in_top_k(x, t, k).sum())


def test_argmax_differs_from_top1_on_a_tie():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0]])
    got = _run(x, torch.tensor([2]), 1, 1)
    assert got["top1"] == 1 and got["argmax_correct"] == 0
    assert got["predicted"].tolist() == [0, 1, 0, 0] and got["confusion"][2, 1] == 1
    assert got["precision_at_1"] == 1.0 and got["accuracy"] == 0.0


def test_fetch_without_updates_and_derived_values():
    m = StreamingMetrics(4, k=2, confusion=True)
    z = m.fetch()
    assert all(z[n] == 0 for n in cases.INT_KEYS) and z["loss_sum"] == 0.0 and math.isnan(z["mean_loss"])
    assert math.isnan(z["mean_per_class_accuracy"]) and not z["confusion"].any()
    m.update(torch.tensor([[0.0, 1.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 5.0]]),
             torch.tensor([1, 1, 3], dtype=torch.int32))
    r = m.fetch()
    assert r["support"].tolist() == [0, 2, 0, 1] and r["top1_correct"].tolist() == [0, 1, 0, 1]
    assert np.isnan(r["per_class_accuracy"][[0, 2]]).all() and r["per_class_accuracy"][1] == 0.5
    assert r["mean_per_class_accuracy"] == 0.75 and r["mean_loss"] == r["loss_sum"] / 3
    m.reset()
    assert m.fetch()["examples"] == 0


def test_limits_are_value_errors():
    with pytest.raises(ValueError):
        StreamingMetrics(65537)
    with pytest.raises(ValueError):
        StreamingMetrics(4097, confusion=True)
    with pytest.raises(ValueError):
        StreamingMetrics(4, k=5)
    with pytest.raises(ValueError):
        StreamingMetrics(4, k=0)
    with pytest.raises(ValueError):
        StreamingMetrics(4).update(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))


# ---- evaluator ---------------------------------------------------------------------------------------------------
BATCH, EXAMPLES = 16, 40  # 3 batches


@pytest.fixture(scope="module")
def lenet_ckpt(tmp_path_factory):
    from distributed_tensorflow_models_amd import trainer
    from distributed_tensorflow_models_amd.ckpt.saver import Saver, TFVar
    from distributed_tensorflow_models_amd.models.layers import tf_variables
    d = str(tmp_path_factory.mktemp("lenet_train"))
    torch.manual_seed(3)
    model = trainer.build_model_for_eval("lenet")
    Saver([TFVar(n, t, layout) for n, t, layout, _ in tf_variables(model)]).save(os.path.join(d, "model.ckpt"), 7)
    return d


def _evaluate(ckpt, eval_dir, capsys, **extra):
    from distributed_tensorflow_models_amd import evaluator
    from distributed_tensorflow_models_amd.compat import flags
    evaluator.define_eval_flags(flags, "lenet")
    F = flags.FLAGS
    F.checkpoint_dir, F.eval_dir, F.run_once, F.synthetic_data = ckpt, str(eval_dir), True, True
    F.batch_size, F.num_examples = BATCH, EXAMPLES
    for n, v in extra.items():
        setattr(F, n, v)
    capsys.readouterr()
    results = evaluator.evaluate("lenet", flags)
    return results, capsys.readouterr().out


def _old_counting(ckpt):
    """eval_once as it was before StreamingMetrics: two in_top_k sums per batch."""
    from distributed_tensorflow_models_amd import evaluator, trainer
    from distributed_tensorflow_models_amd.data.synthetic import SyntheticImages
    model = trainer.build_model_for_eval("lenet")
    model.eval()
    evaluator.restore_for_eval(model, os.path.join(ckpt, "model.ckpt-7"), False)
    data = SyntheticImages(BATCH, 28, 28, 1, 10, "cpu", seed=1234)
    num_iter = int(math.ceil(EXAMPLES / float(BATCH)))
    c1 = c5 = 0
    with torch.no_grad():
        for _ in range(num_iter):
            x, y = data.next_batch()
            out = model(x, training=False)
            c1 += int(E.in_top_k(out, y, 1).sum())
            c5 += int(E.in_top_k(out, y, 5).sum())
    return c1 / (num_iter * BATCH), c5 / (num_iter * BATCH)


def _scalars(eval_dir):
    from distributed_tensorflow_models_amd.utils.tb import read_events
    out = {}
    for f in sorted(os.listdir(eval_dir)):
        if f.startswith("events.out.tfevents"):
            for ev in read_events(os.path.join(eval_dir, f)):
                for v in ev.get("values", []):
                    out.setdefault(v["tag"], []).append((ev["step"], v))
    return out


def test_evaluator_without_new_flags_is_unchanged(lenet_ckpt, tmp_path, capsys):
    results, out = _evaluate(lenet_ckpt, tmp_path / "eval", capsys)
    p1, r5 = _old_counting(lenet_ckpt)
    assert results == [(7, p1, r5)]
    lines = out.splitlines()
    assert len(lines) == 1 and lines[0].endswith(": precision @ 1 = %.3f, global_step: %d" % (p1, 7)), out
    sc = _scalars(tmp_path / "eval")
    assert list(sc) == ["Precision @ 1"] and len(sc["Precision @ 1"]) == 1
    step, v = sc["Precision @ 1"][0]
    assert step == 7 and v["simple_value"] == np.float32(p1)
    assert sorted(f.split(".")[0] for f in os.listdir(tmp_path / "eval")) == ["events"]


def test_evaluator_with_every_flag(lenet_ckpt, tmp_path, capsys):
    ed = tmp_path / "eval"
    jl = tmp_path / "m" / "eval.jsonl"
    results, out = _evaluate(lenet_ckpt, ed, capsys, eval_loss=True, eval_per_class=True, eval_confusion=True,
                             metrics_file=str(jl))
    p1, r5 = _old_counting(lenet_ckpt)
    assert results == [(7, p1, r5)]
    lines = out.splitlines()
    assert len(lines) == 2 and lines[0].endswith(": precision @ 1 = %.3f, global_step: %d" % (p1, 7))
    doc = json.load(open(ed / "metrics-7.json"))
    assert ": eval loss = %.4f" % doc["mean_loss"] in lines[1]
    conf = np.load(ed / "confusion-7.npy")
    assert conf.shape == (10, 10) and conf.dtype == np.int64
    assert doc["examples"] == 48 and doc["nonfinite"] == 0 and doc["top1"] == round(p1 * 48)
    assert conf.sum() == doc["loss_rows"] == 48
    assert (conf.sum(1) == np.array(doc["support"])).all()  # (+ the non-finite rows per class: none here)
    assert np.trace(conf) == doc["argmax_correct"]
    assert (conf.sum(0) == np.array(doc["predicted"])).all()
    sc = _scalars(ed)
    assert set(sc) == {"Precision @ 1", "Loss", "Mean per-class accuracy", "Confusion matrix"}
    assert sc["Loss"][0][1]["simple_value"] == np.float32(doc["mean_loss"])
    assert sc["Mean per-class accuracy"][0][1]["simple_value"] == np.float32(doc["mean_per_class_accuracy"])
    im = sc["Confusion matrix"][0][1]["image"]
    assert (im["height"], im["width"], im["colorspace"]) == (10, 10, 1)
    rec = [json.loads(l) for l in open(jl)]
    assert len(rec) == 1 and rec[0]["global_step"] == 7 and rec[0]["eval_precision_at_1"] == p1
    assert rec[0]["mean_loss"] == doc["mean_loss"]


def test_confusion_rows_with_nonfinite_logits():
    """confusion.sum(1) + (rows not finite, per class) == support; trace == argmax_correct."""
    x, t, _ = cases.pool(10, torch.float32, ROWS)
    got = _run(x, t, 5, 9)
    valid = (t >= 0) & (t < 10)
    bad = valid & ~torch.isfinite(x).all(1)
    per_class = np.bincount(t[bad].numpy(), minlength=10)
    assert bad.sum() == got["nonfinite"] > 0
    assert np.array_equal(got["confusion"].sum(1) + per_class, got["support"])
    assert got["confusion"].sum() == got["loss_rows"] and np.trace(got["confusion"]) == got["argmax_correct"]


def test_nonfinite_logits_are_reported_once(lenet_ckpt, tmp_path, capsys, monkeypatch):
    from distributed_tensorflow_models_amd import evaluator
    seen = []
    monkeypatch.setattr(evaluator.logging, "warning", lambda msg, *a: seen.append(msg % a))
    real = evaluator.StreamingMetrics.update

    def poisoned(self, logits, labels):
        logits = logits.clone()
        logits[0, 0] = float("nan")
        return real(self, logits, labels)

    monkeypatch.setattr(evaluator.StreamingMetrics, "update", poisoned)
    _, out = _evaluate(lenet_ckpt, tmp_path / "eval", capsys)
    assert len(out.splitlines()) == 1 and len(seen) == 1 and "3 of 48 examples" in seen[0]


# ---- merge -------------------------------------------------------------------------------------------------------
def _merge_worker(rank, world):
    x, t, _ = cases.pool(10, torch.float32, ROWS)
    half = x.shape[0] // 2 + 1
    sl = slice(0, half) if rank == 0 else slice(half, None)
    m = StreamingMetrics(10, k=5, confusion=True)
    m.update(x[sl], t[sl])
    m.merge(None)
    return m._rec.clone()


def test_merge_two_ranks_gloo():
    recs = run_workers(_merge_worker, 2)
    assert recs[0].numpy().tobytes() == recs[1].numpy().tobytes()
    x, t, _ = cases.pool(10, torch.float32, ROWS)
    m = StreamingMetrics(10, k=5, confusion=True)
    m.update(x, t)
    m._rec.copy_(recs[0])
    got, single = m.fetch(), _run(x, t, 5, x.shape[0])
    for n in cases.INT_KEYS:
        assert got[n] == single[n], n
    for n in cases.ARRAY_KEYS + ("confusion",):
        assert np.array_equal(got[n], single[n]), n
    cases.check(got, cases.oracle(10, torch.float32, ROWS, 5), x, t)
