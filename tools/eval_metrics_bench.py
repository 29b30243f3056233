#!/usr/bin/env python3
"""Cost of the evaluation metrics, per batch and in a whole eval_once, with the method of tools/adam_bench.py.

Per batch, on logits [256, 1000] bf16 and [512, 10] fp32 (random, int64 labels):
  (a) one StreamingMetrics.update (two launches, no host read; confusion matrix on);
  (b) what eval_once did before StreamingMetrics: two in_top_k launches, each followed by .sum() and int(), i.e. two
      reductions and two host round trips;
  (c) the same quantities as (a) with torch ops on the device (top-1 / top-k counts, argmax, cross-entropy sum,
      bincount support / predicted / confusion), accumulated on the device, no host read.
Each sample is the host wall time of ``--reps`` back-to-back calls ended by one device synchronise (a launch returns
before its kernel ends, and (b) waits on the host by itself), per call; the variants alternate within a round and the
figure is the median over the rounds.  For (a) the device time between two events is given as well.

Whole eval_once on synthetic data, examples/sec: ResNet-50 at 224x224, batch 256, 20 batches, and LeNet, batch 512,
200 batches; eval_once of this tree against the earlier loop (copied below as ``eval_once_in_top_k``), ``--runs``
alternating runs each, min and max.  Prints one JSON line per section.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _sample_ms  # noqa: E402


def _wall_ms(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _alternate(fns, rounds, reps, warmup, sample):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(sample(fn, reps))
    out = {}
    for k, v in times.items():
        v.sort()
        out[k] = dict(median=round(v[len(v) // 2], 5), min=round(v[0], 5), max=round(v[-1], 5))
    return out


def eval_once_in_top_k(model, data, num_examples, batch_size):
    """eval_once as it was before StreamingMetrics (two host reads per batch)."""
    import torch

    from distributed_tensorflow_models_amd.ops import elementwise as E
    num_iter = int(math.ceil(num_examples / float(batch_size)))
    c1 = c5 = 0
    with torch.no_grad():
        for _ in range(num_iter):
            x, y = data.next_batch()
            out = model(x, training=False)
            if isinstance(out, tuple):
                out = out[0]
            c1 += int(E.in_top_k(out, y, 1).sum())
            c5 += int(E.in_top_k(out, y, min(5, out.shape[-1])).sum())
    total = num_iter * batch_size
    return c1 / total, c5 / total


def per_batch(B, C, dtype, args):
    import torch

    from distributed_tensorflow_models_amd.ops import elementwise as E
    from distributed_tensorflow_models_amd.ops.metrics import StreamingMetrics
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(B * 131 + C)
    x = (torch.randn(B, C, generator=g) * 3).to(device=dev, dtype=dtype)
    t = torch.randint(0, C, (B,), generator=g).to(dev)
    k = min(5, C)
    sm = StreamingMetrics(C, k=k, confusion=True, device=dev)
    acc = dict(top1=torch.zeros((), dtype=torch.int64, device=dev), topk=torch.zeros((), dtype=torch.int64, device=dev),
               argmax=torch.zeros((), dtype=torch.int64, device=dev),
               loss=torch.zeros((), dtype=torch.float64, device=dev),
               support=torch.zeros(C, dtype=torch.int64, device=dev),
               predicted=torch.zeros(C, dtype=torch.int64, device=dev),
               confusion=torch.zeros(C * C, dtype=torch.int64, device=dev))

    def a_update():
        sm.update(x, t)

    def b_in_top_k():
        return int(E.in_top_k(x, t, 1).sum()), int(E.in_top_k(x, t, k).sum())

    def c_torch():
        xf = x.float()
        xt = xf.gather(1, t[:, None])
        greater = (xf > xt).sum(1)
        fin = torch.isfinite(xt[:, 0])
        acc["top1"] += (fin & (greater < 1)).sum()
        acc["topk"] += (fin & (greater < k)).sum()
        pred = xf.argmax(1)
        acc["argmax"] += (pred == t).sum()
        acc["loss"] += (torch.logsumexp(xf, 1) - xt[:, 0]).double().sum()
        acc["support"] += torch.bincount(t, minlength=C)
        acc["predicted"] += torch.bincount(pred, minlength=C)
        acc["confusion"] += torch.bincount(t * C + pred, minlength=C * C)

    # the three count the same thing on this batch
    a_update()
    c_torch()
    got = sm.fetch()
    assert (got["top1"], got["topk"]) == b_in_top_k() == (int(acc["top1"]), int(acc["topk"]))
    assert got["argmax_correct"] == int(acc["argmax"]) and abs(got["loss_sum"] - float(acc["loss"])) < 1e-3 * B
    assert (got["confusion"].reshape(-1) == acc["confusion"].cpu().numpy()).all()

    fns = {"a_update": a_update, "b_two_in_top_k_with_host_reads": b_in_top_k, "c_torch_ops": c_torch}
    res = _alternate(fns, args.rounds, args.reps, args.warmup, _wall_ms)
    dev_a = _alternate({"a_update": a_update}, args.rounds, args.reps, 1, _sample_ms)["a_update"]
    out = dict(section="per_batch", B=B, C=C, dtype=str(dtype).split(".")[-1], rounds=args.rounds, reps=args.reps,
               unit="ms per call (host wall, synchronised once per sample)", a_update_device_events_ms=dev_a)
    out.update(res)
    out["b_over_a"] = round(res["b_two_in_top_k_with_host_reads"]["median"] / res["a_update"]["median"], 2)
    out["c_over_a"] = round(res["c_torch_ops"]["median"] / res["a_update"]["median"], 2)
    print(json.dumps(out), flush=True)


def whole(name, model_name, batch, batches, size, channels, classes, args):
    import torch

    from distributed_tensorflow_models_amd import evaluator
    from distributed_tensorflow_models_amd.data.synthetic import SyntheticImages
    from distributed_tensorflow_models_amd.models import nets_factory
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = nets_factory.build(model_name, num_classes=classes).to(dev)
    model.eval()
    data = SyntheticImages(batch, size, size, channels, classes, dev, seed=1234)
    n = batch * batches
    fns = {"this_tree": lambda: evaluator.eval_once(model, data, n, batch),
           "in_top_k_loop": lambda: eval_once_in_top_k(model, data, n, batch)}
    vals = {k: fn() for k, fn in fns.items()}  # warm-up; the two return the same numbers
    assert vals["this_tree"] == vals["in_top_k_loop"], vals
    eps = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            eps[k].append(n / (time.perf_counter() - t0))
    out = dict(section="eval_once", model=name, batch=batch, batches=batches, runs=args.runs, unit="examples/sec",
               p1_r5=vals["this_tree"])
    for k, v in eps.items():
        out[k] = dict(min=round(min(v), 1), max=round(max(v), 1), runs=[round(e, 1) for e in v])
    out["not_slower"] = bool(max(eps["this_tree"]) >= min(eps["in_top_k_loop"]))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5, help="alternating eval_once runs per variant")
    ap.add_argument("--skip-models", action="store_true")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "eval_metrics_bench needs a GPU"
    per_batch(256, 1000, torch.bfloat16, args)
    per_batch(512, 10, torch.float32, args)
    if not args.skip_models:
        whole("resnet_v1_50 224x224", "resnet_v1_50", 256, 20, 224, 3, 1000, args)
        whole("lenet 28x28", "lenet", 512, 200, 28, 1, 10, args)


if __name__ == "__main__":
    main()
