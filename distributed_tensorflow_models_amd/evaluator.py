"""Checkpoint-polling evaluator behind every reference eval script.

Reference behaviour kept: poll ``checkpoint_dir`` every ``eval_interval_secs``, restore the newest
checkpoint (EMA shadows for trainable variables when the trainer keeps them - cnn/cifar10_eval.py:
128-135, inception/inception_eval.py:157-160), run ``ceil(num_examples / batch_size)`` batches,
print ``precision @ 1`` (+ ``recall @ 5`` for ImageNet, inception_eval.py:105-127) and write a TF
event summary to ``eval_dir``.  Reference defects fixed: the checkpoint state is re-read on every
poll (C56/C57 read it once), ResNet eval runs in inference mode (C58 used is_training=True), a
checkpoint already evaluated is not re-evaluated.
"""
import json
import math
import os
import shutil
import time
from datetime import datetime

import numpy as np
import torch

from . import trainer
from .ckpt.saver import Saver, TFVar, get_checkpoint_state, step_from_path
from .models.layers import tf_variables
from .compat import logging
from .ops.metrics import StreamingMetrics
from .utils.metrics import JsonlMetrics
from .utils.tb import SummaryWriter

EVAL_DEFAULTS = {
    # preset: (eval_dir, checkpoint_dir, interval, num_examples, use_ema, top5)
    "cnn": ("/home/ubuntu/cifar10/eval", "/home/ubuntu/cifar10/train", 60, 10000, True, False),
    "alexnet": ("/home/ubuntu/cifar10/eval", "/home/ubuntu/cifar10/train", 60, 1000, False, False),
    "vgg": ("/home/ubuntu/cifar10/eval", "/home/ubuntu/cifar10_train", 60, 1000, False, False),
    "vgg_asp": ("/home/ubuntu/cifar10/eval", "/home/ubuntu/cifar10_train", 60, 1000, False, False),
    "resnet": ("/home/ubuntu/cifar10/eval", "/home/ubuntu/cifar10/train", 60, 1000, False, False),
    "cifarnet": ("/home/ubuntu/cifar10/eval", "/home/ubuntu/cifar10/train", 60, 1000, False, False),
    "inception": ("/home/ubuntu/imagenet/eval", "/home/ubuntu/imagenet/train/", 300, 200, True, True),
    "resnet50": ("/tmp/resnet50_eval", "/tmp/resnet50_train", 300, 1000, False, True),
    "mobilenet_v1": ("/tmp/mobilenet_v1_eval", "/tmp/mobilenet_v1_train", 300, 50000, False, True),
    "lenet": ("/tmp/lenet_eval", "/tmp/lenet_train", 60, 1000, False, False),
}


def define_eval_flags(flags, preset):
    d = EVAL_DEFAULTS[preset]
    p = trainer.PRESETS[preset]
    F = flags.FLAGS
    for name, fn, default, h in (
            ("eval_dir", flags.DEFINE_string, d[0], "Directory where to write event logs."),
            ("eval_data", flags.DEFINE_string, "test", "Either 'test' or 'train_eval'."),
            ("subset", flags.DEFINE_string, "validation", "Either 'validation' or 'train' (ImageNet)."),
            ("checkpoint_dir", flags.DEFINE_string, d[1], "Directory where to read model checkpoints."),
            ("eval_interval_secs", flags.DEFINE_integer, d[2], "How often to run the eval."),
            ("num_examples", flags.DEFINE_integer, d[3], "Number of examples to run."),
            ("run_once", flags.DEFINE_boolean, False, "Whether to run eval only once."),
            ("batch_size", flags.DEFINE_integer, p["batch_size"], "Number of images to process in a batch."),
            ("data_dir", flags.DEFINE_string, p["data_dir"], "Path to the data directory."),
            ("resnet_size", flags.DEFINE_integer, 32, "The size of the ResNet model to use."),
            ("use_ema", flags.DEFINE_boolean, d[4], "restore ExponentialMovingAverage shadows"),
            ("synthetic_data", flags.DEFINE_boolean, False, "evaluate on synthetic batches"),
            ("max_evals", flags.DEFINE_integer, 0, "stop after N evaluations (0 = forever)"),
            ("eval_loss", flags.DEFINE_boolean, False, "print and write the mean cross-entropy of the evaluation"),
            ("eval_per_class", flags.DEFINE_boolean, False,
             "write the mean per-class accuracy and metrics-<step>.json (all scalars and per-class arrays)"),
            ("eval_confusion", flags.DEFINE_boolean, False,
             "write confusion-<step>.npy and a 'Confusion matrix' image summary"),
            ("metrics_file", flags.DEFINE_string, "", "JSONL metrics path: one line per evaluation"),
    ):
        fn(name, default, h)
        F.reset(name)


def restore_for_eval(model, path, use_ema, prefix=""):
    """With ``use_ema`` every variable that has a shadow (trainables and BN moving statistics, as
    tf.train.ExponentialMovingAverage.variables_to_restore maps them; reference
    cnn/cifar10_eval.py:132-135, inception/inception_eval.py:157-160) is restored from
    ``<v>/ExponentialMovingAverage``; everything else by name.  ``prefix``: the trainer's variable
    scope (the reference evals rebuild the net under it: alexnet/cifar10_alexnet_eval.py:125,
    resnet/cifar10_resnet_eval.py:107); partitioned (sliced) checkpoint entries are reassembled."""
    from .ckpt.bundle import BundleReader
    names = set(BundleReader(path).names()) if use_ema else set()
    vs = []
    for name, t, layout, trainable in tf_variables(model):
        name = prefix + name
        shadow = name + "/ExponentialMovingAverage"
        vs.append(TFVar(shadow if (use_ema and shadow in names) else name, t, layout))
    Saver(vs).restore(path)
    from .ops.nn import invalidate_weight_copies
    invalidate_weight_copies(model.parameters())


def _inputs(preset, flags, device):
    F = flags.FLAGS
    cfg = trainer.PRESETS[preset]
    S = cfg["image_size"]
    if cfg["dataset"] == "cifar10" and not F.synthetic_data:
        from .data import cifar10
        return cifar10.inputs(F.eval_data == "test", F.data_dir, F.batch_size, S, device=device)
    if cfg["dataset"] == "imagenet" and not F.synthetic_data:
        from .data import imagenet
        if torch.device(device).type == "cuda":
            from .data import imagenet_gpu
            return imagenet_gpu.inputs(imagenet.ImagenetData(F.subset, F.data_dir), F.batch_size, image_size=S,
                                       device=device)
        return imagenet.inputs(imagenet.ImagenetData(F.subset, F.data_dir), F.batch_size, image_size=S,
                               device=device)
    from .data.synthetic import SyntheticImages
    return SyntheticImages(F.batch_size, S, S, 1 if cfg["dataset"] == "synthetic_mnist" else 3,
                           cfg["num_classes"], device, seed=1234)


@torch.no_grad()
def _eval_once(model, data, num_examples, batch_size, metrics=None, confusion=False):
    """``ceil(num_examples / batch_size)`` batches added to a StreamingMetrics record on the device and read ONCE
    at the end (no host round trip per batch).  Returns (p1, r5, the fetched record)."""
    num_iter = int(math.ceil(num_examples / float(batch_size)))
    if metrics is not None:
        metrics.reset()
    for _ in range(num_iter):
        x, y = data.next_batch()
        out = model(x, training=False)
        if isinstance(out, tuple):
            out = out[0]
        if out.dtype not in (torch.float32, torch.bfloat16):
            out = out.float()
        if y.dtype not in (torch.int32, torch.int64):
            y = y.long()
        if metrics is None:
            C = out.shape[-1]
            metrics = StreamingMetrics(C, k=min(5, C), confusion=confusion, device=out.device)
        # tf.nn.in_top_k (ties at the boundary count as correct), HIP kernel on the GPU
        metrics.update(out, y)
    res = metrics.fetch()
    total = num_iter * batch_size
    return res["top1"] / total, res["topk"] / total, res


def eval_once(model, data, num_examples, batch_size, top5=False, metrics=None):
    """(precision @ 1, recall @ 5) over ``num_iter * batch_size`` examples.  ``metrics``: a StreamingMetrics to use
    (reset first; its ``k`` is the k of the second value) - fetch it afterwards for the loss, the per-class counts
    and the confusion matrix of the same pass; None: one with k = min(5, classes) is made."""
    p1, r5, _ = _eval_once(model, data, num_examples, batch_size, metrics)
    return p1, r5


def _confusion_image(conf):
    """[C, C] counts -> uint8 [C, C, 1], every row scaled to 0-255 by its own sum (an empty row stays black)."""
    rows = conf.sum(1, keepdims=True).astype(np.float64)
    img = np.where(rows > 0, conf / np.maximum(rows, 1.0), 0.0)
    return np.rint(img * 255.0).astype(np.uint8)[:, :, None]


def _write_extras(F, writer, jsonl, res, gs, p1, r5):
    """What the --eval_* flags and --metrics_file add to one evaluation."""
    if res["nonfinite"]:
        logging.warning("evaluation at step %d: %d of %d examples have non-finite logits (left out of the loss and "
                        "of the argmax counts)", gs, res["nonfinite"], res["examples"])
    # (a ratio over nothing is NaN, which JSON cannot hold: null)
    scalars = {n: None if res[n] != res[n] else res[n]
               for n in ("examples", "skipped", "nonfinite", "loss_rows", "top1", "topk", "k", "argmax_correct",
                         "loss_sum", "mean_loss", "precision_at_1", "recall_at_k", "accuracy",
                         "mean_per_class_accuracy")}
    if F.eval_loss:
        print("%s: eval loss = %.4f" % (datetime.now(), res["mean_loss"]), flush=True)
        writer.add_scalar("Loss", res["mean_loss"], gs)
    if F.eval_per_class:
        writer.add_scalar("Mean per-class accuracy", res["mean_per_class_accuracy"], gs)
        doc = dict(scalars, global_step=gs)
        for n in ("support", "top1_correct", "predicted"):
            doc[n] = res[n].tolist()
        doc["per_class_accuracy"] = [None if v != v else v for v in res["per_class_accuracy"].tolist()]
        with open(os.path.join(F.eval_dir, "metrics-%d.json" % gs), "w") as f:
            json.dump(doc, f)
    if F.eval_confusion:
        np.save(os.path.join(F.eval_dir, "confusion-%d.npy" % gs), res["confusion"])
        if res["confusion"].shape[0] <= 512:  # larger matrices are saved, not drawn
            writer.add_image("Confusion matrix", _confusion_image(res["confusion"]), gs)
    # (eval_*: the printed values, over num_iter * batch_size; precision_at_1 / recall_at_k: over the valid rows)
    jsonl.write(global_step=gs, eval_precision_at_1=p1, eval_recall_at_5=r5, **scalars)


def evaluate(preset, flags):
    F = flags.FLAGS
    cfg = trainer.PRESETS[preset]
    top5 = EVAL_DEFAULTS[preset][5]
    device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    kw = {"resnet_size": F.resnet_size} if cfg["model"] == "cifar10_resnet_v2" else {}
    if cfg["model"].startswith("mobilenet") and "depth_multiplier" in F and F.depth_multiplier != 1.0:
        kw["depth_multiplier"] = F.depth_multiplier
    if "quantize" in F and F.quantize:  # create_eval_graph (mobilenet_v1_eval.py:126-127)
        from .compat.quantize import QuantConfig
        kw["quantize"] = QuantConfig(is_training=False, fused=bool("quant_fused" in F and F.quant_fused))
    model = trainer.build_model_for_eval(preset, **kw).to(device)
    model.eval()
    if os.path.isdir(F.eval_dir):
        shutil.rmtree(F.eval_dir)
    os.makedirs(F.eval_dir, exist_ok=True)
    writer = SummaryWriter(F.eval_dir)
    data = _inputs(preset, flags, device)
    extras = F.eval_loss or F.eval_per_class or F.eval_confusion or bool(F.metrics_file)
    jsonl = JsonlMetrics(F.metrics_file or None)
    last = None
    n_evals = 0
    results = []
    while True:
        st = get_checkpoint_state(F.checkpoint_dir)  # re-read every poll
        path = st.model_checkpoint_path if st else None
        if not path:
            print("No checkpoint file found", flush=True)
        elif path != last:
            restore_for_eval(model, path, F.use_ema, prefix=cfg.get("scope_prefix", ""))
            gs = step_from_path(path)
            t0 = time.time()
            p1, r5, res = _eval_once(model, data, F.num_examples, F.batch_size, confusion=F.eval_confusion)
            dt = time.time() - t0
            if top5:
                print("%s: precision @ 1 = %.4f recall @ 5 = %.4f [%d examples] (%.1f examples/sec)"
                      % (datetime.now(), p1, r5, F.num_examples, F.num_examples / max(dt, 1e-9)), flush=True)
                writer.add_scalar("Recall @ 5", r5, gs)
            else:
                print("%s: precision @ 1 = %.3f, global_step: %d" % (datetime.now(), p1, gs), flush=True)
            writer.add_scalar("Precision @ 1", p1, gs)
            if extras or res["nonfinite"]:
                _write_extras(F, writer, jsonl, res, gs, p1, r5)
            results.append((gs, p1, r5))
            last = path
            n_evals += 1
        if F.run_once or (F.max_evals and n_evals >= F.max_evals):
            break
        time.sleep(F.eval_interval_secs)
    writer.close()
    jsonl.close()
    return results
