"""Generic distributed trainer behind every reference entry script.

One process per MI355X.  ``train(preset, FLAGS)`` reproduces the reference trainer skeleton with
MI355X-native machinery underneath:
  parse flags -> (ps: no-op join) -> process group (torchrun env or --ps_hosts/--worker_hosts)
  -> model (TF names) -> input pipeline -> loss/optimizer/schedule (TF semantics)
  -> BSP (bucketed RCCL all-reduce) | ASP (owner-sharded store) | SSP (store + staleness clock)
  -> Supervisor (chief restore-or-init, periodic TF-layout checkpoints) -> step loop with the
  reference per-step log line, NaN guard, optional traces and JSONL metrics.
Deliberate fixes of reference defects: train_dir is NOT wiped unless --fresh,
BN moving statistics are always updated, chief-only duties stay on rank 0, VGG saves checkpoints.
"""
import math
import os
import shutil
import time

import numpy as np
import torch

from .ckpt.saver import AdamPowerVar, MaskVar, Saver, TFVar, ThresholdVar, model_variables
from .compat import logging
from .compat.train import ExponentialDecay, LinearWarmup, PolynomialDecay, Server
from .engine import TrainStep
from .models import nets_factory
from .parallel import process_group as pg
from .utils.heartbeat import Heartbeat
from .utils.metrics import JsonlMetrics, StepTimer, format_step
from .utils.profiler import StepTracer

CIFAR_TRAIN = 50000
IMAGENET_TRAIN = 1281167

# reference hyper-parameters per trainer (constants quoted from the reference trainer files)
PRESETS = {
    # cnn/cifar10_cnn_bsp.py:9-13,46-64 + cnn/cifar10.py:54-81
    "cnn": dict(model="cifar10_cnn", num_classes=10, dataset="cifar10", image_size=24, batch_size=512, lr=0.32,
                lr_scale_workers=False, decay_epochs=350.0, decay_factor=0.1, optimizer="sgd", ema=0.9999,
                wd_all=None, max_steps=20000, save_secs=60, log_style="cnn", max_to_keep=5,
                global_step_name="Variable",
                train_dir="/home/ubuntu/cifar10/train", data_dir="/home/ubuntu/cifar10/data"),
    # alexnet/cifar10_alexnet_bsp.py:18-30,54-94
    "alexnet": dict(model="alexnet_v2", num_classes=10, dataset="cifar10", image_size=32, batch_size=128, lr=0.01,
                    lr_scale_workers=True, decay_epochs=350.0, decay_factor=0.1, optimizer="sgd", ema=0.9999,
                    wd_all=2e-4, max_steps=2000000, save_secs=60, log_style="standard", max_to_keep=5,
                    scope_prefix="partitioned_space/", partitioned=True,
                    global_step_name="partitioned_space/Variable",
                    train_dir="/home/ubuntu/cifar10/train", data_dir="/home/ubuntu/cifar10/data"),
    # vgg/cifar10_vgg_bsp.py:19-30,57-95 (factory vgg_16, 10 classes, is_training=False -> no dropout)
    "vgg": dict(model="vgg_16", num_classes=10, dataset="cifar10", image_size=32, batch_size=72, lr=0.01,
                lr_scale_workers=True, decay_epochs=350.0, decay_factor=0.1, optimizer="sgd", ema=None,
                wd_all=2e-4, max_steps=20000, save_secs=60, log_style="standard", max_to_keep=5,
                model_kw=dict(fc_conv_padding="SAME", dropout_keep_prob=1.0, weight_decay=0.0),
                scope_prefix="root/", partitioned=True, global_step_name="root/Variable",
                train_dir="/home/ubuntu/cifar10_train", data_dir="/home/ubuntu/cifar10_data"),
    # vgg/cifar10_vgg_asp.py:20-31 + vgg/cifar10.py:338-391 (lr not scaled, var EMA)
    "vgg_asp": dict(model="vgg_16", num_classes=10, dataset="cifar10", image_size=32, batch_size=72, lr=0.01,
                    lr_scale_workers=False, decay_epochs=350.0, decay_factor=0.1, optimizer="sgd", ema=0.9999,
                    wd_all=2e-4, max_steps=20000, save_secs=60, log_style="standard", max_to_keep=5,
                    model_kw=dict(fc_conv_padding="SAME", dropout_keep_prob=1.0, weight_decay=0.0),
                    scope_prefix="root/", partitioned=True, global_step_name="root/Variable",
                    train_dir="/home/ubuntu/cifar10_train", data_dir="/home/ubuntu/cifar10_data"),
    # resnet/cifar10_resnet_bsp.py:19-29,57-106 (CIFAR ResNet v2, resnet_size 32)
    "resnet": dict(model="cifar10_resnet_v2", num_classes=10, dataset="cifar10", image_size=32, batch_size=128,
                   lr=0.08, lr_scale_workers=True, decay_epochs=32.0, decay_factor=0.1, optimizer="sgd",
                   ema=0.9999, wd_all=2e-3, max_steps=10000000, save_secs=60, log_style="short", max_to_keep=1,
                   # tf.layers.batch_normalization (resnet_model.py:45) keeps its moving statistics out of
                   # tf.moving_average_variables(): the EMA covers trainables only
                   ema_buffers=False,
                   train_accuracy_every=200, scope_prefix="root/", partitioned=True, global_step_name="Variable",
                   train_dir="/home/ubuntu/cifar10/train",
                   data_dir="/home/ubuntu/cifar10/data"),
    # cifarnet/cifar10_cifarnet_bsp.py:20-32,56-91
    "cifarnet": dict(model="cifarnet", num_classes=10, dataset="cifar10", image_size=32, batch_size=512, lr=0.1,
                     lr_scale_workers=True, decay_epochs=20.0, decay_factor=0.1, optimizer="sgd", ema=0.9999,
                     wd_all=2e-4, max_steps=2000000, save_secs=60, log_style="standard", max_to_keep=5,
                     scope_prefix="partitioned_space/", partitioned=True,
                     global_step_name="partitioned_space/Variable",
                     train_dir="/home/ubuntu/cifar10/train", data_dir="/home/ubuntu/cifar10/data"),
    # inception/imagenet_inception_bsp.py:54-72,104-157 (old-slim Inception-v3, RMSProp, label smoothing)
    "inception": dict(model="inception_v3_slim_old", num_classes=1001, dataset="imagenet", image_size=299,
                      batch_size=32, lr=0.045, lr_scale_workers=True, decay_epochs=2.0, decay_factor=0.94,
                      decay_div_workers=True, optimizer="rmsprop", rmsprop_decay=0.9, momentum=0.9,
                      rmsprop_epsilon=1.0, ema=0.9999, wd_all=None, label_smoothing=0.1, aux_weight=0.4,
                      max_steps=10000000, save_secs=600, log_style="short", max_to_keep=5, nan_guard=True,
                      train_dir="/home/ubuntu/imagenet/train/", data_dir="/home/ubuntu/imagenet/data/",
                      wipe=False, wgrad_stream=False),
    # vgg/nets/mobilenet_v1_train.py:57-160 (SGD 0.045, x0.94 every 2.5 epochs, batch 64)
    "mobilenet_v1": dict(model="mobilenet_v1", num_classes=1001, dataset="imagenet", image_size=224, batch_size=64,
                         lr=0.045, lr_scale_workers=False, decay_epochs=2.5, decay_factor=0.94, optimizer="sgd",
                         ema=None, wd_all=None, max_steps=10000000, save_secs=100,
                         log_style="short", max_to_keep=5, train_dir="/tmp/mobilenet_v1_train",
                         data_dir="/tmp/imagenet"),
    # headline benchmark model (north star) - slim resnet_v1_50 on synthetic ImageNet
    "resnet50": dict(model="resnet_v1_50", num_classes=1000, dataset="synthetic_imagenet", image_size=224,
                     batch_size=256, lr=0.1, lr_scale_workers=True, decay_epochs=30.0, decay_factor=0.1,
                     optimizer="momentum", momentum=0.9, ema=None, wd_all=None, max_steps=1000, save_secs=600,
                     log_style="standard", max_to_keep=5, train_dir="/tmp/resnet50_train", data_dir=""),
    # BASELINE config #1 plumbing: LeNet on synthetic MNIST
    "lenet": dict(model="lenet", num_classes=10, dataset="synthetic_mnist", image_size=28, batch_size=64, lr=0.01,
                  lr_scale_workers=True, decay_epochs=100.0, decay_factor=0.1, optimizer="sgd", ema=None,
                  wd_all=None, max_steps=200, save_secs=60, log_style="standard", max_to_keep=5,
                  train_dir="/tmp/lenet_train", data_dir=""),
}


LARGE_BATCH_BSP_ONLY = ("--optimizer lars and --clip_global_norm need --sync_mode bsp (got %s): under asp / ssp the "
                        "update runs on owner shards from one worker's push, where no global gradient norm exists")


ADAM_BSP_ONLY = ("--optimizer adam needs --sync_mode bsp (got %s): under asp / ssp the update runs on owner shards, "
                 "which would need a shared count of applied updates per shard for the bias correction")


LAMB_BSP_ONLY = ("--optimizer lamb needs --sync_mode bsp (got %s): under asp / ssp the update runs on owner shards, "
                 "which hold neither whole tensors for the trust ratio nor a shared count of applied updates")
LAMB_NO_CLIP = ("--optimizer lamb and --clip_global_norm are not combined: the global norm would have to leave the "
                "decoupled decay term out, which the norm pass does not form")


ACCUM_BSP_ONLY = ("--accum_steps > 1 needs --sync_mode bsp (got %s): under asp / ssp every push is applied by the "
                  "owner shards at once, so there is no step over which gradients could be summed")


MIX_BSP_ONLY = ("--mixup_alpha / --cutmix_alpha need --sync_mode bsp (got %s): the mixing plans are drawn per global "
                "step, which under asp / ssp is no property of a worker's own batch sequence")


DISTILL_BSP_ONLY = ("--distill_teacher needs --sync_mode bsp (got %s): under asp / ssp the step is the parameter "
                    "store's, which has no place for a second network's forward")


PRUNE_BSP_ONLY = ("--prune_sparsity needs --sync_mode bsp (got %s): the masks agree between replicas without "
                  "communication only because every rank holds the same weight bits, which asp / ssp do not give")


RANDAUGMENT_NEEDS_IMAGES = ("--randaugment_layers needs a dataset of uint8 images (cifar10, imagenet), got %s: the "
                            "synthetic batches are random floats with nothing to augment")


def randaugment_config(FLAGS, cfg):
    """The RandAugmentConfig of the --randaugment_* flags, or None with --randaugment_layers 0 (checked before any
    process group exists).  Input-side only, so it works under bsp, asp and ssp alike; the seed is --seed."""
    if not FLAGS.randaugment_layers:
        return None
    from .ops.randaugment import RandAugmentConfig
    ra = RandAugmentConfig(FLAGS.randaugment_layers, FLAGS.randaugment_magnitude, FLAGS.randaugment_prob,
                           FLAGS.randaugment_ops or None, FLAGS.randaugment_translate_ratio,
                           FLAGS.randaugment_cutout_ratio, seed=FLAGS.seed)
    ds = "synthetic_imagenet" if FLAGS.synthetic_data and cfg["dataset"] == "imagenet" else cfg["dataset"]
    if ds not in ("cifar10", "imagenet"):
        raise ValueError(RANDAUGMENT_NEEDS_IMAGES % ds)
    return ra


def prune_config(FLAGS, mode):
    """The PruneConfig of the --prune_* flags, or None with --prune_sparsity 0 (checked before any process group
    exists).  --prune_exclude is a regular expression searched in a variable's TF name."""
    if not FLAGS.prune_sparsity:
        return None
    if mode in ("asp", "ssp"):
        raise ValueError(PRUNE_BSP_ONLY % mode)
    import re
    from .ops.prune import PruneConfig
    select = None
    if FLAGS.prune_exclude:
        rx = re.compile(FLAGS.prune_exclude)
        select = lambda name, p: p.dim() >= 2 and not rx.search(getattr(p, "tf_name", None) or name)  # noqa: E731
    end = FLAGS.max_steps if FLAGS.prune_end_step < 0 else FLAGS.prune_end_step
    return PruneConfig(FLAGS.prune_sparsity, FLAGS.prune_initial_sparsity, FLAGS.prune_begin_step, end,
                       FLAGS.prune_frequency, FLAGS.prune_exponent, select)


SAM_BSP_ONLY = ("--sam_rho needs --sync_mode bsp (got %s): under asp / ssp the step is the parameter store's, which "
                "has no place for a second pass at perturbed weights")
SAM_NO_PRUNE = ("--sam_rho and --prune_sparsity are not combined: the perturbation would refill masked weights")
SAM_NO_QUANTIZE = ("--sam_rho and --quantize are not combined: the fake-quantised weights are derived outside the "
                   "compute copies that the perturbation maintains")


def sam_config(FLAGS, mode):
    """The SamConfig of --sam_rho / --sam_adaptive, or None with --sam_rho 0 (checked before any process group
    exists)."""
    import math
    rho = float(FLAGS.sam_rho)
    if not math.isfinite(rho) or rho < 0.0:
        raise ValueError("--sam_rho must be a finite number, at least 0, got %r" % (FLAGS.sam_rho,))
    if rho == 0.0:
        return None
    if mode in ("asp", "ssp"):
        raise ValueError(SAM_BSP_ONLY % mode)
    if FLAGS.prune_sparsity:
        raise ValueError(SAM_NO_PRUNE)
    if "quantize" in FLAGS and FLAGS.quantize:
        raise ValueError(SAM_NO_QUANTIZE)
    from .ops.sam import SamConfig
    return SamConfig(rho, bool(FLAGS.sam_adaptive))


COMPRESS_BSP_ONLY = ("--grad_compress_ratio needs --sync_mode bsp (got %s): under asp / ssp a worker pushes to the "
                     "parameter store, and a residual kept on the worker would be applied against weights it no "
                     "longer matches")
COMPRESS_NO_BF16 = ("--grad_compress_ratio and --grad_comm_dtype bf16 are not combined: a packet carries fp32 bit "
                    "patterns")
COMPRESS_NO_GRAPH = ("--grad_compress_ratio and --use_hipgraph are not combined: the dense warm-up is a host decision "
                     "per step")


def compress_config(FLAGS, mode):
    """The GradCompress of --grad_compress_ratio / --grad_compress_begin_step, or None with a ratio of 0 (checked
    before any process group exists)."""
    ratio = float(FLAGS.grad_compress_ratio)
    if ratio == 0.0:
        if FLAGS.grad_compress_begin_step:
            raise ValueError("--grad_compress_begin_step needs --grad_compress_ratio")
        return None
    if mode in ("asp", "ssp"):
        raise ValueError(COMPRESS_BSP_ONLY % mode)
    if FLAGS.grad_comm_dtype == "bf16":
        raise ValueError(COMPRESS_NO_BF16)
    if FLAGS.use_hipgraph:
        raise ValueError(COMPRESS_NO_GRAPH)
    from .ops.compress import GradCompress
    return GradCompress(ratio, FLAGS.grad_compress_begin_step)  # (its own checks: a ratio in (0, 1], a step >= 0)


def parse_model_kw(text):
    """"k=v,..." -> {k: int or float}: the numeric model keywords of --distill_teacher_kw."""
    out = {}
    for item in (t.strip() for t in text.split(",")):
        if not item:
            continue
        k, sep, v = item.partition("=")
        try:
            if not sep or not k.strip():
                raise ValueError(item)
            out[k.strip()] = int(v) if v.strip().lstrip("+-").isdigit() else float(v)
        except ValueError:
            raise ValueError("--distill_teacher_kw takes numeric k=v pairs, got %r" % item) from None
    return out


def distill_checkpoint_path(path):
    """The checkpoint prefix --distill_checkpoint names: a prefix itself, or a directory's newest checkpoint."""
    from .ckpt.saver import latest_checkpoint
    if path and os.path.isdir(path):
        path = latest_checkpoint(path) or ""
    if not path or not os.path.exists(path + ".index"):
        raise ValueError("--distill_teacher needs --distill_checkpoint, a checkpoint (or a directory holding one) of "
                         "the trained teacher; got %r" % (path,))
    return path


def define_common_flags(flags, preset):
    """Flags shared by every trainer (reference flag inventory) + MI355X extras."""
    p = PRESETS[preset]
    d = flags.DEFINE_string, flags.DEFINE_integer, flags.DEFINE_float, flags.DEFINE_boolean
    S, I, Fl, B = d
    for name, fn, default, h in (
            ("job_name", S, "", "One of 'ps', 'worker'"),
            ("ps_hosts", S, "", "Comma-separated list of hostname:port pairs"),
            ("worker_hosts", S, "", "Comma-separated list of hostname:port pairs"),
            ("task_id", I, 0, "Task id of the replica running the training."),
            ("batch_size", I, p["batch_size"], "Number of images to process in a batch."),
            ("data_dir", S, p["data_dir"], "Path to the data directory."),
            ("train_dir", S, p["train_dir"], "Directory where to write event logs and checkpoint."),
            ("max_steps", I, p["max_steps"], "Number of batches to run."),
            ("log_device_placement", B, preset == "cnn", "Whether to log device placement."),
            ("resnet_size", I, 32, "The size of the ResNet model to use."),
            ("protocol", S, "grpc", "accepted for compatibility; transport is RCCL/gloo"),
            ("save_interval_secs", I, p["save_secs"], "Save interval seconds."),
            ("save_every_steps", I, 0, "also checkpoint every N global steps (0 = time-based only)"),
            ("save_summaries_secs", I, 180, "train-side TensorBoard scalars at most this often (0 = off)"),
            ("save_summaries_steps", I, 0, "also write the train-side summaries whenever global_step % N == 0, "
             "on logged steps (0 = time-based only)"),
            ("summary_histograms", B, False, "histograms of every trainable variable and its gradient "
             "(<var>, <var>/gradients); the variables are read AFTER the step's update; gradients under BSP only"),
            ("summary_activations", B, False, "activation histograms and sparsity per end point "
             "(<end_point>/activations, <end_point>/sparsity): one extra no-grad forward per summary step"),
            ("summary_images", I, 0, "image summary (images/image/<i>) of the first N images of the input batch"),
            ("initial_learning_rate", Fl, p["lr"], "Initial learning rate."),
            ("num_epochs_per_decay", Fl, p["decay_epochs"], "Epochs after which learning rate decays."),
            ("learning_rate_decay_factor", Fl, p["decay_factor"], "Learning rate decay factor."),
            # large-batch training (all default to the preset's behaviour)
            ("optimizer", S, "", "sgd | momentum | rmsprop | lars | adam | lamb (default: the preset's optimizer); "
             "lars, adam and lamb are BSP only; lamb is Adam's direction with a per-tensor trust ratio |w|/|update| "
             "and uses the weight decay decoupled"),
            ("adam_beta1", Fl, 0.9, "Adam and LAMB: decay of the first-moment estimate"),
            ("adam_beta2", Fl, 0.999, "Adam and LAMB: decay of the second-moment estimate"),
            ("adam_epsilon", Fl, 1e-8, "Adam: epsilon added to sqrt(v)"),
            ("lamb_epsilon", Fl, 1e-6, "LAMB: epsilon added to the bias-corrected sqrt(v)"),
            ("lars_eeta", Fl, 0.001, "LARS trust coefficient"),
            ("lars_epsilon", Fl, 0.0, "LARS epsilon in the trust ratio's denominator"),
            ("clip_global_norm", Fl, 0.0, "clip the gradient by this global norm (0 = off); BSP only, not with lars "
             "or lamb"),
            ("warmup_steps", I, 0, "linear learning-rate warm-up from 0 over the first N steps (0 = off)"),
            ("lr_decay", S, "", "exponential (the preset's staircase decay, the default) | polynomial (from "
             "--initial_learning_rate to --end_learning_rate over --max_steps steps)"),
            ("end_learning_rate", Fl, 0.0001, "polynomial decay: the final learning rate"),
            ("lr_power", Fl, 1.0, "polynomial decay: the power"),
            ("accum_steps", I, 1, "gradient accumulation: every step runs N micro-batches of --batch_size images and "
             "applies one update from the sum of their gradients (BSP only; the learning rate is not rescaled)"),
            # mixup / CutMix (ops/mix.py; BSP only; the sampler's seed is --seed)
            ("mixup_alpha", Fl, 0.0, "mixup: Beta(alpha, alpha) parameter of the blend weight (0 = off)"),
            ("cutmix_alpha", Fl, 0.0, "CutMix: Beta(alpha, alpha) parameter of the kept area (0 = off)"),
            ("mix_prob", Fl, 1.0, "probability that a batch (a row with --mix_per_row) is mixed at all"),
            ("mix_switch_prob", Fl, 0.5, "with both alphas above 0: the probability of CutMix over mixup"),
            ("mix_per_row", B, False, "draw kind, weight and box per row instead of per batch"),
            # RandAugment in the input pipelines (ops/randaugment.py; every sync mode; the sampler's seed is --seed)
            ("randaugment_layers", I, 0, "RandAugment: ops applied per training image (0 = off)"),
            ("randaugment_magnitude", Fl, 9.0, "RandAugment: the magnitude, in [0, 10]"),
            ("randaugment_prob", Fl, 1.0, "RandAugment: probability that a drawn op is applied (else the identity)"),
            ("randaugment_ops", S, "", "RandAugment: comma-separated op names ('' = the 14 default ops; Invert, "
             "SolarizeAdd and Cutout are available by name)"),
            ("randaugment_translate_ratio", Fl, 0.45, "RandAugment: translation at magnitude 10, as a fraction of the "
             "image side"),
            ("randaugment_cutout_ratio", Fl, 0.18, "RandAugment: half side of the Cutout box at magnitude 10, as a "
             "fraction of the shorter image side"),
            # knowledge distillation (engine.DistillConfig; BSP only)
            ("distill_teacher", S, "", "nets_factory name of a frozen teacher network, built with the student's "
             "number of classes ('' = off)"),
            ("distill_teacher_kw", S, "", "numeric model keywords of the teacher, 'k=v,...' (e.g. resnet_size=8)"),
            ("distill_checkpoint", S, "", "the trained teacher's checkpoint, or a directory holding one (required "
             "with --distill_teacher)"),
            ("distill_teacher_ema", B, False, "restore the teacher from the checkpoint's EMA shadows"),
            ("distill_teacher_scope", S, "", "variable-scope prefix of the teacher's names in its checkpoint"),
            ("distill_alpha", Fl, 0.5, "weight of the soft-target term, in [0, 1]"),
            ("distill_temperature", Fl, 4.0, "temperature of the soft targets"),
            # MI355X-native extras
            # gradual magnitude pruning (ops.prune.PruneConfig; BSP only)
            ("prune_sparsity", Fl, 0.0, "target sparsity of gradual magnitude pruning, in (0, 1) (0 = off)"),
            ("prune_initial_sparsity", Fl, 0.0, "sparsity at --prune_begin_step"),
            ("prune_begin_step", I, 0, "first step whose update re-selects the masks"),
            ("prune_end_step", I, -1, "step at which the target is reached (-1 = --max_steps)"),
            ("prune_frequency", I, 100, "steps between two mask updates"),
            ("prune_exponent", Fl, 3.0, "exponent of the sparsity schedule"),
            ("prune_exclude", S, "", "regular expression: variables whose TF name it matches stay dense (usually "
             "the first conv and the logits)"),
            # sharpness-aware minimisation (ops.sam.SamConfig; BSP only)
            ("sam_rho", Fl, 0.0, "radius of the SAM perturbation: every micro-batch runs twice, the update takes the "
             "gradient at p + rho * g / |g| (0 = off; usual starting values: 0.05, with --sam_adaptive 0.5 - 2)"),
            ("sam_adaptive", B, False, "ASAM: the perturbation is scaled element-wise by p^2 (scale-invariant)"),
            ("sync_mode", S, "", "bsp | asp | ssp (default from the entry script)"),
            ("max_staleness", I, 5, "SSP staleness bound in local steps"),
            ("synthetic_data", B, False, "use HBM-resident synthetic batches"),
            ("bucket_mb", Fl, 32.0, "all-reduce bucket size (MB)"),
            ("use_hipgraph", B, False, "capture the BSP training step in a hipGraph (launch-bound models; "
             "single-rank only, ignored with a warning when world > 1)"),
            ("bn_sync_every", I, 1, "BSP: average the BN moving statistics over the replicas every N steps"),
            ("rccl_channels", I, 0, "pin the RCCL channel count (0 = RCCL's choice)"),
            ("grad_comm_dtype", S, "fp32", "gradient all-reduce dtype on the wire: fp32 | bf16"),
            # top-k sparsification with error feedback (ops.compress.GradCompress; BSP only)
            ("grad_compress_ratio", Fl, 0.0, "send only this fraction of every gradient bucket, its largest-magnitude "
             "entries of residual + gradient, and keep the rest for the next step, in (0, 1] (0 = off)"),
            ("grad_compress_begin_step", I, 0, "global steps before this one use the dense all-reduce"),
            ("deterministic", B, False, "bit-reproducible GPU reductions (no cross-block fp32 atomics)"),
            ("trace_steps", S, "", "a:b -> export a Chrome trace of steps [a, b)"),
            ("fresh", B, False, "wipe train_dir before training (the reference always did)"),
            ("log_every", I, 1, "log the per-step line every N steps"),
            ("metrics_file", S, "", "JSONL metrics path (rank 0)"),
            ("batch_weight", Fl, 1.0, "per-rank gradient weight b_r/b_nominal (C15)"),
            ("fault_inject", S, "", "rank:step[:hang] -> hard-exit (or hang) that rank at that step (resume tests)"),
            ("seed", I, 0, "random seed"),
            ("depth_multiplier", Fl, 1.0, "MobileNet depth multiplier"),
            ("fine_tune_checkpoint", S, "", "initialise model variables from this checkpoint (fresh runs only)"),
            ("train_accuracy_every", I, p.get("train_accuracy_every", 0),
             "every worker: every N steps, accuracy of the training-mode network on a fed batch of distorted training "
             "images (reference resnet/cifar10_resnet_bsp.py:146-148; 0 = off)"),
            ("train_accuracy_batch", I, 10000, "images in that fed batch (the reference feeds 10000)"),
    ):
        fn(name, default, h)
        flags.FLAGS.reset(name)  # the entry script's preset defaults win


def _device():
    if torch.cuda.is_available():
        return torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    return torch.device("cpu")


def make_input(cfg, batch_size, device, flags, rank, randaugment=None):
    """The training input of ``cfg``'s dataset.  randaugment: a RandAugmentConfig for the pipelines that hold uint8
    images (None: the calls, launches and bits of a run without it)."""
    ds = "synthetic_imagenet" if flags.synthetic_data and cfg["dataset"] == "imagenet" else cfg["dataset"]
    S = cfg["image_size"]
    ra_kw = dict(randaugment=randaugment, rank=rank) if randaugment is not None else {}
    if ds == "cifar10":
        from .data import cifar10
        return cifar10.distorted_inputs(flags.data_dir, batch_size, S, device=device, seed=flags.seed + rank, **ra_kw)
    if ds == "synthetic_mnist":
        from .data.synthetic import synthetic_mnist

        class _M:
            def __init__(self):
                self.x, self.y = synthetic_mnist(batch_size * 16, device, flags.seed + rank)
                self.i = 0

            def next_batch(self):
                s = (self.i % 16) * batch_size
                self.i += 1
                return self.x[s:s + batch_size], self.y[s:s + batch_size]
        return _M()
    if ds == "imagenet":
        from .data import imagenet
        if torch.device(device).type == "cuda":
            # decode on host threads, crop / resize / flip / colour on the GPU (data/imagenet_gpu.py); the node's
            # host CPUs are checked against what its ranks consume (data/capacity.py), and the device JPEG decode
            # (host marker parse only; HIP Huffman / IDCT / colour) is chosen when the full host decode cannot keep up
            from .data import capacity, imagenet_gpu
            split = capacity.choose_split_decode(cfg["model"])
            capacity.decode_capacity_check(cfg["model"], mode=split, log=logging.warning)
            return imagenet_gpu.distorted_inputs(imagenet.ImagenetData("train", flags.data_dir), batch_size,
                                                 image_size=S, device=device, seed=flags.seed + rank,
                                                 split_decode=split, **ra_kw)
        return imagenet.distorted_inputs(imagenet.ImagenetData("train", flags.data_dir), batch_size, image_size=S,
                                         device=device, seed=flags.seed + rank, **ra_kw)
    from .data.synthetic import SyntheticImages
    return SyntheticImages(batch_size, S, S, 3, cfg["num_classes"], device, seed=flags.seed + rank,
                           label_offset=1 if cfg["num_classes"] == 1001 else 0)


def make_loss_fn(label_smoothing=0.0, aux_weight=0.4, batch_weight=1.0):
    """Cross-entropy (+ weighted aux head) on the HIP softmax-xent kernel; L2 terms are applied as
    coupled weight decay inside the optimizer (identical gradient, K14)."""
    from .ops import nn as F

    def loss_fn(out, labels):
        aux = None
        if isinstance(out, tuple):
            out, aux = out
        heads = [(out, batch_weight)]
        if aux is not None and aux_weight:
            heads.append((aux, aux_weight * batch_weight))
        return F.mean_xent_loss(heads, labels, label_smoothing)
    return loss_fn


def train(preset, flags, default_mode="bsp"):
    FLAGS = flags.FLAGS
    cfg = dict(PRESETS[preset])
    mode = (FLAGS.sync_mode or default_mode).lower()
    logging.set_verbosity(logging.INFO)
    optimizer = (FLAGS.optimizer or cfg["optimizer"]).lower()
    if optimizer not in ("sgd", "momentum", "rmsprop", "lars", "adam", "lamb"):
        raise ValueError("--optimizer must be sgd, momentum, rmsprop, lars or adam, got %r (lamb is accepted too)"
                         % FLAGS.optimizer)
    if FLAGS.lr_decay not in ("", "exponential", "polynomial"):
        raise ValueError("--lr_decay must be exponential or polynomial, got %r" % FLAGS.lr_decay)
    if mode in ("asp", "ssp") and (optimizer == "lars" or FLAGS.clip_global_norm > 0):
        # checked before any process group or store exists: every rank fails at once
        raise ValueError(LARGE_BATCH_BSP_ONLY % mode)
    if mode in ("asp", "ssp") and optimizer == "adam":
        raise ValueError(ADAM_BSP_ONLY % mode)
    if optimizer == "lamb" and mode in ("asp", "ssp"):
        raise ValueError(LAMB_BSP_ONLY % mode)
    if optimizer == "lamb" and FLAGS.clip_global_norm > 0:
        raise ValueError(LAMB_NO_CLIP)
    accum = int(FLAGS.accum_steps)
    if accum < 1:
        raise ValueError("--accum_steps must be at least 1, got %d" % accum)
    if mode in ("asp", "ssp") and accum > 1:
        raise ValueError(ACCUM_BSP_ONLY % mode)
    mix_cfg = None
    if FLAGS.mixup_alpha != 0 or FLAGS.cutmix_alpha != 0:
        if mode in ("asp", "ssp"):
            raise ValueError(MIX_BSP_ONLY % mode)
        from .ops.mix import MixConfig
        mix_cfg = MixConfig(FLAGS.mixup_alpha, FLAGS.cutmix_alpha, FLAGS.mix_prob, FLAGS.mix_switch_prob,
                            FLAGS.mix_per_row, seed=FLAGS.seed)
    ra_cfg = randaugment_config(FLAGS, cfg)
    prune_cfg = prune_config(FLAGS, mode)
    sam_cfg = sam_config(FLAGS, mode)
    compress_cfg = compress_config(FLAGS, mode)
    distill_ckpt = distill_kw = None
    if FLAGS.distill_teacher:
        if mode in ("asp", "ssp"):
            raise ValueError(DISTILL_BSP_ONLY % mode)
        if FLAGS.distill_teacher not in nets_factory.networks_map:
            raise ValueError("--distill_teacher: unknown network %r" % FLAGS.distill_teacher)
        if not 0.0 <= FLAGS.distill_alpha <= 1.0:
            raise ValueError("--distill_alpha must lie in [0, 1], got %r" % FLAGS.distill_alpha)
        if not 0.0 < FLAGS.distill_temperature < float("inf"):
            raise ValueError("--distill_temperature must be positive, got %r" % FLAGS.distill_temperature)
        distill_kw = parse_model_kw(FLAGS.distill_teacher_kw)
        distill_ckpt = distill_checkpoint_path(FLAGS.distill_checkpoint)
    ps_hosts = [h for h in FLAGS.ps_hosts.split(",") if h]
    worker_hosts = [h for h in FLAGS.worker_hosts.split(",") if h]
    if FLAGS.job_name == "ps":
        Server({"ps": ps_hosts, "worker": worker_hosts}, "ps", FLAGS.task_id).join()
        return 0
    # RCCL knobs before the communicator exists: channel count, per-bucket timing for the JSONL metrics
    pg.rccl_env(FLAGS.rccl_channels, timing=bool(FLAGS.metrics_file))
    if worker_hosts and "WORLD_SIZE" not in os.environ:
        Server({"ps": ps_hosts, "worker": worker_hosts}, "worker", FLAGS.task_id)
    else:
        pg.init()
    rank, world = pg.rank(), pg.world_size()
    device = _device()
    logging.info("replica %d of world %d (%s, %s)", rank, world, mode, device)
    torch.manual_seed(FLAGS.seed + (rank if mode != "bsp" else 0))
    from .ops import elementwise as _ew
    _ew.set_base_seed(FLAGS.seed, rank)  # independent dropout masks per replica
    if FLAGS.deterministic and device.type == "cuda":
        from .ops import _lib
        _lib.set_deterministic(True)

    # ---- model ---------------------------------------------------------------------------------
    mkw = dict(cfg.get("model_kw", {}))
    if cfg["model"] == "cifar10_resnet_v2":
        mkw["resnet_size"] = FLAGS.resnet_size
    if cfg["model"].startswith("mobilenet") and FLAGS.depth_multiplier != 1.0:
        mkw["depth_multiplier"] = FLAGS.depth_multiplier
    if "quantize" in FLAGS and FLAGS.quantize:
        # tf.contrib.quantize.create_training_graph(quant_delay=get_quant_delay())
        # (reference vgg/nets/mobilenet_v1_train.py:66-73,138-139): quantise at once when fine-tuning
        from .compat.quantize import QuantConfig
        quant_fused = bool("quant_fused" in FLAGS and FLAGS.quant_fused)
        mkw["quantize"] = QuantConfig(quant_delay=0 if FLAGS.fine_tune_checkpoint else FLAGS.quant_delay,
                                      fused=quant_fused)
        if FLAGS.use_hipgraph and not quant_fused:
            logging.warning("--quantize --use_hipgraph without --quant_fused: the captured step freezes the side of "
                            "--quant_delay it was captured on (quantisation never starts, or never stops)")
    model = nets_factory.build(cfg["model"], num_classes=cfg["num_classes"], **mkw).to(device)
    if cfg.get("wd_all") is not None:  # loss += wd * sum(l2_loss(v) for v in trainable_variables())
        for p in model.parameters():
            if p.requires_grad:
                p.weight_decay = cfg["wd_all"]
    B = FLAGS.batch_size
    data = make_input(cfg, B, device, FLAGS, rank, ra_cfg)

    # ---- schedule (C16, C19) ---------------------------------------------------------------------
    n_train = CIFAR_TRAIN if cfg["dataset"] in ("cifar10",) else IMAGENET_TRAIN
    # (a step consumes accum * B images per worker: --batch_size stays the micro-batch, as in the reference)
    batches_per_epoch = n_train / float(B * accum)
    decay_steps = batches_per_epoch * FLAGS.num_epochs_per_decay
    if cfg.get("decay_div_workers") and mode == "bsp":
        decay_steps /= max(world, 1)
    scale = world if (cfg["lr_scale_workers"] and mode == "bsp") else 1
    sched = ExponentialDecay(FLAGS.initial_learning_rate * scale, max(decay_steps, 1.0),
                             FLAGS.learning_rate_decay_factor, staircase=True)
    if FLAGS.lr_decay == "polynomial":
        sched = PolynomialDecay(FLAGS.initial_learning_rate * scale, max(FLAGS.max_steps, 1), FLAGS.end_learning_rate,
                                FLAGS.lr_power)
    if FLAGS.warmup_steps > 0:
        sched = LinearWarmup(sched, FLAGS.warmup_steps)
    opt_kw = dict(optimizer=optimizer, lr=sched(0), momentum=cfg.get("momentum", 0.9),
                  rho=cfg.get("rmsprop_decay", 0.9),
                  epsilon={"adam": FLAGS.adam_epsilon, "lamb": FLAGS.lamb_epsilon}.get(
                      optimizer, cfg.get("rmsprop_epsilon", 1e-10)))

    # ---- engine + supervisor / checkpoints (C7, §5.4) -------------------------------------------
    from .compat.train import Supervisor, latest_checkpoint
    is_chief = rank == 0
    if is_chief and FLAGS.fresh and os.path.isdir(FLAGS.train_dir):
        shutil.rmtree(FLAGS.train_dir)
    pg.barrier()
    path = latest_checkpoint(FLAGS.train_dir) if os.path.isdir(FLAGS.train_dir) else None
    # TF variable layout of the trainer: its variable_scope prefix and, for the
    # partitioned scopes, P = len(ps_hosts) axis-0 slices per variable (tf.fixed_size_partitioner)
    ckpt_kw = dict(prefix=cfg.get("scope_prefix", ""),
                   partitions=max(1, len(ps_hosts)) if cfg.get("partitioned") else None)
    gstep = torch.zeros((), dtype=torch.int64)
    loss_fn = make_loss_fn(cfg.get("label_smoothing", 0.0), cfg.get("aux_weight", 0.4), FLAGS.batch_weight)
    store = clock = None
    ft_missing = None
    if FLAGS.fine_tune_checkpoint and not path:
        # model variables only (no slots, no global step: the schedule restarts), missing ones keep their
        # initialisation (e.g. a new logits layer).  Restored BEFORE the engine / store exist, so the BSP
        # broadcast, the BN-statistics sync snapshot, the bf16 compute copies and the ASP owner shards all start
        # from the fine-tune values (a restore after them would be folded into the next BN sync as a W-fold delta)
        ft = [v for v in model_variables(model, None, None, prefix=ckpt_kw["prefix"])]
        ft_missing = Saver(ft).restore(FLAGS.fine_tune_checkpoint, strict=False)
    distill_cfg = None
    if distill_ckpt:
        # the frozen teacher: built with the student's classes, restored as an evaluator restores (EMA shadows on
        # request), and handed to the step; it is in none of the variable lists below, so no checkpoint holds it
        from .engine import DistillConfig
        from .evaluator import restore_for_eval
        teacher = nets_factory.build(FLAGS.distill_teacher, num_classes=cfg["num_classes"], **distill_kw).to(device)
        restore_for_eval(teacher, distill_ckpt, FLAGS.distill_teacher_ema, prefix=FLAGS.distill_teacher_scope)
        t_size = nets_factory.default_image_size(FLAGS.distill_teacher)
        if t_size != cfg["image_size"]:
            logging.warning("the teacher %s is built for %d x %d images and is fed the student's %d x %d batches as "
                            "they are", FLAGS.distill_teacher, t_size, t_size, cfg["image_size"], cfg["image_size"])
        distill_cfg = DistillConfig(teacher, FLAGS.distill_alpha, FLAGS.distill_temperature)
        logging.info("distilling from %s (%s), alpha %g, temperature %g", FLAGS.distill_teacher, distill_ckpt,
                     FLAGS.distill_alpha, FLAGS.distill_temperature)
    if mode == "bsp":
        if FLAGS.use_hipgraph and world > 1:
            logging.warning("--use_hipgraph ignored: step capture is single-rank only (world size %d)", world)
        step_fn = TrainStep(model, bucket_mb=FLAGS.bucket_mb, label_smoothing=cfg.get("label_smoothing", 0.0),
                            aux_weight=cfg.get("aux_weight", 0.4), ema_decay=cfg.get("ema"), lr_schedule=sched,
                            batch_weight=FLAGS.batch_weight, use_graph=FLAGS.use_hipgraph and world == 1,
                            ema_buffers=cfg.get("ema_buffers", True), bn_sync_every=FLAGS.bn_sync_every,
                            wgrad_stream=cfg.get("wgrad_stream"),
                            grad_comm_dtype=torch.bfloat16 if FLAGS.grad_comm_dtype == "bf16" else None,
                            timer=StepTimer() if (FLAGS.metrics_file and rank == 0 and not FLAGS.use_hipgraph)
                            else None, lars_eeta=FLAGS.lars_eeta, lars_epsilon=FLAGS.lars_epsilon,
                            clip_global_norm=FLAGS.clip_global_norm if FLAGS.clip_global_norm > 0 else None,
                            beta1=FLAGS.adam_beta1, beta2=FLAGS.adam_beta2, accum_steps=accum, mix=mix_cfg, rank=rank,
                            distill=distill_cfg, prune=prune_cfg, sam=sam_cfg, grad_compress=compress_cfg,
                            **opt_kw)
        # (the pruner's <scope>/mask and <scope>/threshold in front of the global step, which stays last)
        vars_ = model_variables(model, step_fn.opt, gstep, pruner=step_fn.pruner, **ckpt_kw)
        vars_[-1].name = cfg.get("global_step_name", "global_step")
        if path:
            Saver(vars_).restore(path)
        if world > 1:  # one collective replaces the reference's chief-init + 1 s polling of workers
            # (Adam's beta*_power scalars are host values derived from the step count, which every rank restores)
            pg.broadcast_tensors([v.tensor for v in vars_ if v.tensor.is_floating_point()
                                  and not isinstance(v, (AdamPowerVar, MaskVar, ThresholdVar))]
                                 + [b for b in model.buffers()])
        from .ops.nn import invalidate_weight_copies
        invalidate_weight_copies(model.parameters())  # bf16 compute copies follow the restored weights
        step_fn.bufsync.resync()  # the BN statistics' sync snapshot follows the restored / broadcast values
        step_fn.global_step = int(gstep)
        step_fn.opt.restored(int(gstep))  # num_updates; Adam: the applied-update count from beta*_power
        if step_fn.pruner is not None:
            # every rank restored the same masks (all ones where the checkpoint held none): kept counts follow them
            step_fn.pruner.masks_loaded()
    elif mode in ("asp", "ssp"):
        from .engine import moving_average_buffers, prepare_compute_copies
        from .parallel.asp import ASPTrainStep, ParamStore
        from .parallel.ssp import StalenessClock
        vars_ = model_variables(model, None, gstep, **ckpt_kw)
        vars_[-1].name = cfg.get("global_step_name", "global_step")
        if path:  # owners initialise their shards from the restored replica
            Saver(vars_).restore(path)
        prepare_compute_copies(model)
        store = ParamStore(list(model.parameters()), optimizer, sched(0), opt_kw["momentum"], opt_kw["rho"],
                           opt_kw["epsilon"], run_id=os.environ.get("DTM_RUN_ID", "0"),
                           buffers=moving_average_buffers(model))
        if is_chief and int(gstep):
            store.set_global_step(int(gstep))
        # optimizer slots live in the owner shards: checkpointed from there, restored into them
        slot_vars = [v for v in model_variables(model, None, None, store=store, **ckpt_kw)
                     if v.name.endswith(("/Momentum", "/RMSProp", "/RMSProp_1"))]
        if path and is_chief and slot_vars:
            Saver(slot_vars).restore(path, strict=False)
        vars_ = vars_[:-1] + slot_vars + vars_[-1:]
        pg.barrier()
        if mode == "ssp":
            clock = StalenessClock(FLAGS.max_staleness, log_fn=logging.info)
        step_fn = ASPTrainStep(model, loss_fn, store, sched, clock)
    else:
        raise ValueError("sync_mode must be bsp, asp or ssp")
    if path:
        logging.info("rank %d restored %s (global_step %d)", rank, path, int(gstep))
    elif FLAGS.fine_tune_checkpoint:
        logging.info("fine-tuning from %s (%d variables not in the checkpoint)", FLAGS.fine_tune_checkpoint,
                     len(ft_missing or []))
    saver = Saver(vars_, max_to_keep=cfg["max_to_keep"])
    if is_chief and os.path.isdir(FLAGS.train_dir):
        saver.recover_last_checkpoints(FLAGS.train_dir)
    sv = Supervisor(is_chief=is_chief, logdir=FLAGS.train_dir, saver=saver, global_step=gstep,
                    save_model_secs=FLAGS.save_interval_secs)
    start = int(gstep) if mode == "bsp" else store.global_step() if is_chief else int(gstep)

    metrics = JsonlMetrics(FLAGS.metrics_file if is_chief else None)
    tracer = StepTracer(FLAGS.trace_steps, os.path.join(FLAGS.train_dir, "traces"), rank)
    fault = None
    if FLAGS.fault_inject and os.environ.get("DTM_ATTEMPT", "0") == "0":  # only the first attempt
        parts = FLAGS.fault_inject.split(":")
        fault = (int(parts[0]), int(parts[1]), parts[2] if len(parts) > 2 else "exit")
    heartbeat = Heartbeat(rank)

    # training-side TensorBoard scalars (the graph-side summaries the reference defines, e.g.
    # cnn/cifar10.py:309-335,361: learning_rate, total_loss (raw) and its 0.9 moving average), written
    # to train_dir by the chief at most every --save_summaries_secs
    from .utils.tb import SummaryWriter
    tbw = SummaryWriter(FLAGS.train_dir) if (is_chief and (FLAGS.save_summaries_secs > 0 or
                                                           FLAGS.save_summaries_steps > 0)) else None
    loss_avg, t_summary = None, None
    # histogram / sparsity / image summaries (utils/summaries.py; all off by default)
    summ = None
    if tbw is not None and (FLAGS.summary_histograms or FLAGS.summary_activations or FLAGS.summary_images > 0):
        from .utils.summaries import TrainSummaries
        summ = TrainSummaries(model, step_fn, mode, FLAGS.summary_histograms, FLAGS.summary_activations,
                              FLAGS.summary_images)

    # ---- loop (reference hot loop) ------------------------------------------------
    step = start if mode == "bsp" else 0
    probe = None  # the --train_accuracy_every input pipeline (created on first use)
    loss_v = float("nan")
    t_log, n_since = time.time(), 0
    while step < FLAGS.max_steps:
        if fault and fault[0] == rank and fault[1] == step:
            if fault[2] == "hang":
                logging.error("fault injection: rank %d hangs at step %d", rank, step)
                while True:  # a wedged rank: alive, silent, never reaches the next collective
                    time.sleep(3600)
            logging.error("fault injection: rank %d exits at step %d", rank, step)
            os._exit(17)
        tracer.step(step)
        if accum > 1:  # N micro-batches per step, handed over as lists (no concatenation copy)
            images, labels = (list(v) for v in zip(*[data.next_batch() for _ in range(accum)]))
        else:
            images, labels = data.next_batch()
        if mode == "bsp":
            loss = step_fn(images, labels)
            gs = step_fn.global_step
        else:
            loss, gs = step_fn(images, labels)
        n_since += 1
        log_now = step % max(FLAGS.log_every, 1) == 0 or step + 1 >= FLAGS.max_steps
        # a summary step is a logged step on which the time rule or the step rule fires; the device work of the
        # histogram / activation / image summaries is enqueued here, right after the step (the flat gradient
        # buffer keeps its values until the next zero_grad), and read after this logged step's synchronisation
        summ_now = tbw is not None and log_now and (
            (FLAGS.save_summaries_secs > 0 and
             (t_summary is None or time.time() - t_summary >= FLAGS.save_summaries_secs)) or
            (FLAGS.save_summaries_steps > 0 and gs % FLAGS.save_summaries_steps == 0))
        if summ is not None and summ_now:
            summ.launch(images[-1] if accum > 1 else images)  # (the gradients are the whole step's)
        # the loss is read (a device sync) on log steps only; the NaN assertion of the reference
        # (imagenet_inception_bsp.py:191, every step) is checked there, and non-finite steps in
        # between are caught by the engine's device-side guard (update skipped, counted, reported)
        need_log = log_now
        if need_log:
            loss_v = float(loss)
        dt = 0.0
        if log_now:
            # the device is drained only on logged steps (the time is averaged over the steps since the
            # last log line); the other steps leave the host free to run ahead of the GPU
            if device.type == "cuda":
                torch.cuda.synchronize()
            now = time.time()
            dt = (now - t_log) / n_since
            t_log, n_since = now, 0
        if cfg.get("nan_guard") and math.isnan(loss_v):  # imagenet_inception_bsp.py:191
            raise FloatingPointError("Model diverged with loss = NaN")
        skipped_now = mode == "bsp" and need_log and step_fn.poll_skipped()
        if skipped_now:
            if cfg.get("nan_guard"):
                # the reference asserts on a NaN loss every step; here the device-side guard skipped the update
                # of a non-finite step and the check fires at the next log line (at most --log_every steps late)
                raise FloatingPointError("Model diverged with loss = NaN (non-finite gradients at a step since "
                                         "the last log line; %d update(s) skipped)" % step_fn.skipped)
            logging.warning("step %d: non-finite gradients since the last log line, update(s) skipped (%d so far)",
                            step, step_fn.skipped)
        gstep.fill_(gs)
        if log_now:
            ips = accum * B / max(dt, 1e-9)  # images of the whole step: accum micro-batches of B
            print(format_step(cfg["log_style"], step, gs, loss_v, ips, dt), flush=True)
            if tbw is not None and loss_v == loss_v:
                loss_avg = loss_v if loss_avg is None else 0.9 * loss_avg + 0.1 * loss_v
                if summ_now:
                    t_summary = time.time()
                    tbw.add_scalar("learning_rate", float(sched(gs)), gs)
                    tbw.add_scalar("total_loss (raw)", loss_v, gs)
                    tbw.add_scalar("total_loss", loss_avg, gs)
                    tbw.add_scalar("images_per_sec", world * ips, gs)
            if summ is not None and summ_now:
                summ.write(tbw, gs)
            extra = step_fn.timer.sections() if (mode == "bsp" and step_fn.timer is not None) else {}
            if mode == "bsp" and step_fn.opt.normed and (metrics.f is not None or (tbw is not None and summ_now)):
                # the norm pass's results of this step (LARS / clipping / LAMB only), read after the logged step's
                # synchronisation above: no other step reads them on the host
                ns = step_fn.opt.norm_stats()
                if math.isfinite(ns["grad_norm"]) and tbw is not None and summ_now:
                    tbw.add_scalar("gradient_norm", ns["grad_norm"], gs)
                    for k in ("lars/min_trust_ratio", "lars/max_trust_ratio", "update_norm",
                              "lamb/min_trust_ratio", "lamb/max_trust_ratio"):
                        if k in ns:
                            tbw.add_scalar(k, ns[k], gs)
                extra.update(ns)
            if mode == "bsp" and optimizer in ("adam", "lamb") and metrics.f is not None:
                extra["adam_step"] = step_fn.opt.adam_step()  # applied updates: lags global_step after a NaN skip
            if mix_cfg is not None and metrics.f is not None:
                extra["mix_lambda"] = step_fn.last_mix_lambda()  # mean own-label weight of this step (a host value)
            if ra_cfg is not None and metrics.f is not None:
                extra["randaugment_layers"], extra["randaugment_magnitude"] = ra_cfg.layers, ra_cfg.magnitude
            if distill_cfg is not None and metrics.f is not None:
                extra["distill_kl"] = step_fn.last_distill_kl()  # a device read, after the synchronisation above
            if sam_cfg is not None and metrics.f is not None:
                extra["sam_grad_norm"] = step_fn.last_sam_norm()  # a device read, after the synchronisation above
            if compress_cfg is not None and metrics.f is not None:
                extra["grad_compress_ratio"] = compress_cfg.ratio
                extra["wire_mb"] = step_fn.dp.wire_bytes(gs - 1) / 1e6  # sent per rank in the step just run
                extra["residual_norm"] = step_fn.dp.residual_norm()  # a device read, after the synchronisation above
            if prune_cfg is not None and metrics.f is not None:
                # a device read, after the synchronisation above
                extra["sparsity"], extra["prune_target"] = step_fn.last_sparsity()
            if metrics.f is not None and getattr(mkw.get("quantize"), "fused", False):
                # device reads, after the logged step's synchronisation above
                from .ops import fakequant
                extra["quant_step"] = mkw["quantize"].steps_done()
                extra["quant_nonfinite_batches"] = fakequant.nonfinite_batches(model)
            if mode == "bsp" and metrics.f is not None and world > 1:
                bms = step_fn.dp.bucket_ms()  # per-bucket all-reduce durations (RCCL timing events)
                if bms:
                    extra["bucket_allreduce_ms"] = bms
            if device.type == "cuda" and metrics.f is not None:
                extra["max_mem_gb"] = torch.cuda.max_memory_allocated(device) / 2 ** 30
            if skipped_now and metrics.f is not None:
                # which micro-batches of THIS step were non-finite on this rank (the skip may be an earlier step's)
                extra["nonfinite_micro_batches"] = step_fn.nonfinite_micro()
            metrics.write(step=step, global_step=gs, loss=loss_v, lr=sched(gs), images_per_sec=ips,
                          node_images_per_sec=world * ips, step_ms=dt * 1e3, world=world, mode=mode,
                          accum_steps=accum, **extra)
        # every worker runs the probe, as every reference worker does (resnet/cifar10_resnet_bsp.py:146-148)
        if FLAGS.train_accuracy_every and step % FLAGS.train_accuracy_every == 0:
            if probe is None:
                probe = make_input(cfg, FLAGS.train_accuracy_batch, device, FLAGS, rank + 7919, ra_cfg)
            acc = train_accuracy_probe(model, probe)
            # tf.logging.info('evaluation: step - '+str(step)+'; accuracy: '+ str(accuracy))
            logging.info("evaluation: step - %d; accuracy: %s", step, str(np.float32(acc)))
        if mode == "bsp" or is_chief:
            sv.maybe_save(gs, force=bool(FLAGS.save_every_steps) and gs % FLAGS.save_every_steps == 0)
        heartbeat.beat(step)
        step += 1
    if mode in ("asp", "ssp"):
        if clock is not None:
            clock.finish()
        store.pull()
    sv.maybe_save(int(gstep), force=True)
    metrics.close()
    if tbw is not None:
        tbw.close()
    if store is not None:  # owners keep their shards alive until every worker is done with them
        from .parallel.asp import wait_all_done
        wait_all_done(store.store, world, store.run_id)
        store.close()
    pg.barrier()
    return 0


def train_accuracy_probe(model, data):
    """The reference's training-set accuracy probe (resnet/cifar10_resnet_bsp.py:66-70,146-148): accuracy_op =
    mean(argmax(network(inputs, True)) == labels) run on one fed batch of distorted training images - the
    network in TRAINING mode (batch statistics), whose BN moving averages that sess.run leaves alone (the
    reference never runs UPDATE_OPS there).  Here the moving statistics are saved and restored around the
    forward (the fused training-mode kernels update them in place)."""
    from .engine import side_forward
    images, labels = data.next_batch()
    with side_forward(model), torch.no_grad():
        out = model(images, training=True)
        if isinstance(out, tuple):
            out = out[0]
        from .ops.lazy import as_tensor
        acc = (as_tensor(out).float().argmax(-1) == labels).float().mean().item()
    return acc


def build_model_for_eval(preset, flags_values=None, **kw):
    cfg = PRESETS[preset]
    mkw = dict(cfg.get("model_kw", {}))
    mkw.update(kw)
    return nets_factory.build(cfg["model"], num_classes=cfg["num_classes"], **mkw)


__all__ = ["PRESETS", "define_common_flags", "train", "TFVar"]
