#!/usr/bin/env python3
"""Cost of knowledge distillation (dtm_softmax_xent_distill, TrainStep(distill=...)), with the method of
tools/mix_bench.py.

HIP events on one GPU, bf16:
  (a) the distillation loss and its gradient (alpha 0.5, temperature 4, smoothing 0.1, gradient of the batch mean) on
      student / teacher logits of [256, 1000] and [128, 1001]:
        a_kernel   one launch of dtm_softmax_xent_distill (per-row loss, per-row KL, dlogits);
        a_fused    ``mean_xent_loss(..., distill=...)`` forward and backward: that launch, the combine, the scale pass;
        b_torch    the torch-op composition of the same definition (``log_softmax`` / ``softmax`` in fp32) and its
                   autograd backward.
      The kernel's results are checked against the composition's at the timed size first, within the bounds of
      tests/test_distill_gpu.py (L2-relative: loss rows and KL rows 1e-4, bf16 gradient 1e-2).
  (b) with --step: whole training steps at batch --batch on 224 x 224 images: ResNet-50 with ``distill=None`` and with a
      ResNet-50 teacher; MobileNet v1 with ``distill=None`` and with a ResNet-50 teacher; and, to confront the
      expectation that distillation costs one inference forward of the teacher, that forward alone (no grad).
Each sample is one event pair around ``--reps`` back-to-back calls; the variants alternate within a round and the
figure is the median over the rounds, per call, with min and max.  Prints one JSON line and appends it to --log.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

SHAPES = {"256x1000": (256, 1000), "128x1001": (128, 1001)}
ALPHA, TEMP, SMOOTH = 0.5, 4.0, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time whole training steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "distill_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import DistillConfig, TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops import _lib
    from distributed_tensorflow_models_amd.ops import nn as F

    assert torch.cuda.is_available(), "distill_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    L = _lib.lib()

    def rel(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / (b.norm() + 1e-12))

    def torch_rows(s, z, labels):
        """Per-row loss and KL from torch ops, fp32 (the composition of ops/nn.py spelled out)."""
        K = s.shape[1]
        logp = torch.log_softmax(s.float(), -1)
        t = torch.full_like(logp, SMOOTH / K).scatter_(1, labels.view(-1, 1), 1.0 - SMOOTH + SMOOTH / K)
        hard = -(t * logp).sum(-1)
        zt = z.float() / TEMP
        log_q = torch.log_softmax(zt, -1)
        kl = (torch.softmax(zt, -1) * (log_q - torch.log_softmax(s.float() / TEMP, -1))).sum(-1)
        return (1.0 - ALPHA) * hard + (ALPHA * TEMP * TEMP) * kl, kl

    out = dict(rounds=args.rounds, reps=args.reps, alpha=ALPHA, temperature=TEMP)
    fns = {}
    for tag, (B, K) in SHAPES.items():
        s = (torch.randn(B, K, device=dev) * 3).to(torch.bfloat16)
        z = (torch.randn(B, K, device=dev) * 3).to(torch.bfloat16)
        labels = torch.randint(0, K, (B,), device=dev)
        lab32 = labels.to(torch.int32)
        loss, kl, dl = (torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty_like(s))

        def kernel(s=s, z=z, lab32=lab32, loss=loss, kl=kl, dl=dl, B=B, K=K):
            rc = L.dtm_softmax_xent_distill(_lib.ptr(s), 1, _lib.ptr(z), K, _lib.ptr(lab32), None, _lib.ptr(loss),
                                            _lib.ptr(kl), _lib.ptr(dl), B, K, SMOOTH, ALPHA, TEMP, 1.0 / B, K,
                                            _lib.stream_ptr())
            assert rc == 0

        def fused(s=s, z=z, labels=labels):
            si = s.detach().requires_grad_()
            F.mean_xent_loss([(si, 1.0)], labels, SMOOTH, distill=F.Distill(z, ALPHA, TEMP)).backward()
            return si.grad

        def composed(s=s, z=z, labels=labels):
            si = s.detach().requires_grad_()
            torch_rows(si, z, labels)[0].mean().backward()
            return si.grad

        # the same thing on both arms, at the timed size
        kernel()
        want_rows, want_kl = torch_rows(s, z, labels)
        want_grad = composed()
        torch.cuda.synchronize()
        errs = dict(loss=rel(loss, want_rows), kl=rel(kl, want_kl), grad=rel(dl, want_grad),
                    fused_grad=rel(fused(), want_grad))
        assert errs["loss"] < 1e-4 and errs["kl"] < 1e-4 and errs["grad"] < 1e-2 and errs["fused_grad"] < 1e-2, errs
        out["rel_err_" + tag] = {k: float("%.3g" % v) for k, v in errs.items()}
        fns["a_kernel_" + tag], fns["a_fused_" + tag], fns["b_torch_" + tag] = kernel, fused, composed
    res = _alternate(fns, args.rounds, args.reps, args.warmup)
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    for tag in SHAPES:
        out["torch_over_kernel_" + tag] = round(res["b_torch_" + tag][0] / res["a_kernel_" + tag][0], 2)
        out["torch_over_fused_" + tag] = round(res["b_torch_" + tag][0] / res["a_fused_" + tag][0], 2)

    if args.step:
        del fns
        torch.cuda.empty_cache()

        def net(name, seed):
            torch.manual_seed(seed)
            return nets_factory.build(name, num_classes=1000).to(dev)

        def step(student, teacher):
            cfg = DistillConfig(net(teacher, 1), ALPHA, TEMP) if teacher else None
            return TrainStep(net(student, 0), optimizer="momentum", lr=0.01, momentum=0.9, distill=cfg)

        steps = dict(resnet50_plain=step("resnet_v1_50", None), resnet50_distill=step("resnet_v1_50", "resnet_v1_50"),
                     mobilenet_plain=step("mobilenet_v1", None), mobilenet_distill=step("mobilenet_v1", "resnet_v1_50"))
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        calls = {k: (lambda s=s: s(x, y)) for k, s in steps.items()}
        calls["teacher_forward"] = lambda s=steps["resnet50_distill"]: s._teacher_logits(x)
        sres = _alternate(calls, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for k, (med, lo, hi) in sres.items():
            out["step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        fwd = sres["teacher_forward"][0]
        for k in ("resnet50", "mobilenet"):
            over = sres[k + "_distill"][0] - sres[k + "_plain"][0]
            out["step_%s_overhead_ms" % k] = round(over, 3)
            out["step_%s_distill_over_plain" % k] = round(sres[k + "_distill"][0] / sres[k + "_plain"][0], 4)
            out["step_%s_overhead_over_teacher_forward" % k] = round(over / fwd, 3)
        out["distill_kl_resnet50"] = round(steps["resnet50_distill"].last_distill_kl(), 4)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
