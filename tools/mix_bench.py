#!/usr/bin/env python3
"""Cost of mixup / CutMix (csrc/kernels/mix.hip), with the method of tools/accum_bench.py.

HIP events on one GPU, bf16 NHWC batches:
  (a) ``mix_images`` on [256, 224, 224, 3] (rows of 301056 bytes: the 16-byte path) and on [128, 299, 299, 3] (rows
      of 536406 bytes, no multiple of 16: a row and its partner sit at different offsets, the element path), each
      under a mixup plan and under a CutMix plan;
  (b) the same result from torch ops on the device: ``x[partner]``, two multiplies and an add (fp32, cast back) for
      mixup; ``x[partner]``, a box mask and ``torch.where`` for CutMix;
  (c) with --step: the whole ResNet-50 training step (bf16, batch --batch) with ``mix=None`` and with
      ``MixConfig(mixup_alpha=0.2, cutmix_alpha=1.0)``.
Each sample is one event pair around ``--reps`` back-to-back launches; the variants alternate within a round and the
figure is the median over the rounds, per launch, with min and max.  The implied bytes/s divide the bytes the result
needs (mixup: two reads and a write, 6 B per bf16 element; CutMix: one read and a write, 4 B) by that time;
back-to-back launches over the same buffers run partly out of the 256 MiB Infinity Cache, so they are not HBM rates.
``kernel_not_slower``: the kernel's median is at most the torch form's median plus the spread (max - min) of the torch
arm's rounds.  Prints one JSON line and appends it to --log.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

SHAPES = {"224": (256, 224, 224, 3), "299": (128, 299, 299, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time whole ResNet-50 training steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mix_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops import mix

    assert torch.cuda.is_available(), "mix_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)

    def torch_mixup(x, idx, w):
        return (w * x + (1.0 - w) * x[idx]).to(x.dtype)  # (w is fp32 [B, 1, 1, 1]: the products and the sum are fp32)

    def torch_cutmix(x, idx, box):
        B, H, W, _C = x.shape
        ys = torch.arange(H, device=x.device).view(1, H, 1, 1)
        xs = torch.arange(W, device=x.device).view(1, 1, W, 1)
        y0, y1, x0, x1 = (box[:, k].view(B, 1, 1, 1) for k in range(4))
        return torch.where((ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1), x[idx], x)

    out = dict(rounds=args.rounds, reps=args.reps)
    fns, nbytes = {}, {}
    for tag, shape in SHAPES.items():
        B, H, W, _C = shape
        x = torch.randn(shape, device=dev).to(torch.bfloat16)
        buf = torch.empty_like(x)
        mp = mix.sample_plan(mix.MixConfig(mixup_alpha=0.2, seed=1), 0, 0, 0, B, H, W).to(dev)
        cp = mix.sample_plan(mix.MixConfig(cutmix_alpha=1.0, seed=1), 0, 0, 0, B, H, W).to(dev)
        assert mp.kinds()[0] == "mixup" and cp.kinds()[0] == "cutmix"
        y0, y1, x0, x1 = (int(v) for v in cp.box[0])
        out["cutmix_box_share_" + tag] = round((y1 - y0) * (x1 - x0) / (H * W), 4)
        idx = torch.from_numpy(mp.partner.astype("int64")).to(dev)
        w = torch.from_numpy(mp.w_pix.copy()).to(dev).view(B, 1, 1, 1)
        cidx = torch.from_numpy(cp.partner.astype("int64")).to(dev)
        cbox = torch.from_numpy(cp.box.astype("int64")).to(dev)
        # the kernel and the torch form compute the same thing, at the timed size
        assert torch.equal(mix.mix_images(x, mp, out=buf), torch_mixup(x, idx, w))
        assert torch.equal(mix.mix_images(x, cp, out=buf), torch_cutmix(x, cidx, cbox))
        torch.cuda.synchronize()
        fns["a_kernel_mixup_" + tag] = lambda x=x, p=mp, o=buf: mix.mix_images(x, p, out=o)
        fns["b_torch_mixup_" + tag] = lambda x=x, i=idx, w=w: torch_mixup(x, i, w)
        fns["a_kernel_cutmix_" + tag] = lambda x=x, p=cp, o=buf: mix.mix_images(x, p, out=o)
        fns["b_torch_cutmix_" + tag] = lambda x=x, i=cidx, b=cbox: torch_cutmix(x, i, b)
        for kind, per in (("mixup", 6.0), ("cutmix", 4.0)):
            for arm in ("a_kernel_", "b_torch_"):
                nbytes[arm + kind + "_" + tag] = per * x.numel()
    res = _alternate(fns, args.rounds, args.reps, args.warmup)
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        out[k + "_GBps"] = round(nbytes[k] / (med * 1e-3) / 1e9, 1)
    for tag in SHAPES:
        for kind in ("mixup", "cutmix"):
            kern, ref = "a_kernel_%s_%s" % (kind, tag), "b_torch_%s_%s" % (kind, tag)
            spread = res[ref][2] - res[ref][1]
            out["%s_%s_torch_over_kernel" % (kind, tag)] = round(res[ref][0] / res[kern][0], 3)
            out["%s_%s_kernel_not_slower" % (kind, tag)] = bool(res[kern][0] <= res[ref][0] + spread)

    if args.step:
        del fns, x, buf
        torch.cuda.empty_cache()
        steps = {}
        for name, cfg in (("plain", None), ("mixed", mix.MixConfig(mixup_alpha=0.2, cutmix_alpha=1.0))):
            torch.manual_seed(0)
            net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
            steps[name] = TrainStep(net, optimizer="momentum", lr=0.01, momentum=0.9, mix=cfg)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        sres = _alternate({k: (lambda s=s: s(x, y)) for k, s in steps.items()}, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for k, (med, lo, hi) in sres.items():
            out["step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        out["step_mixed_over_plain"] = round(sres["mixed"][0] / sres["plain"][0], 4)
        out["step_overhead_ms"] = round(sres["mixed"][0] - sres["plain"][0], 3)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
