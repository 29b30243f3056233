#!/usr/bin/env python3
"""Cost of gradient accumulation (csrc/kernels/grad_accum.hip) on ResNet-50's 25.6 M gradient elements, with the
method of tools/adam_bench.py.

Two flat fp32 buffers of ResNet-50's gradient size (the flat gradient buffer and the accumulator of
parallel/bsp.py), HIP events on one GPU:
  (a)  mode 1 (acc += g; g = 0) in one launch, 16 B per element, against ``acc.add_(g); g.zero_()``;
  (a1) mode 1 with both ranges starting one element past a 16-byte boundary (16-byte path with a scalar head);
  (a4) mode 1 with acc and g offset differently (the 4-byte path);
  (b)  mode 2 (g = acc + g), 12 B per element, against ``torch.add(acc, g, out=g)``;
  (c)  with --step: the whole ResNet-50 training step (bf16) at accum_steps 1 and 4 with micro-batch --batch, in ms per
       image.
Each sample is one event pair around ``--reps`` back-to-back launches; the variants alternate within a round and the
figure is the median over the rounds, per launch.  The implied bytes/s divide the bytes a mode has to move by that time;
back-to-back launches over the same 0.2 GB of arrays run partly out of the 256 MiB Infinity Cache, so they are not HBM
rates.  ``kernel_not_slower``: the kernel's median is at most the torch form's median plus the spread (max - min) of
the torch arm's rounds.  Prints one JSON line and appends it to --log.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20, help="launches per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time whole ResNet-50 training steps")
    ap.add_argument("--batch", type=int, default=256, help="micro-batch of the timed steps")
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "accum_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops import accum

    assert torch.cuda.is_available(), "accum_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    total = sum(p.numel() for p in nets_factory.build("resnet_v1_50", num_classes=1000).parameters()
                if p.requires_grad)

    def pair(off_acc=0, off_g=0):
        acc = torch.randn(total + 4, device=dev) * 1e-2
        g = torch.randn(total + 4, device=dev) * 1e-2
        return acc[off_acc:off_acc + total], g[off_g:off_g + total]

    # the kernel and the torch form compute the same thing (same seeded inputs, at the timed size)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for mode in (accum.ADD, accum.FOLD):
        (ak, gk), (at, gt) = pair(), pair()
        at.copy_(ak)
        gt.copy_(gk)
        accum.grad_accum(ak, gk, mode, flag)
        if mode == accum.ADD:
            at.add_(gt)
            gt.zero_()
        else:
            torch.add(at, gt, out=gt)
        assert torch.equal(ak, at) and torch.equal(gk, gt) and int(flag.item()) == 0

    ka, kg = pair()
    k1a, k1g = pair(1, 1)
    k4a, k4g = pair(1, 3)
    ta, tg = pair()
    fa, fg = pair()
    fta, ftg = pair()

    def torch_add():
        ta.add_(tg)
        tg.zero_()

    res = _alternate({
        "a_kernel_add": lambda: accum.grad_accum(ka, kg, accum.ADD, flag),
        "a_torch_add_zero": torch_add,
        "a1_kernel_add_head": lambda: accum.grad_accum(k1a, k1g, accum.ADD, flag),
        "a4_kernel_add_4byte": lambda: accum.grad_accum(k4a, k4g, accum.ADD, flag),
        "b_kernel_fold": lambda: accum.grad_accum(fa, fg, accum.FOLD, flag),
        "b_torch_add_out": lambda: torch.add(fta, ftg, out=ftg),
    }, args.rounds, args.reps, args.warmup)
    nbytes = {"a_kernel_add": 16.0, "a_torch_add_zero": 16.0, "a1_kernel_add_head": 16.0, "a4_kernel_add_4byte": 16.0,
              "b_kernel_fold": 12.0, "b_torch_add_out": 12.0}
    out = dict(elements=total, rounds=args.rounds, reps=args.reps)
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        out[k + "_GBps"] = round(nbytes[k] * total / (med * 1e-3) / 1e9, 1)
    for tag, kern, ref in (("a", "a_kernel_add", "a_torch_add_zero"), ("b", "b_kernel_fold", "b_torch_add_out")):
        spread = res[ref][2] - res[ref][1]
        out[tag + "_torch_over_kernel"] = round(res[ref][0] / res[kern][0], 3)
        out[tag + "_torch_spread_ms"] = round(spread, 4)
        out[tag + "_kernel_not_slower"] = bool(res[kern][0] <= res[ref][0] + spread)

    if args.step:
        del ka, kg, k1a, k1g, k4a, k4g, ta, tg, fa, fg, fta, ftg
        steps = {}
        for n in (1, 4):
            torch.manual_seed(0)
            net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
            steps[n] = TrainStep(net, optimizer="momentum", lr=0.01, momentum=0.9, accum_steps=n)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        fns = {"accum_1": lambda: steps[1](x, y), "accum_4": lambda: steps[4]([x] * 4, [y] * 4)}
        sres = _alternate(fns, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for n, k in ((1, "accum_1"), (4, "accum_4")):
            med, lo, hi = sres[k]
            out["step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
            out["step_%s_ms_per_image" % k] = round(med / (n * args.batch), 5)
        out["per_image_accum_4_over_1"] = round(sres["accum_4"][0] / 4 / sres["accum_1"][0], 4)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
