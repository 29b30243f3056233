#!/usr/bin/env python3
"""The grouped 3x3 kernels on the seven grouped convs of ResNeXt-50 32x4d (224x224, batch 64).

Per layer and direction (forward, dgrad, wgrad), with HIP events on one GPU:
  hip   dtm_groupconv_*  (csrc/kernels/groupconv.hip), the entry points called directly;
  aten  torch.nn.functional.conv2d(groups=) on the same bf16 channels-last tensors; the two gradients come from
        autograd over that call, each timed on its own;
  copy  a device-to-device copy of the bytes the op must move (x + y, or x + dy): the byte floor of this run.
Method of tools/optim_bench.py: each sample is one event pair around ``--reps`` back-to-back launches, the arms
alternate within a round, the figure is the median over the rounds with min - max.  With --step one eager
resnext_50_32x4d training step at the same batch.  The expectations go into the log before the timed runs, one JSON
line after them.  Arrays under 256 MB looped back to back run partly out of the Infinity Cache: the copy arm shares
that advantage, an absolute GB/s figure does not transfer to a training step.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

# (H = W of the input, C, D, stride)
LAYERS = [(56, 128, 4, 1), (56, 256, 8, 2), (28, 256, 8, 1), (28, 512, 16, 2), (14, 512, 16, 1), (14, 1024, 32, 2),
          (7, 1024, 32, 1)]
EXPECT = """expectations (none of this had been measured when they were written)
 (i)   hip is faster than aten on every layer and direction, by more than the aten arm's min - max spread
 (ii)  forward and dgrad within 1.5 x the copy arm, wgrad within 2.5 x (what the depthwise tile kernels reached)
 (iii) bench.py's ResNet-50 step is unchanged (measured apart from this tool: the step launches none of these kernels)
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step", action="store_true", help="also time one eager ResNeXt-50 training step")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "groupconv_bench.log"))
    args = ap.parse_args()

    import torch
    import torch.nn.functional as TF

    from distributed_tensorflow_models_amd.ops import _lib
    from distributed_tensorflow_models_amd.ops.geometry import conv_geom
    from distributed_tensorflow_models_amd.ops.groupconv import GcArgs

    assert torch.cuda.is_available(), "groupconv_bench needs a GPU"
    dev, L, N = torch.device("cuda", 0), _lib.lib(), args.batch
    log = open(args.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(EXPECT)
    layers, rows, miss_i, miss_ii = [], [], [], []
    for H, C, D, st in LAYERS:
        g = conv_geom((N, H, H, C), (C, 3, 3, C), st, "SAME")
        a = GcArgs(N, H, H, C, D, g.P, g.Q, st, g.pad_h, g.pad_w)
        x = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
        dy = torch.randn(N, g.P, g.Q, C, device=dev).to(torch.bfloat16)
        w = torch.randn(C, 3, 3, D, device=dev)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.zeros_like(w)
        xc, dyc = torch.empty_like(x), torch.empty_like(dy)
        s, ar, p = _lib.stream_ptr(), ctypes.byref(a), _lib.ptr

        def op(name, *t):
            fn = getattr(L, name)

            def call():
                rc = fn(*[p(v) for v in t], ar, s)
                assert rc == 0, (name, rc)
            return call

        copy = lambda: (xc.copy_(x), dyc.copy_(dy))  # noqa: E731
        # ATen: NCHW views of the same channels-last memory; symmetric pad 1 gives the same output size
        xa = x.permute(0, 3, 1, 2).requires_grad_()
        wa = w.to(torch.bfloat16).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).requires_grad_()
        dya = dy.permute(0, 3, 1, 2)
        ya = TF.conv2d(xa, wa, None, st, 1, 1, C // D)
        assert ya.shape == dya.shape
        rec = dict(H=H, C=C, D=D, stride=st)
        for d, arms in (
                ("fwd", dict(hip=op("dtm_groupconv_fwd", x, w, y),
                             aten=lambda: TF.conv2d(xa.detach(), wa.detach(), None, st, 1, 1, C // D), copy=copy)),
                ("dgrad", dict(hip=op("dtm_groupconv_dgrad", dy, w, dx),
                               aten=lambda: torch.autograd.grad(ya, xa, dya, retain_graph=True), copy=copy)),
                ("wgrad", dict(hip=op("dtm_groupconv_wgrad", x, dy, dw),
                               aten=lambda: torch.autograd.grad(ya, wa, dya, retain_graph=True), copy=copy))):
            r = _alternate(arms, args.rounds, args.reps, args.warmup)
            rec[d] = {k: dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4)) for k, v in r.items()}
            hip, at, cp = r["hip"], r["aten"], r["copy"]
            i_met = hip[0] < at[0] - (at[2] - at[1])
            ii_met = hip[0] <= (2.5 if d == "wgrad" else 1.5) * cp[0]
            rec[d].update(aten_over_hip=round(at[0] / hip[0], 2), hip_over_copy=round(hip[0] / cp[0], 2),
                          i_met=bool(i_met), ii_met=bool(ii_met))
            tag = "%dx%dx%d D=%d s%d %s" % (H, H, C, D, st, d)
            if not i_met:
                miss_i.append("%s (%.2f)" % (tag, at[0] / hip[0]))
            if not ii_met:
                miss_ii.append("%s (%.2f)" % (tag, hip[0] / cp[0]))
            rows.append("| %dx%dx%d D=%d s%d | %s | %.4f (%.4f - %.4f) | %.4f (%.4f - %.4f) | %.4f | %.2f | %.2f |" % (
                H, H, C, D, st, d, hip[0], hip[1], hip[2], at[0], at[1], at[2], cp[0], at[0] / hip[0], hip[0] / cp[0]))
        layers.append(rec)
        del ya
    say("| layer | dir | hip ms (min - max) | aten ms (min - max) | copy ms | aten / hip | hip / copy |")
    say("|---|---|---|---|---|---|---|")
    for r in rows:
        say(r)
    say("(i) %s" % ("met on every layer and direction" if not miss_i else "NOT met on (aten / hip): " + ", ".join(miss_i)))
    say("(ii) %s" % ("met on every layer and direction" if not miss_ii else
                     "NOT met on (hip / copy): " + ", ".join(miss_ii)))
    out = dict(batch=N, rounds=args.rounds, reps=args.reps, i_met=not miss_i, ii_met=not miss_ii, layers=layers)

    if args.step:
        from distributed_tensorflow_models_amd.engine import TrainStep
        from distributed_tensorflow_models_amd.models import nets_factory
        xb = torch.randn(N, 224, 224, 3, device=dev).to(torch.bfloat16)
        yb = torch.randint(0, 1000, (N,), device=dev)
        torch.manual_seed(0)
        step = TrainStep(nets_factory.build("resnext_50_32x4d", num_classes=1000).to(dev), optimizer="momentum",
                         lr=0.01, momentum=0.9)
        r = _alternate({"eager": lambda: step(xb, yb)}, 5, 4, 3)["eager"]
        out["step_resnext_50_32x4d"] = dict(median=round(r[0], 3), min=round(r[1], 3), max=round(r[2], 3))
        say("step resnext_50_32x4d batch %d eager: %.3f ms (%.3f - %.3f)" % ((N,) + r))
    say(json.dumps(out))


if __name__ == "__main__":
    main()
