#!/usr/bin/env python3
"""Group norm on ResNet-50's norm shapes (bf16, batch 64, G = 32, affine + ReLU): forward and forward + backward.

Arms, with HIP events on one GPU:
  kernel  ops.groupnorm.group_norm: the slab-split kernels of csrc/kernels/groupnorm.hip, automatic slabs;
  torch   ops.groupnorm.group_norm_torch: the same definition as torch ops on the device;
  copy    one device-to-device copy y <- x: it reads the x bytes and writes the y bytes, two tensor passes, the byte
          floor of a forward that could keep x on chip (forward only);
and, at G == C on the instance-normalised shapes of the GAN models, ops.activation.instance_norm (dtm_instnorm_fwd /
dtm_instnorm_bwd) against group_norm(groups=C).
Method of tools/optim_bench.py: each sample is one event pair around ``--reps`` back-to-back calls, the arms alternate
within a round, the figure is the median over the rounds with min - max.  The expectations go into the log before the
timed runs, one JSON line after them.  Arrays under 256 MB looped back to back run partly out of the Infinity Cache:
the copy arm shares that advantage, an absolute GB/s figure does not transfer to a training step.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

SHAPES = [(56, 64), (56, 256), (28, 512), (14, 1024), (7, 2048)]  # (H = W, C)
# (iii): (batch, H = W, C) of instance-normalised activations at 256x256 inputs.  gans.cyclegan_generator_resnet
# (num_filters = 64): encoder_0 / decoder2 at full resolution, encoder_1 / decoder1 at half, encoder_2 and the residual
# blocks at a quarter; gans.pix2pix_generator: encoder2 (PIX2PIX_BLOCKS[2] after three stride-2 convs).  Batch 1 cuts a
# sample into the most slabs.  The last row is the shape of the group-norm pull request's log.
INSTANCE = [(n, h, c) for h, c in ((256, 64), (128, 128), (64, 256), (32, 256)) for n in (1, 16)] + [(64, 64, 128)]
EXPECT = """expectations (none of this had been measured)
 (i)   kernel is faster than torch on every shape, forward and forward + backward, by more than torch's min - max spread
 (ii)  byte model of the forward: three tensor passes against the copy's two, kernel / copy = 1.5; the measured
       ratio is reported next to it
 (iii) at G == C the new path is reported against dtm_instnorm_fwd / dtm_instnorm_bwd both ways; it replaces them if on
       every row its median is not slower by more than the row's own min - max spread of the two arms
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "groupnorm_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.ops import _lib
    from distributed_tensorflow_models_amd.ops.activation import instance_norm
    from distributed_tensorflow_models_amd.ops.groupnorm import auto_slab_pixels, group_norm, group_norm_torch

    assert torch.cuda.is_available(), "groupnorm_bench needs a GPU"
    _lib.lib()
    dev, N = torch.device("cuda", 0), args.batch
    log = open(args.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    def tensors(H, C, N=N):
        x = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16).requires_grad_()
        gamma = (torch.rand(C, device=dev) + 0.5).requires_grad_()
        beta = torch.randn(C, device=dev).requires_grad_()
        return x, gamma, beta, torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)

    def fwd_bwd(fn, x, gamma, beta, dy):
        def run():
            x.grad = gamma.grad = beta.grad = None
            fn().backward(dy)
        return run

    say(EXPECT)
    rows, shapes, i_met = [], [], True
    for H, C in SHAPES:
        x, gamma, beta, dy = tensors(H, C)
        yc = torch.empty_like(x)
        kern = lambda: group_norm(x, 32, gamma, beta, 1e-5, relu=True)  # noqa: E731
        comp = lambda: group_norm_torch(x, 32, gamma, beta, 1e-5, relu=True)  # noqa: E731
        with torch.no_grad():
            f = _alternate(dict(kernel=kern, torch=comp, copy=lambda: yc.copy_(x)), args.rounds,
                           args.reps, args.warmup)
        b = _alternate(dict(kernel=fwd_bwd(kern, x, gamma, beta, dy), torch=fwd_bwd(comp, x, gamma, beta, dy)),
                       args.rounds, args.reps, args.warmup)
        met = all(r["kernel"][0] < r["torch"][0] - (r["torch"][2] - r["torch"][1]) for r in (f, b))
        i_met = i_met and met
        shapes.append(dict(H=H, C=C, slab_pixels=auto_slab_pixels(N, H * H, C), i_met=bool(met),
                           fwd={k: [round(t, 4) for t in v] for k, v in f.items()},
                           fwd_bwd={k: [round(t, 4) for t in v] for k, v in b.items()},
                           kernel_over_copy=round(f["kernel"][0] / f["copy"][0], 2)))
        rows.append("| %dx%dx%d | %.4f (%.4f - %.4f) | %.4f (%.4f - %.4f) | %.4f | %.2f | 1.5 | %.4f (%.4f - %.4f) | "
                    "%.4f (%.4f - %.4f) |" % ((H, H, C) + f["kernel"] + f["torch"] + (
                        f["copy"][0], f["kernel"][0] / f["copy"][0]) + b["kernel"] + b["torch"]))
    say("| shape | fwd kernel ms (min - max) | fwd torch ms (min - max) | copy ms | kernel / copy | model | "
        "fwd+bwd kernel ms (min - max) | fwd+bwd torch ms (min - max) |")
    say("|---|---|---|---|---|---|---|---|")
    for r in rows:
        say(r)
    say("(i) %s" % ("met on every shape" if i_met else "NOT met on: " + ", ".join(
        "%dx%dx%d" % (s["H"], s["H"], s["C"]) for s in shapes if not s["i_met"])))
    say("(ii) kernel / copy against the model's 1.5: " + ", ".join(
        "%dx%dx%d %.2f" % (s["H"], s["H"], s["C"], s["kernel_over_copy"]) for s in shapes))

    say("(iii) G == C, bf16, affine + ReLU, eps 1e-6; ms median (min - max); "
        "spread = the larger min - max of the two arms")
    say("| batch | shape | slabs | pass | instnorm ms | groupnorm ms | groupnorm - instnorm | spread | within rule |")
    say("|---|---|---|---|---|---|---|---|---|")
    instance, iii_met = [], True
    for n, H, C in INSTANCE:
        x, gamma, beta, dy = tensors(H, C, n)
        old = lambda: instance_norm(x, gamma, beta, 1e-6, relu=True)  # noqa: E731
        new = lambda: group_norm(x, C, gamma, beta, 1e-6, relu=True)  # noqa: E731
        with torch.no_grad():
            f = _alternate(dict(instnorm=old, groupnorm=new), args.rounds, args.reps, args.warmup)
        b = _alternate(dict(instnorm=fwd_bwd(old, x, gamma, beta, dy), groupnorm=fwd_bwd(new, x, gamma, beta, dy)),
                       args.rounds, args.reps, args.warmup)
        slabs = -(-H * H // auto_slab_pixels(n, H * H, C))
        for name, r in (("fwd", f), ("fwd+bwd", b)):
            diff = r["groupnorm"][0] - r["instnorm"][0]
            spread = max(v[2] - v[1] for v in r.values())
            ok = diff <= spread
            iii_met = iii_met and ok
            say("| %d | %dx%dx%d | %d | %s | %.4f (%.4f - %.4f) | %.4f (%.4f - %.4f) | %+.4f | %.4f | %s |" % (
                (n, H, H, C, slabs, name) + r["instnorm"] + r["groupnorm"] + (diff, spread, "yes" if ok else "NO")))
        instance.append(dict(batch=n, H=H, C=C, slabs=slabs, fwd={k: [round(t, 4) for t in v] for k, v in f.items()},
                             fwd_bwd={k: [round(t, 4) for t in v] for k, v in b.items()}))
        del x, gamma, beta, dy
    say("(iii) rule %s" % ("met on every row" if iii_met else "NOT met"))
    say(json.dumps(dict(batch=N, rounds=args.rounds, reps=args.reps, i_met=bool(i_met), shapes=shapes,
                        iii_met=bool(iii_met), instance=instance)))


if __name__ == "__main__":
    main()
