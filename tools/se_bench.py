#!/usr/bin/env python3
"""The squeeze-and-excitation kernels on the four SE tails of SE-ResNeXt-50 (224x224, batch 64): bf16, with the
shortcut as residual and ReLU, C / 16 hidden units.

Per layer, forward and forward + backward, with HIP events on one GPU:
  kernel  ops.se.squeeze_excite: the kernels of csrc/kernels/se.hip, automatic slabs;
  torch   ops.se.squeeze_excite_torch: the same definition as torch ops on the device, autograd's own backward;
  copy    one device copy of x (2 B read + 2 B written per element): the byte yardstick of this run.
Method of tools/optim_bench.py: each sample is one event pair around ``--reps`` back-to-back calls, the arms alternate
within a round, the figure is the median over the rounds with min - max.  With --step one eager se_resnext_50_32x4d
training step next to resnext_50_32x4d, and the first and last loss of a 20-step run of the se_resnext50 trainer in a
child process.  The expectations go into the log before the timed runs, one JSON line after them.  Arrays under 256 MB
looped back to back run partly out of the Infinity Cache: the copy arm shares that advantage, an absolute GB/s figure
does not transfer to a training step.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

LAYERS = [(56, 256), (28, 512), (14, 1024), (7, 2048)]  # (H = W, C)
# bytes per element of the big tensors, from the launch table: forward x twice, residual, y; backward dy, y, x in the
# sums pass and dy, y, dx, dresidual in the apply pass; the copy moves 4
FWD_BYTES, BWD_BYTES, COPY_BYTES = 8, 14, 4
EXPECT = """expectations (none of this had been measured when they were written)
 (i)   kernel is faster than torch on every layer and direction, by more than the torch arm's min - max spread
 (ii)  forward within %.1f x the copy arm (%d B against %d B per element), forward + backward within %.1f x (%d B)
 (iii) bench.py's ResNet-50 step is unchanged (measured apart from this tool: the step launches none of these kernels)
""" % (FWD_BYTES / COPY_BYTES, FWD_BYTES, COPY_BYTES, (FWD_BYTES + BWD_BYTES) / COPY_BYTES, FWD_BYTES + BWD_BYTES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step", action="store_true", help="also time eager training steps and run the trainer")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "se_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.ops.se import squeeze_excite, squeeze_excite_torch

    assert torch.cuda.is_available(), "se_bench needs a GPU"
    dev, N = torch.device("cuda", 0), args.batch
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(EXPECT)
    layers, rows, miss_i, miss_ii = [], [], [], []
    for H, C in LAYERS:
        Cr = C // 16
        torch.manual_seed(0)
        x, res, dy = (torch.randn(N, H, H, C, device=dev).to(torch.bfloat16).requires_grad_(i < 2) for i in range(3))
        params = [(torch.randn(*shape, device=dev) * scale).requires_grad_() for shape, scale in
                  (((Cr, C), C ** -0.5), ((Cr,), 1.0), ((C, Cr), Cr ** -0.5), ((C,), 1.0))]
        xc = torch.empty_like(x)
        leaves = [x, res] + params

        def fwd(fn):
            def call():
                with torch.no_grad():
                    fn(x, *params, residual=res, relu=True)
            return call

        def fwd_bwd(fn):
            def call():
                for t in leaves:
                    t.grad = None
                fn(x, *params, residual=res, relu=True).backward(dy)
            return call

        copy = lambda: xc.copy_(x.detach())  # noqa: E731
        rec = dict(H=H, C=C, Cr=Cr)
        for d, make, model in (("fwd", fwd, FWD_BYTES / COPY_BYTES),
                               ("fwd+bwd", fwd_bwd, (FWD_BYTES + BWD_BYTES) / COPY_BYTES)):
            r = _alternate(dict(kernel=make(squeeze_excite), torch=make(squeeze_excite_torch), copy=copy), args.rounds,
                           args.reps, args.warmup)
            k, t, cp = r["kernel"], r["torch"], r["copy"]
            i_met, ii_met = k[0] < t[0] - (t[2] - t[1]), k[0] <= model * cp[0]
            rec[d] = {a: dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4)) for a, v in r.items()}
            rec[d].update(torch_over_kernel=round(t[0] / k[0], 2), kernel_over_copy=round(k[0] / cp[0], 2),
                          byte_model=model, i_met=bool(i_met), ii_met=bool(ii_met))
            tag = "%dx%dx%d %s" % (H, H, C, d)
            if not i_met:
                miss_i.append("%s (%.2f)" % (tag, t[0] / k[0]))
            if not ii_met:
                miss_ii.append("%s (%.2f against %.1f)" % (tag, k[0] / cp[0], model))
            ms = "%.4f (%.4f - %.4f)"
            rows.append(("| %dx%dx%d | %s | " + " | ".join([ms] * 3) + " | %.2f | %.2f | %.1f | %s |") % (
                (H, H, C, d) + k + t + cp + (t[0] / k[0], k[0] / cp[0], model, "met" if ii_met else "not met")))
        layers.append(rec)
    say("| layer | dir | kernel ms (min - max) | torch ms (min - max) | copy ms (min - max) | torch / kernel | "
        "kernel / copy | byte model | (ii) |")
    say("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        say(r)
    say("(i) %s" % ("met on every layer and direction" if not miss_i else
                    "NOT met on (torch / kernel): " + ", ".join(miss_i)))
    say("(ii) %s" % ("met on every layer and direction" if not miss_ii else
                     "NOT met on (kernel / copy): " + ", ".join(miss_ii)))
    out = dict(batch=N, rounds=args.rounds, reps=args.reps, i_met=not miss_i, ii_met=not miss_ii, layers=layers)

    if args.step:
        from distributed_tensorflow_models_amd.engine import TrainStep
        from distributed_tensorflow_models_amd.models import nets_factory
        xb = torch.randn(N, 224, 224, 3, device=dev).to(torch.bfloat16)
        yb = torch.randint(0, 1000, (N,), device=dev)
        steps = {}
        for name in ("se_resnext_50_32x4d", "resnext_50_32x4d"):
            torch.manual_seed(0)
            step = TrainStep(nets_factory.build(name, num_classes=1000).to(dev), optimizer="momentum", lr=0.01,
                             momentum=0.9)
            steps[name] = lambda step=step: step(xb, yb)
        for name, r in _alternate(steps, 5, 4, 3).items():
            out["step_" + name] = dict(median=round(r[0], 3), min=round(r[1], 3), max=round(r[2], 3))
            say("step %s batch %d eager: %.3f ms (%.3f - %.3f)" % ((name, N) + r))
        del steps, step
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory() as train_dir:
            cmd = [sys.executable, "-m", "distributed_tensorflow_models_amd.trainers.imagenet_se_resnext50_bsp",
                   "--synthetic_data", "--max_steps", "20", "--batch_size", "32", "--train_dir", train_dir]
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        losses = [float(v) for v in re.findall(r"step \d+ \(global_step \d+\), loss = (\S+) ", p.stdout)]
        finite = len(losses) == 20 and all(v == v and abs(v) != float("inf") for v in losses)
        out["trainer"] = dict(rc=p.returncode, losses=losses, finite=finite)
        say("trainer se_resnext50, 20 steps at batch 32: rc %d, %d loss lines, loss %s at step 0, %s at step 19, "
            "peak %s, %s" % (p.returncode, len(losses), losses[0] if losses else None, losses[-1] if losses else None,
                             max(losses) if losses else None,
                             "finite throughout" if finite else "NOT finite throughout"))
        if p.returncode != 0:
            say(p.stdout[-2000:])
    say(json.dumps(out))


if __name__ == "__main__":
    main()
