#!/usr/bin/env python3
"""The attention kernels on BoTNet-50's two blocks (batch 64, 4 heads, d = 128, L = 196 and 49) and on one long row
(batch 16, 8 heads, d = 64, L = 1024): bf16, q, k, v as the thirds of one fused qkv tensor.

Per shape, forward and forward + backward, with HIP events on one GPU:
  kernel  ops.attention.mhsa: the kernels of csrc/kernels/attention.hip;
  torch   ops.attention.mhsa_torch: two batched GEMMs and a softmax on the device, autograd's own backward;
  sdpa    torch.nn.functional.scaled_dot_product_attention on the same bf16 tensors;
  copy    a device copy of the op's bytes: forward q, k, v, o (two tensors copied = four passes), forward + backward
          adds dO, dq, dk, dv and the reread of q, k, v, o (six tensors copied = twelve passes).
Method of tools/optim_bench.py: each sample is one event pair around ``--reps`` back-to-back calls, the arms alternate
within a round, the figure is the median over the rounds with min - max.  With --step one eager botnet_50 training
step next to se_resnet_50, and the first, peak and last loss of a 20-step run of the botnet50 trainer in a child
process.  The expectations go into the log before the timed runs, one JSON line after them.  Arrays under 256 MB
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

SHAPES = [(64, 196, 4, 128), (64, 49, 4, 128), (16, 1024, 8, 64)]  # (N, L, heads, d)
# matrix products of L x L x d per (n, head): forward S and P V; backward S, dP, dV, dK in the dK/dV kernel and S, dP,
# dQ in the dQ kernel
FWD_GEMMS, BWD_GEMMS = 2, 7
EXPECT = """expectations (none of this had been measured when they were written)
 (i)   kernel is faster than torch on every row, by more than the torch arm's min - max spread
 (ii)  kernel against sdpa is reported whatever it is
 (iii) kernel over copy is reported next to the op's flop count: L = 1024 is arithmetic-bound, L = 49 launch-bound
 (iv)  bench.py's ResNet-50 step is unchanged (measured apart from this tool: the step launches none of these kernels)
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", action="store_true", help="also time eager training steps and run the trainer")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "attention_bench.log"))
    args = ap.parse_args()

    import torch
    import torch.nn.functional as tF

    from distributed_tensorflow_models_amd.ops.attention import mhsa, mhsa_torch

    assert torch.cuda.is_available(), "attention_bench needs a GPU"
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    def sdpa(q, k, v, heads):
        N, L, C = q.shape
        qh, kh, vh = (t.reshape(N, L, heads, C // heads).transpose(1, 2) for t in (q, k, v))
        return tF.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(N, L, C)

    say(EXPECT)
    shapes, rows, miss = [], [], []
    for N, L, heads, d in SHAPES:
        C = heads * d
        torch.manual_seed(0)
        qkv = torch.randn(N, L, 3 * C, device=dev).to(torch.bfloat16).requires_grad_()
        do = torch.randn(N, L, C, device=dev).to(torch.bfloat16)
        src = torch.zeros(6, N, L, C, device=dev, dtype=torch.bfloat16)
        dst = torch.empty_like(src)

        def fwd(fn):
            def call():
                with torch.no_grad():
                    fn(*qkv.split(C, -1), heads)
            return call

        def fwd_bwd(fn):
            def call():
                qkv.grad = None
                fn(*qkv.split(C, -1), heads).backward(do)
            return call

        rec = dict(N=N, L=L, heads=heads, d=d)
        for name, make, copies, gemms in (("fwd", fwd, 2, FWD_GEMMS), ("fwd+bwd", fwd_bwd, 6, FWD_GEMMS + BWD_GEMMS)):
            arms = dict(kernel=make(mhsa), torch=make(mhsa_torch), sdpa=make(sdpa),
                        copy=lambda copies=copies: dst[:copies].copy_(src[:copies]))
            try:
                arms["sdpa"]()
                torch.cuda.synchronize()
            except Exception as e:  # a build without a fused backend for this shape
                say("sdpa arm unavailable at %r %s: %s" % ((N, L, heads, d), name, str(e).splitlines()[0]))
                del arms["sdpa"]
            r = _alternate(arms, args.rounds, args.reps, args.warmup)
            k, t, cp = r["kernel"], r["torch"], r["copy"]
            s = r.get("sdpa", (float("nan"),) * 3)
            gflop = 2.0 * gemms * N * heads * L * L * d / 1e9
            met = k[0] < t[0] - (t[2] - t[1])
            rec[name] = {a: dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4)) for a, v in r.items()}
            rec[name].update(torch_over_kernel=round(t[0] / k[0], 2), sdpa_over_kernel=round(s[0] / k[0], 2),
                             kernel_over_copy=round(k[0] / cp[0], 2), gflop=round(gflop, 2),
                             tflops=round(gflop / k[0], 1), i_met=bool(met))
            if not met:
                miss.append("%dx%dx%dx%d %s (%.2f)" % (N, L, heads, d, name, t[0] / k[0]))
            ms = "%.4f (%.4f - %.4f)"
            rows.append(("| %d x %d x %d x %d | %s | " + " | ".join([ms] * 4) + " | %.2f | %.2f | %.2f | %.1f | %.1f |")
                        % ((N, L, heads, d, name) + k + t + s + cp + (t[0] / k[0], s[0] / k[0], k[0] / cp[0], gflop,
                                                                      gflop / k[0])))
        shapes.append(rec)
    say("| N x L x heads x d | dir | kernel ms (min - max) | torch ms (min - max) | sdpa ms (min - max) | "
        "copy ms (min - max) | torch / kernel | sdpa / kernel | kernel / copy | GFLOP | kernel TFLOP/s |")
    say("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        say(r)
    say("(i) %s" % ("met on every row" if not miss else "NOT met on (torch / kernel): " + ", ".join(miss)))
    out = dict(rounds=args.rounds, reps=args.reps, i_met=not miss, shapes=shapes)

    if args.step:
        from distributed_tensorflow_models_amd.engine import TrainStep
        from distributed_tensorflow_models_amd.models import nets_factory
        xb = torch.randn(64, 224, 224, 3, device=dev).to(torch.bfloat16)
        yb = torch.randint(0, 1000, (64,), device=dev)
        steps = {}
        for name in ("botnet_50", "se_resnet_50"):
            torch.manual_seed(0)
            step = TrainStep(nets_factory.build(name, num_classes=1000).to(dev), optimizer="momentum", lr=0.01,
                             momentum=0.9)
            steps[name] = lambda step=step: step(xb, yb)
        for name, r in _alternate(steps, 5, 4, 3).items():
            out["step_" + name] = dict(median=round(r[0], 3), min=round(r[1], 3), max=round(r[2], 3))
            say("step %s batch 64 eager: %.3f ms (%.3f - %.3f)" % ((name,) + r))
        del steps, step
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory() as train_dir:
            cmd = [sys.executable, "-m", "distributed_tensorflow_models_amd.trainers.imagenet_botnet50_bsp",
                   "--synthetic_data", "--max_steps", "20", "--batch_size", "32", "--train_dir", train_dir]
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        losses = [float(v) for v in re.findall(r"step \d+ \(global_step \d+\), loss = (\S+) ", p.stdout)]
        finite = len(losses) == 20 and all(v == v and abs(v) != float("inf") for v in losses)
        out["trainer"] = dict(rc=p.returncode, losses=losses, finite=finite)
        say("trainer botnet50, 20 steps at batch 32: rc %d, %d loss lines, loss %s at step 0, %s at step 19, "
            "peak %s, %s" % (p.returncode, len(losses), losses[0] if losses else None, losses[-1] if losses else None,
                             max(losses) if losses else None,
                             "finite throughout" if finite else "NOT finite throughout"))
        if p.returncode != 0:
            say(p.stdout[-2000:])
    say(json.dumps(out))


if __name__ == "__main__":
    main()
