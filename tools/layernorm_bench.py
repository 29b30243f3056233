#!/usr/bin/env python3
"""Cost of the channel LayerNorm, layer scale + residual and GELU kernels at ConvNeXt-T's bf16 shapes for batch 256,
with the method of tools/lamb_bench.py: HIP events around ``--reps`` back-to-back calls, the arms alternating within a
round, medians with min - max over the rounds.

Arms per shape M x C: (a) ops.layernorm.channel_layer_norm forward and backward against torch.nn.functional.layer_norm;
(b) ops.layernorm.scale_residual forward and backward against scale_residual_torch; (c) ops.activation gelu against
torch.nn.functional.gelu on the 802816 x 384 hidden tensor; every row next to a plain bf16 copy of the same tensor
(4 bytes per element), the rate the byte models are held to.  A backward is autograd.grad on a graph kept from one
forward, so both arms pay the same autograd cost.  With --step, (d): a whole convnext_tiny training step on this path
against the same model with the three ops forced to their torch forms.  Tensors under 256 MB stay in the Infinity Cache
between back-to-back launches: those rows' rates are cache rates, and the log says which they are.
Appends to --log; the expectations go into the log before anything runs.  Prints one JSON line at the end."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

SHAPES = [(802816, 96), (200704, 192), (50176, 384), (12544, 768)]  # stages 1 - 4 at batch 256
HIDDEN = (802816, 384)
N = 256  # samples: the rows of stochastic depth's per-sample factor
# bytes per element that each op has to move in bf16
BYTES = {"ln_fwd": 4, "ln_bwd": 6, "sr_fwd": 6, "sr_bwd": 6, "gelu_fwd": 4, "gelu_bwd": 6}
EXPECT = """expectations (none of this had been measured when they were written)
 (i)  every kernel takes no longer than its ATen arm (median against median)
 (ii) every kernel is within 1.5x of its byte model at the rate a plain bf16 copy of the same tensor reaches in the
      same run: ln_fwd 4 B, ln_bwd 6 B, sr_fwd 6 B, sr_bwd 6 B, gelu_fwd 4 B, gelu_bwd 6 B per element, the copy 4 B
 (iii) with --step: the convnext_tiny step on the kernels takes no longer than with the three ops in their torch forms
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step", action="store_true", help="also time whole convnext_tiny training steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "layernorm_bench.log"))
    args = ap.parse_args()

    import torch
    import torch.nn.functional as tF

    from distributed_tensorflow_models_amd.ops import activation as A
    from distributed_tensorflow_models_amd.ops import layernorm as LN

    assert torch.cuda.is_available(), "layernorm_bench needs a GPU"
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(EXPECT)
    rows, miss_i, miss_ii, recs = [], [], [], []

    def measure(M, C, op, fwd_kernel, fwd_torch, leaves_k, leaves_t):
        """Times forward and backward of one op; leaves_*: the tensors whose gradients the backward forms."""
        x = leaves_k[0]
        dy = torch.randn(x.shape, device=dev).to(bf)
        src, dst = torch.randn(M, C, device=dev).to(bf), torch.empty(M, C, device=dev, dtype=bf)
        yk, yt = fwd_kernel(), fwd_torch()

        def nograd(fn):
            def call():
                with torch.no_grad():
                    fn()
            return call

        for name, k, t in ((op + "_fwd", nograd(fwd_kernel), nograd(fwd_torch)),
                           (op + "_bwd", lambda: torch.autograd.grad(yk, leaves_k, dy, retain_graph=True),
                            lambda: torch.autograd.grad(yt, leaves_t, dy, retain_graph=True))):
            r = _alternate(dict(kernel=k, torch=t, copy=lambda: dst.copy_(src)), args.rounds, args.reps, args.warmup)
            kk, tt, cp = r["kernel"], r["torch"], r["copy"]
            model = cp[0] * BYTES[name] / 4.0
            met_i, met_ii = kk[0] <= tt[0], kk[0] <= 1.5 * model
            cached = x.numel() * 2 < 256e6
            if not met_i:
                miss_i.append("%s %dx%d (torch / kernel %.2f)" % (name, M, C, tt[0] / kk[0]))
            if not met_ii:
                miss_ii.append("%s %dx%d (kernel / byte model %.2f)" % (name, M, C, kk[0] / model))
            recs.append(dict(op=name, M=M, C=C, kernel_ms=kk, torch_ms=tt, copy_ms=cp, i_met=bool(met_i),
                             ii_met=bool(met_ii), in_cache=bool(cached)))
            ms = "%.4f (%.4f - %.4f)"
            rows.append(("| %s | %d x %d | " + " | ".join([ms] * 3) + " | %.2f | %.2f | %.0f | %s |")
                        % ((name, M, C) + kk + tt + cp + (tt[0] / kk[0], kk[0] / model,
                                                          BYTES[name] * M * C / kk[0] / 1e6,
                                                          "cache" if cached else "HBM")))

    for M, C in SHAPES + [HIDDEN]:
        torch.manual_seed(0)
        x = torch.randn(N, M // N, C, device=dev).to(bf).requires_grad_()
        if (M, C) != HIDDEN:
            g32, b32 = (torch.randn(C, device=dev).requires_grad_() for _ in range(2))
            g16, b16 = (t.detach().to(bf).requires_grad_() for t in (g32, b32))
            measure(M, C, "ln", lambda: LN.channel_layer_norm(x, g32, b32, 1e-6),
                    lambda: tF.layer_norm(x, (C,), g16, b16, 1e-6), (x, g32, b32), (x, g16, b16))
            r = torch.randn(N, M // N, C, device=dev).to(bf).requires_grad_()
            s = (torch.rand(N, device=dev) >= 0.1).float() / 0.9
            measure(M, C, "sr", lambda: LN.scale_residual(x, r, g32, s), lambda: LN.scale_residual_torch(x, r, g32, s),
                    (r, g32), (r, g32))
            del r
        else:
            measure(M, C, "gelu", lambda: A.gelu(x), lambda: tF.gelu(x), (x,), (x,))
        del x
        torch.cuda.empty_cache()

    say("| op | M x C | kernel ms (min - max) | torch ms (min - max) | bf16 copy ms (min - max) | torch / kernel | "
        "kernel / byte model | kernel GB/s | tensor lives in |")
    say("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        say(r)
    say("(i) %s" % ("met on every row" if not miss_i else "NOT met on: " + ", ".join(miss_i)))
    say("(ii) %s" % ("met on every row" if not miss_ii else "NOT met on: " + ", ".join(miss_ii)))
    out = dict(rounds=args.rounds, reps=args.reps, i_met=not miss_i, ii_met=not miss_ii, rows=recs)

    if args.step:
        from distributed_tensorflow_models_amd.engine import TrainStep
        from distributed_tensorflow_models_amd.models import nets_factory
        xb = torch.randn(args.batch, 224, 224, 3, device=dev).to(bf)
        yb = torch.randint(0, 1000, (args.batch,), device=dev)
        kernel_path, gpu = LN._kernel_path, A._gpu

        def forced(step):
            def call():  # the three ops take their torch forms while this arm's step is built and run
                LN._kernel_path, A._gpu = (lambda *a: False), (lambda t: False)
                try:
                    return step(xb, yb)
                finally:
                    LN._kernel_path, A._gpu = kernel_path, gpu
            return call

        steps = {}
        for name in ("kernels", "torch_forms"):
            torch.manual_seed(0)
            step = TrainStep(nets_factory.build("convnext_tiny", num_classes=1000).to(dev), optimizer="lamb", lr=0.001,
                             momentum=0.9)
            steps[name] = forced(step) if name == "torch_forms" else (lambda step=step: step(xb, yb))
        sres = _alternate(steps, 5, 3, 2)
        for name, r in sres.items():
            out["step_" + name] = dict(median=round(r[0], 3), min=round(r[1], 3), max=round(r[2], 3))
            say("step convnext_tiny batch %d, %s: %.3f ms (%.3f - %.3f)" % ((args.batch, name) + r))
        out["iii_met"] = bool(sres["kernels"][0] <= sres["torch_forms"][0])
        say("(iii) %s: torch forms / kernels %.3f" % ("met" if out["iii_met"] else "NOT met",
                                                      sres["torch_forms"][0] / sres["kernels"][0]))
    say(json.dumps(out))


if __name__ == "__main__":
    main()
