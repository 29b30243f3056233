#!/usr/bin/env python3
"""Cost of the fused fake-quantisation passes against the torch-op path, with the method of tools/adam_bench.py.

(a) ONE activation quantiser in training, forward and backward: the fused passes (range + finalize + apply, then the
    straight-through backward: csrc/kernels/fakequant.hip) against ``compat.quantize.quantize_activations`` (aminmax,
    the moving-average ops, ATen's fake-quant op and its backward) on the same bf16 tensor, at MobileNet v1 1.0's
    largest activation at batch 64 ([64, 112, 112, 64]) and its smallest ([64, 7, 7, 1024]).  The fused forward reads
    x twice (range, apply) and writes y; its backward reads x and dy and writes dx: 10 bytes per bf16 element.
(b) ONE whole MobileNet v1 1.0 training step (224 x 224, batch 64, momentum, ``quantize`` with quant_delay 0) in three
    forms: unfused eager, fused eager, fused captured into a hipGraph and replayed.

Each sample is one event pair around ``--reps`` back-to-back calls; the variants alternate within a round and the
figure is the median over the rounds, per call.  Prints one JSON line.
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
    ap.add_argument("--reps", type=int, default=10, help="calls per timed sample of one quantiser")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step measurement")
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.compat import quantize as Q
    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops import fakequant as FQ

    assert torch.cuda.is_available(), "fakequant_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out = dict(rounds=args.rounds, reps=args.reps, batch=args.batch)

    # ---- (a) one activation quantiser ----------------------------------------------------------------------------
    def one_quantiser(shape):
        x = (torch.randn(shape, device=dev) * 2.0 + 1.0).to(torch.bfloat16).requires_grad_()
        dy = torch.randn(shape, device=dev).to(torch.bfloat16)
        store = {}

        def var_fn(tag):
            def fn(name, init):
                key = tag + name
                if key not in store:
                    store[key] = torch.nn.Parameter(torch.tensor(float(init), device=dev), requires_grad=False)
                return store[key]
            return fn

        cfg_f, cfg_u = Q.QuantConfig(fused=True), Q.QuantConfig()

        def fused():
            return torch.autograd.grad(Q.quantize_activations(x, var_fn("f/"), cfg_f, True), x, dy)[0]

        def unfused():
            return torch.autograd.grad(Q.quantize_activations(x, var_fn("u/"), cfg_u, True), x, dy)[0]

        res = _alternate({"fused": fused, "unfused": unfused}, args.rounds, args.reps, args.warmup)
        n = x.numel()
        r = dict(elements=n, grid=FQ.grid_size(n, torch.bfloat16))
        for k, (med, lo, hi) in res.items():
            r[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        r["fused_GBps"] = round(10.0 * n / (res["fused"][0] * 1e-3) / 1e9, 1)
        r["unfused_over_fused"] = round(res["unfused"][0] / res["fused"][0], 3)
        return r

    out["a_largest_64x112x112x64"] = one_quantiser((args.batch, 112, 112, 64))
    out["a_smallest_64x7x7x1024"] = one_quantiser((args.batch, 7, 7, 1024))

    # ---- (b) one whole training step -----------------------------------------------------------------------------
    if not args.no_step:
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)

        def make(fused, graph):
            torch.manual_seed(0)
            cfg = Q.QuantConfig(quant_delay=0, fused=fused)
            model = nets_factory.build("mobilenet_v1", num_classes=1000, quantize=cfg).to(dev)
            step = TrainStep(model, optimizer="momentum", lr=0.01, momentum=0.9, use_graph=graph)
            return lambda: step(x, y)

        forms = {"unfused_eager": make(False, False), "fused_eager": make(True, False),
                 "fused_captured": make(True, True)}
        res = _alternate(forms, args.step_rounds, args.step_reps, args.warmup)
        r = dict(rounds=args.step_rounds, reps=args.step_reps)
        for k, (med, lo, hi) in res.items():
            r[k + "_ms"] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        base = res["unfused_eager"][0]
        r["unfused_over_fused_eager"] = round(base / res["fused_eager"][0], 3)
        r["unfused_over_fused_captured"] = round(base / res["fused_captured"][0], 3)
        out["b_mobilenet_v1_step"] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
