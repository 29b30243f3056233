#!/usr/bin/env python3
"""The int8 kernels (csrc/kernels/int8.hip) against the bf16 ones, and the integer evaluation against the bf16
fake-quant evaluation.  Writes profiles/int8_bench.log (``--log``).

(a) ``dtm_q8_conv`` (codes + bf16 copy out) against ``dtm_conv_fwd`` (``ops.nn.conv2d``, bias + relu fused) on
    MobileNet v1's pointwise shapes at batch 64, 14x14x512->512 and 7x7x1024->1024; ``dtm_q8_depthwise`` against
    ``dtm_depthwise_fwd`` on the 3x3 depthwise layers in front of them.  Method of tools/adam_bench.py: the variants
    alternate within a round, one event pair around ``--reps`` calls, median with min-max over the rounds.
    The expectation is written to the log BEFORE the run; the outcome after it, met or not.
(b) MobileNet v1 0.25 and 1.0, random init, weight ranges recorded by an unfused build pass: the share of elements
    that differ between QuantConfig(integer=True) and the bf16 fused fake-quant evaluation, per quantised layer output
    (one code step or more) and in the logits.  Reported, asserted nowhere.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

EXPECTATION = ("expectation: the int8 pointwise conv is no slower than the bf16 one at both shapes (half the operand "
               "bytes, twice the nominal MFMA rate; it stages nothing through LDS)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "int8_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.compat import quantize as Q
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops import int8
    from distributed_tensorflow_models_amd.ops import nn as F
    from distributed_tensorflow_models_amd.ops.depthwise import depthwise_conv2d

    assert torch.cuda.is_available(), "int8_bench needs a GPU"
    dev = torch.device("cuda", 0)
    log = open(args.log, "w")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    def rec(scale, zp, qmin=0):
        r = torch.zeros(8, dtype=torch.int32)
        f = r.view(torch.float32)
        f[0], f[2], f[3], f[4] = scale, float(zp), float(qmin), 255.0
        f[1:2] = 1.0 / f[0:1]
        return r.to(dev)

    say("int8_bench: batch %d, %d rounds x %d calls per sample, variants alternating" % (args.batch, args.rounds,
                                                                                       args.reps))
    say(EXPECTATION)
    g = torch.Generator().manual_seed(0)
    ra, rw, ro = rec(0.0235, 0), rec(0.004, 128, 1), rec(0.0235, 0)
    met = True
    with torch.no_grad():
        for hw, c in ((14, 512), (7, 1024)):
            a = torch.randint(0, 256, (args.batch, hw, hw, c), generator=g, dtype=torch.uint8).to(dev)
            x = int8.dequantize_u8(a, ra, torch.bfloat16)
            bias = torch.randn(c, generator=g).to(dev)
            w = ((torch.randint(1, 256, (c, 1, 1, c), generator=g).float() - 128) * 0.004).to(dev)
            dw = ((torch.randint(1, 256, (3, 3, c, 1), generator=g).float() - 128) * 0.004).to(dev)
            qw, qdw = int8.prepare_weights(w, rw), int8.prepare_weights(dw, rw, depthwise=True)
            w16 = torch.nn.Parameter(w)
            res = _alternate({
                "pw_int8": lambda: int8.conv2d_q8(a, ra, qw, bias, ro, 1, "SAME", "relu", torch.bfloat16),
                "pw_bf16": lambda: F.conv2d(x, w16, bias, 1, "SAME", relu=True),
                "dw_int8": lambda: int8.depthwise_q8(a, ra, qdw, bias, ro, 1, "SAME", "relu6", torch.bfloat16),
                "dw_bf16": lambda: depthwise_conv2d(x, dw, 1, "SAME"),
            }, args.rounds, args.reps, args.warmup)
            for k, (med, lo, hi) in res.items():
                say("  %2dx%2dx%4d  %-8s median %.4f ms  (min %.4f  max %.4f)" % (hw, hw, c, k, med, lo, hi))
            ratio = res["pw_int8"][0] / res["pw_bf16"][0]
            met = met and ratio <= 1.0
            say("  %2dx%2dx%4d  pointwise int8 / bf16 = %.3f   depthwise int8 / bf16 = %.3f (the bf16 depthwise has "
                "no bias or activation)" % (hw, hw, c, ratio, res["dw_int8"][0] / res["dw_bf16"][0]))
    say("outcome: expectation %s" % ("MET" if met else "NOT MET"))

    # ---- (b) integer against bf16 fake-quant evaluation ---------------------------------------------------------
    for name, size in (("mobilenet_v1_025", 128), ("mobilenet_v1", 224)):
        def make(cfg):
            torch.manual_seed(0)
            return nets_factory.build(name, num_classes=1001, quantize=cfg)
        ref = make(Q.QuantConfig(is_training=False))  # (its build pass records the weight ranges)
        nets = []
        for integer in (True, False):
            m = make(Q.QuantConfig(is_training=False, fused=True, integer=integer))
            m.load_state_dict(ref.state_dict())
            nets.append(m.to(dev))
        x = torch.randn(8, size, size, 3, generator=g).to(dev).to(torch.bfloat16)
        eps = ({}, {})
        int8.reset_layers()
        with torch.no_grad():
            ys = [m(x, training=False, end_points=ep).float() for m, ep in zip(nets, eps)]
        diff = total = 0
        for k in eps[0]:
            if k.startswith("Conv2d_") and k != "Conv2d_0":
                diff += int((eps[0][k].float() != eps[1][k].float()).sum())
                total += eps[0][k].numel()
        say("%s random init, 8 x %d x %d: %d integer layers; layer outputs that differ from the bf16 fake-quant "
            "evaluation: %.3f %% of %d; logits that differ: %.1f %% (max |diff| %.4g, max |logit| %.4g); argmax "
            "agrees on %d of 8" % (name, size, size, int8.layers_run(), 100.0 * diff / total, total,
                                   100.0 * float((ys[0] != ys[1]).float().mean()), float((ys[0] - ys[1]).abs().max()),
                                   float(ys[1].abs().max()), int((ys[0].argmax(-1) == ys[1].argmax(-1)).sum())))
    log.close()
    print(json.dumps(dict(log=args.log, expectation_met=met)))


if __name__ == "__main__":
    main()
