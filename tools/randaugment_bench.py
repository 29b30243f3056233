#!/usr/bin/env python3
"""Cost of RandAugment on the device (csrc/kernels/randaugment.hip), with the method of tools/mix_bench.py.

HIP events on one GPU:
  (a)  ``randaugment`` with N = 2 layers sampled from the 14 default ops at magnitude 9, on [256, 224, 224, 3]
       uint8 -> bf16 and on [128, 299, 299, 3] fp32 -> bf16 (the ImageNet pipeline's call);
  (a1) each sampler op alone as an N = 1 plan (every image on that op), [256, 224, 224, 3] uint8 -> bf16;
  (b)  a ``copy_`` of the same uint8 bytes in the same run: its bytes/s (read + write) is the rate of a byte model of
       (a): the source read once by layer 0 and once more by layer 0's statistics pass for the images whose op needs
       one, 3 B read per pixel of an inner statistics pass that runs, 3 B written + 3 B read per pixel between two
       layers, and the final write in the destination's type;
  (c)  with --step: the ResNet-50 training step (bf16, batch --batch) alone - the step this change leaves as it was -
       and with the N = 2 call on a uint8 batch in front of it.
Each sample is one event pair around ``--reps`` back-to-back calls; the variants alternate within a round and the
figure is the median over the rounds, per call, with min and max.  Back-to-back calls over the same buffers run
partly out of the 256 MiB Infinity Cache, for (a) and for (b) alike, so none of the rates are HBM rates.
The expectation - (a) within 2x its byte model - is written to the log BEFORE anything is timed, and the result line
reports it as met or not met.  Prints one JSON line and appends it to --log.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

EXPECTATION = ("expectation (stated before the run): (a) randaugment N=2 takes at most 2x its byte model at the "
               "copy's rate")


def model_bytes(plan, H, W, src_bytes, dst_bytes):
    """Bytes the call needs, from the plan: see (b) above."""
    from distributed_tensorflow_models_amd.ops import randaugment as ra
    npix = H * W
    total = 0.0
    for l in range(plan.N):
        op = plan.op[:, l]
        stats = int(((op == ra.AUTOCONTRAST) | (op == ra.EQUALIZE) | (op == ra.CONTRAST)).sum())
        rd = src_bytes if l == 0 else 1
        wr = dst_bytes if l == plan.N - 1 else 1
        total += npix * 3 * (plan.B * (rd + wr) + stats * rd)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time whole ResNet-50 training steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "randaugment_bench.log"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from distributed_tensorflow_models_amd.ops import randaugment as ra

    assert torch.cuda.is_available(), "randaugment_bench needs a GPU"
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(EXPECTATION + "\n")
    print(EXPECTATION, flush=True)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out_affine = (2.0 / 255.0, -1.0)

    out = dict(rounds=args.rounds, reps=args.reps)
    fns, nbytes = {}, {}
    cfg = ra.RandAugmentConfig(layers=2, seed=1)
    u8 = torch.randint(0, 256, (256, 224, 224, 3), dtype=torch.uint8, device=dev)
    f32 = torch.rand((128, 299, 299, 3), device=dev) * 2.0 - 1.0
    for tag, x, in_affine in (("224_u8", u8, (1.0, 0.0)), ("299_f32", f32, (0.5, 0.5))):
        B, H, W, _C = x.shape
        plan = ra.sample_plan(cfg, 0, 0, B, H, W).to(dev)
        dst = torch.empty(x.shape, dtype=torch.bfloat16, device=dev)
        got = ra.randaugment(x, plan, "bfloat16", in_affine, out_affine, out=dst)
        torch.cuda.synchronize()
        # the kernel and the numpy form compute the same thing, on the first images of the timed batch
        k = 4
        sub = ra.RandAugmentPlan(plan.rec[:k], H, W)
        want = ra.randaugment(x[:k].cpu(), sub, "bfloat16", in_affine, out_affine)
        assert torch.equal(got[:k].cpu().view(torch.int16), want.view(torch.int16))
        fns["a_randaugment_n2_" + tag] = (lambda x=x, p=plan, d=dst, ia=in_affine:
                                          ra.randaugment(x, p, "bfloat16", ia, out_affine, out=d))
        nbytes["a_randaugment_n2_" + tag] = model_bytes(plan, H, W, x.element_size(), 2)
        out["ops_n2_" + tag] = {ra.OPS[o]: int(c) for o, c in zip(*np.unique(plan.op, return_counts=True))}
        cp_src = x if x.dtype == torch.uint8 else torch.randint(0, 256, x.shape, dtype=torch.uint8, device=dev)
        cp_dst = torch.empty_like(cp_src)
        fns["b_copy_u8_" + tag] = lambda s=cp_src, d=cp_dst: d.copy_(s)
        nbytes["b_copy_u8_" + tag] = 2.0 * cp_src.numel()
    B, H, W, _C = u8.shape
    dst = torch.empty(u8.shape, dtype=torch.bfloat16, device=dev)
    one = ra.RandAugmentConfig(layers=1, magnitude=9.0, seed=1)
    for name in ra.SAMPLER_OPS:
        r = ra.sampled_record(name, 0.9, False, 0.5, 0.5, one, H, W)
        plan = ra.make_plan([[r]] * B, H, W).to(dev)
        key = "a1_%s_224_u8" % name
        fns[key] = lambda p=plan, d=dst: ra.randaugment(u8, p, "bfloat16", (1.0, 0.0), out_affine, out=d)
        nbytes[key] = model_bytes(plan, H, W, 1, 2)
    res = _alternate(fns, args.rounds, args.reps, args.warmup)
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        out[k + "_GBps"] = round(nbytes[k] / (med * 1e-3) / 1e9, 1)
    met = True
    for tag in ("224_u8", "299_f32"):
        rate = nbytes["b_copy_u8_" + tag] / res["b_copy_u8_" + tag][0]  # bytes per ms
        model_ms = nbytes["a_randaugment_n2_" + tag] / rate
        ratio = res["a_randaugment_n2_" + tag][0] / model_ms
        out["model_ms_" + tag] = round(model_ms, 4)
        out["time_over_model_" + tag] = round(ratio, 3)
        met = met and ratio <= 2.0
    out["expectation_within_2x_byte_model"] = "met" if met else "not met"

    if args.step:
        from distributed_tensorflow_models_amd.engine import TrainStep
        from distributed_tensorflow_models_amd.models import nets_factory
        del fns
        torch.cuda.empty_cache()
        torch.manual_seed(0)
        net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
        step = TrainStep(net, optimizer="momentum", lr=0.01, momentum=0.9)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        raw = torch.randint(0, 256, (args.batch, 224, 224, 3), dtype=torch.uint8, device=dev)
        plan = ra.sample_plan(cfg, 0, 0, args.batch, 224, 224).to(dev)
        aug = torch.empty(raw.shape, dtype=torch.bfloat16, device=dev)

        def with_ra():
            ra.randaugment(raw, plan, "bfloat16", (1.0, 0.0), out_affine, out=aug)
            return step(x, y)  # (the same batch as the plain arm: only the input-side call is added)

        sres = _alternate({"plain": lambda: step(x, y), "randaugment": with_ra}, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for k, (med, lo, hi) in sres.items():
            out["step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        out["step_randaugment_over_plain"] = round(sres["randaugment"][0] / sres["plain"][0], 4)
        out["step_overhead_ms"] = round(sres["randaugment"][0] - sres["plain"][0], 3)
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
