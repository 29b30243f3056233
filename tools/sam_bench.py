#!/usr/bin/env python3
"""Cost of the SAM perturb / restore launches on ResNet-50's variables, with the method of tools/lamb_bench.py.

The 161 trainable variables of resnet_v1_50 (fp32 weights in allocations of their own, each with a bf16 compute copy
and a backup; gradients as views into one flat buffer packed back to back, as the BSP engine lays them out) go, with
HIP events on one GPU, through
  (a) ops.sam.SamPerturber.perturb() (three launches: norm, finalize, perturb) and restore() (one launch).  Bytes per
      element with the bf16 copy: norm 4 (ASAM 8), perturb 8 read + 14 written, restore 4 read + 6 written: 36 (ASAM 40);
  (a') the same with ASAM's element-wise scaling;
  (b) the same result from torch._foreach_* ops: _foreach_norm and the scale from the stacked norms on the device,
      _foreach_copy_ into the backups, _foreach_mul / _foreach_add_, the copy into the bf16 copies, _foreach_zero_ of
      the gradients; then the two copies of the restore.  Checked equal to (a) first, from the same weights and
      gradients.
Each sample is one event pair around ``--reps`` back-to-back calls; the variants alternate within a round and the
figure is the median over the rounds, per call, with min - max.  Back-to-back calls over the same 25.6 M elements
(0.36 GB of arrays) run partly out of the 256 MiB Infinity Cache, so the implied bytes/s are not HBM rates.
With --step the whole ResNet-50 training step (bf16, batch --batch) is timed with sam=None and sam=SamConfig(0.05),
alternating the same way; the yardstick of the SAM step is the sam=None arm of the same run.

Expectations, written down before the first run and reported as met or not met, whichever it is:
  1. (a) takes less time than (b);
  2. the SAM step takes about twice the plain step plus (a): ``step_sam / (2 * step_plain + a)`` within 10 % of 1.
Prints one JSON line.
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
    ap.add_argument("--reps", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time whole ResNet-50 training steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=4)
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops.sam import EPS, SamConfig, SamPerturber

    assert torch.cuda.is_available(), "sam_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in nets_factory.build("resnet_v1_50", num_classes=1000).parameters()
              if p.requires_grad]
    numel = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numel)
    rho = 0.05

    def make():
        flat = torch.randn(total, device=dev) * 1e-2
        ws, gs, cs, off = [], [], [], 0
        for s, n in zip(shapes, numel):
            w = torch.randn(s, device=dev) * 0.05
            ws.append(w)
            gs.append(flat[off:off + n].view(s))
            cs.append(w.to(torch.bfloat16))
            off += n
        return flat, ws, gs, cs

    fs, ws, gs, cs = make()
    sam = SamPerturber(list(zip(ws, gs, cs)), config=SamConfig(rho))
    fa, wa, ga, ca = make()
    asam = SamPerturber(list(zip(wa, ga, ca)), config=SamConfig(rho, adaptive=True))
    ft, wt, gt, ct = make()  # the tensors of the ATen route
    bt = [torch.empty_like(w) for w in wt]

    def foreach_perturb():
        s = torch.stack(torch._foreach_norm(gt)).double().square().sum().sqrt()
        scale = (rho / (s + EPS)).float()
        torch._foreach_copy_(bt, wt)
        e = torch._foreach_mul(gt, scale)
        torch._foreach_add_(wt, e)
        torch._foreach_copy_(ct, wt)
        torch._foreach_zero_(gt)

    def foreach_restore():
        torch._foreach_copy_(wt, bt)
        torch._foreach_copy_(ct, wt)

    def foreach_both():
        foreach_perturb()
        foreach_restore()

    def both(sp):
        def run():
            sp.perturb()
            sp.restore()
        return run

    # (a) and (b) compute the same thing: one perturbation of each from the same weights and gradients
    ft.copy_(fs)
    for w, q in zip(ws, wt):
        q.copy_(w)
    old = [w.clone() for w in ws]
    sam.perturb()
    foreach_perturb()
    moved = 0
    for w, q, c, o in zip(ws, wt, cs, old):
        torch.testing.assert_close(w, q, rtol=1e-5, atol=1e-8)
        assert torch.equal(c, w.bfloat16())
        moved += int((w != o).sum())
    assert moved > total // 2 and not fs.any() and not ft.any()
    sam.restore()
    foreach_restore()
    for w, q, c, o in zip(ws, wt, cs, old):
        assert torch.equal(w, o) and torch.equal(q, o) and torch.equal(c, o.bfloat16())

    res = _alternate({"a_sam": both(sam), "a_asam": both(asam), "b_foreach": foreach_both,
                      "a_sam_perturb_only": sam.perturb, "a_sam_restore_only": sam.restore},
                     args.rounds, args.reps, args.warmup)
    out = dict(tensors=len(shapes), elements=total, chunk_rows=sam._nchunks, rounds=args.rounds, reps=args.reps,
               unaligned_grad_bases=sum(g.data_ptr() % 16 != 0 for g in gs))
    nbytes = {"a_sam": 36.0, "a_asam": 40.0, "b_foreach": 36.0, "a_sam_perturb_only": 26.0, "a_sam_restore_only": 10.0}
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        out[k + "_GBps"] = round(nbytes[k] * total / (med * 1e-3) / 1e9, 1)
    a, b = res["a_sam"][0], res["b_foreach"][0]
    out["b_over_a"] = round(b / a, 3)
    out["expected_a_lt_b"] = "met" if a < b else "not met"

    if args.step:
        del sam, asam, fs, ws, gs, cs, fa, wa, ga, ca, ft, wt, gt, ct, bt, old
        torch.cuda.empty_cache()
        steps = {}
        for name, cfg in (("plain", None), ("sam", SamConfig(rho))):
            torch.manual_seed(0)
            net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
            steps[name] = TrainStep(net, optimizer="momentum", lr=0.01, momentum=0.9, sam=cfg)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        sres = _alternate({k: (lambda s=s: s(x, y)) for k, s in steps.items()}, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for k, (med, lo, hi) in sres.items():
            out["step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        ratio = sres["sam"][0] / sres["plain"][0]
        model = sres["sam"][0] / (2.0 * sres["plain"][0] + a)
        out["step_sam_over_plain"] = round(ratio, 4)
        out["step_sam_over_twice_plain_plus_a"] = round(model, 4)
        out["expected_step_about_twice_plus_a_within_10pct"] = "met" if abs(model - 1.0) <= 0.10 else "not met"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
