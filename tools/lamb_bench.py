#!/usr/bin/env python3
"""Cost of the fused LAMB step on ResNet-50's variables, with the method of tools/adam_bench.py.

The 161 trainable variables of resnet_v1_50 (fp32 weights in allocations of their own, each with a bf16 compute copy;
gradients as views into one flat buffer packed back to back, as the BSP engine lays them out) are updated, with HIP
events on one GPU, by
  (a) the Adam step: the one-thread state advance plus multi_tensor_adam_kernel, 16 B read + 14 B written per element;
  (b) the LAMB step: the state advance, the moments pass (16 B read + 8 B written, plus one 24-byte record per 8192
      elements), the one-block finalize and the apply pass (12 B read + 6 B written): 42 B per element (ResNet-50's
      sizes are all multiples of 4, so every tensor takes the 16-byte paths);
  (c) the LAMB step with the flat gradient buffer shifted by one element, so that every gradient is offset against
      its weight within 16 bytes and the moments pass takes its 4-byte path (the apply pass does not read gradients);
  (d) the same update from torch._foreach_* ops (moments, direction, two _foreach_norm, the ratios from the stacked
      norms on the device, the scaled subtraction) plus the torch._foreach_copy_ into the bf16 copies.
Each sample is one event pair around ``--reps`` back-to-back launches; the variants alternate within a round and the
figure is the median over the rounds, per launch.  The implied bytes/s divide the bytes the update has to move by that
time; back-to-back launches over the same 25.6 M elements (0.46 GB of arrays) run partly out of the 256 MiB Infinity
Cache, so they are not HBM rates.  Expectations, reported as measured: (b) takes less time than (d); (b)/(a) is near
the byte ratio 42/30 (the JSON line marks it met within 15 % of that ratio).  With --step the whole ResNet-50
training step (bf16, batch --batch) is timed under momentum, lars and lamb the same way.  Prints one JSON line.
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=4)
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops.optim import FusedOptimizer

    assert torch.cuda.is_available(), "lamb_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in nets_factory.build("resnet_v1_50", num_classes=1000).parameters()
              if p.requires_grad]
    numel = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numel)
    lr, wd, b1, b2, eps = 1e-3, 1e-4, 0.9, 0.999, 1e-6

    def make(kind, shift=0):
        flat = torch.randn(total + shift, device=dev) * 1e-2
        params, off = [], shift
        for s, n in zip(shapes, numel):
            p = torch.nn.Parameter(torch.randn(s, device=dev) * 0.05)
            p.weight_decay = wd
            p.main_grad = flat[off:off + n].view(s)
            p.bf16 = p.detach().to(torch.bfloat16)
            params.append(p)
            off += n
        opt = FusedOptimizer(params, kind, lr=lr, momentum=0.9, beta1=b1, beta2=b2)
        opt.set_dynamic(lr, 1.0)
        return params, flat, opt

    pa, fa, adam = make("adam")
    pl, fl, lamb = make("lamb")
    pu, fu, lamb_u = make("lamb", shift=1)
    pt, ft, _ = make("sgd")  # the tensors of the ATen route
    t32, t16 = [p.detach() for p in pt], [p.bf16 for p in pt]
    tg = [p.main_grad for p in pt]
    tm, tv = [torch.zeros_like(p) for p in t32], [torch.zeros_like(p) for p in t32]
    adapt = torch.tensor([len(s) > 1 for s in shapes], device=dev)
    one = torch.ones((), device=dev)
    t_applied = [0]

    def foreach_lamb():
        t_applied[0] += 1
        bc1, bc2 = 1.0 - b1 ** t_applied[0], (1.0 - b2 ** t_applied[0]) ** 0.5
        torch._foreach_mul_(tm, b1)
        torch._foreach_add_(tm, tg, alpha=1.0 - b1)
        torch._foreach_mul_(tv, b2)
        torch._foreach_addcmul_(tv, tg, tg, value=1.0 - b2)
        den = torch._foreach_sqrt(tv)
        torch._foreach_div_(den, bc2)
        torch._foreach_add_(den, eps)
        r = torch._foreach_div(tm, bc1)
        torch._foreach_div_(r, den)
        torch._foreach_add_(r, t32, alpha=wd)
        pn, rn = torch.stack(torch._foreach_norm(t32)), torch.stack(torch._foreach_norm(r))
        phi = torch.where(adapt & (pn > 0) & (rn > 0), pn / rn, one)
        torch._foreach_mul_(r, list((phi * -lr).unbind()))
        torch._foreach_add_(t32, r)
        torch._foreach_copy_(t16, t32)

    # (b) and (d) compute the same thing: the first step of each from the same weights and gradients
    ft.copy_(fl)
    for p, q in zip(pl, pt):
        q.data.copy_(p.detach())
    lamb.launch()
    foreach_lamb()
    for p, q in zip(pl, pt):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-4, atol=1e-7)
        assert torch.equal(p.bf16, p.detach().bfloat16())
    torch.testing.assert_close(lamb.last_lr_scale(), torch.where(adapt, lamb.last_lr_scale(), one))

    res = _alternate({"a_adam": adam.launch, "b_lamb": lamb.launch, "c_lamb_unaligned": lamb_u.launch,
                      "d_foreach_lamb_plus_bf16_copy": foreach_lamb}, args.rounds, args.reps, args.warmup)
    out = dict(tensors=len(shapes), elements=total, chunk_rows=lamb._nchunks, rounds=args.rounds, reps=args.reps,
               lamb_steps_applied=lamb.adam_step(),
               unaligned_grad_bases_b=sum(p.main_grad.data_ptr() % 16 != 0 for p in pl),
               unaligned_grad_bases_c=sum(p.main_grad.data_ptr() % 16 != 0 for p in pu))
    nbytes = {"a_adam": 30.0, "b_lamb": 42.0, "c_lamb_unaligned": 42.0, "d_foreach_lamb_plus_bf16_copy": 42.0}
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        out[k + "_GBps"] = round(nbytes[k] * total / (med * 1e-3) / 1e9, 1)
    a, b, d = res["a_adam"][0], res["b_lamb"][0], res["d_foreach_lamb_plus_bf16_copy"][0]
    out["b_over_a"] = round(b / a, 3)
    out["byte_ratio_42_over_30"] = round(42.0 / 30.0, 3)
    out["c_over_b"] = round(res["c_lamb_unaligned"][0] / b, 3)
    out["d_over_b"] = round(d / b, 3)
    out["expected_b_lt_d"] = bool(b < d)
    out["expected_b_over_a_within_15pct_of_byte_ratio"] = bool(abs(b / a / 1.4 - 1.0) <= 0.15)

    if args.step:
        del pa, fa, adam, pl, fl, lamb, pu, fu, lamb_u, pt, ft, t32, t16, tg, tm, tv
        torch.cuda.empty_cache()
        steps = {}
        for kind in ("momentum", "lars", "lamb"):
            torch.manual_seed(0)
            net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
            steps[kind] = TrainStep(net, optimizer=kind, lr=0.01 if kind != "lamb" else 0.001, momentum=0.9)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        sres = _alternate({k: (lambda s=s: s(x, y)) for k, s in steps.items()}, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for k, (med, lo, hi) in sres.items():
            out["step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        out["step_lars_over_momentum"] = round(sres["lars"][0] / sres["momentum"][0], 4)
        out["step_lamb_over_momentum"] = round(sres["lamb"][0] / sres["momentum"][0], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
