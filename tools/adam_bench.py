#!/usr/bin/env python3
"""Cost of the fused Adam step on ResNet-50's variables, with the method of tools/optim_bench.py.

The 161 trainable variables of resnet_v1_50 (fp32 weights in allocations of their own, each with a bf16 compute copy;
gradients as views into one flat buffer packed back to back, as the BSP engine lays them out) are updated, with HIP
events on one GPU, by
  (a) the momentum launch (multi_tensor_opt_kernel): 12 B read + 10 B written per element;
  (b) the Adam step: the one-thread state advance plus multi_tensor_adam_kernel, 16 B read + 14 B written (ResNet-50's
      sizes are all multiples of 4, so every tensor takes the 16-byte path);
  (c) the Adam step with the flat gradient buffer shifted by one element, so that every gradient is offset against
      its weight within 16 bytes and the kernel takes its 4-byte path;
  (d) torch.optim.Adam(fused=True) over the same fp32 tensors plus the torch._foreach_copy_ into the bf16 copies that it
      would need to replace (b): the same bytes in more launches.
Each sample is one event pair around ``--reps`` back-to-back launches; the variants alternate within a round and the
figure is the median over the rounds, per launch.  The implied bytes/s divide the bytes the update has to move by that
time; back-to-back launches over the same 25.6 M elements (0.36 GB of arrays for momentum, 0.46 GB for Adam) run partly
out of the 256 MiB Infinity Cache, so they are not HBM rates.  Prints one JSON line.
"""
import argparse
import json
import math
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
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops.optim import FusedOptimizer

    assert torch.cuda.is_available(), "adam_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in nets_factory.build("resnet_v1_50", num_classes=1000).parameters()
              if p.requires_grad]
    numel = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numel)
    lr, wd = 1e-4, 1e-4

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
        opt = FusedOptimizer(params, kind, lr=lr, momentum=0.9)
        opt.set_dynamic(lr, 1.0)
        return params, flat, opt

    pm, fm, mom = make("momentum")
    pa, fa, adam = make("adam")
    pu, fu, adam_u = make("adam", shift=1)
    pt, ft, _ = make("sgd")  # the tensors of the ATen route
    for p in pt:
        p.grad = p.main_grad
    tadam = torch.optim.Adam(pt, lr=lr, weight_decay=wd, fused=True)
    t32, t16 = [p.detach() for p in pt], [p.bf16 for p in pt]

    def torch_adam():
        tadam.step()
        torch._foreach_copy_(t16, t32)

    # (b) and (d) compute the same thing: the first step of each from the same weights and gradients.  ATen adds its
    # epsilon to sqrt(v / (1-b2^t)), TensorFlow's form to sqrt(v): for this one step ATen gets eps / sqrt(1-b2).
    ft.copy_(fa)
    for p, q in zip(pa, pt):
        q.data.copy_(p.detach())
    adam.launch()
    tadam.param_groups[0]["eps"] = 1e-8 / math.sqrt(1.0 - 0.999)
    torch_adam()
    tadam.param_groups[0]["eps"] = 1e-8
    for p, q in zip(pa, pt):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-4, atol=1e-7)
        assert torch.equal(p.bf16, p.detach().bfloat16())

    res = _alternate({"a_momentum": mom.launch, "b_adam": adam.launch, "c_adam_unaligned": adam_u.launch,
                      "d_torch_fused_adam_plus_bf16_copy": torch_adam}, args.rounds, args.reps, args.warmup)
    steps = adam.adam_step()
    out = dict(tensors=len(shapes), elements=total, chunk_rows=adam._nchunks, rounds=args.rounds, reps=args.reps,
               adam_steps_applied=steps,
               unaligned_grad_bases_b=sum(p.main_grad.data_ptr() % 16 != 0 for p in pa),
               unaligned_grad_bases_c=sum(p.main_grad.data_ptr() % 16 != 0 for p in pu))
    nbytes = {"a_momentum": 22.0, "b_adam": 30.0, "c_adam_unaligned": 30.0, "d_torch_fused_adam_plus_bf16_copy": 30.0}
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        out[k + "_GBps"] = round(nbytes[k] * total / (med * 1e-3) / 1e9, 1)
    a, b, d = res["a_momentum"][0], res["b_adam"][0], res["d_torch_fused_adam_plus_bf16_copy"][0]
    out["b_over_a"] = round(b / a, 3)
    out["byte_ratio_30_over_22"] = round(30.0 / 22.0, 3)
    out["c_over_b"] = round(res["c_adam_unaligned"][0] / b, 3)
    out["d_over_b"] = round(d / b, 3)
    out["expected_b_le_d"] = bool(b <= d)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
