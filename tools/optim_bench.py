#!/usr/bin/env python3
"""Cost of the multi-tensor norm pass (LARS / clip by global norm) on ResNet-50's variables.

The 161 trainable variables of resnet_v1_50 (fp32 weights in allocations of their own, gradients as views into one
flat buffer packed back to back, as the BSP engine lays them out) are updated, with HIP events on one GPU, by
  (a) the momentum update launch alone (multi_tensor_opt_kernel: the path without LARS);
  (b) the norm pass + the scaled update (multi_tensor_norm_kernel, multi_tensor_norm_finalize_kernel,
      multi_tensor_opt_kernel with the trust ratios): what ``optimizer="lars"`` enqueues;
  (n) the norm pass alone, for its achieved bytes/s (it reads weight and gradient once: 8 B per element);
  (u) the norm pass alone with the flat gradient buffer shifted by one element, so that every gradient is offset
      against its weight within 16 bytes and the pass takes its 4-byte-load path (ResNet-50's own sizes are all
      multiples of 4, so (n) runs on 16-byte loads throughout);
  (c) the weight and gradient norms tensor by tensor with torch._foreach_norm (two of the pass's three norms and no
      trust ratios: the ATen route it replaces, a lower bound of it).
Each sample is one event pair around ``--reps`` back-to-back launches; the variants alternate within a round and the
figure is the median over the rounds, per launch.  With --step the whole ResNet-50 training step (batch 256, bf16) is
timed with ``momentum`` and with ``lars``, alternating as well.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _sample_ms(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _alternate(fns, rounds, reps, warmup):
    """{name: (median, min, max)} ms per call; every round times each variant once, in turn."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(_sample_ms(fn, reps))
    out = {}
    for k, v in times.items():
        v.sort()
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


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

    assert torch.cuda.is_available(), "optim_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in nets_factory.build("resnet_v1_50", num_classes=1000).parameters()
              if p.requires_grad]
    numel = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numel)

    def make(kind, shift=0):
        flat = torch.randn(total + shift, device=dev) * 1e-2
        params, off = [], shift
        for s, n in zip(shapes, numel):
            p = torch.nn.Parameter(torch.randn(s, device=dev) * 0.05)
            p.weight_decay = 1e-4
            p.main_grad = flat[off:off + n].view(s)
            params.append(p)
            off += n
        opt = FusedOptimizer(params, kind, lr=1e-4, momentum=0.9)
        opt.set_dynamic(1e-4, 1.0)
        return params, flat, opt

    pm, fm, mom = make("momentum")
    pl, fl, lars = make("lars")
    pu, fu, lars_u = make("lars", shift=1)
    grads = [p.main_grad for p in pl]
    weights = [p.detach() for p in pl]

    def foreach_norms():
        return torch._foreach_norm(weights), torch._foreach_norm(grads)

    res = _alternate({"a_momentum_update": mom.launch, "b_norms_plus_scaled_update": lars.launch,
                      "n_norm_pass": lars.launch_norms, "u_norm_pass_unaligned": lars_u.launch_norms,
                      "c_foreach_norm": foreach_norms},
                     args.rounds, args.reps, args.warmup)
    # the pass and the ATen route agree on the norms they share
    lars.launch_norms()
    wn, gn = foreach_norms()
    got = lars.last_norms()
    torch.testing.assert_close(got[:, 0], torch.stack(wn), rtol=1e-4, atol=0)
    torch.testing.assert_close(got[:, 1], torch.stack(gn), rtol=1e-4, atol=0)

    out = dict(tensors=len(shapes), elements=total, chunk_rows=mom._nchunks, rounds=args.rounds, reps=args.reps,
               unaligned_grad_bases=sum(g.data_ptr() % 16 != 0 for g in grads),
               unaligned_grad_bases_u=sum(p.main_grad.data_ptr() % 16 != 0 for p in pu))
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    a, b, n = res["a_momentum_update"][0], res["b_norms_plus_scaled_update"][0], res["n_norm_pass"][0]
    out["b_minus_a_ms"] = round(b - a, 4)
    out["b_minus_a_over_a"] = round((b - a) / a, 3)
    out["sanity_b_minus_a_le_a"] = bool(b - a <= a)
    out["norm_pass_read_GBps"] = round(8.0 * total / (n * 1e-3) / 1e9, 1)      # 8 B per element read
    out["norm_pass_unaligned_read_GBps"] = round(8.0 * total / (res["u_norm_pass_unaligned"][0] * 1e-3) / 1e9, 1)
    out["update_traffic_GBps"] = round(22.0 * total / (a * 1e-3) / 1e9, 1)     # 12 B read + 10 B written
    out["norm_pass_vs_foreach"] = round(res["c_foreach_norm"][0] / n, 2)

    if args.step:
        del pm, fm, mom, pl, fl, lars, pu, fu, lars_u, grads, weights
        steps = {}
        for kind in ("momentum", "lars"):
            torch.manual_seed(0)
            net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
            steps[kind] = TrainStep(net, optimizer=kind, lr=0.01, momentum=0.9)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        sres = _alternate({k: (lambda s=s: s(x, y)) for k, s in steps.items()}, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for k, (med, lo, hi) in sres.items():
            out["step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        out["step_lars_over_momentum"] = round(sres["lars"][0] / sres["momentum"][0], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
