#!/usr/bin/env python3
"""Cost of a summary step's histogram pass over ResNet-50's variables and gradients (161 + 161 tensors).

Times, with HIP events on one GPU:
* the two-launch multi-tensor pass (ops.summary.TensorStats.launch: bins memset, tensor_stats_kernel,
  tensor_stats_finalize_kernel and the device-to-pinned-host copies of the results);
* the same quantities tensor by tensor with torch ops (bucketize + bincount, sum, min, max, zero and non-finite
  counts) - the baseline the kernel replaces.  Nothing is read back per tensor, but the boolean indexing and
  torch.bincount each wait for the device to size their outputs, so the figure holds those host round trips (two or
  more per tensor) as well as the launches: it is the cost of the ATen route as written, not of its kernels alone;
* optionally (--step) the ResNet-50 training step (batch 256, bf16, momentum) of the same process, so the pass can
  be stated as a share of a step.
Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _time_ms(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time the ResNet-50 batch-256 training step")
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops.summary import NUM_BUCKETS, TensorStats, limits

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
    step = TrainStep(net, optimizer="momentum", lr=0.01, momentum=0.9)
    x = torch.randn(args.batch if args.step else 16, 224, 224, 3, device=dev).to(torch.bfloat16)
    y = torch.randint(0, 1000, (x.shape[0],), device=dev)
    step(x, y)  # real gradients in the flat buffer
    torch.cuda.synchronize()
    params = [p for p in net.parameters() if p.requires_grad]
    tensors = [p.detach() for p in params] + [p.main_grad for p in params]
    scales = [1.0] * len(params) + [step.dp.grad_scale] * len(params)
    out = dict(tensors=len(tensors), elements=int(sum(t.numel() for t in tensors)))

    st = TensorStats(tensors, scales)
    out["pass_ms_median"], out["pass_ms_min"] = _time_ms(st.launch, args.iters, args.warmup)
    recs = st.fetch()

    lim = torch.from_numpy(limits().copy()).to(dev)

    def per_tensor():
        res = []
        for t, s in zip(tensors, scales):
            v = t.reshape(-1).float() * s
            fin = torch.isfinite(v)
            d = v[fin].double()
            counts = torch.bincount(torch.bucketize(d, lim, right=True), minlength=NUM_BUCKETS)
            res.append((counts, d.sum(), (d * d).sum(), d.min(), d.max(), (d == 0).sum(), (~fin).sum()))
        return res

    out["per_tensor_ms_median"], out["per_tensor_ms_min"] = _time_ms(per_tensor, args.iters, args.warmup)
    base = per_tensor()
    torch.cuda.synchronize()
    for r, b in zip(recs, base):  # the two compute the same histograms
        assert (b[0].cpu().numpy() == r["counts"]).all() and int(b[6]) == r["nonfinite"]
    out["speedup"] = out["per_tensor_ms_median"] / out["pass_ms_median"]

    if args.step:
        out["batch"] = args.batch
        out["step_ms_median"], out["step_ms_min"] = _time_ms(lambda: step(x, y), args.iters, args.warmup)
        out["pass_share_of_step"] = out["pass_ms_median"] / out["step_ms_median"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
