#!/usr/bin/env python3
"""Cost of top-k gradient sparsification (csrc/kernels/grad_compress.hip) on one bucket of 8 M fp32 elements at
rho = 0.01 and 0.001, with the method of tools/adam_bench.py.

HIP events on one GPU:
  (a) compress_bucket: the 10 launches of the select, count and pack stages, about 32 B per element; at rho = 0.01
      also its three stages on their own (dtm_grad_compress_stages): a1 the init and the select (7 launches, 20 B per
      element), a2 the count and the row scan (2 launches, 4 B), a3 the pack (1 launch, 4 B read and the changed
      residual groups and the packet written);
  (b) the torch form of the same result (add, a 63-bit (key, reversed index) composite, topk, sort, gather, masked
      residual), checked bit-equal to (a) at the timed size first: packet and residual;
  (c) decompress_bucket for W = 8 packets;
  (f) the fold kernel (grad_accum mode 2, 12 B per element) on the same size: the measured rate the byte model of (a)
      is taken against, model_ms = 32 / 12 * fold_ms;
  (d) with --step: the whole ResNet-50 training step (bf16, batch --batch, world 1) with compression off and on at
      rho = 0.01 (the local path: select, residual, zero and scatter, no collective).
Each sample is one event pair around ``--reps`` back-to-back calls; the variants alternate within a round and the figure
is the median over the rounds, per call.  Back-to-back calls over the same 64 MB of arrays run partly out of the
256 MiB Infinity Cache, so the implied rates are not HBM rates.  The expectations are written to the log before anything
is timed; the result line marks each met or not met.  Prints one JSON line and appends it to --log.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

EXPECT = {
    "a_below_b": "compress_bucket's median is below the torch form's at both ratios",
    "a_near_model": "compress_bucket's median is at most 1.5 x its byte model, 32 B per element at the fold kernel's "
                    "measured rate (12 B per element), at both ratios",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=8 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", action="store_true", help="also time whole ResNet-50 training steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "compress_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import GradCompress, TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops import _lib, accum
    from distributed_tensorflow_models_amd.ops import compress as C

    assert torch.cuda.is_available(), "compress_bench needs a GPU"
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(json.dumps({"expectations": EXPECT}) + "\n")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n, W = args.elements, 8
    index = torch.arange(n, device=dev, dtype=torch.int64)

    def torch_form(res, g, k, packet):
        u = res + g
        bits = u.view(torch.int32)
        comp = ((bits & C.KEY_MASK).to(torch.int64) << 31) | (n - 1 - index)  # (key descending, index ascending)
        sel = (n - 1 - (torch.topk(comp, k, sorted=False).values & C.KEY_MASK)).sort().values
        packet[:k] = sel
        packet[k:] = bits[sel]
        u[sel] = 0.0
        res.copy_(torch.where(torch.isfinite(u), u, torch.zeros_like(u)))

    def arrays():
        return torch.randn(n, device=dev) * 1e-2, torch.randn(n, device=dev) * 1e-2

    scratch = torch.zeros(C.scratch_words(n), dtype=torch.int32, device=dev)
    fns, ks = {}, {}
    keep = []
    for rho in (0.01, 0.001):
        k = ks[rho] = C.bucket_k(n, rho)
        # the kernels and the torch form compute the same thing (same seeded inputs, at the timed size, two steps so
        # that the second one starts from a non-zero residual)
        (rk, g), pk, pt = arrays(), torch.zeros(2 * k, dtype=torch.int32, device=dev), None
        rt, pt = rk.clone(), torch.zeros_like(pk)
        for _ in range(2):
            C.compress_bucket(rk, g, k, pk, scratch)
            torch_form(rt, g, k, pt)
            assert torch.equal(pk, pt) and torch.equal(rk.view(torch.int32), rt.view(torch.int32))
        tag = "rho%g" % rho
        packets = torch.stack([torch.cat([torch.randperm(n, device=dev)[:k].sort().values.to(torch.int32),
                                          torch.randn(k, device=dev).view(torch.int32)]) for _ in range(W)])
        gd = torch.zeros(n, device=dev)
        keep.append((rk, rt, g, pk, pt, packets, gd))
        fns["a_compress_" + tag] = lambda rk=rk, g=g, k=k, pk=pk: C.compress_bucket(rk, g, k, pk, scratch)
        fns["b_torch_" + tag] = lambda rt=rt, g=g, k=k, pt=pt: torch_form(rt, g, k, pt)
        fns["c_decompress_w8_" + tag] = lambda gd=gd, packets=packets, k=k: C.decompress_bucket(gd, packets, k)
    L = _lib.lib()
    k = ks[0.01]
    (sr, sg), sp = arrays(), torch.zeros(2 * k, dtype=torch.int32, device=dev)
    C.compress_bucket(sr, sg, k, sp, scratch)

    def stage(bits):
        rc = L.dtm_grad_compress_stages(_lib.ptr(sr), _lib.ptr(sg), n, k, _lib.ptr(sp), _lib.ptr(scratch), bits,
                                        _lib.stream_ptr())
        assert rc == 0, rc

    for name, bits in (("a1_select", 1), ("a2_count_rowscan", 2), ("a3_pack", 4)):
        fns[name + "_rho0.01"] = lambda bits=bits: stage(bits)
    fa, fg = arrays()
    fns["f_fold"] = lambda: accum.grad_accum(fa, fg, accum.FOLD, None)
    res = _alternate(fns, args.rounds, args.reps, args.warmup)

    out = dict(elements=n, rounds=args.rounds, reps=args.reps, k={("%g" % r): k for r, k in ks.items()})
    for name, (med, lo, hi) in res.items():
        out[name + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    fold = res["f_fold"][0]
    out["fold_GBps"] = round(12.0 * n / (fold * 1e-3) / 1e9, 1)
    out["a_model_ms"] = round(32.0 / 12.0 * fold, 4)
    below, near = True, True
    for rho in ks:
        tag = "rho%g" % rho
        a, b = res["a_compress_" + tag][0], res["b_torch_" + tag][0]
        out["b_over_a_" + tag] = round(b / a, 2)
        out["a_over_model_" + tag] = round(a / (32.0 / 12.0 * fold), 2)
        out["a_GBps_" + tag] = round(32.0 * n / (a * 1e-3) / 1e9, 1)
        below &= a < b
        near &= a <= 1.5 * 32.0 / 12.0 * fold
    out["expect_a_below_b"] = "met" if below else "not met"
    out["expect_a_near_model"] = "met" if near else "not met"

    if args.step:
        del keep, fns
        steps = {}
        for name, cfg in (("off", None), ("on", GradCompress(0.01))):
            torch.manual_seed(0)
            net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
            steps[name] = TrainStep(net, optimizer="momentum", lr=0.01, momentum=0.9, grad_compress=cfg)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        sres = _alternate({"off": lambda: steps["off"](x, y), "on": lambda: steps["on"](x, y)},
                          args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for name in ("off", "on"):
            med, lo, hi = sres[name]
            out["step_compress_%s_ms" % name] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        out["step_on_over_off"] = round(sres["on"][0] / sres["off"][0], 4)
        out["step_buckets"] = len(steps["on"].dp.buckets)
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
