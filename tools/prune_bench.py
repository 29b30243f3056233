#!/usr/bin/env python3
"""Cost of gradual magnitude pruning (csrc/kernels/prune.hip) over ResNet-50's pruned tensors (its dim() >= 2 weights,
about 25.5 M elements) with bf16 copies, at sparsity 0.5, with the method of tools/accum_bench.py.

HIP events on one GPU:
  (a)  an update step of the pruner (pre-apply + select stages + mask write + apply), from dense weights: every
       sample restores the weights and the masks first, and (a0) times that restore alone; (a_steady) repeats the
       update on the weights it has already pruned (half of them zeros: the first digit's hottest bin);
  (b)  the torch form: per tensor ``torch.kthvalue`` on the int32 keys plus ``torch.where`` on the weight and its bf16
       copy, checked equal to the kernels bit for bit at the timed size first;
  (c)  a non-update step (the early exits + apply);
  (d)  the first digit's histogram launch alone, on standard-normal * 0.05 values, on a trained-weight-like set
       with few exponents (uniform magnitudes in [0.01, 0.04), two exponents) and on the first set with half of it
       zeros (what an update after the first one sees);
  (e)  with --step: the whole ResNet-50 training step (bf16, batch --batch) without pruning, with pruning on a
       non-update step and with pruning on an update step.
Each sample is one event pair around ``--reps`` back-to-back calls; the variants alternate within a round and the
figure is the median over the rounds, per call.  The byte floor of an update is digits x 4 B + apply (4 B read + 1 B
mask written, and 4 + 4 + 2 + 2 B where a group of four holds a pruned element) per element; the implied bytes/s divide
it by the time.  Back-to-back loops over these 0.1 GB of weights run partly from the 256 MiB Infinity Cache, so these
are not HBM rates.  Prints one JSON line and appends it to --log.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

SPARSITY = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-rounds", type=int, default=3, help="rounds of the (slow) torch form, one call each")
    ap.add_argument("--step", action="store_true", help="also time whole ResNet-50 training steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--step-reps", type=int, default=4)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "prune_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.engine import PruneConfig, TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.ops import _lib, prune

    assert torch.cuda.is_available(), "prune_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in nets_factory.build("resnet_v1_50", num_classes=1000).parameters()
              if p.requires_grad and p.dim() >= 2]
    numel = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numel)

    def carve(flat):
        out, pos = [], 0
        for s, n in zip(shapes, numel):
            out.append(flat[pos:pos + n].view(s))
            pos += (n + 3) // 4 * 4
        return out

    span = sum((n + 3) // 4 * 4 for n in numel)
    g = torch.Generator(dev).manual_seed(0)
    src = {"normal": torch.randn(span, device=dev, generator=g) * 0.05}
    few = 0.01 + 0.03 * torch.rand(span, device=dev, generator=g)
    src["fewexp"] = torch.where(torch.rand(span, device=dev, generator=g) < 0.5, few, -few)
    src["halfzero"] = torch.where(torch.rand(span, device=dev, generator=g) < 0.5, src["normal"],
                                  torch.zeros((), device=dev))
    w = src["normal"].clone()
    w16_src = w.to(torch.bfloat16)
    w16 = w16_src.clone()
    ws, w16s = carve(w), carve(w16)
    pr = prune.Pruner([("t%d" % i, a, b, None) for i, (a, b) in enumerate(zip(ws, w16s))])

    def restore(name="normal"):
        w.copy_(src[name])
        w16.copy_(w16_src)
        pr.reset()

    # ---- (b) the torch form, and equality with the kernels at the timed size ------------------------------------
    tw, tw16 = src["normal"].clone(), w16_src.clone()
    tws, tw16s = carve(tw), carve(tw16)

    def torch_form():
        out = []
        for a, b in zip(tws, tw16s):
            n = a.numel()
            key = a.view(-1).view(torch.int32) & 0x7FFFFFFF
            tau = torch.kthvalue(key, int(SPARSITY * n)).values
            keep = (key > tau).view(a.shape)
            a.copy_(torch.where(keep, a, torch.zeros((), device=dev)))
            b.copy_(torch.where(keep, b, torch.zeros((), device=dev, dtype=torch.bfloat16)))
            out.append((keep, tau))
        return out

    restore()
    pr.step(SPARSITY, True)
    ref = torch_form()
    torch.cuda.synchronize()
    assert torch.equal(w, tw) and torch.equal(w16, tw16)
    for i, (keep, tau) in enumerate(ref):
        assert torch.equal(pr.masks[i].bool(), keep) and int(pr.tau[i]) == int(tau)
    achieved = pr.sparsity()

    def torch_fresh():
        tw.copy_(src["normal"])
        tw16.copy_(w16_src)
        torch_form()

    def update_fresh():
        restore()
        pr.step(SPARSITY, True)

    L = _lib.lib()

    def hist0():
        rc = L.dtm_prune_hist_stage(_lib.ptr(pr._tens_dev), len(pr.entries), _lib.ptr(pr._chunks_dev), pr._nchunks,
                                    _lib.ptr(pr._rec), _lib.ptr(pr._state), _lib.ptr(pr.z), _lib.ptr(pr._hist), 0,
                                    pr._max_n, _lib.stream_ptr())
        assert rc == 0

    res = _alternate({
        "a_update": update_fresh,
        "a0_restore": restore,
        "a_steady_update": lambda: pr.step(SPARSITY, True),
        "c_non_update": lambda: pr.step(SPARSITY, False),
    }, args.rounds, args.reps, args.warmup)
    res.update(_alternate({"b_torch_kthvalue_where": torch_fresh, "b0_torch_restore": lambda: (
        tw.copy_(src["normal"]), tw16.copy_(w16_src))}, args.torch_rounds, 1, 1))
    # (d): z as a select at 0.5 left it (every tensor takes part), the prefix 0 of the first digit; the record
    # says update
    for name in ("normal", "fewexp", "halfzero"):
        restore(name)
        pr.stage(SPARSITY, True)
        pr.launch_select()
        pr._state.zero_()
        w.copy_(src[name])
        res.update(_alternate({"d_hist_digit0_%s" % name: hist0}, args.rounds, args.reps, args.warmup))

    out = dict(elements=total, tensors=len(shapes), chunks=pr._nchunks, sparsity=SPARSITY,
               achieved_sparsity=round(achieved, 6), rounds=args.rounds, reps=args.reps)
    for k, (med, lo, hi) in res.items():
        out[k + "_ms"] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
    upd = res["a_update"][0] - res["a0_restore"][0]
    tor = res["b_torch_kthvalue_where"][0] - res["b0_torch_restore"][0]
    out["a_update_net_ms"] = round(upd, 4)
    out["b_torch_net_ms"] = round(tor, 4)
    out["b_torch_over_kernels"] = round(tor / upd, 2)
    # pre-apply on all-ones masks reads 1 B; three digits read 4 B each; apply reads 4, writes 1 and, in (nearly)
    # every group of four at sparsity 0.5, writes 4 and reads + writes the 2-byte copy
    floor_update = total * (1.0 + 3 * 4.0 + 4.0 + 1.0 + 4.0 + 2.0 + 2.0)
    floor_apply = total * (1.0 + 4.0 + 4.0 + 2.0 + 2.0)
    out["a_update_floor_GB"] = round(floor_update / 1e9, 4)
    out["a_update_implied_GBps"] = round(floor_update / (upd * 1e-3) / 1e9, 1)
    out["c_non_update_implied_GBps"] = round(floor_apply / (res["c_non_update"][0] * 1e-3) / 1e9, 1)
    for name in ("normal", "fewexp", "halfzero"):
        out["d_hist_digit0_%s_GBps" % name] = round(4.0 * total / (res["d_hist_digit0_%s" % name][0] * 1e-3) / 1e9, 1)

    if args.step:
        del w, w16, tw, tw16, src, pr
        never, always = 10 ** 9, dict(initial_sparsity=SPARSITY, begin_step=0, end_step=10 ** 9, frequency=1)
        cfgs = {"none": None, "non_update": PruneConfig(SPARSITY, begin_step=never, end_step=never),
                "update": PruneConfig(SPARSITY, **always)}
        steps = {}
        for k, cfg in cfgs.items():
            torch.manual_seed(0)
            net = nets_factory.build("resnet_v1_50", num_classes=1000).to(dev)
            steps[k] = TrainStep(net, optimizer="momentum", lr=0.01, momentum=0.9, prune=cfg)
        if cfgs["non_update"] is not None:  # masks at 0.5 for the arm that only applies them
            steps["non_update"].pruner.step(SPARSITY, True)
        x = torch.randn(args.batch, 224, 224, 3, device=dev).to(torch.bfloat16)
        y = torch.randint(0, 1000, (args.batch,), device=dev)
        sres = _alternate({k: (lambda s=s: s(x, y)) for k, s in steps.items()}, args.step_rounds, args.step_reps, 3)
        out["batch"] = args.batch
        for k, (med, lo, hi) in sres.items():
            out["e_step_%s_ms" % k] = dict(median=round(med, 3), min=round(lo, 3), max=round(hi, 3))
        base = sres["none"][0]
        out["e_non_update_over_none"] = round(sres["non_update"][0] / base, 4)
        out["e_update_over_none"] = round(sres["update"][0] / base, 4)
        out["e_expected_non_update_over_none"] = round(1.0 + res["c_non_update"][0] / base, 4)
        out["e_pruned_elements"] = sum(steps["update"].pruner.numel)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
