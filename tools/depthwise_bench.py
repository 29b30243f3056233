#!/usr/bin/env python3
"""The two depthwise kernel families on the 3x3 depthwise layers of MobileNet v2 1.0 and v1 1.0 (224x224, batch 64).

Per layer and direction (forward, dgrad, wgrad), with HIP events on one GPU and the entry points called directly:
  legacy  dtm_depthwise_*       (dw_*8 where 256 % (C/8) == 0, the scalar kernels elsewhere);
  tile    dtm_depthwise_tile_*  (LDS-tiled, csrc/kernels/depthwise_tile.hip);
  copy    a device-to-device copy of the bytes the op must move (x + y, or x + dy): the byte floor of this run.
Method of tools/optim_bench.py: each sample is one event pair around ``--reps`` back-to-back launches, the arms
alternate within a round, the figure is the median over the rounds with min - max.  With --step the whole mobilenet_v2
and mobilenet_v1 training steps (eager, batch 64) under DTM_DW_IMPL=legacy and =auto; v1's widths all stay on dw_*8
under auto, so that pair is the same launches twice: the run's own noise floor.  The expectations go into the log
before the timed runs, one JSON line after them.  Arrays under 256 MB looped back to back run partly out of the
Infinity Cache: the copy arm shares that advantage, an absolute GB/s figure does not transfer to a training step.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.optim_bench import _alternate  # noqa: E402

# (H = W of the input, C, stride)
V2 = [(112, 32, 1), (112, 96, 2), (56, 144, 1), (56, 144, 2), (28, 192, 1), (28, 192, 2), (14, 384, 1), (14, 576, 1),
      (14, 576, 2), (7, 960, 1)]
V1 = [(112, 32, 1), (112, 64, 2), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1), (14, 512, 2),
      (7, 1024, 1)]
EXPECT = """expectations (no threshold fixed: none of this had been measured)
 (i)   tile is faster than legacy on every layer that auto moves, by more than the legacy arm's min - max spread
 (ii)  tile over its byte floor (the copy arm) is reported per layer and direction
 (iii) on the fast8 layers tile is reported against dw_*8 both ways
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step", action="store_true", help="also time whole MobileNet training steps")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "depthwise_bench.log"))
    args = ap.parse_args()

    import torch

    from distributed_tensorflow_models_amd.ops import _lib
    from distributed_tensorflow_models_amd.ops.depthwise import DwArgs, fast8, resolve_impl
    from distributed_tensorflow_models_amd.ops.geometry import conv_geom

    assert torch.cuda.is_available(), "depthwise_bench needs a GPU"
    dev, L, N = torch.device("cuda", 0), _lib.lib(), args.batch
    log = open(args.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(EXPECT)
    layers, moved_ok, rows = [], True, []
    for H, C, st in sorted(set(V2 + V1), key=lambda t: (-t[0], t[1], t[2])):
        g = conv_geom((N, H, H, C), (C, 3, 3, C), st, "SAME")
        a = DwArgs(N, H, H, C, 1, 3, 3, g.P, g.Q, st, g.pad_h, g.pad_w, 1)
        x = torch.randn(N, H, H, C, device=dev).to(torch.bfloat16)
        dy = torch.randn(N, g.P, g.Q, C, device=dev).to(torch.bfloat16)
        w = torch.randn(3, 3, C, 1, device=dev)
        y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.zeros_like(w)
        xc, dyc = torch.empty_like(x), torch.empty_like(dy)
        s, ar, p = _lib.stream_ptr(), ctypes.byref(a), _lib.ptr

        def op(name, *t):
            fn = getattr(L, name)
            return lambda: fn(*[p(v) for v in t], ar, s)

        def copy2(a0, a1, b0, b1):
            return lambda: (a1.copy_(a0), b1.copy_(b0))

        moved = resolve_impl(a, "auto") == "tile"
        rec = dict(H=H, C=C, stride=st, auto="tile" if moved else "legacy", fast8=bool(fast8(a)))
        for d, arms in (
                ("fwd", dict(legacy=op("dtm_depthwise_fwd", x, w, y), tile=op("dtm_depthwise_tile_fwd", x, w, y),
                             copy=copy2(x, xc, dy, dyc))),
                ("dgrad", dict(legacy=op("dtm_depthwise_dgrad", dy, w, dx),
                               tile=op("dtm_depthwise_tile_dgrad", dy, w, dx), copy=copy2(x, xc, dy, dyc))),
                ("wgrad", dict(legacy=op("dtm_depthwise_wgrad", x, dy, dw),
                               tile=op("dtm_depthwise_tile_wgrad", x, dy, dw), copy=copy2(x, xc, dy, dyc)))):
            r = _alternate(arms, args.rounds, args.reps, args.warmup)
            rec[d] = {k: dict(median=round(v[0], 4), min=round(v[1], 4), max=round(v[2], 4)) for k, v in r.items()}
            leg, til, cp = r["legacy"], r["tile"], r["copy"]
            rec[d]["legacy_over_tile"] = round(leg[0] / til[0], 2)
            rec[d]["tile_over_copy"] = round(til[0] / cp[0], 2)
            met = til[0] < leg[0] - (leg[2] - leg[1])
            if moved:
                rec[d]["i_met"] = bool(met)
                moved_ok = moved_ok and met
            rows.append("| %dx%dx%d s%d | %s | %s | %.4f (%.4f - %.4f) | %.4f (%.4f - %.4f) | %.4f | %.2f | %.2f |" % (
                H, H, C, st, d, rec["auto"], leg[0], leg[1], leg[2], til[0], til[1], til[2], cp[0],
                leg[0] / til[0], til[0] / cp[0]))
        layers.append(rec)
    say("| layer | dir | auto | legacy ms (min - max) | tile ms (min - max) | copy ms | legacy / tile | tile / copy |")
    say("|---|---|---|---|---|---|---|---|")
    for r in rows:
        say(r)
    say("(i) %s" % ("met on every layer auto moves" if moved_ok else "NOT met on: " + ", ".join(
        "%dx%dx%d s%d %s" % (r["H"], r["H"], r["C"], r["stride"], d) for r in layers for d in ("fwd", "dgrad", "wgrad")
        if r[d].get("i_met") is False)))
    out = dict(batch=N, rounds=args.rounds, reps=args.reps, i_met=bool(moved_ok), layers=layers)

    if args.step:
        from distributed_tensorflow_models_amd.engine import TrainStep
        from distributed_tensorflow_models_amd.models import nets_factory
        xb = torch.randn(N, 224, 224, 3, device=dev).to(torch.bfloat16)
        yb = torch.randint(0, 1001, (N,), device=dev)
        for name in ("mobilenet_v2", "mobilenet_v1"):
            torch.manual_seed(0)
            step = TrainStep(nets_factory.build(name, num_classes=1001).to(dev), optimizer="momentum", lr=0.01,
                             momentum=0.9)

            def run(impl, step=step):
                os.environ["DTM_DW_IMPL"] = impl
                return step(xb, yb)
            r = _alternate({k: (lambda k=k: run(k)) for k in ("legacy", "auto")}, 5, 4, 3)
            out["step_" + name] = {k: dict(median=round(v[0], 3), min=round(v[1], 3), max=round(v[2], 3))
                                   for k, v in r.items()}
            out["step_" + name]["legacy_over_auto"] = round(r["legacy"][0] / r["auto"][0], 3)
            say("step %s batch %d: legacy %.3f ms (%.3f - %.3f), auto %.3f ms (%.3f - %.3f)" % (
                (name, N) + r["legacy"] + r["auto"]))
            del step
        os.environ.pop("DTM_DW_IMPL", None)
    say(json.dumps(out))


if __name__ == "__main__":
    main()
