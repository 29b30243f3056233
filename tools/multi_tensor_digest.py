#!/usr/bin/env python3
"""sha256 of every output of the multi-tensor kernels (optimizer / norm / Adam / LAMB passes, SAM, summary statistics,
evaluation metrics) and of the softmax cross-entropy family, from seeded inputs at the smallest shapes that reach
every branch of the row walk (csrc/kernels/chunk_walk.h): one `<case> <output> <sha256>` line each.

Usage: python tools/multi_tensor_digest.py OUT.txt
       python tools/multi_tensor_digest.py --compare A.txt B.txt      (prints "<n> A, <n> B, <k> differ"; exit 1 if k)
Compare two library builds with DTM_KERNELS_SO (the C ABI is the same: tools/ab_prepare.sh builds a baseline).  Every
sum in these kernels has a fixed order, so two runs of one build give the same file."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CH = 8192
LENS = [1, 2, 3, 4, 5, 255, 256, 257, 1027, CH - 1, CH, CH + 1, 3 * CH + 5, 65 * CH + 3]
OFFS = [(0, 0), (1, 1), (3, 3), (0, 1), (2, 3)]  # element offsets of weight and gradient from a 16-byte boundary


def compare(a, b):
    da, db = ({tuple(l.split()[:2]): l.split()[2] for l in open(p) if l.strip()} for p in (a, b))
    bad = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    for k in bad[:40]:
        print("DIFFER", *k)
    print("%d %s, %d %s, %d differ" % (len(da), os.path.basename(a), len(db), os.path.basename(b), len(bad)))
    return 1 if bad else 0


def main(out_path):
    import torch

    from distributed_tensorflow_models_amd.ops import _lib
    from distributed_tensorflow_models_amd.ops.metrics import StreamingMetrics
    from distributed_tensorflow_models_amd.ops.optim import KINDS, FusedOptimizer
    from distributed_tensorflow_models_amd.ops.sam import SamConfig, SamPerturber
    from distributed_tensorflow_models_amd.ops.summary import TensorStats

    dev = torch.device("cuda")
    lines = []

    def put(case, name, t):
        raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
        lines.append("%s %s %s" % (case, name, hashlib.sha256(raw).hexdigest()))

    def put_all(case, name, ts):
        h = hashlib.sha256()
        for t in ts:
            h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
        lines.append("%s %s %s" % (case, name, h.hexdigest()))

    def at_offset(n, off, dtype=torch.float32, fill=None):
        """n elements that start ``off`` elements past a 16-byte boundary (fresh allocations are 256-byte aligned)."""
        buf = torch.empty(n + off, dtype=dtype, device=dev)
        v = buf[off:]
        assert v.data_ptr() % 16 == (off * buf.element_size()) % 16
        if fill is not None:
            v.copy_(fill)
        return v

    def rows(seed):
        """(weight, gradient, bf16 copy or None) per length x offset pair; the copy follows the weight's offset, is
        absent, or sits one element further (so its 8-byte stores would be misaligned), in turn."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        out = []
        for n in LENS:
            for po, go in OFFS:
                p = at_offset(n, po, fill=torch.randn(n, generator=g))
                gr = at_offset(n, go, fill=torch.randn(n, generator=g) * 0.1)
                k = len(out) % 3
                cp = None if k == 1 else at_offset(n, po + (1 if k == 2 else 0), torch.bfloat16, fill=p)
                out.append((p, gr, cp))
        return out

    # ---- optimizer kinds, the norm pass, Adam, LAMB ------------------------------------------------------------
    def optimizer(case, kind, seed, ema, clip=None, steps=2, direct=False):
        params = []
        for p, gr, cp in rows(seed):
            q = torch.nn.Parameter(p)
            assert q.data_ptr() == p.data_ptr()
            q.main_grad = gr
            if cp is not None:
                q.bf16 = cp
            params.append(q)
        g = torch.Generator(device="cpu").manual_seed(seed + 1)
        bufs = [torch.randn(n, generator=g).to(dev) for n in (1, 257, CH + 1)] if ema else []  # EMA-only rows
        skip = {id(q) for q in params[::4]}  # not adapted (LARS / LAMB)
        opt = FusedOptimizer(params, kind=kind, lr=0.1, ema_decay=0.999 if ema else None, weight_decay=1e-4,
                             ema_buffers=bufs, clip_global_norm=clip, lars_skip=lambda q: id(q) in skip)
        for s in range(steps):
            opt.set_dynamic(0.05 / (s + 1), grad_scale=0.5)
            opt.launch()
            for b in bufs:
                b.mul_(1.25)
        if direct:  # dtm_multi_tensor_opt_scaled itself: per-tensor rate factors alone, then with a clip factor too
            L = _lib.lib()
            scale = (0.5 + torch.rand(len(params) + len(bufs), generator=g)).to(dev)
            clipf = torch.full((1,), 0.75, device=dev)
            for gc in (None, clipf):
                L.dtm_multi_tensor_opt_scaled(_lib.ptr(opt._tens_dev), _lib.ptr(opt._chunks_dev), opt._nchunks,
                                              KINDS[kind], 0.0, 0.9, 0.9, 1e-10, 1.0, 0.0, int(ema), None,
                                              _lib.ptr(opt._dyn), _lib.ptr(scale), _lib.ptr(gc), _lib.stream_ptr())
        torch.cuda.synchronize()
        put_all(case, "p", [q.data for q in params])
        put_all(case, "pcopy", [q.bf16 for q in params if hasattr(q, "bf16")])
        for slot in ("s1", "s2", "ema"):
            ts = [opt.state[q][slot] for q in params if slot in opt.state[q]]
            if ts:
                put_all(case, slot, ts)
        if bufs:
            put_all(case, "buffer_ema", [opt.buffer_ema[id(b)] for b in bufs])
        if opt.normed:
            put(case, "norms", opt.last_norms())
            put(case, "lr_scale", opt.last_lr_scale())
            put(case, "gclip", opt._gclip)
        if kind in ("adam", "lamb"):
            put(case, "state", opt._adam_state)
        return opt

    for kind in ("sgd", "momentum", "rmsprop"):  # dtm_multi_tensor_opt_scaled without and with gclip
        optimizer("opt_%s" % kind, kind, 10, ema=False)
        optimizer("opt_%s_ema" % kind, kind, 11, ema=True)
        optimizer("opt_%s_clip_ema" % kind, kind, 12, ema=True, clip=0.5)
        optimizer("opt_%s_scaled_ema" % kind, kind, 9, ema=True, direct=True)  # ... with lr_scale, every kind
    optimizer("opt_lars", "lars", 13, ema=False)  # ... with lr_scale
    optimizer("opt_lars_ema", "lars", 14, ema=True)
    opt = optimizer("adam_clip_ema", "adam", 15, ema=True, clip=0.5)
    opt.launch_norms()  # dtm_multi_tensor_norms alone, over the updated weights
    torch.cuda.synchronize()
    put("norms_alone", "norms", opt.last_norms())
    put("norms_alone", "gclip", opt._gclip)
    optimizer("adam", "adam", 16, ema=False)
    optimizer("adam_ema", "adam", 17, ema=True)
    optimizer("lamb", "lamb", 18, ema=False)
    optimizer("lamb_ema", "lamb", 19, ema=True)

    # ---- SAM / ASAM --------------------------------------------------------------------------------------------
    for adaptive in (False, True):
        case = "asam" if adaptive else "sam"
        ent = rows(20 + adaptive)
        g = torch.Generator(device="cpu").manual_seed(30)
        bufs = [torch.randn(n, generator=g).to(dev) for n in (3, CH + 5)]  # backup-only rows
        sp = SamPerturber(ent, buffers=bufs, config=SamConfig(0.05 if not adaptive else 1.0, adaptive=adaptive))
        sp.perturb()
        torch.cuda.synchronize()
        put(case, "rec", sp._rec)
        put_all(case, "p_hat", [e[0] for e in ent])
        put_all(case, "g", [e[1] for e in ent])
        put_all(case, "pcopy_hat", [e[2] for e in ent if e[2] is not None])
        put_all(case, "backup", [r[2] for r in sp.rows])
        for b in bufs:
            b.add_(1.0)
        sp.restore()
        torch.cuda.synchronize()
        put_all(case, "p_restored", [e[0] for e in ent] + bufs)
        put_all(case, "pcopy_restored", [e[2] for e in ent if e[2] is not None])

    # ---- summary statistics (32768-element rows), fp32 and bf16 -----------------------------------------------
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        g = torch.Generator(device="cpu").manual_seed(40)
        ts = []
        for n in LENS + [32767, 32768, 32769]:
            for off in (0, 1, 3, 5):
                x = torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-6, 6, (1,), generator=g))
                if n >= 5:
                    x[0], x[n // 2], x[n - 1], x[1] = 0.0, float("nan"), float("inf"), -0.0
                ts.append(at_offset(n, off, dtype, fill=x))
        st = TensorStats(ts, scales=[1.0 if i % 2 else 0.5 for i in range(len(ts))])
        st.launch()
        torch.cuda.synchronize()
        put("stats_" + name, "bins", st._bins_host)
        put("stats_" + name, "results", st._results_host)

    # ---- evaluation metrics and the softmax cross-entropy family ----------------------------------------------
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream_ptr
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        for C in (1, 10, 65, 1001):
            for B in (1, 5):
                for off in (0, 1):  # the first row one element past a 16-byte boundary
                    case = "%s_C%d_B%d_o%d" % (name, C, B, off)
                    g = torch.Generator(device="cpu").manual_seed(50 + C + B)
                    x = at_offset(B * C, off, dtype, fill=torch.randn(B * C, generator=g) * 3.0).view(B, C)
                    z = at_offset(B * C, off, dtype, fill=torch.randn(B * C, generator=g) * 3.0).view(B, C)
                    lab = torch.randint(0, C, (B,), generator=g, dtype=torch.int32).to(dev)
                    m = StreamingMetrics(C, k=min(5, C), confusion=C <= 65, device=dev)
                    m.update(x, lab)
                    m.update(x, lab.long())
                    torch.cuda.synchronize()
                    put("metrics_" + case, "rec", m._rec)
                    put("metrics_" + case, "rowloss", m._rowloss)
                    put("metrics_" + case, "flags", m._flags)

                    bf = int(dtype == torch.bfloat16)
                    loss = torch.zeros(B, device=dev)
                    kl = torch.zeros(B, device=dev)
                    d = torch.zeros(B, C, dtype=dtype, device=dev)
                    w = torch.rand(B, generator=g).to(dev)
                    L.dtm_softmax_xent(P(x), bf, P(lab), P(loss), P(d), B, C, 0.1, 1.0 / B, P(w), C, S())
                    torch.cuda.synchronize()
                    put("xent_" + case, "loss", loss)
                    put("xent_" + case, "dlogits", d)
                    plan = torch.zeros(B, 8, dtype=torch.int32)
                    plan[:, 0] = torch.randperm(B, generator=g).int()
                    plan[:, 2] = torch.rand(B, generator=g).view(torch.int32)
                    plan[0, 2] = torch.ones(1).view(torch.int32)[0]  # wl == 1: the plain kernel's expressions
                    plan = plan.to(dev)
                    rc = L.dtm_softmax_xent_mix(P(x), bf, P(lab), P(plan), P(loss), P(d), B, C, 0.1, 1.0 / B, C, S())
                    assert rc == 0, rc
                    torch.cuda.synchronize()
                    put("xent_mix_" + case, "loss", loss)
                    put("xent_mix_" + case, "dlogits", d)
                    for pl, pname in ((None, "distill"), (plan, "distill_mix")):
                        rc = L.dtm_softmax_xent_distill(P(x), bf, P(z), C, P(lab), P(pl), P(loss), P(kl), P(d), B, C,
                                                        0.1, 0.7, 2.0, 1.0 / B, C, S())
                        assert rc == 0, rc
                        torch.cuda.synchronize()
                        put("xent_%s_%s" % (pname, case), "loss", loss)
                        put("xent_%s_%s" % (pname, case), "kl", kl)
                        put("xent_%s_%s" % (pname, case), "dlogits", d)

    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d digests -> %s (library %s)" % (len(lines), out_path, _lib.LIB_PATH))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
