"""The fused fake-quantisation definitions (ops/fakequant.py) in torch ops on the CPU against the torch-op path of
compat/quantize.py: values, gradients, range state, the non-finite rule, and a whole MobileNet."""
import pytest
import torch

from distributed_tensorflow_models_amd.compat import quantize as Q
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import fakequant as FQ


def tie_points(scale):
    """Every (k + 0.5) * scale for k in -300..300: the rounding ties of a quantiser with that scale."""
    return (torch.arange(-300, 301, dtype=torch.float32) + 0.5) * scale


def make_cases():
    """name -> fp32 tensor; shared with tests/test_fakequant_gpu.py."""
    g = torch.Generator().manual_seed(11)
    cases = {
        "random": torch.randn(4099, generator=g) * 1.7 + 0.3,
        "positive": torch.rand(515, generator=g) * 5.0 + 0.25,
        "negative": -torch.rand(515, generator=g) * 3.0 - 0.5,
        "zero": torch.zeros(130),
    }
    # ties of the 8-bit full-range and narrow-range grids of a tensor spanning [-1.5, 2.5], and of a 4-bit grid
    for name, steps in (("ties255", 255.0), ("ties254", 254.0), ("ties15", 15.0)):
        cases[name] = torch.cat([tie_points(4.0 / steps), torch.tensor([-1.5, 2.5])])
    return cases


class Cfg:
    """The part of QuantConfig that FQ.quantize reads, with a CPU counter."""

    def __init__(self, step=0, quant_delay=0, num_bits=8, ema_decay=0.999, is_training=True):
        self.quant_delay, self.num_bits, self.ema_decay = quant_delay, num_bits, ema_decay
        self.is_training = is_training
        self._c = torch.tensor([step], dtype=torch.int64)

    def counter(self, device):
        return self._c


def _vars(lo=0.0, hi=0.0):
    return torch.nn.Parameter(torch.tensor(lo), requires_grad=False), \
        torch.nn.Parameter(torch.tensor(hi), requires_grad=False)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("narrow", [False, True], ids=["full", "narrow"])
def test_cpu_path_equals_fake_quant(narrow, bits):
    for name, x in make_cases().items():
        # the tensor's own range, then one that leaves inputs outside on both sides
        for rng in ((float(x.min()), float(x.max())), (-0.75, 1.25)):
            vmin, vmax = _vars(*rng)
            a = x.clone().requires_grad_()
            b = x.clone().requires_grad_()
            ya = FQ.quantize(a, vmin, vmax, Cfg(num_bits=bits, is_training=False), FQ.FROZEN, narrow)
            yb = Q.fake_quant(b, vmin.detach(), vmax.detach(), bits, narrow)
            dy = torch.arange(x.numel(), dtype=torch.float32) % 7 - 3.0
            ya.backward(dy)
            yb.backward(dy)
            assert torch.equal(ya, yb), (name, rng)
            assert torch.equal(a.grad, b.grad), (name, rng)
            assert float(vmin) == rng[0] and float(vmax) == rng[1]  # FROZEN reads only
    # the all-zero tensor takes the scale -> 1 branch
    vmin, vmax = _vars()
    FQ.quantize(torch.zeros(5), vmin, vmax, Cfg(), FQ.WEIGHTS, narrow)
    rec = FQ.state_of(vmin).record()
    assert rec["scale"] == 1.0 and rec["inv_scale"] == 1.0 and rec["zp"] == float(narrow)


def test_range_state_equals_torch_op_path():
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(3, 17, generator=g) * (i + 1) - 0.4 * i for i in range(3)]
    store_a, store_b = {}, {}

    def var_fn(store):
        def fn(name, init):
            if name not in store:
                store[name] = torch.nn.Parameter(torch.tensor(float(init)), requires_grad=False)
            return store[name]
        return fn

    cfg_a, cfg_b = Q.QuantConfig(fused=True), Q.QuantConfig()
    for x in xs:
        for dt in (torch.float32, torch.bfloat16):
            ya = Q.quantize_activations(x.to(dt), var_fn(store_a), cfg_a, True)
            yb = Q.quantize_activations(x.to(dt), var_fn(store_b), cfg_b, True)
            assert torch.equal(ya, yb)
        wa = Q.quantize_weights(x, var_fn(store_a), cfg_a)
        wb = Q.quantize_weights(x, var_fn(store_b), cfg_b)
        assert torch.equal(wa, wb)
    assert set(store_a) == set(store_b) == {"act_quant/min", "act_quant/max", "weights_quant/min", "weights_quant/max"}
    for n in store_a:
        assert torch.equal(store_a[n], store_b[n]), n
    assert float(store_a["act_quant/max"]) != 6.0 and float(store_a["weights_quant/min"]) < 0


@pytest.mark.parametrize("mode", [FQ.ACT_TRAIN, FQ.WEIGHTS])
def test_nonfinite_batches_leave_the_range_alone(mode):
    vmin, vmax = _vars(-1.0, 2.0)
    cfg = Cfg()
    good = torch.linspace(-3.0, 4.0, 50)
    FQ.quantize(good, vmin, vmax, cfg, mode, False)
    before = (float(vmin), float(vmax))
    assert before != (-1.0, 2.0)
    for bad in (float("nan"), float("inf")):
        x = good.clone()
        x[7] = bad
        x.requires_grad_()
        y = FQ.quantize(x, vmin, vmax, cfg, mode, False)
        y.backward(torch.ones_like(y))
        assert (float(vmin), float(vmax)) == before
        if bad != bad:
            assert bool(torch.isnan(y[7]))  # the NaN passes through, so the optimizer's guard still sees it
        else:
            yd = y.detach()
            assert float(yd[7]) == float(yd[torch.isfinite(yd)].max())  # +Inf clamps to the upper end of the range
        assert float(x.grad[7]) == 0.0
        keep = torch.ones(50, dtype=torch.bool)
        keep[7] = False
        assert bool(torch.isfinite(y.detach()[keep]).all())
    assert FQ.state_of(vmin).record()["nonfinite_batches"] == 2


def _mobilenet(cfg):
    torch.manual_seed(0)
    return nets_factory.build("mobilenet_v1_025", num_classes=11, quantize=cfg)


def test_mobilenet_fused_equals_unfused_cpu():
    from distributed_tensorflow_models_amd.ops import elementwise as E
    outs = []
    for fused in (True, False):
        cfg = Q.QuantConfig(quant_delay=2, fused=fused)
        net = _mobilenet(cfg)
        g = torch.Generator().manual_seed(2)
        logits = []
        for i in range(3):
            x = torch.randn(2, 64, 64, 3, generator=g)
            E._seed[0] = 7 + i  # the same dropout masks in both models
            out = net(x, training=True)
            logits.append(out.detach().clone())
        out.float().square().mean().backward()
        grads = {n: v.grad.clone() for n, v in net.store.vars.items() if v.grad is not None}
        qvars = {n: v.detach().clone() for n, v in net.store.vars.items() if "_quant/" in n}
        assert cfg.step == 3 and cfg.steps_done() == 3
        outs.append((logits, grads, qvars))
    (la, ga, qa), (lb, gb, qb) = outs
    for a, b in zip(la, lb):
        assert torch.equal(a, b)
    assert not torch.equal(la[1], la[2])
    assert set(ga) == set(gb) and len(ga) > 20
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    assert set(qa) == set(qb) and len(qa) == 4 * 28
    for n in qa:
        assert torch.equal(qa[n], qb[n]), n


def test_eval_graph_fused_reads_stored_ranges():
    """QuantConfig(is_training=False, fused=True), the evaluator's config: FROZEN quantisers, active whatever the
    delay, that read the ranges on record (the weights' too, as TF's eval graph does) and leave them alone."""
    a = _mobilenet(Q.QuantConfig(quant_delay=10 ** 9, is_training=False, fused=True))
    b = _mobilenet(Q.QuantConfig(is_training=False))
    a.load_state_dict(b.state_dict())  # (the unfused build pass recorded weight ranges)
    before = {n: v.detach().clone() for n, v in a.store.vars.items() if "_quant/" in n}
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        ya = a(x, training=False)
    assert len(before) == 4 * 28 and all(torch.equal(v, a.store.vars[n]) for n, v in before.items())
    assert a.store.quant.steps_done() == 0 and bool(torch.isfinite(ya).all())
    recs = [st.record() for st in FQ.quantizer_states(a)]
    assert len(recs) == 2 * 28 and all(r["active"] == 1 and r["nonfinite_batches"] == 0 for r in recs)
    w0 = [r for r in recs if r["qmin"] == 1.0][0]  # the first weight quantiser: the range on record, narrow
    lo, hi = (float(a.store.vars["MobilenetV1/Conv2d_0/weights_quant/" + k]) for k in ("min", "max"))
    assert lo < 0 < hi and w0["scale"] == float((torch.tensor(hi) - torch.tensor(lo)) / 254.0)


def test_train_entry_quant_fused_metrics(tmp_path):
    """mobilenet_v1_train --quantize --quant_fused: the metrics line carries the device step count and the skipped
    range updates, the checkpoint the same quantiser variables."""
    import json
    import os
    import subprocess
    import sys
    from distributed_tensorflow_models_amd.ckpt.bundle import BundleReader
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", "distributed_tensorflow_models_amd.trainers.mobilenet_v1_train",
                        "--quantize", "--quant_fused", "--quant_delay=1", "--max_steps=2", "--batch_size=2",
                        "--train_dir=" + d, "--data_dir=/nonexistent", "--synthetic_data", "--depth_multiplier=0.25",
                        "--metrics_file=" + mf], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [json.loads(l) for l in open(mf) if l.startswith("{")]
    assert lines and lines[-1]["quant_step"] == 2 and lines[-1]["quant_nonfinite_batches"] == 0
    rd = BundleReader(os.path.join(d, "model.ckpt-2"))
    names = set(rd.names())
    assert sum(n.endswith(("act_quant/min", "act_quant/max", "weights_quant/min", "weights_quant/max"))
               for n in names) == 4 * 28
