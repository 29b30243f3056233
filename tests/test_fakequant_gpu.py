"""The fake-quantisation kernels (csrc/kernels/fakequant.hip) against the torch-op definitions of ops/fakequant.py on
the CPU, exactly; the inactive path; the non-finite rule; a captured MobileNet step replayed across the quant_delay
boundary against the eager run; the fused path against the unfused one on the GPU."""
import math

import pytest
import torch

from distributed_tensorflow_models_amd.compat import quantize as Q
from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops import fakequant as FQ
from test_fakequant_cpu import tie_points

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 63, 64, 65, 4095, 8192 * 3 + 5)
OFFSETS = (0, 1, 3)
PER_VEC = {torch.float32: 4, torch.bfloat16: 8}
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def base():
    """One fp32 value pool in [-1.5, 2.5] (the ties of the 255-, 254- and 15-step grids of that span in front),
    shared by every case and never written."""
    g = torch.Generator().manual_seed(21)
    ties = torch.cat([tie_points(4.0 / s) for s in (255.0, 254.0, 15.0)])
    ties = ties[(ties > -1.5) & (ties < 2.5)]
    pool = torch.cat([ties, torch.rand(SIZES[-1], generator=g) * 4.0 - 1.5])
    dy = torch.randn(SIZES[-1], generator=g)
    return pool, dy


def _placed(dev_dtype_buf, off, src):
    """``src`` (CPU) copied into a fresh 16-byte-aligned device buffer at element ``off``; the view is returned."""
    n = src.numel()
    buf = torch.zeros(n + 16, dtype=src.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n]
    v.copy_(src)
    dev_dtype_buf.append(buf)
    return v


def _positions(n, off, dtype):
    """Where the extremes go: the head element, the tail element, the last element of the 16-byte body (the last
    element the last block loads as part of a vector)."""
    pv = PER_VEC[dtype]
    head = min((-off) % pv, n)
    body_end = head + (n - head) // pv * pv
    return sorted({0, n - 1, max(body_end - 1, 0)})


def _vars(device, lo, hi):
    return torch.tensor(lo, device=device), torch.tensor(hi, device=device)


def _pipeline(x, dy, device, off, y_off, mode, narrow, bits, step, delay, init=(-0.75, 1.25), training_cfg=True,
              hold=None):
    """range + finalize + apply + apply_bwd of one quantiser on ``device``; x, dy: CPU tensors of the case's dtype."""
    vmin, vmax = _vars(device, *init)
    counter = torch.tensor([step], dtype=torch.int64, device=device)
    st = FQ.QuantizerState(device)
    if device.type == "cuda":
        xd, dyd = _placed(hold, off, x), _placed(hold, off, dy)
        y, dx = _placed(hold, y_off, torch.zeros_like(x)), _placed(hold, y_off, torch.zeros_like(x))
    else:
        xd, dyd, y, dx = x, dy, torch.zeros_like(x), torch.zeros_like(x)
    FQ.finalize(xd, vmin, vmax, st, counter, mode, 0.999, bits, narrow, delay, training_cfg)
    FQ.apply_into(xd, y, st.rec)
    FQ.apply_bwd_into(xd, dyd, dx, st.rec)
    return y.cpu(), dx.cpu(), float(vmin), float(vmax), st.record()


def _case_input(base, n, dtype, pos):
    pool, dyp = base
    x = pool[:n].clone()
    x[pos] = 2.5            # the maximum ...
    x[(pos + n // 2) % n] = -1.5 if n > 1 else 2.5  # ... and, half the tensor away, the minimum
    return x.to(dtype), dyp[:n].to(dtype)


@pytest.mark.parametrize("narrow,bits", [(False, 8), (True, 8), (False, 4), (True, 4)],
                         ids=["full8", "narrow8", "full4", "narrow4"])
@pytest.mark.parametrize("mode", [FQ.WEIGHTS, FQ.ACT_TRAIN, FQ.FROZEN], ids=["weights", "act_train", "frozen"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_kernels_equal_cpu_oracle(base, dtype, mode, narrow, bits):
    big = SIZES[-1]
    grid, threads = FQ.grid_size(big, dtype), FQ.block_threads()
    assert grid > 1 and big // PER_VEC[dtype] > grid * threads  # more than one block, more than one grid-stride trip
    for n in SIZES:
        for off in OFFSETS:
            # the outputs at the input's offset (16-byte path with a scalar head), and for one offset shifted against
            # it (the element-wise path)
            for y_off in ((off, off + 1) if off == 1 else (off,)):
                for pos in _positions(n, off, dtype):
                    x, dy = _case_input(base, n, dtype, pos)
                    hold = []
                    got = _pipeline(x, dy, DEV, off, y_off, mode, narrow, bits, 5, 3, hold=hold)
                    want = _pipeline(x, dy, torch.device("cpu"), 0, 0, mode, narrow, bits, 5, 3)
                    tag = (n, off, y_off, pos)
                    assert want[4]["active"] == 1
                    assert got[2:] == want[2:], tag            # vmin, vmax and the record
                    assert torch.equal(got[0], want[0]), tag   # y
                    assert torch.equal(got[1], want[1]), tag   # dx
                    assert ((want[2], want[3]) == (-0.75, 1.25)) == (mode == FQ.FROZEN)
                    if n >= 4095 and mode != FQ.WEIGHTS:
                        # the range is about [-0.75, 1.25]: the straight-through mask cuts the inputs beyond it on
                        # both sides and passes the ones well inside
                        xf, dxw = x.float(), want[1]
                        assert bool((dxw[xf < -1.0] == 0).all()) and bool((xf < -1.0).any())
                        assert bool((dxw[xf > 2.0] == 0).all()) and bool((xf > 2.0).any())
                        inside = (xf > -0.5) & (xf < 1.0)
                        assert torch.equal(dxw[inside], dy[inside]) and bool(inside.any())


@pytest.mark.parametrize("mode", [FQ.WEIGHTS, FQ.ACT_TRAIN], ids=["weights", "act_train"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_inactive_path_is_identity_and_tracks_the_range(base, dtype, mode):
    for n, off, y_off in ((65, 1, 1), (4095, 3, 3), (4095, 1, 2)):
        x, dy = _case_input(base, n, dtype, 0)
        got = _pipeline(x, dy, DEV, off, y_off, mode, False, 8, 2, 3, hold=[])
        want = _pipeline(x, dy, torch.device("cpu"), 0, 0, mode, False, 8, 2, 3)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert got[4]["active"] == 0 and got[2:] == want[2:]
        assert torch.equal(got[0].view(bits), x.view(bits))
        assert torch.equal(got[1].view(bits), dy.view(bits))
        assert (got[2], got[3]) != (-0.75, 1.25)  # the range state moved all the same


@pytest.mark.parametrize("mode", [FQ.WEIGHTS, FQ.ACT_TRAIN], ids=["weights", "act_train"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_nonfinite_rule_on_the_device(base, dtype, mode):
    n, off = 4095, 1
    for where in (0, 2000):  # the scalar head; the middle of the 16-byte body
        vmin, vmax = _vars(DEV, -0.75, 1.25)
        counter = torch.tensor([5], dtype=torch.int64, device=DEV)
        st = FQ.QuantizerState(DEV)
        hold = []
        x, dy = _case_input(base, n, dtype, 7)
        FQ.finalize(_placed(hold, off, x), vmin, vmax, st, counter, mode, 0.999, 8, False, 3, True)
        before = (float(vmin), float(vmax))
        assert before != (-0.75, 1.25)
        for bad in (float("nan"), float("inf")):
            xb = x.clone()
            xb[where] = bad
            xd, y, dx = _placed(hold, off, xb), _placed(hold, off, torch.zeros_like(x)), \
                _placed(hold, off, torch.zeros_like(x))
            FQ.finalize(xd, vmin, vmax, st, counter, mode, 0.999, 8, False, 3, True)
            FQ.apply_into(xd, y, st.rec)
            FQ.apply_bwd_into(xd, _placed(hold, off, torch.ones_like(x)), dx, st.rec)
            assert (float(vmin), float(vmax)) == before
            y, dx = y.float().cpu(), dx.float().cpu()
            keep = torch.ones(n, dtype=torch.bool)
            keep[where] = False
            assert bool(torch.isfinite(y[keep]).all()) and float(dx[where]) == 0.0
            if bad != bad:
                assert math.isnan(float(y[where]))       # the optimizer's NaN guard still sees it
            else:
                assert float(y[where]) == float(y[keep].max())  # +Inf clamps to the upper end of the range
        assert st.record()["nonfinite_batches"] == 2


@pytest.mark.parametrize("narrow", [False, True], ids=["full", "narrow"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_apply_equals_aten_device_kernel_given_the_record(base, dtype, narrow):
    """With the scale and zero point of the record handed to ``torch.fake_quantize_per_tensor_affine`` on the device,
    values and straight-through gradients are equal element for element (the arithmetic is the same; what differs
    between the fused and the torch-op path on the GPU is how the scale is formed:
    test_fused_equals_unfused_on_the_gpu)."""
    pool, dyp = base
    n = dyp.numel()
    x = (pool[:n] * 1.5).to(DEV, dtype).requires_grad_()   # [-2.25, 3.75]: beyond the range on both sides
    dy = dyp.to(DEV, dtype)
    vmin, vmax = _vars(DEV, -1.5, 2.5)
    st = FQ.QuantizerState(DEV)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    FQ.finalize(x, vmin, vmax, st, counter, FQ.FROZEN, 0.999, 8, narrow, 0, False)
    ya = FQ.apply(x, st)
    (ga,) = torch.autograd.grad(ya, x, dy)
    f = st.rec.view(torch.float32)
    qmin, qmax = FQ.qrange(8, narrow)
    yb = torch.fake_quantize_per_tensor_affine(x.float(), f[0:1].clone(), f[2:3].to(torch.int32), qmin, qmax).to(dtype)
    (gb,) = torch.autograd.grad(yb, x, dy)
    assert torch.equal(ya, yb) and torch.equal(ga, gb)
    assert 0 < int((ga == 0).sum()) < x.numel()


def test_first_call_inside_a_capture_raises():
    cfg = Q.QuantConfig(fused=True)
    vmin = torch.nn.Parameter(torch.tensor(0.0, device=DEV), requires_grad=False)
    vmax = torch.nn.Parameter(torch.tensor(1.0, device=DEV), requires_grad=False)
    x = torch.randn(64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x.add_(1.0)  # (a non-empty capture)
        with pytest.raises(RuntimeError, match="inside a hipGraph capture"):
            FQ.quantize(x, vmin, vmax, cfg, FQ.ACT_TRAIN, False)
    assert cfg._counter is None and FQ.state_of(vmin, create=False) is None


def _reset_seeds():
    from distributed_tensorflow_models_amd.ops import elementwise as E
    torch.manual_seed(0)
    E.seed_offset(DEV).zero_()
    E.set_base_seed(1234)


def _train(use_graph, delay, steps=6):
    _reset_seeds()
    cfg = Q.QuantConfig(quant_delay=delay, fused=True)
    model = nets_factory.build("mobilenet_v1_025", num_classes=11, quantize=cfg, dropout_keep_prob=1.0).to(DEV)
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, use_graph=use_graph, wgrad_stream=False)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(4, 96, 96, 3, generator=g).to(DEV, torch.bfloat16) for _ in range(2)]
    ys = [torch.randint(0, 11, (4,), generator=g).to(DEV) for _ in range(2)]
    losses = [float(step(xs[i % 2], ys[i % 2])) for i in range(steps)]
    torch.cuda.synchronize()
    state = {n: v.detach().clone() for n, v in model.store.vars.items()}
    step.dp.close()
    return losses, state, cfg, step


def test_captured_step_crosses_the_delay_like_the_eager_one():
    """quant_delay = 4: TrainStep runs steps 0 and 1 eagerly, captures at step 2 (before the delay) and replays the
    graph at steps 3 (before), 4 and 5 (after): the replays must start quantising by themselves."""
    _lib.set_deterministic(True)
    side_was = _lib.side_enabled()
    try:
        la, sa, ca, st = _train(True, 4)
        lb, sb, cb, _ = _train(False, 4)
        lc, _, _, _ = _train(True, 10 ** 9)
    finally:
        _lib.set_deterministic(False)
        _lib.set_side_enabled(side_was)
    assert st._graph is not None and st.global_step == 6
    assert all(math.isfinite(v) for v in la)
    print("captured", la, "eager", lb, "never quantised", lc)
    assert ca.steps_done() == 6 and cb.steps_done() == 6 and cb.step == 6
    assert la == lb
    assert set(sa) == set(sb)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n
    assert sum("_quant/" in n for n in sa) == 4 * 28
    assert la[:4] == lc[:4] and la[5] != lc[5]  # the replay really switched the quantisers on


def _quant_state(model, layer):
    return {n: v.detach().clone() for n, v in model.store.vars.items() if layer in n and "_quant/" in n}


def test_fused_equals_unfused_on_the_gpu():
    """One training forward past the delay from identical state.

    The range state of the first layer is equal bit for bit: same conv, exact min / max, the moving average spelled
    operation by operation.

    The logits are not: ATen's device kernel for ``tensor / python_scalar`` multiplies by the scalar's reciprocal, so
    the unfused path's ``scale = (hi - lo) / 255`` is ``(hi - lo) * (1 / 255)`` on the GPU and a true division on
    the CPU and in the fused kernel (which follows the CPU arithmetic, tests/test_fakequant_cpu.py).  Measured on an
    MI355X over 200 random ranges: the scale differs by 1 ulp in 150 (full range) and 10 (narrow range), the zero
    point in none; with the scale and zero point given, 0 of 65536 elements differ between the fused apply kernel and
    ``torch.fake_quantize_per_tensor_affine``.  A 1-ulp scale moves a few values across a rounding tie by one
    quantisation step, and this random-initialised network (batch statistics over 4 x 3 x 3 positions in its last
    layers) amplifies that layer by layer: measured here, 0 elements differ after the first two layers, 25 of 147456
    after Conv2d_1_pointwise (by one bf16 ulp, 0.031), a third to a half of all elements from Conv2d_5_pointwise on,
    and the logits by up to 3.2 of a range of 6.05.  No bound tighter than the width of the last quantiser's range
    follows from the arithmetic, so that is what is asserted for them (the element-wise kernel itself is held to
    ATen's in test_apply_equals_aten_device_kernel_given_the_record), and the figures are printed."""
    x = torch.randn(4, 96, 96, 3, generator=torch.Generator().manual_seed(5)).to(DEV, torch.bfloat16)
    outs = []
    for fused in (True, False):
        _reset_seeds()
        cfg = Q.QuantConfig(quant_delay=1, fused=fused)
        model = nets_factory.build("mobilenet_v1_025", num_classes=11, quantize=cfg, dropout_keep_prob=1.0).to(DEV)
        with torch.no_grad():
            model(x, training=True)          # step 0, before the delay
            logits = model(x, training=True)  # step 1, quantised
        torch.cuda.synchronize()
        last = _quant_state(model, "Logits/")
        outs.append((_quant_state(model, "Conv2d_0/"), logits.float().cpu(),
                     [float(v) for n, v in sorted(last.items()) if "act_quant/" in n]))
    (sa, la, _), (sb, lb, (hi, lo)) = outs
    assert len(sa) == 4 and set(sa) == set(sb)
    for n in sa:
        print(n, float(sa[n]), float(sb[n]))
        assert torch.equal(sa[n], sb[n]), n
    err = (la - lb).abs().max().item()
    print("logits: max |fused - unfused| = %.3e, last activation range [%.4g, %.4g]" % (err, lo, hi))
    assert bool(torch.isfinite(la).all()) and bool(torch.isfinite(lb).all())
    step = (max(hi, 0.0) - min(lo, 0.0)) / 255.0
    assert lo < hi and err <= (max(hi, 0.0) - min(lo, 0.0)) + step
