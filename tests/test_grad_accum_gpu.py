"""Gradient accumulation on the GPU: the dtm_grad_accum kernel against the torch form of its three modes, and
TrainStep(accum_steps=N) on the device - ordered sum across split buckets, forced RCCL collectives, the captured
step, a windowed parameter, BN statistics, LARS."""
import copy

import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep, moving_average_buffers
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib, accum
from distributed_tensorflow_models_amd.utils.testing import run_workers

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64  # elements (256 bytes) on each side of both buffers
LENGTHS = [1, 3, 4, 255, 256, 1027, 8197, 1048579]
NAN_PAYLOAD = 0x7FC01234
# (acc, g) pairs planted in every case: g stays finite, so the flag must not move - not for an overflowing sum, and
# not for an Inf or NaN that sits in the accumulator
FINITE_G = [(1.0, -0.0), (-0.0, -0.0), (3e38, 3e38), (-3e38, -3e38), (3e38, -3e38), (float("inf"), 1.0),
            (float("nan"), 2.0)]
NONFINITE_G = [(float("inf"), float("-inf")), (1.0, float("inf")), (1.0, float("-inf")), (0.5, None)]  # None: the NaN


def _case(n, off_acc, off_g, planted, seed):
    """CPU buffers [guard | off | n | guard] for acc and g (guards hold 7.0) and the range's slices."""
    gen = torch.Generator().manual_seed(seed)
    acc = torch.full((GUARD + off_acc + n + GUARD,), 7.0)
    g = torch.full((GUARD + off_g + n + GUARD,), 7.0)
    sa, sg = slice(GUARD + off_acc, GUARD + off_acc + n), slice(GUARD + off_g, GUARD + off_g + n)
    acc[sa] = torch.randn(n, generator=gen)
    g[sg] = torch.randn(n, generator=gen)
    for k, (a, v) in enumerate(FINITE_G + (NONFINITE_G if planted else [])):  # (the last ones win where n is tiny)
        i = (k * 7919 + 3) % n
        acc[sa][i] = a
        if v is None:
            g[sg].view(torch.int32)[i] = NAN_PAYLOAD
        else:
            g[sg][i] = v
    assert bool(torch.isfinite(g[sg]).all()) != planted
    return acc, g, sa, sg


def _same(got, want, bitwise):
    got, want = got.cpu(), want.cpu()
    if bitwise:
        return torch.equal(got.view(torch.int32), want.view(torch.int32))
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


def _run_case(n, off_acc, off_g, planted, mode, with_flag=True):
    acc, g, sa, sg = _case(n, off_acc, off_g, planted, seed=n + 17 * mode)
    flag = torch.tensor([7, 0, 7], dtype=torch.int32)
    acc_d, g_d, flag_d = acc.to(DEV), g.to(DEV), flag.to(DEV)
    assert acc_d.data_ptr() % 16 == 0 and g_d.data_ptr() % 16 == 0
    accum.grad_accum(acc_d[sa], g_d[sg], mode, flag_d[1:2] if with_flag else None)
    accum.grad_accum(acc[sa], g[sg], mode, flag[1:2] if with_flag else None)  # the torch form, same tensors
    torch.cuda.synchronize()
    what = "n %d offsets %d/%d mode %d planted %s" % (n, off_acc, off_g, mode, planted)
    # whole buffers: the range and the 64 guard elements on each side of both
    assert _same(acc_d, acc, bitwise=mode == accum.STORE), what
    assert _same(g_d, g, bitwise=False), what
    assert flag_d.tolist() == [7, int(planted and with_flag), 7], what
    if mode != accum.FOLD:
        assert not g_d[sg].any()
    assert bool((acc_d[:sa.start] == 7.0).all()) and bool((acc_d[sa.stop:] == 7.0).all()), what
    assert bool((g_d[:sg.start] == 7.0).all()) and bool((g_d[sg.stop:] == 7.0).all()), what


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("mode", [accum.STORE, accum.ADD, accum.FOLD], ids=["store", "add", "fold"])
def test_kernel_matches_torch(mode, n):
    for off in range(4):  # elements past a 16-byte boundary, acc and g alike: the 16-byte path with head and tail
        for planted in (False, True):
            _run_case(n, off, off, planted, mode)


@pytest.mark.parametrize("mode", [accum.STORE, accum.ADD, accum.FOLD], ids=["store", "add", "fold"])
def test_kernel_offsets_that_differ_and_null_flag(mode):
    for planted in (False, True):
        _run_case(8197, 1, 3, planted, mode)  # acc and g never reach a boundary together: the 4-byte path
        _run_case(1027, 2, 2, planted, mode, with_flag=False)
        _run_case(1027, 0, 3, planted, mode, with_flag=False)
    z = torch.zeros(8, device=DEV)
    accum.grad_accum(z[:0], z[:0], mode, None)  # an empty range is no launch
    z2 = z.clone()
    assert _lib.lib().dtm_grad_accum(_lib.ptr(z), _lib.ptr(z2), 8, 3, None, _lib.stream_ptr()) == -1  # no mode 3
    assert _lib.lib().dtm_grad_accum(_lib.ptr(z), None, 8, mode, None, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert not z.any() and not z2.any()


# ---- the step ---------------------------------------------------------------------------------------------------
MB = 8


@pytest.fixture()
def deterministic():
    """Fixed-order reductions, weight gradients on the main stream (the side stream sizes its split-K otherwise)."""
    side_was = _lib.side_enabled()
    _lib.set_deterministic(True)
    _lib.set_side_enabled(False)
    try:
        yield
    finally:
        _lib.set_deterministic(False)
        _lib.set_side_enabled(side_was)


def lenet(keep=1.0):
    torch.manual_seed(0)
    return nets_factory.build("lenet", 10, dropout_keep_prob=keep).to(DEV)


def rows(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 28, 28, 1, generator=g).to(DEV, torch.bfloat16),
            torch.randint(0, 10, (n,), generator=g).to(DEV))


def params_of(model):
    return [p.detach().clone() for p in model.parameters()]


def ordered_sum(gs):
    s = gs[0].clone()
    for g in gs[1:]:
        s = s + g
    return s


def twin_gradients_and_update(build, xs, ys, **kw):
    """From a twin model and a TrainStep without accumulation: the flat gradient of every micro-batch (separate
    zero-grad / forward / loss / backward passes on the initial weights), their ordered sum, and the parameters
    after the twin's own optimizer launch on that sum with grad_scale 1 / n."""
    twin = build()
    st = TrainStep(twin, **kw)
    gs = []
    for x, y in zip(xs, ys):
        st._forward_backward(x, y)
        gs.append(st.dp.flat.clone())
    st.dp.close()
    want = ordered_sum(gs)
    st.dp.flat.copy_(want)
    st.opt.step(kw["lr"], grad_scale=1.0 / len(xs))
    torch.cuda.synchronize()
    return gs, want, params_of(twin)


def test_step_ordered_sum_across_split_buckets(deterministic):
    n = 4
    x, y = rows(n * MB)
    xs, ys = list(x.split(MB)), list(y.split(MB))
    kw = dict(optimizer="momentum", lr=0.05, momentum=0.9, bucket_mb=4.0, weight_decay=0.0)
    gs, want, want_params = twin_gradients_and_update(lenet, xs, ys, **kw)
    assert not torch.equal(gs[0], gs[1])
    model = lenet()
    step = TrainStep(model, accum_steps=n, **kw)
    dp = step.dp
    assert len(dp.buckets) >= 3 and any(len(c) >= 2 for c in dp.contrib.values())  # a tensor split across buckets
    # the 10-element bias comes first in backward order: every later offset is off the 16-byte grid
    assert dp.order[0].numel() == 10 and sum(dp.offsets[p] % 4 != 0 for p in dp.order) >= 6
    step(xs, ys)
    torch.cuda.synchronize()
    assert torch.equal(dp.flat, want)
    assert dp.grad_scale == 0.25 and step.nonfinite_micro() == [0] * n
    assert all(torch.equal(a, p.detach()) for a, p in zip(want_params, model.parameters()))
    dp.close()


def test_captured_step_matches_eager(deterministic):
    n = 3
    x, y = rows(2 * n * MB, seed=9)
    batches = [(x[:n * MB], y[:n * MB]), (x[n * MB:], y[n * MB:])]
    bad = batches[1][0].clone()
    bad[MB + 1, 3, 3, 0] = float("nan")  # step 3 (the replay): a NaN row in micro-batch 1
    runs = []
    for graph in (False, True):
        model = lenet()
        step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, ema_decay=0.99, accum_steps=n,
                         use_graph=graph)
        losses, flags = [], []
        for i in range(4):
            xb, yb = batches[i % 2]
            losses.append(float(step(bad if i == 3 else xb, yb)))
            flags.append(step.nonfinite_micro())
        torch.cuda.synchronize()
        assert (step._graph is not None) == graph and step.global_step == 4 and step.opt.num_updates == 4
        assert step.poll_skipped() and step.skipped == 1
        runs.append((losses, flags, params_of(model)))
        step.dp.close()
    (le, fe, pe), (lg, fg, pg_) = runs
    assert fe == fg == [[0, 0, 0]] * 3 + [[0, 1, 0]]
    assert all(a == b or (a != a and b != b) for a, b in zip(le, lg)), (le, lg)
    assert all(torch.equal(a, b) for a, b in zip(pe, pg_))


def test_bn_statistics_take_one_update_per_micro_batch():
    """Tolerance: the one tests/test_distributed.py holds the synced statistics to (fp32 statistics whose sums may
    be taken in another order); one update more or less moves them by (1 - decay) of their distance to the batch's."""
    n = 3
    torch.manual_seed(0)
    model = nets_factory.build("resnet_v1_50", num_classes=16).to(DEV)
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, accum_steps=n)
    g = torch.Generator().manual_seed(100)
    xs = [(torch.randn(4, 64, 64, 3, generator=g) * (1 + i)).to(DEV, torch.bfloat16) for i in range(n)]
    ys = [torch.randint(0, 16, (4,), generator=g).to(DEV) for _ in range(n)]
    cat = lambda m: torch.cat([b.reshape(-1) for b in moving_average_buffers(m)]).clone()  # noqa: E731
    init = cat(model)
    shadow = copy.deepcopy(model)
    after = []
    with torch.no_grad():
        for x in xs:  # three sequential training forwards (the weights do not move inside a step)
            shadow(x, training=True)
            after.append(cat(shadow))
    step(xs, ys)
    torch.cuda.synchronize()
    got = cat(model)
    assert init.numel() > 0
    torch.testing.assert_close(got, after[2], rtol=1e-5, atol=1e-6)
    for other in (init, after[0], after[1]):  # fewer updates would have been seen
        assert float((got - other).abs().max()) > 1e-3
    step.dp.close()


def test_lars_reads_the_folded_buffer(deterministic):
    x, y = rows(2 * MB)
    model = lenet()
    step = TrainStep(model, optimizer="lars", lr=0.05, momentum=0.9, weight_decay=0.0, accum_steps=2)
    step(x, y)
    torch.cuda.synchronize()
    dp = step.dp
    assert dp.grad_scale == 0.5
    gs = dp.flat * dp.grad_scale  # fp32 terms as the kernel forms them, fp64 sums
    want = float(gs.double().square().sum().sqrt())
    got = step.opt.norm_stats()["grad_norm"]
    print("grad_norm: norm pass %.9g, torch %.9g" % (got, want))
    assert want > 0.0
    torch.testing.assert_close(torch.tensor(got, dtype=torch.float64), torch.tensor(want, dtype=torch.float64),
                               rtol=1e-5, atol=0.0)
    per = torch.stack([gs[dp.offsets[p]:dp.offsets[p] + p.numel()].double().square().sum().sqrt()
                       for p in step.opt.params]).cpu()
    torch.testing.assert_close(step.opt.last_norms()[:len(per), 1].cpu().double(), per, rtol=1e-5, atol=0.0)
    dp.close()


# ---- forced collectives (RCCL at world 1): one spawned rank runs both comparisons -----------------------------------
class _DeadTapNet(torch.nn.Module):
    """A 7x7 'SAME' conv over a 3x3 map (only its inner 5x5 taps ever read data: a windowed parameter with a
    compact bucket), between a conv stem and a 1x1 classifier."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.w1 = torch.nn.Parameter(torch.randn(8, 3, 3, 8, generator=g) * 0.2)
        self.w6 = torch.nn.Parameter(torch.randn(16, 7, 7, 8, generator=g) * 0.05)
        self.w8 = torch.nn.Parameter(torch.randn(16, 1, 1, 16, generator=g) * 0.1)

    def forward(self, x, training=True):
        from distributed_tensorflow_models_amd.ops import nn as F
        h = F.conv2d(x, self.w1, None, 2, "SAME", relu=True)
        h = F.conv2d(h, self.w6, None, 1, "SAME", relu=True)
        h = F.max_pool(h, h.shape[1], h.shape[1], "VALID")
        h = F.conv2d(h, self.w8, None, 1, "SAME")
        return h.reshape(h.shape[0], -1)


def _rccl_accum_worker(rank, world):
    import torch.distributed as dist
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    _lib.set_deterministic(True)
    _lib.set_side_enabled(False)
    out = {}
    # (a) LeNet, 3 micro-batches, two steps: with and without the collectives
    x, y = rows(3 * MB)
    for forced in (False, True):
        model = lenet()
        step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, bucket_mb=4.0, accum_steps=3,
                         force_comm=forced)
        losses = [float(step(x, y)) for _ in range(2)]
        torch.cuda.synchronize()
        out["lenet_%d" % forced] = {"params": torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(),
                                    "flat": step.dp.flat.cpu(), "losses": losses,
                                    "works": len(step.dp._done_works), "buckets": len(step.dp.buckets)}
        step.dp.close()
    # (b) a windowed parameter, 2 micro-batches, collectives on
    g = torch.Generator().manual_seed(7)
    xs = [torch.randn(8, 6, 6, 8, generator=g).to(DEV, torch.bfloat16) for _ in range(2)]
    ys = [torch.randint(0, 16, (8,), generator=g).to(DEV) for _ in range(2)]

    def build():
        return _DeadTapNet().to(DEV)
    kw = dict(optimizer="momentum", lr=0.05, momentum=0.9, bucket_mb=0.01, force_comm=True)
    gs, want, want_params = twin_gradients_and_update(build, xs, ys, **kw)
    model = build()
    step = TrainStep(model, accum_steps=2, **kw)
    step(xs, ys)
    torch.cuda.synchronize()
    dp = step.dp
    w6 = dp.offsets[model.w6]
    out["window"] = {"compact": len(dp.compact), "works": len(dp._done_works), "buckets": len(dp.buckets),
                     "flat": dp.flat.cpu(), "want": want.cpu(), "differ": not torch.equal(gs[0], gs[1]),
                     "w6_grad": dp.flat[w6:w6 + model.w6.numel()].view(model.w6.shape).cpu(),
                     "params": [p.detach().cpu() for p in model.parameters()],
                     "want_params": [p.cpu() for p in want_params]}
    dp.close()
    return out


@pytest.fixture(scope="module")
def rccl():
    return run_workers(_rccl_accum_worker, 1, backend="nccl")[0]


def test_forced_collectives_change_nothing(rccl):
    off, on = rccl["lenet_0"], rccl["lenet_1"]
    assert off["works"] == 0 and on["works"] == on["buckets"] >= 3  # as many collectives as a step of one batch
    assert on["losses"] == off["losses"]
    assert torch.equal(on["flat"], off["flat"]) and torch.equal(on["params"], off["params"])
    assert bool(torch.isfinite(on["params"]).all()) and float(on["flat"].abs().max()) > 0.0


def test_windowed_parameter_is_folded_before_its_gather(rccl):
    r = rccl["window"]
    assert r["compact"] == 1 and r["works"] == r["buckets"] and r["differ"]
    assert torch.equal(r["flat"], r["want"])
    g = r["w6_grad"]
    dead = g.clone()
    dead[:, 1:6, 1:6] = 0.0
    assert float(g[:, 1:6, 1:6].abs().sum()) > 0.0 and not dead.any()  # only the live 5x5 window holds a gradient
    assert all(torch.equal(a, b) for a, b in zip(r["params"], r["want_params"]))
