"""StreamingMetrics on the GPU (csrc/kernels/metrics.hip) against the numpy oracle and the CPU path."""
import math

import numpy as np
import pytest
import torch

import eval_metrics_cases as cases
from distributed_tensorflow_models_amd.ops import elementwise as E
from distributed_tensorflow_models_amd.ops.metrics import StreamingMetrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def _dev_pool(C, dtype, rows):
    """The pool on the device, again as a view one element into its allocation."""
    x, t, n_adv = cases.pool(C, dtype, rows)
    flat = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
    flat[1:] = x.reshape(-1).to(DEV)
    xd = flat[1:].view(x.shape)
    assert xd.data_ptr() % 16 != 0
    return xd, t.to(DEV), n_adv


def _run(x, t, k, batch, confusion=True):
    """Rows in batches of ``batch`` (the last one wraps round to the first rows, so every update has B = batch
    exactly); returns (fetched record, rows fed)."""
    m = StreamingMetrics(x.shape[1], k=k, confusion=confusion, device=DEV)
    P = x.shape[0]
    idx = torch.arange(-(-P // batch) * batch) % P
    for s in range(0, idx.numel(), batch):
        a, b = int(idx[s]), int(idx[s + batch - 1])
        if b - a == batch - 1:  # a contiguous slice of the view: read in place
            m.update(x[a:b + 1], t[a:b + 1])
        else:
            sl = idx[s:s + batch].to(x.device)
            m.update(x[sl], t[sl])
    return m.fetch(), idx


@DTYPES
@pytest.mark.parametrize("C", [1, 2, 10, 63, 64, 65, 1001])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 257])
def test_gpu_matches_oracle_and_cpu_path(B, C, dtype):
    """Every batch has exactly B rows; the pool (adversarial rows first) is fed whole, so B = 1 sees every
    adversarial row alone and B = 257 all of them in one launch."""
    rows = B if B > 32 else 0  # (0: the adversarial rows and MIN_RANDOM random ones - one pool for every short B)
    x, t, n_adv = _dev_pool(C, dtype, rows)
    xc, tc, _ = cases.pool(C, dtype, rows)
    P = x.shape[0]
    for k in cases.ks(C):
        got, idx = _run(x, t, k, B)
        if idx.numel() == P:
            ref, xr, tr = cases.oracle(C, dtype, rows, k), xc, tc
        else:  # the wrapped rows count twice
            from distributed_tensorflow_models_amd.ops import reference
            xr, tr = xc[idx], tc[idx]
            ref = reference.eval_metrics(xr.double(), tr, k)
        cases.check(got, ref, xr, tr)
        cpu = StreamingMetrics(C, k=k, confusion=True)
        cpu.update(xr, tr)
        cpu = cpu.fetch()
        for n in cases.INT_KEYS:
            assert got[n] == cpu[n], n
        for n in cases.ARRAY_KEYS + ("confusion",):
            assert np.array_equal(got[n], cpu[n]), n
    # the random rows alone, int32 labels: the loss against a bound that the 3e38 rows do not swamp
    m = StreamingMetrics(C, k=1, device=DEV)
    m.update(x[n_adv:], t[n_adv:].int())
    cases.check(m.fetch(), cases.oracle(C, dtype, rows, 1, n_adv), xc[n_adv:], tc[n_adv:], confusion=False)


@DTYPES
def test_updates_accumulate_reset_and_repeat_bit_identically(dtype):
    C, rows = 65, 300
    x, t, _ = _dev_pool(C, dtype, rows)
    cuts = [(0, 5), (5, 262), (262, x.shape[0])]  # three different B

    def parts():
        out = []
        for a, b in cuts:
            m = StreamingMetrics(C, k=5, confusion=True, device=DEV)
            m.update(x[a:b], t[a:b])
            out.append(m.fetch())
        return out

    def whole():
        m = StreamingMetrics(C, k=5, confusion=True, device=DEV)
        for a, b in cuts:
            m.update(x[a:b], t[a:b])
        return m, m._rec.cpu().numpy().tobytes()

    m, bits = whole()
    got, ps = m.fetch(), parts()
    for n in cases.INT_KEYS:
        assert got[n] == sum(p[n] for p in ps), n
    for n in cases.ARRAY_KEYS + ("confusion",):
        assert np.array_equal(got[n], sum(p[n] for p in ps)), n
    assert got["loss_sum"] == (ps[0]["loss_sum"] + ps[1]["loss_sum"]) + ps[2]["loss_sum"]
    assert whole()[1] == bits  # a fresh run: the same bits, loss_sum included
    m.reset()
    assert not m._rec.cpu().numpy().any()
    for a, b in cuts:
        m.update(x[a:b], t[a:b])
    assert m._rec.cpu().numpy().tobytes() == bits


def test_fetch_without_updates():
    m = StreamingMetrics(10, k=5, confusion=True, device=DEV)
    m.update(torch.zeros(0, 10, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    z = m.fetch()
    torch.cuda.synchronize()
    assert all(z[n] == 0 for n in cases.INT_KEYS) and z["loss_sum"] == 0.0 and math.isnan(z["mean_loss"])
    assert not z["support"].any() and not z["confusion"].any()


@DTYPES
@pytest.mark.parametrize("C", [2, 65, 1001])
def test_top1_topk_equal_in_top_k_kernel(C, dtype):
    x, t, _ = _dev_pool(C, dtype, 64)
    for k in cases.ks(C):
        m = StreamingMetrics(C, k=k, device=DEV)
        m.update(x, t)
        got = m.fetch()
        assert got["top1"] == int(E.in_top_k(x, t, 1).sum())
        assert got["topk"] == int(E.in_top_k(x, t, k).sum())


def test_limits():
    L = __import__("distributed_tensorflow_models_amd.ops._lib", fromlist=["lib"])
    x = torch.zeros(4, 8, device=DEV)
    t = torch.zeros(4, dtype=torch.int32, device=DEV)
    rec = torch.zeros(8 + 24, dtype=torch.int64, device=DEV)
    rl = torch.zeros(4, dtype=torch.float64, device=DEV)
    fl = torch.zeros(4, dtype=torch.int32, device=DEV)

    def call(B, C, k, conf=0):
        return L.lib().dtm_eval_metrics(L.ptr(x), 0, L.ptr(t), 0, B, C, k, conf, L.ptr(rec), L.ptr(rl), L.ptr(fl),
                                        L.stream_ptr())

    assert call(4, 8, 5) == 0
    for bad in ((65537, 8, 5), (4, 65537, 5), (4, 8, 0), (4, 8, 9), (4, 0, 1), (-1, 8, 5)):
        assert call(*bad) != 0, bad
    assert call(4, 4097, 5, 1) != 0
    torch.cuda.synchronize()
    assert int(rec[0]) == 4  # only the valid call reached the record


def test_eval_once_matches_the_old_counting():
    from distributed_tensorflow_models_amd import evaluator
    from distributed_tensorflow_models_amd.data.synthetic import SyntheticImages
    from distributed_tensorflow_models_amd.models import nets_factory
    torch.manual_seed(5)
    model = nets_factory.build("lenet", num_classes=10).to(DEV)
    model.eval()
    data = SyntheticImages(16, 28, 28, 1, 10, DEV, seed=1234, shuffle_labels=True)
    torch.manual_seed(11)
    c1 = c5 = 0
    with torch.no_grad():
        for _ in range(3):
            xb, yb = data.next_batch()
            out = model(xb, training=False)
            c1 += int(E.in_top_k(out, yb, 1).sum())
            c5 += int(E.in_top_k(out, yb, 5).sum())
    data = SyntheticImages(16, 28, 28, 1, 10, DEV, seed=1234, shuffle_labels=True)
    torch.manual_seed(11)
    m = StreamingMetrics(10, k=5, confusion=True, device=DEV)
    assert evaluator.eval_once(model, data, 40, 16, metrics=m) == (c1 / 48, c5 / 48)
    got = m.fetch()
    assert got["examples"] == 48 and got["top1"] == c1 and got["confusion"].sum() == got["loss_rows"] == 48
    data = SyntheticImages(16, 28, 28, 1, 10, DEV, seed=1234, shuffle_labels=True)
    torch.manual_seed(11)
    assert evaluator.eval_once(model, data, 40, 16) == (c1 / 48, c5 / 48)
