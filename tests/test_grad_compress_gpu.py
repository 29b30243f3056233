"""Top-k gradient sparsification with error feedback on the GPU (csrc/kernels/grad_compress.hip): every function case
of compress_cases.py bit for bit against the CPU path (idx, val bits, res bits, decompressed g bits), and the
training step with compression against the same step with the CPU forms in the kernels' place."""
import ctypes

import numpy as np
import pytest
import torch

import compress_cases as cc
from test_grad_compress_cpu import _bits, run_case
from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops import compress as C
from distributed_tensorflow_models_amd.utils.testing import run_workers

pytestmark = pytest.mark.gpu

_CPU = {}


def _cpu(case):
    """The CPU path's result of a case, computed once."""
    if case.name not in _CPU:
        _CPU[case.name] = run_case(case)
    return _CPU[case.name]


def test_library_constants_match_the_binding():
    L = _lib.lib()
    assert L.dtm_gc_chunk_size() == cc.CHUNK == C.CHUNK
    for n in (1, 5, cc.CHUNK, cc.CHUNK + 3, 1 << 23, (1 << 31) - 1):
        assert L.dtm_gc_scratch_words(n) == C.scratch_words(n)
    assert L.dtm_gc_scratch_words(0) == -2 and L.dtm_gc_scratch_words(1 << 31) == -2


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_kernels_match_the_cpu_path_bit_for_bit(case):
    got = run_case(case, device="cuda")
    for name, a, b in zip(("idx", "val", "res", "g"), got, _cpu(case)):
        assert np.array_equal(a, b), "%s differs at %s" % (name, np.flatnonzero(a != b)[:8])


def test_compress_is_bit_identical_run_to_run_on_several_rows():
    case = [c for c in cc.CASES if c.name == "normal-n%d-off1" % (3 * cc.CHUNK + 5)][0]
    a, b = run_case(case, device="cuda"), run_case(case, device="cuda")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_exact_error_feedback_on_the_device():
    n, T = cc.CHUNK + 3, 6
    k = C.bucket_k(n, 0.1)
    g0 = torch.from_numpy(np.random.default_rng(5).integers(-8, 9, n).astype(np.float32)).cuda()
    res, total = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    packet = torch.zeros(2 * k, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(C.scratch_words(n), dtype=torch.int32, device="cuda")
    for _ in range(T):
        g = g0.clone()
        C.compress_bucket(res, g, k, packet, scratch)
        C.decompress_bucket(g, packet.view(1, -1), k)
        total += g
    assert torch.equal(total + res, T * g0)
    assert float(res.abs().max()) > 0


def test_decompress_adds_the_packets_in_rank_order():
    k, n = cc.ORDER_K, cc.ORDER_N
    packets = torch.tensor(np.stack([np.concatenate([i, v.view(np.int32)]) for i, v in cc.ORDER_PACKETS])).cuda()
    g = torch.full((n,), 7.0, device="cuda")
    C.decompress_bucket(g, packets, k)
    assert np.array_equal(_bits(g), cc.oracle_decompress(n, cc.ORDER_PACKETS))
    assert float(g[3]) == 0.0


def test_entry_points_return_their_codes_and_launch_nothing():
    L = _lib.lib()
    n = 64
    res, g = torch.ones(n, device="cuda"), torch.full((n,), 2.0, device="cuda")
    packet = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
    scratch = torch.full((C.scratch_words(n),), -1, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()
    P = _lib.ptr
    for nn, kk, code in ((0, 1, -2), (-1, 1, -2), (1 << 31, 1, -2), (n, 0, -3), (n, n + 1, -3), (n, -5, -3)):
        assert L.dtm_grad_compress(P(res), P(g), nn, kk, P(packet), P(scratch), st) == code
        assert L.dtm_grad_decompress(P(g), nn, P(packet), 1, kk, st) == code
    assert L.dtm_grad_compress(None, P(g), n, 1, P(packet), P(scratch), st) == -1
    assert L.dtm_grad_compress(P(res), P(g), n, 1, None, P(scratch), st) == -1
    assert L.dtm_grad_compress(ctypes.c_void_p(res.data_ptr() + 2), P(g), n - 1, 1, P(packet), P(scratch), st) == -1
    assert L.dtm_grad_decompress(P(g), n, P(packet), 0, 1, st) == -1
    assert L.dtm_grad_decompress(P(g), n, None, 1, 1, st) == -1
    torch.cuda.synchronize()
    assert bool((res == 1).all()) and bool((g == 2).all()) and bool((packet == -1).all())
    assert bool((scratch == -1).all())
    with pytest.raises(ValueError):
        C.compress_bucket(res, g, 0, packet, scratch)
    with pytest.raises(ValueError):
        C.compress_bucket(res, g, 4, packet[:8], scratch[:16])  # scratch too small


# ---- step level -----------------------------------------------------------------------------------------------------
def _resnet_step(cfg, **kw):
    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = nets_factory.build("resnet_v1_50", num_classes=16).to(dev)
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, bucket_mb=4.0, grad_compress=cfg, **kw)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4, 64, 64, 3, generator=g).to(dev, torch.bfloat16)
    y = torch.randint(0, 16, (4,), generator=g).to(dev)
    return model, step, x, y


def _flat_params(model):
    return torch.cat([p.detach().float().reshape(-1) for p in model.parameters()]).cpu()


def _bsp_gpu_worker(rank, world, steps=2):
    """tests/test_distributed.py's two-gloo-ranks-on-one-GPU worker with rho = 0.01; a hook keeps a host copy of every
    plain bucket's residual and gradient right before it is compressed, and the packet must be the CPU function of
    them."""
    model, step, x, y = _resnet_step(C.GradCompress(0.01))
    dp = step.dp
    seen = {}
    dp.compress_hook = lambda bi, s, e: seen.__setitem__(bi, (dp.res[s:e].cpu(), dp.flat[s:e].cpu()))
    checked, bad = 0, []
    losses = []
    for t in range(steps):
        seen.clear()
        losses.append(float(step(x, y)))
        torch.cuda.synchronize()
        for bi, (r, g) in seen.items():
            k = dp._cbufs[bi][0]
            want = torch.zeros(2 * k, dtype=torch.int32)
            C.compress_cpu(r, g, k, want)
            checked += 1
            s, e = dp.buckets[bi]
            if not torch.equal(dp.packets[bi].cpu(), want) or not torch.equal(dp.res[s:e].cpu(), r):
                bad.append((t, bi))
    out = {"params": _flat_params(model), "losses": losses, "buckets": len(dp.buckets), "checked": checked, "bad": bad,
           "plain": sum(1 for bi in range(len(dp.buckets)) if bi not in dp.compact), "res": dp.residual_norm(),
           "wire": dp.wire_elements(), "total": dp.flat.numel()}
    dp.close()
    return out


def test_two_gloo_ranks_on_one_gpu_stay_identical_and_send_the_cpu_functions_packets():
    two = run_workers(_bsp_gpu_worker, 2)  # (two processes with the GPU open, and this one)
    assert two[0]["buckets"] > 4
    assert torch.equal(two[0]["params"], two[1]["params"])
    for r in two:
        assert r["bad"] == [] and r["checked"] == 2 * r["plain"] and r["plain"] == r["buckets"]
        assert r["res"] > 0 and all(np.isfinite(r["losses"]))
        assert r["wire"] <= 0.0201 * r["total"] + 2 * r["buckets"]


def test_world_1_step_matches_the_cpu_forms_bit_for_bit():
    """Three steps of ResNet-50 with compression at world 1 (the local path: select, residual, zero and scatter) against
    the same three steps with compress_bucket / decompress_bucket running their CPU forms on host copies.  Fixed-order
    reductions make the rest of the step bit-reproducible."""
    was = _lib.lib().dtm_get_deterministic()
    _lib.set_deterministic(True)
    try:
        out = []
        for force in (False, True):
            C.FORCE_CPU = force
            model, step, x, y = _resnet_step(C.GradCompress(0.01))
            losses = [float(step(x, y)) for _ in range(3)]
            torch.cuda.synchronize()
            out.append((_flat_params(model), step.dp.res.cpu(), step.dp.flat.cpu(), losses))
            assert len(step.dp.packets) == len(step.dp.buckets) > 4
            step.dp.close()
    finally:
        C.FORCE_CPU = False
        _lib.set_deterministic(was)
    (pa, ra, fa, la), (pb, rb, fb, lb) = out
    assert la == lb and all(np.isfinite(la))
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and bool(ra.any())
    assert torch.equal(fa.view(torch.int32), fb.view(torch.int32))
    assert torch.equal(pa, pb)
