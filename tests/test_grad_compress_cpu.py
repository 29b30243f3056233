"""Top-k gradient sparsification with error feedback: the CPU path (torch / numpy; the gloo path and the kernels'
oracle) against the numpy oracle of the definition in compress_cases.py, and the step-level behaviour of
BSPDataParallel(compress=...) / TrainStep(grad_compress=...) / the trainer's flags on CPU tensors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import compress_cases as cc
from distributed_tensorflow_models_amd.ops import compress as C
from distributed_tensorflow_models_amd.utils.testing import run_workers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."


def _t(bits):
    return torch.from_numpy(np.asarray(bits, np.uint32).view(np.float32).copy())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def run_case(case, device="cpu"):
    """(idx, val, res, g after decompress of the one packet) as numpy bit patterns, through the public functions."""
    n = case.res.size
    rbuf = torch.zeros(n + 8, device=device)
    gbuf = torch.zeros(n + 8, device=device)
    res, g = rbuf[case.off_res:case.off_res + n], gbuf[case.off_g:case.off_g + n]
    res.copy_(_t(case.res))
    g.copy_(_t(case.g))
    packet = torch.full((2 * case.k,), -1, dtype=torch.int32, device=device)
    scratch = torch.zeros(C.scratch_words(n), dtype=torch.int32, device=device) if device != "cpu" else None
    C.compress_bucket(res, g, case.k, packet, scratch)
    assert np.array_equal(_bits(g), case.g)  # g is only read
    C.decompress_bucket(g, packet.view(1, -1), case.k)
    # nothing outside the two ranges was written
    for buf, off in ((rbuf, case.off_res), (gbuf, case.off_g)):
        assert not _bits(buf[:off]).any() and not _bits(buf[off + n:]).any()
    p = packet.cpu().numpy()
    return p[:case.k].copy(), p[case.k:].view(np.uint32).copy(), _bits(res).copy(), _bits(g).copy()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_cpu_path_matches_the_oracle(case):
    idx, val, res, g = run_case(case)
    o_idx, o_val, o_res, u = cc.oracle(case.res, case.g, case.k)
    assert np.array_equal(idx, o_idx) and np.array_equal(val, o_val) and np.array_equal(res, o_res)
    assert np.array_equal(g, cc.oracle_decompress(u.size, [(o_idx, o_val)]))
    assert len(set(idx.tolist())) == case.k and (np.diff(idx) > 0).all()
    finite = (u & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    assert (cc.b2f(res)[~finite] == 0).all() and np.isfinite(cc.b2f(res)).all()
    if finite.all():
        # conservation: the scattered packet and the new residual partition u bit for bit (the decompressed buffer
        # is +0 + val, which differs from val in the sign of a sent -0 alone)
        sent = np.zeros(u.size, bool)
        sent[idx] = True
        scattered = np.zeros(u.size, np.uint32)
        scattered[idx] = val
        assert np.array_equal(scattered[sent], u[sent]) and not res[sent].any()
        assert np.array_equal(res[~sent], u[~sent]) and not g[~sent].any()
        assert np.array_equal(cc.b2f(g), cc.b2f(scattered))  # (value equality)
    else:
        assert not np.isfinite(cc.b2f(g)).all()  # sent first: the reduced buffer is non-finite, the guard skips
        bad = np.flatnonzero(~finite)  # (one key per case: the first k of them in index order)
        assert set(bad[:case.k].tolist()) <= set(idx.tolist())


def test_oracle_order_is_key_descending_then_index():
    """The lexsort of the oracle against a plain sort of (-(key), index) tuples, on the tie-heavy cases."""
    for case in cc.CASES:
        if not case.name.startswith(("ties-", "mostly", "signed", "digit")):
            continue
        o_idx, _val, _res, u = cc.oracle(case.res, case.g, case.k)
        key = (u & cc.KEY).tolist()
        want = sorted(sorted(range(len(key)), key=lambda i: (-key[i], i))[:case.k])
        assert o_idx.tolist() == want, case.name


def test_named_tie_cases_select_what_the_definition_says():
    by = {c.name: c for c in cc.CASES}
    idx = run_case(by["ties-all-equal"])[0]
    assert idx.tolist() == list(range(100))
    idx = run_case(by["ties-wave-boundary"])[0]
    assert [i for i in idx.tolist() if 250 <= i < 262] == list(range(250, 258))  # need = 8 cuts inside the run
    idx = run_case(by["ties-row-boundary"])[0]
    assert [i for i in idx.tolist() if 8186 <= i < 8200] == list(range(8186, 8195))  # over the row boundary
    c = by["mostly-zeros"]
    idx, val, _res, _g = run_case(c)
    nz = np.flatnonzero(cc.b2f(c.g))
    zeros = [i for i in range(c.g.size) if cc.b2f(c.g)[i] == 0][:c.k - nz.size]
    assert sorted(idx.tolist()) == sorted(nz.tolist() + zeros)
    c = by["kn"]
    idx, val, res, _g = run_case(c)
    assert not res.any() and idx.tolist() == list(range(c.k))
    assert np.array_equal(val, cc.oracle(c.res, c.g, c.k)[3])  # the packet is u itself


def test_exact_error_feedback():
    """g integer-valued in [-8, 8] and constant over T = 6 steps at W = 1, rho = 0.1: every sum is exact in fp32, so
    the decompressed outputs plus the final residual add up to T * g exactly - nothing is lost or counted twice."""
    n, T = cc.CHUNK + 3, 6
    k = C.bucket_k(n, 0.1)
    g0 = torch.from_numpy(np.random.default_rng(5).integers(-8, 9, n).astype(np.float32))
    res, total = torch.zeros(n), torch.zeros(n)
    packet = torch.zeros(2 * k, dtype=torch.int32)
    for _ in range(T):
        g = g0.clone()
        C.compress_bucket(res, g, k, packet)
        C.decompress_bucket(g, packet.view(1, -1), k)
        total += g
    assert torch.equal(total + res, T * g0)
    assert float(res.abs().max()) > 0  # the residual really carried something


def test_decompress_adds_the_packets_in_rank_order():
    k, n = cc.ORDER_K, cc.ORDER_N
    packets = torch.tensor(np.stack([np.concatenate([i, v.view(np.int32)]) for i, v in cc.ORDER_PACKETS]))
    g = torch.full((n,), 7.0)
    C.decompress_bucket(g, packets, k)
    want = cc.oracle_decompress(n, cc.ORDER_PACKETS)
    assert np.array_equal(_bits(g), want)
    assert float(g[3]) == 0.0  # ((0 + 1) + 1e8) + -1e8; with the 1 added last it would be 1
    rev = cc.oracle_decompress(n, cc.ORDER_PACKETS[::-1])
    assert cc.b2f(rev)[3] == 1.0  # the inputs do tell the orders apart


def test_bad_arguments_raise_and_touch_nothing():
    assert C.check(0, 1) == -2 and C.check(1 << 31, 1) == -2 and C.check((1 << 31) - 1, 1) == 0
    assert C.check(5, 0) == -3 and C.check(5, 6) == -3 and C.check(5, 5) == 0
    res, g = torch.ones(5), torch.full((5,), 2.0)
    packet = torch.full((4,), -1, dtype=torch.int32)
    for k in (0, 6):
        with pytest.raises(ValueError):
            C.compress_bucket(res, g, k, packet)
        with pytest.raises(ValueError):
            C.decompress_bucket(g, packet.view(1, -1), k)
    with pytest.raises(ValueError):
        C.compress_bucket(res[:0], g[:0], 1, packet)
    with pytest.raises(ValueError):
        C.compress_bucket(res, g, 3, packet)  # a packet of the wrong size
    with pytest.raises(ValueError):
        C.compress_bucket(res, g.double(), 2, packet)
    assert torch.equal(res, torch.ones(5)) and torch.equal(g, torch.full((5,), 2.0)) and bool((packet == -1).all())
    for n, rho, k in ((1, 0.5, 1), (8195, 1.0, 8195), (8195, 0.0002, 2), (100, 1e-9, 1), (1000, 0.0101, 11)):
        assert C.bucket_k(n, rho) == k == cc.bucket_k(n, rho)


@pytest.mark.parametrize("ratio", [0.0, -0.1, 1.5, float("nan"), "x"])
def test_config_refuses_a_ratio_outside_0_1(ratio):
    with pytest.raises(ValueError):
        C.GradCompress(ratio)


def test_config_and_constructor_refusals():
    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    from distributed_tensorflow_models_amd.parallel.bsp import BSPDataParallel
    with pytest.raises(ValueError):
        C.GradCompress(0.1, begin_step=-1)
    p = [torch.nn.Parameter(torch.zeros(10))]
    with pytest.raises(ValueError):
        BSPDataParallel(p, comm_dtype=torch.bfloat16, compress=C.GradCompress(0.1))
    with pytest.raises(ValueError):
        BSPDataParallel(p, compress=0.1)
    model = nets_factory.build("cifar10_cnn", num_classes=10)
    with pytest.raises(ValueError):
        TrainStep(model, use_graph=True, grad_compress=C.GradCompress(0.1))
    with pytest.raises(ValueError):
        TrainStep(model, grad_comm_dtype=torch.bfloat16, grad_compress=C.GradCompress(0.1))
    with pytest.raises(ValueError):
        TrainStep(model, grad_compress=0.1)


# ---- step level -----------------------------------------------------------------------------------------------------
B, S = 8, 24


def _batch():
    g = torch.Generator().manual_seed(123)
    return torch.randn(B, S, S, 3, generator=g), torch.randint(0, 10, (B,), generator=g)


def _make(cfg, accum=1):
    from distributed_tensorflow_models_amd.engine import TrainStep
    from distributed_tensorflow_models_amd.models import nets_factory
    torch.manual_seed(0)
    model = nets_factory.build("cifar10_cnn", num_classes=10)
    return model, TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, bucket_mb=0.25, grad_compress=cfg,
                            accum_steps=accum)


def _params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


def _bsp_worker(rank, world, steps=3):
    """tests/test_distributed.py's worker with the compression config added: dense, rho 0.05 and rho 1 in one spawn."""
    from distributed_tensorflow_models_amd.parallel import process_group as pg
    x, y = _batch()
    per = B // world
    xs, ys = x[rank * per:(rank + 1) * per], y[rank * per:(rank + 1) * per]
    out = {}
    for name, cfg in (("dense", None), ("r005", C.GradCompress(0.05)), ("r1", C.GradCompress(1.0))):
        model, step = _make(cfg)
        pg.broadcast_tensors(list(model.parameters()))
        losses = [float(step(xs, ys)) for _ in range(steps)]
        out[name] = {"params": _params(model), "losses": losses, "buckets": len(step.dp.buckets),
                     "wire": step.dp.wire_elements(), "res": step.dp.residual_norm()}
        step.dp.close()
    return out


def test_two_gloo_ranks_stay_identical_and_rho_1_equals_dense():
    res = run_workers(_bsp_worker, 2)
    assert res[0]["dense"]["buckets"] > 1
    for name in ("dense", "r005", "r1"):
        assert torch.equal(res[0][name]["params"], res[1][name]["params"])  # replicas stay bit-identical
    assert not torch.equal(res[0]["r005"]["params"], res[0]["dense"]["params"])
    # rho = 1: every element travels, (0 + a) + b is the all-reduce's two-term sum (value equality: -0 == +0)
    assert bool((res[0]["r1"]["params"] == res[0]["dense"]["params"]).all())
    assert res[0]["r1"]["res"] == 0.0 and res[0]["r005"]["res"] > 0.0 and res[0]["dense"]["res"] == 0.0
    assert res[0]["r1"]["wire"] == 2 * res[0]["dense"]["wire"]
    assert res[0]["r005"]["wire"] < 0.11 * res[0]["dense"]["wire"]


def test_begin_step_runs_dense_first_and_leaves_the_residual_zero():
    x, y = _batch()
    md, dense = _make(None)
    mc, comp = _make(C.GradCompress(0.05, begin_step=2))
    dense_wire = dense.dp.wire_elements()
    for t in range(3):
        assert comp.dp.compressing() == (t >= 2)
        dense(x, y)
        comp(x, y)
        if t < 2:
            assert torch.equal(_params(md), _params(mc))
            assert comp.dp.res is None or not bool(comp.dp.res.any())
            assert comp.dp.wire_elements(t) == dense_wire
    assert not torch.equal(_params(md), _params(mc))
    assert comp.dp.residual_norm() > 0 and comp.dp.wire_elements(2) < 0.11 * dense_wire
    # off: nothing is constructed
    assert dense.dp.compress is None and dense.dp.res is None and not dense.dp.packets and not dense.dp._cbufs
    assert dense.dp._cscratch is None and not dense.dp.compressing()
    dense.dp.close()
    comp.dp.close()


def test_accumulation_compresses_the_folded_gradient():
    """accum_steps = 2, one step, W = 1: the dense run's flat buffer after the step is the folded gradient G; the
    compressed run's buffer and residual must be the function applied by hand to G, bucket by bucket."""
    x, y = _batch()
    _md, dense = _make(None, accum=2)
    _mc, comp = _make(C.GradCompress(0.05), accum=2)
    dense(x, y)
    comp(x, y)
    G = dense.dp.flat
    assert comp.dp.buckets == dense.dp.buckets and len(comp.dp.buckets) > 1
    for bi, (s, e) in enumerate(comp.dp.buckets):
        k = cc.bucket_k(e - s, 0.05)
        idx, val, new_res, u = cc.oracle(np.zeros(e - s, np.uint32), _bits(G[s:e]), k)
        assert np.array_equal(comp.dp.packets[bi].numpy()[:k], idx)
        assert np.array_equal(comp.dp.packets[bi].numpy()[k:].view(np.uint32), val)
        assert np.array_equal(_bits(comp.dp.res[s:e]), new_res)
        assert np.array_equal(_bits(comp.dp.flat[s:e]), cc.oracle_decompress(e - s, [(idx, val)]))
    dense.dp.close()
    comp.dp.close()


def test_convergence_on_one_repeated_batch():
    """cifar10_cnn, momentum 0.9, lr 0.05, one repeated batch of 8, 12 steps, world 1.  The condition: the compressed
    run (rho = 0.05) ends below its own first-step loss; the dense run satisfies the same condition with room.
    The 12 losses recorded on the CPU path:
      dense       2.3137 2.0680 1.9689 1.7906 1.7183 1.5061 1.3551 1.6039 0.7930 0.7311 0.4527 0.2812
      rho = 0.05  2.3137 2.0698 1.9644 1.8064 1.7289 1.5845 1.3692 1.0119 0.6671 0.5257 0.8987 0.1024
    12 steps: both curves are below half their first value from step 8 on, so the condition holds with room.
    """
    x, y = _batch()
    for cfg in (None, C.GradCompress(0.05)):
        _m, step = _make(cfg)
        losses = [float(step(x, y)) for _ in range(12)]
        print(cfg, " ".join("%.4f" % v for v in losses))
        assert all(np.isfinite(losses))
        assert losses[-1] < losses[0], losses
        step.dp.close()


# ---- the trainer ----------------------------------------------------------------------------------------------------
def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--synthetic_data", "--batch_size=8", "--data_dir=/nonexistent", "--seed=3", "--max_steps=3"]


@pytest.mark.parametrize("args,message", [
    (["--grad_compress_ratio=0.05", "--sync_mode=asp"], "--grad_compress_ratio needs --sync_mode bsp"),
    (["--grad_compress_ratio=0.05", "--sync_mode=ssp"], "--grad_compress_ratio needs --sync_mode bsp"),
    (["--grad_compress_ratio=0.05", "--grad_comm_dtype=bf16"], "--grad_compress_ratio and --grad_comm_dtype bf16"),
    (["--grad_compress_ratio=0.05", "--use_hipgraph"], "--grad_compress_ratio and --use_hipgraph"),
    (["--grad_compress_ratio=1.5"], "ratio must lie in (0, 1]"),
    (["--grad_compress_ratio=-0.5"], "ratio must lie in (0, 1]"),
], ids=["asp", "ssp", "bf16", "hipgraph", "above-1", "negative"])
def test_trainer_refuses_at_start_up(tmp_path, args, message):
    d = tmp_path / "train"
    p = _trainer("mnist_lenet_bsp", "--train_dir=%s" % d, *(COMMON + args))
    assert p.returncode != 0
    assert "ValueError" in p.stderr and message in p.stderr, p.stderr[-2000:]
    assert not d.exists()  # refused before anything was set up


def test_trainer_logs_ratio_wire_and_residual(tmp_path):
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    p = _trainer("mnist_lenet_bsp", "--train_dir=" + d, "--grad_compress_ratio=0.05", "--grad_compress_begin_step=1",
                 "--metrics_file=" + mf, *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    recs = [json.loads(line) for line in open(mf)]
    assert [r["global_step"] for r in recs] == [1, 2, 3]
    assert all(r["grad_compress_ratio"] == 0.05 for r in recs)
    assert recs[0]["residual_norm"] == 0.0 and recs[1]["residual_norm"] > 0.0  # step 0 ran dense
    assert recs[1]["wire_mb"] < 0.11 * recs[0]["wire_mb"] and recs[2]["wire_mb"] == recs[1]["wire_mb"]
    assert all(np.isfinite(r["loss"]) for r in recs)
