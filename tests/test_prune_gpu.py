"""Gradual magnitude pruning on the GPU: the radix-select and apply kernels against the numpy oracle (equal, no
tolerance), the early exits, the entry points' refusals, TrainStep(prune=...) captured against eager, sibling groups."""
import ctypes

import numpy as np
import pytest
import torch

import prune_cases as cases
from distributed_tensorflow_models_amd.engine import PruneConfig, TrainStep, prepare_compute_copies
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib, prune
from test_mix_gpu import deterministic  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5A5A5A5A


def test_chunk_size_is_the_one_the_cases_assume():
    assert _lib.lib().dtm_prune_chunk_size() == cases.CHUNK and _lib.lib().dtm_prune_hist_bins() == 2048


class Layout:
    """Tensors of the given element counts in one flat fp32 buffer, tensor i starting ``offs[i]`` elements past a
    16-byte boundary; a bf16 buffer and a shadow buffer of the same layout beside it."""

    def __init__(self, sizes_offs, name, seed=0, copies=True, vector=True):
        self.spans, pos = [], 0
        for n, off in sizes_offs:
            start = (pos + 3) // 4 * 4 + 4 + off  # (a gap of at least 4 elements in front of every tensor)
            self.spans.append((start, n))
            pos = start + n
        total = pos + 8
        self.bits = np.full(total, SENTINEL, np.uint32)  # the gaps hold a sentinel no kernel may touch
        for i, (start, n) in enumerate(self.spans):
            self.bits[start:start + n] = cases.value_set(name, n, seed + i % 4)
        self.src = torch.from_numpy(self.bits.view(np.int32)).to(DEV).view(torch.float32)
        assert self.src.data_ptr() % 16 == 0
        self.w = self.src.clone()
        self.sh = self.src.clone() if copies else None
        self.src16 = self.src.to(torch.bfloat16) if copies else None  # (values only: the gaps are compared as bf16)
        self.w16 = self.src16.clone() if copies else None
        ent = []
        for i, (start, n) in enumerate(self.spans):
            assert (self.w[start:].data_ptr() % 16) // 4 == sizes_offs[i][1]
            ent.append(("t%d" % i, self.w[start:start + n],
                        self.w16[start:start + n] if copies else None, self.sh[start:start + n] if copies else None))
        self.pruner = prune.Pruner(ent, vector=vector)

    def reset(self):
        self.pruner.reset()  # (an update applies the masks so far first: every case starts from all ones)
        self.w.copy_(self.src)
        if self.sh is not None:
            self.sh.copy_(self.src)
            self.w16.copy_(self.src16)

    def host(self):
        torch.cuda.synchronize()
        p = self.pruner
        out = {"w": self.w.view(torch.int32).cpu().numpy().view(np.uint32),
               "masks": [m.cpu().numpy() for m in p.masks], "tau": p.tau.cpu().numpy(), "kept": p.kept.cpu().numpy(),
               "z": p.z.cpu().numpy()}
        if self.sh is not None:
            out["sh"] = self.sh.view(torch.int32).cpu().numpy().view(np.uint32)
            out["w16"] = self.w16.view(torch.int16).cpu().numpy().view(np.uint16)
        return out

    def check(self, sparsity, got=None, which=None):
        """Everything the update wrote, against the oracle: equal."""
        got = got or self.host()
        want_w = self.bits.copy()
        src16 = self.src16.view(torch.int16).cpu().numpy().view(np.uint16) if self.sh is not None else None
        want16 = src16.copy() if src16 is not None else None
        for i, (start, n) in enumerate(self.spans):
            if which is not None and i not in which:
                continue
            mask, tau, kept, z = cases.oracle(self.bits[start:start + n], sparsity)
            tag = (i, n, start % 4, sparsity)
            assert (int(got["tau"][i]), int(got["kept"][i]), int(got["z"][i])) == (tau, kept, z), tag
            assert np.array_equal(got["masks"][i].reshape(-1), mask), tag
            want_w[start:start + n][mask == 0] = 0
            if want16 is not None:
                want16[start:start + n][mask == 0] = 0
        if which is None:
            assert np.array_equal(got["w"], want_w)  # kept elements bit for bit, pruned ones +0, the gaps untouched
            if want16 is not None:
                assert np.array_equal(got["sh"], want_w) and np.array_equal(got["w16"], want16)
        return got


ALL = [(n, off) for n in cases.SIZES for off in (0, 1, 2, 3)]


@pytest.mark.parametrize("name", cases.SETS)
def test_kernels_equal_the_oracle(name):
    """One call carries every size at every offset from a 16-byte boundary; one call per sparsity of any size."""
    lay = Layout(ALL, name)
    for s in sorted({s for n in cases.SIZES for s in cases.sparsities(n)}):
        lay.reset()
        lay.pruner.step(s, True)
        lay.check(s)


def test_ranks_at_bin_ends():
    """Consecutive keys: the running count of the scan equals the rank exactly at a bin's end (second digit: every
    1024th key; last digit: every key), with the ranks 1 and n - 1."""
    n = 3 * cases.CHUNK + 5
    lay = Layout([(n, off) for off in (0, 1, 2, 3)], "digit1", copies=False)
    zs = cases.bin_end_ranks(cases.BASE1, n)
    assert len(zs) >= 20
    for z in zs + [z + 1 for z in zs[1:-1:6]] + [z - 1 for z in zs[1:-1:6]]:
        s = cases.sparsity_for_rank(z, n)
        lay.reset()
        lay.pruner.step(s, True)
        got = lay.check(s)
        assert [int(t) for t in got["tau"]] == [cases.BASE1 + z - 1] * 4 and [int(k) for k in got["kept"]] == [n - z] * 4
    # both digits shared, and keys that cross a boundary of the FIRST digit at rank 100
    lay = Layout([(1024, 1), (257, 2)], "digit12", copies=False)
    cross = np.arange(0x3D100000 - 100, 0x3D100000 + 157, dtype=np.uint32)
    np.random.default_rng(3).shuffle(cross)
    start = lay.spans[1][0]
    lay.bits[start:start + 257] = cross
    lay.src[start:start + 257] = torch.from_numpy(cross.view(np.int32)).to(DEV).view(torch.float32)
    for z in (1, 99, 100, 101, 256, 512, 1023):
        s = cases.sparsity_for_rank(z, 1024)  # (rank floor(s * 257) of the second tensor follows from it)
        lay.reset()
        lay.pruner.step(s, True)
        lay.check(s)
    for z in (99, 100, 101, 256):
        s = cases.sparsity_for_rank(z, 257)
        lay.reset()
        lay.pruner.step(s, True)
        got = lay.check(s)
        assert int(got["tau"][1]) == 0x3D100000 - 100 + z - 1


def test_scalar_path_gives_the_same_bytes():
    sizes = [(n, off) for n in (7, 257, cases.CHUNK + 1, 3 * cases.CHUNK + 5) for off in (0, 3)]
    outs = []
    for vector in (True, False):
        lay = Layout(sizes, "special", vector=vector)
        lay.pruner.step(0.5, True)
        got = lay.check(0.5)
        lay.pruner.step(0.9, False)  # and an apply alone
        outs.append((got, lay.host()))
    for a, b in zip(outs[0], outs[1]):
        for k in ("w", "sh", "w16", "tau", "kept", "z"):
            assert np.array_equal(a[k], b[k]), k
        assert all(np.array_equal(x, y) for x, y in zip(a["masks"], b["masks"]))


def test_apply_alone_and_the_early_exits():
    lay = Layout([(n, off) for n in (65, 257, cases.CHUNK + 1) for off in (0, 1, 2, 3)], "normal")
    p = lay.pruner
    p.step(0.5, True)
    first = lay.check(0.5)
    # the optimizer moves every coordinate; a NaN lands on a pruned one
    torch.cuda.synchronize()
    moved = torch.randn(lay.w.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    pruned_at = []
    for (start, n), m in zip(lay.spans, first["masks"]):
        lay.w[start:start + n] = moved[start:start + n]
        lay.sh[start:start + n] = moved[start:start + n]
        lay.w16[start:start + n] = moved[start:start + n].to(torch.bfloat16)
        j = start + int(np.flatnonzero(m.reshape(-1) == 0)[0])
        lay.w[j] = float("nan")
        lay.sh[j] = float("nan")
        lay.w16[j] = float("nan")
        pruned_at.append(j)
    before = {"w": lay.w.clone(), "sh": lay.sh.clone(), "w16": lay.w16.clone()}
    p._state.fill_(SENTINEL)
    p._hist.fill_(SENTINEL)
    p.step(0.9, False)  # update == 0: select exits at once, apply only applies
    got = lay.host()
    assert bool((p._state == SENTINEL).all()) and bool((p._hist == SENTINEL).all())  # the select stage wrote nothing
    for k in ("tau", "kept", "z"):
        assert np.array_equal(got[k], first[k])
    assert all(np.array_equal(a, b) for a, b in zip(got["masks"], first["masks"]))
    keep = np.ones(lay.bits.size, bool)
    for (start, n), m in zip(lay.spans, first["masks"]):
        keep[start:start + n] = m.reshape(-1) != 0
    for k, view, np_t in (("w", torch.int32, np.uint32), ("sh", torch.int32, np.uint32), ("w16", torch.int16, np.uint16)):
        was = before[k].view(view).cpu().numpy().view(np_t)
        now = got[k]
        assert np.array_equal(now[keep], was[keep]) and not now[~keep].any()  # (the NaNs did not survive)
    assert all(not keep[j] for j in pruned_at)
    # an update after the sentinel fill: the init kernel clears what the stages read
    lay.reset()
    p.step(0.9, True)
    lay.check(0.9)


def test_masks_only_shrink_across_updates():
    """The stored masks are applied in front of an update's selection: what the optimizer wrote to a pruned
    coordinate, however large, does not bring it back."""
    lay = Layout([(257, 1), (cases.CHUNK + 1, 2)], "normal")
    p = lay.pruner
    p.step(0.5, True)
    first = lay.check(0.5)
    for (start, n), m in zip(lay.spans, first["masks"]):
        off = torch.from_numpy(m.reshape(-1) == 0).to(DEV)
        lay.w[start:start + n][off] = 100.0
    p.step(0.7, True)
    got = lay.host()
    for i, ((start, n), m0, m1) in enumerate(zip(lay.spans, first["masks"], got["masks"])):
        assert not (m1.astype(bool) & ~m0.astype(bool)).any()
        masked = lay.bits[start:start + n].copy()
        masked[m0.reshape(-1) == 0] = 0
        mask, tau, kept, z = cases.oracle(masked, 0.7)
        assert np.array_equal(m1.reshape(-1), mask) and (int(got["tau"][i]), int(got["kept"][i])) == (tau, kept)
        assert not got["w"][start:start + n][mask == 0].any()


def test_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    lay = Layout([(257, 1), (65, 0)], "normal")
    p = lay.pruner
    p.step(0.5, True)
    before = lay.host()
    p._state.fill_(SENTINEL)
    args = (_lib.ptr(p._tens_dev), 2, _lib.ptr(p._chunks_dev), p._nchunks, _lib.ptr(p._rec))
    for max_n in (2 ** 31, 2 ** 33, 0):
        assert L.dtm_prune_select(*args, _lib.ptr(p._state), _lib.ptr(p._hist), _lib.ptr(p.tau), _lib.ptr(p.kept),
                                  _lib.ptr(p.z), max_n, _lib.stream_ptr()) == -2
        assert L.dtm_prune_apply(*args, _lib.ptr(p.tau), _lib.ptr(p.kept), _lib.ptr(p.z), max_n, 0,
                                 _lib.stream_ptr()) == -2
    assert L.dtm_prune_num_chunks(_lib.ptr(lay.w), 2 ** 31) == -2 and L.dtm_prune_num_chunks(_lib.ptr(lay.w), 0) == -2
    assert L.dtm_prune_num_chunks(_lib.ptr(lay.w), 2 ** 31 - 1) == (2 ** 31 - 1 + cases.CHUNK - 1) // cases.CHUNK
    assert L.dtm_prune_select(None, 2, *args[2:], _lib.ptr(p._state), _lib.ptr(p._hist), _lib.ptr(p.tau),
                              _lib.ptr(p.kept), _lib.ptr(p.z), 257, _lib.stream_ptr()) == -1
    row = (ctypes.c_ubyte * 16)(*([0xAB] * 16))
    for bad in (1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert L.dtm_prune_fill_record(row, bad, 1) == -3 and bytes(row) == b"\xab" * 16
        with pytest.raises(ValueError):
            p.stage(bad, True)
    assert L.dtm_prune_fill_record(row, 0.25, 7) == 0
    assert np.frombuffer(bytes(row), np.float64, 1)[0] == 0.25 and list(np.frombuffer(bytes(row), np.int32)[2:]) == [1, 0]
    after = lay.host()  # nothing was launched: every output as before, the scratch still the sentinel
    assert bool((p._state == SENTINEL).all())
    for k in ("w", "sh", "w16", "tau", "kept", "z"):
        assert np.array_equal(before[k], after[k]), k


# ---- TrainStep: captured against eager ----------------------------------------------------------------------------
MB = 16
STEPS = 12


def lenet():
    torch.manual_seed(0)
    return nets_factory.build("lenet", 10, dropout_keep_prob=1.0).to(DEV)


def batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(MB, 28, 28, 1, generator=g).to(DEV, torch.bfloat16),
             torch.randint(0, 10, (MB,), generator=g).to(DEV)) for _ in range(n)]


def run_steps(graph, accum=1, optimizer="momentum", cfg="default"):
    if cfg == "default":
        cfg = PruneConfig(0.8, begin_step=1, frequency=3, end_step=10)
    model = lenet()
    step = TrainStep(model, optimizer=optimizer, lr=0.05 if optimizer == "momentum" else 0.002, momentum=0.9,
                     ema_decay=0.99, accum_steps=accum, prune=cfg, use_graph=graph)
    data = batches(STEPS * accum)
    losses, sparsity = [], []
    for s in range(STEPS):
        xs, ys = (list(v) for v in zip(*data[s * accum:(s + 1) * accum]))
        losses.append(float(step(xs, ys) if accum > 1 else step(xs[0], ys[0])))
        if cfg is not None:
            sparsity.append(step.last_sparsity())
    torch.cuda.synchronize()
    assert (step._graph is not None) == graph and step.global_step == STEPS
    state = [p.detach().clone() for p in model.parameters()]
    state += [p.bf16.clone() for p in model.parameters() if getattr(p, "bf16", None) is not None]
    state += [st["ema"].clone() for st in step.opt.state.values()]
    if cfg is not None:
        state += [m.clone() for m in step.pruner.masks] + [step.pruner.tau.clone(), step.pruner.kept.clone()]
        for p, m in zip(step.pruner.params, step.pruner.masks):
            off = m == 0
            for v in (p.detach(), p.bf16, step.opt.state[p]["ema"]):
                assert not v.view(torch.int32 if v.dtype == torch.float32 else torch.int16)[off].any()
            assert torch.equal(p.bf16, p.detach().to(torch.bfloat16))
    step.dp.close()
    return losses, state, sparsity


@pytest.mark.parametrize("accum,optimizer", [(1, "momentum"), (2, "momentum"), (1, "adam")])
def test_captured_step_matches_eager(deterministic, accum, optimizer):  # noqa: F811
    """Two eager warm-up steps (the update of step 1 among them), the capture between two updates, and replays that
    cross the updates of steps 4, 7 and 10."""
    cfg = PruneConfig(0.8, begin_step=1, frequency=3, end_step=10)
    assert [t for t in range(STEPS) if cfg.updates_at(t)] == [1, 4, 7, 10]
    le, se, spe = run_steps(False, accum, optimizer)
    lg, sg, spg = run_steps(True, accum, optimizer)
    assert le == lg, (le, lg)
    assert len(se) == len(sg) and all(torch.equal(a, b) for a, b in zip(se, sg))
    assert spe == spg and [t for _a, t in spe] == [cfg.sparsity_at(t) for t in range(STEPS)]
    achieved = [a for a, _t in spe]
    assert all(a <= b for a, b in zip(achieved, achieved[1:])) and achieved[0] == 0.0
    assert len(set(achieved)) == 4  # 0, then the updates of steps 4, 7 and 10 (step 1's asks for sparsity 0)
    assert 0.8 - 1e-4 <= achieved[10] <= 0.8 + 1e-4 and achieved[11] == achieved[10]


def test_prune_none_is_the_plain_step(deterministic):  # noqa: F811
    l0, s0, _ = run_steps(False, cfg=None)
    model = lenet()
    step = TrainStep(model, optimizer="momentum", lr=0.05, momentum=0.9, ema_decay=0.99)
    l1 = [float(step(x, y)) for x, y in batches(STEPS)]
    torch.cuda.synchronize()
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(s0, [p.detach() for p in model.parameters()]))
    step.dp.close()
    assert l0 != run_steps(False)[0]


# ---- sibling groups ---------------------------------------------------------------------------------------------
def test_sibling_group_views_are_masked_and_their_neighbours_untouched():
    """An Inception mixed block's 1x1 heads keep their bf16 copies as views into one buffer: pruning two of the heads
    masks their rows of it and leaves the rows between and behind them alone."""
    torch.manual_seed(0)
    net = nets_factory.build("inception_v3_slim_old", num_classes=11).to(DEV)
    prepare_compute_copies(net)
    group = net.sibling_weight_groups()[0]
    assert len(group) >= 3
    buf, _off = group[0]._sib_cat
    assert all(p._sib_cat[0] is buf and p.bf16.data_ptr() == buf[p._sib_cat[1]:].data_ptr() for p in group)
    before = buf.clone()
    chosen = [group[0], group[2]]
    want = []
    for p in chosen:
        bits = p.detach().view(torch.int32).cpu().numpy().view(np.uint32)
        want.append((bits.copy(), cases.oracle(bits, 0.6)))
    pr = prune.Pruner([("h%d" % i, p.data, p.bf16, None) for i, p in enumerate(chosen)])
    pr.step(0.6, True)
    torch.cuda.synchronize()
    touched = torch.zeros(buf.shape[0], dtype=torch.bool)
    for i, (p, (bits, (mask, tau, kept, z))) in enumerate(zip(chosen, want)):
        assert (int(pr.tau[i]), int(pr.kept[i]), int(pr.z[i])) == (tau, kept, z)
        assert np.array_equal(pr.masks[i].cpu().numpy(), mask)
        rows = slice(p._sib_cat[1], p._sib_cat[1] + p.shape[0])
        touched[rows] = True
        now = buf[rows].view(torch.int16).cpu().numpy()
        was = before[rows].view(torch.int16).cpu().numpy()
        assert np.array_equal(now[mask != 0], was[mask != 0]) and not now[mask == 0].any()
        w = p.detach().view(torch.int32).cpu().numpy().view(np.uint32)
        assert np.array_equal(w[mask != 0], bits[mask != 0]) and not w[mask == 0].any()
    assert 0 < int(touched.sum()) < buf.shape[0]
    assert torch.equal(buf[~touched.to(DEV)], before[~touched.to(DEV)])
