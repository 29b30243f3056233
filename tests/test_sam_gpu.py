"""Sharpness-aware minimisation on the GPU: the four launches of csrc/kernels/sam.hip against the torch form of
ops/sam.py (both access paths, guards, bit copies, non-finite values, bad arguments), and TrainStep(sam=...) on the
device against the composition written out by hand (tests/sam_cases.py): eager, captured, accumulated, with forced
collectives, mixing and distillation."""
import math

import pytest
import torch

from distributed_tensorflow_models_amd.engine import DistillConfig, TrainStep, moving_average_buffers
from distributed_tensorflow_models_amd.models import nets_factory
from distributed_tensorflow_models_amd.ops import _lib, sam
from distributed_tensorflow_models_amd.ops import elementwise as E
from distributed_tensorflow_models_amd.ops.mix import MixConfig
from distributed_tensorflow_models_amd.ops.sam import SamConfig
from distributed_tensorflow_models_amd.utils.testing import run_workers

import sam_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64  # elements on each side of every array, holding 7.0
LENGTHS = [1, 3, 4, 255, 256, 1027, 8197, 3 * 8192 + 5]
TABLES = [[1], [3, 4], [255, 256, 1027], [8197], [3 * 8192 + 5, 3], [4, 8197, 255]]  # every length, 1-3 tensors
ALIGNED = [(0, 0), (1, 1), (2, 2), (3, 3)]  # weight and gradient reach a 16-byte boundary together
SPLIT = [(0, 1), (2, 3)]                    # they never do: 4-byte accesses
NAN_PAYLOAD = 0x7FC01234
STAT_LEN = 37  # the backup-only row


def _guarded(n, off, dtype=torch.float32):
    buf = torch.full((GUARD + off + n + GUARD,), 7.0, dtype=dtype)
    return buf, slice(GUARD + off, GUARD + off + n)


def _plant(p, with_nan):
    """-0.0, a subnormal, 3e38 and (``with_nan``) a NaN with a payload, at fixed places (the last win where n is
    tiny)."""
    n = p.numel()
    vals = [(-0.0, None), (1e-41, None), (3e38, None)] + ([(None, NAN_PAYLOAD)] if with_nan else [])
    for k, (v, bits) in enumerate(vals):
        i = (k * 7919 + 3) % n
        if bits is None:
            p[i] = v
        else:
            p.view(torch.int32)[i] = bits


class Case:
    """One table on the CPU (the torch form's tensors) and its copy on the device."""

    def __init__(self, lengths, off_p, off_g, with_copy, cfg, seed, planted=True, g_fix=None):
        gen = torch.Generator().manual_seed(seed)
        self.cfg = cfg
        self.cpu, self.slices = [], []
        for n in lengths:
            p, sp = _guarded(n, off_p)
            g, sg = _guarded(n, off_g)
            b, _ = _guarded(n, off_p)
            p[sp] = torch.randn(n, generator=gen) * 0.3
            g[sg] = torch.randn(n, generator=gen) * 0.01
            b[sp] = 5.0
            if planted:
                _plant(p[sp], with_nan=not cfg.adaptive)  # (a NaN weight makes ASAM's S NaN: its own test below)
            c = None
            if with_copy:
                c, _ = _guarded(n, off_p, torch.bfloat16)
                c[sp] = p[sp].to(torch.bfloat16)
            self.cpu.append((p, g, b, c))
            self.slices.append((sp, sg))
        if g_fix is not None:
            g_fix(self.cpu[0][1][self.slices[0][1]])
        stat, ss = _guarded(STAT_LEN, 1)
        sb, _ = _guarded(STAT_LEN, 1)
        stat[ss] = torch.randn(STAT_LEN, generator=gen)
        self.stat_cpu, self.stat_slice = (stat, sb), ss
        self.dev = [tuple(None if t is None else t.to(DEV) for t in row) for row in self.cpu]
        self.stat_dev = tuple(t.to(DEV) for t in self.stat_cpu)
        for row in self.dev + [self.stat_dev]:
            assert all(t is None or t.data_ptr() % 16 == 0 for t in row)
        self.old = [tuple(None if t is None else t.clone() for t in row) for row in self.cpu]
        self.old_stat = self.stat_cpu[0].clone()

    def perturber(self, rows, stat):
        ent = [(p[sp], g[sg], None if c is None else c[sp], b[sp]) for (p, g, b, c), (sp, sg) in zip(rows, self.slices)]
        return sam.SamPerturber(ent, [(stat[0][self.stat_slice], stat[1][self.stat_slice])], config=self.cfg)

    def old_p(self):
        return [p[sp] for (p, _g, _b, _c), (sp, _sg) in zip(self.old, self.slices)]

    def old_g(self):
        return [g[sg] for (_p, g, _b, _c), (_sp, sg) in zip(self.old, self.slices)]


def _check_case(lengths, off_p, off_g, with_copy, cfg, seed, planted=True):
    case = Case(lengths, off_p, off_g, with_copy, cfg, seed, planted)
    what = "lengths %r offsets %d/%d copy %s %r" % (lengths, off_p, off_g, with_copy, cfg)
    dev = case.perturber(case.dev, case.stat_dev)
    cpu = case.perturber(case.cpu, case.stat_cpu)
    assert dev._dev is not None and cpu._dev is None
    dev.perturb()
    torch.cuda.synchronize()
    C.check_norm_scale(dev.last_norm(), dev.last_scale(), case.old_p(), case.old_g(), cfg.rho, cfg.adaptive, what)
    cpu.perturb_with(float(dev.last_scale()))  # the torch form from the device's own scale
    for (p, g, b, c), (pd, gd, bd, cd), (po, _go, _bo, _co), (sp, sg) in zip(case.cpu, case.dev, case.old,
                                                                            case.slices):
        assert C.same_bits(pd, p, nan_ok=True), what        # p_hat, and the guards around it
        assert C.same_bits(bd, b) and C.same_bits(bd[sp], po[sp]), what  # backup = the old bits
        assert C.same_bits(gd, g) and not gd[sg].view(torch.int32).any(), what  # +0 over the range, guards kept
        if c is not None:
            assert C.same_bits(cd, c, nan_ok=True), what    # bf16(p_hat) where p_hat is no NaN
        assert bool((pd[:sp.start] == 7.0).all()) and bool((pd[sp.stop:] == 7.0).all()), what
    assert C.same_bits(case.stat_dev[1], case.stat_cpu[1]) and C.same_bits(case.stat_dev[0], case.old_stat), what
    case.stat_dev[0][case.stat_slice].add_(1.0)  # the descent forward's in-place update of the statistic
    dev.restore()
    torch.cuda.synchronize()
    for (pd, gd, _bd, cd), (po, _go, _bo, co), (sp, sg) in zip(case.dev, case.old, case.slices):
        assert C.same_bits(pd, po), what                    # every old bit: -0.0, the NaN's payload, the subnormal
        assert not gd[sg].view(torch.int32).any(), what     # restore leaves the gradient alone
        if cd is not None:
            want = co.clone()
            want[sp] = po[sp].to(torch.bfloat16)
            # bit for bit, but for the planted NaN: its bf16 encoding is the converter's choice (on an MI355X the
            # device's conversion and torch's CPU one encode the NaN 0x7FC01234 differently)
            assert C.same_bits(cd, want, nan_ok=True), what
    assert C.same_bits(case.stat_dev[0], case.old_stat), what
    return dev


@pytest.mark.parametrize("with_copy", [False, True], ids=["nocopy", "copy"])
@pytest.mark.parametrize("cfg", [SamConfig(0.05), SamConfig(1.0, adaptive=True)], ids=["sam", "asam"])
def test_kernels_match_the_torch_form(cfg, with_copy):
    """Both access paths against the torch form, each with its own scale: so the two paths give the same p_hat bits
    for the same scale."""
    seed = 0
    for lengths in TABLES:
        for off_p, off_g in ALIGNED + SPLIT:
            seed += 1
            _check_case(lengths, off_p, off_g, with_copy, cfg, seed)
    assert sorted(set(n for t in TABLES for n in t)) == sorted(LENGTHS)


def test_two_runs_give_the_same_bits():
    for cfg in (SamConfig(0.05), SamConfig(1.0, adaptive=True)):
        recs = []
        for _ in range(2):
            case = Case([3 * 8192 + 5, 1027, 8197], 1, 1, True, cfg, seed=3, planted=False)
            dev = case.perturber(case.dev, case.stat_dev)
            dev.perturb()
            torch.cuda.synchronize()
            recs.append(dev._rec.clone())
        assert C.same_bits(recs[0], recs[1]) and float(recs[0][0]) > 0.0


def test_unplanted_table_and_a_nan_weight_under_asam():
    for cfg in (SamConfig(0.05), SamConfig(1.0, adaptive=True)):
        for off_p, off_g in ((2, 2), (0, 1)):
            _check_case([255, 8197], off_p, off_g, True, cfg, 5, planted=False)
    case = Case([1027], 1, 1, True, SamConfig(1.0, adaptive=True), 6, planted=False)
    case.dev[0][0].view(torch.int32)[case.slices[0][0].start + 9] = NAN_PAYLOAD
    old = case.dev[0][0].clone()
    dev = case.perturber(case.dev, case.stat_dev)
    dev.perturb()
    dev.restore()
    torch.cuda.synchronize()
    assert math.isnan(float(dev.last_norm())) and C.same_bits(case.dev[0][0], old)


@pytest.mark.parametrize("offsets", [(1, 1), (0, 1)], ids=["16B", "4B"])
def test_nonfinite_gradients(offsets):
    def nan(g):
        g[g.numel() // 2] = float("nan")

    def inf(g):
        g[g.numel() // 2] = float("inf")
    for fix, all_nan in ((nan, True), (inf, False)):
        case = Case([1027, 255], offsets[0], offsets[1], True, SamConfig(0.05), 8, planted=True, g_fix=fix)
        dev = case.perturber(case.dev, case.stat_dev)
        dev.perturb()
        torch.cuda.synchronize()
        got = [pd[sp].cpu() for (pd, _g, _b, _c), (sp, _sg) in zip(case.dev, case.slices)]
        old = case.old_p()
        if all_nan:
            assert math.isnan(float(dev.last_scale())) and all(bool(torch.isnan(t).all()) for t in got)
        else:
            assert float(dev.last_scale()) == 0.0 and math.isinf(float(dev.last_norm()))
            where = torch.isnan(got[0]) & ~torch.isnan(old[0])
            assert where.nonzero().tolist() == [[1027 // 2]]  # e = 0 * Inf at that element only
            for t, o in zip(got, old):  # e = +-0 elsewhere: the values stay (-0.0 + 0.0 is +0.0)
                keep = ~torch.isnan(t)
                assert torch.equal(t[keep], o[keep])
        dev.restore()
        torch.cuda.synchronize()
        for (pd, _g, _b, _c), (po, _go, _bo, _co) in zip(case.dev, case.old):
            assert C.same_bits(pd, po)


def test_bad_arguments_launch_nothing():
    case = Case([1027], 0, 0, True, SamConfig(0.05), 9)
    dev = case.perturber(case.dev, case.stat_dev)
    L = _lib.lib()

    def perturb(rho, nchunks):
        return L.dtm_sam_perturb(_lib.ptr(dev._tens_dev), _lib.ptr(dev._chunks_dev), nchunks, _lib.ptr(dev._meta_dev),
                                 dev._ntens, rho, 0, _lib.ptr(dev._scratch), _lib.ptr(dev._rec), _lib.stream_ptr())

    def restore(rho, nchunks):
        return L.dtm_sam_restore(_lib.ptr(dev._tens_dev), _lib.ptr(dev._chunks_dev), nchunks, rho, _lib.stream_ptr())
    for rho, nchunks in ((-0.05, dev._nchunks), (0.0, dev._nchunks), (float("nan"), dev._nchunks),
                         (float("inf"), dev._nchunks), (0.05, 0)):
        assert perturb(rho, nchunks) < 0 and restore(rho, nchunks) < 0
    torch.cuda.synchronize()
    for row, old in zip(case.dev, case.old):
        assert all(C.same_bits(t, o) for t, o in zip(row, old) if t is not None)
    assert not dev._rec.any()
    assert perturb(0.05, dev._nchunks) == 0 and restore(0.05, dev._nchunks) == 0
    torch.cuda.synchronize()
    assert float(dev.last_norm()) > 0.0 and C.same_bits(case.dev[0][0], case.old[0][0])


# ---- the step ---------------------------------------------------------------------------------------------------
MB, CLASSES = 8, 11


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


def _reset_seeds():
    torch.manual_seed(0)
    E.seed_offset(DEV).zero_()
    E.set_base_seed(1234)


def net(keep=0.8):
    """MobileNet-v1 0.25 at CIFAR size: conv + BN, depthwise conv + BN, dropout, the 1x1 logits layer."""
    _reset_seeds()
    return nets_factory.build("mobilenet_v1_025", num_classes=CLASSES, dropout_keep_prob=keep).to(DEV)


def rows(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 32, 32, 3, generator=g).to(DEV, torch.bfloat16),
            torch.randint(0, CLASSES, (n,), generator=g).to(DEV))


def run_pair(batches, cfg, n=1, keep=0.8, **kw):
    model = net(keep)
    step = TrainStep(model, sam=cfg, accum_steps=n, **kw)
    got_losses = [float(step(x, y)) for x, y in batches]
    torch.cuda.synchronize()
    got = C.model_state(model, step)
    step.dp.close()
    twin = net(keep)
    plain = TrainStep(twin, **kw)
    hand = C.HandSam(plain, cfg)
    want_losses = [float(hand.step(list(x.chunk(n)), list(y.chunk(n)), kw["lr"])) for x, y in batches]
    torch.cuda.synchronize()
    want = C.model_state(twin, plain)
    plain.dp.close()
    return got, want, got_losses, want_losses, step


KW = dict(optimizer="momentum", lr=0.05, momentum=0.9, ema_decay=0.99)


@pytest.mark.parametrize("cfg", [SamConfig(0.05), SamConfig(1.0, adaptive=True)], ids=["sam", "asam"])
def test_eager_step_matches_the_hand_composition(deterministic, cfg):
    x, y = rows(3 * MB)
    got, want, gl, wl, step = run_pair(list(zip(x.split(MB), y.split(MB))), cfg, **KW)
    assert any(getattr(p, "bf16", None) is not None for p in step.model.parameters())
    assert len(moving_average_buffers(step.model)) > 0 and step.samp.backup_bytes() > 0
    assert gl == wl and all(math.isfinite(v) for v in gl), (gl, wl)
    assert C.states_equal(got, want)
    assert step.global_step == 3 and step.last_sam_norm() > 0.0


def test_accumulated_step_matches_the_hand_composition(deterministic):
    x, y = rows(2 * 2 * MB, seed=6)
    got, want, gl, wl, step = run_pair(list(zip(x.split(2 * MB), y.split(2 * MB))), SamConfig(0.05), n=2, **KW)
    assert gl == wl and C.states_equal(got, want)
    assert step.dp.grad_scale == 0.5 and step.nonfinite_micro() == [0, 0]


def test_bn_statistics_are_the_plain_step_s(deterministic):
    x, y = rows(MB, seed=7)
    stats = []
    for cfg in (None, SamConfig(0.05), SamConfig(1.0, adaptive=True)):
        model = net()
        init = torch.cat([b.reshape(-1) for b in moving_average_buffers(model)]).clone()
        step = TrainStep(model, sam=cfg, **KW)
        step(x, y)
        torch.cuda.synchronize()
        stats.append(torch.cat([b.reshape(-1) for b in moving_average_buffers(model)]).clone())
        step.dp.close()
        assert not torch.equal(stats[-1], init)
    assert C.same_bits(stats[0], stats[1]) and C.same_bits(stats[0], stats[2])


@pytest.mark.parametrize("cfg", [SamConfig(0.05), SamConfig(1.0, adaptive=True)], ids=["sam", "asam"])
def test_captured_step_matches_eager(deterministic, cfg):
    """Two warm-up steps, the capture, two replays.  No dropout: an eager step draws a new host seed per step, a
    replayed graph keeps the captured one and advances the device offset."""
    x, y = rows(2 * MB, seed=9)
    batches = [(x[:MB], y[:MB]), (x[MB:], y[MB:])]
    runs = []
    for graph in (False, True):
        model = net(keep=1.0)
        step = TrainStep(model, sam=cfg, use_graph=graph, **KW)
        losses = [float(step(*batches[i % 2])) for i in range(5)]
        torch.cuda.synchronize()
        assert (step._graph is not None) == graph and step.global_step == 5 and not step.poll_skipped()
        runs.append((losses, C.model_state(model, step), step.last_sam_norm()))
        step.dp.close()
    (le, se, ne), (lg, sg, ng) = runs
    assert le == lg and all(math.isfinite(v) for v in le), (le, lg)
    assert C.states_equal(se, sg) and ne == ng and ne > 0.0


def test_nan_input_skips_and_leaves_every_bit(deterministic):
    x, y = rows(2 * MB, seed=8)
    model = net()
    step = TrainStep(model, sam=SamConfig(0.05), **KW)
    step(x[:MB], y[:MB])
    torch.cuda.synchronize()
    assert not step.poll_skipped()
    before = C.model_state(model, step)
    nstat = len(moving_average_buffers(model))
    bad = x[MB:].clone()
    bad[2, 5, 5, 0] = float("nan")
    step(bad, y[MB:])
    torch.cuda.synchronize()
    assert step.poll_skipped() and step.skipped == 1
    after = C.model_state(model, step)
    assert C.states_equal(before[:-nstat], after[:-nstat])  # weights, copies, slots, shadows
    step.dp.close()


def test_mixing_and_distillation_match_their_hand_compositions(deterministic):
    x, y = rows(MB, seed=10)
    torch.manual_seed(1)
    teacher = nets_factory.build("mobilenet_v1_025", num_classes=CLASSES, dropout_keep_prob=1.0).to(DEV)
    for extra in (dict(mix=MixConfig(mixup_alpha=0.4, cutmix_alpha=1.0, seed=3)),
                  dict(distill=DistillConfig(teacher, alpha=0.5, temperature=2.0))):
        got, want, gl, wl, step = run_pair([(x, y)], SamConfig(0.05), **dict(KW, **extra))
        assert gl == wl and math.isfinite(gl[0]), (extra, gl, wl)
        assert C.states_equal(got, want), extra


# ---- forced collectives (RCCL at world 1) -------------------------------------------------------------------------------
def _rccl_worker(rank, world):
    import torch.distributed as dist
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    _lib.set_deterministic(True)
    _lib.set_side_enabled(False)
    x, y = rows(2 * MB, seed=11)
    out = {}
    for forced in (False, True):
        model = net()
        step = TrainStep(model, sam=SamConfig(0.05), bucket_mb=0.25, force_comm=forced, **KW)
        losses = [float(step(x[i * MB:(i + 1) * MB], y[i * MB:(i + 1) * MB])) for i in range(2)]
        torch.cuda.synchronize()
        state = [t.cpu() for t in C.model_state(model, step)]
        nstat = len(moving_average_buffers(model)) + len(step.opt.buffer_shadows())
        out["run_%d" % forced] = {"state": state[:-nstat], "stats": state[-nstat:], "losses": losses,
                                  "works": len(step.dp._done_works), "buckets": len(step.dp.buckets)}
        step.dp.close()
    return out


def test_forced_collectives_change_nothing():
    r = run_workers(_rccl_worker, 1, backend="nccl")[0]
    off, on = r["run_0"], r["run_1"]
    assert off["works"] == 0 and on["works"] == on["buckets"] >= 2  # the collectives of a plain step, no more
    assert on["losses"] == off["losses"] and all(math.isfinite(v) for v in on["losses"])
    assert C.states_equal(on["state"], off["state"])  # weights, bf16 copies, slots and shadows: the same bits
    # the BN statistics (and their shadows) went through BufferSync's fp64 combine, which at one rank returns the
    # replica's own values up to fp32 rounding: the tolerance tests/test_distributed.py holds synced statistics to
    assert len(on["stats"]) == len(off["stats"]) > 0
    for a, b in zip(on["stats"], off["stats"]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
