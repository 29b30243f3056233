"""Single training step: forward -> loss -> backward (+ overlapped bucket all-reduce) -> fused update.

This is the MI355X replacement for the reference's per-step ``sess.run([train_op, loss,
global_step])``: no PS round trips, gradients reduced over RCCL while backward
runs, one multi-tensor optimizer launch, TF 1.x optimizer / loss semantics.
"""
import contextlib
import os

import torch

from .ops import _lib
from .ops import elementwise as _elementwise
from .ops import fused as _fused
from .ops import mix as _mix
from .ops import nn as F
from .ops import prune as _prune
from .ops import sam as _sam
from .ops.optim import FusedOptimizer
from .ops.compress import GradCompress  # noqa: F401  (TrainStep(grad_compress=GradCompress(...)))
from .ops.prune import PruneConfig  # noqa: F401  (TrainStep(prune=PruneConfig(...)))
from .ops.sam import SamConfig  # noqa: F401  (TrainStep(sam=SamConfig(...)))
from .parallel.bsp import BSPDataParallel, BufferSync
from .utils.profiler import range_pop, range_push, roctx


def prepare_compute_copies(model):
    """Create the bf16 compute copy of every matrix/conv weight (refreshed by the optimizer).  Weight groups the
    model declares (``sibling_weight_groups``: the 1x1 branch heads of an Inception mixed block, same input
    channels) get their copies as consecutive views of ONE [sum K][1][1][C] buffer, recorded as ``p._sib_cat =
    (buffer, row offset)``: the merged head conv reads them as one weight (ops.fused._SiblingGroup.forward_all)."""
    groups = model.sibling_weight_groups() if hasattr(model, "sibling_weight_groups") else []
    for grp in groups:
        if not grp or not all(p.is_cuda and p.dim() == 4 and p.shape[1:] == grp[0].shape[1:] for p in grp):
            continue
        if any(getattr(p, "_sib_cat", None) is not None for p in grp):
            continue
        buf = torch.empty((sum(p.shape[0] for p in grp),) + tuple(grp[0].shape[1:]), device=grp[0].device,
                          dtype=torch.bfloat16)
        off = 0
        for p in grp:
            v = buf[off:off + p.shape[0]]
            v.copy_(p.detach())
            p.bf16 = v
            p._sib_cat = (buf, off)
            off += p.shape[0]
    for p in model.parameters():
        if p.is_cuda and p.dim() >= 2 and getattr(p, "bf16", None) is None:
            p.bf16 = p.detach().to(torch.bfloat16)


def moving_average_buffers(model):
    """The tensors TF puts in moving_average_variables(): every BN moving mean / variance."""
    from .models.layers import tf_variables
    return [t for _n, t, _l, trainable in tf_variables(model)
            if not trainable and t.dtype == torch.float32 and t.is_floating_point()]


@contextlib.contextmanager
def side_forward(model, device=None, rng=False):
    """A training-mode forward NEXT TO the training run (the accuracy probe, the activation summaries): the BN
    moving statistics, which the fused training-mode kernels update in place, are saved on entry and put back on
    exit.  ``rng``: also put back the dropout seed stream and torch's CPU (and ``device``'s) generator state, so
    the training run is bit-identical with and without the forward."""
    bufs = moving_average_buffers(model)
    saved = [b.detach().clone() for b in bufs]
    if rng:
        seed = _elementwise._seed[0]
        cpu_state = torch.get_rng_state()
        dev_state = torch.cuda.get_rng_state(device) if (device is not None and device.type == "cuda") else None
    try:
        yield
    finally:
        with torch.no_grad():
            for b, v in zip(bufs, saved):
                b.copy_(v)
        if rng:
            _elementwise._seed[0] = seed
            torch.set_rng_state(cpu_state)
            if dev_state is not None:
                torch.cuda.set_rng_state(dev_state, device)


def moving_average_decays(model, buffers):
    """The moving-average decay of each BN statistic in ``buffers`` (None where unknown): a module BatchNorm
    (models/layers.py) carries ``decay``; slim / old-slim batch_norm tag their variables with ``_bn_decay``."""
    by_id = {}
    for m in model.modules():
        names = getattr(m, "tf_buffer_names", None)
        if names and getattr(m, "decay", None) is not None:
            for b in names:
                by_id[id(getattr(m, b))] = float(m.decay)
    return [getattr(b, "_bn_decay", by_id.get(id(b))) for b in buffers]


def reserved_cus_default():
    """CUs kept out of the compute grids' sizing under data parallelism (ops/_lib.set_reserved_cus):
    DTM_RESERVED_CUS if set, else RESERVED_CUS_DP.  (A pinned RCCL channel count - NCCL_MAX_NCHANNELS, trainer
    --rccl_channels - does not reserve anything by itself: reserving measured slower, see below.)"""
    v = os.environ.get("DTM_RESERVED_CUS")
    if v is not None:
        return int(v)
    return RESERVED_CUS_DP


# Measured on one MI355X with a CU-occupying copy kernel on a second stream for 8 ms of every backward standing in
# for the RCCL channels (profiles/ab/r4_ab_hog_reserve.log, ResNet-50): 16 CUs taken +2.4 % step, 32 CUs +3.5 %;
# reserving the same CUs from the compute grids' sizing made both worse (+3.3 %, +4.8 %; +0.8 % with no
# contention): the non-persistent tiles rebalance by themselves, so nothing is reserved by default.
RESERVED_CUS_DP = 0


def _map_batches(fn, a, *more):
    """fn over one batch (tensors) or over the micro-batches of a step (lists of tensors)."""
    if isinstance(a, list):
        return [fn(*t) for t in zip(a, *more)]
    return fn(a, *more)


def _stage(static, new):
    if new.data_ptr() != static.data_ptr():
        static.copy_(new, non_blocking=True)


class DistillConfig:
    """Knowledge distillation for TrainStep: ``teacher`` (a model of the zoo, already holding its trained weights)
    is frozen and run in inference mode on every micro-batch; the main head's loss becomes
    (1 - alpha) * hard + alpha * temperature^2 * KL(softmax(teacher / T) || softmax(student / T))."""
    __slots__ = ("teacher", "alpha", "temperature")

    def __init__(self, teacher, alpha=0.5, temperature=4.0):
        if not isinstance(teacher, torch.nn.Module):
            raise ValueError("the distillation teacher must be a torch.nn.Module, got %r" % (teacher,))
        F.Distill(torch.zeros(1, 1), alpha, temperature)  # its checks of alpha and temperature
        self.teacher, self.alpha, self.temperature = teacher, float(alpha), float(temperature)


class TrainStep:
    def __init__(self, model, optimizer="momentum", lr=0.1, momentum=0.9, rho=0.9, epsilon=None, bucket_mb=32.0,
                 label_smoothing=0.0, aux_weight=0.4, ema_decay=None, lr_schedule=None, use_graph=False,
                 process_group=None, weight_decay=None, batch_weight=1.0, nan_guard=True, timer=None,
                 grad_comm_dtype=None, ema_buffers=True, bn_sync_every=1, wgrad_stream=None, bsp_check=None,
                 overlap=True, force_comm=False, graph_comm=False, lars_eeta=0.001, lars_epsilon=0.0,
                 clip_global_norm=None, beta1=0.9, beta2=0.999, accum_steps=1, mix=None, rank=None,
                 distill=None, prune=None, lars_skip=None, sam=None, grad_compress=None):
        # epsilon None: the optimizer's own default (1e-10; Adam 1e-8; LAMB 1e-6); beta1 / beta2: Adam and LAMB
        # lars_skip: predicate on a parameter, True = no trust ratio for it under lars / lamb (default: ndim <= 1)
        # accum_steps N: a call runs N micro-batches, sums their gradients (parallel/bsp.py begin_micro /
        # accumulate) and applies ONE update: an effective batch of N times the micro-batch on the same memory
        # mix: an ops.mix.MixConfig - every micro-batch is mixed with a permutation of itself (mixup / CutMix) into
        # a buffer this step owns and the loss takes both labels; the plan of micro-batch i of step s is
        # sample_plan(mix, rank, s, i, ...).  None: nothing is constructed, today's launches and bits.
        # rank: the rank the plans are drawn for (default: the process group's)
        # distill: a DistillConfig - its frozen teacher runs (no grad, inference mode) on every micro-batch the
        # student sees, mixed ones included, and the main head's loss takes its logits (ops.nn.Distill).  The teacher
        # belongs to nothing below: not the optimizer's tables, the buckets, the BN sync or the EMA rows.  None:
        # nothing is constructed, today's launches and bits.
        # prune: an ops.prune.PruneConfig - gradual magnitude pruning.  After the optimizer's launch of step t (=
        # global_step at entry) the masks are re-selected when prune.updates_at(t), on the updated weights with the
        # masks so far applied (so a mask only shrinks), and on every step the masks are applied to the weights,
        # their bf16 copies and EMA shadows, before the dgrad copies are re-derived.  Neither pass looks at the skip
        # flag.  None: nothing is constructed, today's launches and bits.
        # grad_compress: an ops.compress.GradCompress - top-k sparsification of the gradient exchange with error
        # feedback (parallel/bsp.py): each plain bucket sends the k largest-magnitude entries of residual + gradient.
        # The NaN guard, the norm pass, clipping and the optimizer read the decompressed buffer.  Whether a step sends
        # packets is a host decision (begin_step), so captured steps are refused.  None: nothing is constructed,
        # today's launches and bits.
        if grad_compress is not None and not isinstance(grad_compress, GradCompress):
            raise ValueError("grad_compress must be an ops.compress.GradCompress or None, got %r" % (grad_compress,))
        if grad_compress is not None and use_graph:
            raise ValueError("grad_compress is not combined with use_graph: the dense warm-up is a host decision per "
                             "step")
        if prune is not None and not isinstance(prune, PruneConfig):
            raise ValueError("prune must be an ops.prune.PruneConfig or None, got %r" % (prune,))
        self.prune = prune
        self.pruner = None
        # sam: an ops.sam.SamConfig - sharpness-aware minimisation.  Every micro-batch runs twice: forward and
        # backward at the weights p (the ascent pass: rank-local, no collective), the perturbation p_hat = p + e(g)
        # (SAM: e = rho*g/|g|; ASAM: scaled by p^2 element-wise), forward and backward at p_hat on the same batch with
        # the same dropout masks, then p is put back bit for bit.  The descent gradient takes the ascent gradient's
        # place in everything after (accumulate / fold, all-reduces, NaN guard, norm pass, optimizer); the BN moving
        # statistics keep the ascent forward's update.  None: nothing is constructed, today's launches and bits.
        if sam is not None and not isinstance(sam, SamConfig):
            raise ValueError("sam must be an ops.sam.SamConfig or None, got %r" % (sam,))
        if sam is not None and prune is not None:
            raise ValueError("sam and prune are not combined: the perturbation would refill masked weights")
        self.sam = sam
        self.samp = None
        self.model = model
        if distill is not None and not isinstance(distill, DistillConfig):
            raise ValueError("distill must be an engine.DistillConfig or None, got %r" % (distill,))
        self.distill = distill
        self._kl_rows = []  # per micro-batch of the last step: the device KL rows of the loss
        if distill is not None:
            if distill.teacher is model or any(m is model for m in distill.teacher.modules()) \
                    or any(m is distill.teacher for m in model.modules()):
                raise ValueError("the distillation teacher must be a network of its own, not (part of) the student")
            distill.teacher.requires_grad_(False)
            first = next(model.parameters(), None)
            if first is not None:
                distill.teacher.to(first.device)
            # its bf16 compute copies, once: no optimizer owns them, so nothing rewrites them (the process-wide
            # refresh of the dgrad copies after an update re-derives a registered copy from these same bits)
            prepare_compute_copies(distill.teacher)
        if mix is not None and not isinstance(mix, _mix.MixConfig):
            raise ValueError("mix must be an ops.mix.MixConfig or None, got %r" % (mix,))
        self.mix = mix
        self._mix_bufs = {}       # (shape, dtype, device) -> the mixed batch
        self._mix_lambda = None   # mean w_lab over the last step's plans (host)
        self.accum_steps = int(accum_steps)
        if self.accum_steps < 1:
            raise ValueError("accum_steps must be at least 1, got %r" % (accum_steps,))
        if wgrad_stream is not None:
            # conv+BN weight gradients on the side stream (ops/_lib.py side_stream; process-wide): ResNet-50
            # -4.3 % step time, Inception-v3 +3.4 % eager (its per-conv stream forks cost more host time than
            # they overlap)
            _lib.set_side_enabled(wgrad_stream)
        prepare_compute_copies(model)
        params = [p for p in model.parameters() if p.requires_grad]
        # bsp_check (or DTM_BSP_CHECK=1): assert every gradient write precedes its bucket's all-reduce (debug)
        # force_comm: issue the collectives even with one rank (tests of the RCCL path on a one-GPU box)
        self.dp = BSPDataParallel(params, bucket_mb, process_group, comm_dtype=grad_comm_dtype, overlap=overlap,
                                  check=bsp_check, names=list(model.named_parameters()), force_comm=force_comm,
                                  compress=grad_compress)
        if use_graph and self.dp.comm_on and not graph_comm:
            # a captured step holds the bucket all-reduces, the BN-statistics sync and their waits inside the graph
            # (RCCL collectives captured on the current stream, replayed every step): opt in with graph_comm=True -
            # validated bit-identical to the eager step at world 1 over RCCL
            # (tests/test_distributed.py::test_bsp_rccl_captured_step_matches_eager)
            raise ValueError("use_graph (hipGraph step capture) is only for steps without collectives unless "
                             "graph_comm=True; world size %d, force_comm %s" % (self.dp.world, bool(force_comm)))
        # BN moving statistics: one flat buffer, averaged over the replicas every step (reference
        # keeps ONE PS-resident copy that every worker updates); must precede the optimizer tables
        bufs = moving_average_buffers(model)
        self.bufsync = BufferSync(bufs, process_group, every=bn_sync_every,
                                  decays=moving_average_decays(model, bufs), force_comm=force_comm)
        # ema_buffers: whether the statistics also get EMA shadows (slim BN lists them in
        # moving_average_variables(); tf.layers BN - the CIFAR ResNet preset - does not)
        self.opt = FusedOptimizer(params, optimizer, lr, momentum, rho, epsilon, ema_decay, weight_decay,
                                  ema_buffers=moving_average_buffers(model)
                                  if (ema_decay is not None and ema_buffers) else (),
                                  lars_eeta=lars_eeta, lars_epsilon=lars_epsilon, clip_global_norm=clip_global_norm,
                                  beta1=beta1, beta2=beta2, lars_skip=lars_skip)
        if prune is not None:
            pruned = [(name, p) for name, p in model.named_parameters() if p.requires_grad and prune.selects(name, p)]
            self.pruner = _prune.Pruner([(name, p.data, getattr(p, "bf16", None), self.opt.state[p].get("ema"))
                                         for name, p in pruned])
            self.pruner.params = [p for _name, p in pruned]  # for the checkpoint's <scope>/mask, <scope>/threshold
        if sam is not None:
            # after BufferSync (it may re-home the statistics into one flat buffer) and the optimizer: the tables
            # hold raw pointers of the weights, their flat-buffer gradients, the bf16 copies and the statistics
            self.samp = _sam.SamPerturber([(p.data, p.main_grad, getattr(p, "bf16", None)) for p in params],
                                          moving_average_buffers(model), config=sam)
        if rank is None:
            import torch.distributed as dist
            rank = dist.get_rank(process_group) if dist.is_available() and dist.is_initialized() else 0
        self.rank = int(rank)
        self.lr = lr
        self.lr_schedule = lr_schedule
        self.smoothing = label_smoothing
        self.aux_weight = aux_weight
        self.batch_weight = batch_weight
        self.global_step = 0
        self.use_graph = use_graph
        self.nan_guard = nan_guard
        self.last_skip = None   # device int32 flag of the last step (1 = non-finite grads, update skipped)
        self.skipped = 0        # host count, updated by poll_skipped()
        self.timer = timer      # utils.metrics.StepTimer for fwd/bwd/allreduce/optimizer HIP-event sections
        self._graph = None
        self._eager_steps = 0
        self._skip_total = None  # device int32: number of skipped (non-finite) steps so far
        self._skip_seen = 0
        self.on_backward = None  # optional callable run right before loss.backward() (tools/ab_step.py 'hog')
        if self.dp.world > 1 and params and params[0].is_cuda:
            _lib.set_reserved_cus(reserved_cus_default())

    def loss_fn(self, out, labels, plan=None, teacher_logits=None):
        aux = None
        if isinstance(out, tuple):
            out, aux = out
        bw = self.batch_weight
        heads = [(out, bw)] + ([(aux, self.aux_weight * bw)] if aux is not None and self.aux_weight else [])
        if teacher_logits is not None:
            loss = F.mean_xent_loss(heads, labels, self.smoothing, mix=plan, distill=F.Distill(
                teacher_logits, self.distill.alpha, self.distill.temperature))
            self._kl_rows.append(F.mean_xent_loss.kl_rows)
            return loss
        if plan is None:
            return F.mean_xent_loss(heads, labels, self.smoothing)
        return F.mean_xent_loss(heads, labels, self.smoothing, mix=plan)

    # ---- knowledge distillation --------------------------------------------------------------
    def _teacher_logits(self, images):
        """The frozen teacher's main-head logits on the batch the student is about to see."""
        with torch.no_grad():
            out = self.distill.teacher(images, training=False)
        return out[0] if isinstance(out, tuple) else out

    def last_distill_kl(self):
        """Mean over the last step's rows (all its micro-batches) of KL(teacher || student) at the temperature,
        unweighted.  Reads the device: call on logged steps only.  None without distillation or before the first
        step."""
        if not self._kl_rows:
            return None
        return float(torch.cat([k.detach().float().reshape(-1) for k in self._kl_rows]).mean())

    # ---- mixup / CutMix (ops/mix.py) ---------------------------------------------------------
    def _draw_plans(self, images):
        """The host plans of this step's micro-batches (a pure function of the config, the rank, the step count
        and the micro-batch index) and their mean label weight."""
        micro = images if isinstance(images, (list, tuple)) else [images]
        for x in micro:
            if x.dim() != 4:
                raise ValueError("mix needs [B, H, W, C] image batches, got shape %r" % (tuple(x.shape),))
        plans = [_mix.sample_plan(self.mix, self.rank, self.global_step, i, x.shape[0], x.shape[1], x.shape[2])
                 for i, x in enumerate(micro)]
        self._mix_lambda = float(sum(float(p.w_lab.sum(dtype="float64")) for p in plans) / sum(p.B for p in plans))
        return plans

    def _mixed(self, images, plan):
        """``images`` mixed under ``plan`` into the step's own buffer of that shape (never the caller's tensor:
        the synthetic pipelines hand the same batch in for ever)."""
        key = (tuple(images.shape), images.dtype, images.device)
        buf = self._mix_bufs.get(key)
        if buf is None:
            buf = self._mix_bufs[key] = torch.empty_like(images, memory_format=torch.contiguous_format)
        return _mix.mix_images(images.contiguous(), plan, out=buf)

    def last_mix_lambda(self):
        """Mean w_lab (the weight of a row's own label) over the last step's plans; a host value, nothing is read
        from the device.  None without mixing or before the first step."""
        return self._mix_lambda

    def current_lr(self):
        if self.lr_schedule is not None:
            return float(self.lr_schedule(self.global_step))
        return self.lr

    def _mark(self, name):
        if self.timer is not None:
            self.timer.mark(name)

    def _micro_batches(self, images, labels):
        """The step's ``accum_steps`` micro-batches as (list of images, list of labels): each argument is a list /
        tuple of that length, or one tensor split into equal contiguous views along the leading dimension."""
        n = self.accum_steps
        out = []
        for name, v in (("images", images), ("labels", labels)):
            if isinstance(v, (list, tuple)):
                if len(v) != n:
                    raise ValueError("%s: %d micro-batches given, accum_steps is %d" % (name, len(v), n))
                out.append(list(v))
            else:
                if v.shape[0] % n:
                    raise ValueError("%s: leading dimension %d is not divisible by accum_steps %d"
                                     % (name, v.shape[0], n))
                b = v.shape[0] // n
                out.append([v[i * b:(i + 1) * b] for i in range(n)])
        return out[0], out[1]

    def _forward_loss(self, images, labels, plan, tz):
        """Training-mode forward and loss of one micro-batch (``plan``: its MixPlan or None; ``tz``: the teacher's
        logits or None)."""
        with roctx("forward"):
            out = self.model(images, training=True)
        with roctx("loss"):
            if tz is not None:
                return self.loss_fn(out, labels, plan, tz)
            return self.loss_fn(out, labels) if plan is None else self.loss_fn(out, labels, plan)

    def last_sam_norm(self):
        """The ascent gradient's norm sqrt(S) of the last micro-batch (ops/sam.py; ASAM: of |p|*g).  Reads the
        device: call on logged steps only.  None without SAM."""
        if self.samp is None:
            return None
        return float(self.samp.last_norm())

    def _forward_backward(self, images, labels, plans=None):
        """One batch (two tensors), or the micro-batches of one step (two lists of tensors): micro-batches
        0 .. n-2 end in the accumulate launch, the last one folds and reduces.  ``plans`` (mixing only): one
        MixPlan per micro-batch with its record on the device (the captured step's static ones); None: drawn
        here and copied to the device."""
        if self.mix is not None and plans is None:
            plans = [p.to(x.device) for p, x in zip(self._draw_plans(images),
                                                    images if isinstance(images, (list, tuple)) else [images])]
        micro = list(zip(images, labels)) if isinstance(images, (list, tuple)) else [(images, labels)]
        n = len(micro)
        if self.dp.compress is not None:
            self.dp.steps = self.global_step  # begin_step counts global steps (a resumed run included)
        losses = []
        if self.distill is not None:
            self._kl_rows = []
        for i, (images, labels) in enumerate(micro):
            last = i == n - 1
            self.dp.begin_micro(i, n)
            if i == 0:
                self._mark("start")
            if images.is_cuda:
                _fused.arena.begin_step(images.device)
                _elementwise.advance_seed_offset(images.device)  # fresh dropout masks, replay included
            perturbed = False
            try:
                if plans is not None:
                    with roctx("mix"):
                        images = self._mixed(images, plans[i])
                tz = None
                if self.distill is not None:
                    with roctx("teacher"):
                        tz = self._teacher_logits(images)
                plan = plans[i] if plans is not None else None
                if self.samp is not None:
                    # SAM (ops/sam.py): the ascent pass at p on this rank's micro-batch (no collective), the
                    # perturbation (which also clears the flat buffer), then the descent pass below at p_hat with the
                    # same dropout masks; the BN statistics keep the ascent forward's update
                    seed = _elementwise._seed[0]
                    self.dp.begin_ascent()
                    with roctx("sam_ascent"):
                        loss_a = self._forward_loss(images, labels, plan, tz)
                        if last:
                            self.bufsync.issue()  # the statistics are final: the sync runs under both backwards
                        else:
                            self.bufsync.local_update()
                        loss_a.backward()
                        if images.is_cuda:
                            _lib.side_join()
                    self.dp.end_ascent()
                    _fused.arena.end_step()
                    with roctx("sam_perturb"):
                        self.samp.perturb()  # (launches everything or, for a bad argument, nothing)
                        perturbed = True
                        if self.opt._dev is not None:
                            F.refresh_flipped()
                    _elementwise._seed[0] = seed
                    if images.is_cuda:
                        _fused.arena.begin_step(images.device)
                    kl = len(self._kl_rows)
                    loss = self._forward_loss(images, labels, plan, tz)
                    del self._kl_rows[kl:]  # the reported loss and KL rows are the ascent pass's: taken at p
                    if last:
                        self._mark("fwd")
                else:
                    loss = self._forward_loss(images, labels, plan, tz)
                    if last:
                        self._mark("fwd")
                        self.bufsync.issue()  # forward has finished every moving-statistics update
                    else:
                        self.bufsync.local_update()  # one more local update for the last micro-batch's sync to cover
                if self.on_backward is not None:
                    self.on_backward()
                with roctx("backward"):  # bucket all-reduces are issued (own ranges) from the grad hooks
                    loss.backward()
                if images.is_cuda:
                    _lib.side_join()  # weight gradients enqueued on the side stream (ops/_lib.py)
                if perturbed:
                    with roctx("sam_restore"):
                        perturbed = False
                        self.samp.restore()  # p, the bf16 copies and the BN statistics of the ascent pass, bit for bit
                    loss = loss_a
                if last:
                    self._mark("bwd")
            except BaseException:
                self.dp.end_ascent()
                if perturbed:
                    self.samp.restore()
                self.bufsync.abort()  # the live BN statistics stay this replica's own (never a partial sum)
                raise
            finally:
                _fused.arena.end_step()
            losses.append(loss.detach())
            if not last:
                self.dp.accumulate(i)
        loss = losses[0]
        if n > 1:  # fp32 mean of the micro-batch losses, summed in micro-batch order
            for v in losses[1:]:
                loss = loss + v
            loss = loss / n
        with roctx("allreduce_wait"):
            self.dp.finish()
            self.bufsync.finish()
        self._mark("allreduce")
        skip = None
        if self.nan_guard:
            # NaN/Inf guard on the reduced gradient: identical on every rank after the all-reduce,
            # so all replicas skip the same update
            flat = self.dp.flat
            if flat.is_cuda:
                skip = torch.zeros(1, device=flat.device, dtype=torch.int32)
                with roctx("nan_guard"):
                    _lib.lib().dtm_check_finite(_lib.ptr(flat), flat.numel(), _lib.ptr(skip), _lib.stream_ptr())
            else:
                skip = torch.tensor([0 if bool(torch.isfinite(flat).all()) else 1], dtype=torch.int32)
            self.last_skip = skip
            if self._skip_total is None:
                self._skip_total = torch.zeros(1, device=flat.device, dtype=torch.int32)
            self._skip_total.add_(skip)  # sticky device count: read on log steps only, no per-step sync
        return loss.detach(), skip

    def __call__(self, images, labels):
        """One optimizer step.  With ``accum_steps`` N > 1 each argument is a list / tuple of N micro-batches, or
        one tensor whose leading dimension N divides (split into equal contiguous views): the gradients of the N
        micro-batches are summed and applied once; the returned loss is the mean of their losses."""
        if self.accum_steps > 1:
            images, labels = self._micro_batches(images, labels)
        if self.use_graph and (images[0] if self.accum_steps > 1 else images).is_cuda:
            return self._graph_step(images, labels)
        return self._eager_step(images, labels)

    def nonfinite_micro(self):
        """Per micro-batch of the last step, 1 where its gradients held an Inf or a NaN (this rank's own: the
        flags are set before the all-reduce).  Reads the device: call on logged steps only."""
        if self.accum_steps == 1 or self.dp.micro_flags is None:
            return [0] * self.accum_steps
        return [int(v) for v in self.dp.micro_flags.tolist()]

    # ---- gradual magnitude pruning (ops/prune.py) -----------------------------------------------
    def _prune_stage(self):
        t = self.global_step
        self.pruner.stage(self.prune.sparsity_at(t), self.prune.updates_at(t))

    def last_sparsity(self):
        """(achieved, target): the achieved sparsity (sum n - sum kept) / sum n over the pruned tensors and the
        schedule's value at the last step.  Reads the device: call on logged steps only.  None without pruning."""
        if self.pruner is None:
            return None
        return self.pruner.sparsity(), self.prune.sparsity_at(max(self.global_step - 1, 0))

    def _eager_step(self, images, labels):
        rng = range_push("train_step")
        loss, skip = self._forward_backward(images, labels)
        with roctx("optimizer"):
            if self.pruner is None:
                self.opt.step(self.current_lr(), grad_scale=self.dp.grad_scale, skip_flag=skip)
            else:
                self.opt.step(self.current_lr(), grad_scale=self.dp.grad_scale, skip_flag=skip, refresh=False)
                self._prune_stage()
                self.pruner.launch()
                if self.opt._dev is not None:
                    F.refresh_flipped()
        self._mark("optimizer")
        self.global_step += 1
        range_pop(rng)
        return loss

    # ---- hipGraph path -----------------------------------------------------------------------
    # The whole step (zero-grad memset, forward, backward with its hook-issued bucket all-reduces,
    # NaN guard, fused optimizer, dgrad weight-copy refresh) is captured once into a hipGraph and
    # replayed: one host submission per step instead of ~600 kernel launches, so launch-bound
    # models (LeNet, CIFAR nets, small batches) stop being host-bound.  Per-step scalars (lr, EMA
    # decay, 1/W) live in a device buffer staged before every replay (FusedOptimizer.set_dynamic);
    # host counters (global_step, EMA num_updates) advance outside the graph.  The first
    # ``graph_warmup`` steps run eagerly so every lazily grown workspace, the zero-arena high-water
    # mark and the weight-flip table exist before capture (no allocation inside the graph).
    graph_warmup = 2

    def _graph_step(self, images, labels):
        if self._graph is None and self._eager_steps < self.graph_warmup:
            self._eager_steps += 1
            self.use_graph = False
            try:
                return self(images, labels)
            finally:
                self.use_graph = True
        if self._graph is None:
            # (with accum_steps > 1: one static copy per micro-batch, all of them inside the one graph)
            self._static_x = _map_batches(torch.Tensor.clone, images)
            self._static_y = _map_batches(torch.Tensor.clone, labels)
            # mixing: one static record per micro-batch; the captured mix kernel and loss read it, and the kind of
            # mixing is data in it (no host decision lives inside the capture)
            self._static_plans = None
            if self.mix is not None:
                self._static_plans = [p.to(x.device) for p, x in zip(
                    self._draw_plans(images), images if isinstance(images, list) else [images])]
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            timer, self.timer = self.timer, None  # no event records inside the capture
            try:
                with torch.cuda.graph(g):
                    loss, skip = self._forward_backward(self._static_x, self._static_y, self._static_plans)
                    self.opt.launch(skip)
                    if self.pruner is not None:  # what it does is data in its device record, staged per replay
                        self.pruner.launch()
                    from .ops.nn import refresh_flipped
                    refresh_flipped()
            finally:
                self.timer = timer
            self._graph, self._static_loss = g, loss
        else:
            _map_batches(_stage, self._static_x, images)
            _map_batches(_stage, self._static_y, labels)
            if self.mix is not None:
                # a fresh pinned tensor per plan: torch's host allocator recycles it only after the copy's stream
                # event, so the next step's records never overwrite one whose copy has not run
                for static, plan in zip(self._static_plans, self._draw_plans(images)):
                    static.dev.copy_(plan.host_tensor(pin=True), non_blocking=True)
        self.opt.set_dynamic(self.current_lr(), self.dp.grad_scale)
        if self.pruner is not None:
            self._prune_stage()
        self._graph.replay()
        self.opt.num_updates += 1
        self.global_step += 1
        return self._static_loss.clone()

    def poll_skipped(self):
        """Host-side check (one small sync; call on log steps): True if any step since the last poll
        had non-finite gradients and skipped its update.  ``self.skipped`` = total so far."""
        if self._skip_total is None:
            return False
        n = int(self._skip_total.item())
        new = n - self._skip_seen
        self._skip_seen = n
        self.skipped = n
        return new > 0
