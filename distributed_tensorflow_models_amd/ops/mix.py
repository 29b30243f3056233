"""Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019): a host sampler, one device record per batch, and the image
mixing kernel (csrc/kernels/mix.hip).

A batch is mixed with a permutation of itself.  What happens to row ``r`` is one 32-byte record, int32[8]:

    [partner, bits(w_pix), bits(w_lab), y0, y1, x0, x1, 0]          (the weights are float32 bit patterns)

  mixup      w_pix = w_lab = float32(lam), an empty box (y0 == y1): out = w_pix * x[r] + (1 - w_pix) * x[partner]
  CutMix     w_pix = 1 and a box: out = x[r] with x[partner] pasted into [y0, y1) x [x0, x1);
             w_lab = 1 - (box area) / (H * W), from the box as clipped by the image border
  identity   partner = r, both weights 1, an empty box

``w_lab`` weighs the row's own label in the loss (ops/nn.py mean_xent_loss(..., mix=plan)), ``1 - w_lab`` the
partner's.  The kind of mixing is data in the record, so a captured step replays whatever the step's record holds.

``sample_plan`` is a pure function of (config, rank, step, micro-batch, shape): a resumed run, an eager run and a
captured run draw the same plans; ranks and micro-batches draw different ones.

On CPU tensors ``mix_images`` runs the same definition as torch ops: the CPU path of the feature and the kernel's
oracle (bit for bit: each product and the sum are rounded separately, then cast to the storage type).
"""
import numpy as np
import torch

from . import _lib

REC_WORDS = 8


class MixConfig:
    """mixup_alpha / cutmix_alpha: the Beta(alpha, alpha) parameter of each kind (0 = that kind is off; both 0 is
    invalid - "no mixing" is ``mix=None``); prob: the probability that a batch (a row with per_row) is mixed at all;
    switch_prob: with both kinds on, the probability of CutMix; per_row: draw per row instead of per batch."""

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, per_row=False, seed=0):
        self.mixup_alpha = float(mixup_alpha)
        self.cutmix_alpha = float(cutmix_alpha)
        self.prob = float(prob)
        self.switch_prob = float(switch_prob)
        self.per_row = bool(per_row)
        self.seed = int(seed)
        if not (self.mixup_alpha >= 0.0 and self.cutmix_alpha >= 0.0):
            raise ValueError("mixup_alpha and cutmix_alpha must not be negative, got %r and %r"
                             % (mixup_alpha, cutmix_alpha))
        if self.mixup_alpha == 0.0 and self.cutmix_alpha == 0.0:
            raise ValueError("mixup_alpha and cutmix_alpha are both 0: pass mix=None for no mixing")
        for name, v in (("prob", self.prob), ("switch_prob", self.switch_prob)):
            if not 0.0 <= v <= 1.0:
                raise ValueError("%s must lie in [0, 1], got %r" % (name, v))
        if self.seed < 0:
            raise ValueError("seed must not be negative, got %r" % (seed,))

    def __repr__(self):
        return ("MixConfig(mixup_alpha=%g, cutmix_alpha=%g, prob=%g, switch_prob=%g, per_row=%s, seed=%d)"
                % (self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob, self.per_row, self.seed))


class MixPlan:
    """The records of one batch: ``rec`` the host copy (numpy int32[B, 8]), ``dev`` the same rows as a tensor on
    the device the batch lives on (None until ``to``), ``H`` x ``W`` the image size the boxes refer to."""

    def __init__(self, rec, H, W, dev=None):
        rec = np.ascontiguousarray(rec, dtype=np.int32)
        if rec.ndim != 2 or rec.shape[1] != REC_WORDS:
            raise ValueError("a mixing plan is an int32[B, %d] array, got shape %r" % (REC_WORDS, rec.shape))
        self.rec, self.H, self.W, self.dev = rec, int(H), int(W), dev
        self._checked = False

    @property
    def B(self):
        return self.rec.shape[0]

    @property
    def partner(self):
        return self.rec[:, 0]

    @property
    def w_pix(self):
        return self.rec[:, 1].view(np.float32)

    @property
    def w_lab(self):
        return self.rec[:, 2].view(np.float32)

    @property
    def box(self):
        """int32[B, 4]: y0, y1, x0, x1"""
        return self.rec[:, 3:7]

    def kinds(self):
        """Per row: 'cutmix' (a non-empty box), 'mixup' (w_pix != 1), else 'identity'."""
        b = self.box
        boxed = (b[:, 1] > b[:, 0]) & (b[:, 3] > b[:, 2])
        return ["cutmix" if c else "mixup" if w != 1.0 else "identity" for c, w in zip(boxed, self.w_pix)]

    def validate(self):
        """The checks the kernels rely on, on the host copy (the kernels trust the device copy)."""
        if self._checked:
            return self
        B, b = self.B, self.box
        if B < 1:
            raise ValueError("an empty mixing plan")
        if not ((self.partner >= 0) & (self.partner < B)).all():
            raise ValueError("mixing plan: partner outside [0, %d)" % B)
        if not ((0 <= b[:, 0]) & (b[:, 0] <= b[:, 1]) & (b[:, 1] <= self.H)).all():
            raise ValueError("mixing plan: box rows violate 0 <= y0 <= y1 <= %d" % self.H)
        if not ((0 <= b[:, 2]) & (b[:, 2] <= b[:, 3]) & (b[:, 3] <= self.W)).all():
            raise ValueError("mixing plan: box columns violate 0 <= x0 <= x1 <= %d" % self.W)
        for name, w in (("w_pix", self.w_pix), ("w_lab", self.w_lab)):
            if not ((w >= 0.0) & (w <= 1.0)).all():  # (a NaN fails both comparisons)
                raise ValueError("mixing plan: %s outside [0, 1]" % name)
        self._checked = True
        return self

    def host_tensor(self, pin=False):
        """The records as a fresh CPU tensor (a copy: the plan may be dropped before an asynchronous copy of it has
        run).  pin: page-locked, from torch's host allocator, which recycles the block only after the stream
        event of the copy that read it."""
        t = torch.from_numpy(self.rec.copy())
        return t.pin_memory() if pin else t

    def to(self, device):
        """A MixPlan with the same host records and ``dev`` on ``device`` (copied asynchronously on the current
        stream from a fresh pinned tensor)."""
        device = torch.device(device)
        if device.type == "cuda":
            dev = torch.empty(self.rec.shape, dtype=torch.int32, device=device)
            dev.copy_(self.host_tensor(pin=True), non_blocking=True)
        else:
            dev = self.host_tensor()
        p = MixPlan(self.rec, self.H, self.W, dev)
        p._checked = self._checked
        return p


def make_plan(partner, w_pix, w_lab, box, H, W):
    """A plan from per-row arrays: partner int[B], w_pix / w_lab float[B], box int[B, 4] = (y0, y1, x0, x1)."""
    partner = np.asarray(partner, dtype=np.int64).reshape(-1)
    B = partner.shape[0]
    rec = np.zeros((B, REC_WORDS), dtype=np.int32)
    rec[:, 0] = partner
    rec[:, 1] = np.asarray(w_pix, dtype=np.float32).reshape(B).view(np.int32)
    rec[:, 2] = np.asarray(w_lab, dtype=np.float32).reshape(B).view(np.int32)
    rec[:, 3:7] = np.asarray(box, dtype=np.int64).reshape(B, 4)
    return MixPlan(rec, H, W)


def identity_plan(B, H, W):
    z = np.zeros((B, 4), dtype=np.int64)
    return make_plan(np.arange(B), np.ones(B, np.float32), np.ones(B, np.float32), z, H, W)


def _cutmix_box(lam, cy, cx, H, W):
    """The paper's box for lam (scalars or arrays): side ratio sqrt(1 - lam) around (cy, cx), clipped by the image;
    returns (y0, y1, x0, x1, w_lab) with w_lab recomputed from the clipped box."""
    rat = np.sqrt(1.0 - lam)
    ch, cw = (H * rat).astype(np.int64), (W * rat).astype(np.int64)
    y0, y1 = np.maximum(cy - ch // 2, 0), np.minimum(cy + ch // 2, H)
    x0, x1 = np.maximum(cx - cw // 2, 0), np.minimum(cx + cw // 2, W)
    w_lab = 1.0 - (y1 - y0) * (x1 - x0) / float(H * W)
    return y0, y1, x0, x1, w_lab


def sample_plan(cfg, rank, step, micro, B, H, W):
    """The plan of micro-batch ``micro`` of step ``step`` on rank ``rank``: a pure function of its arguments, drawn
    from ``numpy.random.default_rng([cfg.seed, rank, step, micro])``.

    Batch-wise rule (per_row=False), in this order:
      1. u_apply = rng.random()
      2. u_switch = rng.random()
      3. partner = rng.permutation(B)                      (fixed points are allowed)
      4. u_apply >= prob: the identity plan
      5. CutMix if cutmix_alpha > 0 and (mixup_alpha <= 0 or u_switch < switch_prob), else mixup
      6. lam = rng.beta(a, a) with the chosen alpha
      7. CutMix only: cy = rng.integers(H), cx = rng.integers(W)
    Per-row rule (per_row=True), every draw an array of B in this order (a draw is skipped where its alpha is 0):
      1. u_apply = rng.random(B)
      2. u_switch = rng.random(B)
      3. partner = rng.permutation(B)                      (one permutation for the batch)
      4. lam_mixup = rng.beta(mixup_alpha, mixup_alpha, B)          if mixup_alpha > 0
      5. lam_cutmix = rng.beta(cutmix_alpha, cutmix_alpha, B)       if cutmix_alpha > 0
      6. cy = rng.integers(H, size=B), cx = rng.integers(W, size=B) if cutmix_alpha > 0
    and row r is the identity where u_apply[r] >= prob, else CutMix or mixup by rule 5 with u_switch[r].  Every draw
    is made whatever the other draws say, so one row's kind does not move another row's numbers."""
    rank, step, micro, B, H, W = int(rank), int(step), int(micro), int(B), int(H), int(W)
    if min(rank, step, micro) < 0 or min(B, H, W) < 1:
        raise ValueError("sample_plan: rank, step, micro must be >= 0 and B, H, W >= 1")
    rng = np.random.default_rng([cfg.seed, rank, step, micro])
    one = np.ones(B, np.float32)
    if not cfg.per_row:
        u_apply = rng.random()
        u_switch = rng.random()
        partner = rng.permutation(B)
        if u_apply >= cfg.prob:
            return identity_plan(B, H, W).validate()
        cut = cfg.cutmix_alpha > 0 and (cfg.mixup_alpha <= 0 or u_switch < cfg.switch_prob)
        a = cfg.cutmix_alpha if cut else cfg.mixup_alpha
        lam = rng.beta(a, a)
        if not cut:
            w = one * np.float32(lam)
            return make_plan(partner, w, w, np.zeros((B, 4), np.int64), H, W).validate()
        cy, cx = rng.integers(H), rng.integers(W)
        y0, y1, x0, x1, w_lab = _cutmix_box(np.float64(lam), np.int64(cy), np.int64(cx), H, W)
        box = np.tile(np.array([y0, y1, x0, x1], dtype=np.int64), (B, 1))
        return make_plan(partner, one, one * np.float32(w_lab), box, H, W).validate()
    u_apply = rng.random(B)
    u_switch = rng.random(B)
    partner = rng.permutation(B)
    lam_m = rng.beta(cfg.mixup_alpha, cfg.mixup_alpha, B) if cfg.mixup_alpha > 0 else None
    lam_c = rng.beta(cfg.cutmix_alpha, cfg.cutmix_alpha, B) if cfg.cutmix_alpha > 0 else None
    w_pix, w_lab, box = one.copy(), one.copy(), np.zeros((B, 4), np.int64)
    apply = u_apply < cfg.prob
    cut = apply & (cfg.cutmix_alpha > 0) & ((cfg.mixup_alpha <= 0) | (u_switch < cfg.switch_prob))
    mup = apply & ~cut
    if lam_c is not None:
        cy, cx = rng.integers(H, size=B), rng.integers(W, size=B)
        y0, y1, x0, x1, wl = _cutmix_box(lam_c, cy, cx, H, W)
        box[cut] = np.stack([y0, y1, x0, x1], axis=1)[cut]
        w_lab[cut] = wl.astype(np.float32)[cut]
    if lam_m is not None:
        w_pix[mup] = lam_m.astype(np.float32)[mup]
        w_lab[mup] = w_pix[mup]
    partner = np.where(apply, partner, np.arange(B))
    return make_plan(partner, w_pix, w_lab, box, H, W).validate()


def _check_images(x, plan, out):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("mix_images needs a [B, H, W, C] bf16 or fp32 tensor, got %s %s"
                         % (getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
    if not x.is_contiguous() or x.numel() == 0:
        raise ValueError("mix_images needs a contiguous, non-empty NHWC batch")
    B, H, W, _C = x.shape
    if plan.B != B or plan.H != H or plan.W != W:
        raise ValueError("mixing plan for B, H, W = %d, %d, %d used on a batch of %d, %d, %d"
                         % (plan.B, plan.H, plan.W, B, H, W))
    plan.validate()
    if out is not None:
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise ValueError("mix_images: out must match x in shape, dtype, device and be contiguous")
        nbytes = x.numel() * x.element_size()
        if x.data_ptr() < out.data_ptr() + nbytes and out.data_ptr() < x.data_ptr() + nbytes:
            # partners are read after other rows have been written: in place is not defined
            raise ValueError("mix_images: out overlaps x")


def _mix_images_torch(x, plan):
    B, H, W, _C = x.shape
    idx = torch.from_numpy(plan.partner.astype(np.int64)).to(x.device)
    w = torch.from_numpy(plan.w_pix.copy()).to(x.device).view(B, 1, 1, 1)
    box = torch.from_numpy(plan.box.astype(np.int64)).to(x.device)
    b = x[idx]
    # three roundings in fp32 (no fused multiply-add: each torch op rounds its own result), then the storage type
    blend = ((w * x.float()) + ((1.0 - w) * b.float())).to(x.dtype)
    ys = torch.arange(H, device=x.device).view(1, H, 1, 1)
    xs = torch.arange(W, device=x.device).view(1, 1, W, 1)
    y0, y1, x0, x1 = (box[:, k].view(B, 1, 1, 1) for k in range(4))
    inside = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
    return torch.where(inside, b, torch.where(w == 1.0, x, blend))  # the two copies are bit copies


@torch.no_grad()
def mix_images(x, plan, out=None):
    """The mixed batch of ``x`` ([B, H, W, C], bf16 or fp32, contiguous; may start at any element of a larger
    buffer) under ``plan``, into ``out`` (not overlapping x) or a new tensor.  One launch on the current stream."""
    _check_images(x, plan, out)
    if not x.is_cuda:
        res = _mix_images_torch(x, plan)
        if out is None:
            return res
        out.copy_(res)
        return out
    if plan.dev is None or plan.dev.device != x.device:
        raise ValueError("mix_images: the plan has no record on %s (plan.to(device))" % x.device)
    if out is None:
        out = torch.empty_like(x)
    B, H, W, C = x.shape
    rc = _lib.lib().dtm_mix_images(_lib.ptr(x), _lib.ptr(out), _lib.ptr(plan.dev), B, H, W, C,
                                   int(x.dtype == torch.bfloat16), _lib.stream_ptr())
    if rc != 0:
        raise RuntimeError("dtm_mix_images failed (%d)" % rc)
    return out
