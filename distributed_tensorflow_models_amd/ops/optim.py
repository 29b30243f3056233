"""Fused multi-tensor optimizers (one HIP launch per step for every parameter).

TF 1.x update semantics:
  GradientDescentOptimizer  p -= lr*g                                  (C20)
  MomentumOptimizer         a = mu*a + g; p -= lr*a   (use_nesterov=False)  (C20b)
  RMSPropOptimizer          ms = rho*ms + (1-rho)g^2 (ms init 1.0); mom = mu*mom + lr*g/sqrt(ms+eps);
                            p -= mom                                       (C21)
  LARS (You, Gitman, Ginsburg 2017, in the form of TF 1.x's contrib optimizer): the Momentum update with the
                            rate lr*lr_scale[t]:  a = mu*a + g; p -= lr*lr_scale[t]*a, where
                            lr_scale[t] = eeta*|p| / (|gs| + wd_t*|p| + eps)  for an adapted tensor with |p| > 0
                            and |gs| > 0 (gs = grad*grad_scale), 1 otherwise; tensors with ndim <= 1 (biases, BN
                            beta / gamma) are not adapted
  AdamOptimizer             m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
                            p -= lr * sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
                            (eps outside the root and not bias-corrected; no Nesterov, no AMSGrad; m, v start at 0).
                            t = the number of updates actually APPLIED, this one included: an update that the NaN
                            guard skips on the device does not count, so t lives in a small device record that a
                            one-thread launch advances in front of the update (also inside a replayed hipGraph); the
                            host reads it only in ``adam_step()``.  Weight decay stays the coupled L2 term (no AdamW).
  LAMB (You et al. 2020)    gs = grad*grad_scale;  m = b1*m + (1-b1)*gs;  v = b2*v + (1-b2)*gs*gs;
                            r = (m / (1-b1^t)) / (sqrt(v) / sqrt(1-b2^t) + eps) + wd_t*p;
                            phi[t] = |p| / |r| for an adapted tensor with |p| > 0 and |r| > 0, 1 otherwise (no clamp);
                            p -= lr*lr_mult[t]*phi[t] * r
                            (eps outside the root, added to the bias-corrected sqrt(v): the paper's and TensorFlow
                            Addons' form; t and the slots are Adam's).  The weight decay is DECOUPLED for this kind:
                            wd_t*p enters r only, never gs, m or v - the same ``weight_decay`` number that is the
                            coupled L2 term under every other kind.  |r| depends on the moments after this step's
                            gradient, so the kind has a pass of its own: state advance, moments + per-chunk fp64
                            records, per-tensor finalize, apply (four launches, no host decision in between).
  g = grad*grad_scale + weight_decay*p   (coupled L2 = d/dp of wd*sum(p^2)/2; K14; every kind but LAMB)
  clip_global_norm (tf.clip_by_global_norm): g *= clip / max(sqrt(sum over all tensors of |g|^2), clip); the L2
                            term is part of g because the reference puts it in the loss
  optional ExponentialMovingAverage shadows: ema -= (1-d)(ema - p), d = min(decay,(1+n)/(10+n)) (C22)
and a bf16 copy-out of every updated weight (the compute copy read by the conv kernels).

The norms LARS and clipping need come from one two-launch multi-tensor pass on the device (fp64 sums in a fixed
order: bit-identical on every rank), enqueued before the update; the host never waits for them.  LAMB's norms (|p|,
|r|, |gs|) come out of its own pass in the same fixed order.

On CPU the same math runs as torch ops (gloo plumbing tests, reference checks).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._tables import chunk_rows, to_device_bytes

# kernel update rule per kind (LARS is the momentum rule with a per-tensor rate factor; Adam and LAMB have entry
# points of their own)
KINDS = {"sgd": 0, "momentum": 1, "rmsprop": 2, "lars": 1, "adam": 3, "lamb": 4}
ADAM_LIKE = ("adam", "lamb")  # m, v slots at the weight's offset and the device record of applied updates


def _bias_corrections(b1, b2, t):
    """(1 - b1^t, sqrt(1 - b2^t)) from t in fp64, rounded once to fp32: what the device record holds."""
    return np.float32(1.0 - b1 ** t), np.float32(math.sqrt(1.0 - b2 ** t))


def _slot_like(p, fill=0.0):
    """An fp32 slot for ``p`` that sits at p's own offset from a 16-byte boundary, so that the Adam kernel's 16-byte
    path depends on the weight and its gradient alone (a fresh allocation is aligned; a weight that is a view may not
    be)."""
    off = (p.data_ptr() % 16) // 4 if p.is_cuda else 0
    if off == 0:
        return torch.full_like(p, fill, dtype=torch.float32)
    buf = torch.full((p.numel() + off,), fill, dtype=torch.float32, device=p.device)
    return buf[off:].view(p.shape)


class FusedOptimizer:
    def __init__(self, params, kind="momentum", lr=0.1, momentum=0.9, rho=0.9, epsilon=None, ema_decay=None,
                 weight_decay=None, lr_mults=None, ema_buffers=(), lars_eeta=0.001, lars_epsilon=0.0,
                 clip_global_norm=None, lars_skip=None, beta1=0.9, beta2=0.999):
        """``lars_skip``: predicate on a parameter, True = its rate is not adapted (default: ``p.ndim <= 1``); it
        serves LARS and LAMB alike.  ``kind="lamb"`` with a predicate that skips every tensor is AdamW (decoupled
        decay, no trust ratio).
        ``clip_global_norm``: threshold of the clip by global norm (None or 0: off); not combined with LARS or LAMB.
        ``epsilon``: None = 1e-10 (RMSProp's), for Adam 1e-8, for LAMB 1e-6.  ``beta1`` / ``beta2``: Adam and LAMB.
        ``weight_decay`` (or ``p.weight_decay``): the coupled L2 term, except under LAMB, where it is decoupled."""
        self.params = [p for p in params if p.requires_grad]
        # non-trainable tensors that also get an EMA shadow (BN moving mean/variance: the reference
        # averages trainable_variables() + moving_average_variables(), e.g. reference
        # alexnet/cifar10_alexnet_bsp.py:79-86, inception/imagenet_inception_bsp.py:123-126)
        self.ema_buffers = [b for b in ema_buffers] if ema_decay is not None else []
        self.buffer_ema = {id(b): b.detach().clone().float() for b in self.ema_buffers}
        if kind not in KINDS:
            raise ValueError(kind)
        clip = float(clip_global_norm) if clip_global_norm else 0.0
        if clip < 0.0:
            raise ValueError("clip_global_norm must be positive, got %r" % (clip_global_norm,))
        if kind == "lars" and clip > 0.0:
            raise ValueError("LARS and clip_global_norm are not combined (the order of the two is not defined)")
        if kind == "lamb" and clip > 0.0:
            raise ValueError("LAMB and clip_global_norm are not combined (the global norm would have to leave the "
                             "decoupled decay term out, which the norm pass does not form)")
        if epsilon is None:
            epsilon = {"adam": 1e-8, "lamb": 1e-6}.get(kind, 1e-10)
        self.kind, self.lr, self.mu, self.rho, self.eps = kind, lr, momentum, rho, epsilon
        self.b1, self.b2 = float(beta1), float(beta2)
        if kind in ADAM_LIKE and not (0.0 <= self.b1 < 1.0 and 0.0 <= self.b2 < 1.0):
            raise ValueError("beta1 and beta2 must be in [0, 1), got %r, %r" % (beta1, beta2))
        if kind == "lamb" and not float(epsilon) >= 0.0:
            raise ValueError("epsilon must not be negative, got %r" % (epsilon,))
        self.lars_eeta, self.lars_eps, self.clip = float(lars_eeta), float(lars_epsilon), clip
        self.scaled = kind == "lars" or clip > 0.0  # the step needs the norm pass
        self.normed = self.scaled or kind == "lamb"  # ... or writes norms and rate factors itself
        if lars_skip is None:
            lars_skip = lambda p: p.ndim <= 1  # noqa: E731
        self.ema_decay = ema_decay
        self.num_updates = 0
        self.state = {}
        for p in self.params:
            st = {}
            if kind in ("momentum", "rmsprop", "lars"):
                st["s1"] = torch.zeros_like(p, dtype=torch.float32)
            if kind == "rmsprop":
                st["s2"] = torch.ones_like(p, dtype=torch.float32)  # TF RMSProp ms slot init 1.0
            if kind in ADAM_LIKE:
                st["s1"], st["s2"] = _slot_like(p), _slot_like(p)  # m, v
            if ema_decay is not None:
                st["ema"] = _slot_like(p).copy_(p.detach()) if kind in ADAM_LIKE else p.detach().clone().float()
            st["wd"] = float(getattr(p, "weight_decay", 0.0) if weight_decay is None else weight_decay)
            st["lr_mult"] = 1.0 if lr_mults is None else float(lr_mults.get(p, 1.0))
            st["adapt"] = kind in ("lars", "lamb") and not lars_skip(p)
            self.state[p] = st
        self._dev = None
        self._norms = self._lr_scale = self._gclip = None
        self._adam_t = 0          # CPU path: applied updates (the device path keeps them in _adam_state)
        self._adam_state = None   # device record {int32 t, fp32 1-b1^t, fp32 sqrt(1-b2^t), pad}
        self._adam_loaded = {}    # beta*_power values a checkpoint restore delivered (restored())
        if self.normed and not (self.params and self.params[0].is_cuda):
            n = len(self.params) + len(self.ema_buffers)
            self._norms = torch.zeros((n, 3), dtype=torch.float32)
            self._lr_scale = torch.ones(n, dtype=torch.float32)
            self._gclip = torch.ones(1, dtype=torch.float32)
        if self.params and self.params[0].is_cuda:
            self._build_tables()

    # ---- device tables ---------------------------------------------------------------------
    def _build_tables(self):
        L = _lib.lib()
        tb, cb, chunk = L.dtm_opt_tensor_bytes(), L.dtm_opt_chunk_bytes(), L.dtm_opt_chunk_size()
        assert tb == 64 and cb == 16, (tb, cb)
        dev = self.params[0].device
        tens = np.zeros((len(self.params), 8), dtype=np.uint64)
        self._keep = []
        for i, p in enumerate(self.params):
            st = self.state[p]
            g = self._grad_tensor(p)
            w16 = getattr(p, "bf16", None)
            if w16 is not None and (w16.dtype != torch.bfloat16 or w16.shape != p.shape):
                w16 = None
            ptrs = [p.data_ptr(), g.data_ptr(), st["s1"].data_ptr() if "s1" in st else 0,
                    st["s2"].data_ptr() if "s2" in st else 0, w16.data_ptr() if w16 is not None else 0,
                    st["ema"].data_ptr() if "ema" in st else 0]
            tens[i, :6] = ptrs
            tens[i, 6] = p.numel()
            tens[i, 7] = np.array([st["wd"], st["lr_mult"]], dtype=np.float32).view(np.uint64)[0]
        # EMA-only rows (grad pointer 0): the kernel just moves the shadow towards the buffer
        base = len(self.params)
        if self.ema_buffers:
            tens = np.concatenate([tens, np.zeros((len(self.ema_buffers), 8), dtype=np.uint64)])
        for j, b in enumerate(self.ema_buffers):
            assert b.dtype == torch.float32 and b.is_contiguous(), "EMA buffers must be contiguous fp32"
            tens[base + j, 0] = b.data_ptr()
            tens[base + j, 5] = self.buffer_ema[id(b)].data_ptr()
            tens[base + j, 6] = b.numel()
        ct, chunk0, nchunks = chunk_rows([t.numel() for t in self.params + self.ema_buffers], chunk)
        self._tens_dev = to_device_bytes(tens, dev)
        self._chunks_dev = to_device_bytes(ct, dev)
        self._nchunks = len(ct)
        if self.normed:
            # the norm pass: a side table beside the 64-byte tensor rows (first chunk row, row count, LARS flag),
            # its scratch (one fp64 record per chunk row) and its outputs - all allocated here, none in launch()
            ntens = tens.shape[0]
            assert L.dtm_opt_norm_meta_bytes() == 16
            meta = np.zeros((ntens, 4), dtype=np.int32)
            meta[:, 0], meta[:, 1] = chunk0, nchunks
            for i, p in enumerate(self.params):
                meta[i, 2] = int(self.state[p]["adapt"])
            self._ntens = ntens
            self._meta_dev = to_device_bytes(meta, dev)
            self._norm_scratch = torch.zeros(int(L.dtm_opt_norm_scratch_bytes(len(ct), ntens)) // 8,
                                             dtype=torch.float64, device=dev)
            self._norms = torch.zeros((ntens, 3), dtype=torch.float32, device=dev)
            self._lr_scale = torch.ones(ntens, dtype=torch.float32, device=dev)
            self._gclip = torch.ones(1, dtype=torch.float32, device=dev)
        if self.kind in ADAM_LIKE:
            assert L.dtm_adam_state_bytes() == 16
            self._adam_state = torch.zeros(4, dtype=torch.int32, device=dev)
        self._dyn = torch.zeros(3, dtype=torch.float32, device=dev)
        # ring of pinned staging rows: the host runs ahead of the GPU, so a row is reused only
        # after the copy that last read it has executed (its event), never overwritten in flight
        self._dyn_ring = torch.zeros((16, 3), dtype=torch.float32).pin_memory()
        self._dyn_ev = [None] * 16
        self._dyn_i = 0
        self._dev = dev

    @staticmethod
    def _grad_tensor(p):
        g = getattr(p, "main_grad", None)
        if g is None:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            g = p.grad
        return g

    def ema_decay_now(self):
        if self.ema_decay is None:
            return 0.0
        n = self.num_updates
        return min(self.ema_decay, (1.0 + n) / (10.0 + n))

    def set_dynamic(self, lr, grad_scale=1.0):
        """Stage per-step scalars on the device (safe to call before a hipGraph replay)."""
        i = self._dyn_i
        self._dyn_i = (i + 1) % len(self._dyn_ev)
        if self._dyn_ev[i] is not None:
            self._dyn_ev[i].synchronize()
        row = self._dyn_ring[i]
        row[0] = float(lr)
        row[1] = float(self.ema_decay_now())
        row[2] = float(grad_scale)
        self._dyn.copy_(row, non_blocking=True)
        ev = self._dyn_ev[i] or torch.cuda.Event()
        ev.record()
        self._dyn_ev[i] = ev

    def launch(self, skip_flag=None):
        """Issue the fused update reading lr/ema/grad_scale from the device scalars."""
        L = _lib.lib()
        if self.kind == "lamb":
            # state advance, moments + records, finalize (norms, trust ratios), apply: all inside the entry point
            rc = L.dtm_multi_tensor_lamb(_lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks,
                                         _lib.ptr(self._meta_dev), self._ntens, self.b1, self.b2, float(self.eps),
                                         int(self.ema_decay is not None), _lib.ptr(skip_flag), _lib.ptr(self._dyn),
                                         _lib.ptr(self._adam_state), _lib.ptr(self._norm_scratch),
                                         _lib.ptr(self._norms), _lib.ptr(self._lr_scale), _lib.stream_ptr())
            if rc != 0:
                raise RuntimeError("dtm_multi_tensor_lamb failed (%d)" % rc)
            return
        if self.kind == "adam":
            # norm pass when clipping, then the state advance and the update (both inside the entry point)
            if self.scaled:
                self.launch_norms()
            rc = L.dtm_multi_tensor_adam(_lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks,
                                         self.b1, self.b2, float(self.eps), int(self.ema_decay is not None),
                                         _lib.ptr(skip_flag), _lib.ptr(self._dyn),
                                         _lib.ptr(self._gclip) if self.clip > 0.0 else None,
                                         _lib.ptr(self._adam_state), _lib.stream_ptr())
            if rc != 0:
                raise RuntimeError("dtm_multi_tensor_adam failed (%d)" % rc)
            return
        if not self.scaled:
            L.dtm_multi_tensor_opt(_lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks,
                                   KINDS[self.kind], 0.0, float(self.mu), float(self.rho), float(self.eps), 1.0, 0.0,
                                   int(self.ema_decay is not None), _lib.ptr(skip_flag), _lib.ptr(self._dyn),
                                   _lib.stream_ptr())
            return
        # norm pass (two launches), then the update reading the trust ratios / the clip factor it wrote
        self.launch_norms()
        L.dtm_multi_tensor_opt_scaled(_lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks,
                                      KINDS[self.kind], 0.0, float(self.mu), float(self.rho), float(self.eps), 1.0,
                                      0.0, int(self.ema_decay is not None), _lib.ptr(skip_flag), _lib.ptr(self._dyn),
                                      _lib.ptr(self._lr_scale) if self.kind == "lars" else None,
                                      _lib.ptr(self._gclip) if self.clip > 0.0 else None, _lib.stream_ptr())

    def launch_norms(self):
        """Issue the two-launch norm pass alone (norms, trust ratios and clip factor of the current weights and
        gradients, with grad_scale from the device scalars); ``launch()`` runs it before the update."""
        rc = _lib.lib().dtm_multi_tensor_norms(
            _lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks, _lib.ptr(self._meta_dev),
            self._ntens, _lib.ptr(self._dyn), 1.0, self.lars_eeta, self.lars_eps, self.clip,
            _lib.ptr(self._norm_scratch), _lib.ptr(self._norms), _lib.ptr(self._lr_scale), _lib.ptr(self._gclip),
            _lib.stream_ptr())
        if rc != 0:
            raise RuntimeError("dtm_multi_tensor_norms failed (%d)" % rc)

    def last_norms(self):
        """The device tensor [ntens, 3] of (|p|, |grad*grad_scale|, |grad*grad_scale + wd*p|) per table row (the
        parameters in order, then the EMA-only rows, which stay 0) that the last step's norm pass wrote; None when
        none of LARS, clipping and LAMB is on.  Returned without synchronising: the global gradient norm is
        ``last_norms()[:, 2].double().square().sum().sqrt()``, the trust ratios are ``last_lr_scale()``.
        Under LAMB the columns are (|p|, |r|, |grad*grad_scale|) of the last applied step, r being the update
        direction with its decoupled decay term."""
        return self._norms

    def last_lr_scale(self):
        """The device tensor [ntens] of per-tensor rate factors (LARS trust ratios, LAMB's phi; 1 where not
        adapted)."""
        return self._lr_scale

    def norm_stats(self):
        """Host-side digest of the last step's norms (reads the device: call on logged steps, after their sync)."""
        if self._norms is None:
            return {}
        n = self._norms.detach().cpu().double()
        out = {"grad_norm": float(n[:, 2].square().sum().sqrt())}  # (LAMB: |gs|, no decay term in it)
        if self.kind == "lamb":
            out["update_norm"] = float(n[:, 1].square().sum().sqrt())
        adapted = [i for i, p in enumerate(self.params) if self.state[p]["adapt"]]
        if self.kind in ("lars", "lamb") and adapted:
            r = self._lr_scale.detach().cpu()[adapted]
            out[self.kind + "/min_trust_ratio"], out[self.kind + "/max_trust_ratio"] = float(r.min()), float(r.max())
        return out

    def adam_step(self):
        """The number of Adam (or LAMB) updates applied so far (skipped ones not counted).  Reads the device: call it
        on logged steps and at checkpoints only."""
        if self._adam_state is not None:
            return int(self._adam_state[0].item())
        return self._adam_t

    def set_adam_step(self, t):
        """Set the applied-update count (a restore); the correction terms follow from it."""
        t = max(0, int(t))
        self._adam_t = t
        if self._adam_state is not None:
            bc1, bc2 = _bias_corrections(self.b1, self.b2, t)
            rec = np.zeros(4, dtype=np.int32)
            rec[0] = t
            rec[1:3] = np.array([bc1, bc2], dtype=np.float32).view(np.int32)
            self._adam_state.copy_(torch.from_numpy(rec))

    def beta_powers(self):
        """(b1^(t+1), b2^(t+1)) in fp32: the values of TensorFlow's beta1_power / beta2_power variables after t
        applies (they start at b1 and b2).  Reads the device."""
        t = self.adam_step()
        return np.float32(self.b1 ** (t + 1)), np.float32(self.b2 ** (t + 1))

    def restored(self, global_step):
        """After a checkpoint restore: ``num_updates`` follows ``global_step``; Adam's applied-update count is
        recovered from the restored beta2_power (b2^(t+1)), from beta1_power when b2 is 0 or the entry was absent
        (or has underflowed), and from ``global_step`` when neither is there."""
        self.num_updates = int(global_step)
        if self.kind not in ADAM_LIKE:
            return
        t = None
        for name, b in (("beta2_power", self.b2), ("beta1_power", self.b1)):
            v = self._adam_loaded.get(name)
            if v is not None and 0.0 < b < 1.0 and 1.1754944e-38 <= v <= b * (1.0 + 1e-6):  # a normal fp32 b^(t+1)
                t = int(round(math.log(v) / math.log(b))) - 1
                break
        self._adam_loaded = {}
        self.set_adam_step(int(global_step) if t is None else t)

    def step(self, lr=None, grad_scale=1.0, skip_flag=None, refresh=True):
        """``refresh`` False: the caller re-derives the dgrad copies itself (``ops.nn.refresh_flipped``) after a pass
        of its own over the updated weights (the pruning apply)."""
        lr = self.lr if lr is None else lr
        if self._dev is not None:
            self.set_dynamic(lr, grad_scale)
            self.launch(skip_flag)
            if refresh:
                from .nn import refresh_flipped
                refresh_flipped()
        else:
            self._step_cpu(lr, grad_scale, skip_flag)
        self.num_updates += 1

    @torch.no_grad()
    def _step_cpu(self, lr, grad_scale, skip_flag):
        if skip_flag is not None and int(skip_flag.item()) != 0:
            return
        d = self.ema_decay_now()
        gclip = 1.0
        if self.kind in ADAM_LIKE:  # applied updates only: the early return above leaves the count alone
            self._adam_t += 1
            bc1, bc2 = _bias_corrections(self.b1, self.b2, self._adam_t)
        if self.scaled:  # the norm pass: fp32 terms as the kernel forms them, fp64 sums
            self._norms.zero_()
            self._lr_scale.fill_(1.0)
            total = 0.0
            for i, p in enumerate(self.params):
                st = self.state[p]
                g = getattr(p, "main_grad", None)
                if g is None:
                    g = p.grad
                if g is None:
                    continue
                gs = g.float() * grad_scale
                ge = g.float() * grad_scale + st["wd"] * p
                pn = math.sqrt(float(p.detach().double().square().sum()))
                gn = math.sqrt(float(gs.double().square().sum()))
                ge2 = float(ge.double().square().sum())
                total += ge2
                self._norms[i, 0], self._norms[i, 1], self._norms[i, 2] = pn, gn, math.sqrt(ge2)
                if st["adapt"] and pn > 0.0 and gn > 0.0:
                    self._lr_scale[i] = self.lars_eeta * pn / (gn + st["wd"] * pn + self.lars_eps)
            if self.clip > 0.0:
                gclip = float(np.float32(self.clip / max(math.sqrt(total), self.clip)))
            self._gclip.fill_(gclip)
        if self.kind == "lamb":
            self._norms.zero_()
            self._lr_scale.fill_(1.0)
        for i, p in enumerate(self.params):
            st = self.state[p]
            g = getattr(p, "main_grad", None)
            if g is None:
                g = p.grad
            if g is None:
                continue
            if self.kind == "lamb":  # fp32 terms, fp64 sums, phi and the step rounded to fp32 as in the kernels
                gs = g.float() * grad_scale
                st["s1"].mul_(self.b1).add_(gs, alpha=1 - self.b1)
                st["s2"].mul_(self.b2).addcmul_(gs, gs, value=1 - self.b2)
                r = (st["s1"] / float(bc1)) / (torch.sqrt(st["s2"]) / float(bc2) + self.eps) + st["wd"] * p
                pn, rn, gn = (math.sqrt(float(x.detach().double().square().sum())) for x in (p, r, gs))
                self._norms[i, 0], self._norms[i, 1], self._norms[i, 2] = pn, rn, gn
                if st["adapt"] and pn > 0.0 and rn > 0.0:
                    self._lr_scale[i] = pn / rn
                step = np.float32(np.float32(lr) * np.float32(st["lr_mult"])) * np.float32(float(self._lr_scale[i]))
                p.sub_(float(step) * r)
                w16 = getattr(p, "bf16", None)
                if w16 is not None:
                    w16.copy_(p)
                if "ema" in st:
                    st["ema"].sub_((1 - d) * (st["ema"] - p))
                continue
            g = g.float() * grad_scale + st["wd"] * p
            if self.clip > 0.0:
                g = g * gclip
            lr_p = lr * st["lr_mult"]
            if self.kind == "lars":
                lr_p = lr_p * float(self._lr_scale[i])
            if self.kind == "adam":
                st["s1"].mul_(self.b1).add_(g, alpha=1 - self.b1)
                st["s2"].mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
                p.sub_(float(np.float32(lr_p) * bc2 / bc1) * st["s1"] / (torch.sqrt(st["s2"]) + self.eps))
            elif self.kind == "sgd":
                p.sub_(lr_p * g)
            elif self.kind in ("momentum", "lars"):
                st["s1"].mul_(self.mu).add_(g)
                p.sub_(lr_p * st["s1"])
            else:
                st["s2"].mul_(self.rho).add_((1 - self.rho) * g * g)
                st["s1"].mul_(self.mu).add_(lr_p * g / torch.sqrt(st["s2"] + self.eps))
                p.sub_(st["s1"])
            w16 = getattr(p, "bf16", None)
            if w16 is not None:
                w16.copy_(p)
            if "ema" in st:
                st["ema"].sub_((1 - d) * (st["ema"] - p))
        for b in self.ema_buffers:
            e = self.buffer_ema[id(b)]
            e.sub_((1 - d) * (e - b.float()))

    # ---- state for checkpoints (TF slot names) -------------------------------------------------
    def slot_variables(self):
        """(tf_name, tensor) for optimizer slots: Momentum -> <v>/Momentum, RMSProp -> <v>/RMSProp (ms),
        <v>/RMSProp_1 (mom), EMA -> <v>/ExponentialMovingAverage.  LARS saves its accumulator as <v>/Momentum too,
        so momentum and LARS runs resume into each other; the slot name TensorFlow's own contrib LARS optimizer
        writes is not checked here (TensorFlow is not part of the test environment).  Adam -> <v>/Adam (m), <v>/Adam_1
        (v) and the scalars beta1_power, beta2_power (``beta_powers()``); parity of these names with a file written
        by TensorFlow itself is not checked here either.  LAMB saves the same four names as Adam, so Adam and LAMB
        runs resume into each other; parity with the names a TensorFlow LAMB writes is not checked."""
        out = []
        for p in self.params:
            name = getattr(p, "tf_name", None)
            if name is None:
                continue
            st = self.state[p]
            if self.kind in ("momentum", "lars"):
                out.append((name + "/Momentum", st["s1"]))
            elif self.kind == "rmsprop":
                out.append((name + "/RMSProp", st["s2"]))
                out.append((name + "/RMSProp_1", st["s1"]))
            elif self.kind in ADAM_LIKE:
                out.append((name + "/Adam", st["s1"]))
                out.append((name + "/Adam_1", st["s2"]))
            if "ema" in st:
                out.append((name + "/ExponentialMovingAverage", st["ema"]))
        if self.kind in ADAM_LIKE:
            b1p, b2p = self.beta_powers()
            out.append(("beta1_power", torch.tensor(b1p)))
            out.append(("beta2_power", torch.tensor(b2p)))
        return out

    def buffer_shadows(self):
        """[(buffer, shadow)] for the EMA-averaged non-trainable tensors (BN moving statistics)."""
        return [(b, self.buffer_ema[id(b)]) for b in self.ema_buffers]
