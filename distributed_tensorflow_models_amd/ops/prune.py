"""Gradual magnitude pruning (Zhu and Gupta 2017, "To prune, or not to prune"; tf.contrib.model_pruning):
the schedule, the selection and the mask apply (csrc/kernels/prune.hip).

Schedule (a pure function of the step t, in Python floats):
  sparsity_at(t) = target + (initial - target) * (1 - clamp((t - begin) / (end - begin), 0, 1)) ** exponent
                   (``target`` when end == begin)
  updates_at(t)  = begin <= t <= end and ((t - begin) % frequency == 0 or t == end)
Selection, per pruned tensor of n elements at sparsity s:
  z = floor(float64(s) * n); key = bits(w) & 0x7fffffff as an unsigned integer (-0 == +0, denormals order, Inf and
  NaN sort largest and are kept); z == 0: mask all ones, threshold key 0; else tau = the z-th smallest key (1-based),
  mask = key > tau, kept = the number of ones.  Ties at tau are all pruned (n - kept >= z): the definition is a
  threshold, so the order of the elements never matters and the result is exact.
Apply, every step after the optimizer's update: w = mask ? w : +0.0 on the weight, its bf16 compute copy and its EMA
  shadow; kept elements stay bit for bit, optimizer slots are not touched.
Update: the masks so far are applied to the freshly updated weights in front of the selection (the optimizer moves
  a pruned coordinate off zero, its gradient is not masked), so pruned weights are zeros, the smallest keys of the
  selection, and masks only shrink: there is no regrowth.

On CUDA tensors ``Pruner`` runs the HIP kernels over its own tensor table and chunk list (9 launches, every decision
in a 16-byte device record, so the launches can sit in a captured hipGraph); on CPU tensors the same definition runs
as torch ops (the CPU path of the feature and the kernels' oracle).
"""
import math

import numpy as np
import torch

from . import _lib


class PruneConfig:
    """``select(name, p) -> bool`` picks the pruned tensors (default: every trainable parameter with dim() >= 2).
    ``end_step`` None: ``begin_step`` (one update, straight to the target)."""
    __slots__ = ("target_sparsity", "initial_sparsity", "begin_step", "end_step", "frequency", "exponent", "select")

    def __init__(self, target_sparsity, initial_sparsity=0.0, begin_step=0, end_step=None, frequency=100,
                 exponent=3.0, select=None):
        target, initial = float(target_sparsity), float(initial_sparsity)
        begin = int(begin_step)
        end = begin if end_step is None else int(end_step)
        if not 0.0 <= initial <= target < 1.0:
            raise ValueError("pruning needs 0 <= initial_sparsity <= target_sparsity < 1, got %r, %r"
                             % (initial_sparsity, target_sparsity))
        if not 0 <= begin <= end:
            raise ValueError("pruning needs 0 <= begin_step <= end_step, got %r, %r" % (begin_step, end_step))
        if int(frequency) < 1:
            raise ValueError("pruning frequency must be at least 1, got %r" % (frequency,))
        if not float(exponent) > 0.0:
            raise ValueError("pruning exponent must be positive, got %r" % (exponent,))
        if select is not None and not callable(select):
            raise ValueError("select must be a callable (name, parameter) -> bool or None")
        self.target_sparsity, self.initial_sparsity = target, initial
        self.begin_step, self.end_step, self.frequency, self.exponent = begin, end, int(frequency), float(exponent)
        self.select = select

    def sparsity_at(self, t):
        if self.end_step == self.begin_step:
            return self.target_sparsity
        x = min(max((t - self.begin_step) / float(self.end_step - self.begin_step), 0.0), 1.0)
        return self.target_sparsity + (self.initial_sparsity - self.target_sparsity) * (1.0 - x) ** self.exponent

    def updates_at(self, t):
        return self.begin_step <= t <= self.end_step and \
            ((t - self.begin_step) % self.frequency == 0 or t == self.end_step)

    def selects(self, name, p):
        if self.select is not None:
            return bool(self.select(name, p))
        return p.dim() >= 2


def magnitude_keys(w):
    """int32 tensor [n] of the 31-bit magnitude patterns of a contiguous fp32 tensor."""
    return w.detach().reshape(-1).view(torch.int32) & 0x7fffffff


def rank_of(sparsity, n):
    return int(math.floor(float(sparsity) * n))


@torch.no_grad()
def select_mask(w, sparsity):
    """(mask uint8 of w's shape, tau, kept, z) of the definition above, as torch ops on w's device."""
    n = w.numel()
    z = rank_of(sparsity, n)
    if z == 0:
        return torch.ones(w.shape, dtype=torch.uint8, device=w.device), 0, n, 0
    k = magnitude_keys(w)
    tau = torch.kthvalue(k, z).values
    mask = (k > tau).to(torch.uint8).view(w.shape)
    return mask, int(tau), int(mask.sum()), z


@torch.no_grad()
def apply_mask(mask, *tensors):
    """t = mask ? t : +0 on every given tensor (None entries skipped)."""
    off = mask == 0
    for t in tensors:
        if t is not None:
            t.masked_fill_(off, 0.0)


def _check_sparsity(s):
    if not 0.0 <= s < 1.0:  # (a NaN fails both comparisons)
        raise ValueError("sparsity must lie in [0, 1), got %r" % (s,))


class Pruner:
    """Masks, thresholds and kept counts of a list of pruned tensors, and the passes over them.

    ``entries``: (name, w, w16, shadow) per tensor - ``w`` a contiguous fp32 tensor (it may start at any element of
    a larger buffer), ``w16`` its bf16 copy or None, ``shadow`` its fp32 EMA shadow or None.  ``vector`` False: the
    kernels use 4-byte accesses throughout (a row whose copies do not share the weight's offset from a 16-byte
    boundary does so by itself)."""

    def __init__(self, entries, vector=True):
        self.entries = [tuple(e) for e in entries]
        if not self.entries:
            raise ValueError("nothing to prune: no tensor was selected")
        dev = self.entries[0][1].device
        for name, w, w16, sh in self.entries:
            if w.dtype != torch.float32 or not w.is_contiguous() or w.device != dev or w.numel() < 1:
                raise ValueError("pruned tensor %s must be a non-empty contiguous fp32 tensor on %s" % (name, dev))
            if w16 is not None and (w16.dtype != torch.bfloat16 or w16.shape != w.shape or not w16.is_contiguous()):
                raise ValueError("bf16 copy of %s must be contiguous bf16 of the weight's shape" % name)
            if sh is not None and (sh.dtype != torch.float32 or sh.shape != w.shape or not sh.is_contiguous()):
                raise ValueError("shadow of %s must be contiguous fp32 of the weight's shape" % name)
        nt = len(self.entries)
        self.names = [e[0] for e in self.entries]
        self.numel = [e[1].numel() for e in self.entries]
        self.tau = torch.zeros(nt, dtype=torch.int32, device=dev)   # the key's 31 bits (never negative)
        self.kept = torch.tensor(self.numel, dtype=torch.int32, device=dev)
        self.z = torch.zeros(nt, dtype=torch.int32, device=dev)
        self._staged = (0.0, 0)
        self._dev = dev if dev.type == "cuda" else None
        if self._dev is None:
            self.masks = [torch.ones(e[1].shape, dtype=torch.uint8) for e in self.entries]
        else:
            self._build_tables(bool(vector))

    # ---- device tables ---------------------------------------------------------------------
    def _build_tables(self, vector):
        L = _lib.lib()
        assert L.dtm_prune_tensor_bytes() == 64 and L.dtm_prune_chunk_bytes() == 8 and L.dtm_prune_rec_bytes() == 16
        dev, nt = self._dev, len(self.entries)
        heads = [((16 - e[1].data_ptr() % 16) % 16) // 4 for e in self.entries]
        # masks: one flat byte buffer; a mask reaches a 16-byte boundary where its weight does
        offs, total = [], 0
        for n, h in zip(self.numel, heads):
            offs.append(total + (16 - h) % 16)
            total += (n + 31) // 16 * 16
        self._mask_flat = torch.ones(total, dtype=torch.uint8, device=dev)
        assert self._mask_flat.data_ptr() % 16 == 0
        self.masks = [self._mask_flat[o:o + n].view(e[1].shape) for o, n, e in zip(offs, self.numel, self.entries)]
        tens = np.zeros((nt, 8), dtype=np.uint64)
        chunk_t = []
        for i, ((name, w, w16, sh), h) in enumerate(zip(self.entries, heads)):
            nc = int(L.dtm_prune_num_chunks(_lib.ptr(w), w.numel()))
            if nc < 0:
                raise ValueError("pruned tensor %s has %d elements: 2^31 or more are not supported" % (name, w.numel()))
            vec = vector and (w16 is None or (w16.data_ptr() + 2 * h) % 8 == 0) \
                and (sh is None or sh.data_ptr() % 16 == w.data_ptr() % 16)
            tens[i, :4] = [w.data_ptr(), w16.data_ptr() if w16 is not None else 0,
                           sh.data_ptr() if sh is not None else 0, self.masks[i].data_ptr()]
            tens[i, 4] = w.numel()
            tens[i, 5] = np.array([len(chunk_t), nc], dtype=np.int32).view(np.uint64)[0]
            tens[i, 6] = np.array([int(vec), 0], dtype=np.int32).view(np.uint64)[0]
            chunk_t.extend([i] * nc)
        ct = np.zeros((len(chunk_t), 2), dtype=np.int32)
        ct[:, 0] = chunk_t
        self._tens_dev = torch.from_numpy(tens.view(np.uint8).reshape(-1).copy()).to(dev)
        self._chunks_dev = torch.from_numpy(ct.view(np.uint8).reshape(-1).copy()).to(dev)
        self._nchunks, self._max_n = len(chunk_t), max(self.numel)
        # select scratch: {prefix, rank} per tensor and one histogram row per tensor
        self._state = torch.zeros((nt, 2), dtype=torch.int32, device=dev)
        self._hist = torch.zeros((nt, int(L.dtm_prune_hist_bins())), dtype=torch.int32, device=dev)
        self._rec = torch.zeros(16, dtype=torch.uint8, device=dev)
        # ring of pinned staging rows, as FusedOptimizer.set_dynamic: a row is reused only after its copy has run
        self._rec_ring = torch.zeros((16, 16), dtype=torch.uint8).pin_memory()
        self._rec_ev = [None] * 16
        self._rec_i = 0

    # ---- the step's two halves -----------------------------------------------------------------
    def stage(self, sparsity, update):
        """Stage the step's record {sparsity, update} (safe to call before a hipGraph replay)."""
        sparsity, update = float(sparsity), int(bool(update))
        if self._dev is None:
            _check_sparsity(sparsity)
            self._staged = (sparsity, update)
            return
        i = self._rec_i
        row = self._rec_ring[i]
        if self._rec_ev[i] is not None:
            self._rec_ev[i].synchronize()
        rc = _lib.lib().dtm_prune_fill_record(_lib.ptr(row), sparsity, update)
        if rc == -3:
            _check_sparsity(sparsity)
        if rc != 0:
            raise RuntimeError("dtm_prune_fill_record failed (%d)" % rc)
        self._rec_i = (i + 1) % len(self._rec_ev)
        self._rec.copy_(row, non_blocking=True)
        ev = self._rec_ev[i] or torch.cuda.Event()
        ev.record()
        self._rec_ev[i] = ev
        self._staged = (sparsity, update)

    def launch_select(self):
        rc = _lib.lib().dtm_prune_select(
            _lib.ptr(self._tens_dev), len(self.entries), _lib.ptr(self._chunks_dev), self._nchunks,
            _lib.ptr(self._rec), _lib.ptr(self._state), _lib.ptr(self._hist), _lib.ptr(self.tau), _lib.ptr(self.kept),
            _lib.ptr(self.z), self._max_n, _lib.stream_ptr())
        if rc != 0:
            raise RuntimeError("dtm_prune_select failed (%d)" % rc)

    def launch_apply(self, pre=False):
        """``pre``: the launch in front of the select stages (the stored masks, on an update step only)."""
        rc = _lib.lib().dtm_prune_apply(
            _lib.ptr(self._tens_dev), len(self.entries), _lib.ptr(self._chunks_dev), self._nchunks,
            _lib.ptr(self._rec), _lib.ptr(self.tau), _lib.ptr(self.kept), _lib.ptr(self.z), self._max_n,
            int(pre), _lib.stream_ptr())
        if rc != 0:
            raise RuntimeError("dtm_prune_apply failed (%d)" % rc)

    def launch(self):
        """Select (a no-op on the device unless the staged record says update) and apply."""
        if self._dev is None:
            self._step_cpu()
            return
        self.launch_apply(pre=True)
        self.launch_select()
        self.launch_apply()

    def step(self, sparsity, update):
        self.stage(sparsity, update)
        self.launch()

    @torch.no_grad()
    def _step_cpu(self):
        sparsity, update = self._staged
        for i, (_name, w, w16, sh) in enumerate(self.entries):
            if update:
                apply_mask(self.masks[i], w, w16, sh)
                mask, tau, kept, z = select_mask(w, sparsity)
                self.masks[i].copy_(mask)
                self.tau[i], self.kept[i], self.z[i] = tau, kept, z
            apply_mask(self.masks[i], w, w16, sh)

    # ---- state ---------------------------------------------------------------------------------
    @torch.no_grad()
    def masks_loaded(self):
        """After masks were written from outside (a checkpoint restore): the kept counts follow them, and the
        weights, copies and shadows are masked at once."""
        for i, (_name, w, w16, sh) in enumerate(self.entries):
            self.masks[i].ne_(0)
            self.kept[i] = int(self.masks[i].sum())
            apply_mask(self.masks[i], w, w16, sh)

    @torch.no_grad()
    def reset(self):
        """All masks back to ones (nothing pruned); the tensors themselves are not touched."""
        for m in self.masks:
            m.fill_(1)
        self.kept.copy_(torch.tensor(self.numel, dtype=torch.int32))
        self.tau.zero_()
        self.z.zero_()

    def sparsity(self):
        """(sum n - sum kept) / sum n over the pruned tensors.  Reads the device."""
        total = float(sum(self.numel))
        return (total - float(self.kept.sum().item())) / total


# ---- checkpoint variables ------------------------------------------------------------------
def mask_scope(var_name):
    """``<scope>/weights`` (or ``kernel``) -> ``<scope>``; any other variable keeps its own name as the scope."""
    head, _, last = var_name.rpartition("/")
    return head if head and last in ("weights", "kernel") else var_name
