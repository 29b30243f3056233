"""Sharpness-aware minimisation (Foret et al. 2021) and ASAM (Kwon et al. 2021): the weight perturbation between the
two passes of a micro-batch and its undoing (csrc/kernels/sam.hip; engine.TrainStep(sam=SamConfig(...))).

For the trainable tensors ``p``, their raw gradients ``g`` (what backward wrote, before any grad_scale or all-reduce),
``rho > 0`` and ``eps = 1e-12``:
  SAM :  S = sum over all elements of g*g         scale = rho / (sqrt(S) + eps)    e = scale * g
  ASAM:  S = sum of (|p|*g)^2   (T_w = |p|)       scale = rho / (sqrt(S) + eps)    e = ((scale * p) * p) * g
  p_hat = p + e
S is summed in fp64, ``scale`` is formed in fp64 and rounded once to fp32, ``e`` and ``p_hat`` are fp32 with one
rounding per operation in the order written and no fused multiply-add.  The norm is global over every row.

``perturb()``:  backup = p (a bit copy);  p = p_hat;  bf16 copy = bf16(p_hat);  g = +0 (the zero-grad of the second
                pass);  a backup-only row (a BN moving statistic): backup = p
``restore()``:  p = backup (a bit copy);  bf16 copy = bf16(p);  g is left alone
Non-finite values are not special-cased: a NaN in ``g`` makes S, scale and every p_hat NaN; an Inf makes scale 0 and
e = 0 * Inf = NaN at that element.  ``restore()`` puts every bit back either way.

On CPU tensors the same four steps run as torch ops - S is ``x.double().square().sum()`` per tensor, added in tensor
order; everything else is one element-wise fp32 op per rounding.  That form is the CPU path of the feature and the
kernels' oracle: it gives the kernels' bits for p_hat given the same ``scale``, and S up to the order of an fp64 sum.
"""
import math

import numpy as np
import torch

from . import _lib
from ._tables import chunk_rows, to_device_bytes

EPS = 1e-12


class SamConfig:
    """``rho``: the radius of the perturbation (finite, above 0; usual starting values: SAM 0.05, ASAM 0.5 - 2).
    ``adaptive``: ASAM's element-wise scaling by |p|."""
    __slots__ = ("rho", "adaptive")

    def __init__(self, rho, adaptive=False):
        try:
            r = float(rho)
        except (TypeError, ValueError):
            raise ValueError("sam rho must be a finite number above 0, got %r" % (rho,))
        if not (math.isfinite(r) and r > 0.0):
            raise ValueError("sam rho must be a finite number above 0, got %r" % (rho,))
        self.rho, self.adaptive = r, bool(adaptive)

    def __repr__(self):
        return "SamConfig(rho=%r, adaptive=%r)" % (self.rho, self.adaptive)


def _backup_like(p):
    """Backup storage for ``p`` at p's own offset from a 16-byte boundary, so that the kernels' 16-byte path depends
    on the weight and its gradient alone."""
    off = (p.data_ptr() % 16) // 4 if p.is_cuda else 0
    buf = torch.zeros(p.numel() + off, dtype=torch.float32, device=p.device)
    return buf[off:].view(p.shape)


class SamPerturber:
    """``entries``: one ``(p, g, pcopy)`` or ``(p, g, pcopy, backup)`` per trainable tensor - the fp32 weight (its
    ``.data``), the fp32 gradient of the same shape (a view into the flat buffer), the bf16 compute copy or None, and
    optionally the backup tensor to use (default: allocated here).  ``buffers``: fp32 tensors that are only saved and
    put back (BN moving statistics), each alone or as ``(tensor, backup)``.  The tables and the backup storage are
    built once, here."""

    def __init__(self, entries, buffers=(), config=None):
        if not isinstance(config, SamConfig):
            raise ValueError("SamPerturber needs an ops.sam.SamConfig, got %r" % (config,))
        self.config = config
        self.rows = []
        for ent in entries:
            p, g, pcopy = ent[0], ent[1], ent[2]
            backup = ent[3] if len(ent) > 3 else None
            if p.dtype != torch.float32 or g.dtype != torch.float32 or p.shape != g.shape or p.device != g.device:
                raise ValueError("sam: weight and gradient must be fp32 tensors of one shape on one device")
            if not (p.is_contiguous() and g.is_contiguous()):
                raise ValueError("sam: weight and gradient must be contiguous")
            if pcopy is not None and (pcopy.dtype != torch.bfloat16 or pcopy.shape != p.shape
                                      or not pcopy.is_contiguous() or pcopy.device != p.device):
                pcopy = None  # (as the optimizer's tables: not a compute copy this pass maintains)
            self.rows.append((p, g, self._backup(p, backup), pcopy))
        for b in buffers:
            b, backup = b if isinstance(b, (tuple, list)) else (b, None)
            if b.dtype != torch.float32 or not b.is_contiguous():
                raise ValueError("sam: buffers must be contiguous fp32 tensors")
            self.rows.append((b, None, self._backup(b, backup), None))
        self._dev = None
        first = self.rows[0][0] if self.rows else None
        self._rec = torch.zeros(2, dtype=torch.float32, device=first.device if first is not None else "cpu")
        if first is not None and first.is_cuda:
            self._build_tables(first.device)

    @staticmethod
    def _backup(p, given):
        if given is None:
            return _backup_like(p)
        if given.dtype != torch.float32 or given.shape != p.shape or not given.is_contiguous() \
                or given.device != p.device:
            raise ValueError("sam: a backup must be a contiguous fp32 tensor of the weight's shape and device")
        return given

    def backup_bytes(self):
        return sum(4 * r[2].numel() for r in self.rows)

    # ---- device tables ---------------------------------------------------------------------
    def _build_tables(self, dev):
        L = _lib.lib()
        chunk = L.dtm_sam_chunk_size()
        assert L.dtm_sam_tensor_bytes() == 40 and L.dtm_sam_chunk_bytes() == 16 and L.dtm_sam_meta_bytes() == 8
        rows = [r for r in self.rows if r[0].numel() > 0]
        tens = np.zeros((len(rows), 5), dtype=np.uint64)
        for i, (p, g, backup, pcopy) in enumerate(rows):
            tens[i] = [p.data_ptr(), g.data_ptr() if g is not None else 0, backup.data_ptr(),
                       pcopy.data_ptr() if pcopy is not None else 0, p.numel()]
        ct, chunk0, nchunks = chunk_rows([r[0].numel() for r in rows], chunk)
        meta = np.stack([chunk0, nchunks], axis=1).astype(np.int32)
        self._tens_dev, self._chunks_dev = to_device_bytes(tens, dev), to_device_bytes(ct, dev)
        self._meta_dev = to_device_bytes(meta, dev)
        self._nchunks, self._ntens = len(ct), len(rows)
        self._scratch = torch.zeros(max(1, int(L.dtm_sam_scratch_bytes(self._nchunks, self._ntens)) // 8),
                                    dtype=torch.float64, device=dev)
        self._dev = dev

    # ---- the two passes --------------------------------------------------------------------
    @torch.no_grad()
    def perturb(self):
        """Launches 1-3: the global norm, {sqrt(S), scale}, and the perturbation of every row."""
        if self._dev is not None:
            rc = _lib.lib().dtm_sam_perturb(_lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks,
                                            _lib.ptr(self._meta_dev), self._ntens, self.config.rho,
                                            int(self.config.adaptive), _lib.ptr(self._scratch), _lib.ptr(self._rec),
                                            _lib.stream_ptr())
            if rc != 0:
                raise RuntimeError("dtm_sam_perturb failed (%d)" % rc)
            return
        adaptive = self.config.adaptive
        S = 0.0
        for p, g, _b, _c in self.rows:
            if g is not None:
                x = p.abs() * g if adaptive else g
                S += float(x.double().square().sum())
        nrm = math.sqrt(S) if S == S else float("nan")
        with np.errstate(all="ignore"):
            scale = np.float32(np.float64(self.config.rho) / (np.float64(nrm) + np.float64(EPS)))
            self._rec[0] = float(np.float32(nrm))
        self._rec[1] = float(scale)
        self.perturb_with(float(scale))

    @torch.no_grad()
    def perturb_with(self, scale):
        """(the torch form only) launch 3 with a given fp32 ``scale``: what the kernel computes from that scale."""
        adaptive = self.config.adaptive
        s = torch.tensor(float(scale), dtype=torch.float32)
        for p, g, backup, pcopy in self.rows:
            backup.view(torch.int32).copy_(p.view(torch.int32))
            if g is None:
                continue
            e = ((s * p) * p) * g if adaptive else s * g
            p.copy_(p + e)
            if pcopy is not None:
                pcopy.copy_(p)
            g.zero_()

    @torch.no_grad()
    def restore(self):
        """Launch 4: every row's weight (or statistic) back from its backup, bit for bit, and the bf16 copies from
        the restored weights."""
        if self._dev is not None:
            rc = _lib.lib().dtm_sam_restore(_lib.ptr(self._tens_dev), _lib.ptr(self._chunks_dev), self._nchunks,
                                            self.config.rho, _lib.stream_ptr())
            if rc != 0:
                raise RuntimeError("dtm_sam_restore failed (%d)" % rc)
            return
        for p, g, backup, pcopy in self.rows:
            p.view(torch.int32).copy_(backup.view(torch.int32))
            if g is not None and pcopy is not None:
                pcopy.copy_(p)

    def last_norm(self):
        """The fp32 sqrt(S) of the last ``perturb()``: a one-element view on the rows' device, returned without
        synchronising."""
        return self._rec[0:1]

    def last_scale(self):
        """The fp32 ``scale`` of the last ``perturb()`` (as ``last_norm``)."""
        return self._rec[1:2]
