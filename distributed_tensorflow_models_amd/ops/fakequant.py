"""Fused fake quantisation: TF FakeQuantWithMinMaxVars with its range tracking, as device passes whose state lives
in device memory (csrc/kernels/fakequant.hip), so a quantised training step can be captured into a hipGraph and
replayed across the ``quant_delay`` boundary.  ``compat.quantize`` routes here with ``QuantConfig(fused=True)``.

One quantiser call is ``quantize(x, vmin, vmax, cfg, mode, narrow)``:

* range pass (modes ``WEIGHTS`` and ``ACT_TRAIN``): min and max of the finite elements of ``x`` and whether a NaN or
  +-Inf was seen;
* finalize: the range variables move -- ``WEIGHTS``: ``vmin = min(lo, 0)``, ``vmax = max(hi, 0)``; ``ACT_TRAIN``:
  ``vmin = vmin * d + (1 - d) * min(lo, 0)`` and likewise ``vmax`` (every operation a separate fp32 rounding, ``1 - d``
  formed in double); ``FROZEN``: read only -- and the quantiser's record is written from them with the arithmetic of
  ``compat.quantize.fake_quant``: ``scale = (max(vmax, 0) - min(vmin, 0)) / (qmax - qmin)`` (1 unless > 1e-12),
  ``zp = clamp(rint(qmin - lo / scale), qmin, qmax)``, ``inv_scale = 1 / scale``, and
  ``active = (mode == FROZEN and not cfg.is_training) or step >= cfg.quant_delay`` with ``step`` the config's DEVICE
  counter of training forwards (``QuantConfig.counter``), so nothing on the host decides whether a step quantises;
* apply: ``y = (clamp(rint(x * inv_scale) + zp, qmin, qmax) - zp) * scale`` when active and ``x`` bit for bit otherwise;
  backward: the straight-through mask ``qmin <= q <= qmax`` recomputed from the saved ``x``.  NaN stays NaN with
  gradient 0, +-Inf clamps to the range ends with gradient 0.

The one deliberate difference from the torch-op path of ``compat.quantize``: a batch with a NaN or +-Inf element
leaves ``vmin`` / ``vmax`` untouched (the step quantises with the stored range) and adds 1 to the record's
``nonfinite_batches`` -- there such a batch poisons the range variables for the rest of the run.

The record is one int32[8] tensor: fp32 bits of ``scale, inv_scale, zp, qmin, qmax``, then ``active``,
``nonfinite_batches`` and a zero.  On a CPU tensor the same definitions run as torch ops (the CPU fallback and the
tests' oracle); on the GPU a missing kernel library is an error.
"""
import torch

from . import _lib

WEIGHTS, ACT_TRAIN, FROZEN = 0, 1, 2
REC_WORDS = 8
PARTIAL_STRIDE = 4
_DTYPES = {torch.float32: 0, torch.bfloat16: 1}


def qrange(num_bits, narrow):
    return (1 if narrow else 0), (1 << num_bits) - 1


def grid_size(n, dtype):
    """Blocks of the range and apply passes over ``n`` elements (= partials the range pass writes)."""
    g = _lib.lib().dtm_fq_grid(int(n), _DTYPES[dtype])
    if g < 1:
        raise ValueError("dtm_fq_grid(%d) failed (%d)" % (n, g))
    return g


def block_threads():
    return _lib.lib().dtm_fq_threads()


class QuantizerState:
    """Record and range-pass scratch of one quantiser, on the device of its range variables."""

    def __init__(self, device):
        self.device = device
        if device.type == "cuda":
            L = _lib.lib()
            assert L.dtm_fq_rec_words() == REC_WORDS and L.dtm_fq_partial_stride() == PARTIAL_STRIDE
        self.rec = torch.zeros(REC_WORDS, dtype=torch.int32, device=device)
        self.partials = None

    def record(self):
        """The record as a dict (one device read)."""
        r = self.rec.cpu()
        f = r.view(torch.float32)
        return {"scale": float(f[0]), "inv_scale": float(f[1]), "zp": float(f[2]), "qmin": float(f[3]),
                "qmax": float(f[4]), "active": int(r[5]), "nonfinite_batches": int(r[6])}


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


def state_of(vmin, create=True):
    """The QuantizerState that travels with a quantiser's ``min`` variable (made on first use, and again after the
    variable has moved to another device)."""
    st = getattr(vmin, "_fq_state", None)
    if st is None or st.device != vmin.device:
        if not create:
            return None
        if _capturing(vmin.device):
            raise RuntimeError("fakequant: a quantiser's first call on this device inside a hipGraph capture")
        new = QuantizerState(vmin.device)
        if st is not None:
            new.rec[6] = int(st.rec[6])  # the count follows the variable
        vmin._fq_state = st = new
    return st


def _check(x, vmin, vmax):
    if x.dtype not in _DTYPES:
        raise TypeError("fakequant: fp32 or bf16 expected, got %s" % x.dtype)
    for v in (vmin, vmax):
        if v.dtype != torch.float32 or v.numel() != 1 or v.device != x.device:
            raise ValueError("fakequant: range variables are 1-element fp32 tensors on the input's device")


def _rc(name, rc):
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (name, rc))


# ---- the definitions in torch ops (CPU) ---------------------------------------------------------------------------
def _finalize_cpu(x, vmin, vmax, st, counter, mode, d, bits, narrow, quant_delay, training_cfg):
    rec = st.rec
    if mode != FROZEN:
        xf = x.detach().float().reshape(-1)
        fin = torch.isfinite(xf)
        if not bool(fin.all()):
            rec[6] += 1
        else:
            lo, hi = xf.aminmax()
            lo0, hi0 = torch.clamp(lo, max=0.0), torch.clamp(hi, min=0.0)
            if mode == WEIGHTS:
                vmin.data.copy_(lo0)
                vmax.data.copy_(hi0)
            else:
                vmin.data.mul_(d).add_((1 - d) * lo0)
                vmax.data.mul_(d).add_((1 - d) * hi0)
    qmin, qmax = qrange(bits, narrow)
    lo = torch.clamp(vmin.detach().reshape(1).float(), max=0.0)
    hi = torch.clamp(vmax.detach().reshape(1).float(), min=0.0)
    scale = (hi - lo) / float(qmax - qmin)
    scale = torch.where(scale > 1e-12, scale, torch.ones_like(scale))
    zp = torch.clamp(torch.round(qmin - lo / scale), qmin, qmax)
    f = rec.view(torch.float32)
    f[0:1] = scale
    f[1:2] = 1.0 / scale
    f[2:3] = zp
    f[3], f[4] = float(qmin), float(qmax)
    rec[5] = int((mode == FROZEN and not training_cfg) or int(counter) >= quant_delay)
    rec[7] = 0


def _apply_cpu(x, rec):
    if not int(rec[5]):
        return x.clone()
    f = rec.view(torch.float32)
    q = torch.round(x.float() * f[1]) + f[2]
    return ((torch.clamp(q, f[3], f[4]) - f[2]) * f[0]).to(x.dtype)


def _apply_bwd_cpu(x, dy, rec):
    if not int(rec[5]):
        return dy.clone()
    f = rec.view(torch.float32)
    q = torch.round(x.float() * f[1]) + f[2]
    # (the result takes dy's strides, as ATen's dy * mask does: the layout decides which kernels run downstream)
    return torch.where((q >= f[3]) & (q <= f[4]), dy, torch.zeros((), dtype=dy.dtype), out=torch.empty_like(dy))


# ---- the device passes -------------------------------------------------------------------------------------------
def _finalize_gpu(x, vmin, vmax, st, counter, mode, d, bits, narrow, quant_delay, training_cfg):
    L = _lib.lib()
    nparts = 0
    if mode != FROZEN:
        nparts = grid_size(x.numel(), x.dtype)
        if st.partials is None or st.partials.numel() < nparts * PARTIAL_STRIDE:
            if _capturing(x.device):
                raise RuntimeError("fakequant: first call at this size inside a hipGraph capture")
            st.partials = torch.empty(nparts * PARTIAL_STRIDE, dtype=torch.float32, device=x.device)
        _rc("dtm_fq_range", L.dtm_fq_range(_lib.ptr(x), _DTYPES[x.dtype], x.numel(), _lib.ptr(st.partials),
                                           _lib.stream_ptr()))
    _rc("dtm_fq_finalize", L.dtm_fq_finalize(_lib.ptr(st.partials), nparts, _lib.ptr(vmin), _lib.ptr(vmax),
                                             _lib.ptr(st.rec), _lib.ptr(counter), mode, float(d), float(1.0 - d),
                                             int(bits), int(bool(narrow)), int(quant_delay), int(bool(training_cfg)),
                                             _lib.stream_ptr()))


def _same_layout(*ts):
    for t in ts:
        if not t.is_contiguous() or t.dtype != ts[0].dtype or t.numel() != ts[0].numel() or t.device != ts[0].device:
            raise ValueError("fakequant: contiguous tensors of one dtype, size and device expected")


def apply_into(x, y, rec):
    """y = Q(x) by the record ``rec``; x, y contiguous on one device, starting at any element (the 16-byte path
    when both share one misalignment, else the element-wise one)."""
    _same_layout(x, y)
    if not x.is_cuda:
        y.copy_(_apply_cpu(x, rec))
        return y
    _rc("dtm_fq_apply", _lib.lib().dtm_fq_apply(_lib.ptr(x), _lib.ptr(y), _DTYPES[x.dtype], x.numel(),
                                                _lib.ptr(rec), _lib.stream_ptr()))
    return y


def apply_bwd_into(x, dy, dx, rec):
    """dx = straight-through gradient of ``apply_into`` at the saved input x."""
    _same_layout(x, dy, dx)
    if not x.is_cuda:
        dx.copy_(_apply_bwd_cpu(x, dy, rec))
        return dx
    _rc("dtm_fq_apply_bwd", _lib.lib().dtm_fq_apply_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dx), _DTYPES[x.dtype],
                                                        x.numel(), _lib.ptr(rec), _lib.stream_ptr()))
    return dx


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rec):
        # x is saved and the quantised code recomputed in backward from it and the record: a quantiser's record is
        # written only by its own finalize in a training forward, so it is unchanged between a step's forward and
        # its backward
        ctx.save_for_backward(x)
        ctx.rec = rec
        if not x.is_cuda:
            return _apply_cpu(x, rec)
        return apply_into(x, torch.empty_like(x), rec)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        if not x.is_cuda:
            return _apply_bwd_cpu(x, dy, ctx.rec), None
        return apply_bwd_into(x, dy.contiguous(), torch.empty_like(x), ctx.rec), None


def finalize(x, vmin, vmax, st, counter, mode, ema_decay=0.999, num_bits=8, narrow=False, quant_delay=0,
             training_cfg=True):
    """Range pass (unless FROZEN) and finalize of one quantiser: moves ``vmin`` / ``vmax`` and writes ``st.rec``.
    ``x``: contiguous fp32 or bf16 (unused when FROZEN); ``counter``: 1-element int64 on the same device."""
    _check(x, vmin, vmax)
    if not 2 <= int(num_bits) <= 16:
        raise ValueError("fakequant: num_bits %d outside [2, 16]" % num_bits)
    if counter.dtype != torch.int64 or counter.numel() != 1 or counter.device != x.device:
        raise ValueError("fakequant: the step counter is a 1-element int64 tensor on the input's device")
    fn = _finalize_gpu if x.is_cuda else _finalize_cpu
    with torch.no_grad():
        fn(x.detach(), vmin.data, vmax.data, st, counter, mode, ema_decay, num_bits, narrow, int(quant_delay),
           training_cfg)


def apply(x, st):
    """``x`` through the quantiser whose record ``st.rec`` holds (differentiable, straight-through)."""
    return _Apply.apply(x, st.rec)


def quantize(x, vmin, vmax, cfg, mode, narrow):
    """One quantiser call of a layer: ``vmin`` / ``vmax`` the layer's range variables, ``cfg`` the model's
    ``compat.quantize.QuantConfig`` (decay, bits, delay, training flag and the device step counter)."""
    if x.numel() == 0:
        return x
    if x.is_cuda and not x.is_contiguous():  # (the torch ops of the CPU path keep the input's strides)
        x = x.contiguous()
    st = state_of(vmin)
    finalize(x, vmin, vmax, st, cfg.counter(x.device), mode, cfg.ema_decay, cfg.num_bits, narrow, cfg.quant_delay,
             cfg.is_training)
    return apply(x, st)


def advance(counter):
    """counter += 1 on the counter's device, in stream order."""
    if counter.is_cuda:
        _rc("dtm_fq_advance", _lib.lib().dtm_fq_advance(_lib.ptr(counter), _lib.stream_ptr()))
    else:
        counter += 1


def quantizer_states(model):
    """The QuantizerStates of a slim-built model, in variable order."""
    out = []
    for n, v in model.store.vars.items():
        if n.endswith("_quant/min"):
            st = state_of(v, create=False)
            if st is not None:
                out.append(st)
    return out


def nonfinite_batches(model):
    """Sum over the model's quantisers of the batches whose range update was skipped (one device read)."""
    recs = [st.rec for st in quantizer_states(model)]
    return int(torch.stack(recs)[:, 6].sum()) if recs else 0
