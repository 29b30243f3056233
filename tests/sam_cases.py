"""Shared pieces of the SAM tests (tests/test_sam_cpu.py, tests/test_sam_gpu.py): the fp64 numpy evaluation of the
definition and the hand-written composition of a SAM step from a plain TrainStep, ops.sam and FusedOptimizer."""
import numpy as np
import torch

from distributed_tensorflow_models_amd.engine import TrainStep, moving_average_buffers
from distributed_tensorflow_models_amd.ops import elementwise as E
from distributed_tensorflow_models_amd.ops import nn as F
from distributed_tensorflow_models_amd.ops import sam

ULP32 = 2.0 ** -23


def oracle_norm_scale(ps, gs, rho, adaptive):
    """(sqrt(S), float32(rho / (sqrt(S) + 1e-12))) from numpy: the fp32 terms of the definition, an fp64 sum."""
    S = np.float64(0.0)
    with np.errstate(all="ignore"):
        for p, g in zip(ps, gs):
            p, g = p.detach().cpu().numpy().reshape(-1), g.detach().cpu().numpy().reshape(-1)
            x = (np.abs(p) * g).astype(np.float32) if adaptive else g
            S = S + np.sum(x.astype(np.float64) ** 2, dtype=np.float64)
        nrm = np.sqrt(S)
        return float(nrm), np.float32(np.float64(rho) / (nrm + np.float64(1e-12)))


def oracle_p_hat(p, g, scale, adaptive):
    """p_hat from numpy fp32 arithmetic, one rounding per operation, given the fp32 ``scale``."""
    p, g = p.detach().cpu().numpy(), g.detach().cpu().numpy()
    s = np.float32(scale)
    with np.errstate(all="ignore"):
        e = ((s * p).astype(np.float32) * p).astype(np.float32) * g if adaptive else s * g
        return torch.from_numpy((p + e.astype(np.float32)).astype(np.float32))


def check_norm_scale(got_norm, got_scale, ps, gs, rho, adaptive, what=""):
    """sqrt(S) within relative n * 2^-52 (the worst case of any order of an fp64 sum of n non-negative terms; the
    value read back is fp32, so half an fp32 ulp of rounding comes on top) and scale within one fp32 ulp."""
    n = sum(g.numel() for g in gs)
    want_norm, want_scale = oracle_norm_scale(ps, gs, rho, adaptive)
    got_norm, got_scale = float(got_norm), float(got_scale)
    print("%s sqrt(S) got %.9g want %.17g; scale got %.9g want %.9g" % (what, got_norm, want_norm, got_scale,
                                                                         float(want_scale)))
    assert abs(got_norm - want_norm) <= want_norm * (n * 2.0 ** -52 + 0.5 * ULP32), what
    assert abs(got_scale - float(want_scale)) <= float(np.spacing(want_scale)), what


def same_bits(a, b, nan_ok=False):
    """Bitwise equality of two tensors of one dtype; ``nan_ok``: a NaN equals any NaN (an arithmetic result's NaN
    encoding is the unit's choice)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not nan_ok:
        return torch.equal(a.view(it), b.view(it))
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.view(it)[~na], b.view(it)[~nb])


def model_state(model, step):
    """Every bit a step may move: weights, bf16 copies, optimizer slots and shadows, BN statistics (last; a slim
    model keeps them as parameters that do not require a gradient, so only trainable ones count as weights)."""
    out = [p.detach().clone() for p in model.parameters() if p.requires_grad]
    out += [p.bf16.detach().clone() for p in model.parameters() if getattr(p, "bf16", None) is not None]
    for p in step.opt.params:
        out += [step.opt.state[p][k].detach().clone() for k in ("s1", "s2", "ema") if k in step.opt.state[p]]
    out += [e.detach().clone() for _b, e in step.opt.buffer_shadows()]
    out += [b.detach().clone() for b in moving_average_buffers(model)]
    return out


def states_equal(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


class HandSam:
    """A SAM step composed by hand around a plain step ``st`` (a TrainStep built WITHOUT sam on a twin model): its
    ``_forward_backward`` is the model, ``loss_fn`` and backward of one pass; the perturbation is an ops.sam
    perturber of this class's own; the update is the step's FusedOptimizer."""

    def __init__(self, st, config):
        self.st = st
        params = [p for p in st.model.parameters() if p.requires_grad]
        self.samp = sam.SamPerturber([(p.data, p.main_grad, getattr(p, "bf16", None)) for p in params],
                                     moving_average_buffers(st.model), config=config)

    def micro(self, x, y):
        """(ascent loss, descent gradient) of one micro-batch; the weights and statistics end as the ascent pass
        left them."""
        st = self.st
        cuda = st.dp.flat.is_cuda
        seed = E._seed[0]
        loss, _skip = st._forward_backward(x, y)          # zero-grad, forward, loss, backward at p
        self.samp.perturb()
        if cuda:
            F.refresh_flipped()
        E._seed[0] = seed                                  # the same dropout masks: host stream and device offset
        if cuda:
            E.seed_offset(x.device).sub_(1)
        st._forward_backward(x, y)                         # the same at p_hat
        self.samp.restore()
        return loss, st.dp.flat.clone()

    def step(self, xs, ys, lr):
        """One update from the micro-batches ``xs``, ``ys`` (lists): the descent gradients summed in order, the
        NaN guard on the sum, the optimizer with grad_scale 1 / n.  Returns the mean ascent loss."""
        st = self.st
        losses, total = [], None
        for x, y in zip(xs, ys):
            loss, g = self.micro(x, y)
            losses.append(loss)
            total = g if total is None else total + g
        st.dp.flat.copy_(total)
        skip = torch.tensor([0 if bool(torch.isfinite(total).all()) else 1], dtype=torch.int32,
                            device=total.device)
        st.opt.step(lr, grad_scale=1.0 / len(xs), skip_flag=skip)
        st.global_step += 1
        loss = losses[0]
        for v in losses[1:]:
            loss = loss + v
        return loss / len(xs) if len(xs) > 1 else loss


__all__ = ["TrainStep", "HandSam", "oracle_norm_scale", "oracle_p_hat", "check_norm_scale", "same_bits",
           "model_state", "states_equal"]
