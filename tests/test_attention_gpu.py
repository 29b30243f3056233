"""The attention kernels (csrc/kernels/attention.hip) against the float64 definition on the same stored bf16 inputs.

Forward, element-wise: |o - o64| <= 2^-8 |o64| + 2^-7 sum_j p64_ij |v_jc| (one bf16 rounding of the result with a
margin of 2; the bf16 rounding of each P operand, 2^-9, with a margin of 4 for the fp32 summation order and exp).
Backward, per tensor: e = |got - want64|_2 / |want64|_2 of the kernels is at most 1.5 times the e of mhsa_torch with
autograd on the same bf16 tensors on the device.  With one token dS is exactly zero, so dq = dk = 0 and e has no
meaning: there the kernels' dq, dk are held to the fp32 rounding that dP - delta leaves, two sums of d products
(2 * d * 2^-24 <= 2^-17 of sum_c |dO_c v_c|), times scale and the other operand."""
import copy

import pytest
import torch

from distributed_tensorflow_models_amd.engine import TrainStep
from distributed_tensorflow_models_amd.models import slim_nets
from distributed_tensorflow_models_amd.models.slim_model import SlimModel
from distributed_tensorflow_models_amd.ops.attention import mhsa, mhsa_torch
from test_attention_cpu import definition

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _inputs(N, L, heads, d, variant):
    g = torch.Generator().manual_seed(11)
    q, k, v, do = (torch.randn(N, L, heads * d, generator=g).to(BF) for _ in range(4))
    if variant == "jump":  # the running max jumps after the first key tile
        k[:, 64:] *= 6
    if variant == "hot":  # logits in the hundreds, near one-hot rows
        q, k = q * 8, k * 8
    if variant == "nan":
        k[1], v[1], do[1] = (float("nan"),) * 3
    return q, k, v, do


def _kernels(q, k, v, do, heads, thirds=False):
    """o, lse, dq, dk, dv of the kernel path; thirds: q, k, v as slices of one [N, L, 3 C] tensor."""
    C = q.shape[-1]
    if thirds:
        qkv = torch.cat([q, k, v], -1).to(DEV).requires_grad_()
        args = qkv.split(C, -1)
    else:
        args = [t.to(DEV).requires_grad_() for t in (q, k, v)]
    o = mhsa(*args, heads)
    lse = o.grad_fn.saved_tensors[4]  # the kernel path's own node
    o.backward(do.to(DEV))
    grads = qkv.grad.split(C, -1) if thirds else [t.grad for t in args]
    return [t.detach().cpu() for t in (o, lse, *grads)]


def _rel(got, want):
    return ((got.double() - want).norm() / want.norm()).item()


def _run(N, L, heads, d, variant=None):
    q, k, v, do = _inputs(N, L, heads, d, variant)
    o, lse, *grads = _kernels(q, k, v, do, heads, thirds=variant == "thirds")
    keep = slice(0, 1) if variant == "nan" else slice(None)  # sample 1 is NaN by construction
    q, k, v, do, o, lse = (t[keep] for t in (q, k, v, do, o, lse))
    ref = [t.double().requires_grad_() for t in (q, k, v)]
    o64, lse64, p64 = definition(*ref, heads, d ** -0.5)
    o64.backward(do.double())
    bound = 2.0 ** -8 * o64.abs() + 2.0 ** -7 * torch.einsum(
        "nhij,njhc->nihc", p64, v.double().abs().reshape(-1, L, heads, d)).reshape(o64.shape)
    fwd = ((o.double() - o64).abs() / bound).max().item()
    lse_err = ((lse.double() - lse64).abs() / (1e-4 * (1 + lse64.abs()))).max().item()
    dev = [t.to(DEV).requires_grad_() for t in (q, k, v)]
    mhsa_torch(*dev, heads).backward(do.to(DEV))
    out = {}
    for name, got, t, w in zip(("dq", "dk", "dv"), grads, dev, ref):
        got, want = got[keep], w.grad
        assert torch.isfinite(got).all(), name
        if want.norm() == 0:  # one token
            cap = 2.0 ** -17 * d ** -0.5 * (do.double() * v.double()).abs().sum() * max(q.abs().max(), k.abs().max())
            out[name] = (got.abs().max().item(), cap.item())
        else:
            out[name] = (_rel(got, want), 1.5 * _rel(t.grad.cpu(), want))
    print((N, L, heads, d, variant), "fwd err / bound %.3f, lse %.3f," % (fwd, lse_err),
          ", ".join("%s %.2e, limit %.2e" % (n, a, b) for n, (a, b) in out.items()))
    assert torch.isfinite(o).all() and fwd <= 1.0 and lse_err <= 1.0, (fwd, lse_err)
    assert all(a <= b for a, b in out.values()), out


CASES = [
    pytest.param(1, 1, 1, 32, None, id="one-token"),
    pytest.param(2, 17, 2, 32, None, id="ragged-tile-two-heads"),
    pytest.param(1, 64, 1, 64, None, id="one-tile"),
    pytest.param(2, 65, 3, 64, None, id="one-row-past-a-tile"),
    pytest.param(2, 49, 4, 128, None, id="botnet-7x7"),
    pytest.param(1, 196, 4, 128, None, id="botnet-14x14"),
    pytest.param(1, 257, 1, 128, None, id="five-key-tiles"),
    pytest.param(2, 65, 2, 64, "thirds", id="pitch-is-not-width"),
    pytest.param(1, 130, 1, 64, "jump", id="max-jumps-after-a-tile"),
    pytest.param(1, 65, 1, 32, "hot", id="logits-in-the-hundreds"),
    pytest.param(2, 17, 1, 32, "nan", id="nan-neighbour-sample"),
]


@pytest.mark.parametrize("N,L,heads,d,variant", CASES)
def test_kernels_against_float64(N, L, heads, d, variant):
    _run(N, L, heads, d, variant)


def test_bit_identical_runs():
    q, k, v, do = _inputs(2, 65, 3, 64, None)
    a, b = _kernels(q, k, v, do, 3), _kernels(q, k, v, do, 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_nhwc_input_keeps_its_shape():
    q, k, v, do = (t.reshape(2, 7, 7, 128) for t in _inputs(2, 49, 4, 32, None))
    got = _kernels(q, k, v, do, 4)
    want = _kernels(*(t.reshape(2, 49, 128) for t in (q, k, v, do)), 4)
    assert got[0].shape == q.shape and all(torch.equal(x.reshape(y.shape), y) for x, y in zip(got, want))


def test_tiny_botnet_matches_the_cpu_path_and_trains():
    torch.manual_seed(0)
    cpu = SlimModel(slim_nets.resnext, 64, num_classes=10, name="resnext", blocks=(1, 1, 1, 2), cardinality=1,
                    base_width=8, mhsa_heads=2)  # block4: 64 channels, d = 32, L = 16 and 4
    gpu = copy.deepcopy(cpu).to(DEV)
    x = torch.randn(2, 64, 64, 3)
    with torch.no_grad():
        want = cpu(x, training=False)
        got = gpu(x.to(DEV, BF), training=False).cpu()
        # the bound of tests/test_se_gpu.py: the oracle's own sensitivity to a bf16-sized input perturbation
        g = torch.Generator().manual_seed(1)
        sens = _rel(cpu(x * (1 + 0.004 * torch.randn(x.shape, generator=g)), training=False), want.double())
    assert _rel(got, want.double()) < max(6e-2, 3 * sens)
    watched = {n: p.detach().clone() for n, p in gpu.named_parameters()
               if "mhsa" in n and n.endswith(("qkv_weights", "pos_h", "pos_w"))}
    assert len(watched) == 6
    step = TrainStep(gpu, optimizer="momentum", lr=0.05, momentum=0.9)
    for _ in range(2):
        loss = float(step(x.to(DEV, BF), torch.tensor([3, 7], device=DEV)))
    assert loss == loss and abs(loss) < 1e3
    now = dict(gpu.named_parameters())
    assert all(not torch.equal(now[n].detach(), old) for n, old in watched.items())
