"""The torch integer form of ops/int8.py (the kernels' oracle) against a literal loop in exact arithmetic and against
F.conv2d on fp64; the integer configuration's validation; a 3-layer slim net against a hand-composed chain; the
evaluator's --quant_int8 flag."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import pytest
import torch

from distributed_tensorflow_models_amd.compat import quantize as Q
from distributed_tensorflow_models_amd.ops import fakequant as FQ
from distributed_tensorflow_models_amd.ops import int8
from distributed_tensorflow_models_amd.ops.geometry import conv_geom
from int8_cases import layer, tiny_input, tiny_model

ACTS = {None: lambda r: r, "relu": lambda r: max(r, 0.0), "relu6": lambda r: min(max(r, 0.0), 6.0)}


def _f32(fr):
    """A rational rounded once to fp32 (nearest, ties to even; normal range)."""
    if fr == 0:
        return 0.0
    e = 0
    while Fraction(2) ** e > abs(fr):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(fr):
        e += 1
    m = abs(fr) / Fraction(2) ** (e - 23)
    n, rem = divmod(m.numerator, m.denominator)
    if 2 * rem > m.denominator or (2 * rem == m.denominator and n & 1):
        n += 1
    return (-1.0 if fr < 0 else 1.0) * n * 2.0 ** (e - 23)


def _t32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@pytest.mark.parametrize("depthwise,H,stride,act,za,zw", [
    (False, 5, 2, None, 0, 1), (False, 6, 2, "relu", 37, 128), (False, 5, 1, "relu6", 255, 255),
    (True, 5, 1, "relu6", 37, 1), (True, 6, 2, None, 255, 128)])
def test_cpu_form_literal(depthwise, H, stride, act, za, zw):
    C, K = (5, 5) if depthwise else (3, 4)
    a, w, bias, ra, rw, ro = layer(11, 2, H, H, C, K, 3, 3, za, zw, depthwise)
    qw = int8.prepare_weights(w, rw, depthwise)
    fn = int8.depthwise_q8 if depthwise else int8.conv2d_q8
    codes, deq = fn(a, ra, qw, bias, ro, stride, "SAME", act, torch.float32)
    g = conv_geom(tuple(a.shape), (K, 3, 3, C), stride, "SAME")
    fa, fw, fo = (r.view(torch.float32) for r in (ra, rw, ro))
    wc = (torch.round(w / fw[0]) + zw).long()  # (layer() built w from these codes)
    assert torch.equal(qw.codes.long(), wc)
    t = _t32(float(fa[0]) * float(fw[0]))  # (the fp64 product of two fp32 values is exact)
    # F.conv2d on fp64 (exact below 2^53) gives the accumulators a second way
    x64 = torch.nn.functional.pad((a.double() - za).permute(0, 3, 1, 2), (g.pad_w, g.pad_r, g.pad_h, g.pad_b))
    w64 = (wc.double() - zw)
    w64 = w64.permute(2, 0, 1).unsqueeze(1) if depthwise else w64.permute(0, 3, 1, 2)
    acc64 = torch.nn.functional.conv2d(x64, w64, stride=stride, groups=C if depthwise else 1).permute(0, 2, 3, 1)
    for n in range(2):
        for p in range(g.P):
            for q in range(g.Q):
                for k in range(K):
                    acc = 0
                    for r in range(3):
                        for s in range(3):
                            ih, iw = p * stride - g.pad_h + r, q * stride - g.pad_w + s
                            if 0 <= ih < H and 0 <= iw < H:
                                for c in ([k] if depthwise else range(C)):
                                    wv = wc[r, s, c] if depthwise else wc[k, r, s, c]
                                    acc += (int(a[n, ih, iw, c]) - za) * (int(wv) - zw)
                    assert acc == int(acc64[n, p, q, k])
                    r32 = ACTS[act](_f32(Fraction(_f32(Fraction(acc))) * Fraction(t) + Fraction(float(bias[k]))))
                    code = min(max(round(_t32(r32 * float(fo[1]))) + 100, 0), 255)  # (round(): ties to even)
                    assert int(codes[n, p, q, k]) == code
                    assert float(deq[n, p, q, k]) == _t32((code - 100) * float(fo[0]))


def test_config_validation():
    for kw in (dict(fused=False, is_training=False), dict(fused=True, is_training=True), dict(fused=True)):
        with pytest.raises(ValueError):
            Q.QuantConfig(integer=True, **kw)
    assert Q.QuantConfig(integer=True, fused=True, is_training=False).integer
    with pytest.raises(ValueError):
        int8.prepare_weights(torch.zeros(2, 1, 1, 32784), layer(0, 1, 1, 1, 1, 1, 1, 1, 0, 1)[4])


def test_slim_net_equals_composed_chain():
    m = tiny_model()
    x = tiny_input(m)
    int8.reset_layers()
    with torch.no_grad():
        y = m(x, training=False)
    assert int8.layers_run() == 3 and y.q8[0].dtype == torch.uint8
    v = m.store.vars
    codes, r_in = x.q8[0], x.q8[1].rec
    for scope, dw in (("t/dw1", 2), ("t/dw2", 1), ("t/pw", 0)):
        w = v[scope + ("/depthwise_weights" if dw else "/weights")].detach()
        bn = {n: v["%s/BatchNorm/%s" % (scope, n)].detach() for n in ("gamma", "beta", "moving_mean", "moving_variance")}
        mult = torch.rsqrt(bn["moving_variance"] + 0.001) * bn["gamma"]
        wf = w * (mult.reshape(1, 1, -1, 1) if dw else mult.reshape(-1, 1, 1, 1))
        r_w = FQ.state_of(v[scope + ("/depthwise_weights_q" if dw else "") + "/weights_quant/min"]).rec
        r_o = FQ.state_of(v[scope + "/act_quant/min"]).rec
        qw = int8.prepare_weights(wf, r_w, depthwise=bool(dw))
        fn = int8.depthwise_q8 if dw else int8.conv2d_q8
        codes, deq = fn(codes, r_in, qw, bn["beta"] - bn["moving_mean"] * mult, r_o, dw or 1, "SAME", "relu6",
                        torch.float32)
        r_in = r_o
    assert torch.equal(codes, y.q8[0]) and torch.equal(deq, y)
    assert len(torch.unique(codes)) > 20  # (a live net, not saturated codes)


def test_evaluator_quant_int8(tmp_path):
    """mobilenet_v1_train writes a tiny fake-quant checkpoint; mobilenet_v1_eval --quantize --quant_int8 evaluates it
    with 26 integer layers and says so on the result line and in the metrics file."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d, mf = str(tmp_path / "train"), str(tmp_path / "eval.jsonl")
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    common = ["--quantize", "--batch_size=2", "--synthetic_data", "--depth_multiplier=0.25", "--data_dir=/nonexistent"]
    for mod, args in (("mobilenet_v1_train", ["--max_steps=1", "--train_dir=" + d]),
                      ("mobilenet_v1_eval", ["--quant_int8", "--run_once", "--num_examples=2", "--checkpoint_dir=" + d,
                                             "--eval_dir=" + str(tmp_path / "eval"), "--metrics_file=" + mf])):
        p = subprocess.run([sys.executable, "-m", "distributed_tensorflow_models_amd.trainers." + mod] + common + args,
                           cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert "int8_layers = 26" in p.stdout
    lines = [json.loads(l) for l in open(mf) if l.startswith("{")]
    assert lines[-1]["int8_layers"] == 26
