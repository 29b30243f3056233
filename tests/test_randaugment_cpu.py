"""RandAugment on the CPU path: the numpy form of ops/randaugment.py against Pillow bit for bit and against
hand-computed cases, the sampler, the validation, the CIFAR pipeline and the trainer's flags."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import randaugment_cases as cases
from distributed_tensorflow_models_amd.data import cifar10
from distributed_tensorflow_models_amd.ops import randaugment as ra
from distributed_tensorflow_models_amd.ops.randaugment import RandAugmentConfig, sample_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributed_tensorflow_models_amd.trainers."


def one(img, op, i=(), f=()):
    """One record on one image through the public call."""
    plan = ra.make_plan([[cases.rec(op, i, f)]], img.shape[0], img.shape[1])
    return ra.randaugment(torch.from_numpy(img[None].copy()), plan).numpy()[0]


# ---- the oracle against Pillow ------------------------------------------------------------------------------------
def _pil_images():
    """Uniform random, narrow-range and clipped-normal images of sizes 1 x 1 to 39 x 39."""
    g = np.random.default_rng(11)
    out = []
    for k in range(120):
        H, W = (1, 1) if k == 0 else (39, 39) if k == 1 else (int(g.integers(1, 40)), int(g.integers(1, 40)))
        make = (cases.uniform_images, cases.narrow_images, cases.normal_images)[k % 3]
        out.append(make(1, H, W, seed=k)[0])
    return out


def _pil_factors():
    g = np.random.default_rng(12)
    return [0.0, 1.0] + [float(v) for v in g.uniform(0.1, 1.9, 4)]


def test_oracle_equals_pillow_bit_for_bit():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageOps

    def check(got, im, what):
        want = np.asarray(im)
        assert np.array_equal(got, want), "%s on %s: %d bytes differ" % (what, got.shape, (got != want).sum())

    factors = _pil_factors()
    for k, x in enumerate(_pil_images()):
        im = Image.fromarray(x, "RGB")
        check(one(x, "Invert"), ImageOps.invert(im), "Invert")
        check(one(x, "AutoContrast"), ImageOps.autocontrast(im), "AutoContrast")
        check(one(x, "Equalize"), ImageOps.equalize(im), "Equalize")
        bits = 1 + k % 8
        check(one(x, "Posterize", (bits,)), ImageOps.posterize(im, bits), "Posterize %d" % bits)
        thr = (0, 128, 256, 77)[k % 4]
        check(one(x, "Solarize", (thr,)), ImageOps.solarize(im, thr), "Solarize %d" % thr)
        for f in (factors[k % len(factors)], factors[(k + 1) % len(factors)]):
            for name, enh in (("Color", ImageEnhance.Color), ("Contrast", ImageEnhance.Contrast),
                              ("Brightness", ImageEnhance.Brightness), ("Sharpness", ImageEnhance.Sharpness)):
                check(one(x, name, f=(f,)), enh(im).enhance(f), "%s %r" % (name, f))


def test_sharpness_smoothing_and_blend_equal_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageFilter
    for k, x in enumerate(_pil_images()[:40]):
        im = Image.fromarray(x, "RGB")
        smooth = im.filter(ImageFilter.SMOOTH)
        assert np.array_equal(ra._sharp_smooth(x), np.asarray(smooth))
        f = (0.25, 0.5, 0.75, 1.0)[k % 4]
        other = Image.fromarray(cases.uniform_images(1, x.shape[0], x.shape[1], seed=1000 + k)[0], "RGB")
        want = np.asarray(Image.blend(other, im, f))
        assert np.array_equal(ra._blend(np.asarray(other), x, np.float32(f)), want)


def test_equalize_clamp_case_equals_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageOps
    x = cases.clamp_images()[0]
    h = np.bincount(x[..., 0].reshape(-1), minlength=256)
    step = (600 - h[255]) // 255
    assert (step // 2 + 600 - h[255]) // step > 255  # the last LUT entry exceeds 255 before the clamp
    got = one(x, "Equalize")
    assert np.array_equal(got, np.asarray(ImageOps.equalize(Image.fromarray(x, "RGB"))))
    assert got[x == 255].tolist() == [255] * int((x == 255).sum())


# ---- the oracle against hand-computed cases -----------------------------------------------------------------------
def _img(rows):
    """[H][W] grey values -> an image whose channels are v, v + 1, v + 2"""
    v = np.array(rows, dtype=np.int64)
    return np.stack([v, v + 1, v + 2], -1).astype(np.uint8)


def test_point_ops_by_hand():
    x = _img([[0, 100, 127], [128, 200, 253]])
    assert np.array_equal(one(x, "Identity"), x)
    assert one(x, "Invert")[0, 1].tolist() == [155, 154, 153]
    assert one(x, "Posterize", (0,)).max() == 0
    assert one(x, "Posterize", (3,))[1, 1].tolist() == [192, 192, 192]  # 200, 201, 202 & 0xe0
    assert np.array_equal(one(x, "Posterize", (8,)), x)
    assert one(x, "Solarize", (128,))[..., 0].tolist() == [[0, 100, 127], [127, 55, 2]]
    assert np.array_equal(one(x, "Solarize", (256,)), x)
    assert np.array_equal(one(x, "Solarize", (0,)), 255 - x)
    assert one(x, "SolarizeAdd", (200,))[..., 0].tolist() == [[200, 255, 255], [128, 200, 253]]
    assert np.array_equal(one(x, "SolarizeAdd", (0,)), x)
    assert one(x, "Brightness", f=(0.5,))[..., 0].tolist() == [[0, 50, 63], [64, 100, 126]]
    assert one(x, "Brightness", f=(1.9,))[1, 1].tolist() == [255, 255, 255]
    assert one(x, "Brightness", f=(0.0,)).max() == 0


def test_autocontrast_and_equalize_by_hand():
    x = np.zeros((2, 2, 3), dtype=np.uint8)
    x[..., 0] = 7                       # a constant channel: unchanged
    x[..., 1] = [[50, 150], [50, 150]]  # two values: to 0 and 255
    x[..., 2] = [[0, 85], [170, 255]]   # the full range: scale 1
    got = one(x, "AutoContrast")
    assert got[..., 0].tolist() == [[7, 7], [7, 7]]
    assert got[..., 1].tolist() == [[0, 255], [0, 255]]
    assert got[..., 2].tolist() == [[0, 85], [170, 255]]
    assert np.array_equal(one(x, "Equalize"), x)  # 4 pixels: step == 0
    # 1 x 512: value v < 255 twice, 255 twice: step = 510 // 255 = 2, lut[v] = (1 + 2 v) // 2 = v
    ramp = np.repeat(np.arange(256), 2).astype(np.uint8).reshape(1, 512)
    y = np.stack([ramp, ramp // 2, np.full_like(ramp, 3)], -1)
    got = one(y, "Equalize")
    assert np.array_equal(got[..., 0], ramp)
    # channel 1: values 0..127 four times: step = (512 - 4) // 255 = 1, lut[v] = min(255, 4 v)
    assert np.array_equal(got[..., 1], np.minimum(255, 4 * (ramp // 2).astype(np.int64)))
    assert np.array_equal(got[..., 2], y[..., 2])  # one bin


def test_color_and_contrast_by_hand():
    x = np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [10, 20, 30]]], dtype=np.uint8)
    # grey: 76 (19595 * 255 + 32768 >> 16), 150, 29, 18
    assert ra._grey(x).tolist() == [[76, 150], [29, 18]]
    assert one(x, "Color", f=(0.0,)).tolist() == [[[76] * 3, [150] * 3], [[29] * 3, [18] * 3]]
    assert np.array_equal(one(x, "Color", f=(1.0,)), x)
    assert one(x, "Color", f=(0.5,))[0, 0].tolist() == [165, 38, 38]  # 76 + 0.5 * 179 = 165.5, 76 - 38 = 38
    # the mean grey: (2 * 273 + 4) // 8 = 68
    assert one(x, "Contrast", f=(0.0,)).tolist() == [[[68] * 3] * 2] * 2
    assert one(x, "Contrast", f=(0.5,))[1, 1].tolist() == [39, 44, 49]
    assert one(x, "Contrast", f=(1.9,))[0, 0].tolist() == [255, 0, 0]


def test_sharpness_by_hand():
    v = [[10, 20, 30], [40, 50, 60], [70, 80, 200]]
    x = _img(v)
    # the one interior pixel: (5 * 50 + 10 + 20 + 30 + 40 + 60 + 70 + 80 + 200 + 6) // 13 = 58
    got = one(x, "Sharpness", f=(0.0,))
    assert got[1, 1].tolist() == [58, 59, 60]
    got[1, 1] = x[1, 1]
    assert np.array_equal(got, x)  # the border keeps its bytes
    assert one(x, "Sharpness", f=(1.9,))[1, 1, 0] == 42  # 58 + 1.9 * (50 - 58) = 42.8
    for shape in ((2, 5), (5, 2), (1, 1)):  # H or W below 3: all border
        y = cases.uniform_images(1, *shape)[0]
        assert np.array_equal(one(y, "Sharpness", f=(0.3,)), y)


def test_affine_by_hand():
    x = cases.uniform_images(1, 3, 5)[0]
    fill = np.array(cases.FILL, dtype=np.uint8)
    assert np.array_equal(one(x, "Affine", f=(1, 0, 0, 0, 1, 0)), x)  # the identity matrix: a bit copy
    assert (one(x, "Affine", f=(1, 0, 5, 0, 1, 0)) == fill).all()     # a translation by W fills everything
    assert (one(x, "Affine", f=(1, 0, -5, 0, 1, 0)) == fill).all()
    got = one(x, "Affine", f=(1, 0, 1, 0, 1, 0))                      # xin = x + 1: the image moves left
    assert np.array_equal(got[:, :4], x[:, 1:]) and (got[:, 4] == fill).all()
    got = one(x, "Affine", f=(1, 0, 0, 0, 1, -1))                     # yin = y - 1: the image moves down
    assert np.array_equal(got[1:], x[:2]) and (got[0] == fill).all()
    # a rotation by 90 degrees about (2.5, 1.5): xin = yf + 1, yin = 4 - xf (c = 6e-17 changes nothing), so the
    # output pixel (x, y) reads the input pixel (y + 1, 3 - x) where that lies inside the 3 x 5 image
    got = one(x, "Affine", f=ra.rotate_matrix(90.0, 3, 5))
    want = np.empty_like(x)
    for y in range(3):
        for xx in range(5):
            sx, sy = y + 1, 3 - xx
            want[y, xx] = x[sy, sx] if 0 <= sy < 3 else fill
    assert np.array_equal(got, want)
    assert (one(x, "Affine", f=(1e30, -1e30, 1e30, 1e30, 1e30, -1e30)) == fill).all()


def test_cutout_by_hand():
    x = cases.uniform_images(1, 4, 6)[0]
    fill = np.array(cases.FILL, dtype=np.uint8)
    assert np.array_equal(one(x, "Cutout", (2, 2, 0, 6)), x)
    assert (one(x, "Cutout", (0, 4, 0, 6)) == fill).all()
    got = one(x, "Cutout", (1, 3, 4, 6))
    assert (got[1:3, 4:6] == fill).all()
    got[1:3, 4:6] = x[1:3, 4:6]
    assert np.array_equal(got, x)


def test_layers_apply_in_order_and_kinds():
    x = cases.uniform_images(2, 6, 5)
    plan = ra.make_plan([[cases.rec("Solarize", (100,)), cases.rec("Contrast", f=(1.5,))],
                         [cases.translate(2, 0), cases.rec("Equalize")]], 6, 5)
    want = np.stack([ra.apply_record(ra.apply_record(x[b], plan.rec[b, 0]), plan.rec[b, 1]) for b in range(2)])
    assert np.array_equal(ra.randaugment(torch.from_numpy(x), plan).numpy(), want)
    assert not np.array_equal(want[0], ra.apply_record(ra.apply_record(x[0], plan.rec[0, 1]), plan.rec[0, 0]))
    # a float source is quantised on read, q(y) = rint(clamp((y * 0.5 + 0.5) * 255)); 0.5 rounds to even; NaN is 0
    y = torch.tensor([-1.0, 1.0, 0.0, -3.0, 7.0, float("nan"), 1.0 / 255.0, -1.0 + 5.0 / 255.0, 0.2],
                     dtype=torch.float32)
    q = ra.quantize_source(y.numpy(), 0.5, 0.5)
    assert q.tolist() == [0, 255, 128, 0, 255, 0, 128, 2, 153]
    ident = ra.identity_plan(1, 2, 1, 3)
    src = y.view(1, 1, 3, 3)
    assert ra.randaugment(src, ident, in_affine=(0.5, 0.5)).reshape(-1).tolist() == q.tolist()
    assert ra.randaugment(src.bfloat16(), ident, in_affine=(0.5, 0.5)).reshape(-1).tolist() == \
        ra.quantize_source(src.bfloat16().float().numpy(), 0.5, 0.5).reshape(-1).tolist()
    # float destinations: float(v) * s + b in fp32, bf16 rounded to nearest even
    s, b = np.float32(2.0 / 255.0), np.float32(-1.0)
    out32 = ra.randaugment(src, ident, out_kind="float32", in_affine=(0.5, 0.5), out_affine=(2.0 / 255.0, -1.0))
    assert out32.dtype == torch.float32
    assert np.array_equal(out32.numpy().reshape(-1), q.astype(np.float32) * s + b)
    out16 = ra.randaugment(src, ident, out_kind=torch.bfloat16, in_affine=(0.5, 0.5), out_affine=(2.0 / 255.0, -1.0))
    assert out16.dtype == torch.bfloat16 and torch.equal(out16, out32.bfloat16())
    into = torch.empty(1, 1, 3, 3, dtype=torch.bfloat16)
    assert ra.randaugment(src, ident, "bfloat16", (0.5, 0.5), (2.0 / 255.0, -1.0), out=into) is into
    assert torch.equal(into, out16)


# ---- the sampler --------------------------------------------------------------------------------------------------
def test_plan_is_a_pure_function_of_its_arguments():
    cfg = RandAugmentConfig(layers=2, seed=3)
    base = sample_plan(cfg, 1, 5, 16, 12, 10)
    again = sample_plan(RandAugmentConfig(layers=2, seed=3), 1, 5, 16, 12, 10)
    assert base.rec.dtype == np.int32 and base.rec.shape == (16, 2, 12) and np.array_equal(base.rec, again.rec)
    for other in (sample_plan(RandAugmentConfig(layers=2, seed=4), 1, 5, 16, 12, 10),
                  sample_plan(cfg, 2, 5, 16, 12, 10), sample_plan(cfg, 1, 6, 16, 12, 10)):
        assert not np.array_equal(base.rec, other.rec)
    dev = base.to("cpu").dev
    assert dev.dtype == torch.int32 and np.array_equal(dev.numpy(), base.rec)


def test_prob_zero_is_the_identity_plan():
    p = sample_plan(RandAugmentConfig(layers=3, prob=0.0, seed=1), 0, 0, 8, 9, 7)
    assert np.array_equal(p.rec, ra.identity_plan(8, 3, 9, 7).rec)
    half = sample_plan(RandAugmentConfig(layers=1, prob=0.5, ops="Invert", seed=1), 0, 0, 400, 4, 4)
    kept = int((half.op == ra.INVERT).sum())
    assert 140 < kept < 260 and kept + int((half.op == ra.IDENTITY).sum()) == 400


@pytest.mark.parametrize("M", [0.0, 5.0, 10.0])
def test_argument_table(M):
    H, W, m = 20, 30, M / 10
    cfg = RandAugmentConfig(layers=1, magnitude=M, ops=ra.SAMPLER_OPS, seed=2)
    f32 = lambda *v: np.array(v, dtype=np.float64).astype(np.float32)  # noqa: E731
    seen = set()
    for bi in range(6):
        cfg.seed = 2 + bi
        g = np.random.default_rng([cfg.seed, 0, bi])
        op, u, neg = g.integers(0, 17, (64, 1)), g.random((64, 1)), g.integers(0, 2, (64, 1))
        cy, cx = g.random((64, 1)), g.random((64, 1))  # y before x
        p = sample_plan(cfg, 0, bi, 64, H, W)
        assert (p.rec[:, :, 11] == (128 | 128 << 8 | 128 << 16)).all()
        for b in range(64):
            name, sg = ra.SAMPLER_OPS[op[b, 0]], -1.0 if neg[b, 0] else 1.0
            seen.add(name)
            o, i, f = int(p.op[b, 0]), p.iargs[b, 0].tolist(), p.fargs[b, 0]
            if name in ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY"):
                assert o == ra.AFFINE
                if name == "Rotate":
                    a = math.radians(sg * 30.0 * m)
                    c, s = math.cos(a), math.sin(a)
                    want = f32(c, s, 15 - c * 15 - s * 10, -s, c, 10 + s * 15 - c * 10)
                elif name == "ShearX":
                    want = f32(1, sg * 0.3 * m, 0, 0, 1, 0)
                elif name == "ShearY":
                    want = f32(1, 0, 0, sg * 0.3 * m, 1, 0)
                elif name == "TranslateX":
                    want = f32(1, 0, sg * int(m * 0.45 * W), 0, 1, 0)
                else:
                    want = f32(1, 0, 0, 0, 1, sg * int(m * 0.45 * H))
                assert np.array_equal(f, want), (name, f, want)
            elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
                assert o == ra.OP_ID[name] and f[0] == np.float32(0.1 + 1.8 * m)
            elif name == "Posterize":
                assert (o, i[0]) == (ra.POSTERIZE, 8 - int(4 * m))
            elif name == "Solarize":
                assert (o, i[0]) == (ra.SOLARIZE, 256 - int(256 * m))
            elif name == "SolarizeAdd":
                assert (o, i[0]) == (ra.SOLARIZE_ADD, int(110 * m))
            elif name == "Cutout":
                pad = int(m * 0.18 * min(H, W))
                yc, xc = int(cy[b, 0] * H), int(cx[b, 0] * W)
                assert o == ra.CUTOUT
                assert i == [max(0, yc - pad), min(H, yc + pad), max(0, xc - pad), min(W, xc + pad)]
            else:
                assert o == ra.OP_ID[name] and not p.rec[b, 0, 1:11].any()
    assert seen == set(ra.SAMPLER_OPS)


def test_every_default_op_occurs_and_every_sampled_plan_validates():
    cfg = RandAugmentConfig(layers=2, seed=7)
    assert cfg.ops == ra.DEFAULT_OPS and len(cfg.ops) == 14 and cfg.magnitude == 9.0 and cfg.prob == 1.0
    assert RandAugmentConfig().layers == 0
    seen = {}
    for bi in range(10):  # 10 x 100 x 2 = 2000 records
        g = np.random.default_rng([7, 3, bi])
        names = np.array(cfg.ops)[g.integers(0, 14, (100, 2))]
        p = sample_plan(cfg, 3, bi, 100, 24, 32)
        p._checked = False
        p.validate()
        for name, o in zip(names.reshape(-1), p.op.reshape(-1)):
            seen.setdefault(name, set()).add(int(o))
    assert set(seen) == set(ra.DEFAULT_OPS)
    geometric = ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY")
    assert all(seen[n] == {ra.AFFINE if n in geometric else ra.OP_ID[n]} for n in seen)
    for ops, M in (("Cutout,SolarizeAdd,Invert", 10.0), (ra.SAMPLER_OPS, 0.0), (ra.SAMPLER_OPS, 10.0)):
        for shape in ((1, 1), (3, 2), (299, 299)):
            p = sample_plan(RandAugmentConfig(layers=3, magnitude=M, ops=ops, seed=1), 0, 0, 32, *shape)
            p._checked = False
            p.validate()


# ---- validation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [
    cases.rec(13), cases.rec(-1), cases.rec("Posterize", (9,)), cases.rec("Posterize", (-1,)),
    cases.rec("Solarize", (257,)), cases.rec("Solarize", (-1,)), cases.rec("SolarizeAdd", (256,)),
    cases.rec("SolarizeAdd", (-1,)), cases.rec("Cutout", (3, 2, 0, 1)), cases.rec("Cutout", (0, 7, 0, 1)),
    cases.rec("Cutout", (-1, 2, 0, 1)), cases.rec("Cutout", (0, 1, 4, 3)), cases.rec("Cutout", (0, 1, 0, 9)),
    cases.rec("Color", f=(float("nan"),)), cases.rec("Affine", f=(1, 0, float("inf"), 0, 1, 0)),
    cases.rec("Affine", f=(1, 0, 0, 0, 1, float("-inf"))), cases.rec("Identity", f=(0, 0, 0, 0, 0, float("nan")))])
def test_validation_of_the_host_copy(bad):
    x = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    good = cases.rec("Cutout", (0, 6, 0, 8))
    ra.make_plan([[good], [good]], 6, 8).validate()
    for rows in ([[bad], [good]], [[good, good], [good, bad]]):
        with pytest.raises(ValueError):
            ra.randaugment(x, ra.make_plan(rows, 6, 8))


def test_bad_calls_and_configs_raise():
    x = torch.zeros(2, 6, 8, 3, dtype=torch.uint8)
    plan = ra.identity_plan(2, 1, 6, 8)
    for bad_x in (x[:1], x[:, :5], x.permute(0, 2, 1, 3), torch.zeros(2, 6, 8, 4, dtype=torch.uint8), x.int()):
        with pytest.raises(ValueError):
            ra.randaugment(bad_x, plan)
    with pytest.raises(ValueError):
        ra.randaugment(x, plan, out=x)  # overlapping
    with pytest.raises(ValueError):
        ra.randaugment(x, plan, out_kind="int8")
    with pytest.raises(ValueError):
        ra.RandAugmentPlan(np.zeros((2, 12), np.int32), 6, 8)
    for kw in (dict(magnitude=10.5), dict(magnitude=-1), dict(prob=1.5), dict(prob=-0.1), dict(ops="Rotate,Twirl"),
               dict(layers=-1), dict(fill=(1, 2, 256)), dict(seed=-1), dict(translate_ratio=2.0)):
        with pytest.raises(ValueError):
            RandAugmentConfig(**kw)
    with pytest.raises(ValueError):
        sample_plan(RandAugmentConfig(layers=0), 0, 0, 4, 8, 8)


# ---- pipelines and trainer ----------------------------------------------------------------------------------------
def test_cifar_input_with_a_config_is_the_hand_built_chain():
    cfg = RandAugmentConfig(layers=2, magnitude=7.0, seed=5)
    with_ra = cifar10.Cifar10Input("", 6, 24, seed=4, randaugment=cfg, rank=2)
    raw_src = cifar10.Cifar10Input("", 6, 24, seed=4)
    plain = cifar10.Cifar10Input("", 6, 24, seed=4)
    assert with_ra.synthetic and plain.randaugment is None
    rng_hand, rng_plain = np.random.RandomState(4), np.random.RandomState(4)
    for bi in range(3):
        got, lab = with_ra.next_batch()
        raw, lab_raw = raw_src._raw_batch()
        plan = sample_plan(cfg, 2, bi, 6, 32, 32)
        mid = ra.randaugment(raw, plan)
        assert mid.dtype == torch.uint8 and not torch.equal(mid, raw)
        want = cifar10.augment(mid, 24, rng=rng_hand, dtype=torch.float32)
        assert torch.equal(got, want) and torch.equal(lab, lab_raw)
        # without a config: today's path, bit for bit
        got_plain, _ = plain.next_batch()
        assert torch.equal(got_plain, cifar10.augment(raw, 24, rng=rng_plain, dtype=torch.float32))
    assert with_ra.batch_index == 3
    # evaluation inputs are untouched, and 0 layers is off
    ev = cifar10.inputs(True, "", 6, 24, seed=4, randaugment=cfg)
    off = cifar10.distorted_inputs("", 6, 24, seed=4, randaugment=RandAugmentConfig(layers=0))
    assert ev.randaugment is None and off.randaugment is None
    assert torch.equal(ev.next_batch()[0], cifar10.inputs(True, "", 6, 24, seed=4).next_batch()[0])


def _trainer(mod, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", PKG + mod] + list(args), cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=600)


COMMON = ["--batch_size=8", "--data_dir=/nonexistent", "--seed=3"]


def test_trainer_cifar_run_writes_the_metrics_fields(tmp_path):
    d, mf = str(tmp_path / "train"), str(tmp_path / "metrics.jsonl")
    p = _trainer("cifar10_cnn_bsp", "--train_dir=" + d, "--max_steps=3", "--randaugment_layers=2",
                 "--randaugment_magnitude=5", "--metrics_file=" + mf, *COMMON)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    recs = [json.loads(line) for line in open(mf)]
    assert [r["global_step"] for r in recs] == [1, 2, 3]
    for r in recs:
        assert r["randaugment_layers"] == 2 and r["randaugment_magnitude"] == 5.0 and np.isfinite(r["loss"])


@pytest.mark.parametrize("mod,args,msg", [
    ("mnist_lenet_bsp", ["--randaugment_layers=2"], "needs a dataset of uint8 images"),
    ("imagenet_resnet50_bsp", ["--randaugment_layers=1", "--synthetic_data"], "needs a dataset of uint8 images"),
    ("cifar10_cnn_bsp", ["--randaugment_layers=2", "--randaugment_ops=Rotate,Twirl"], "unknown randaugment op"),
    ("cifar10_cnn_bsp", ["--randaugment_layers=2", "--randaugment_magnitude=11"], "magnitude must lie in [0, 10]"),
    ("cifar10_cnn_bsp", ["--randaugment_layers=2", "--randaugment_prob=1.5"], "prob must lie in [0, 1]"),
])
def test_trainer_start_up_errors(tmp_path, mod, args, msg):
    p = _trainer(mod, "--train_dir=%s" % (tmp_path / "t"), "--max_steps=2", *args, *COMMON)
    assert p.returncode != 0
    assert "ValueError" in p.stderr and msg in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "t").exists()  # refused at start-up, before anything was set up


def _tiny_imagenet(tmp_path, n=12):
    import io

    from PIL import Image

    from distributed_tensorflow_models_amd.data import imagenet
    from distributed_tensorflow_models_amd.data.tfrecord import TFRecordWriter, encode_example
    out = tmp_path / "data"
    out.mkdir()
    rng = np.random.RandomState(0)
    with TFRecordWriter(str(out / "train-00000-of-00001")) as w:
        for i in range(n):
            b = io.BytesIO()
            Image.fromarray((rng.rand(40 + i, 50, 3) * 255).astype(np.uint8)).save(b, format="JPEG")
            w.write(encode_example({"image/encoded": b.getvalue(), "image/class/label": i % 5 + 1}))
    return imagenet.ImagenetData("train", str(out))


def test_imagenet_host_pipeline_runs_the_same_call_on_the_cpu_batch(tmp_path):
    pytest.importorskip("PIL")
    from distributed_tensorflow_models_amd.data import imagenet
    ds = _tiny_imagenet(tmp_path)
    cfg = RandAugmentConfig(layers=2, seed=9)
    kw = dict(num_preprocess_threads=1, image_size=16, num_readers=1, seed=2)  # one reader, one thread: one order
    plain = imagenet.distorted_inputs(ds, 4, **kw)
    with_ra = imagenet.distorted_inputs(ds, 4, randaugment=cfg, rank=3, **kw)
    try:
        for bi in range(2):
            x, y = plain.next_batch()
            got, y2 = with_ra.next_batch()
            want = ra.randaugment(x, sample_plan(cfg, 3, bi, 4, 16, 16), "float32", (0.5, 0.5), (2.0 / 255.0, -1.0))
            assert got.dtype == torch.float32 and torch.equal(got, want) and torch.equal(y, y2)
            assert not torch.equal(got, x)
        assert with_ra.batch_index == 2 and plain.randaugment is None
        ev = imagenet.inputs(ds, 4, 1, 16, seed=2, randaugment=cfg)
        ev.close()
        assert ev.randaugment is None  # evaluation inputs are untouched
    finally:
        plain.close()
        with_ra.close()
