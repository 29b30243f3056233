"""RandAugment on the GPU: dtm_randaugment against the numpy form of ops/randaugment.py bit for bit (every op at its
edges, sampled plans, statistics of changed images, the source and destination kinds, buffer placement), the
return codes, and the two device pipelines."""
import ctypes

import numpy as np
import pytest
import torch

import randaugment_cases as cases
from distributed_tensorflow_models_amd.data import cifar10
from distributed_tensorflow_models_amd.ops import _lib
from distributed_tensorflow_models_amd.ops import randaugment as ra
from distributed_tensorflow_models_amd.ops.randaugment import RandAugmentConfig, sample_plan

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64  # sentinel elements on each side of the source and of the destination
PLACEMENTS = [(0, 0), (1, 0), (0, 5), (5, 1)]  # element offsets of (source, destination) in their buffers
IN_AFFINE, OUT_AFFINE = (0.5, 0.5), (2.0 / 255.0, -1.0)
_SENT = {torch.uint8: 7, torch.float32: 7.0, torch.bfloat16: 7.0}


def _bits(t):
    return t.cpu().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def run_case(x_cpu, plan, off_x=0, off_out=0, out_kind="uint8", in_affine=(1.0, 0.0), out_affine=(1.0, 0.0)):
    """The call with x and out inside larger device buffers ([guard | offset | images | guard], the guards and the
    offset hold 7); checks that the source and the destination's guards are intact; returns the images (CPU)."""
    n = x_cpu.numel()
    odt = ra._KIND_DTYPE[ra._kind_name(out_kind)]
    bx = torch.full((GUARD + off_x + n + GUARD,), _SENT[x_cpu.dtype], dtype=x_cpu.dtype)
    sx = slice(GUARD + off_x, GUARD + off_x + n)
    bx[sx] = x_cpu.reshape(-1)
    bx_d = bx.to(DEV)
    bo_d = torch.full((GUARD + off_out + n + GUARD,), _SENT[odt], dtype=odt, device=DEV)
    so = slice(GUARD + off_out, GUARD + off_out + n)
    assert bx_d.data_ptr() % 16 == 0 and bo_d.data_ptr() % 16 == 0
    out = ra.randaugment(bx_d[sx].view(x_cpu.shape), plan.to(DEV), out_kind, in_affine, out_affine,
                         out=bo_d[so].view(x_cpu.shape))
    torch.cuda.synchronize()
    assert out.data_ptr() == bo_d.data_ptr() + so.start * out.element_size()
    assert torch.equal(_bits(bx_d), _bits(bx))  # the source, its guards included, is only read
    bo = bo_d.cpu()
    sent = torch.full((1,), _SENT[odt], dtype=odt)
    assert (_bits(bo[:so.start]) == _bits(sent)).all() and (_bits(bo[so.stop:]) == _bits(sent)).all()
    return bo[so].view(x_cpu.shape)


_ORACLE = {}


def oracle(key, x, plan):
    """The numpy form's uint8 result, computed once per (case, plan) and shared among the placements."""
    if key not in _ORACLE:
        _ORACLE[key] = torch.from_numpy(ra.apply_numpy(x, plan.rec))
    return _ORACLE[key]


def check_plans(tag, x, plans, off_x, off_out):
    xt = torch.from_numpy(x)
    for k, plan in enumerate(plans):
        got = run_case(xt, plan, off_x, off_out)
        want = oracle((tag, x.shape, k), x, plan)
        bad = (got != want).reshape(x.shape[0], -1).any(1).nonzero().reshape(-1).tolist()
        assert not bad, "%s plan %d: images %s differ (ops %s)" % (tag, k, bad, plan.op[bad].tolist())


# ---- every op at its edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_edge_plans(shape, placement):
    B, H, W = shape
    plans = cases.plans_of(cases.edge_records(H, W), B, H, W)
    check_plans("edge", cases.uniform_images(B, H, W), plans, *placement)


@pytest.mark.parametrize("placement", PLACEMENTS[:2])
@pytest.mark.parametrize("shape", cases.SHAPES + [cases.CLAMP_SHAPE])
def test_histogram_ops_on_crafted_images(shape, placement):
    """AutoContrast: a constant, a two-valued and a 0..255 channel; Equalize: a constant image, step == 0 and the
    clamp case; Contrast at every factor; narrow-range images (every pixel on four bins)."""
    B, H, W = shape
    recs = [cases.rec("AutoContrast"), cases.rec("Equalize")] + [cases.rec("Contrast", f=(f,)) for f in cases.FACTORS]
    plans = [ra.make_plan([[r]] * B, H, W) for r in recs]
    crafted = cases.clamp_images() if shape == cases.CLAMP_SHAPE else cases.histogram_images(B, H, W)
    check_plans("hist", crafted, plans, *placement)
    check_plans("narrow", cases.narrow_images(B, H, W), plans, *placement)


def test_equalize_clamp_case_reaches_the_clamp():
    x = cases.clamp_images()
    got = run_case(torch.from_numpy(x), ra.make_plan([[cases.rec("Equalize")]] * 2, 1, 600))
    assert (got[torch.from_numpy(x == 255)] == 255).all() and not torch.equal(got, torch.from_numpy(x))


# ---- sampled plans, statistics of changed images ------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_sampled_plans(shape, N):
    B, H, W = shape
    plans = cases.rotating_plans(B, H, W, N)
    for p in plans:  # every image of a layer on a different op
        for l in range(N):
            assert len({bytes(p.rec[b, l]) for b in range(B)}) == B or H * W == 1
    plans += [sample_plan(RandAugmentConfig(layers=N, fill=cases.FILL, seed=5), 1, bi, B, H, W) for bi in range(3)]
    off = PLACEMENTS[N % len(PLACEMENTS)]
    check_plans("sampled%d" % N, cases.normal_images(B, H, W), plans, *off)


@pytest.mark.parametrize("shape", [(3, 17, 23), (2, 33, 31), (2, 64, 48)])
def test_statistics_are_taken_at_the_input_of_their_layer(shape):
    B, H, W = shape
    x = cases.uniform_images(B, H, W, seed=3)
    x[..., 1] //= 2  # (a channel that Equalize and AutoContrast change)
    plans = cases.stats_order_plans(B, H, W)
    # Contrast after Solarize: the mean of the original image is another one, so a histogram taken from the wrong
    # buffer gives other bytes
    sol = ra.apply_numpy(x, plans[1].rec[:, :1])
    assert all(ra._grey(sol[b]).sum() // (H * W) != ra._grey(x[b]).sum() // (H * W) for b in range(B))
    check_plans("order", x, plans, 1, 5)


# ---- source and destination kinds ---------------------------------------------------------------------------------
def float_source(B, H, W, dtype, seed=0):
    """[-1, 1] values with some out of range, exact halves of the 8-bit grid, and NaN / Inf."""
    g = np.random.default_rng([seed, B, H, W, 9])
    y = g.uniform(-1.2, 1.2, (B, H, W, 3)).astype(np.float32)
    flat = y.reshape(-1)
    k = np.arange(flat.size)
    flat[k % 11 == 0] = (np.float32(2.0) * (g.integers(0, 255, flat.size) + np.float32(0.5)) / np.float32(255)
                         - np.float32(1))[k % 11 == 0]  # q lands on a half: rint to even
    flat[k % 37 == 5] = np.nan
    flat[k % 41 == 7] = np.inf
    flat[k % 43 == 9] = -np.inf
    flat[k % 47 == 3] = 3e38
    return torch.from_numpy(y).to(dtype)


@pytest.mark.parametrize("dst", ["uint8", "float32", "bfloat16"])
@pytest.mark.parametrize("src", [torch.uint8, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 17, 23), (2, 64, 48)])
def test_source_and_destination_kinds(shape, src, dst):
    B, H, W = shape
    x = torch.from_numpy(cases.uniform_images(B, H, W)) if src == torch.uint8 else float_source(B, H, W, src)
    plans = cases.rotating_plans(B, H, W, 1)[:3] + cases.rotating_plans(B, H, W, 2)[2:5] + \
        cases.stats_order_plans(B, H, W)[1:3] + [ra.identity_plan(B, 1, H, W)]
    for k, plan in enumerate(plans):
        off = PLACEMENTS[k % len(PLACEMENTS)]
        got = run_case(x, plan, off[0], off[1], dst, IN_AFFINE, OUT_AFFINE)
        want = ra.randaugment(x, plan, dst, IN_AFFINE, OUT_AFFINE)  # the CPU path: the numpy form
        assert got.dtype == want.dtype and torch.equal(_bits(got), _bits(want)), "plan %d" % k
    if src != torch.uint8:  # the quantisation alone, through the identity
        got = run_case(x, ra.identity_plan(B, 2, H, W), 1, 0, "uint8", IN_AFFINE)
        assert torch.equal(got, torch.from_numpy(ra.quantize_source(x.float().numpy(), *IN_AFFINE)))


# ---- repeatability, buffers ---------------------------------------------------------------------------------------
def test_same_call_twice_gives_the_same_bits_and_reuses_its_buffers():
    B, H, W = 2, 64, 48
    x = torch.from_numpy(cases.normal_images(B, H, W)).to(DEV)
    plan = cases.stats_order_plans(B, H, W)[3].to(DEV)
    a = ra.randaugment(x, plan, "bfloat16", out_affine=OUT_AFFINE)
    held = ra._BUFFERS[(x.device, B, H, W, 3)]
    ptrs = [t.data_ptr() for t in held]
    assert held[0].numel() == held[1].numel() == B * H * W * 3 and held[2].numel() == 3 * B * 4 * 256
    b = ra.randaugment(x, plan, "bfloat16", out_affine=OUT_AFFINE)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))
    assert [t.data_ptr() for t in ra._BUFFERS[(x.device, B, H, W, 3)]] == ptrs
    # another plan in between, on the same buffers, changes nothing
    ra.randaugment(x, cases.stats_order_plans(B, H, W)[2].to(DEV))
    c = ra.randaugment(x, plan, "bfloat16", out_affine=OUT_AFFINE)
    assert torch.equal(_bits(a), _bits(c))


# ---- return codes -------------------------------------------------------------------------------------------------
def test_return_codes_leave_the_destination_unwritten():
    L = _lib.lib()
    B, H, W, N = 2, 5, 7, 2
    n = B * H * W * 3
    x = torch.from_numpy(cases.uniform_images(B, H, W)).to(DEV)
    xf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    plan = ra.identity_plan(B, N, H, W).to(DEV)
    b0, b1 = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    scr = torch.zeros(N * B * 4 * 256, dtype=torch.int32, device=DEV)
    dst = torch.full((n * 4,), 7, dtype=torch.uint8, device=DEV)  # room for an fp32 destination

    def call(src=x.data_ptr(), sk=0, plan_p=plan.dev.data_ptr(), B=B, H=H, W=W, N=N, p0=b0.data_ptr(),
             p1=b1.data_ptr(), ps=scr.data_ptr(), pd=dst.data_ptr(), dk=0):
        P = ctypes.c_void_p
        return L.dtm_randaugment(P(src), sk, 1.0, 0.0, P(plan_p), B, H, W, N, P(p0), P(p1), P(ps), P(pd), dk, 1.0,
                                 0.0, _lib.stream_ptr())

    assert call(src=None) == -1 and call(plan_p=None) == -1 and call(p0=None) == -1 and call(p1=None) == -1
    assert call(ps=None) == -1 and call(pd=None) == -1
    assert call(src=xf.data_ptr() + 2, sk=1) == -1 and call(src=xf.data_ptr() + 1, sk=2) == -1
    assert call(pd=dst.data_ptr() + 2, dk=1) == -1 and call(pd=dst.data_ptr() + 1, dk=2) == -1
    assert call(B=0) == -2 and call(H=0) == -2 and call(W=-1) == -2
    assert call(H=65536, W=32768) == -2  # H * W == 2^31
    assert call(N=0) == -3 and call(N=-2) == -3
    torch.cuda.synchronize()
    assert (dst == 7).all() and not scr.any() and not b0.any()  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(dst[:n].view(B, H, W, 3), x) and (dst[n:] == 7).all()


# ---- wiring -------------------------------------------------------------------------------------------------------
def test_cifar_device_batch_is_the_hand_built_chain():
    cfg = RandAugmentConfig(layers=2, magnitude=7.0, seed=5)
    with_ra = cifar10.Cifar10Input("", 6, 24, device=DEV, seed=4, randaugment=cfg, rank=2)
    raw_src = cifar10.Cifar10Input("", 6, 24, device=DEV, seed=4)
    rng = np.random.RandomState(4)
    for bi in range(2):
        got, lab = with_ra.next_batch()
        raw, lab_raw = raw_src._raw_batch()
        plan = sample_plan(cfg, 2, bi, 6, 32, 32)
        mid = ra.randaugment(raw, plan.to(DEV))
        assert torch.equal(mid.cpu(), ra.randaugment(raw.cpu(), plan))  # the kernel, against the numpy form
        want = cifar10.augment(mid, 24, rng=rng, dtype=torch.bfloat16)
        assert got.dtype == torch.bfloat16 and got.is_cuda
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(lab, lab_raw)
    off = cifar10.Cifar10Input("", 6, 24, device=DEV, seed=4)
    before = set(ra._BUFFERS)
    off.next_batch()
    assert off.randaugment is None and set(ra._BUFFERS) == before  # off: no new buffer of it exists


def test_imagenet_prep_with_a_plan_equals_the_oracle_on_the_prep_output():
    from distributed_tensorflow_models_amd.data import imagenet, imagenet_gpu
    g = np.random.RandomState(3)
    images = [g.randint(0, 256, (40, 50, 3)).astype(np.uint8) for _ in range(3)]
    params = [imagenet.sample_params(40, 50, None, np.random.RandomState(10 + i), i, True) for i in range(3)]
    S = 16
    plan = ra.make_plan([[cases.rec("Equalize"), cases.rec("Affine", f=ra.rotate_matrix(30.0, S, S))],
                         [cases.rec("Sharpness", f=(1.7,)), cases.rec("AutoContrast")],
                         [cases.rec("Color", f=(0.3,)), cases.rec("Cutout", (2, 9, 5, 16))]], S, S)
    prep32, _ = imagenet_gpu.gpu_preprocess(images, params, S, DEV, torch.float32)
    got, _ = imagenet_gpu.gpu_preprocess(images, params, S, DEV, torch.bfloat16, randaugment=plan)
    torch.cuda.synchronize()
    want = ra.randaugment(prep32.cpu(), plan, "bfloat16", IN_AFFINE, OUT_AFFINE)
    assert got.dtype == torch.bfloat16 and got.shape == (3, S, S, 3)
    assert torch.equal(_bits(got), _bits(want))
    plain, _ = imagenet_gpu.gpu_preprocess(images, params, S, DEV, torch.bfloat16)
    assert not torch.equal(_bits(plain), _bits(got))


def test_imagenet_device_pipeline_batches_lie_on_the_8_bit_grid(tmp_path):
    """GPUBatchInputs with a config: the bf16 batch holds only values bf16(v * (2 / 255) - 1) of bytes v (the prep's
    own sums are fp32 atomics, so its batches are compared by this property, not bit for bit)."""
    import io

    from PIL import Image

    from distributed_tensorflow_models_amd.data import imagenet, imagenet_gpu
    from distributed_tensorflow_models_amd.data.tfrecord import TFRecordWriter, encode_example
    out = tmp_path / "data"
    out.mkdir()
    rng = np.random.RandomState(0)
    with TFRecordWriter(str(out / "train-00000-of-00001")) as w:
        for i in range(12):
            b = io.BytesIO()
            Image.fromarray((rng.rand(40 + i, 50, 3) * 255).astype(np.uint8)).save(b, format="JPEG")
            w.write(encode_example({"image/encoded": b.getvalue(), "image/class/label": i % 5 + 1}))
    ds = imagenet.ImagenetData("train", str(out))
    cfg = RandAugmentConfig(layers=2, seed=9)
    bi = imagenet_gpu.GPUBatchInputs(ds, 4, train=True, image_size=16, num_readers=1, num_decoders=2, seed=1,
                                     device=DEV, decode_processes=False, randaugment=cfg, rank=1)
    try:
        x, y = bi.next_batch()
        x2, _ = bi.next_batch()
        torch.cuda.synchronize()
    finally:
        bi.close()
    grid = (torch.arange(256, dtype=torch.float32) * np.float32(2.0 / 255.0) - 1.0).bfloat16()
    assert x.dtype == torch.bfloat16 and tuple(x.shape) == (4, 16, 16, 3) and bi.batch_index == 2
    for t in (x, x2):
        assert torch.isin(_bits(t).int(), _bits(grid).int()).all()
    ev = imagenet_gpu.GPUBatchInputs(ds, 4, train=False, image_size=16, num_readers=1, num_decoders=2, seed=1,
                                     device=DEV, decode_processes=False, randaugment=cfg)
    ev.close()
    assert ev.randaugment is None  # evaluation inputs are untouched
