"""RandAugment (Cubuk et al. 2020) on uint8 NHWC batches: a host sampler, one device record per image and layer, the
kernels of csrc/kernels/randaugment.hip, and the numpy form of the same definitions.

A **plan** is an int32[B][N][12] array: one record per image and layer, the layers applied in order.  A record is

    [op, i0, i1, i2, i3, bits(f0), ..., bits(f5), fill]      (f0..f5 are float32 bit patterns; fill = r | g<<8 | b<<16)

  0  Identity       the bytes
  1  AutoContrast   per channel, lo / hi = first / last non-empty bin; hi <= lo: unchanged; else in fp64, each operation
                    rounded on its own: scale = 255 / (hi - lo), offset = -lo * scale,
                    lut[v] = clamp(trunc(v * scale + offset), 0, 255)                              (Pillow's form)
  2  Equalize       per channel, nz = the non-empty bins; fewer than two: unchanged; step = (sum(nz) - nz[-1]) // 255;
                    step == 0: unchanged; else lut[v] = min(255, (step // 2 + sum_{u<v} h[u]) // step)
  3  Invert         255 - v
  4  Posterize      i0 = bits in [0, 8]: v & ~((1 << (8 - bits)) - 1)
  5  Solarize       i0 = thr in [0, 256]: v if v < thr else 255 - v
  6  SolarizeAdd    i0 = add in [0, 255]: min(255, v + add) if v < 128 else v
  7  Color          blend(grey, v, f0), grey the pixel's grey value
  8  Contrast       blend(m, v, f0), m = (2 * S + n) // (2 * n), S the sum of the image's grey values, n = H * W
  9  Brightness     blend(0, v, f0)
  10 Sharpness      blend(d, v, f0): d = v on the outermost rows and columns, elsewhere (s + 6) // 13 with s the 3x3 sum
                    of the channel, weight 5 at the centre and 1 for the other eight
  11 Affine         output pixel (x, y), xf = x + 0.5f, yf = y + 0.5f, in fp32 operation by operation:
                    xin = (f0 * xf + f1 * yf) + f2, yin = (f3 * xf + f4 * yf) + f5;
                    0 <= xin < W and 0 <= yin < H (tested on the floats: false for NaN): the input pixel at
                    (floor(yin), floor(xin)); else the fill colour
  12 Cutout         i0..i3 = y0, y1, x0, x1: the fill colour inside [y0, y1) x [x0, x1), v elsewhere

  blend(a, b, f)    t = a + f * (b - a) as three separately rounded fp32 operations (no fused multiply-add);
                    0 if t <= 0, 255 if t >= 255, else t truncated toward zero
  grey(r, g, b)     (19595 * r + 38470 * g + 7471 * b + 32768) >> 16

Histograms (ops 1, 2, 8) are taken over the image as it is at the input of that layer.

The source of layer 0 may be uint8, or fp32 / bf16 quantised on read, q(y) = rint(min(max((y * in_scale + in_shift) *
255, 0), 255)) (each operation rounded in fp32, rint to even, a NaN reads as 0).  The last layer writes uint8, or fp32
float(v) * out_scale + out_shift (two roundings), or bf16 (that value rounded to nearest even).

``sample_plan`` is a pure function of (config, rank, batch index, shape).  The input pipelines own the batch counter,
which restarts at 0 in a resumed run: a resumed run repeats the plans of the run's first batches instead of continuing
the sequence.

On CPU tensors ``randaugment`` runs the numpy form below: the CPU path of the feature (the host pipelines) and the
kernels' oracle, bit for bit.
"""
import math

import numpy as np
import torch

from . import _lib

REC_WORDS = 12
OPS = ("Identity", "AutoContrast", "Equalize", "Invert", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
       "Brightness", "Sharpness", "Affine", "Cutout")
OP_ID = {n: i for i, n in enumerate(OPS)}
(IDENTITY, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS,
 AFFINE, CUTOUT) = range(13)
# the sampler's names: the five geometric ones are all op Affine
SAMPLER_OPS = ("Identity", "AutoContrast", "Equalize", "Rotate", "Solarize", "Color", "Posterize", "Contrast",
               "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Invert", "SolarizeAdd",
               "Cutout")
DEFAULT_OPS = SAMPLER_OPS[:14]
KINDS = {"uint8": 0, "float32": 1, "bfloat16": 2}
_KIND_DTYPE = {"uint8": torch.uint8, "float32": torch.float32, "bfloat16": torch.bfloat16}
_DTYPE_KIND = {v: k for k, v in _KIND_DTYPE.items()}
DEFAULT_FILL = (128, 128, 128)


class RandAugmentConfig:
    """layers: ops per image (0 = off); magnitude in [0, 10]; prob: the probability that a drawn op is kept (else
    Identity); ops: names out of SAMPLER_OPS (a sequence or a comma-separated string); translate_ratio / cutout_ratio:
    the translation / the Cutout half side at magnitude 10 as a fraction of the image side; fill: the colour of
    pixels an Affine or Cutout leaves without a source; seed: the sampler's seed."""

    def __init__(self, layers=0, magnitude=9.0, prob=1.0, ops=None, translate_ratio=0.45, cutout_ratio=0.18,
                 fill=DEFAULT_FILL, seed=0):
        if isinstance(ops, str):
            ops = [s.strip() for s in ops.split(",") if s.strip()]
        self.layers = int(layers)
        self.magnitude = float(magnitude)
        self.prob = float(prob)
        self.ops = tuple(ops) if ops else DEFAULT_OPS
        self.translate_ratio = float(translate_ratio)
        self.cutout_ratio = float(cutout_ratio)
        self.fill = tuple(int(c) for c in fill)
        self.seed = int(seed)
        if self.layers < 0:
            raise ValueError("randaugment layers must not be negative, got %r" % (layers,))
        if not 0.0 <= self.magnitude <= 10.0:
            raise ValueError("randaugment magnitude must lie in [0, 10], got %r" % (magnitude,))
        if not 0.0 <= self.prob <= 1.0:
            raise ValueError("randaugment prob must lie in [0, 1], got %r" % (prob,))
        for n in self.ops:
            if n not in SAMPLER_OPS:
                raise ValueError("unknown randaugment op %r (known: %s)" % (n, ", ".join(SAMPLER_OPS)))
        for name, v in (("translate_ratio", self.translate_ratio), ("cutout_ratio", self.cutout_ratio)):
            if not 0.0 <= v <= 1.0:
                raise ValueError("randaugment %s must lie in [0, 1], got %r" % (name, v))
        if len(self.fill) != 3 or not all(0 <= c <= 255 for c in self.fill):
            raise ValueError("randaugment fill must be three values in [0, 255], got %r" % (fill,))
        if self.seed < 0:
            raise ValueError("seed must not be negative, got %r" % (seed,))

    def __repr__(self):
        return ("RandAugmentConfig(layers=%d, magnitude=%g, prob=%g, ops=%s, translate_ratio=%g, cutout_ratio=%g, "
                "fill=%r, seed=%d)" % (self.layers, self.magnitude, self.prob, ",".join(self.ops),
                                       self.translate_ratio, self.cutout_ratio, self.fill, self.seed))


class RandAugmentPlan:
    """The records of one batch: ``rec`` the host copy (numpy int32[B, N, 12]), ``dev`` the same records as a tensor
    on the device the batch lives on (None until ``to``), ``H`` x ``W`` the image size the boxes refer to."""

    def __init__(self, rec, H, W, dev=None):
        rec = np.ascontiguousarray(rec, dtype=np.int32)
        if rec.ndim != 3 or rec.shape[2] != REC_WORDS:
            raise ValueError("a randaugment plan is an int32[B, N, %d] array, got shape %r" % (REC_WORDS, rec.shape))
        self.rec, self.H, self.W, self.dev = rec, int(H), int(W), dev
        self._checked = False

    @property
    def B(self):
        return self.rec.shape[0]

    @property
    def N(self):
        return self.rec.shape[1]

    @property
    def op(self):
        return self.rec[:, :, 0]

    @property
    def iargs(self):
        return self.rec[:, :, 1:5]

    @property
    def fargs(self):
        return self.rec[:, :, 5:11].view(np.float32)

    def validate(self):
        """The checks the kernels rely on, on the host copy (the kernels trust the device copy)."""
        if self._checked:
            return self
        if self.B < 1 or self.N < 1:
            raise ValueError("an empty randaugment plan")
        op, i = self.op, self.iargs
        if not ((op >= 0) & (op < len(OPS))).all():
            raise ValueError("randaugment plan: op id outside [0, %d)" % len(OPS))
        for o, hi, what in ((POSTERIZE, 8, "Posterize bits"), (SOLARIZE, 256, "Solarize threshold"),
                            (SOLARIZE_ADD, 255, "SolarizeAdd addend")):
            v = i[:, :, 0][op == o]
            if not ((v >= 0) & (v <= hi)).all():
                raise ValueError("randaugment plan: %s outside [0, %d]" % (what, hi))
        b = i[op == CUTOUT]
        if not ((0 <= b[:, 0]) & (b[:, 0] <= b[:, 1]) & (b[:, 1] <= self.H)).all():
            raise ValueError("randaugment plan: Cutout rows violate 0 <= y0 <= y1 <= %d" % self.H)
        if not ((0 <= b[:, 2]) & (b[:, 2] <= b[:, 3]) & (b[:, 3] <= self.W)).all():
            raise ValueError("randaugment plan: Cutout columns violate 0 <= x0 <= x1 <= %d" % self.W)
        if not np.isfinite(self.fargs).all():
            raise ValueError("randaugment plan: a float argument is not finite")
        self._checked = True
        return self

    def host_tensor(self, pin=False):
        """The records as a fresh CPU tensor (a copy: the plan may be dropped before an asynchronous copy of it has
        run)."""
        t = torch.from_numpy(self.rec.copy())
        return t.pin_memory() if pin else t

    def to(self, device):
        """A plan with the same host records and ``dev`` on ``device`` (copied asynchronously on the current stream
        from a fresh pinned tensor)."""
        device = torch.device(device)
        if device.type == "cuda":
            dev = torch.empty(self.rec.shape, dtype=torch.int32, device=device)
            dev.copy_(self.host_tensor(pin=True), non_blocking=True)
        else:
            dev = self.host_tensor()
        p = RandAugmentPlan(self.rec, self.H, self.W, dev)
        p._checked = self._checked
        return p


def record(op, i=(), f=(), fill=DEFAULT_FILL):
    """One int32[12] record: ``op`` an id or a name of OPS, ``i`` up to four integers, ``f`` up to six floats
    (rounded once to fp32)."""
    r = np.zeros(REC_WORDS, dtype=np.int32)
    r[0] = OP_ID[op] if isinstance(op, str) else int(op)
    i = np.asarray(i, dtype=np.int64).reshape(-1)
    r[1:1 + i.size] = i
    f = np.asarray(f, dtype=np.float64).reshape(-1).astype(np.float32)
    r[5:5 + f.size] = f.view(np.int32)
    r[11] = int(fill[0]) | int(fill[1]) << 8 | int(fill[2]) << 16
    return r


def make_plan(rows, H, W):
    """A plan from hand-made records: ``rows[b][l]`` is the ``record(...)`` of layer l of image b."""
    return RandAugmentPlan(np.array([[np.asarray(r, dtype=np.int32) for r in row] for row in rows], dtype=np.int32)
                           .reshape(len(rows), -1, REC_WORDS), H, W)


def identity_plan(B, N, H, W, fill=DEFAULT_FILL):
    return make_plan([[record(IDENTITY, fill=fill)] * N for _ in range(B)], H, W)


def rotate_matrix(degrees, H, W):
    """The Affine arguments of a rotation by ``degrees`` about (W / 2, H / 2), in Python floats."""
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    cx, cy = W / 2, H / 2
    return (c, s, cx - c * cx - s * cy, -s, c, cy + s * cx - c * cy)


def sampled_record(name, m, neg, cy, cx, cfg, H, W):
    """The record of sampler op ``name`` at m = magnitude / 10 with sign ``neg`` and Cutout centre draws (cy, cx):
    the argument table of the sampler, computed in Python floats (matrix entries and factors rounded once to fp32)."""
    sg = -1.0 if neg else 1.0
    fill = cfg.fill
    if name in ("Identity", "AutoContrast", "Equalize", "Invert"):
        return record(name, fill=fill)
    if name == "Rotate":
        return record(AFFINE, f=rotate_matrix(sg * 30.0 * m, H, W), fill=fill)
    if name == "ShearX":
        return record(AFFINE, f=(1.0, sg * 0.3 * m, 0.0, 0.0, 1.0, 0.0), fill=fill)
    if name == "ShearY":
        return record(AFFINE, f=(1.0, 0.0, 0.0, sg * 0.3 * m, 1.0, 0.0), fill=fill)
    if name == "TranslateX":
        return record(AFFINE, f=(1.0, 0.0, sg * int(m * cfg.translate_ratio * W), 0.0, 1.0, 0.0), fill=fill)
    if name == "TranslateY":
        return record(AFFINE, f=(1.0, 0.0, 0.0, 0.0, 1.0, sg * int(m * cfg.translate_ratio * H)), fill=fill)
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        return record(name, f=(0.1 + 1.8 * m,), fill=fill)
    if name == "Posterize":
        return record(POSTERIZE, i=(8 - int(4 * m),), fill=fill)
    if name == "Solarize":
        return record(SOLARIZE, i=(256 - int(256 * m),), fill=fill)
    if name == "SolarizeAdd":
        return record(SOLARIZE_ADD, i=(int(110 * m),), fill=fill)
    if name == "Cutout":
        pad = int(m * cfg.cutout_ratio * min(H, W))
        yc, xc = int(cy * H), int(cx * W)
        return record(CUTOUT, i=(max(0, yc - pad), min(H, yc + pad), max(0, xc - pad), min(W, xc + pad)), fill=fill)
    raise ValueError("unknown randaugment op %r" % (name,))


def sample_plan(cfg, rank, batch_index, B, H, W):
    """The plan of batch ``batch_index`` on rank ``rank``: a pure function of its arguments, drawn from
    ``g = numpy.random.default_rng([cfg.seed, rank, batch_index])`` in this order, every draw a [B, layers] array:
      1. g.integers(0, len(ops), (B, N))   the op, an index into cfg.ops
      2. g.random((B, N))                  the op is replaced by Identity unless the draw is < prob
      3. g.integers(0, 2, (B, N))          the sign of the signed ops (Rotate, Shear, Translate): negative if 1
      4. g.random((B, N))                  the Cutout centre's y (row) draw
      5. g.random((B, N))                  the Cutout centre's x (column) draw: y is drawn before x
    Every draw is made whatever the others say, so one record's op does not move another record's numbers."""
    rank, batch_index, B, H, W = int(rank), int(batch_index), int(B), int(H), int(W)
    if min(rank, batch_index) < 0 or min(B, H, W) < 1 or cfg.layers < 1:
        raise ValueError("sample_plan: rank, batch_index must be >= 0 and B, H, W, layers >= 1")
    N = cfg.layers
    g = np.random.default_rng([cfg.seed, rank, batch_index])
    op = g.integers(0, len(cfg.ops), (B, N))
    keep = g.random((B, N)) < cfg.prob
    neg = g.integers(0, 2, (B, N)) == 1
    cy = g.random((B, N))
    cx = g.random((B, N))
    m = cfg.magnitude / 10
    rec = np.zeros((B, N, REC_WORDS), dtype=np.int32)
    for b in range(B):
        for l in range(N):
            name = cfg.ops[op[b, l]] if keep[b, l] else "Identity"
            rec[b, l] = sampled_record(name, m, bool(neg[b, l]), float(cy[b, l]), float(cx[b, l]), cfg, H, W)
    return RandAugmentPlan(rec, H, W).validate()


# ---- the numpy form of the definitions ------------------------------------------------------------------------------
def _blend(a, b, f):
    """a, b: float32 arrays (or scalars) of byte values, f: np.float32 -> uint8"""
    with np.errstate(over="ignore"):
        t = np.float32(a) + f * (np.float32(b) - np.float32(a))  # three fp32 roundings
    return np.trunc(np.clip(t, np.float32(0), np.float32(255))).astype(np.uint8)


def _grey(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16


def _channel_luts(img, fn):
    out = np.empty_like(img)
    for c in range(3):
        h = np.bincount(img[..., c].reshape(-1), minlength=256).astype(np.int64)
        out[..., c] = fn(h)[img[..., c]]
    return out


def _autocontrast_lut(h):
    ident = np.arange(256, dtype=np.uint8)
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return ident
    scale = np.float64(255.0) / np.float64(hi - lo)
    offset = -np.float64(lo) * scale
    return np.clip(np.trunc(np.arange(256, dtype=np.float64) * scale + offset), 0, 255).astype(np.uint8)


def _equalize_lut(h):
    ident = np.arange(256, dtype=np.uint8)
    nz = h[h > 0]
    if nz.size < 2:
        return ident
    step = (int(nz.sum()) - int(nz[-1])) // 255
    if step == 0:
        return ident
    before = np.cumsum(h) - h
    return np.minimum(255, (step // 2 + before) // step).astype(np.uint8)


def _sharp_smooth(img):
    H, W, _ = img.shape
    d = img.copy()
    if H >= 3 and W >= 3:
        x = img.astype(np.int32)
        s = 4 * x[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                s = s + x[dy:H - 2 + dy, dx:W - 2 + dx]
        d[1:-1, 1:-1] = ((s + 6) // 13).astype(np.uint8)
    return d


def _affine(img, f, fill):
    H, W, _ = img.shape
    half = np.float32(0.5)
    xf = (np.arange(W, dtype=np.float32) + half)[None, :]
    yf = (np.arange(H, dtype=np.float32) + half)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        xin = (f[0] * xf + f[1] * yf) + f[2]
        yin = (f[3] * xf + f[4] * yf) + f[5]
        ok = (xin >= 0) & (xin < np.float32(W)) & (yin >= 0) & (yin < np.float32(H))
    xi = np.minimum(np.where(ok, xin, 0).astype(np.int64), W - 1)
    yi = np.minimum(np.where(ok, yin, 0).astype(np.int64), H - 1)
    return np.where(ok[..., None], img[yi, xi], fill[None, None, :])


def apply_record(img, rec):
    """One layer on one image: img uint8 [H, W, 3], rec int32[12] -> a new uint8 [H, W, 3]."""
    op = int(rec[0])
    i = [int(v) for v in rec[1:5]]
    f = rec[5:11].view(np.float32)
    fill = np.array([rec[11] & 255, (rec[11] >> 8) & 255, (rec[11] >> 16) & 255], dtype=np.uint8)
    if op == IDENTITY:
        return img.copy()
    if op == AUTOCONTRAST:
        return _channel_luts(img, _autocontrast_lut)
    if op == EQUALIZE:
        return _channel_luts(img, _equalize_lut)
    if op == INVERT:
        return 255 - img
    if op == POSTERIZE:
        return img & np.uint8(~((1 << (8 - i[0])) - 1) & 255)
    if op == SOLARIZE:
        return np.where(img.astype(np.int32) < i[0], img, 255 - img)
    if op == SOLARIZE_ADD:
        return np.where(img < 128, np.minimum(255, img.astype(np.int32) + i[0]), img).astype(np.uint8)
    if op == COLOR:
        return _blend(_grey(img)[..., None], img, f[0])
    if op == CONTRAST:
        n = img.shape[0] * img.shape[1]
        m = (2 * int(_grey(img).sum()) + n) // (2 * n)
        return _blend(m, img, f[0])
    if op == BRIGHTNESS:
        return _blend(0, img, f[0])
    if op == SHARPNESS:
        return _blend(_sharp_smooth(img), img, f[0])
    if op == AFFINE:
        return _affine(img, f, fill)
    if op == CUTOUT:
        out = img.copy()
        out[i[0]:i[1], i[2]:i[3]] = fill
        return out
    raise ValueError("randaugment: op id %d" % op)


def quantize_source(y, in_scale, in_shift):
    """float32 array -> the uint8 values layer 0 reads"""
    s, b = np.float32(in_scale), np.float32(in_shift)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (y.astype(np.float32) * s + b) * np.float32(255)
        t = np.where(t > 0, t, np.float32(0))  # (a NaN reads as 0)
        t = np.where(t < 255, t, np.float32(255))
    return np.rint(t).astype(np.uint8)


def apply_numpy(x_u8, rec):
    """x_u8 uint8 [B, H, W, 3], rec int32[B, N, 12] -> uint8 [B, H, W, 3]"""
    out = np.empty_like(x_u8)
    for b in range(x_u8.shape[0]):
        img = x_u8[b]
        for l in range(rec.shape[1]):
            img = apply_record(img, rec[b, l])
        out[b] = img
    return out


def _randaugment_cpu(x, plan, out_kind, in_affine, out_affine):
    if x.dtype == torch.uint8:
        u8 = x.numpy()
    else:
        u8 = quantize_source(x.float().numpy(), *in_affine)
    res = apply_numpy(u8, plan.rec)
    if out_kind == "uint8":
        return torch.from_numpy(res)
    y = res.astype(np.float32) * np.float32(out_affine[0]) + np.float32(out_affine[1])  # two fp32 roundings
    return torch.from_numpy(y).to(_KIND_DTYPE[out_kind])  # (bf16: round to nearest even)


_BUFFERS = {}


def _device_buffers(device, B, H, W, N):
    """The two ping-pong layer buffers and the histogram scratch of a shape, allocated once per (device, shape) and
    reused by every later call (calls on one device are ordered by the stream they run on)."""
    key = (device, B, H, W, N)
    bufs = _BUFFERS.get(key)
    if bufs is None:
        nbytes = B * H * W * 3
        bufs = _BUFFERS[key] = (torch.empty(nbytes, dtype=torch.uint8, device=device),
                                torch.empty(nbytes, dtype=torch.uint8, device=device),
                                torch.empty(N * B * 4 * 256, dtype=torch.int32, device=device))
    return bufs


def _kind_name(k):
    k = _DTYPE_KIND.get(k, k)
    if k not in KINDS:
        raise ValueError("randaugment: kind must be uint8, float32 or bfloat16, got %r" % (k,))
    return k


@torch.no_grad()
def randaugment(x, plan, out_kind="uint8", in_affine=(1.0, 0.0), out_affine=(1.0, 0.0), out=None):
    """``plan`` applied to ``x`` ([B, H, W, 3] uint8, fp32 or bf16, contiguous; may start at any element of a larger
    buffer) into ``out`` (not overlapping x) or a new tensor of ``out_kind`` ('uint8', 'float32', 'bfloat16' or the
    torch dtype).  in_affine = (in_scale, in_shift) maps a float source to [0, 1] before the 8-bit quantisation;
    out_affine = (out_scale, out_shift) maps the bytes of a float destination.  On the device: one memset and two
    launches per layer on the current stream, no host synchronisation."""
    out_kind = _kind_name(out_kind)
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[3] != 3 or x.dtype not in _DTYPE_KIND:
        raise ValueError("randaugment needs a [B, H, W, 3] uint8, fp32 or bf16 tensor, got %s %s"
                         % (getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
    if not x.is_contiguous() or x.numel() == 0:
        raise ValueError("randaugment needs a contiguous, non-empty NHWC batch")
    B, H, W, _C = x.shape
    if plan.B != B or plan.H != H or plan.W != W:
        raise ValueError("randaugment plan for B, H, W = %d, %d, %d used on a batch of %d, %d, %d"
                         % (plan.B, plan.H, plan.W, B, H, W))
    plan.validate()
    if out is not None:
        if (out.shape != x.shape or out.dtype != _KIND_DTYPE[out_kind] or out.device != x.device
                or not out.is_contiguous()):
            raise ValueError("randaugment: out must match x in shape and device, be %s and contiguous" % out_kind)
        xb, ob = x.numel() * x.element_size(), out.numel() * out.element_size()
        if x.data_ptr() < out.data_ptr() + ob and out.data_ptr() < x.data_ptr() + xb:
            raise ValueError("randaugment: out overlaps x")  # (Affine and Sharpness read other pixels than they write)
    if not x.is_cuda:
        res = _randaugment_cpu(x, plan, out_kind, in_affine, out_affine)
        if out is None:
            return res
        out.copy_(res)
        return out
    if plan.dev is None or plan.dev.device != x.device:
        raise ValueError("randaugment: the plan has no record on %s (plan.to(device))" % x.device)
    if out is None:
        out = torch.empty(x.shape, dtype=_KIND_DTYPE[out_kind], device=x.device)
    buf0, buf1, scratch = _device_buffers(x.device, B, H, W, plan.N)
    rc = _lib.lib().dtm_randaugment(_lib.ptr(x), KINDS[_DTYPE_KIND[x.dtype]], float(in_affine[0]),
                                    float(in_affine[1]), _lib.ptr(plan.dev), B, H, W, plan.N, _lib.ptr(buf0),
                                    _lib.ptr(buf1), _lib.ptr(scratch), _lib.ptr(out), KINDS[out_kind],
                                    float(out_affine[0]), float(out_affine[1]), _lib.stream_ptr())
    if rc != 0:
        raise RuntimeError("dtm_randaugment failed (%d)" % rc)
    return out
