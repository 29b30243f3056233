"""Shared inputs of the gradient-compression tests (CPU and GPU): the numpy oracle of the definition and the cases.

Everything is compared as uint32 / int32 bit patterns of fp32 values, so NaN payloads, -0.0 and denormals pass through
numpy untouched.  The oracle is written from the definition alone (ops/compress.py is not imported here):
  u = res + g;  key = bits(u) & 0x7fffffff;  S = the first k of numpy.lexsort((index, 0x7fffffff - key)), ascending;
  packet = (S, bits(u)[S]);  res' = +0 on S and where u is not finite, else u;
  decompress: g = +0, then the packets added in rank order.
"""
import collections

import numpy as np

CHUNK = 8192  # elements per chunk row of the kernels (asserted against the library in the GPU tests)
KEY = np.uint32(0x7FFFFFFF)

Case = collections.namedtuple("Case", "name res g k off_res off_g")  # res, g: uint32 patterns [n]; offsets in elements


def f2b(x):
    return np.asarray(x, np.float32).view(np.uint32)


def b2f(b):
    return np.asarray(b, np.uint32).view(np.float32)


def bucket_k(n, rho):
    return min(n, max(1, int(np.ceil(rho * n))))


def oracle(res_bits, g_bits, k):
    """(idx int32 [k], val uint32 [k], new res uint32 [n], u uint32 [n])."""
    with np.errstate(all="ignore"):
        u = b2f(res_bits) + b2f(g_bits)
    bits = u.view(np.uint32)
    key = (bits & KEY).astype(np.int64)
    n = key.size
    order = np.lexsort((np.arange(n), int(KEY) - key))
    sel = np.sort(order[:k])
    new = bits.copy()
    new[sel] = 0
    new[(bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)] = 0
    return sel.astype(np.int32), bits[sel].copy(), new, bits.copy()


def oracle_decompress(n, packets):
    """uint32 [n]: +0, then every (idx, val bits) of ``packets`` added in list order."""
    g = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for idx, val in packets:
            for i, v in zip(np.asarray(idx).tolist(), b2f(val).tolist()):
                g[i] = np.float32(g[i]) + np.float32(v)
    return g.view(np.uint32).copy()


def _normal(rng, n, scale=1.0):
    return f2b(rng.standard_normal(n).astype(np.float32) * np.float32(scale))


def _zeros(n):
    return np.zeros(n, np.uint32)


def _tie_run(rng, n, lo, hi, big):
    """Small noise, ``big`` elements of magnitude 2 in front of and behind a run [lo, hi) of magnitude 1 with
    alternating signs."""
    g = b2f(_normal(rng, n, 0.01)).copy()
    g[lo:hi] = np.where(np.arange(lo, hi) % 2 == 0, 1.0, -1.0)
    for i in list(range(3, 3 + big // 2)) + list(range(n - 7, n - 7 + (big - big // 2))):
        g[i] = -2.0
    return f2b(g)


def cases():
    out = []
    rng = np.random.default_rng(20171)
    N1, N3 = CHUNK + 3, 3 * CHUNK + 5
    # sizes x alignments: tiny (head and tail only), one element over a row, several rows
    for n in (1, 5, N1, N3):
        for off in range(4):
            out.append(Case("normal-n%d-off%d" % (n, off), _normal(rng, n), _normal(rng, n), bucket_k(n, 0.01), off,
                            off))
    out.append(Case("normal-n%d-mixed-1-2" % N1, _normal(rng, N1), _normal(rng, N1), bucket_k(N1, 0.01), 1, 2))
    out.append(Case("normal-n%d-mixed-0-3" % N3, _normal(rng, N3), _normal(rng, N3), bucket_k(N3, 0.05), 0, 3))
    # k extremes
    out.append(Case("k1", _normal(rng, N1), _normal(rng, N1), 1, 0, 0))
    out.append(Case("k1-n5", _normal(rng, 5), _normal(rng, 5), 1, 1, 1))
    out.append(Case("kn", _normal(rng, N1), _normal(rng, N1), N1, 3, 3))
    out.append(Case("kn-n5", _normal(rng, 5), _normal(rng, 5), 5, 2, 2))
    out.append(Case("k2", _normal(rng, N1), _normal(rng, N1), bucket_k(N1, 0.0002), 0, 0))
    assert out[-1].k == 2
    # ties
    out.append(Case("ties-all-equal", _zeros(N1), f2b(np.full(N1, 0.5, np.float32)), 100, 1, 1))
    out.append(Case("ties-wave-boundary", _zeros(N3), _tie_run(rng, N3, 250, 262, 3), 3 + 8, 0, 0))
    out.append(Case("ties-wave-boundary-scalar", _zeros(N3), _tie_run(rng, N3, 250, 262, 3), 3 + 8, 0, 1))
    out.append(Case("ties-row-boundary", _zeros(N3), _tie_run(rng, N3, 8186, 8200, 4), 4 + 9, 0, 0))
    out.append(Case("ties-row-boundary-off2", _zeros(N3), _tie_run(rng, N3, 8186, 8200, 4), 4 + 7, 2, 2))
    g = np.zeros(N1, np.float32)
    g[rng.choice(N1, 100, replace=False)] = rng.standard_normal(100).astype(np.float32)
    out.append(Case("mostly-zeros", _zeros(N1), f2b(g), 300, 0, 0))
    sign = (rng.integers(0, 2, N1).astype(np.uint32) << np.uint32(31))
    out.append(Case("signed-zeros", sign.copy(), sign.copy(), 50, 3, 3))  # (-0) + (-0) = -0, (+0) + (+0) = +0
    den = rng.integers(1, 0x800000, N1).astype(np.uint32) | (rng.integers(0, 2, N1).astype(np.uint32) << np.uint32(31))
    out.append(Case("denormals", _zeros(N1), den, bucket_k(N1, 0.01), 0, 0))
    # keys that differ in one digit of the radix select only: the low 10 bits (u = 1 + j * 2^-23), the middle 10
    j = rng.permutation(N1).astype(np.uint32) % np.uint32(1024)
    out.append(Case("digit-low", _zeros(N1), np.uint32(0x3F800000) + j, 700, 0, 0))
    out.append(Case("digit-middle", _zeros(N1), np.uint32(0x3F800000) + (j << np.uint32(10)), 700, 1, 1))
    # non-finite values rank first, are sent while k allows and never enter the residual
    for name, bad, k in (("one-nan", [(5000, 0x7FC00000)], 82), ("one-neg-inf", [(N1 - 1, 0xFF800000)], 82),
                         ("k-plus-1-nans", [(i, 0x7FC00000) for i in (0, 255, 256, 8191, 8194)], 4)):
        g = _normal(rng, N1)
        for i, b in bad:
            g[i] = b
        out.append(Case("nonfinite-" + name, _normal(rng, N1), g, k, 0, 0))
    return out


CASES = cases()
IDS = [c.name for c in CASES]

# W = 3 packets over n = 16 with overlapping indices; at index 3 the ranks send 1, 1e8, -1e8:
# ((0 + 1) + 1e8) + -1e8 = 0 in fp32, while any order that adds 1 last gives 1
ORDER_N, ORDER_K = 16, 2
ORDER_PACKETS = [(np.array([3, 7], np.int32), f2b([1.0, 0.5])),
                 (np.array([3, 9], np.int32), f2b([1e8, 0.25])),
                 (np.array([3, 7], np.int32), f2b([-1e8, 2.0 ** -30]))]
