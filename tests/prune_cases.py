"""Shared inputs of the pruning tests (CPU and GPU): the numpy oracle of the selection and the value sets.

Everything here works on the uint32 bit patterns of fp32 values, so NaN payloads, -0.0 and denormals pass through
numpy untouched.  The oracle has no ambiguity: the definition is a threshold on the key."""
import math

import numpy as np

CHUNK = 8192  # elements per chunk row of the kernels (asserted against the library in the GPU tests)
SIZES = (1, 7, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
SETS = ("normal", "ties", "zeros", "equal", "digit1", "digit12", "special", "sparse60")
# keys base .. base + n - 1: BASE1 keeps them inside one bin of the first digit (bits 30..20) for every n used here and
# starts 300 keys past a boundary of the second digit (bits 19..10); BASE12 is such a boundary, so up to 1024 keys
# share both digits
BASE1 = 0x3D080000 + 300
BASE12 = 0x3D0C0000


def keys_of(bits):
    return bits & np.uint32(0x7FFFFFFF)


def oracle(bits, sparsity):
    """(mask uint8, tau, kept, z) of the definition for the uint32 patterns ``bits`` (any shape)."""
    key = keys_of(bits).reshape(-1)
    z = int(math.floor(float(sparsity) * key.size))
    if z == 0:
        return np.ones(bits.shape, np.uint8), 0, key.size, 0
    tau = np.partition(key, z - 1)[z - 1]
    mask = (key > tau).astype(np.uint8).reshape(bits.shape)
    return mask, int(tau), int(mask.sum()), z


def _signs(bits, rng):
    return bits | (rng.integers(0, 2, bits.size, dtype=np.uint32) << np.uint32(31))


def value_set(name, n, seed=0):
    """uint32 patterns [n] of the named set."""
    rng = np.random.default_rng([seed, n, SETS.index(name)])
    if name == "normal":  # (a)
        return (rng.standard_normal(n).astype(np.float32) * np.float32(0.05)).view(np.uint32)
    if name == "ties":  # (b) five magnitudes, random signs: ties everywhere, the threshold included
        mags = np.array([0.0, 1e-3, 0.02, 0.02000001, 1.5], np.float32).view(np.uint32)
        return _signs(mags[rng.integers(0, 5, n)], rng)
    if name == "zeros":  # (c)
        return np.zeros(n, np.uint32)
    if name == "equal":
        return np.full(n, np.float32(0.37).view(np.uint32), np.uint32)
    if name in ("digit1", "digit12"):  # (d) consecutive keys, shuffled
        base = BASE12 if (name == "digit12" and n <= 1024) else BASE1
        return _signs(rng.permutation(np.arange(base, base + n, dtype=np.uint32)), rng)
    if name == "special":  # (e)
        bits = (rng.standard_normal(n).astype(np.float32) * np.float32(0.05)).view(np.uint32).copy()
        special = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,
                            0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001], np.uint32)
        pos = rng.integers(0, n, max(1, n // 3))
        bits[pos] = special[rng.integers(0, special.size, pos.size)]
        return bits
    if name == "sparse60":  # (f) already 60 % zeros
        bits = (rng.standard_normal(n).astype(np.float32) * np.float32(0.05)).view(np.uint32).copy()
        bits[rng.permutation(n)[:int(math.ceil(0.6 * n))]] = 0
        return bits
    raise ValueError(name)


def sparsities(n):
    """The sparsities of the issue for a tensor of n elements (0.7 is the second request of the sparse60 set)."""
    return sorted({0.0, 1.0 / n, 0.5, 0.7, 0.9, (n - 1.0) / n} - {1.0})


def bin_end_ranks(base, n):
    """Ranks z in [1, n - 1] of the consecutive keys base .. base + n - 1 at which the running count of the scan
    equals z exactly at the end of a bin of the first or the second digit, with 1 and n - 1."""
    zs = {1, n - 1} | {z for z in range(1, n) if (base + z) % 1024 == 0}
    return sorted(z for z in zs if 1 <= z <= n - 1)


def sparsity_for_rank(z, n):
    """A sparsity s with floor(float64(s) * n) == z."""
    s = (z + 0.5) / n
    assert int(math.floor(s * n)) == z and s < 1.0
    return s
