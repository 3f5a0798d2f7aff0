"""A plain Philox4x32-10 in numpy, and the three layouts the device streams are defined by.

The generator is written from the Random123 definition (Salmon, Moraes, Dror, Shaw, "Parallel random
numbers: as easy as 1, 2, 3", SC'11): ten rounds of

    hi0, lo0 = mulhilo(0xD2511F53, c0);  hi1, lo1 = mulhilo(0xCD9E8D57, c2)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)

with the key bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.  Everything is
uint64 arithmetic on 32-bit words (a 32 x 32 product fits in 64 bits), vectorised over an array of
counters.  ``tests/test_rng_optim_refs.py`` holds it to the Random123 known-answer vectors; the GPU
tests then hold the kernels to it.

Stream layout (what a draw *is*):

* counter ``(tag, 0, ctr & 0xffffffff, ctr >> 32)``, key ``(seed & 0xffffffff, seed >> 32)``;
  ``tag`` is ``TAG_FILL`` for uniform / normal fills and ``TAG_SAMPLE`` for the window sampler;
* quad ``q`` of a fill of ``n`` values uses counter ``ctr + q`` and yields values ``4q .. 4q + 3``; the
  fill consumes ``ceil(n / 4)`` counters;
* sample ``b`` of a batch uses counter ``ctr + b``; the sampler consumes ``B`` counters.
"""
import numpy as np

M0 = np.uint64(0xD2511F53)
M1 = np.uint64(0xCD9E8D57)
W0 = np.uint64(0x9E3779B9)
W1 = np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

TAG_FILL = 0x5EED
TAG_SAMPLE = 0xB47C


def philox4x32_10(counter, key):
    """``counter``: (..., 4) and ``key``: (..., 2) arrays of 32-bit words (broadcast against each
    other).  Returns the (..., 4) uint32 output block."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        if r:
            k0 = (k0 + W0) & MASK32
            k1 = (k1 + W1) & MASK32
        p0 = M0 * c0
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def stream_blocks(seed, ctr, count, tag):
    """The ``count`` output blocks of stream ``seed`` at 64-bit counters ``ctr .. ctr + count - 1``
    (wrapping at 2^64): a (count, 4) uint32 array."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = np.full(count, int(ctr) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64) + np.arange(count, dtype=np.uint64)
    counter = np.zeros((count, 4), dtype=np.uint64)
    counter[:, 0] = tag
    counter[:, 2] = c & MASK32
    counter[:, 3] = c >> S32
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(counter, key)


def n_quads(n):
    return (int(n) + 3) // 4


def _unit(x):
    """uint32 -> (0, 1]: ((x >> 8) + 1) * 2^-24, exact in fp32 (and in fp64)."""
    return ((x >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24


def uniform_ref(seed, ctr, n):
    """The ``n`` uniforms of a fill at counter ``ctr``, as float64 (every value is an fp32 number)."""
    return _unit(stream_blocks(seed, ctr, n_quads(n), TAG_FILL)).reshape(-1)[:n]


def normal_ref(seed, ctr, n):
    """The ``n`` normals of a fill at counter ``ctr``: fp64 Box-Muller in quads,
    (z0, z1) = r_a (cos, sin)(2 pi u1) with r_a = sqrt(-2 ln u0); (z2, z3) likewise from (u2, u3)."""
    u = _unit(stream_blocks(seed, ctr, n_quads(n), TAG_FILL))
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    ta, tb = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=-1)
    return z.reshape(-1)[:n]


def window_index_ref(seed, ctr, batch, n_windows):
    """The ``batch`` window indices of a sampler call at counter ``ctr``: ((r0 << 32) | r1) % N."""
    r = stream_blocks(seed, ctr, batch, TAG_SAMPLE).astype(np.uint64)
    return (((r[:, 0] << S32) | r[:, 1]) % np.uint64(n_windows)).astype(np.int64)
