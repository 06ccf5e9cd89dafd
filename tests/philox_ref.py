"""numpy restatement of the seeded sampler noise (include/ctta.h, ctta_philox_normal), written from the
definition: integer Philox4x32-10 as published, and float64 for u, log, sqrt, cos and sin.

  q = (h * C + c) * W + w                         rows are the outer index
  key = (seed & 0xffffffff, seed >> 32)           seed: int64 taken as uint64
  counter = (q >> 2, d, m, 0)                     d: draw, m: sample, 0: the domain tag of sampler noise
  words x0..x3 serve q & 3 = 0..3
  u(x) = ((x >> 9) + 0.5) * 2^-23;  r(x) = sqrt(-2 ln u(x))
  z0 = r(x0) cos(2 pi u(x1)), z1 = r(x0) sin(2 pi u(x1)), z2 = r(x2) cos(2 pi u(x3)), z3 = r(x2) sin(2 pi u(x3))
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
MAX_ABS = float(np.sqrt(-2.0 * np.log(2.0 ** -24)))          # 5.768: the largest magnitude the stream can produce

# the published known-answer vectors: (counter, key, output)
KNOWN_ANSWERS = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; returns the four output word arrays (uint64 holding
    32-bit values), broadcast over the inputs."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def words(seed, sample, draw, latent):
    """The raw words of draw `draw` of the stream (seed, sample) on a (C, H, W) latent: uint32 array (C, H, W)."""
    C, H, W = latent
    assert W % 4 == 0 and C * H * W < 2 ** 34
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    c, h, w4 = np.meshgrid(np.arange(C, dtype=np.uint64), np.arange(H, dtype=np.uint64),
                           np.arange(W // 4, dtype=np.uint64), indexing="ij")
    q = (h * np.uint64(C) + c) * np.uint64(W) + np.uint64(4) * w4
    x = philox4x32_10((q >> np.uint64(2), int(draw), int(sample), 0), (s & 0xFFFFFFFF, s >> 32))
    return np.stack(x, axis=-1).reshape(C, H, W).astype(np.uint32)


def unit(x):
    """u(x) in float64 (the value is exact in fp32 too)."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals_from_words(x):
    """(z, r) in float64 from raw words whose last axis is a multiple of 4: Box-Muller on the pairs (x0, x1), (x2, x3);
    r is each element's pair radius."""
    x = np.asarray(x)
    g = x.reshape(x.shape[:-1] + (x.shape[-1] // 2, 2))
    r = np.sqrt(-2.0 * np.log(unit(g[..., 0])))
    a = 2.0 * np.pi * unit(g[..., 1])
    z = np.stack([r * np.cos(a), r * np.sin(a)], axis=-1).reshape(x.shape)
    return z, np.repeat(r, 2, axis=-1).reshape(x.shape)


def normal(seeds, samples, draw0, draws, latent):
    """What ctta_philox_words / ctta_philox_normal (scale 1) define: (words uint32, z float64, r float64), each
    (draws, B, C, H, W)."""
    samples = [0] * len(seeds) if samples is None else samples
    w = np.stack([np.stack([words(s, m, draw0 + d, latent) for s, m in zip(seeds, samples)]) for d in range(draws)])
    z, r = normals_from_words(w)
    return w, z, r
