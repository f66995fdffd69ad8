"""Seeded per-utterance sampler noise: the definition (csrc/noise_philox.hip) in executable form.

Pure numpy.  This is what the HIP kernel is tested against, NOT a fallback on the synthesis path: host.seeded_noise and the
seeded sampler run noise_philox.hip and nothing here.

The value at (utterance seed, draw, frame, mel bin) is a pure function of those four numbers:

    key      (seed mod 2^32, seed >> 32)                                     the utterance's 64-bit seed
    counter  (j mod 2^32, j >> 32, draw, 0x434D5454),  j = (t0 + t) * ceil(M / 4) + floor(m / 4)
    bits     Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85, ten rounds)
    normals  Box-Muller on 24-bit uniforms: u1 = ((x_a >> 8) + 1) * 2^-24, u2 = (x_b >> 8) * 2^-24, r = sqrt(-2 ln u1);
             lanes 0, 1 = r cos(2 pi u2), r sin(2 pi u2) from (x0, x1), lanes 2, 3 the same from (x2, x3); |z| <= 5.77
    element (t, m) is lane m mod 4 of its block; draw 0 is x_T, draw 1 + i the re-noise after evaluation i.
"""
import numpy as np

PHILOX_M0 = 0xD2511F53
PHILOX_M1 = 0xCD9E8D57
PHILOX_W0 = 0x9E3779B9
PHILOX_W1 = 0xBB67AE85
COUNTER_TAG = 0x434D5454          # "CMTT": the fourth counter word
_M32 = np.uint64(0xFFFFFFFF)
_M64 = (1 << 64) - 1


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: uint32 [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
    ctr = np.asarray(ctr, dtype=np.uint32)
    key = np.asarray(key, dtype=np.uint32)
    c0, c1, c2, c3 = (ctr[..., i].astype(np.uint64) for i in range(4))
    k0, k1 = (key[..., i].astype(np.uint64) for i in range(2))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def splitmix64(x):
    """One step of splitmix64 on a Python int (mod 2^64)."""
    x = (int(x) + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def utterance_seeds(seed, ids):
    """seeds[i] = splitmix64((splitmix64(seed) + ids[i]) mod 2^64) as int64 (two's complement of the 64-bit value)."""
    base = splitmix64(int(seed) & _M64)
    out = [splitmix64((base + (int(i) & _M64)) & _M64) for i in np.asarray(ids).reshape(-1)]
    return np.asarray(out, dtype=np.uint64).view(np.int64)


def _as_u64(seeds):
    """Seeds as uint64 [B]: int64 values by their two's complement, Python ints mod 2^64."""
    a = np.atleast_1d(np.asarray(seeds))
    if a.dtype == np.uint64:
        return a
    if a.dtype.kind in "iu":
        return a.astype(np.int64).view(np.uint64)
    return np.asarray([int(v) & _M64 for v in a.reshape(-1)], dtype=np.uint64)


def reference_bits(seeds, n_draws, T, n_mels=80, first_draw=0, t0=0):
    """The raw Philox blocks: uint32 [n_draws, B, T, ceil(n_mels / 4), 4]."""
    s = _as_u64(seeds)
    Q = (int(n_mels) + 3) // 4
    j = (np.uint64(int(t0)) + np.arange(int(T), dtype=np.uint64))[:, None] * np.uint64(Q) + np.arange(Q, dtype=np.uint64)[None, :]
    d = np.arange(int(first_draw), int(first_draw) + int(n_draws), dtype=np.uint64)
    shape = (len(d), len(s), int(T), Q)
    ctr = np.empty(shape + (4,), np.uint32)
    ctr[..., 0] = (j & _M32)[None, None]
    ctr[..., 1] = (j >> np.uint64(32))[None, None]
    ctr[..., 2] = d[:, None, None, None]
    ctr[..., 3] = COUNTER_TAG
    key = np.empty(shape + (2,), np.uint32)
    key[..., 0] = (s & _M32)[None, :, None, None]
    key[..., 1] = (s >> np.uint64(32))[None, :, None, None]
    return philox4x32_10(ctr, key)


def normals_from_bits(bits):
    """uint32 [..., 4] -> float64 [..., 4] (Box-Muller as defined above)."""
    b = np.asarray(bits, dtype=np.uint32)
    out = np.empty(b.shape, np.float64)
    for a in (0, 2):
        u1 = ((b[..., a] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (b[..., a + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[..., a] = r * np.cos(2.0 * np.pi * u2)
        out[..., a + 1] = r * np.sin(2.0 * np.pi * u2)
    return out


def reference_normals(seeds, n_draws, T, n_mels=80, first_draw=0, t0=0):
    """float64 [n_draws, B, 1, T, n_mels]: what cmtts_noise_fill writes, before its rounding to fp32."""
    z = normals_from_bits(reference_bits(seeds, n_draws, T, n_mels, first_draw, t0))
    nd, B = z.shape[:2]
    return z.reshape(nd, B, 1, int(T), -1)[..., :int(n_mels)]


def indiv_indices(n, num_samples, done_samples=0, rank=0, world=1):
    """Global sample indices of the n rows a "determ-indiv" generator draws next: done_samples + rank + k * world for k < n,
    clamped to num_samples - 1."""
    idx = int(done_samples) + int(rank) + np.arange(int(n), dtype=np.int64) * int(world)
    return np.minimum(idx, int(num_samples) - 1)
