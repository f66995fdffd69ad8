"""Inputs and references shared by tests/test_loudness_cpu.py and tests/test_gpu_loudness.py (not a test module): the three signals of
the kernel-vs-definition test, the row lengths, and the definition (cmtts_amd/loudness.py) of every row in float64 and in float32.
A filter started from zero state is causal, so the K-weighted prefix of a signal is the prefix of the K-weighted signal: every signal is
filtered once per dtype and the rows share it.  Computed once and left unchanged."""
import functools
import math

import numpy as np

from cmtts_amd import loudness as ld

FS = ld.NATIVE_RATE
BLOCK, HOP = ld.block_sizes(FS)          # 8820, 2205
SECONDS = 3
# a chunk that starts at sample 0 exactly, a row with no block at all, one block exactly, a partial last chunk, the first chunk that needs
# a warm-up (3 HOP), 3 s
LENGTHS = (0, 1, BLOCK - 1, BLOCK, BLOCK + HOP - 1, BLOCK + HOP, 3 * HOP + BLOCK + 5, SECONDS * FS)
SIGNALS = ("gating", "modulated", "dc")
GATE_MARGIN = 0.5                        # LU: the block counts are compared only where every block is at least this far from both gates


@functools.lru_cache(maxsize=None)
def signal(name):
    """float32 [3 s] at 22 050 Hz."""
    t = np.arange(SECONDS * FS) / FS
    if name == "gating":          # 997 Hz: 1 s at -20 dBFS, 1 s at -36 dBFS, 1 s at -80 dBFS
        x = np.sin(2 * np.pi * 997 * t) * np.repeat(10.0 ** (np.array([-20.0, -36.0, -80.0]) / 20.0), FS)
    elif name == "modulated":     # a modulated tone, noise and a DC offset
        x = 0.3 * np.sin(2 * np.pi * 140 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + 0.02 * np.random.RandomState(5).standard_normal(len(t)) + 0.05
    elif name == "dc":            # the high-pass must remove it
        x = np.full(len(t), 0.25)
    else:
        raise KeyError(name)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def weighted(name, dtype):
    y = ld.k_weight(signal(name), FS, dtype)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(name, n, dtype=np.float64):
    """(L, n_blocks_total, n_blocks_gated) of signal(name)[:n] by the definition evaluated in `dtype`."""
    return ld.gated_loudness(weighted(name, dtype)[:n], FS)


@functools.lru_cache(maxsize=None)
def gate_margin(name, n):
    """The smallest distance in LU of a block of signal(name)[:n] from a gate it is compared with, by the float64 definition (inf where
    there is no block, or no block passes the absolute gate; a silent block is infinitely far from both)."""
    z, l = ld.block_loudness(weighted(name, np.float64)[:n], FS)
    if not len(z):
        return math.inf
    m = float(np.min(np.abs(l - ld.ABSOLUTE_GATE)))
    keep = l > ld.ABSOLUTE_GATE
    if n >= BLOCK and keep.any():
        m = min(m, float(np.min(np.abs(l - (ld._lk(float(np.mean(z[keep]))) + ld.RELATIVE_GATE)))))
    return m


def pin(name, n):
    """The bound on |L(kernel) - L(float64 definition)| in LU: max(10 d32, 2e-4), d32 = the deviation of the definition's own float32
    evaluation on this case (the kernel sums in another order: the run-and-scan form simulated in float32 was 2.2 x the sequential one)."""
    L64, L32 = reference(name, n)[0], reference(name, n, np.float32)[0]
    d32 = 0.0 if L64 == L32 else abs(L32 - L64)
    return max(10.0 * d32, 2e-4), d32
