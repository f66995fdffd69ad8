"""Inputs and references shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py (not a test module): the five required
rates, their filters, the waves of the kernel-vs-definition test and the float64 definition of every row with its derived fp32 bound.
Computed once per rate and left unchanged."""
import functools

import numpy as np

from cmtts_amd import resample as rs

RATES = (8000, 16000, 24000, 44100, 48000)
ROW_LENGTHS = (1000, 257, 1)          # plus a row of R - 1 samples per rate
GARBAGE = 7.0                         # what the wave buffers hold after a row's valid samples: must never reach an output


@functools.lru_cache(maxsize=None)
def filt(rate):
    L, M = rs.ratio(rs.NATIVE_RATE, rate)
    taps, half = rs.design_taps(L, M)
    return L, M, taps, half, rs.half_width(L, half)


@functools.lru_cache(maxsize=None)
def waves(rate):
    """[x float32 [n]] for n = 1000, 257, 1, R - 1: waveform-like values in (-1, 1)."""
    R = filt(rate)[4]
    g = np.random.RandomState(rate)
    return tuple(np.tanh(g.standard_normal(n) * 0.8).astype(np.float32) for n in ROW_LENGTHS + (R - 1,))


def term_counts(n, L, M, half):
    """K_m: the number of source samples under the taps of output m, for every output of an n-sample wave."""
    K = np.zeros(rs.out_len(n, L, M), np.int64)
    for m in range(len(K)):
        lo, hi = rs.term_range(m, L, M, half)
        K[m] = max(min(hi, n - 1) - max(lo, 0) + 1, 0)
    return K


def definition_and_bound(x, L, M, taps, half):
    """(y float64, bound): the definition and (K_m + 2) * 2^-24 * sum_j |x_j h| per output — the standard bound of an fp32
    accumulation of K products (each product and each addition rounds once, relative error 2^-24; valid for any order)."""
    y = rs.resample(x, L, M, taps)
    mag = rs.resample(np.abs(x), L, M, np.abs(taps))
    return y, (term_counts(len(x), L, M, half) + 2) * 2.0 ** -24 * mag


@functools.lru_cache(maxsize=None)
def reference(rate):
    """[(y float64, bound)] for waves(rate)."""
    L, M, taps, half, _ = filt(rate)
    return tuple(definition_and_bound(x, L, M, taps, half) for x in waves(rate))
