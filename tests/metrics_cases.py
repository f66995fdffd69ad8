"""Shared inputs of the metric tests (tests/test_metrics_cpu.py, tests/test_gpu_metrics.py): the smallest pairs at which tiles, halos and
raggedness can go wrong.  Computed once, shared, never written."""
import functools

import numpy as np

from cmtts_amd import metrics as M

# (Ts, Tr): above, at and below a 64 x 64 cost tile and a strip of 64 rows, both Ts > Tr and Tr > Ts; 12 and 11 recording frames give two
# and one window row of the SSIM; (1, 1) has no window at all.  The buffers are wider than the longest pair, so every pair has padding.
PAIRS = [(130, 67), (67, 130), (65, 64), (64, 65), (12, 11), (11, 12), (1, 1)]
TS, TR = 133, 132
LOG_LO, LOG_HI = float(np.log(1e-5)), 2.0

# the float32 just above 1.2: the smallest ratio f_syn / f_rec = RATIO_OVER on f_rec = 100 Hz that is a gross pitch error
F_REC = np.float32(100.0)
F_AT = np.float32(120.0)                                  # |120 - 100| = 20 = 0.2f * 100 in float32: not a gross error
F_OVER = np.nextafter(np.float32(120.0), np.float32(np.inf))


@functools.lru_cache(maxsize=None)
def inputs():
    """mel_syn [B, TS, 80], mel_rec [B, TR, 80]: log-mels random within [ln 1e-5, 2]; a recording is its rendering resampled to the pair's
    recording length plus 5 % noise; NaN beyond the lengths.  f0_syn [B, TS], f0_rec [B, TR]: 80 to 400 Hz with unvoiced runs, the
    recording's track the resampled rendering's times a ratio near 1, and the two boundary ratios planted where the identity row meets them;
    NaN beyond the lengths."""
    rs = np.random.RandomState(23)
    B = len(PAIRS)
    x = np.full((B, TS, 80), np.nan, np.float32)
    y = np.full((B, TR, 80), np.nan, np.float32)
    fx = np.full((B, TS), np.nan, np.float32)
    fy = np.full((B, TR), np.nan, np.float32)
    span = LOG_HI - LOG_LO
    for b, (xl, yl) in enumerate(PAIRS):
        x[b, :xl] = LOG_LO + span * rs.rand(xl, 80)
        idx = (np.arange(yl) * xl) // yl
        y[b, :yl] = np.clip(x[b, idx] + 0.05 * span * rs.standard_normal((yl, 80)), LOG_LO, LOG_HI)
        f = 80.0 + 320.0 * rs.rand(xl)
        f[rs.rand(xl) < 0.25] = 0.0                       # unvoiced frames, alone and in runs
        if xl > 20:
            f[5:9] = 0.0
        fx[b, :xl] = f
        g = fx[b, idx].astype(np.float64) * (1.0 + 0.15 * rs.standard_normal(yl))      # some beyond 20 %: gross errors
        g[rs.rand(yl) < 0.1] = 0.0                        # voicing decision errors
        fy[b, :yl] = g
        if xl > 20 and yl > 20:                           # frames 15 and 16 are matched to themselves by the identity row
            fx[b, 15], fy[b, 15] = F_AT, F_REC
            fx[b, 16], fy[b, 16] = F_OVER, F_REC
    return x, y, fx, fy


def lens():
    return np.asarray([p[0] for p in PAIRS], np.int32), np.asarray([p[1] for p in PAIRS], np.int32)


def cepstra_error_bound(mel, n, n_cep):
    """The forward bound of an 80-term float32 dot product, any order: 82 * 2^-24 * sum_n |mel[t, n]| |D[n, k]|, float64 [n, n_cep]."""
    D = np.abs(M.dct_table(80, n_cep).astype(np.float64))
    return 82.0 * 2.0 ** -24 * (np.abs(np.asarray(mel[:n], np.float64)) @ D)


def ulp32(a):
    """The spacing of float32 at |a| (float64 array)."""
    a = np.abs(np.asarray(a, np.float32))
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)
