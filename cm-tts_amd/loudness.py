"""Integrated loudness (ITU-R BS.1770) and output gain: the definition (csrc/loudness.hip) in executable form.

Pure numpy, float64.  This is what the HIP kernels are tested against, NOT a fallback: host.vocoder_loudness / vocoder_infer with
loudness= run loudness.hip and nothing here.

    K-weighting  two biquads from the analogue prototypes by the bilinear transform, K = tan(pi f0 / fs): a high shelf (f0 1681.97 Hz,
                 +4 dB, Q 0.7072), then a high-pass (f0 38.135 Hz, Q 0.5003); at 48 kHz they are the BS.1770-4 table
    filter       x[0:n] from zero state, each biquad in transposed direct form II, stage 1 then stage 2
    blocks       0.4 s with a 0.1 s hop (fs % 10 == 0), only blocks wholly inside [0, n); z_j = mean square of block j,
                 l_j = -0.691 + 10 log10 z_j
    gates        absolute: l_j > -70; relative: l_j > -0.691 + 10 log10(mean of the absolutely gated z) - 10
    L            -0.691 + 10 log10(mean of the z that pass both); 0 < n < one block: one block [0, n), absolute gate only;
                 n == 0 or no block passes: -inf
    peak         max |x[0:n]|: the SAMPLE peak (no true-peak oversampling)
    gain         g = 10^((target - L) / 20), lowered to 10^(ceiling_db / 20) / peak where peak * g exceeds the ceiling; 1 when
                 L = -inf, target is NaN or peak == 0.  The gain enters before the resampler, one float32 multiplication per source
                 sample: y = resample(fl32(g * x)) by cmtts_amd.resample's definition
"""
import math

import numpy as np

NATIVE_RATE = 22050
SHELF_F0, SHELF_GAIN_DB, SHELF_Q, SHELF_VB_EXP = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HIGHPASS_F0, HIGHPASS_Q = 38.13547087602444, 0.5003270373238773
OFFSET = -0.691
ABSOLUTE_GATE = -70.0
RELATIVE_GATE = -10.0
MIN_RATE, MAX_RATE = 8000, 48000          # what cmtts_loudness_coefficients accepts


def k_weighting(fs):
    """((b0, b1, b2, a1, a2) of the high shelf, the same of the high-pass) at sample rate fs, float64."""
    fs = float(fs)
    if not fs > 0:
        raise ValueError(f"k_weighting: fs = {fs}")
    K = math.tan(math.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_GAIN_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    s1 = ((Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
          2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0)
    K = math.tan(math.pi * HIGHPASS_F0 / fs)
    a0 = 1.0 + K / HIGHPASS_Q + K * K
    s2 = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HIGHPASS_Q + K * K) / a0)
    return s1, s2


def block_sizes(fs):
    """(block, hop) in samples: 0.4 s and 0.1 s."""
    fs = int(fs)
    if fs <= 0 or fs % 10:
        raise ValueError(f"loudness: the sample rate must be a positive multiple of 10, got {fs}")
    return 4 * (fs // 10), fs // 10


def k_weight(x, fs=NATIVE_RATE, dtype=np.float64):
    """x filtered by both biquads from zero state, sample by sample in `dtype` (transposed direct form II, stage 1 then stage 2)."""
    t = np.dtype(dtype).type
    (b0, b1, b2, a1, a2), (c0, c1, c2, d1, d2) = [[t(v) for v in s] for s in k_weighting(fs)]
    xs = np.asarray(x, dtype=np.float32).astype(dtype)
    y = np.empty(len(xs), dtype)
    z1 = z2 = w1 = w2 = t(0)
    if t is np.float64:          # plain Python floats are float64 and much quicker than numpy scalars
        b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = map(float, (b0, b1, b2, a1, a2, c0, c1, c2, d1, d2))
        z1 = z2 = w1 = w2 = 0.0
        xs = xs.tolist()
    for i, v in enumerate(xs):
        u = b0 * v + z1
        z1 = b1 * v - a1 * u + z2
        z2 = b2 * v - a2 * u
        o = c0 * u + w1
        w1 = c1 * u - d1 * o + w2
        w2 = c2 * u - d2 * o
        y[i] = o
    return y


def _lk(z):
    return OFFSET + 10.0 * math.log10(z) if z > 0 else -math.inf


def block_loudness(y, fs=NATIVE_RATE):
    """(z, l): the mean squares and loudnesses of the blocks of a K-weighted signal y (one block [0, n) when 0 < n < 0.4 s)."""
    block, hop = block_sizes(fs)
    n = len(y)
    sq = np.asarray(y) * np.asarray(y)
    if n == 0:
        z = []
    elif n < block:
        z = [float(np.sum(sq, dtype=sq.dtype)) / n]
    else:
        z = [float(np.sum(sq[j * hop:j * hop + block], dtype=sq.dtype)) / block for j in range((n - block) // hop + 1)]
    return np.asarray(z, np.float64), np.asarray([_lk(v) for v in z], np.float64)


def gated_loudness(y, fs=NATIVE_RATE):
    """(L, n_blocks_total, n_blocks_gated) of a K-weighted signal y."""
    z, l = block_loudness(y, fs)
    block, _ = block_sizes(fs)
    keep = l > ABSOLUTE_GATE
    if len(y) >= block and keep.any():
        keep &= l > _lk(float(np.mean(z[keep]))) + RELATIVE_GATE
    if not keep.any():
        return -math.inf, len(z), 0
    return _lk(float(np.mean(z[keep]))), len(z), int(keep.sum())


def integrated_loudness(x, fs=NATIVE_RATE, dtype=np.float64):
    """(L in LKFS, n_blocks_total, n_blocks_gated) of the mono signal x.  dtype=np.float32 evaluates the same sequential recurrence and
    the block sums in float32: the yardstick of a float32 implementation's rounding, not a product path."""
    return gated_loudness(k_weight(x, fs, dtype), fs)


def sample_peak(x):
    """max |x[0:n]| (0 for n == 0): the sample peak, not the true peak."""
    x = np.asarray(x, dtype=np.float32)
    return float(np.max(np.abs(x))) if len(x) else 0.0


def gain_for(L, peak, target_lufs, ceiling_db=-1.0):
    """The linear gain that brings loudness L to target_lufs with the sample peak kept at or under ceiling_db dBFS."""
    L, peak, target = float(L), float(peak), float(target_lufs)
    if math.isinf(L) or math.isnan(L) or math.isnan(target) or peak == 0:
        return 1.0
    g = 10.0 ** ((target - L) / 20.0)
    ceil = 10.0 ** (float(ceiling_db) / 20.0)
    return ceil / peak if peak * g > ceil else g


def apply_gain(x, g):
    """fl32(g * x): what the resampler's staging line stores."""
    return (np.float32(g) * np.asarray(x, dtype=np.float32)).astype(np.float32)
