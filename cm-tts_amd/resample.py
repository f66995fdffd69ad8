"""Output sample rates and G.711 encoding: the definition (csrc/resample.hip) in executable form.

Pure numpy.  This is what the HIP kernel is tested against, NOT a fallback: host.vocoder_infer / vocoder_infer_stream with
sample_rate / encoding run resample.hip and nothing here except the tap design and the segment arithmetic.

    ratio     L / M = dst_rate / src_rate, reduced
    taps      Kaiser-windowed sinc on the x L grid: fc = rolloff * 0.5 / max(L, M), half = ceil(zeros / (2 fc)),
              h[n + half] = L * 2 fc * sinc(2 fc n) * kaiser(2 half + 1, beta)[n + half], n in [-half, half];
              float64, rounded ONCE to float32: those float32 values are the taps of every party
    resample  y[m] = sum_j x[j] * h[m M - j L + half], ceil((m M - half) / L) <= j <= floor((m M + half) / L), j ascending,
              x zero outside [0, n), 0 <= m < ceil(n L / M)      (= scipy.signal.upfirdn(h, x, up=L)[half::M])
    encode    "f32" y; "s16" saturate(trunc(y * max_wav_value)); "mulaw" / "alaw" ITU-T G.711 of that s16 value
    pieces    a piece [s0, s1) of the source yields outputs m in [ceil(s0 L / M), ceil(s1 L / M)) and needs source samples
              [s0 - R, s1 + R) (R = ceil(half / L)); the phase comes from the absolute m, so pieces concatenate to the whole
"""
from math import gcd

import numpy as np

NATIVE_RATE = 22050
HOP = 256                         # the streamed form carries one extra mel frame of margin: R <= HOP is required
ENCODINGS = {"f32": 0, "s16": 1, "mulaw": 2, "alaw": 3}          # include/cmtts_hip.h: CMTTS_ENC_*
DTYPES = {"f32": np.float32, "s16": np.int16, "mulaw": np.uint8, "alaw": np.uint8}
MAX_TABLE_FLOATS = 1 << 16        # csrc/resample.hip: the phase-major tap table [L][2 R + 1] holds at most this many floats


def ratio(src_rate, dst_rate):
    """(L, M) with dst_rate / src_rate = L / M in lowest terms."""
    src_rate, dst_rate = int(src_rate), int(dst_rate)
    if src_rate <= 0 or dst_rate <= 0:
        raise ValueError(f"ratio: rates must be positive, got {src_rate} -> {dst_rate}")
    g = gcd(src_rate, dst_rate)
    return dst_rate // g, src_rate // g


def half_width(L, half):
    """R: the filter's half-width in source samples."""
    return -(-int(half) // int(L))


def design_taps(L, M, zeros=16, beta=9.0, rolloff=0.95, hop=HOP):
    """float32 taps h[0 .. 2 half] of the L / M resampler and `half`.  Raises ValueError when the half-width in source samples
    exceeds `hop` (the streamed form's margin) or the phase table would not fit the kernel's tap storage."""
    L, M = int(L), int(M)
    if L <= 0 or M <= 0:
        raise ValueError(f"design_taps: L = {L}, M = {M}")
    fc = rolloff * 0.5 / max(L, M)
    half = int(np.ceil(zeros / (2.0 * fc)))
    R = half_width(L, half)
    if R > hop:
        raise ValueError(f"design_taps: {L}/{M} needs {R} source samples on each side, more than one frame ({hop}): "
                         "the streamed form carries one frame of margin")
    if L * (2 * R + 1) > MAX_TABLE_FLOATS:
        raise ValueError(f"design_taps: {L}/{M} needs a tap table of {L} x {2 * R + 1} floats, more than the kernel's "
                         f"{MAX_TABLE_FLOATS}")
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = L * 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(2 * half + 1, beta)
    return h.astype(np.float32), half


def out_len(n, L, M):
    """ceil(n L / M): output samples of n source samples."""
    return -(-int(n) * int(L) // int(M))


def term_range(m, L, M, half):
    """(j_lo, j_hi) inclusive: the source samples with a tap under output m (before clipping to [0, n))."""
    return -(-(m * M - half) // L), (m * M + half) // L


def resample(x, L, M, taps, m0=0, m1=None, origin=0, n=None):
    """The definition, in float64.  x float32: the source samples [origin, origin + len(x)) of an utterance of n samples (default:
    all of it, origin 0); returns y[m0:m1] (default: every output).  Samples outside [0, n) are zero; a sample inside [0, n) that a
    requested output needs and x does not hold is an error."""
    x = np.asarray(x, dtype=np.float32)
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    half = (len(h) - 1) // 2
    n = origin + len(x) if n is None else int(n)
    m1 = out_len(n, L, M) if m1 is None else int(m1)
    xd = x.astype(np.float64)
    y = np.zeros(max(m1 - m0, 0), np.float64)
    for i, m in enumerate(range(m0, m1)):
        lo, hi = term_range(m, L, M, half)
        lo, hi = max(lo, 0), min(hi, n - 1)
        if hi < lo:
            continue
        if lo < origin or hi >= origin + len(x):
            raise ValueError(f"resample: output {m} needs source samples [{lo}, {hi}], given [{origin}, {origin + len(x)})")
        j = np.arange(lo, hi + 1)
        y[i] = np.cumsum(xd[j - origin] * h[m * M - j * L + half])[-1]          # a running sum: j ascending
    return y


def plan_segments(pieces, n, L, M, half):
    """pieces: [(s0, s1)] absolute source-sample ranges of one utterance of n valid samples.  Returns per piece
    (m0, m1, need_lo, need_hi): the outputs [m0, m1) it yields and the source samples [need_lo, need_hi) it needs
    ([s0 - R, s1 + R) clipped to [0, n))."""
    R = half_width(L, half)
    plan = []
    for s0, s1 in pieces:
        s0, s1 = int(s0), int(s1)
        if not 0 <= s0 <= s1 <= n:
            raise ValueError(f"plan_segments: piece [{s0}, {s1}) outside [0, {n}]")
        plan.append((out_len(s0, L, M), out_len(s1, L, M), max(s0 - R, 0), min(s1 + R, n)))
    return plan


def phase_table(taps, L):
    """The kernel's tap table, float32 [L][2 R + 1]: row p, column d + R holds h[p - d L + half] (0 outside the taps), so that
    y[m] = sum over d = -R .. R of x[floor(m M / L) + d] * table[(m M) mod L][d + R], d ascending = j ascending."""
    h = np.asarray(taps, dtype=np.float32)
    half = (len(h) - 1) // 2
    R = half_width(L, half)
    p = np.arange(L)[:, None]
    d = np.arange(-R, R + 1)[None, :]
    idx = p - d * L + half
    ok = (idx >= 0) & (idx <= 2 * half)
    return np.where(ok, h[np.clip(idx, 0, 2 * half)], np.float32(0)).astype(np.float32)


# ---- encodings: exact integer functions

def to_s16(y, max_wav_value=32768.0):
    """trunc(float32(y) * float32(max_wav_value)) toward zero — cmtts_wav_to_int16's cast — then SATURATED to [-32768, 32767]
    (the native cast wraps; they agree wherever that one does not overflow)."""
    v = np.asarray(y).astype(np.float32) * np.float32(max_wav_value)
    return np.clip(np.trunc(v.astype(np.float64)), -32768, 32767).astype(np.int16)


_SEG_UEND = np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF])
_SEG_AEND = np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF])


def lin2ulaw(s16):
    """G.711 mu-law of int16 samples (the 14-bit magnitude of the sample >> 2, bias 33, clip 8159), uint8."""
    v = np.asarray(s16).astype(np.int32) >> 2
    neg = v < 0
    mag = np.minimum(np.where(neg, -v, v), 8159) + 0x21
    seg = np.searchsorted(_SEG_UEND, mag, side="left")           # first segment whose end is >= mag; 8: the clipped magnitude
    u = np.where(seg >= 8, 0x7F, (seg << 4) | ((mag >> (seg + 1)) & 0xF))
    return (u ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def lin2alaw(s16):
    """G.711 A-law of int16 samples (the 13-bit value sample >> 3), uint8."""
    v = np.asarray(s16).astype(np.int32) >> 3
    neg = v < 0
    mag = np.where(neg, -v - 1, v)
    seg = np.searchsorted(_SEG_AEND, mag, side="left")
    a = (seg << 4) | np.where(seg < 2, (mag >> 1) & 0xF, (mag >> np.maximum(seg, 1)) & 0xF)
    return (a ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def ulaw2lin(u):
    u = ~np.asarray(u).astype(np.int32) & 0xFF
    t = (((u & 0xF) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def alaw2lin(a):
    a = (np.asarray(a).astype(np.int32) ^ 0x55) & 0xFF
    seg = (a & 0x70) >> 4
    t = (a & 0xF) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


def encode(y, encoding, max_wav_value=32768.0):
    if encoding not in ENCODINGS:
        raise ValueError(f"encoding {encoding!r}: expected one of {sorted(ENCODINGS)}")
    if encoding == "f32":
        return np.asarray(y).astype(np.float32)
    s = to_s16(y, max_wav_value)
    return s if encoding == "s16" else lin2ulaw(s) if encoding == "mulaw" else lin2alaw(s)
