"""Shared inputs of the pitch tests (tests/test_pitch_cpu.py, tests/test_gpu_pitch.py): the smallest rows at which the kernels can go wrong,
the hand-made autocorrelation matrices of the tie rules, and the model's reconstruction of a contour from its CWT, restated."""
import functools

import numpy as np

from cmtts_amd import pitch as P

FS, HOP = P.SAMPLE_RATE, P.HOP
HALF = P.default_geometry().W // 2

# test_tracker_follows_the_rows: the worst relative f0 error of the float64 definition on the frames whose window lies wholly inside a voiced
# stretch, measured with numpy 2.2 on the rows of pitch_cases.rows(): glide 3.21e-4, mixed 7.99e-5, mixed_i16 7.97e-5 (the peak is
# refined by a parabola only).  Asserted with a margin of 2 x.
F0_ERR_MEASURED = 3.21e-4
# test_reconstruction_gives_the_contour_back: the worst relative error of cwt2f0(targets(f0)) against f0 on the voiced frames of the fully
# voiced rows: short 4.1e-4, glide 5.40e-2 — a property of the ten-scale wavelet sum (utils/pitch_tools.py:244-250), not of the tracker.
# Asserted with a margin of 2 x; tests/test_gpu_pitch.py uses the same bound end to end.
RECON_ERR_MEASURED = 5.40e-2


def harmonic(f_of_sample, amp=0.2):
    """Five harmonics at 1 / k, the phase by cumulative sum of the instantaneous frequency."""
    f = np.asarray(f_of_sample, np.float64)
    ph = 2.0 * np.pi * np.cumsum(f) / FS
    return amp * sum(np.sin(k * ph) / k for k in range(1, 6))


class Row:
    """wav float32 [n]; truth [n]: the f0 at each sample, 0 in noise and silence; stretches: (start, end, kind) with kind 'v' / 'u'."""

    def __init__(self, name, wav, truth, stretches):
        self.name, self.wav, self.truth, self.stretches = name, wav.astype(np.float32), truth, stretches
        self.n = wav.shape[0]
        self.T = 1 + self.n // HOP

    def frame_kinds(self):
        """Per frame: 'v' / 'u' when its window [hop f - W/2, hop f + W/2) lies wholly inside one stretch (the clip's ends count as the
        stretch going on: the samples outside are zeros, which a voiced frame at the edge tolerates but the bound is not asked of), else
        'x' (straddles a boundary, or reaches outside the clip)."""
        kinds = []
        for f in range(self.T):
            lo, hi = HOP * f - HALF, HOP * f + HALF
            k = "x"
            for a, b, kind in self.stretches:
                if lo >= a and hi <= b:
                    k = kind
            kinds.append(k)
        return kinds


@functools.lru_cache(maxsize=None)
def rows():
    rng = np.random.default_rng(20)
    out = []
    n = 513
    out.append(Row("short", harmonic(np.full(n, 200.0)), np.full(n, 200.0), [(0, n, "v")]))
    n = 4200
    f = np.linspace(110.0, 160.0, n)
    out.append(Row("glide", harmonic(f), f, [(0, n, "v")]))
    n = 8300
    a, b, c = 2600, 4400, 7000                                   # voiced | noise | voiced | silence
    f = np.zeros(n)
    f[:a] = 140.0
    f[b:c] = np.linspace(300.0, 250.0, c - b)
    wav = np.zeros(n)
    wav[:a] = harmonic(f[:a])
    wav[b:c] = harmonic(f[b:c])
    peak = np.abs(wav).max()
    wav[a:b] = rng.uniform(-1.0, 1.0, b - a) * peak * 10.0 ** (-26.0 / 20.0)      # a burst whose peak is 26 dB below the voiced peak
    mixed = Row("mixed", wav, f, [(0, a, "v"), (a, b, "u"), (b, c, "v"), (c, n, "u")])
    out.append(mixed)
    out.append(Row("zeros", np.zeros(4096), np.zeros(4096), [(0, 4096, "u")]))
    i16 = np.round(mixed.wav.astype(np.float64) * 32767.0).astype(np.int16)
    r = Row("mixed_i16", i16.astype(np.float64) / 32768.0, f, mixed.stretches)
    r.pcm = i16
    out.append(r)
    return tuple(out)


def batch(float_rows):
    """The float rows as one [B, n] float32 array, NaN beyond each row's samples, and the lengths."""
    n = max(r.n for r in float_rows)
    wav = np.full((len(float_rows), n + 7), np.nan, np.float32)
    for i, r in enumerate(float_rows):
        wav[i, :r.n] = r.wav
    return wav, np.array([r.n for r in float_rows], np.int32)


# ---- hand-made r for the tie rules: float32 [T, LMAX + 2] -------------------------------------------------------------------------------

def handmade():
    """name -> (r float32 [T, LMAX + 2], pk float32 [T])."""
    g = P.default_geometry()
    L = g.LMAX + 2
    rng = np.random.default_rng(5)
    out = {}

    def base(T, level=0.0):
        return np.full((T, L), level, np.float32), np.full(T, 0.5, np.float32)

    r, pk = base(6)
    r[:, 100:104] = 0.9                                        # a plateau: only its first cell is > its left and >= its right
    r[2:, 50] = 0.9                                            # from frame 2 on the same height at a shorter lag (the octave cost prefers it)
    out["plateaus"] = (r, pk)

    r, pk = base(5)
    for t in (40, 80, 160):
        r[:, t] = np.float32(0.8) + np.float32(P.OC) * (g.lg[t] - g.lg_floor)      # equal strengths after the octave cost, up to rounding
    r[3, 60] = r[3, 40]
    out["equal"] = (r, pk)

    r, pk = base(7)
    peaks = np.arange(g.LMIN + 1, g.LMAX, 9)                  # 27 maxima
    r[:, peaks] = rng.uniform(0.3, 0.95, (7, peaks.size)).astype(np.float32)
    r[4, peaks] = 0.7                                          # and a frame where all of them tie
    out["many"] = (r, pk)

    r, pk = base(6)
    r[:, 120] = 0.9
    r[1, 120] = np.nan
    r[2, 119] = np.nan
    r[3, 121] = np.nan
    r[4, :] = np.nan
    pk[5] = np.nan
    out["nan"] = (r, pk)

    r, pk = base(4)
    r[:, 70] = np.inf
    r[2, 140] = np.inf
    out["inf"] = (r, pk)

    out["zero"] = base(5)
    r, pk = base(5)
    pk[:] = 0.0
    out["zero_pk"] = (r, pk)

    for T in (1, 2):
        r, pk = base(T)
        r[:, 90] = 0.95
        r[T - 1, 200] = 0.97
        out[f"T{T}"] = (r, pk)

    r = rng.uniform(-0.3, 1.0, (40, L)).astype(np.float32)    # nothing smooth about it: every rule at once
    pk = rng.uniform(0.0, 1.0, 40).astype(np.float32)
    out["random"] = (r, pk)
    return out


def long_r(T, seed):
    """A long row for the Viterbi kernel: a few wandering peaks per frame over weak noise, stretches of silence in between."""
    g = P.default_geometry()
    rng = np.random.default_rng(seed)
    r = rng.uniform(-0.2, 0.35, (T, g.LMAX + 2)).astype(np.float32)
    pk = rng.uniform(0.2, 1.0, T).astype(np.float32)
    lag = 100.0
    for f in range(T):
        lag = float(np.clip(lag + rng.normal(0.0, 3.0), g.LMIN + 2, g.LMAX / 2 - 2))
        if (f // 97) % 3 == 2:
            pk[f] *= 0.01
            continue
        t = int(round(lag))
        r[f, t] = rng.uniform(0.6, 0.99)
        r[f, 2 * t] = rng.uniform(0.6, 0.99)
    return r, pk


CONTOUR_FRAMES = (3, 4, 16, 17, 33, 257)


def contours():
    """f0 rows (float32, 0 = unvoiced) for the targets: one per length of CONTOUR_FRAMES — a wandering contour with unvoiced runs in the
    interior and, from 16 frames on, at both ends — then a row without a voiced frame (status 1), one with a single voiced frame
    (status 2) and one of two frames (status 3)."""
    rng = np.random.default_rng(11)
    out = []
    for n in CONTOUR_FRAMES:
        f0 = (180.0 * np.exp(0.25 * np.sin(np.arange(n) / 7.0) + 0.05 * rng.standard_normal(n))).astype(np.float32)
        if n >= 16:
            f0[:2] = 0
            f0[-3:] = 0
            for s in range(5, n - 4, 23):
                f0[s:s + 1 + s % 4] = 0
        elif n == 4:
            f0[1] = 0
        out.append(f0)
    out.append(np.zeros(20, np.float32))
    one = np.zeros(9, np.float32)
    one[4] = 187.5
    out.append(one)
    out.append(np.array([100.0, 110.0], np.float32))
    return out


# ---- the model's reconstruction (utils/pitch_tools.py:244-272, restated): cwt_spec [T, 10], mean, std -> f0 [T] ---------------------------

def inverse_cwt(cwt_spec):
    w = np.asarray(cwt_spec, np.float64)
    b = (np.arange(w.shape[-1]) + 1 + 2.5) ** -2.5
    s = (w * b).sum(-1)
    return (s - s.mean(-1, keepdims=True)) / s.std(-1, ddof=1, keepdims=True)       # torch.std: unbiased


def cwt2f0(cwt_spec, mean, std):
    return np.exp(inverse_cwt(cwt_spec) * std + mean)
