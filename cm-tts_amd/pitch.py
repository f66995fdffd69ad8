"""Pitch of a recording: F0 tracking and the CWT pitch targets, the definition in executable form.

numpy only — no torch, no GPU.  Like analysis.py and align.py this file is what the kernels (csrc/pitch.hip: cmtts_pitch_nacf,
cmtts_pitch_track, cmtts_pitch_targets) are tested against; it is not a fallback.

The reference makes these targets offline: utils/pitch_tools.py:81-118 (Praat's autocorrelation tracker through parselmouth: floor 80 Hz,
ceiling 750 Hz, voicing threshold 0.6, one value per hop) and preprocessor/preprocessor.py:408-414 (continuous log-f0, its mean and std,
a Mexican-hat CWT at 10 dyadic scales through pycwt).  Neither package can be pinned here, so this file restates the public recipes —
Boersma 1993 for the tracker, Torrence & Compo as pycwt 0.3.0a22 implements them for the CWT — and is pinned analytically
(tests/test_pitch_cpu.py).  It is NOT Praat bit for bit; it knowingly differs in the framing (frame f is centred on sample hop * f, the
centre of mel frame f of analysis.py's pad="reference"; the reference shifts Praat's frames by a fixed lpad instead) and in the peak
(a parabola through three lags; no sinc interpolation of the peak's height or place).

    nacf     frame f covers samples [hop f - W / 2, hop f + W / 2), W = 3 periods of the floor rounded up to even, zeros outside the clip.
             Mean removed, pk = max |x|, Hann window 0.5 - 0.5 cos(2 pi (i + 0.5) / W), a[tau] = sum_i x[i] x[i + tau] for tau = 0 ..
             LMAX + 1, r[tau] = a[tau] / a[0] / r_w[tau] with r_w the window's own normalised autocorrelation; all zeros when a[0] is
             not positive.
    track    on ANY float32 r, pk.  Candidates: integer lags in [LMIN, LMAX] with r[t] > r[t-1], r[t] >= r[t+1], r[t] > 0; strength
             r[t] - OC (lg[t] - lg_floor); the NC strongest (ties to the smaller lag), listed by ascending lag.  State 0 is unvoiced with
             strength VT + max(0, 2 - (pk / gpk) ((1 + VT) / ST)).  Viterbi maximises sum strength - sum transition (0 / VUC / OJC
             |lg[t1] - lg[t2]|); predecessors in ascending state order, a later one wins only if strictly greater; absent states hold
             -inf; the final state is the first maximum.  Every operation is one rounded float32 operation in the written order, so a
             kernel reproduces the path bit for bit.  f0 = fs / (t + delta), delta the vertex of the parabola through r[t-1], r[t],
             r[t+1] (0 unless concave); only f0 uses delta.
    targets  uv = (f0 == 0); convert_continuos_f0 (ends filled with the first / last voiced value, interior runs interpolated linearly);
             lf0 = log; mean, std (population) over the row; x = (lf0 - mean) / std; cwt_spec[:, j] = the real part of the DOG-2 CWT of x
             at s_j = 0.01 2^j, dt = 0.005, zero-padded to the next power of two: what get_lf0_cwt returns and dataset.py:103 loads.
             status 0 fine, 1 no voiced frame, 2 a constant contour (std == 0, tested as max == min so that it does not hang on the
             rounding of a mean), 3 fewer than 3 frames (pycwt's own omega_1 is negative at N = 2); for 1-3 cwt_spec is zeros, f0_std 1
             and f0_mean the single log value (0 for 1 and 3).
"""
import math

import numpy as np

SAMPLE_RATE = 22050
HOP = 256
FLOOR_HZ = 80.0
CEILING_HZ = 750.0
NC = 8                            # candidates kept per frame
VT = 0.6                          # voicing threshold (the reference's value)
ST = 0.03                         # silence threshold
OC = 0.01                         # octave cost
OJC = 0.35                        # octave-jump cost
VUC = 0.14                        # voiced / unvoiced cost
MAX_FRAMES = 4096                 # frames per row the device path takes
MAX_WINDOW = 2048
MAX_LAGS = 512

CWT_DT = 0.005
CWT_S0 = 0.01
CWT_SCALES = 10
CWT_MIN_N = 4

_f32 = np.float32


class Geometry:
    """Window, lag range and the host tables of one (fs, hop, floor, ceiling): what cmtts_pitch_create makes in double."""

    def __init__(self, fs=SAMPLE_RATE, hop=HOP, floor_hz=FLOOR_HZ, ceiling_hz=CEILING_HZ):
        fs, hop = int(fs), int(hop)
        if fs < 1 or hop < 1 or not (0.0 < float(floor_hz) < float(ceiling_hz) <= fs / 2.0):
            raise ValueError("pitch: fs >= 1, hop >= 1 and 0 < floor < ceiling <= fs / 2")
        self.fs, self.hop, self.floor_hz, self.ceiling_hz = fs, hop, float(floor_hz), float(ceiling_hz)
        w = int(math.ceil(3.0 * fs / self.floor_hz))
        self.W = w + (w & 1)
        self.LMIN = int(math.ceil(fs / self.ceiling_hz))
        self.LMAX = int(math.floor(fs / self.floor_hz))
        if self.W > MAX_WINDOW or self.LMAX + 2 > MAX_LAGS or self.LMIN < 1 or self.LMIN > self.LMAX or self.LMAX + 2 > self.W:
            raise ValueError(f"pitch: unsupported geometry (window {self.W} > {MAX_WINDOW} or {self.LMAX + 2} lags > {MAX_LAGS})")
        self.window = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(self.W) + 0.5) / self.W)
        rw = _acf(self.window, self.LMAX + 1)
        self.r_w = rw / rw[0]
        self.lg = np.concatenate([[0.0], np.log2(np.arange(1, self.LMAX + 2, dtype=np.float64))]).astype(np.float32)
        self.lg_floor = _f32(math.log2(fs / self.floor_hz))

    def frame_count(self, n):
        return 1 + int(n) // self.hop


_default = None


def default_geometry():
    global _default
    if _default is None:
        _default = Geometry()
    return _default


def _acf(x, L):
    """a[tau] = sum_i x[i] x[i + tau], tau = 0 .. L, in x's dtype."""
    xp = np.concatenate([x, np.zeros(L + 1, x.dtype)])
    S = np.lib.stride_tricks.sliding_window_view(xp, x.shape[0])[:L + 1]
    return S @ x


def as_samples(wav, dtype=np.float64):
    """float audio clipped to [-1, 1], or int16 / 32768 (what cmtts_mel_analysis and cmtts_pitch_nacf take)."""
    wav = np.asarray(wav)
    if wav.ndim != 1:
        raise ValueError("pitch: one row of audio expected")
    if wav.dtype == np.int16:
        return wav.astype(dtype) / dtype(32768.0)
    if wav.dtype.kind != "f":
        raise ValueError(f"pitch: float or int16 audio expected, not {wav.dtype}")
    return np.clip(wav.astype(dtype), -1.0, 1.0)


def nacf(wav, geo=None, dtype=np.float64):
    """wav [n] -> (r [T, LMAX + 2], pk [T]) in `dtype`, T = 1 + n // hop.  float64 is the definition; float32 — numpy's float32 mean,
    products and sums — is the yardstick arm the kernel's bound is derived from."""
    g = geo or default_geometry()
    x = as_samples(wav, dtype)
    n, W, L = x.shape[0], g.W, g.LMAX + 1
    T = g.frame_count(n)
    pad = np.concatenate([np.zeros(W // 2, dtype), x, np.zeros(W // 2 + g.hop, dtype)])
    win, rw = g.window.astype(dtype), g.r_w.astype(dtype)
    r, pk = np.zeros((T, L + 1), dtype), np.zeros(T, dtype)
    for f in range(T):
        fr = pad[f * g.hop:f * g.hop + W]
        fr = fr - fr.mean(dtype=dtype)
        pk[f] = np.abs(fr).max()
        a = _acf(fr * win, L)
        if a[0] > 0:
            r[f] = a / a[0] / rw
    return r, pk


def unvoiced_strength(pk):
    """State 0's strength per frame, float32, from float32 pk [T]; gpk = the largest pk that is a number (0 if none is positive)."""
    pk = np.asarray(pk, np.float32)
    ok = pk[~np.isnan(pk)]
    gpk = _f32(max(float(ok.max()), 0.0)) if ok.size else _f32(0.0)
    out = np.full(pk.shape, _f32(VT), np.float32)
    if gpk > 0:
        K = (_f32(1.0) + _f32(VT)) / _f32(ST)
        with np.errstate(invalid="ignore", over="ignore"):
            s = _f32(2.0) - (pk / gpk) * K
            out = _f32(VT) + np.where(s > 0, s, _f32(0.0)).astype(np.float32)
    return out


def candidates(r, geo=None):
    """float32 r [T, LMAX + 2] -> (lag int32 [T, NC] ascending with 0 for none, strength float32 [T, NC] with -inf for none)."""
    g = geo or default_geometry()
    r = np.asarray(r)
    if r.dtype != np.float32 or r.ndim != 2 or r.shape[1] != g.LMAX + 2:
        raise ValueError(f"pitch.track: r must be float32 [T, {g.LMAX + 2}]")
    T, lo, hi = r.shape[0], g.LMIN, g.LMAX
    with np.errstate(invalid="ignore", over="ignore"):
        c = r[:, lo:hi + 1]
        is_c = (c > r[:, lo - 1:hi]) & (c >= r[:, lo + 1:hi + 2]) & (c > 0)
        R = c - _f32(OC) * (g.lg[lo:hi + 1] - g.lg_floor)
    lag = np.zeros((T, NC), np.int32)
    stren = np.full((T, NC), -np.inf, np.float32)
    for f in range(T):
        idx = np.nonzero(is_c[f])[0]
        if idx.size > NC:
            s = R[f, idx]
            idx = np.sort(idx[np.lexsort((idx, -s))[:NC]])
        lag[f, :idx.size] = idx + lo
        stren[f, :idx.size] = R[f, idx]
    return lag, stren


def track(r, pk, geo=None):
    """float32 r [T, LMAX + 2], pk [T] -> (lag int32 [T], 0 = unvoiced; f0 float32 [T], 0 where unvoiced)."""
    g = geo or default_geometry()
    r = np.asarray(r)
    pk = np.asarray(pk)
    if pk.dtype != np.float32 or pk.shape != r.shape[:1]:
        raise ValueError("pitch.track: pk must be float32 [T]")
    clag, cstr = candidates(r, g)
    T = r.shape[0]
    if T == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float32)
    S = NC + 1
    stren = np.concatenate([unvoiced_strength(pk)[:, None], cstr], axis=1)            # [T, 9]
    lags = np.concatenate([np.zeros((T, 1), np.int32), clag], axis=1)
    lgc = g.lg[lags]                                                                  # 0 for state 0 and absent states
    absent = np.concatenate([np.zeros((T, 1), bool), clag == 0], axis=1)
    bp = np.zeros((T, S), np.int8)
    D = stren[0].copy()
    D[absent[0]] = -np.inf
    ninf = _f32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(1, T):
            best = D[0] - np.full(S, _f32(VUC), np.float32)
            best[0] = D[0]
            bi = np.zeros(S, np.int8)
            for p in range(1, S):
                tc = _f32(OJC) * np.abs(lgc[f - 1, p] - lgc[f])
                tc[0] = _f32(VUC)
                v = D[p] - tc
                win = v > best
                best = np.where(win, v, best)
                bi = np.where(win, np.int8(p), bi)
            D = (best + stren[f]).astype(np.float32)
            D[absent[f]] = ninf
            bi[absent[f]] = 0
            bp[f] = bi
        c, top = 0, D[0]
        for k in range(1, S):
            if D[k] > top:
                c, top = k, D[k]
        state = np.zeros(T, np.int64)
        for f in range(T - 1, -1, -1):
            state[f] = c
            c = int(bp[f, c])
        lag = lags[np.arange(T), state].astype(np.int32)
        f0 = np.zeros(T, np.float32)
        v = np.nonzero(lag > 0)[0]
        if v.size:
            t = lag[v]
            a, b, cc = r[v, t - 1], r[v, t], r[v, t + 1]
            den = (a - _f32(2.0) * b) + cc
            with np.errstate(divide="ignore"):
                d = np.where(den < 0, (_f32(0.5) * (a - cc)) / den, _f32(0.0)).astype(np.float32)
                f0[v] = _f32(g.fs) / (t.astype(np.float32) + d)
    return lag, f0


def convert_continuos_f0(f0):
    """utils/pitch_tools.py:138-169 on float64 f0 [T] with at least one non-zero value: the first / last voiced value fills the ends,
    interior unvoiced runs are interpolated linearly (scipy's interp1d: slope (x - x_lo) + y_lo)."""
    f0 = np.asarray(f0, np.float64)
    nz = np.nonzero(f0 != 0)[0]
    if nz.size == 0:
        raise ValueError("convert_continuos_f0: no voiced frame")
    t = np.arange(f0.shape[0])
    hi = np.searchsorted(nz, t, side="left")                  # first voiced index >= t (nz.size if none)
    lo = np.searchsorted(nz, t, side="right") - 1             # last voiced index <= t (-1 if none)
    out = np.empty_like(f0)
    for k in range(f0.shape[0]):
        if lo[k] < 0:
            out[k] = f0[nz[0]]
        elif hi[k] >= nz.size:
            out[k] = f0[nz[-1]]
        elif nz[lo[k]] == nz[hi[k]]:
            out[k] = f0[k]
        else:
            x0, x1 = nz[lo[k]], nz[hi[k]]
            slope = (f0[x1] - f0[x0]) / float(x1 - x0)
            out[k] = slope * float(k - x0) + f0[x0]
    return out


def cwt_scales():
    return CWT_S0 * 2.0 ** np.arange(CWT_SCALES)


def psi_ft(w):
    """The DOG-2 (Mexican hat) wavelet in frequency, pycwt's MexicanHat.psi_ft: w^2 exp(-w^2 / 2) / sqrt(Gamma(2.5))."""
    w = np.asarray(w, np.float64)
    return w ** 2 * np.exp(-0.5 * w ** 2) / math.sqrt(math.gamma(2.5))


def cwt_length(T):
    """The transform length of a row of T frames: the next power of two, 4 at the least."""
    n = CWT_MIN_N
    while n < T:
        n *= 2
    return n


def _cwt_factor(N):
    w = 2.0 * np.pi * np.fft.fftfreq(N, CWT_DT)
    s = cwt_scales()[:, None]
    return np.sqrt(s * w[1] * N) * psi_ft(s * w)              # [10, N]; real, so its conjugate is itself


def cwt_fft(x):
    """pycwt.cwt(x, dt, 1, 2 dt, 9, MexicanHat()), real part, transposed: float64 x [T >= 3] -> [T, 10]."""
    x = np.asarray(x, np.float64)
    T = x.shape[0]
    if x.ndim != 1 or T < 3:
        raise ValueError("cwt: one row of at least 3 frames")
    N = cwt_length(T)
    return np.real(np.fft.ifft(np.fft.fft(x, N)[None, :] * _cwt_factor(N), axis=1))[:, :T].T.copy()


def cwt_table(N):
    """h [10, N]: the periodised wavelet of transform length N, the inverse DFT of the factor (real and even)."""
    if N < CWT_MIN_N or N & (N - 1):
        raise ValueError("cwt_table: N must be a power of two >= 4")
    return np.real(np.fft.ifft(_cwt_factor(N), axis=1))


def cwt_direct(x, dtype=np.float64):
    """The form the kernel uses: W[t, j] = sum_{u < T} x[u] h_j[(t - u) mod N].  float32: x, table and sums in float32 (the yardstick arm)."""
    x = np.asarray(x, np.float64)
    T = x.shape[0]
    if x.ndim != 1 or T < 3:
        raise ValueError("cwt: one row of at least 3 frames")
    N = cwt_length(T)
    h = cwt_table(N).astype(dtype)
    idx = (np.arange(T)[:, None] - np.arange(T)[None, :]) % N
    xd = x.astype(dtype)
    return np.stack([h[j][idx] @ xd for j in range(CWT_SCALES)], axis=1)


def targets(f0):
    """f0 [T] (0 = unvoiced) -> {"cwt_spec" float64 [T, 10], "f0_mean", "f0_std", "uv" bool [T], "status"}."""
    f0 = np.asarray(f0, np.float64)
    if f0.ndim != 1:
        raise ValueError("pitch.targets: one row expected")
    T = f0.shape[0]
    uv = f0 == 0
    out = {"cwt_spec": np.zeros((T, CWT_SCALES)), "f0_mean": 0.0, "f0_std": 1.0, "uv": uv, "status": 0}
    if T < 3:
        out["status"] = 3
        return out
    if uv.all():
        out["status"] = 1
        return out
    lf0 = np.log(convert_continuos_f0(f0))
    if lf0.max() == lf0.min():
        out["status"], out["f0_mean"] = 2, float(lf0[0])
        return out
    mean, std = float(np.mean(lf0)), float(np.std(lf0))
    out["f0_mean"], out["f0_std"] = mean, std
    out["cwt_spec"] = cwt_fft((lf0 - mean) / std)
    return out
