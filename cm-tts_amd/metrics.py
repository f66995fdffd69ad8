"""Objective metrics of a rendering against the recording it was made from: the definition in executable form.

numpy only — no torch, no GPU.  Like align.py, pitch.py and loudness.py this file is what the kernels (csrc/metrics.hip: cmtts_metric_*) are
tested against; it is not a fallback.

The reference reports SSIM, FFE and MCD (all_metrics.py: Cal.get_all) through librosa, pyworld, pysptk, fastdtw, pymcd and torchmetrics.
None of them can run beside the model, so no golden can be captured: the public recipes are restated here on the features the project already
makes on the device, and pinned analytically (tests/test_metrics_cpu.py).  Where this differs from the reference:

    cepstra    the orthonormal DCT-II of the project's own 80-channel natural-log mel (mel_from_audio), NOT WORLD / SPTK mel-cepstra
               (all_metrics.py:401-408) and not librosa's MFCC of a dB mel (all_metrics.py:360-361): an MCD from here is comparable within
               this project and not with the figures of the reference's README.
    cost       c[i, j] = sqrt(sum_{k_lo <= k <= k_hi} (cx[i, k] - cy[j, k])^2) in the difference form: log_spec_dB_dist without its constant
               (all_metrics.py:396-399), coefficients 1 .. 13 by default (c0, the level, is excluded), no mean removal.
    mcd        (10 sqrt 2 / ln 10) total / path_len with total and path_len from align.dtw on the float32 cost: pymcd's "dtw" mode
               (all_metrics.py:447-452) with this project's exact DTW in fastdtw's place.  align="frame": no DTW, i = j over min(x_len,
               y_len) frames, the float32 sum along the diagonal with j ascending.
    f0         counted on the recording's frames j < y_len against the rendering's frame row[j].  A voicing decision error is a frame with
               exactly one side voiced (f0_frame_error.py:47-48).  A gross pitch error is a both-voiced frame with |f_syn - f_rec| >
               0.2f * f_rec in float32 (one multiply, one subtract, one compare): the reference writes |est / (true + 1e-8) - 1| > 0.2
               (f0_frame_error.py:53-57); the multiplied form has no division to round, so the counts can be demanded bit for bit.
               mae_cents = mean |1200 log2(f_syn / f_rec)| is what the reference's compute_f0_rmse returns (all_metrics.py:327-329);
               rmse_cents is the root mean square its name promises; corr is Pearson's (all_metrics.py:306-310).
    ssim       Wang et al. 2004 as torchmetrics' default evaluates it (all_metrics.py:379-387) on the first C cepstra of both sides,
               aligned on the RECORDING's time axis (one frame per recording frame, not one per path point as all_metrics.py:365-366)
               and with each column divided by its L2 norm (all_metrics.py:368-369).  The data range is max - min over the pairs of ONE
               call (the reference takes it over the corpus).

Fixed orders (the kernels follow them; the results that are demanded bit for bit depend on them):
    f0_stats   double sums over the both-voiced frames: 64 interleaved partial sums (partial l takes frames j = l, l + 64, ... ascending,
               other frames add 0), joined by halving: p[:s] + p[s:2s] for s = 32, 16, 8, 4, 2, 1.  Two passes: the means of both tracks
               first, then the cents errors and the centred second moments.
    ssim_images  the column norms: four interleaved partial sums of squares in double, joined (0 + 1) + (2 + 3).
"""
import math

import numpy as np

from . import align as _align

N_MELS = 80
MAX_SIDE = _align.MAX_SIDE        # frames per side the device path takes
MCD_CONST = 10.0 * math.sqrt(2.0) / math.log(10.0)
GPE_THRESHOLD = np.float32(0.2)
SSIM_WIN, SSIM_SIGMA, SSIM_K1, SSIM_K2 = 11, 1.5, 0.01, 0.03
F0_LANES = 64


def dct_table(n_mels=N_MELS, n_cep=20):
    """Orthonormal DCT-II: D[n, 0] = sqrt(1 / N), D[n, k] = sqrt(2 / N) cos(pi (n + 1/2) k / N), made in double and rounded once to float32
    [n_mels, n_cep].  The float32 table is part of the definition."""
    n_mels, n_cep = int(n_mels), int(n_cep)
    if n_mels != N_MELS or not 1 <= n_cep <= N_MELS:
        raise ValueError(f"metrics.dct_table: n_mels must be {N_MELS} and 1 <= n_cep <= {N_MELS}, not ({n_mels}, {n_cep})")
    N = float(n_mels)
    n = np.arange(n_mels, dtype=np.float64)[:, None]
    k = np.arange(n_cep, dtype=np.float64)[None, :]
    D = math.sqrt(2.0 / N) * np.cos(math.pi * (n + 0.5) * k / N)
    D[:, 0] = math.sqrt(1.0 / N)
    return D.astype(np.float32)


def cepstra(mel, n, n_cep=20, dtype=np.float64):
    """mel [>= n, 80] (natural-log mel) -> c [n, n_cep], c[t, k] = sum_n mel[t, n] D[n, k] on the float32 table, in `dtype`.  float64 is the
    definition; float32 is the yardstick arm."""
    mel = np.asarray(mel)
    n = int(n)
    if mel.ndim != 2 or mel.shape[1] != N_MELS or not 0 <= n <= mel.shape[0]:
        raise ValueError(f"metrics.cepstra: mel must be [T, {N_MELS}] with 0 <= n <= T, not {mel.shape}, n = {n}")
    return mel[:n].astype(dtype) @ dct_table(N_MELS, n_cep).astype(dtype)


def _coef_range(k_lo, k_hi, width):
    k_lo, k_hi = int(k_lo), int(k_hi)
    if not 0 <= k_lo <= k_hi < width:
        raise ValueError(f"metrics: coefficients {k_lo} .. {k_hi} outside the {width} given")
    return k_lo, k_hi


def cost(cx, x_len, cy, y_len, k_lo=1, k_hi=13, dtype=np.float64):
    """cx [>= x_len, n_cep], cy [>= y_len, n_cep] -> c [x_len, y_len] in `dtype`: the Euclidean distance over coefficients k_lo .. k_hi."""
    cx, cy = np.asarray(cx), np.asarray(cy)
    if cx.ndim != 2 or cy.ndim != 2 or cx.shape[1] != cy.shape[1]:
        raise ValueError(f"metrics.cost: cepstra [T, n_cep] of one width expected, not {cx.shape}, {cy.shape}")
    k_lo, k_hi = _coef_range(k_lo, k_hi, cx.shape[1])
    x_len, y_len = int(x_len), int(y_len)
    if not (1 <= x_len <= cx.shape[0] and 1 <= y_len <= cy.shape[0]):
        raise ValueError(f"metrics.cost: lengths ({x_len}, {y_len}) outside the cepstra")
    x = cx[:x_len, k_lo:k_hi + 1].astype(dtype)
    y = cy[:y_len, k_lo:k_hi + 1].astype(dtype)
    c = np.empty((x_len, y_len), dtype)
    for i in range(x_len):
        d = x[i][None, :] - y
        c[i] = np.sqrt((d * d).sum(axis=1, dtype=dtype))
    return c


def diagonal(c):
    """align="frame": float32 c [Ts, Tr] -> (total float32: c[0, 0] + c[1, 1] + ... in float32, j ascending; the number of frames
    min(Ts, Tr))."""
    c = np.asarray(c)
    if c.dtype != np.float32 or c.ndim != 2:
        raise ValueError("metrics.diagonal: a float32 cost matrix expected")
    n = min(c.shape)
    s = np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(n):
            s = np.float32(s + c[j, j])
    return s, n


def mcd(total, path_len):
    """(10 sqrt 2 / ln 10) total / path_len: the product and the quotient in double, rounded once to float32."""
    return np.float32(MCD_CONST * np.float64(total) / np.float64(path_len))


def _identity_row(x_len, y_len):
    return np.minimum(np.arange(y_len), x_len - 1).astype(np.int32)


def _row(row, x_len, y_len):
    if row is None:
        return _identity_row(x_len, y_len)
    row = np.asarray(row)
    if row.shape != (y_len,):
        raise ValueError(f"metrics: row must hold one rendering frame per recording frame ({y_len}), not {row.shape}")
    return np.clip(row, 0, x_len - 1).astype(np.int32)


def _lane_sum(vals):
    """The fixed order of f0_stats: float64 vals [n] -> 64 interleaved partial sums, joined by halving."""
    n = len(vals)
    rows = (n + F0_LANES - 1) // F0_LANES
    padded = np.zeros(rows * F0_LANES, np.float64)
    padded[:n] = vals
    p = np.zeros(F0_LANES, np.float64)
    for r in padded.reshape(rows, F0_LANES):
        p = p + r
    s = F0_LANES // 2
    while s >= 1:
        p = p[:s] + p[s:2 * s]
        s //= 2
    return float(p[0])


def cents(f_syn, f_rec):
    """e = 1200 log2(f_syn / f_rec) in double: the quotient first, then one log2."""
    return 1200.0 * np.log2(np.asarray(f_syn, np.float64) / np.asarray(f_rec, np.float64))


def f0_stats(f0_syn, f0_rec, row=None):
    """f0_syn [x_len], f0_rec [y_len] in Hz with 0 = unvoiced, row int [y_len] or None (identity, clamped to x_len - 1) -> dict: the counts
    n, n_vv, n_gpe, n_vde (int), the rates ffe, gpe, vde (float32 of the double quotient) and rmse_cents, mae_cents, corr (float32 of the
    double result).  Undefined values are NaN: n_vv = 0, or a zero variance for corr.  The counts are always valid."""
    a_all, b = np.asarray(f0_syn, np.float32), np.asarray(f0_rec, np.float32)
    if a_all.ndim != 1 or b.ndim != 1 or len(a_all) < 1 or len(b) < 1:
        raise ValueError("metrics.f0_stats: two 1-D tracks of at least one frame expected")
    a = a_all[_row(row, len(a_all), len(b))]
    va, vb = a != 0, b != 0
    vv = va & vb
    with np.errstate(invalid="ignore", over="ignore"):
        gross = vv & (np.abs(a - b) > GPE_THRESHOLD * b)           # float32: one subtract, one multiply, one compare
    n, n_vv, n_gpe, n_vde = len(b), int(vv.sum()), int(gross.sum()), int((va != vb).sum())
    out = {"n": n, "n_vv": n_vv, "n_gpe": n_gpe, "n_vde": n_vde}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["ffe"] = np.float32(np.float64(n_gpe + n_vde) / np.float64(n))
        out["gpe"] = np.float32(np.float64(n_gpe) / np.float64(n_vv))
        out["vde"] = np.float32(np.float64(n_vde) / np.float64(n))
    nan = np.float32(np.nan)
    if n_vv == 0:
        out.update(rmse_cents=nan, mae_cents=nan, corr=nan)
        return out
    x = np.where(vv, a, 0).astype(np.float64)
    y = np.where(vv, b, 0).astype(np.float64)
    mx, my = _lane_sum(x) / n_vv, _lane_sum(y) / n_vv
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(vv, cents(np.where(vv, x, 1.0), np.where(vv, y, 1.0)), 0.0)
        dx, dy = np.where(vv, x - mx, 0.0), np.where(vv, y - my, 0.0)
        se2, sae = _lane_sum(e * e), _lane_sum(np.abs(e))
        sxx, syy, sxy = _lane_sum(dx * dx), _lane_sum(dy * dy), _lane_sum(dx * dy)
        out["rmse_cents"] = np.float32(math.sqrt(se2 / n_vv)) if se2 >= 0 else nan
        out["mae_cents"] = np.float32(sae / n_vv)
        out["corr"] = np.float32(sxy / math.sqrt(sxx * syy)) if sxx > 0 and syy > 0 else nan
    return out


def ssim_images(cx, cy, row=None, C=20):
    """cx [x_len, >= C], cy [y_len, >= C] float32 cepstra -> (u, v, (min, max)): a[j] = cx[row[j], :C], b[j] = cy[j, :C], each column
    divided by its L2 norm over the y_len frames (norm and quotient in double, the quotient rounded once to float32; a zero column stays
    zero).  u, v float32 [y_len, C]; min and max over both, float32."""
    cx, cy = np.asarray(cx, np.float32), np.asarray(cy, np.float32)
    C = int(C)
    if cx.ndim != 2 or cy.ndim != 2 or not 1 <= C <= min(cx.shape[1], cy.shape[1]) or len(cx) < 1 or len(cy) < 1:
        raise ValueError(f"metrics.ssim_images: cepstra [T, >= C] expected, not {cx.shape}, {cy.shape}, C = {C}")
    a = cx[_row(row, len(cx), len(cy)), :C]
    b = cy[:, :C]

    def unit(m):
        sq = m.astype(np.float64) ** 2
        part = []
        for g in range(4):
            s = np.zeros(C, np.float64)
            for r in sq[g::4]:
                s = s + r
            part.append(s)
        norm = np.sqrt((part[0] + part[1]) + (part[2] + part[3]))
        with np.errstate(invalid="ignore", divide="ignore"):
            q = m.astype(np.float64) / norm[None, :]
        return np.where(norm[None, :] > 0, q, 0.0).astype(np.float32)

    u, v = unit(a), unit(b)
    return u, v, (np.float32(min(u.min(), v.min())), np.float32(max(u.max(), v.max())))


def gaussian_window():
    """The 11 taps of the separable window: exp(-(t - 5)^2 / (2 sigma^2)), sigma = 1.5, normalised to sum 1 (double; summed t ascending)."""
    g = np.asarray([math.exp(-((t - SSIM_WIN // 2) ** 2) / (2.0 * SSIM_SIGMA * SSIM_SIGMA)) for t in range(SSIM_WIN)], np.float64)
    s = 0.0
    for t in range(SSIM_WIN):
        s += g[t]
    return g / s


def _index(mu_x, mu_y, e_xx, e_yy, e_xy, L):
    c1, c2 = (SSIM_K1 * float(L)) ** 2, (SSIM_K2 * float(L)) ** 2
    mxy = mu_x * mu_y
    mxx, myy = mu_x * mu_x, mu_y * mu_y
    num = (2.0 * mxy + c1) * (2.0 * (e_xy - mxy) + c2)
    den = (mxx + myy + c1) * ((e_xx - mxx) + (e_yy - myy) + c2)
    return num / den


def ssim_map(u, v, L):
    """The index of every window that lies inside the image, float64 [T - 10, C - 10]: the five moments (u, v, u u, v v, u v) filtered along
    time first, then along the coefficients, taps ascending."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    T, C = u.shape
    g = gaussian_window()
    maps = []
    for m in (u, v, u * u, v * v, u * v):
        t1 = np.zeros((T - 10, C), np.float64)
        for t in range(SSIM_WIN):
            t1 = t1 + g[t] * m[t:t + T - 10]
        t2 = np.zeros((T - 10, C - 10), np.float64)
        for t in range(SSIM_WIN):
            t2 = t2 + g[t] * t1[:, t:t + C - 10]
        maps.append(t2)
    return _index(*maps, L)


def ssim_map_direct(u, v, L):
    """The same by a double loop over the windows with the 11 x 11 window written out: the check of the separable evaluation."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    T, C = u.shape
    g = gaussian_window()
    w = g[:, None] * g[None, :]
    out = np.empty((T - 10, C - 10), np.float64)
    for r in range(T - 10):
        for c in range(C - 10):
            a, b = u[r:r + 11, c:c + 11], v[r:r + 11, c:c + 11]
            out[r, c] = _index((w * a).sum(), (w * b).sum(), (w * a * a).sum(), (w * b * b).sum(), (w * a * b).sum(), L)
    return out


def ssim(u, v, L):
    """Structural similarity of two images [T, C] with data range L: the mean over the (T - 10) x (C - 10) windows inside the image, taken in
    double and rounded to float32.  NaN when T < 11 or C < 11."""
    u, v = np.asarray(u), np.asarray(v)
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError(f"metrics.ssim: two images of one shape [T, C] expected, not {u.shape}, {v.shape}")
    if u.shape[0] < SSIM_WIN or u.shape[1] < SSIM_WIN:
        return np.float32(np.nan)
    m = ssim_map(u, v, L)
    return np.float32(m.sum() / m.size)


def score(mel_syn, x_len, mel_rec, y_len, f0_syn=None, f0_rec=None, align="dtw", mcd_coefs=(1, 13), ssim_coefs=20, data_range=None,
          cepstra_syn=None, cepstra_rec=None, cost_matrix=None):
    """One pair, through the float32 cepstra and the float32 cost.  cepstra_syn / cepstra_rec / cost_matrix: float32 arrays to use instead of the
    definition's own (a test passes the device's).  Returns {"mcd", "ssim", "row", "path_len", "total", "minmax"} and, with both F0 tracks,
    f0_stats' entries under "ffe", "gpe", "vde", "f0_rmse_cents", "f0_mae_cents", "f0_corr", "n", "n_vv", "n_gpe", "n_vde"."""
    if align not in ("dtw", "frame"):
        raise ValueError(f"metrics.score: align = {align!r}: expected 'dtw' or 'frame'")
    k_lo, k_hi = int(mcd_coefs[0]), int(mcd_coefs[1])
    C = int(ssim_coefs)
    n_cep = max(k_hi + 1, C)
    x_len, y_len = int(x_len), int(y_len)
    cx = cepstra(mel_syn, x_len, n_cep).astype(np.float32) if cepstra_syn is None else np.asarray(cepstra_syn, np.float32)[:x_len]
    cy = cepstra(mel_rec, y_len, n_cep).astype(np.float32) if cepstra_rec is None else np.asarray(cepstra_rec, np.float32)[:y_len]
    c = cost(cx, x_len, cy, y_len, k_lo, k_hi).astype(np.float32) if cost_matrix is None else np.ascontiguousarray(cost_matrix, np.float32)
    if align == "dtw":
        total, n, row = _align.dtw(c)
    else:
        total, n = diagonal(c)
        row = _identity_row(x_len, y_len)
    u, v, mm = ssim_images(cx, cy, row, C)
    L = float(mm[1]) - float(mm[0]) if data_range is None else float(data_range)
    out = {"mcd": mcd(total, n), "ssim": ssim(u, v, np.float32(L)), "row": row, "path_len": n, "total": total, "minmax": mm}
    if f0_syn is not None and f0_rec is not None:
        s = f0_stats(np.asarray(f0_syn)[:x_len], np.asarray(f0_rec)[:y_len], row)
        for k in ("ffe", "gpe", "vde", "n", "n_vv", "n_gpe", "n_vde"):
            out[k] = s[k]
        out["f0_rmse_cents"], out["f0_mae_cents"], out["f0_corr"] = s["rmse_cents"], s["mae_cents"], s["corr"]
    return out


def summarise(scores):
    """A list of score() dicts (or of dicts of numbers) -> the corpus means of every scalar entry they share, NaN entries left out of their
    mean (as Cal.get_metrics_by_list averages per-pair figures); {"pairs": how many}."""
    scores = list(scores)
    out = {"pairs": len(scores)}
    if not scores:
        return out
    for k in scores[0]:
        vals = [s[k] for s in scores if k in s and np.ndim(s[k]) == 0]
        if len(vals) != len(scores) or k in ("n", "n_vv", "n_gpe", "n_vde", "path_len", "total"):
            continue
        vals = np.asarray(vals, np.float64)
        good = vals[~np.isnan(vals)]
        out[k] = float(good.mean()) if len(good) else float("nan")
    return out
