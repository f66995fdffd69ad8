"""Re-taking spans of an utterance: the definition (csrc/retake.hip) in executable form.

Pure numpy.  This is what the HIP kernels are tested against, NOT a fallback: host.retake runs cmtts_retake (the unchanged denoiser
on gathered frame windows, retake_step_kernel between its evaluations) and nothing here except the planner, which is host logic.

    sampler    the project's stochastic_iterative_sampler (karras_diffusion.py:830-854, with its 0.85) with the reference's
               replacement step (iterative_inpainting, karras_diffusion.py:985-1001): after every evaluation the KEPT frames of x0
               are put back before re-noising.  Kept frames of the result are the known values verbatim.
    halo       the denoiser has res_layers k = 3 convs with dilation 1 and is pointwise otherwise: one evaluation's output at frame f
               depends on its input at frames f - res_layers .. f + res_layers.  Kept frames are reset to known + noise after every
               evaluation, so a regenerated frame never sees further than res_layers frames, however many steps are taken: a span
               can be sampled on a window of span + 2 res_layers frames.
    noise      the seeded noise is a pure function of (seed, draw, ABSOLUTE frame, bin) (noise.py): a window draws what the whole
               utterance would.
"""
import numpy as np


def regen_mask(spans, B, T):
    """bool [B, T]: True inside the half-open frame intervals spans = [(b, lo, hi)].  ValueError for an empty, reversed or out-of-range span."""
    B, T = int(B), int(T)
    mask = np.zeros((B, T), bool)
    for b, lo, hi in spans:
        b, lo, hi = int(b), int(lo), int(hi)
        if not (0 <= b < B) or not (0 <= lo < hi <= T):
            raise ValueError(f"retake: span ({b}, {lo}, {hi}) is empty or outside B = {B}, T = {T}")
        mask[b, lo:hi] = True
    return mask


def schedule_from_ts(ts, steps, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """The general schedule of stochastic_iterative_sampler (karras_diffusion.py:838-852) as cmtts_schedule returns its own:
    (sigmas fp32 [n], renoise_std fp32 [n]) for the n = len(ts) - 1 evaluations, float64 arithmetic rounded once; the std does
    not include the 0.85."""
    ts = [int(t) for t in ts]
    steps = int(steps)
    if len(ts) < 2 or steps < 2 or any(t < 0 or t > steps - 1 for t in ts):
        raise ValueError(f"retake: ts = {ts} with steps = {steps}")
    tmax, tmin = float(sigma_max) ** (1 / rho), float(sigma_min) ** (1 / rho)
    sig = [(tmax + t / (steps - 1) * (tmin - tmax)) ** rho for t in ts]
    nxt = np.clip(np.asarray(sig[1:], np.float64), sigma_min, sigma_max)
    return np.asarray(sig[:-1], np.float32), np.sqrt(nxt ** 2 - float(sigma_min) ** 2).astype(np.float32)


def retake_reference(denoise, known, regen, z, sigmas, nstd, sigma_max=80.0, dtype=np.float32):
    """The masked sampler.  denoise(x [B,1,T,M], sigma [B]) -> x0; known [B,1,T,M]; regen bool [B,T] (True = regenerate);
    z [n_steps + 1,B,1,T,M] (draw 0 is x_T, draw 1 + i the re-noise after evaluation i; n_steps draws suffice when the last
    evaluation is not re-noised); sigmas, nstd [n_steps] as cmtts_schedule returns them (nstd without the 0.85; negative = no
    re-noising, the last evaluation only).  Returns [B,1,T,M] in `dtype`: every operation is rounded to it (fp32 is the kernels'
    arithmetic, float64 the yardstick).

        x = z[0] * sigma_max                                       every frame, kept ones too
        x0 = where(regen, denoise(x, sigmas[i]), known)
        x = x0 + (z[1 + i] * nstd[i]) * 0.85                       every frame, i < n_steps - 1
        last: regenerated frames x0 (+ the same term when nstd[i] >= 0), kept frames `known` verbatim — cmtts_schedule's last std
        is ~1e-10, not 0, and must not touch them."""
    F = np.dtype(dtype).type
    known = np.asarray(known).astype(F)
    B, one, T, M = known.shape
    mask = np.asarray(regen).astype(bool).reshape(B, 1, T, 1)
    n = len(sigmas)
    if n < 1 or len(nstd) != n or any(not (float(v) >= 0) for v in nstd[:-1]):
        raise ValueError("retake_reference: one nstd per sigma, only the last may be negative")
    x = (np.asarray(z[0]).astype(F) * F(sigma_max)).astype(F)
    for i in range(n):
        x0 = np.asarray(denoise(x, np.full((B,), sigmas[i], F))).astype(F)
        x0 = np.where(mask, x0, known)
        if float(nstd[i]) >= 0:
            term = ((np.asarray(z[1 + i]).astype(F) * F(nstd[i])).astype(F) * F(0.85)).astype(F)
            x = (x0 + term).astype(F)
        else:
            x = x0
    return np.where(mask, x, known)


def plan_retake_windows(spans, T, halo):
    """Windows of a retake: spans = [(b, lo, hi)] half-open frame intervals of utterances T frames long, halo = the denoiser's
    res_layers.  Returns (Tw, [(b, start, core_off, core_len)]) — the table of cmtts_retake, the format of plan_stream_windows.
    Spans of one utterance with fewer than `halo` kept frames between them interact (a frame between them is in reach of both) and
    form one cluster; the cluster's extent is the core of one window, which reaches at least `halo` frames beyond it on either side
    unless it is clamped at 0 or T — the only places where the whole run sees zero padding too.  Spans with a gap of at least `halo` get
    windows of their own.  All windows share one width: the widest core + 2 halo, rounded up to a multiple of 4; when T is at most
    that, Tw = T and every window starts at 0.  Cores of one utterance are disjoint.  ValueError for an empty, reversed or
    out-of-range span and for an empty list."""
    T, halo = int(T), int(halo)
    if T < 1 or halo < 0:
        raise ValueError(f"plan_retake_windows: T = {T}, halo = {halo}")
    per = {}
    for b, lo, hi in spans:
        b, lo, hi = int(b), int(lo), int(hi)
        if b < 0 or not (0 <= lo < hi <= T):
            raise ValueError(f"plan_retake_windows: span ({b}, {lo}, {hi}) is empty or outside [0, {T}]")
        per.setdefault(b, []).append((lo, hi))
    if not per:
        raise ValueError("plan_retake_windows: no spans")
    clusters = []
    for b in sorted(per):
        cur = None
        for lo, hi in sorted(per[b]):
            if cur is not None and lo - cur[1] < halo:
                cur[1] = max(cur[1], hi)
            else:
                cur = [lo, hi]
                clusters.append((b, cur))
    Tw = (max(c[1] - c[0] for _, c in clusters) + 2 * halo + 3) // 4 * 4
    if T <= Tw:
        return T, [(b, 0, lo, hi - lo) for b, (lo, hi) in clusters]
    windows = []
    for b, (lo, hi) in clusters:
        start = min(max(lo - halo, 0), T - Tw)
        windows.append((b, start, lo - start, hi - lo))
    return Tw, windows


def whole_windows(spans, T):
    """One whole-utterance window per utterance with spans (Tw = T): the yardstick the windowed plan is compared with."""
    T = int(T)
    ext = {}
    for b, lo, hi in spans:
        b, lo, hi = int(b), int(lo), int(hi)
        if b < 0 or not (0 <= lo < hi <= T):
            raise ValueError(f"whole_windows: span ({b}, {lo}, {hi}) is empty or outside [0, {T}]")
        e = ext.setdefault(b, [lo, hi])
        e[0], e[1] = min(e[0], lo), max(e[1], hi)
    if not ext:
        raise ValueError("whole_windows: no spans")
    return T, [(b, 0, lo, hi - lo) for b, (lo, hi) in sorted(ext.items())]


def retake_pcm_range(lo, hi, H, T):
    """The output frames whose samples can change when mel frames [lo, hi) change: [lo - H, hi + H) clipped to [0, T), H = the
    generator's receptive radius in frames (13 for V1)."""
    lo, hi, H, T = int(lo), int(hi), int(H), int(T)
    if not (0 <= lo < hi <= T) or H < 0:
        raise ValueError(f"retake_pcm_range: [{lo}, {hi}) with T = {T}, H = {H}")
    return max(lo - H, 0), min(hi + H, T)
