"""Mixed step counts in one batch: per-utterance sampler schedules (cmtts_sample_mixed) in executable form.

Pure numpy.  This is what the HIP path is tested against, NOT a fallback: host.sample_with_cond with a sequence of step counts runs
cmtts_sample_mixed and nothing here except `order`, `active` and `validate`, which are host logic.

    definition   utterance b has n_b >= 1 evaluations with its own sigmas[b][0 .. n_b) and renoise_std[b][0 .. n_b).  Its result is row b
                 of the uniform sampler (karras_diffusion.py:801-811, 830-854, with the project's 0.85) run on that schedule.  The draw
                 numbering does not change: draw 0 is x_T, draw 1 + i the re-noise after evaluation i.
    batch        the utterances are ordered by non-increasing n_b, so the ones still evaluated at evaluation i are the PREFIX
                 [0, B_i), B_i = #{b : n_b > i}: every buffer of the denoiser is batch-major and a prefix is the same pointers with a
                 smaller B.  An utterance's last evaluation writes its result; it takes no part in later ones.
"""
import numpy as np

from . import retake


def order(n_steps):
    """Stable permutation into non-increasing step counts: order(n)[k] = the caller's index of the k-th utterance of the sorted batch
    (ties keep the caller's order).  int64 [B]."""
    n = np.asarray(n_steps, np.int64).reshape(-1)
    return np.argsort(-n, kind="stable").astype(np.int64)


def active(n_steps_sorted):
    """B_i = #{b : n_b > i} for every evaluation i in [0, n_steps_sorted[0]): the prefix evaluation i runs on.  Needs a non-increasing
    sequence of counts >= 1 (ValueError otherwise)."""
    n = _counts(n_steps_sorted)
    return [int((n > i).sum()) for i in range(int(n[0]))]


def _counts(n_steps):
    n = np.asarray(n_steps)
    if n.ndim != 1 or n.size < 1 or not np.issubdtype(n.dtype, np.integer):
        raise ValueError("steps: n_steps must be a non-empty sequence of ints")
    n = n.astype(np.int64)
    if (n < 1).any():
        raise ValueError(f"steps: every step count must be >= 1, got {n.tolist()}")
    if (np.diff(n) > 0).any():
        raise ValueError(f"steps: step counts must be non-increasing, got {n.tolist()}; sort the batch with steps.order")
    return n


def validate(n_steps, sigmas=None, renoise_std=None):
    """The checks of cmtts_sample_mixed on a plan.  n_steps: non-increasing ints >= 1 [B]; sigmas, renoise_std: [max_steps][B] (the
    layout of cmtts_step_plan; entry (i, b) is read only where i < n_steps[b]) — finite positive sigmas, and a negative std (no
    re-noising) only at an utterance's last evaluation.  Returns the counts as int64; ValueError otherwise."""
    n = _counts(n_steps)
    if (sigmas is None) != (renoise_std is None):
        raise ValueError("steps: give sigmas and renoise_std together")
    if sigmas is not None:
        sig, std = np.asarray(sigmas, np.float64), np.asarray(renoise_std, np.float64)
        if sig.shape != (int(n[0]), n.size) or std.shape != sig.shape:
            raise ValueError(f"steps: sigmas / renoise_std must be [max_steps = {int(n[0])}][B = {n.size}]")
        for b in range(n.size):
            for i in range(int(n[b])):
                if not (np.isfinite(sig[i, b]) and sig[i, b] > 0):
                    raise ValueError(f"steps: sigma of utterance {b}, evaluation {i} is not a finite positive number")
                if not (std[i, b] >= 0) and i != n[b] - 1:
                    raise ValueError(f"steps: utterance {b} has a negative renoise_std before its last evaluation ({i} of {int(n[b])})")
    return n


def default_plan(n_steps, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """The plan of the reference's own schedules (cmtts_schedule(n_b) per utterance): (sigmas, renoise_std) fp32 [max_steps][B], unused
    entries 0.  n = 1: one evaluation at sigma_max, no re-noising; n > 1: ts = (0,) * n + (1,) with steps = 2."""
    n = _counts(n_steps)
    sig = np.zeros((int(n[0]), n.size), np.float32)
    std = np.zeros_like(sig)
    for b, nb in enumerate(n.tolist()):
        if nb == 1:
            sig[0, b], std[0, b] = np.float32(sigma_max), np.float32(-1.0)
        else:
            sig[:nb, b], std[:nb, b] = retake.schedule_from_ts((0,) * nb + (1,), 2, sigma_min, sigma_max, rho)
    return sig, std


def plan_from_schedules(schedules):
    """[(sigmas [n_b], renoise_std [n_b])] per utterance, already in non-increasing length -> (n_steps int64 [B], sigmas, renoise_std
    fp32 [max_steps][B])."""
    n = _counts([len(s[0]) for s in schedules])
    sig = np.zeros((int(n[0]), n.size), np.float32)
    std = np.zeros_like(sig)
    for b, (s, d) in enumerate(schedules):
        if len(d) != len(s):
            raise ValueError("steps: one renoise_std per sigma")
        sig[:len(s), b], std[:len(s), b] = np.asarray(s, np.float32), np.asarray(d, np.float32)
    return n, sig, std


def mixed_reference(denoise, z, sigmas, nstd, n_steps, sigma_max=80.0, dtype=np.float32):
    """The mixed sampler as the batched loop over shrinking prefixes.  denoise(x [B',1,T,M], sigma [B']) -> x0 for any prefix B' of the
    batch, row-wise (row b depends on x[b] and sigma[b] alone); z [n_draws,B,1,T,M] (draw 0 is x_T, draw 1 + i the re-noise after
    evaluation i); sigmas, nstd [max_steps][B]; n_steps non-increasing [B].  Returns [B,1,T,M] in `dtype`, every operation rounded to it.

        x = z[0] * sigma_max
        evaluation i, rows [0, B_i):   x0 = denoise(x, sigmas[i]);  x = x0 + (z[1 + i] * nstd[i]) * 0.85  where nstd[i][b] >= 0, else x0
        row b leaves after evaluation n_b - 1: its x is the result and is not touched again."""
    F = np.dtype(dtype).type
    sig, std = np.asarray(sigmas), np.asarray(nstd)
    n = validate(n_steps, sig, std)
    z = np.asarray(z)
    B = n.size
    x = (z[0].astype(F) * F(sigma_max)).astype(F)
    out = np.empty_like(x)
    for i, Bi in enumerate(active(n)):
        x0 = np.asarray(denoise(x[:Bi], sig[i, :Bi].astype(F))).astype(F)
        re = std[i, :Bi] >= 0
        if re.any():
            term = ((z[1 + i][:Bi].astype(F) * std[i, :Bi].astype(F).reshape(Bi, 1, 1, 1)).astype(F) * F(0.85)).astype(F)
            x0 = np.where(re.reshape(Bi, 1, 1, 1), (x0 + term).astype(F), x0)
        x = x.copy()
        x[:Bi] = x0
        last = n[:Bi] == i + 1
        out[:Bi][last] = x0[last]
    assert B == out.shape[0]
    return out
