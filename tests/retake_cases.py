"""Cases and helpers shared by test_retake_cpu.py and test_gpu_retake.py (re-taking spans of an utterance)."""
import numpy as np

from cmtts_amd import retake as R

# B = 3, T = 200 (the GPU tests' shape): one group of spans per property the kernels can get wrong
T_GPU = 200
SPAN_CASES = {
    "tile":  [(0, 60, 70)],                         # crosses a 64-frame tile
    "head":  [(1, 0, 9)],                           # clamped at 0
    "tail":  [(2, 191, 200)],                       # clamped at T
    "odd":   [(0, 101, 103)],                       # not quad-aligned
    "mixed": [(0, 60, 70), (1, 0, 9), (1, 191, 200), (2, 101, 103)],
}


def gap_spans(halo, near):
    """Two spans of utterance 0 with halo - 1 (near: one cluster) or halo (two windows) kept frames between them."""
    gap = halo - 1 if near else halo
    return [(0, 30, 36), (0, 36 + gap, 36 + gap + 5)]


def default_schedule(cfg, n_steps):
    """cmtts_schedule in numpy: (sigmas fp32 [n], nstd fp32 [n]); n_steps = 1 is one evaluation without re-noising."""
    if n_steps == 1:
        return np.asarray([cfg.sigma_max], np.float32), np.asarray([-1.0], np.float32)
    return R.schedule_from_ts((0,) * n_steps + (1,), 2, cfg.sigma_min, cfg.sigma_max, cfg.rho)


def cheap_denoise(x, sigma):
    """A stand-in denoiser with a reach of one frame: deterministic, nonlinear, any dtype."""
    s = np.asarray(sigma, x.dtype).reshape(-1, 1, 1, 1)
    p = np.pad(x, ((0, 0), (0, 0), (1, 1), (0, 0)))
    return (np.tanh((p[:, :, :-2] + x + x + p[:, :, 2:]) / (4 + s)) + x / (1 + s * s)).astype(x.dtype)


def windowed_reference(make_denoise, known, mask, z, sigmas, nstd, Tw, wins, sigma_max, dtype):
    """retake_reference window by window: known [B,1,T,M], mask bool [B,T], z [n,B,1,T,M] at absolute frames;
    make_denoise(b, frames) -> the callable for frames `frames` (a slice) of utterance b.  Only regenerated frames inside a window's
    core are written back."""
    out = np.asarray(known).astype(dtype).copy()
    for b, start, off, n in wins:
        sl = slice(start, start + Tw)
        m = np.zeros((1, Tw), bool)
        m[0, off:off + n] = mask[b, start + off:start + off + n]
        r = R.retake_reference(make_denoise(b, sl), known[b:b + 1, :, sl], m, z[:, b:b + 1, :, sl], sigmas, nstd, sigma_max, dtype)
        sel = np.nonzero(m[0])[0]
        out[b, 0, start + sel] = r[0, 0, sel]
    return out
