"""Re-taking spans of an utterance without a GPU: the window planner, the numpy definition of the masked sampler
(cmtts_amd/retake.py) and the argument checks of the C entry points (include/cmtts_hip.h: cmtts_retake)."""
import ctypes
import os
import re

import numpy as np
import pytest

from cmtts_amd import _lib, noise as N, retake as R
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from oracle import cmtts_oracle as O
from retake_cases import SPAN_CASES, T_GPU, cheap_denoise, default_schedule, gap_spans, windowed_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALO = 20


# ----------------------------------------------------------------------------- planner

def _check_plan(spans, T, halo):
    Tw, wins = R.plan_retake_windows(spans, T, halo)
    assert Tw == T or (Tw % 4 == 0 and Tw < T)
    mask = R.regen_mask(spans, 1 + max(b for b, _, _ in spans), T)
    covered = np.zeros_like(mask)
    for b, start, off, n in wins:
        assert 0 <= start and start + Tw <= T and 0 <= off and n >= 1 and off + n <= Tw
        lo, hi = start + off, start + off + n
        assert not covered[b, lo:hi].any(), "cores of one utterance overlap"
        covered[b, lo:hi] = True
        assert mask[b, lo] and mask[b, hi - 1], "a core is the extent of its cluster"
        assert off >= halo or start == 0, (b, start, off, n)                      # reach to the left, unless clamped at 0
        assert Tw - off - n >= halo or start + Tw == T, (b, start, off, n)        # to the right, unless clamped at T
        if Tw == T:
            assert start == 0
        # every regenerated frame outside this core is out of reach of it: at least `halo` kept frames lie between
        other = mask[b].copy()
        other[lo:hi] = False
        near = np.nonzero(other[max(lo - halo, 0):min(hi + halo, T)])[0]
        assert near.size == 0, (b, lo, hi, near)
    assert not (mask & ~covered).any(), "a regenerated frame is in no core"
    return Tw, wins


@pytest.mark.parametrize("case", sorted(SPAN_CASES))
def test_plan_cases(case):
    Tw, wins = _check_plan(SPAN_CASES[case], T_GPU, HALO)
    widest = max(hi - lo for _, lo, hi in SPAN_CASES[case])
    assert Tw == (widest + 2 * HALO + 3) // 4 * 4
    assert len(wins) == len(SPAN_CASES[case])


def test_plan_clusters_by_gap():
    Tw, wins = _check_plan(gap_spans(HALO, near=True), T_GPU, HALO)          # halo - 1 kept frames between: they interact
    assert len(wins) == 1 and wins[0][3] == 6 + HALO - 1 + 5
    assert Tw == (6 + HALO - 1 + 5 + 2 * HALO + 3) // 4 * 4
    Tw, wins = _check_plan(gap_spans(HALO, near=False), T_GPU, HALO)         # halo kept frames: independent
    assert len(wins) == 2 and [w[3] for w in wins] == [6, 5]
    # overlapping and touching spans are one cluster; another utterance never joins
    _, wins = _check_plan([(0, 10, 20), (0, 15, 30), (0, 30, 31), (1, 12, 14)], T_GPU, HALO)
    assert [(w[0], w[1] + w[2], w[3]) for w in wins] == [(0, 10, 21), (1, 12, 2)]


def test_plan_short_utterance_and_random():
    Tw, wins = _check_plan([(0, 5, 9), (1, 30, 40)], 48, HALO)              # T <= widest + 2 halo: whole-utterance windows
    assert Tw == 48 and all(w[1] == 0 for w in wins)
    assert R.plan_retake_windows([(0, 5, 9)], 44, HALO) == (44, [(0, 0, 5, 4)])          # T = 4 + 2 halo: still whole
    assert R.plan_retake_windows([(0, 5, 9)], 45, HALO) == (44, [(0, 0, 5, 4)])          # one more: a window, clamped at 0
    assert R.plan_retake_windows([(0, 40, 44)], 45, HALO) == (44, [(0, 1, 39, 4)])       # ... clamped at T
    rs = np.random.RandomState(0)
    for _ in range(200):
        T = int(rs.randint(1, 300))
        halo = int(rs.randint(0, 25))
        spans = []
        for _ in range(int(rs.randint(1, 6))):
            lo = int(rs.randint(0, T))
            spans.append((int(rs.randint(0, 3)), lo, int(rs.randint(lo + 1, T + 1))))
        _check_plan(spans, T, halo)
    assert R.whole_windows([(1, 3, 5), (1, 40, 44), (0, 7, 8)], 50) == (50, [(0, 0, 7, 1), (1, 0, 3, 41)])


@pytest.mark.parametrize("spans", [[(0, 5, 5)], [(0, 9, 5)], [(0, -1, 5)], [(0, 190, 201)], [(-1, 0, 5)], []])
def test_plan_rejects(spans):
    with pytest.raises(ValueError):
        R.plan_retake_windows(spans, T_GPU, HALO)
    if spans:
        with pytest.raises(ValueError):
            R.regen_mask(spans, 3, T_GPU)


def test_pcm_range():
    assert R.retake_pcm_range(60, 70, 13, 200) == (47, 83)
    assert R.retake_pcm_range(0, 9, 13, 200) == (0, 22)
    assert R.retake_pcm_range(191, 200, 13, 200) == (178, 200)
    with pytest.raises(ValueError):
        R.retake_pcm_range(5, 5, 13, 200)


# ----------------------------------------------------------------------------- the definition

def _case(cfg, B, T, M, seed=3):
    rs = np.random.RandomState(seed)
    known = rs.standard_normal((B, 1, T, M)).astype(np.float32)
    z = N.reference_normals(N.utterance_seeds(seed, np.arange(B)), 5, T, M).astype(np.float32)
    return known, z


@pytest.mark.parametrize("n_steps", [1, 2, 4])
def test_kept_frames_bitwise_and_all_regen_is_the_plain_loop(n_steps):
    cfg = get_config("VCTK")
    B, T, M = 2, 40, 6
    known, z = _case(cfg, B, T, M)
    sig, nstd = default_schedule(cfg, n_steps)
    assert sig.dtype == np.float32 and (n_steps == 1 or 0 < nstd[-1] < 1e-6)      # the trap: the last std is tiny, not 0
    mask = R.regen_mask([(0, 11, 17), (1, 0, 3), (1, 37, 40)], B, T)
    got = R.retake_reference(cheap_denoise, known, mask, z, sig, nstd, cfg.sigma_max)
    assert got.dtype == np.float32 and got.shape == known.shape
    keep = ~mask[:, None, :, None] & np.ones_like(known, bool)
    assert np.array_equal(got[keep].view(np.uint32), known[keep].view(np.uint32))
    assert np.isfinite(got).all() and (got != known)[~keep].mean() > 0.99
    # everything regenerated = the plain stochastic loop (karras_diffusion.py:830-854 with the 0.85), written here
    F = np.float32
    x = z[0] * F(cfg.sigma_max)
    for i in range(n_steps):
        x = cheap_denoise(x, np.full((B,), sig[i], F))
        if nstd[i] >= 0:
            x = x + (z[1 + i] * F(nstd[i])) * F(0.85)
    assert x.dtype == np.float32
    full = R.retake_reference(cheap_denoise, known, np.ones((B, T), bool), z, sig, nstd, cfg.sigma_max)
    assert np.array_equal(full.view(np.uint32), x.view(np.uint32))
    with pytest.raises(ValueError):
        R.retake_reference(cheap_denoise, known, mask, z, [80.0, 80.0], [-1.0, 0.0], cfg.sigma_max)


def test_schedule_from_ts():
    cfg = get_config("VCTK")
    sig, nstd = R.schedule_from_ts((0, 13, 26, 39), 40, cfg.sigma_min, cfg.sigma_max, cfg.rho)
    osig, ostd = O.multistep_schedule(3, cfg, ts=(0, 13, 26, 39), steps=40)
    assert np.array_equal(sig, np.asarray(osig, np.float32)) and (np.diff(sig) < 0).all()
    assert np.allclose(nstd * 0.85, ostd, rtol=1e-6, atol=1e-12) and nstd[-1] < 1e-6
    with pytest.raises(ValueError):
        R.schedule_from_ts((0, 40), 40)


def test_oracle_window_equals_whole_at_res_layers_and_not_below():
    """The halo argument on the float64 oracle (as test_oracle_stitched_windows_equal_whole_mel does for the generator): the planner's
    window at halo = res_layers reproduces the whole-utterance retake on the span exactly; one frame less does not."""
    cfg = get_config("VCTK")
    sd = {k: np.asarray(v) for k, v in synth_cmtts_state_dict(cfg, seed=5).items()}
    NL, T, M = cfg.res_layers, 96, cfg.n_mels
    assert NL == HALO
    rs = np.random.RandomState(0)
    cond = rs.standard_normal((1, T, cfg.hidden)).astype(np.float32)
    spk = rs.standard_normal((1, cfg.hidden)).astype(np.float32)
    known = rs.standard_normal((1, 1, T, M)).astype(np.float32)
    z = N.reference_normals(N.utterance_seeds(3, np.arange(1)), 3, T, M).astype(np.float32)
    sig, nstd = default_schedule(cfg, 2)
    spans = [(0, 44, 50)]
    mask = R.regen_mask(spans, 1, T)

    def make(b, sl):
        return lambda x, s: O.karras_denoise(sd, cfg, x, s, cond[b:b + 1, sl], spk[b:b + 1])

    with O.precision("f64"):
        whole = windowed_reference(make, known, mask, z, sig, nstd, *R.whole_windows(spans, T), cfg.sigma_max, np.float64)
        gaps = {}
        for halo in (NL, NL - 1):
            Tw, wins = R.plan_retake_windows(spans, T, halo)
            assert Tw < T and wins[0][2] >= halo
            win = windowed_reference(make, known, mask, z, sig, nstd, Tw, wins, cfg.sigma_max, np.float64)
            assert np.array_equal(win[:, :, ~mask[0]], known[:, :, ~mask[0]].astype(np.float64))
            gaps[halo] = float(np.abs(win - whole)[:, :, mask[0]].max())
    assert whole.dtype == np.float64 and np.abs(whole[:, :, mask[0]] - known[:, :, mask[0]]).max() > 1e-3
    assert gaps[NL] == 0.0, gaps
    assert gaps[NL - 1] > 1e-14, gaps


# ----------------------------------------------------------------------------- C ABI

def test_cabi_symbols_and_argument_checks():
    text = open(os.path.join(ROOT, "include", "cmtts_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cmtts_retake", "cmtts_retake_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert hasattr(raw, "cmtts_internal_retake_step") and "cmtts_internal_retake_step" not in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cmtts_abi_version() == 8 and _lib.ABI_VERSION == 8          # entry points only: the revision stays
    f1 = (ctypes.c_float * 1)(80.0)
    assert lib.cmtts_retake(None, 1, 1, 1, None, 1, 1, 8, 1, 1, 8, 1, f1, f1, 1, 1, 0, None) == -1          # null model: CMTTS_E_INVALID
    assert lib.cmtts_retake_workspace_bytes(None, 1, 8) == 0
    h = ctypes.c_void_p()
    cfg, cs = get_config("VCTK"), _lib.CMTTSConfigStruct()
    for name, _ in cs._fields_:
        setattr(cs, name, type(getattr(cs, name))(getattr(cfg, name)))
    assert lib.cmtts_create(ctypes.byref(cs), ctypes.byref(h)) == 0 and h.value
    try:
        assert lib.cmtts_retake_workspace_bytes(h, 0, 48) == 0 and lib.cmtts_retake_workspace_bytes(h, 2, 0) == 0
        one, two = lib.cmtts_retake_workspace_bytes(h, 1, 48), lib.cmtts_retake_workspace_bytes(h, 2, 48)
        assert 0 < one < two
        # a model that is not finalized is refused before anything else is looked at
        assert lib.cmtts_retake(h, 1, 1, 1, None, 1, 1, 8, 1, 1, 8, 1, f1, f1, 1, 1, 0, None) == -1
        assert b"finalized" in lib.cmtts_last_error()
    finally:
        lib.cmtts_destroy(h)
