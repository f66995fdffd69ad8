"""Mixed step counts in one batch without a GPU: the ordering helpers and the numpy definition of the per-utterance sampler
(cmtts_amd/steps.py) and the argument checks of the C entry points (include/cmtts_hip.h: cmtts_sample_mixed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from cmtts_amd import _lib, retake as R, steps as S
from cmtts_amd.config import get_config
from retake_cases import cheap_denoise, default_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (4, 4, 2, 1, 1)
TS = ((0, 13, 26, 39), (0, 20, 39), (0, 39), (0, 39))        # general schedules, steps = 40: 3, 2, 1, 1 evaluations


# ----------------------------------------------------------------------------- order / active / validate

def test_order_is_stable_and_sorts():
    n = [1, 4, 2, 4, 1, 2, 4]
    perm = S.order(n)
    assert perm.dtype == np.int64 and perm.tolist() == [1, 3, 6, 2, 5, 0, 4]          # ties keep the caller's order
    assert [n[k] for k in perm] == [4, 4, 4, 2, 2, 1, 1]
    assert S.order([2, 2, 2]).tolist() == [0, 1, 2]
    assert S.order([4]).tolist() == [0] and S.active([4]) == [1, 1, 1, 1]
    assert S.order(np.asarray([1, 2], np.int32)).tolist() == [1, 0]
    rs = np.random.RandomState(0)
    for _ in range(50):
        n = rs.choice([1, 2, 4], size=int(rs.randint(1, 40)))
        perm = S.order(n)
        assert sorted(perm.tolist()) == list(range(n.size))
        s = n[perm]
        assert (np.diff(s) <= 0).all()
        for v in (1, 2, 4):          # stable within every count
            assert (np.diff(perm[s == v]) > 0).all()
        act = S.active(s)
        assert len(act) == s[0] and sum(act) == int(n.sum()) and act[0] == n.size


def test_active_prefixes():
    assert S.active(COUNTS) == [5, 3, 2, 2]
    assert S.active([12 * [4] + 12 * [2] + 16 * [1]][0]) == [40, 24, 12, 12]
    assert S.active([1, 1, 1]) == [3]


@pytest.mark.parametrize("bad", [[1, 2], [4, 2, 4], [2, 0], [0], [], [2, -1]])
def test_counts_rejected(bad):
    with pytest.raises(ValueError):
        S.validate(bad)
    with pytest.raises(ValueError):
        S.active(bad)


def test_increasing_counts_name_the_remedy():
    with pytest.raises(ValueError, match="steps.order"):
        S.validate([1, 4])


def test_validate_schedules():
    cfg = get_config("VCTK")
    sig, std = S.default_plan(COUNTS, cfg.sigma_min, cfg.sigma_max, cfg.rho)
    assert sig.shape == (4, 5) and sig.dtype == np.float32
    assert S.validate(COUNTS, sig, std).tolist() == list(COUNTS)
    for b, n in enumerate(COUNTS):          # column b is cmtts_schedule(n_b)
        s, d = default_schedule(cfg, n)
        assert np.array_equal(sig[:n, b], s) and np.array_equal(std[:n, b], d)
    assert std[0, 3] < 0 and std[0, 4] < 0          # a one-step utterance is not re-noised: negative at ITS last evaluation is fine
    bad = std.copy()
    bad[1, 0] = -1.0                                 # a negative std in the middle of a four-step utterance
    with pytest.raises(ValueError, match="last evaluation"):
        S.validate(COUNTS, sig, bad)
    bad = std.copy()
    bad[3, 0] = -1.0                                 # at its last: allowed
    S.validate(COUNTS, sig, bad)
    for v in (0.0, -1.0, np.nan, np.inf):
        bs = sig.copy()
        bs[1, 2] = v
        with pytest.raises(ValueError, match="sigma"):
            S.validate(COUNTS, bs, std)
    bs = sig.copy()
    bs[3, 2] = np.nan                                # not read: utterance 2 takes two evaluations
    S.validate(COUNTS, bs, std)
    with pytest.raises(ValueError):
        S.validate(COUNTS, sig[:3], std[:3])
    with pytest.raises(ValueError):
        S.validate(COUNTS, sig, None)


# ----------------------------------------------------------------------------- the definition

def _uniform_loop(z, sig, nstd, sigma_max, F):
    """The plain stochastic loop (karras_diffusion.py:830-854 with the 0.85) on a batch, written here."""
    x = (z[0].astype(F) * F(sigma_max)).astype(F)
    for i in range(len(sig)):
        x = cheap_denoise(x, np.full((x.shape[0],), sig[i], F))
        if nstd[i] >= 0:
            x = (x + ((z[1 + i].astype(F) * F(nstd[i])).astype(F) * F(0.85)).astype(F)).astype(F)
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mixed_reference_rows_are_uniform_runs(dtype):
    cfg = get_config("VCTK")
    B, T, M = len(COUNTS), 37, 6
    z = np.random.RandomState(1).standard_normal((5, B, 1, T, M)).astype(np.float32)
    sig, std = S.default_plan(COUNTS, cfg.sigma_min, cfg.sigma_max, cfg.rho)
    got = S.mixed_reference(cheap_denoise, z, sig, std, COUNTS, cfg.sigma_max, dtype)
    assert got.dtype == dtype and got.shape == (B, 1, T, M) and np.isfinite(got).all()
    for b, n in enumerate(COUNTS):
        s, d = default_schedule(cfg, n)
        alone = _uniform_loop(z[:, b:b + 1], s, d, cfg.sigma_max, dtype)
        assert alone.dtype == dtype and np.array_equal(got[b:b + 1], alone), b
    assert not np.array_equal(got[0], got[2])
    # the same utterance at another count gives another result: the counts matter
    other = S.mixed_reference(cheap_denoise, z, *S.default_plan((4, 4, 4, 1, 1), cfg.sigma_min, cfg.sigma_max, cfg.rho), (4, 4, 4, 1, 1),
                              cfg.sigma_max, dtype)
    assert np.array_equal(other[:2], got[:2]) and np.array_equal(other[3:], got[3:]) and not np.array_equal(other[2], got[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mixed_reference_general_schedules(dtype):
    cfg = get_config("VCTK")
    scheds = [R.schedule_from_ts(ts, 40, cfg.sigma_min, cfg.sigma_max, cfg.rho) for ts in TS]
    n, sig, std = S.plan_from_schedules(scheds)
    assert n.tolist() == [3, 2, 1, 1] and sig.shape == (3, 4)
    assert len({float(v) for v in sig[1, :2]}) == 2          # two sigmas inside one evaluation
    B, T, M = 4, 29, 5
    z = np.random.RandomState(2).standard_normal((4, B, 1, T, M)).astype(np.float32)
    got = S.mixed_reference(cheap_denoise, z, sig, std, n, cfg.sigma_max, dtype)
    for b, (s, d) in enumerate(scheds):
        assert np.array_equal(got[b:b + 1], _uniform_loop(z[:, b:b + 1], s, d, cfg.sigma_max, dtype)), b
    with pytest.raises(ValueError):
        S.plan_from_schedules(scheds[::-1])


# ----------------------------------------------------------------------------- C ABI

def test_cabi_symbols_and_argument_checks():
    text = open(os.path.join(ROOT, "include", "cmtts_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cmtts_sample_mixed", "cmtts_sample_mixed_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert "typedef struct cmtts_step_plan {" in text
    assert [n for n, _ in _lib.StepPlanStruct._fields_] == ["max_steps", "n_steps", "sigmas", "renoise_std"]
    assert ctypes.sizeof(_lib.StepPlanStruct) == 32
    assert hasattr(raw, "cmtts_internal_sample_rows") and "cmtts_internal_sample_rows" not in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cmtts_abi_version() == 8 and _lib.ABI_VERSION == 8          # entry points only: the revision stays
    ns = (ctypes.c_int32 * 2)(2, 1)
    f4 = (ctypes.c_float * 4)(80.0, 80.0, 80.0, 80.0)
    plan = _lib.StepPlanStruct(2, ctypes.cast(ns, ctypes.c_void_p), ctypes.cast(f4, ctypes.c_void_p), ctypes.cast(f4, ctypes.c_void_p))

    def call(h):
        return lib.cmtts_sample_mixed(h, 1, None, 1, None, 2, 8, ctypes.byref(plan), 1, 1, 0, None, None, None, 0, 0, None, None)

    assert call(None) == -1          # null model: CMTTS_E_INVALID
    assert lib.cmtts_sample_mixed_workspace_bytes(None, 2, 8, 2) == 0
    h = ctypes.c_void_p()
    cfg, cs = get_config("VCTK"), _lib.CMTTSConfigStruct()
    for name, _ in cs._fields_:
        setattr(cs, name, type(getattr(cs, name))(getattr(cfg, name)))
    assert lib.cmtts_create(ctypes.byref(cs), ctypes.byref(h)) == 0 and h.value
    try:
        q = lib.cmtts_sample_mixed_workspace_bytes
        assert q(h, 0, 48, 2) == 0 and q(h, -1, 48, 2) == 0 and q(h, 2, 0, 2) == 0 and q(h, 2, 48, 0) == 0
        assert 0 < q(h, 1, 48, 1) < q(h, 2, 48, 1) < q(h, 3, 48, 1)          # monotone in B
        assert q(h, 2, 48, 1) < q(h, 2, 48, 2) < q(h, 2, 48, 4)               # ... and in max_steps
        assert q(h, 2, 48, 4) >= lib.cmtts_sample_seeded_workspace_bytes(h, 2, 48, 4) + 4 * 2 * 24
        # a model that is not finalized is refused before anything else is looked at
        assert call(h) == -1
        assert b"finalized" in lib.cmtts_last_error()
    finally:
        lib.cmtts_destroy(h)
