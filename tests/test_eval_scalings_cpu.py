"""CPU: the sampler's fp32 scalings of one evaluation (cm-tts_amd/csrc/denoiser_side.hip: scalings, the one function the uniform loops, the mixed
sampler's table and the ragged shard call; reached through csrc/internal_hooks.h: cmtts_internal_eval_scalings) on the reference's own schedule
sigmas for T = 1, 2, 4 in each dataset config.  c_in, c_out and c_skip are add / multiply / divide / sqrt in fp32 — IEEE-exact operations — so they
must be BIT-equal to the same numpy float32 expressions.  The rescaled timestep goes through logf, another implementation than numpy's log: it
must lie within 2^-22 relative of 250 log(sigma) in float64 (logf's sub-ulp error plus one rounding of the product)."""
import numpy as np
import pytest

from cmtts_amd import _lib
from cmtts_amd.config import get_config
from oracle import cmtts_oracle as O

F32 = np.float32


@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
@pytest.mark.parametrize("n_steps", [1, 2, 4])
def test_eval_scalings(variant, n_steps):
    cfg = get_config(variant)
    sigmas, _ = O.multistep_schedule(n_steps, cfg)
    assert len(sigmas) == n_steps
    smin, sd = F32(cfg.sigma_min), F32(cfg.sigma_data)
    sd2 = sd * sd
    for sigma in sigmas:
        s = F32(sigma)
        got = _lib.internal_eval_scalings(s, smin, sd)
        dm = s - smin
        c_skip = sd2 / (dm * dm + sd2)
        rt = np.sqrt(s * s + sd2)
        c_out = dm * sd / rt
        c_in = F32(1.0) / rt
        want = np.asarray([c_in, c_out, c_skip], F32)
        assert want.dtype == F32 and got.dtype == F32
        assert got[:3].tobytes() == want.tobytes(), (variant, n_steps, float(s), got[:3], want)
        t64 = 250.0 * np.log(np.float64(s))
        assert abs(np.float64(got[3]) - t64) <= 2.0 ** -22 * abs(t64), (variant, n_steps, float(s), float(got[3]), t64)
