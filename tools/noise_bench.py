#!/usr/bin/env python3
"""What the seeded sampler noise (csrc/noise_philox.hip) costs against the torch noise it can replace, at the headline shapes
(B = 32, T = 512, 80 mel bins, 4 sampling steps = 5 draws):

  fill     5 x torch.randn([32, 1, 512, 80])                 against one cmtts_noise_fill of 5 draws
  groups   the 32-utterance utterance_noise loop + stack     against one cmtts_noise_fill_groups launch (one group of 32)
  step     the headline-shaped step (duration net, noise, 4-step sampler) with torch.randn inside the step
                                                             against the same step with seeds (cmtts_sample_seeded)

Device events around windows of --calls calls, after warming every arm; the arms of a pair alternate window by window; median, min
and max over --reps windows.  On a build without cmtts_sample_seeded only the torch arms run (the run a seeded build is compared
against, in the same session on the same box).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, host  # noqa: E402
from cmtts_amd.config import get_config  # noqa: E402
from cmtts_amd.weights import synth_cmtts_state_dict  # noqa: E402

BATCH, PHONEMES, FRAMES, DUR, N_STEPS = 32, 85, 512, 6, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    torch.cuda.manual_seed(4321)
    seeded = "cmtts_sample_seeded" in _lib.SIGNATURES
    cfg = get_config("LJSpeech")
    model = host.CMTotalTTS(cfg, dev).load_state_dict(synth_cmtts_state_dict(cfg, seed=0, dur_frames=float(DUR), dur_spread=0.0))
    rs = np.random.RandomState(0)
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(BATCH, PHONEMES)).astype(np.int64)).to(dev)
    lens = torch.full((BATCH,), PHONEMES, dtype=torch.int64, device=dev)
    M, draws = cfg.n_mels, N_STEPS + 1
    keep = {}

    def fill_torch():
        keep["z"] = [torch.randn(BATCH, 1, FRAMES, M, device=dev) for _ in range(draws)]

    def loop_torch():
        keep["z"] = torch.stack([host.utterance_noise(0, i, draws, FRAMES, M, dev) for i in range(BATCH)], 1)

    def step_torch():
        out = model.duration_pitch_energy_net(None, texts, lens, max_mel_len=FRAMES)
        nz = torch.randn(draws, BATCH, 1, FRAMES, M, device=dev)
        keep["mel"] = host.sample_with_cond(model, out["cond_ct"], None, N_STEPS, nz, factors=out.get("cond_factors"))

    pairs = {"fill": [("torch_randn_x5", fill_torch)], "groups": [("utterance_noise_loop", loop_torch)], "step": [("torch_noise", step_torch)]}
    if seeded:
        from cmtts_amd import noise
        sv = torch.from_numpy(noise.utterance_seeds(1, np.arange(BATCH))).to(dev)

        def fill_seeded():
            keep["z"] = host.seeded_noise(sv, draws, FRAMES, M, dev)

        def groups_seeded():
            keep["z"] = host.seeded_noise_groups([(sv, FRAMES)], draws, M, dev)

        def step_seeded():
            out = model.duration_pitch_energy_net(None, texts, lens, max_mel_len=FRAMES)
            keep["mel"] = host.sample_with_cond(model, out["cond_ct"], None, N_STEPS, factors=out.get("cond_factors"), seeds=sv)

        pairs["fill"].append(("noise_fill", fill_seeded))
        pairs["groups"].append(("noise_fill_groups", groups_seeded))
        pairs["step"].append(("seeded", step_seeded))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.calls          # microseconds per call

    out = {"tool": "noise_bench", "B": BATCH, "T": FRAMES, "n_mels": M, "draws": draws, "calls": a.calls, "reps": a.reps, "seeded_build": seeded}
    for name, arms in pairs.items():
        for _, fn in arms:                                  # warm every arm's kernels and allocations
            for _ in range(3):
                fn()
        host.synchronize()
        times = {arm: [] for arm, _ in arms}
        for _ in range(a.reps):
            for arm, fn in arms:                            # alternating: drift hits both arms alike
                times[arm].append(window(fn))
        for arm, v in times.items():
            out[f"{name}_{arm}_us"] = {"median": round(float(np.median(v)), 1), "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}
        if len(arms) == 2:
            out[f"{name}_ratio"] = round(float(np.median(times[arms[1][0]]) / np.median(times[arms[0][0]])), 4)
    host.synchronize()
    assert torch.isfinite(keep["mel"]).all()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
