#!/usr/bin/env python3
"""What a new take of one span costs against synthesizing the batch again (host.retake / host.retake_pcm, csrc/retake.hip), at
B = 32, T = 512, 80 mel bins, one 40-frame span per utterance (at a different place in each), 4 sampling steps:

  mel      host.retake(spans)                               against host.sample_with_cond(seeds=) on the whole batch
  audio    host.retake + host.retake_pcm (int16 on the host) against sample_with_cond(seeds=) + vocoder_infer of the same batch

Both arms of a pair start from the same conditioning (the frame side is not timed: a retake under unchanged prosody re-uses it) and
end with their result where a caller reads it: the mel on the device, the PCM in host memory.  Device events around windows of
--calls calls, after warming every arm; the arms of a pair alternate window by window; median, min and max over --reps windows.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import host, noise, retake  # noqa: E402
from cmtts_amd.config import get_config, HifiGanConfig  # noqa: E402
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict  # noqa: E402

BATCH, FRAMES, SPAN, N_STEPS = 32, 512, 40, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retake_bench.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    cfg, hcfg = get_config("LJSpeech"), HifiGanConfig()
    model = host.CMTotalTTS(cfg, dev).load_state_dict(synth_cmtts_state_dict(cfg, seed=0))
    voc = host.Generator(hcfg, dev).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    g = torch.Generator().manual_seed(0)
    cond_ct = torch.randn(BATCH, cfg.hidden, FRAMES, generator=g).to(dev)
    seeds = noise.utterance_seeds(1, np.arange(BATCH))
    take = noise.utterance_seeds(2, np.arange(BATCH))
    rs = np.random.RandomState(0)
    spans = [(b, int(lo), int(lo) + SPAN) for b, lo in enumerate(rs.randint(0, FRAMES - SPAN + 1, size=BATCH))]
    mel = host.sample_with_cond(model, cond_ct, None, N_STEPS, seeds=seeds).clone()
    pcm_old = host.vocoder_infer(mel.transpose(1, 2), voc)
    Tw, wins = retake.plan_retake_windows(spans, FRAMES, cfg.res_layers)
    keep = {}

    def mel_full():
        keep["mel"] = host.sample_with_cond(model, cond_ct, None, N_STEPS, seeds=take)

    def mel_retake():
        keep["mel"] = host.retake(model, mel, cond_ct, None, spans, take, n_steps=N_STEPS)

    def audio_full():
        mel_full()
        keep["pcm"] = host.vocoder_infer(keep["mel"].transpose(1, 2), voc)

    def audio_retake():
        mel_retake()
        keep["pcm"] = host.retake_pcm(keep["mel"].transpose(1, 2), voc, pcm_old, spans)

    pairs = {"mel": [("sample_with_cond", mel_full), ("retake", mel_retake)],
             "audio": [("sample_and_vocode", audio_full), ("retake_and_retake_pcm", audio_retake)]}

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls          # milliseconds per call

    out = {"tool": "retake_bench", "B": BATCH, "T": FRAMES, "span": SPAN, "n_steps": N_STEPS, "windows": len(wins), "Tw": Tw,
           "calls": a.calls, "reps": a.reps}
    for name, arms in pairs.items():
        for _, fn in arms:                                  # warm every arm's kernels and allocations
            for _ in range(2):
                fn()
        host.synchronize()
        times = {arm: [] for arm, _ in arms}
        for _ in range(a.reps):
            for arm, fn in arms:                            # alternating: drift hits both arms alike
                times[arm].append(window(fn))
        for arm, v in times.items():
            out[f"{name}_{arm}_ms"] = {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
        out[f"{name}_ratio"] = round(float(np.median(times[arms[1][0]]) / np.median(times[arms[0][0]])), 4)
    host.synchronize()
    kept = ~torch.from_numpy(retake.regen_mask(spans, BATCH, FRAMES)).to(dev)
    assert torch.isfinite(keep["mel"]).all() and torch.equal(keep["mel"][kept], mel[kept])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
