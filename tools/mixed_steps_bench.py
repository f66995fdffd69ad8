#!/usr/bin/env python3
"""Mixed step counts against a tier per batch: LJSpeech config, 32 utterances of 512 frames, fp32 default form, seeded
noise.  Three arms, alternated in one process, device events around every call with a final synchronise:
  (a) one uniform call, 32 x T = 4;
  (b) one mixed call, 16 x T = 4 + 16 x T = 1 (cmtts_sample_mixed);
  (c) the two uniform calls a tier-per-batch server makes for the same requests, 16 x T = 1 then 16 x T = 4, back to back.
Prints the median, the min-max spread and the utterance-evaluations of each arm; --md appends a markdown table to a file.  Needs a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cmtts_amd import _lib, host, noise as N
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mixed_steps_bench: needs a GPU (a CPU run is not a timing)")
    B, T, half = a.batch, a.frames, a.batch // 2
    cfg = get_config("LJSpeech")
    model = host.CMTotalTTS(cfg, "cuda:0").load_state_dict(synth_cmtts_state_dict(cfg, seed=0))
    g = torch.Generator().manual_seed(0)
    cond = torch.randn(B, cfg.hidden, T, generator=g).cuda()
    lo, hi = cond[:half].contiguous(), cond[half:].contiguous()          # hi: the T = 1 drafts (the batch is sorted by step count)
    seeds = N.utterance_seeds(1, np.arange(B))
    counts = [4] * half + [1] * (B - half)
    rows = {}

    def arm_a():
        host.sample_with_cond(model, cond, None, 4, seeds=seeds)
        rows["a"] = _lib.internal_sample_rows()

    def arm_b():
        host.sample_with_cond(model, cond, None, counts, seeds=seeds)
        rows["b"] = _lib.internal_sample_rows()

    def arm_c():
        host.sample_with_cond(model, hi, None, 1, seeds=seeds[half:])
        r = _lib.internal_sample_rows()
        host.sample_with_cond(model, lo, None, 4, seeds=seeds[:half])
        rows["c"] = r + _lib.internal_sample_rows()

    arms = [("a", "uniform 32 x T=4", arm_a), ("b", "mixed 16 x T=4 + 16 x T=1, one call", arm_b),
            ("c", "two uniform calls: 16 x T=1, then 16 x T=4", arm_c)]
    for _ in range(a.warmup):          # every shape of the timed window
        for _, _, fn in arms:
            fn()
    host.synchronize()
    ms = {k: [] for k, _, _ in arms}
    for _ in range(a.calls):
        for k, _, fn in arms:          # alternated: drift of the machine lands on every arm alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    host.synchronize()
    lines = [f"| arm | what | utterance-evaluations | median ms | min ms | max ms |", "|---|---|---|---|---|---|"]
    for k, what, _ in arms:
        v = np.asarray(ms[k])
        lines.append(f"| ({k}) | {what} | {rows[k]} | {np.median(v):.3f} | {v.min():.3f} | {v.max():.3f} |")
    head = f"B = {B}, T = {T}, LJSpeech config, fp32 default form, seeded noise, {a.calls} timed calls per arm after {a.warmup} warm-up rounds, device events"
    print(head)
    print("\n".join(lines))
    if a.md:
        with open(a.md, "a") as f:
            f.write(head + "\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
