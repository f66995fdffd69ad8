#!/usr/bin/env python3
"""Cost of the loudness measurement (cmtts_loudness_measure, csrc/loudness.hip) next to the generator it follows.  One process, device
events, median and spread over --reps windows of --calls calls each, the two alternating:

  generator    cmtts_vocoder_forward (fp32 HiFi-GAN) at B = --batch, T = --frames: unchanged code, the yardstick
  loudness     the two launches of cmtts_loudness_measure on that call's waveform [B, T * 256], every row fully valid, with targets

Prints one JSON line: both times in microseconds and their ratio."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, host  # noqa: E402
from cmtts_amd.config import HifiGanConfig  # noqa: E402
from cmtts_amd.weights import synth_hifigan_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loudness_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    lib = _lib.load()
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, dev).load_state_dict(synth_hifigan_state_dict(hcfg, seed=0))
    B, T = a.batch, a.frames
    mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(0)) * 0.8 - 1.0).to(dev)
    wav = voc(mel).squeeze(1)
    n = wav.shape[1]
    fs = 22050
    n_valid = torch.full((B,), n, dtype=torch.int32, device=dev)
    target = torch.full((B,), -23.0, device=dev)
    stats = torch.empty(B, 4, device=dev)
    nb = lib.cmtts_loudness_workspace_bytes(B, n, fs)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def generator():
        voc(mel)

    def loudness():
        _lib.check(lib.cmtts_loudness_measure(wav.data_ptr(), B, n, n_valid.data_ptr(), fs, target.data_ptr(), -1.0, stats.data_ptr(),
                                              ws.data_ptr(), nb, stream))

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.calls          # microseconds per call

    fns = {"generator": generator, "loudness": loudness}
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, fn in fns.items():
            times[k].append(window(fn))
    host.check_async_error()
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {"tool": "loudness_bench", "B": B, "T": T, "samples": n, "calls": a.calls, "reps": a.reps,
           "generator_us": {"median": round(med["generator"], 1), "min": round(min(times["generator"]), 1), "max": round(max(times["generator"]), 1)},
           "loudness_us": {"median": round(med["loudness"], 1), "min": round(min(times["loudness"]), 1), "max": round(max(times["loudness"]), 1)},
           "ratio": round(med["loudness"] / med["generator"], 5),
           "lufs_first_row": round(float(stats[0, 0]), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
