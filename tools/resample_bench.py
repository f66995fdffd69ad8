#!/usr/bin/env python3
"""Resampled / G.711 output (host.vocoder_infer_stream and host.vocoder_infer with sample_rate / encoding) against the native int16
stream of the same process: time to the first chunk, time to the last chunk and the one-shot time, for configs[1]'s vocoder batch
(32 x 512 frames) and one 510-frame utterance, fp32 and bf16, native s16 / 8 kHz mu-law / 48 kHz s16.  Wall clock from the call to the
host-visible samples (medians of --reps runs after a warm-up).  Prints one JSON line per (case, precision, format); the native line
is the baseline (the path a build without the resampler runs, unchanged)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import host  # noqa: E402
from cmtts_amd.config import HifiGanConfig  # noqa: E402
from cmtts_amd.weights import synth_hifigan_state_dict  # noqa: E402

FORMATS = {"native_s16": {}, "8k_mulaw": {"sample_rate": 8000, "encoding": "mulaw"}, "48k_s16": {"sample_rate": 48000, "encoding": "s16"}}


def one(voc, mel, lens, chunks, fmt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = None
    n = nbytes = 0
    for _, _, chunk, _ in host.vocoder_infer_stream(mel, voc, lens, chunks, **fmt):
        if first is None:
            first = time.perf_counter() - t0
        n += 1
        nbytes += chunk.nbytes
    return first, time.perf_counter() - t0, n, nbytes


def oneshot(voc, mel, lens, fmt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host.vocoder_infer(mel, voc, lengths=[n * 256 for n in lens], **fmt)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--chunks", default="32,64,128,256")
    a = ap.parse_args()
    chunks = tuple(int(c) for c in a.chunks.split(","))
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, "cuda:0").load_state_dict(synth_hifigan_state_dict(hcfg, seed=0))
    g = torch.Generator().manual_seed(0)
    cases = {"configs1_32x512": (torch.randn(32, 80, 512, generator=g) * 1.5 - 4, [512] * 32),
             "single_510": (torch.randn(1, 80, 510, generator=g) * 1.5 - 4, [510])}
    for prec in a.precisions.split(","):
        voc.set_precision(prec)
        for name, (mel, lens) in cases.items():
            mel = mel.cuda()
            for fname, fmt in FORMATS.items():
                one(voc, mel, lens, chunks, fmt)
                oneshot(voc, mel, lens, fmt)
                runs = [one(voc, mel, lens, chunks, fmt) for _ in range(a.reps)]
                shots = [oneshot(voc, mel, lens, fmt) for _ in range(a.reps)]
                print(json.dumps({"case": name, "precision": prec, "format": fname, "chunk_frames": list(chunks), "chunks": runs[0][2],
                                  "d2h_bytes": runs[0][3],
                                  "first_chunk_ms": round(1e3 * statistics.median(r[0] for r in runs), 3),
                                  "last_chunk_ms": round(1e3 * statistics.median(r[1] for r in runs), 3),
                                  "oneshot_vocoder_infer_ms": round(1e3 * statistics.median(shots), 3)}), flush=True)


if __name__ == "__main__":
    main()
