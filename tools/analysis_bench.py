#!/usr/bin/env python3
"""Cost of the recorded-speech analysis (csrc/mel_analysis.hip) at --rows rows of --frames frames (default 32 x 512).  One process, device
events, median over --reps windows of --calls calls each, the arms alternating:

  kernel   cmtts_mel_analysis on preallocated buffers: STFT + mel + energy in one launch (pad "reference", layout [B,T,80])
  hosted   host.mel_from_audio: the same launch behind the host layer (length check, output allocations, the lengths' upload)
  torch    YARDSTICK ONLY, outside the product path: the same computation composed on the same card from torch.stft (center, reflect, periodic
           Hann) + abs + a matmul with the dense filterbank + clamp + log + the energy norm

Also prints the kernel's bytes moved and its share of what the HBM could do in that time, and max |kernel - torch| on the log-mel (the two
agree to float32 rounding).  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import analysis as A  # noqa: E402
from cmtts_amd import host  # noqa: E402

HBM_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("analysis_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    an = host.get_analyzer(device=dev)
    n = (a.frames - 1) * A.HOP + 17                            # 1 + n // 256 = --frames
    rs = np.random.RandomState(0)
    t = np.arange(n) / 22050.0
    wav = torch.from_numpy((0.3 * np.sin(2 * np.pi * 200.0 * t)[None] + 0.05 * rs.standard_normal((a.rows, n))).astype(np.float32)).to(dev)
    basis = torch.from_numpy(A.mel_basis()).to(dev)
    window = torch.from_numpy(A.hann_window(np.float32)).to(dev)

    lib = an.lib
    n_valid = torch.full((a.rows,), n, dtype=torch.int32, device=dev)
    out = {"mel": torch.empty(a.rows, a.frames, A.N_MELS, device=dev), "energy": torch.empty(a.rows, a.frames, device=dev)}
    frames = torch.empty(a.rows, dtype=torch.int32, device=dev)
    nb = lib.cmtts_analysis_workspace_bytes(a.rows, a.frames)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def kernel():
        rc = lib.cmtts_mel_analysis(an._h, p(wav), 0, a.rows, n, p(n_valid), 0, a.frames, 0, p(out["mel"]), p(out["energy"]), p(frames), p(ws), nb,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        return out

    def hosted():
        return host.mel_from_audio(an, wav)

    def composed():
        spec = torch.stft(wav, A.N_FFT, hop_length=A.HOP, win_length=A.N_FFT, window=window, center=True, pad_mode="reflect", return_complex=True)
        mag = spec.abs()                                       # [B, 513, T]
        mel = torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5)).transpose(1, 2)
        return {"mel": mel, "energy": torch.linalg.vector_norm(mag, dim=1)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls                   # milliseconds per call

    k, c = kernel(), composed()
    assert torch.equal(hosted()["mel"], k["mel"])
    assert k["mel"].shape == c["mel"].shape == (a.rows, a.frames, A.N_MELS)
    diff = float((k["mel"] - c["mel"]).abs().max())
    for fn in (kernel, composed, hosted):                      # warm every arm
        timed(fn)
    tk, tc, th = [], [], []
    for _ in range(a.reps):
        tk.append(timed(kernel))
        tc.append(timed(composed))
        th.append(timed(hosted))
    ms_k, ms_c = float(np.median(tk)), float(np.median(tc))
    moved = a.rows * (n * 4 + a.frames * (A.N_MELS + 1) * 4)   # samples in once, mel and energy out
    print(json.dumps({"rows": a.rows, "frames": a.frames, "samples_per_row": n, "kernel_ms": round(ms_k, 4), "torch_ms": round(ms_c, 4),
                      "kernel_ms_spread": [round(min(tk), 4), round(max(tk), 4)], "torch_ms_spread": [round(min(tc), 4), round(max(tc), 4)],
                      "torch_over_kernel": round(ms_c / ms_k, 3), "kernel_bytes": moved,
                      "kernel_share_of_hbm": round(moved / (ms_k * 1e-3) / (HBM_TBS * 1e12), 5), "max_abs_mel_diff": diff,
                      "host_mel_from_audio_ms": round(float(np.median(th)), 4)}))


if __name__ == "__main__":
    main()
