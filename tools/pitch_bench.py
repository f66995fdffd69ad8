#!/usr/bin/env python3
"""Cost of the pitch kernels (csrc/pitch.hip) per call at B = 1, 8, 32 rows of 512 frames (and of 4096).  One process, device events, median
over --reps windows of --calls calls each, on preallocated buffers:

  nacf       cmtts_pitch_nacf: framing, mean, window and the 277-lag autocorrelation in the direct form, one launch
  track      cmtts_pitch_track: the candidates launch and the Viterbi launch (one wave per row)
  targets    cmtts_pitch_targets: fill, log, mean / std and the 10-scale CWT in the direct circular form, one launch
  hosted     host.pitch_targets(check=False): the four launches behind the host layer (checks, allocations)
  torch_fft  the same autocorrelation composed from torch on the same card: unfold, mean, window, rfft(2048), |X|^2, irfft, normalise

The input is a five-harmonic glide with a noise burst and a silence per row; the results are checked against the numpy definition on the first
row before anything is timed.  A report, not a pass mark.  One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, pitch as P  # noqa: E402
from cmtts_amd import host  # noqa: E402


def make_rows(B, T, g):
    n = (T - 1) * g.hop + g.hop // 2
    rng = np.random.default_rng(B * 10007 + T)
    wav = np.zeros((B, n), np.float32)
    t = np.arange(n)
    for b in range(B):
        f = 150.0 + (20.0 * b) % 140.0 + 50.0 * np.sin(2 * np.pi * t / n * (1.0 + 0.1 * b))
        ph = 2.0 * np.pi * np.cumsum(f) / g.fs
        x = 0.2 * sum(np.sin(k * ph) / k for k in range(1, 6))
        a = n // 3
        x[a:a + n // 10] = 0.02 * rng.standard_normal(n // 10)
        x[-n // 12:] = 0.0
        wav[b] = x + 1e-3 * rng.standard_normal(n)
    return wav


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="512,4096")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pitch_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    lib = _lib.load()
    pt = host.get_pitch_tracker(device=dev)
    g = pt.geometry
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L2 = g.LMAX + 2
    win_t = torch.from_numpy(g.window.astype(np.float32)).to(dev)
    rw_t = torch.from_numpy(g.r_w.astype(np.float32)).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls                   # milliseconds per call

    for T in (int(v) for v in a.frames.split(",")):
        for B in (int(v) for v in a.batches.split(",")):
            wav_h = make_rows(B, T, g)
            n = wav_h.shape[1]
            wav = torch.from_numpy(wav_h).to(dev)
            n_valid = torch.full((B,), n, dtype=torch.int32, device=dev)
            r = torch.empty(B, T, L2, device=dev)
            pk = torch.empty(B, T, device=dev)
            frames = torch.empty(B, dtype=torch.int32, device=dev)
            lag = torch.empty(B, T, dtype=torch.int32, device=dev)
            f0 = torch.empty(B, T, device=dev)
            cwt = torch.empty(B, T, 10, device=dev)
            mean, std = torch.empty(B, device=dev), torch.empty(B, device=dev)
            uv = torch.empty(B, T, dtype=torch.uint8, device=dev)
            status = torch.empty(B, dtype=torch.int32, device=dev)
            nb = lib.cmtts_pitch_workspace_bytes(B, T)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            padded = torch.nn.functional.pad(wav, (g.W // 2, g.W // 2 + g.hop))

            def k_nacf():
                assert lib.cmtts_pitch_nacf(pt._h, p(wav), 0, B, n, p(n_valid), T, p(r), p(pk), p(frames), p(ws), nb, st()) == 0

            def k_track():
                assert lib.cmtts_pitch_track(pt._h, p(r), p(pk), p(frames), B, T, p(lag), p(f0), p(ws), nb, st()) == 0

            def k_targets():
                assert lib.cmtts_pitch_targets(pt._h, p(f0), p(frames), B, T, p(cwt), p(mean), p(std), p(uv), p(status), p(ws), nb, st()) == 0

            def hosted():
                return host.pitch_targets(pt, wav, check=False)

            def torch_fft():
                fr = padded.unfold(1, g.W, g.hop)[:, :T]
                fr = (fr - fr.mean(-1, keepdim=True)) * win_t
                spec = torch.fft.rfft(fr, n=2048)
                ac = torch.fft.irfft(spec.real ** 2 + spec.imag ** 2, n=2048)[..., :L2]
                return ac / ac[..., :1] / rw_t

            k_nacf(), k_track(), k_targets()
            torch.cuda.synchronize()
            r64, pk64 = P.nacf(wav_h[0])
            err = float(np.abs(r[0].cpu().numpy() - r64).max())
            err_fft = float(np.abs(torch_fft()[0].cpu().numpy() - r64).max())
            want_lag, _ = P.track(r[0].cpu().numpy(), pk[0].cpu().numpy())
            assert np.array_equal(lag[0].cpu().numpy(), want_lag) and int(status[0]) == 0
            want = P.targets(f0[0].cpu().numpy())
            err_cwt = float(np.abs(cwt[0].cpu().numpy() - want["cwt_spec"]).max() / np.abs(want["cwt_spec"]).max())
            arms = {"nacf": k_nacf, "track": k_track, "targets": k_targets, "hosted": hosted, "torch_fft": torch_fft}
            for fn in arms.values():
                timed(fn)
            ms = {k: [] for k in arms}
            for _ in range(a.reps):
                for k, fn in arms.items():
                    ms[k].append(timed(fn))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            print(json.dumps({"T": T, "B": B, **{k + "_ms": round(v, 4) for k, v in med.items()},
                              **{k + "_ms_spread": [round(min(v), 4), round(max(v), 4)] for k, v in ms.items() if k in ("nacf", "track", "targets")},
                              "viterbi_ns_per_frame": round(med["track"] * 1e6 / T, 1), "voiced_row0": round(float((want_lag > 0).mean()), 3),
                              "r_err_row0": err, "r_err_torch_fft_row0": err_fft, "cwt_err_row0": err_cwt,
                              "nacf_gflop": round(2.0 * B * T * L2 * g.W / 1e9, 3)}), flush=True)


if __name__ == "__main__":
    main()
