#!/usr/bin/env python3
"""Cost of the speaker encoder (csrc/speaker_encoder.hip) at W = 1, 8, 32 windows.  One process, device events, median over --reps
windows of --calls calls each, the arms alternating:

  features     cmtts_spkenc_features on W rows of --seconds of audio (trim + fbank, centre window: W windows)
  network      cmtts_spkenc_forward on those W windows (28 Conv2D launches + the tail), with the issued TFLOP/s against the 157.3 TF
               fp32 matrix peak (2 x 16-padded K x output pixels x output channels per conv: what the MFMAs execute)
  stage 1..4   the seven Conv2D launches of each stage through the kernel-alone hook
  torch        YARDSTICK ONLY, outside the product path: the same net (BatchNorm folded) as torch-ROCm F.conv2d / clamp on the same card,
               whole and per stage

Prints one JSON line per W."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, host  # noqa: E402
from cmtts_amd import speaker as sp  # noqa: E402
from cmtts_amd.weights import synth_deepspeaker_state_dict  # noqa: E402

PEAK_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("speaker_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    sd = synth_deepspeaker_state_dict(0)
    enc = host.get_speaker_encoder(sd, dev)
    stream = torch.cuda.current_stream().cuda_stream
    layers = sp.layer_names()
    packed, folded = [], []
    for name, k, s, cin, cout in layers:
        bn = np.stack([sd[name + "_bn/" + p] for p in ("gamma", "beta", "moving_mean", "moving_variance")])
        frag, bias = _lib.internal_spkenc_pack(sd[name + "/kernel"], sd[name + "/bias"], bn)
        packed.append((torch.from_numpy(frag).to(dev), torch.from_numpy(bias).to(dev)))
        k64, b64 = sp.fold_bn(sd, name)
        folded.append((torch.from_numpy(k64.astype(np.float32)).permute(3, 2, 0, 1).contiguous().to(dev), torch.from_numpy(b64.astype(np.float32)).to(dev)))
    dense, dense_b = torch.from_numpy(sd["affine/kernel"]).to(dev), torch.from_numpy(sd["affine/bias"]).to(dev)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls          # milliseconds per call

    rs = np.random.RandomState(0)
    n = int(a.seconds * 22050)
    for W in a.windows:
        t = np.arange(n) / 22050.0
        wav = torch.from_numpy((0.3 * np.sin(2 * np.pi * 200.0 * t)[None] * (1 + 0.5 * np.sin(2 * np.pi * 3.0 * t))[None]
                                + 0.05 * rs.standard_normal((W, n))).astype(np.float32)).to(dev)
        win, info = host.speaker_features(enc, wav)
        assert win.shape[0] == W
        row_map = torch.arange(W, dtype=torch.int32, device=dev)
        # geometry and issued flops per stage
        flops, shapes, H, Wd = [0.0] * 4, [], 160, 64
        for i, (name, k, s, cin, cout) in enumerate(layers):
            Ho, Wo = -(-H // s), -(-Wd // s)
            shapes.append((H, Wd))
            flops[i // 7] += 2.0 * (-(-k * k * cin // 16) * 16) * W * Ho * Wo * cout
            H, Wd = Ho, Wo
        bufs = [torch.empty(W * 80 * 32 * 64, device=dev) for _ in range(2)]

        def ours_stage(st, x):
            i = 7 * st
            (name, k, s, cin, cout), (Hi, Wi) = layers[i], shapes[i]
            cur = 0
            _lib.check(_lib.internal_spkenc_conv(x.data_ptr(), packed[i][0].data_ptr(), packed[i][1].data_ptr(), None, W, Hi, Wi, cin, cout, k, s,
                                                 bufs[cur].data_ptr(), stream))
            Hi, Wi = shapes[i + 1]
            for b in range(3):
                pa, pb = packed[i + 1 + 2 * b], packed[i + 2 + 2 * b]
                _lib.check(_lib.internal_spkenc_conv(bufs[cur].data_ptr(), pa[0].data_ptr(), pa[1].data_ptr(), None, W, Hi, Wi, cout, cout, 3, 1,
                                                     bufs[cur ^ 1].data_ptr(), stream))
                _lib.check(_lib.internal_spkenc_conv(bufs[cur ^ 1].data_ptr(), pb[0].data_ptr(), pb[1].data_ptr(), bufs[cur].data_ptr(), W, Hi, Wi, cout,
                                                     cout, 3, 1, bufs[cur].data_ptr(), stream))
            return bufs[cur][:W * Hi * Wi * cout]

        def torch_stage(st, x):
            i = 7 * st
            k, b = folded[i]
            pt, pb_, _ = sp.same_pad(x.shape[2], 5, 2)
            pl, pr, _ = sp.same_pad(x.shape[3], 5, 2)
            x = F.conv2d(F.pad(x, (pl, pr, pt, pb_)), k, b, stride=2).clamp_(0, 20)
            for j in range(3):
                (ka, ba), (kb, bb) = folded[i + 1 + 2 * j], folded[i + 2 + 2 * j]
                t_ = F.conv2d(x, ka, ba, padding=1).clamp_(0, 20)
                x = (F.conv2d(t_, kb, bb, padding=1).clamp_(0, 20) + x).clamp_(0, 20)
            return x

        def torch_net():
            x = win[:, None]
            for st in range(4):
                x = torch_stage(st, x)
            v = x.permute(0, 2, 3, 1).reshape(W, 10, 2048).mean(1)
            return F.normalize(v @ dense + dense_b, dim=1, eps=1e-6)

        stage_in = [win]
        tin = [win[:, None]]
        for st in range(3):
            stage_in.append(ours_stage(st, stage_in[-1]).clone())
            tin.append(torch_stage(st, tin[-1]))
        emb = host.speaker_forward(enc, win, row_map, W)
        agree = float((emb - torch_net()).abs().max())
        fns = {"features": lambda: host.speaker_features(enc, wav), "network": lambda: host.speaker_forward(enc, win, row_map, W), "torch": torch_net}
        for st in range(4):
            fns[f"stage{st + 1}"] = (lambda st=st: ours_stage(st, stage_in[st]))
            fns[f"torch_stage{st + 1}"] = (lambda st=st: torch_stage(st, tin[st]))
        times = {k: [] for k in fns}
        for fn in fns.values():
            fn()
        for _ in range(a.reps):
            for k, fn in fns.items():
                times[k].append(window(fn))
        host.check_async_error()
        med = {k: float(np.median(v)) for k, v in times.items()}
        out = {"tool": "speaker_bench", "W": W, "samples_per_row": n, "calls": a.calls, "reps": a.reps,
               "features_ms": round(med["features"], 3), "network_ms": round(med["network"], 3), "torch_ms": round(med["torch"], 3),
               "issued_gflop": round(sum(flops) / 1e9, 2), "issued_tflops": round(sum(flops) / med["network"] / 1e9, 2),
               "of_peak": round(sum(flops) / med["network"] / 1e9 / PEAK_TF, 3),
               "stage_ms": [round(med[f"stage{s + 1}"], 3) for s in range(4)],
               "stage_tflops": [round(flops[s] / med[f"stage{s + 1}"] / 1e9, 2) for s in range(4)],
               "torch_stage_ms": [round(med[f"torch_stage{s + 1}"], 3) for s in range(4)],
               "network_vs_torch": round(med["network"] / med["torch"], 2), "max_abs_diff_vs_torch": agree}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
