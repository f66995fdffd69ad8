"""Times of the GE2E speaker encoder on the device (profiles/ge2e.md): the front end, the three LSTM layers (projection GEMM + recurrence) and
the tail at 1, 32 and 256 windows of 160 frames, next to the same network as torch.nn.LSTM +
Linear on the same device.  Records, not pass marks.

    python tools/ge2e_bench.py [--iters 20] [--out ge2e_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, host  # noqa: E402
from cmtts_amd.weights import synth_ge2e_state_dict  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters, warmup=3):
    """Median milliseconds of fn() between two events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sd = synth_ge2e_state_dict(0)
    enc = host.get_ge2e_encoder(sd, DEV)
    lstm = torch.nn.LSTM(40, 256, 3, batch_first=True)
    lstm.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("lstm.")})
    lin = torch.nn.Linear(256, 256)
    lin.load_state_dict({"weight": torch.from_numpy(sd["linear.weight"]), "bias": torch.from_numpy(sd["linear.bias"])})
    lstm, lin = lstm.to(DEV).eval(), lin.to(DEV).eval()
    rs = np.random.RandomState(0)
    rows = []
    for W in (1, 32, 256):
        win = torch.from_numpy(np.abs(rs.standard_normal((W, 160, 40))).astype(np.float32)).to(DEV)
        # W windows of one clip: 80 frames apart, so (W - 1) * 17600 + 35200 samples
        wav = torch.from_numpy((rs.standard_normal((1, (W - 1) * 17600 + 35200)) * 0.1).astype(np.float32)).to(DEV)
        rec = {"windows": W}
        rec["features_ms"] = timed(lambda: host.ge2e_features(enc, wav), args.iters)          # includes the read-back of info
        hl = torch.zeros(W, 256, device=DEV)
        lt, lb = torch.from_numpy(np.ascontiguousarray(sd["linear.weight"].T)).to(DEV), torch.from_numpy(sd["linear.bias"]).to(DEV)
        ew, em = torch.empty(W, 256, device=DEV), torch.empty(1, 256, device=DEV)
        rm = torch.zeros(W, dtype=torch.int32, device=DEV)
        st = host._stream
        rec["tail_ms"] = timed(lambda: _lib.internal_ge2e_tail(hl.data_ptr(), W, lt.data_ptr(), lb.data_ptr(), ew.data_ptr(), rm.data_ptr(), 1,
                                                               em.data_ptr(), st()), args.iters)
        rec["forward_ms"] = timed(lambda: host.ge2e_forward(enc, win, np.zeros(W, np.int32), 1), args.iters)
        with torch.no_grad():
            def ref():
                _, (h, _) = lstm(win)
                y = torch.relu(lin(h[-1]))
                return y / (torch.norm(y, dim=1, keepdim=True) + 1e-5)
            rec["torch_lstm_ms"] = timed(ref, args.iters)
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
