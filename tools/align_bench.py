#!/usr/bin/env python3
"""Cost of the alignment kernels (csrc/align.hip) per call at B = 1, 8, 32 pairs of 512 x 512 frames and of 300 x 600 (rendering x recording).
One process, device events, median over --reps windows of --calls calls each, on preallocated buffers:

  cost       cmtts_align_cost: the two means launches' worth of work and the difference-form cost matrix
  dp         cmtts_align_dtw: the DP, the walk back and row[] in one launch, one workgroup per pair
  durations  cmtts_align_durations
  hosted     host.dtw_align: the three calls behind the host layer (checks, allocations, the tables' upload)

The input is a noisy stretch of N(0, 1) features, so the path wanders as it does on speech; the result is checked against the numpy
definition on the first pair before anything is timed.  Also prints the DP's time per anti-diagonal step.  One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, align as A  # noqa: E402
from cmtts_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512,300x600")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda v: C.c_void_p(v.ctypes.data)
    L = 64

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls                   # milliseconds per call

    for shape in a.shapes.split(","):
        Ts, Tr = (int(v) for v in shape.split("x"))
        for B in (int(v) for v in a.batches.split(",")):
            rs = np.random.RandomState(B)
            x = rs.standard_normal((B, Ts, 80)).astype(np.float32)
            y = (x[:, (np.arange(Tr) * Ts) // Tr] + 0.3 * rs.standard_normal((B, Tr, 80))).astype(np.float32)
            d = np.zeros((B, L), np.int32)
            for b in range(B):
                d[b] = np.diff(np.concatenate([[0], np.sort(rs.randint(0, Ts + 1, size=L - 1)), [Ts]]))
            xl, yl = np.full(B, Ts, np.int32), np.full(B, Tr, np.int32)
            xd, yd, dd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(d).to(dev)
            cost = torch.empty(B, Ts, Tr, device=dev)
            row = torch.empty(B, Tr, dtype=torch.int32, device=dev)
            total, n = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
            d_rec, pc = torch.empty(B, L, dtype=torch.int32, device=dev), torch.empty(B, L, device=dev)
            nb = lib.cmtts_align_workspace_bytes(B, Ts, Tr)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def k_cost():
                assert lib.cmtts_align_cost(p(xd), hp(xl), Ts, p(yd), hp(yl), Tr, B, 80, 1, p(cost), p(ws), nb, st()) == 0

            def k_dp():
                assert lib.cmtts_align_dtw(p(cost), hp(xl), hp(yl), B, Ts, Tr, p(row), p(total), p(n), p(ws), nb, st()) == 0

            def k_dur():
                assert lib.cmtts_align_durations(p(row), p(cost), p(dd), hp(d), hp(xl), hp(yl), B, Ts, Tr, L, p(d_rec), p(pc), p(ws), nb, st()) == 0

            def hosted():
                return host.dtw_align(xd, xl, d, yd, yl)

            k_cost(), k_dp(), k_dur()
            torch.cuda.synchronize()
            c0 = cost[0].cpu().numpy()
            t_ref, n_ref, row_ref = A.dtw(c0)
            d_ref, _ = A.durations(row_ref, c0, d[0])
            assert np.array_equal(row[0].cpu().numpy(), row_ref) and int(n[0]) == n_ref and d_rec[0].cpu().tolist() == d_ref.tolist()
            assert hosted()["d_targets"][0].cpu().tolist() == d_ref.tolist()
            arms = {"cost": k_cost, "dp": k_dp, "durations": k_dur, "hosted": hosted}
            for fn in arms.values():
                timed(fn)
            ms = {k: [] for k in arms}
            for _ in range(a.reps):
                for k, fn in arms.items():
                    ms[k].append(timed(fn))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            print(json.dumps({"Ts": Ts, "Tr": Tr, "B": B, **{k + "_ms": round(v, 4) for k, v in med.items()},
                              "dp_ms_spread": [round(min(ms["dp"]), 4), round(max(ms["dp"]), 4)],
                              "cost_ms_spread": [round(min(ms["cost"]), 4), round(max(ms["cost"]), 4)],
                              "dp_ns_per_antidiagonal": round(med["dp"] * 1e6 / (Ts + Tr - 1), 1), "path_len_pair0": n_ref,
                              "cost_bytes": B * (Ts * Tr + (Ts + Tr) * 80) * 4}), flush=True)


if __name__ == "__main__":
    main()
