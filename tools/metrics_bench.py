#!/usr/bin/env python3
"""Cost of the metric kernels (csrc/metrics.hip) per call at B = 1, 8, 32 pairs of 512 x 512 frames and of 300 x 600 (rendering x recording),
next to the same composed from torch ops on the device.  One process, device events, median over --reps windows of --calls calls each,
on preallocated buffers, the arms alternating inside every repetition:

  cepstra    cmtts_metric_cepstra, both sides (n_cep = 20)          torch: two matmuls with the DCT table
  cost       cmtts_metric_cost, coefficients 1 .. 13                torch: torch.cdist on the cepstra
  dtw        cmtts_align_dtw on that cost (unchanged code)          —
  f0         cmtts_metric_f0 with the DTW's row                     —
  prepare    cmtts_metric_ssim_prepare (C = 20)                     torch: gather, norm over the frames, divide
  ssim       cmtts_metric_ssim                                      torch: F.conv2d with the 11 x 11 window over the five maps, fp64
  scored     host.score_pairs: all of it behind the host layer (checks, allocations, the lengths' upload)

The torch arms take full-length pairs (no raggedness) and are checked against the kernels' results before anything is timed.  One JSON line
per shape."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, metrics as M  # noqa: E402
from cmtts_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512,300x600")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda v: C.c_void_p(v.ctypes.data)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    NC, K_LO, K_HI, CI = 20, 1, 13, 20
    tab = torch.from_numpy(M.dct_table(80, NC)).to(dev)
    g = torch.from_numpy(M.gaussian_window()).to(dev)
    win = (g[:, None] * g[None, :])[None, None].expand(5, 1, 11, 11).contiguous()      # fp64, one window per moment map

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
            lo, hi = float(np.log(1e-5)), 2.0
            x = (lo + (hi - lo) * rs.rand(B, Ts, 80)).astype(np.float32)
            y = np.clip(x[:, (np.arange(Tr) * Ts) // Tr] + 0.05 * (hi - lo) * rs.standard_normal((B, Tr, 80)), lo, hi).astype(np.float32)
            fx = (80.0 + 320.0 * rs.rand(B, Ts)).astype(np.float32)
            fx[rs.rand(B, Ts) < 0.25] = 0.0
            fy = (fx[:, (np.arange(Tr) * Ts) // Tr] * (1.0 + 0.1 * rs.standard_normal((B, Tr)))).astype(np.float32)
            xl, yl = np.full(B, Ts, np.int32), np.full(B, Tr, np.int32)
            xd, yd, fxd, fyd = (torch.from_numpy(v).to(dev) for v in (x, y, fx, fy))
            xld, yld = torch.from_numpy(xl).to(dev), torch.from_numpy(yl).to(dev)
            cx, cy = torch.empty(B, Ts, NC, device=dev), torch.empty(B, Tr, NC, device=dev)
            cost = torch.empty(B, Ts, Tr, device=dev)
            row = torch.empty(B, Tr, dtype=torch.int32, device=dev)
            total, n = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
            counts, vals = torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, 3, device=dev)
            u, v, mm = torch.empty(B, Tr, CI, device=dev), torch.empty(B, Tr, CI, device=dev), torch.empty(B, 2, device=dev)
            rng, ssim = torch.ones(1, device=dev), torch.empty(B, device=dev)
            nb = lib.cmtts_align_workspace_bytes(B, Ts, Tr)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            nbm = lib.cmtts_metric_workspace_bytes(B, Tr, CI)
            wsm = torch.empty(nbm, dtype=torch.uint8, device=dev)

            def k_cep():
                assert lib.cmtts_metric_cepstra(p(xd), p(xld), p(tab), B, Ts, 80, NC, p(cx), st()) == 0
                assert lib.cmtts_metric_cepstra(p(yd), p(yld), p(tab), B, Tr, 80, NC, p(cy), st()) == 0

            def k_cost():
                assert lib.cmtts_metric_cost(p(cx), p(xld), Ts, p(cy), p(yld), Tr, B, NC, K_LO, K_HI, p(cost), st()) == 0

            def k_dtw():
                assert lib.cmtts_align_dtw(p(cost), hp(xl), hp(yl), B, Ts, Tr, p(row), p(total), p(n), p(ws), nb, st()) == 0

            def k_f0():
                assert lib.cmtts_metric_f0(p(fxd), p(xld), Ts, p(fyd), p(yld), Tr, p(row), B, p(counts), p(vals), st()) == 0

            def k_prep():
                assert lib.cmtts_metric_ssim_prepare(p(cx), p(xld), Ts, p(cy), p(yld), Tr, p(row), B, NC, CI, p(u), p(v), p(mm), st()) == 0

            def k_ssim():
                assert lib.cmtts_metric_ssim(p(u), p(v), p(yld), B, Tr, CI, p(rng), p(ssim), p(wsm), nbm, st()) == 0

            def scored():
                return host.score_pairs(xd, xl, yd, yl, f0_syn=fxd, f0_rec=fyd)

            def t_cep():
                return torch.matmul(xd, tab), torch.matmul(yd, tab)

            def t_cost():
                return torch.cdist(cx[:, :, K_LO:K_HI + 1], cy[:, :, K_LO:K_HI + 1])

            def t_prep():
                a_ = torch.gather(cx[:, :, :CI], 1, row.long()[:, :, None].expand(B, Tr, CI))
                b_ = cy[:, :, :CI]
                return a_ / a_.double().norm(dim=1, keepdim=True).float(), b_ / b_.double().norm(dim=1, keepdim=True).float()

            def t_ssim():
                a_, b_ = u.double(), v.double()
                maps = torch.stack([a_, b_, a_ * a_, b_ * b_, a_ * b_], dim=1)                      # [B, 5, Tr, C]
                m = F.conv2d(maps, win, groups=5)
                L = rng.double()
                c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
                mxy, mxx, myy = m[:, 0] * m[:, 1], m[:, 0] ** 2, m[:, 1] ** 2
                idx = (2 * mxy + c1) * (2 * (m[:, 4] - mxy) + c2) / ((mxx + myy + c1) * ((m[:, 2] - mxx) + (m[:, 3] - myy) + c2))
                return idx.mean(dim=(1, 2)).float()

            k_cep(), k_cost(), k_dtw(), k_f0(), k_prep()
            rng.copy_((mm[:, 1].max() - mm[:, 0].min()).reshape(1))
            k_ssim()
            torch.cuda.synchronize()
            # the torch arms compute the same things, and the kernels the definition (pair 0)
            tcx, tcy = t_cep()
            assert float((tcx - cx).abs().max()) <= 1e-3 and float((tcy - cy).abs().max()) <= 1e-3
            assert float((t_cost() - cost).abs().max()) <= 1e-3 * float(cost.max())
            tu, tv = t_prep()
            assert float((tu - u).abs().max()) <= 1e-6 and float((tv - v).abs().max()) <= 1e-6
            assert float((t_ssim() - ssim).abs().max()) <= 1e-6
            ref = M.score(x[0], Ts, y[0], Tr, f0_syn=fx[0], f0_rec=fy[0], data_range=float(rng[0]), cepstra_syn=cx[0].cpu().numpy(),
                          cepstra_rec=cy[0].cpu().numpy(), cost_matrix=cost[0].cpu().numpy())
            out = scored()
            assert np.array_equal(out["row"][0].cpu().numpy(), ref["row"]) and float(out["mcd"][0]) == float(ref["mcd"])
            assert counts[0].cpu().tolist() == [ref["n"], ref["n_vv"], ref["n_gpe"], ref["n_vde"]]
            assert abs(float(ssim[0]) - float(ref["ssim"])) <= 1e-6
            arms = {"cepstra": k_cep, "cepstra_torch": t_cep, "cost": k_cost, "cost_torch": t_cost, "dtw": k_dtw, "f0": k_f0, "prepare": k_prep,
                    "prepare_torch": t_prep, "ssim": k_ssim, "ssim_torch": t_ssim, "scored": scored}
            for fn in arms.values():
                timed(fn)
            ms = {k: [] for k in arms}
            for _ in range(a.reps):
                for k, fn in arms.items():
                    ms[k].append(timed(fn))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            print(json.dumps({"Ts": Ts, "Tr": Tr, "B": B, **{k + "_ms": round(v, 4) for k, v in med.items()},
                              **{k + "_ms_spread": [round(min(ms[k]), 4), round(max(ms[k]), 4)] for k in ("cost", "cost_torch", "ssim", "ssim_torch", "scored")},
                              "mcd_pair0": round(float(ref["mcd"]), 4), "ssim_pair0": round(float(ref["ssim"]), 6), "ffe_pair0": round(float(ref["ffe"]), 4),
                              "cost_bytes": B * (Ts * Tr + (Ts + Tr) * (K_HI - K_LO + 1)) * 4}), flush=True)


if __name__ == "__main__":
    main()
