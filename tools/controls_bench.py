#!/usr/bin/env python3
"""Cost of the prosody controls on the text side and the frame side at the BASELINE.json configs[1] shapes (B = 32, L = 85 phonemes ->
T = 512 frames): cmtts_text_forward and cmtts_frame_forward_sub_t timed separately with device events, with no controls, with the
scalar controls (p, e, d) = (1.3, 0.8, 1.25), and with the same values as [B, L] control tables (cmtts_set_control_tables).  The
controls are installed once, outside the timed window: the window holds what the C ABI's calls enqueue.  Median and spread over
--reps windows of --calls calls each, the three modes alternating.  On a build without cmtts_set_control_tables only the first two
modes run (that is the run the tables are compared against).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd  # noqa: E402,F401
from cmtts_amd import _lib, host  # noqa: E402
from cmtts_amd.config import get_config  # noqa: E402
from cmtts_amd.weights import synth_cmtts_state_dict  # noqa: E402

P, E, D = 1.3, 0.8, 1.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phonemes", type=int, default=85)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("controls_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    lib = _lib.load()
    cfg = get_config("VCTK")
    # 4 frames per phoneme, all equal (dur_spread = 0): 85 * 4 * 1.25 = 425 <= 512
    m = host.CMTotalTTS(cfg, dev).load_state_dict(synth_cmtts_state_dict(cfg, seed=0, dur_frames=4.0, dur_spread=0.0))
    B, L, T = a.batch, a.phonemes, a.frames
    rs = np.random.RandomState(0)
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)).to(dev)
    src = torch.full((B,), L, dtype=torch.int64, device=dev)
    spk = torch.from_numpy(rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32)).to(dev)
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    i64 = lambda *s: torch.empty(*s, dtype=torch.int64, device=dev)
    log_d, d_r, e_pred, mel_len, e_idx = f(B, L), f(B, L), f(B, L), i64(B), i64(B, L)
    cond, mel2ph, cwt, f0, p_idx, stats = f(B, cfg.hidden, T), i64(B, T), f(B, T, cfg.cwt_out), f(B, T), i64(B, T), f(B, 2)
    p1_ld = (L + 3) // 4 * 4
    p1, p1t = f(B, cfg.res_layers * cfg.res_channels, p1_ld), f(B, cfg.res_layers, p1_ld, cfg.res_channels)
    nb, nf = lib.cmtts_text_workspace_bytes(m._h, B, L), lib.cmtts_frame_workspace_bytes(m._h, B, T)
    tws, fws = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(nf, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()

    def text(d):
        _lib.check(lib.cmtts_text_forward(m._h, ptr(texts), ptr(src), ptr(spk), None, B, L, d, ptr(log_d), ptr(d_r), ptr(mel_len),
                                          ptr(e_pred), ptr(e_idx), None, None, ptr(tws), nb, stream))

    def frame(_d):
        _lib.check(lib.cmtts_frame_forward_sub_t(m._h, ptr(tws), B, L, 0, B, T, ptr(cond), ptr(mel2ph), ptr(cwt), ptr(f0), ptr(p_idx),
                                                 ptr(stats), ptr(p1), ptr(p1t), ptr(fws), nf, stream))

    tabs = [torch.full((B, L), v, dtype=torch.float32, device=dev) for v in (D, E, P)]

    def install(mode):
        lib.cmtts_set_variance_controls(m._h, None)
        if hasattr(lib, "cmtts_set_control_tables"):
            lib.cmtts_set_control_tables(m._h, None)
        if mode == "scalar":
            vc = _lib.VarianceControlsStruct(p_control=P, e_control=E)
            _lib.check(lib.cmtts_set_variance_controls(m._h, C.byref(vc)))
            return D
        if mode == "tables":
            ct = _lib.ControlTablesStruct(d=ptr(tabs[0]), e=ptr(tabs[1]), p=ptr(tabs[2]), ld=L)
            _lib.check(lib.cmtts_set_control_tables(m._h, C.byref(ct)))
        return 1.0

    def window(fn, d):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn(d)
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.calls          # microseconds per call

    modes = ["none", "scalar"] + (["tables"] if "cmtts_set_control_tables" in _lib.SIGNATURES else [])
    times = {mo: {"text_us": [], "frame_us": []} for mo in modes}
    lens = {}
    try:
        for mo in modes:                                    # warm every mode's kernels
            d = install(mo)
            for _ in range(5):
                text(d)
                frame(d)
            torch.cuda.synchronize()
            lens[mo] = int(mel_len.max())
        for _ in range(a.reps):
            for mo in modes:                                # alternating: drift hits every mode alike
                d = install(mo)
                times[mo]["text_us"].append(window(text, d))
                times[mo]["frame_us"].append(window(frame, d))
    finally:
        install("none")
        torch.cuda.synchronize()
    assert lens["scalar"] <= T, lens
    if "tables" in lens:
        assert lens["tables"] == lens["scalar"], lens
    out = {"tool": "controls_bench", "B": B, "L": L, "T": T, "calls": a.calls, "reps": a.reps, "max_mel_len": lens}
    for mo in modes:
        for k, v in times[mo].items():
            out[f"{mo}_{k}"] = {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
