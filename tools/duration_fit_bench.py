#!/usr/bin/env python3
"""Cost of the duration targets (cmtts_set_duration_targets, csrc/duration_fit.hip).  Three measurements, device events, median
and spread over --reps windows of --calls calls each, the modes alternating inside one process:

  text side    cmtts_text_forward at B = --batch, L = --phonemes with nothing installed ("none"), with one target per utterance
               ("utterance") and with --segments segments per utterance ("segments").  The targets are installed once, outside the
               timed window: the window holds what the C ABI's calls enqueue.
  kernel       duration_fit_kernel alone (csrc/internal_hooks.h: cmtts_internal_duration_fit) at the same shape and at
               B = 1 and B = --batch with L = --long-phonemes, utterance and segment form.  It runs in place, so calls after the
               first re-fit durations that already meet their target: the same loops over the same number of phonemes.
  predictor    for scale, the text side itself at B = 1, L = --long-phonemes (what stands in front of the fit there) — skipped
               with --no-long-text.

On a build without cmtts_set_duration_targets only the "none" text side runs: that is the parent's run the rest is compared
against.  Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--phonemes", type=int, default=85)
    ap.add_argument("--long-phonemes", type=int, default=1000)
    ap.add_argument("--segments", type=int, default=12)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-long-text", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("duration_fit_bench.py needs a GPU: there is nothing to time without one")
    dev = "cuda:0"
    lib = _lib.load()
    have = "cmtts_set_duration_targets" in _lib.SIGNATURES
    cfg = get_config("VCTK")
    m = host.CMTotalTTS(cfg, dev).load_state_dict(synth_cmtts_state_dict(cfg, seed=0, dur_frames=4.0, dur_spread=0.03))
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()
    rs = np.random.RandomState(0)

    def text_side(B, L):
        texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)).to(dev)
        src = torch.full((B,), L, dtype=torch.int64, device=dev)
        spk = torch.from_numpy(rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32)).to(dev)
        log_d, d_r, e_pred = (torch.empty(B, L, dtype=torch.float32, device=dev) for _ in range(3))
        mel_len, e_idx = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, L, dtype=torch.int64, device=dev)
        nb = lib.cmtts_text_workspace_bytes(m._h, B, L)
        tws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.cmtts_text_forward(m._h, ptr(texts), ptr(src), ptr(spk), None, B, L, 1.0, ptr(log_d), ptr(d_r), ptr(mel_len),
                                              ptr(e_pred), ptr(e_idx), None, None, ptr(tws), nb, stream))
        return call, mel_len, src, (texts, spk, log_d, d_r, e_pred, e_idx, tws)

    def segment_table(B, L, G):
        seg = np.minimum(np.arange(L) * G // L, G - 1)[None].repeat(B, 0).astype(np.int32)
        seg[:, -max(1, L // 20):] = -1                          # an unsegmented tail
        return torch.from_numpy(seg).to(dev)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.calls          # microseconds per call

    def summary(v):
        return {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)}

    def alternate(fns, setup=None):
        """fns: {name: callable}; warm each, then --reps rounds with the names alternating (drift hits every one alike)."""
        times = {k: [] for k in fns}
        for k, fn in fns.items():
            if setup:
                setup(k)
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in fns.items():
                if setup:
                    setup(k)
                times[k].append(window(fn))
        return {k: summary(v) for k, v in times.items()}

    out = {"tool": "duration_fit_bench", "B": a.batch, "L": a.phonemes, "L_long": a.long_phonemes, "segments": a.segments,
           "calls": a.calls, "reps": a.reps, "targets_available": have}

    # ---- the text side with and without targets
    B, L, G = a.batch, a.phonemes, a.segments
    call, mel_len, src, _keep = text_side(B, L)
    call()
    torch.cuda.synchronize()
    S = mel_len.clone()
    out["plain_mel_len_max"] = int(S.max())
    tgt1 = (S * 5 // 4 + 3).to(torch.int32).reshape(B, 1).contiguous()
    tgtG = torch.full((B, G), int(S.max()) // G + 5, dtype=torch.int32, device=dev)
    seg = segment_table(B, L, G)
    unmet = torch.zeros(B, dtype=torch.int32, device=dev)

    def install(mode):
        if not have:
            return
        if mode == "none":
            lib.cmtts_set_duration_targets(m._h, None)
            return
        dt = _lib.DurationTargetsStruct(seg=ptr(seg) if mode == "segments" else None, target=ptr(tgtG if mode == "segments" else tgt1),
                                        unmet=ptr(unmet), ld=L, n_seg=G if mode == "segments" else 1)
        _lib.check(lib.cmtts_set_duration_targets(m._h, C.byref(dt)))

    modes = ["none"] + (["utterance", "segments"] if have else [])
    try:
        out["text_us"] = alternate({mo: call for mo in modes}, install)
        if have:
            install("utterance")
            call()
            torch.cuda.synchronize()
            assert torch.equal(mel_len, tgt1[:, 0].to(torch.int64)) and not bool(unmet.any()), "the targets were not met"
    finally:
        install("none")
        torch.cuda.synchronize()

    # ---- the kernel alone
    if have:
        def kernel(Bk, Lk, Gk):
            d = torch.from_numpy(rs.randint(0, 9, size=(Bk, Lk)).astype(np.float32)).to(dev)
            cum = torch.empty(Bk, Lk, dtype=torch.int32, device=dev)
            ml = torch.empty(Bk, dtype=torch.int64, device=dev)
            sl = torch.full((Bk,), Lk, dtype=torch.int64, device=dev)
            sg = segment_table(Bk, Lk, Gk) if Gk > 1 else None
            tg = torch.full((Bk, Gk), 5 * Lk // Gk + 7, dtype=torch.int32, device=dev)
            um = torch.zeros(Bk, dtype=torch.int32, device=dev)
            keep = (d, cum, ml, sl, sg, tg, um)

            def run():
                _lib.check(_lib.internal_duration_fit(ptr(d), ptr(cum), ptr(ml), ptr(sl), ptr(sg), ptr(tg), ptr(um), Bk, Lk, Gk, stream))
            run.keep = keep
            return run
        LL = a.long_phonemes
        out["kernel_us"] = alternate({f"B{a.batch}_L{L}_utterance": kernel(a.batch, L, 1), f"B{a.batch}_L{L}_segments": kernel(a.batch, L, G),
                                      f"B1_L{LL}_utterance": kernel(1, LL, 1), f"B1_L{LL}_segments": kernel(1, LL, 10 * G),
                                      f"B{a.batch}_L{LL}_utterance": kernel(a.batch, LL, 1), f"B{a.batch}_L{LL}_segments": kernel(a.batch, LL, 10 * G)})

    # ---- for scale: the text side in front of the fit at the long shape
    if not a.no_long_text:
        call_long, _, _, _keep2 = text_side(1, a.long_phonemes)
        out["text_long_us"] = alternate({f"B1_L{a.long_phonemes}_none": call_long})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
