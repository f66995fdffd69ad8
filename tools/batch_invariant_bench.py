#!/usr/bin/env python3
"""Small-batch latency with the batch-invariance options: text -> mel at T = 1 / 4 for 1 x 25, 1 x 85 and 8 x 25 phonemes
(LJSpeech, 6 frames per phoneme) with the model option "batch_invariant" at 0 (default: per-layer kernels, direct form) and at 1 (per-layer
kernels, the persistent stack's F(4,3) form), and the fp32 generator on 1 x 512 / 8 x 512 frames with the vocoder option off / on.
Wall time per request (median of 20), stream idle between requests."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, cmtts_amd  # noqa: E401,F401
from cmtts_amd import host
from cmtts_amd.config import get_config, HifiGanConfig
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict

cfg = get_config("LJSpeech")
DUR = 6
model = host.CMTotalTTS(cfg, "cuda:0").load_state_dict(synth_cmtts_state_dict(cfg, seed=0, dur_frames=float(DUR), dur_spread=0.0))
voc = host.Generator(HifiGanConfig(), "cuda:0").load_state_dict(synth_hifigan_state_dict(HifiGanConfig(), seed=0))


def clock(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


for B, L in [(1, 25), (1, 85), (8, 25)]:
    rs = np.random.RandomState(B * 100 + L)
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)).cuda()
    lens = torch.full((B,), L, dtype=torch.int64, device="cuda")
    T = L * DUR
    noise = torch.randn(5, B, 1, T, cfg.n_mels, device="cuda")

    def text2mel(n_steps):
        out = model.duration_pitch_energy_net(None, texts, lens, max_mel_len=T)
        host.sample_with_cond(model, out["cond_ct"], None, n_steps, noise[:n_steps + 1])

    r = {}
    for bi in (0, 1):
        model.set_option("batch_invariant", bi)
        r[bi] = [clock(lambda: text2mel(n)) for n in (1, 4)]
    model.set_option("batch_invariant", 0)
    print(f"{B} x {L} phonemes (T = {T} frames): text->mel T=1 {r[0][0]:.3f} -> {r[1][0]:.3f} ms ({r[1][0] / r[0][0]:.2f}x)   "
          f"T=4 {r[0][1]:.3f} -> {r[1][1]:.3f} ms ({r[1][1] / r[0][1]:.2f}x)", flush=True)

for B in (1, 8):
    mel = torch.randn(B, 80, 512, device="cuda")
    v = {}
    for bi in (0, 1):
        voc.set_option("batch_invariant", bi)
        v[bi] = clock(lambda: voc(mel))
    voc.set_option("batch_invariant", 0)
    print(f"generator fp32 {B} x 512 frames: {v[0]:.3f} -> {v[1]:.3f} ms ({v[1] / v[0]:.2f}x)", flush=True)
