"""Batch-invariant fp32 synthesis: with the model option "batch_invariant" at 1 the per-layer residual blocks of small batches run the
persistent stack's Winograd F(4,3) form (csrc/resblock_split_w43.hip), and with the vocoder option at 1 the generator takes its
large-launch forms at every size — an utterance's mel, waveform and int16 PCM then do not depend on what it was batched with."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmtts_amd import _lib
from cmtts_amd.config import get_config, HifiGanConfig
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict
from conftest import WINO_TOL, WINO_TRIM_TOL, report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_MODELS = {}


def _host():
    from cmtts_amd import host
    return host


def _model(variant):
    if variant not in _MODELS:
        cfg = get_config(variant)
        _MODELS[variant] = _host().CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=5))
    return _MODELS[variant]


class _opts:
    """Model option "batch_invariant" = 1 plus process-wide switches for the duration of a block; everything restored on exit."""

    def __init__(self, model, persist=None, split=None, fused=None):
        self.model, self.persist, self.split, self.fused = model, persist, split, fused

    def __enter__(self):
        lib = _lib.load()
        self.prev = (self.model.set_option("batch_invariant", 1), lib.cmtts_set_persistent_denoiser(-1),
                     lib.cmtts_set_option(b"resblock_split", -1), lib.cmtts_set_fused_resblock(1))
        lib.cmtts_set_fused_resblock(self.prev[3])
        self.set(self.persist, self.split, self.fused)
        return self

    def set(self, persist=None, split=None, fused=None):
        lib = _lib.load()
        if persist is not None:
            lib.cmtts_set_persistent_denoiser(persist)
        if split is not None:
            lib.cmtts_set_option(b"resblock_split", split)
        if fused is not None:
            lib.cmtts_set_fused_resblock(fused)

    def __exit__(self, *exc):
        lib = _lib.load()
        self.model.set_option("batch_invariant", self.prev[0])
        lib.cmtts_set_persistent_denoiser(self.prev[1])
        lib.cmtts_set_option(b"resblock_split", self.prev[2])
        lib.cmtts_set_fused_resblock(self.prev[3])


def _inputs(cfg, B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, cfg.n_mels, generator=gen)
    cond = torch.randn(B, T, cfg.hidden, generator=gen)
    spk = torch.randn(B, cfg.hidden, generator=gen) if cfg.multi_speaker else None
    noise = torch.randn(5, B, 1, T, cfg.n_mels, generator=gen).to(DEV)
    return x, cond, spk, noise


def _routes(model, x, t, cond, spk, cond_ct, spk_d, noise, factors=None):
    """One network evaluation + T = 1 / 2 / 4 samples."""
    host = _host()
    out = [model.net(x, t, cond, spk).clone()]
    for n in (1, 2, 4):
        out.append(host.sample_with_cond(model, cond_ct, spk_d, n, noise, factors=factors).clone())
    return out


@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
@pytest.mark.parametrize("B", [1, 3, 40])
@pytest.mark.parametrize("T", [1, 3, 33, 130, 257, 1000])
def test_persistent_vs_per_layer_bitwise(variant, B, T):
    """Option at 1, winograd at its default (F(4,3)): the forced persistent stack and every per-layer route (split, fused one-workgroup,
    three-launch) give the same bits — T not a multiple of 4, T < 4, multi-tile halos, B = 40 chunked over the chip."""
    model = _model(variant)
    cfg = model.config
    x, cond, spk, noise = _inputs(cfg, B, T, B * 1000 + T)
    t = torch.full((B,), 1095.5)
    cond_ct = cond.transpose(1, 2).contiguous().to(DEV)
    spk_d = spk.to(DEV) if spk is not None else None
    with _opts(model, persist=2) as o:
        ref = _routes(model, x, t, cond, spk, cond_ct, spk_d, noise)
        got = {}
        for name, kw in (("split", dict(persist=0, split=2)), ("fused", dict(persist=0, split=0)), ("unfused", dict(persist=0, fused=0))):
            o.set(**kw)
            got[name] = _routes(model, x, t, cond, spk, cond_ct, spk_d, noise)
            o.set(fused=1)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    for name, outs in got.items():
        for i, (a, b) in enumerate(zip(outs, ref)):
            assert torch.equal(a, b), (name, i, float((a - b).abs().max()))


@pytest.mark.parametrize("B,L", [(1, 9), (3, 30), (40, 22)])
def test_persistent_vs_per_layer_factors_bitwise(B, L):
    """The same with the conditioner factors of the duration net (cmtts_sample_factored: the persistent stack gathers them, the per-layer
    routes expand them first)."""
    host = _host()
    model = _model("LJSpeech")
    cfg = model.config
    rs = np.random.RandomState(B * 10 + L)
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)).to(DEV)
    lens = torch.full((B,), L, dtype=torch.int64, device=DEV)
    out = model.duration_pitch_energy_net(None, texts, lens)
    cond_ct, f = out["cond_ct"], out["cond_factors"]
    T = cond_ct.shape[2]
    noise = torch.randn(5, B, 1, T, cfg.n_mels, generator=torch.Generator().manual_seed(L)).to(DEV)
    with _opts(model, persist=2) as o:
        ref = [host.sample_with_cond(model, cond_ct, None, n, noise, factors=f).clone() for n in (1, 2, 4)]
        o.set(persist=0, split=2)
        split = [host.sample_with_cond(model, cond_ct, None, n, noise, factors=f).clone() for n in (1, 2, 4)]
        o.set(split=0)
        fused = [host.sample_with_cond(model, cond_ct, None, n, noise, factors=f).clone() for n in (1, 2, 4)]
    torch.cuda.synchronize()
    for a, b, c in zip(ref, split, fused):
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c), (T, float((a - b).abs().max()), float((a - c).abs().max()))


@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
def test_utterance_alone_equals_in_batch(variant):
    """End to end: an utterance alone (B = 1: per-layer route) gives the mel bits it gets inside a B = 40 batch (persistent route), with the
    same padded T, conditioning and noise — at the default persistent policy, nothing forced."""
    host = _host()
    model = _model(variant)
    cfg = model.config
    B, T = 40, 200
    x, cond, spk, noise = _inputs(cfg, B, T, 77)
    t = torch.full((B,), 1095.5)
    cond_ct = cond.transpose(1, 2).contiguous().to(DEV)
    spk_d = spk.to(DEV) if spk is not None else None
    with _opts(model, persist=1, split=1):
        one_b = model.net(x, t, cond, spk).clone()
        mel_b = host.sample_with_cond(model, cond_ct, spk_d, 4, noise).clone()
        alone = {}
        for b in (0, 17, B - 1):
            sl = slice(b, b + 1)
            alone[b] = (model.net(x[sl], t[sl], cond[sl], spk[sl] if spk is not None else None).clone(),
                        host.sample_with_cond(model, cond_ct[sl].contiguous(), spk_d[sl].contiguous() if spk_d is not None else None, 4,
                                              noise[:, sl].contiguous()).clone())
    torch.cuda.synchronize()
    for b, (o1, m1) in alone.items():
        assert torch.equal(o1[0], one_b[b]), (b, float((o1[0] - one_b[b]).abs().max()))
        assert torch.equal(m1[0], mel_b[b]), (b, float((m1[0] - mel_b[b]).abs().max()))


@pytest.mark.parametrize("n_steps", [1, 4])
def test_ragged_set_aside_bitwise(n_steps):
    """cmtts_sample_ragged: the small group set aside for the per-layer kernels (15 x 1024 + 8 x 256 frames: leaving the 256-frame group out
    fits one persistent round) gives bitwise the mels of its bucket's uniform persistent launch, like the group that shares the launch.
    Trimmed runs keep the F(4,3) trimming caveat: frames near the end of a trimmed utterance are within WINO_TRIM_TOL (conftest.py), because a
    quad rounds every output from all six of its inputs."""
    host = _host()
    lib = _lib.load()
    cfg = get_config("LibriTTS")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=12, dur_frames=4.0, dur_spread=0.0))
    rs = np.random.RandomState(6)

    def make(bucket, n):
        Lmax = bucket // 4
        ln = np.maximum((rs.uniform(0.3, 1.0, size=n) * Lmax).astype(np.int64), 1)
        ln[0] = Lmax
        tx = rs.randint(1, cfg.n_symbols, size=(n, Lmax)).astype(np.int64)
        tx[np.arange(Lmax)[None, :] >= ln[:, None]] = 0
        gen = torch.Generator().manual_seed(bucket + n)
        return (torch.from_numpy(tx).to(DEV), torch.from_numpy(ln).to(DEV), torch.randn(n, cfg.external_speaker_dim, generator=gen).to(DEV),
                torch.randn(n_steps + 1, n, 1, bucket, cfg.n_mels, generator=gen).to(DEV), bucket)

    groups = [make(1024, 15), make(256, 8)]
    with _opts(model):
        prev = lib.cmtts_set_persistent_denoiser(2)
        try:
            seq = []
            for tx, ln, spk, nz, bucket in groups:
                o = model.duration_pitch_energy_net(None, tx, ln, spker_embeds=spk, max_mel_len=bucket)
                seq.append((host.sample_with_cond(model, o["cond_ct"], o["speaker_emb"], n_steps, nz, factors=o["cond_factors"]), o["mel_lens"]))
        finally:
            lib.cmtts_set_persistent_denoiser(prev)
        full = host.BucketedSynthesizer(model, n_steps=n_steps, n_streams=2, trim=False, batch_text=True).run(groups)
        trim = host.BucketedSynthesizer(model, n_steps=n_steps, n_streams=2, tail_frames=16).run(groups)
    host.synchronize()
    for gi, ((m0, l0), (m1, l1), (m2, l2)) in enumerate(zip(seq, full, trim)):
        assert torch.equal(l0, l1) and torch.equal(l0, l2)
        assert torch.isfinite(m0).all() and torch.equal(m0, m1), (gi, float((m0 - m1).abs().max()))
        for b, n in enumerate(l0.tolist()):
            keep = min(n + 16, m0.shape[1])
            assert float((m2[b, :keep] - m0[b, :keep]).abs().max()) <= WINO_TRIM_TOL, (gi, b)


def test_accuracy_small_batch():
    """Option at 1, small batch: within WINO_TOL of the per-layer direct form (and not equal to it: the F(4,3) form ran), and no farther
    from the float64 oracle than the direct form (a factor 2 of slack on two fp32 roundings of the same size)."""
    from oracle import cmtts_oracle as O
    host = _host()
    cfg = get_config("VCTK")
    sd = synth_cmtts_state_dict(cfg, seed=3, dur_frames=4.0, dur_spread=0.0)
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(sd)
    B, T = 2, 130
    rs = np.random.RandomState(1)
    cond = rs.standard_normal(size=(B, T, cfg.hidden)).astype(np.float32)
    spk = rs.standard_normal(size=(B, cfg.hidden)).astype(np.float32)
    noise = np.stack([rs.standard_normal(size=(B, 1, T, cfg.n_mels)).astype(np.float32) for _ in range(3)])
    cond_ct = torch.from_numpy(np.ascontiguousarray(cond.transpose(0, 2, 1))).to(DEV)
    args = (cond_ct, torch.from_numpy(spk).to(DEV), 2, torch.from_numpy(noise).to(DEV))
    direct = host.sample_with_cond(model, *args).clone()
    with _opts(model, persist=1):
        w43 = host.sample_with_cond(model, *args).clone()
    ref = O.karras_sample_tts(sd, cfg, cond, spk, 2, list(noise))
    d = float((w43 - direct).abs().max())
    e_d = float(np.abs(direct.cpu().numpy() - ref).max())
    e_w = float(np.abs(w43.cpu().numpy() - ref).max())
    report(f"BATCH_INVARIANT accuracy B={B} T={T}: |F(4,3) - direct| {d:.2e}; vs float64: direct {e_d:.2e}, F(4,3) {e_w:.2e}")
    assert 0 < d <= WINO_TOL
    assert e_w <= 2.0 * e_d


def test_generator_row_alone_equals_batch():
    """Vocoder option at 1: every row of a B = 32 fp32 batch is bitwise the same mel vocoded alone (waveform and int16 PCM), and the B = 32
    output equals the default B = 32 output (large launches are unchanged)."""
    host = _host()
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    B, T = 32, 300
    mel = (0.5 * torch.randn(B, hcfg.num_mels if hasattr(hcfg, "num_mels") else 80, T, generator=torch.Generator().manual_seed(9))).to(DEV)
    default = voc(mel).clone()
    alone0 = voc(mel[:1].contiguous()).clone()
    prev = voc.set_option("batch_invariant", 1)
    try:
        big = voc(mel).clone()
        alone = [voc(mel[b:b + 1].contiguous()).clone() for b in range(B)]
        pcm_big = host.vocoder_infer(mel, voc)
        pcm_alone = [host.vocoder_infer(mel[b:b + 1].contiguous(), voc)[0] for b in range(B)]
    finally:
        voc.set_option("batch_invariant", prev)
    torch.cuda.synchronize()
    assert not torch.equal(alone0[0], default[0])       # without the option a lone row takes other forms (the test is not vacuous)
    assert torch.equal(big, default)
    for b in range(B):
        assert torch.equal(alone[b][0], big[b]), (b, float((alone[b][0] - big[b]).abs().max()))
        assert np.array_equal(pcm_alone[b], pcm_big[b]), b


def test_plumbing_winograd2_unsupported_and_16bit():
    """winograd = 2 with the option at 1: every denoiser call returns CMTTS_E_UNSUPPORTED and writes nothing; the 16-bit models' outputs are
    the same bits with the option on and off."""
    host = _host()
    lib = _lib.load()
    model = _model("VCTK")
    cfg = model.config
    B, T = 2, 70
    x, cond, spk, noise = _inputs(cfg, B, T, 3)
    cond_ct = cond.transpose(1, 2).contiguous().to(DEV)
    spk_d = spk.to(DEV)
    prev_w = model.set_option("winograd", 2)
    try:
        with _opts(model, persist=1):
            sig = (C.c_float * 1)()
            std = (C.c_float * 1)()
            _lib.check(lib.cmtts_schedule(model._h, 1, sig, std))
            nb = lib.cmtts_denoiser_workspace_bytes(model._h, B, T)
            ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
            mel = torch.full((B, T, cfg.n_mels), 7.0, device=DEV)
            torch.cuda.synchronize()
            rc = lib.cmtts_sample(model._h, host._ptr(noise), host._ptr(cond_ct), host._ptr(spk_d), B, T, 1, sig, std, host._ptr(mel),
                                  host._ptr(ws), nb, host._stream())
            assert rc == -2 and b"batch_invariant" in lib.cmtts_last_error()
            xd = x.reshape(B, T, cfg.n_mels).transpose(1, 2).contiguous().to(DEV)
            tt = torch.full((B,), 1095.5, device=DEV)
            rc = lib.cmtts_denoiser_forward(model._h, host._ptr(xd), host._ptr(tt), host._ptr(cond_ct), host._ptr(spk_d), B, T, host._ptr(mel),
                                            host._ptr(ws), nb, host._stream())
            assert rc == -2
            torch.cuda.synchronize()
            assert bool((mel == 7.0).all())
    finally:
        model.set_option("winograd", prev_w)
    t = torch.full((B,), 1095.5)
    try:
        for prec in ("bf16", "fp16"):
            model.set_precision(prec)
            off = model.net(x, t, cond, spk).clone()
            with _opts(model, persist=0):
                on = model.net(x, t, cond, spk).clone()
            assert torch.equal(on, off), prec
    finally:
        model.set_precision("fp32")
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    voc.set_precision("bf16")
    m = torch.randn(1, 80, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    off = voc(m).clone()
    voc.set_option("batch_invariant", 1)
    on = voc(m).clone()
    assert torch.equal(on, off)
