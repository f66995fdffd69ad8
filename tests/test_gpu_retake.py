"""Re-taking spans of an utterance on the GPU (include/cmtts_hip.h: cmtts_retake; csrc/retake.hip; host.retake / host.retake_pcm;
DESIGN.md §3.6e): the step kernel against the numpy definition bit for bit, kept frames bit for bit, the sampler against the float64
oracle with the plain sampler's own error as the yardstick, windows against the whole utterance, and the spliced PCM."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmtts_amd import _lib, noise as N, retake as R
from cmtts_amd.config import get_config, HifiGanConfig
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict
from conftest import report, same_pcm, same_trimmed
from oracle import cmtts_oracle as O
from retake_cases import SPAN_CASES, T_GPU, default_schedule, gap_spans

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = 256
_MODELS, _SDS, _BATCH, _ORACLE = {}, {}, {}, {}
SEEDS = np.asarray([0, -1, -(1 << 63) + 12345, 0x0123456789ABCDEF], np.int64)


def _host():
    from cmtts_amd import host
    return host


def _sd(variant):
    if variant not in _SDS:
        _SDS[variant] = synth_cmtts_state_dict(get_config(variant), seed=5)
    return _SDS[variant]


def _model(variant):
    if variant not in _MODELS:
        _MODELS[variant] = _host().CMTotalTTS(get_config(variant), DEV).load_state_dict(_sd(variant))
    return _MODELS[variant]


def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _batch(variant, B, T):
    """Random conditioning of a (B, T) batch, its seeds, and the utterances as they are: the plain seeded sampler's mel."""
    key = (variant, B, T)
    if key not in _BATCH:
        host, model = _host(), _model(variant)
        cfg = model.config
        g = torch.Generator().manual_seed(1000 + T)
        cond_ct = torch.randn(B, cfg.hidden, T, generator=g).to(DEV)
        spk = torch.randn(B, cfg.hidden, generator=g).to(DEV) if cfg.multi_speaker else None
        seeds = N.utterance_seeds(31, np.arange(B))
        mel = host.sample_with_cond(model, cond_ct, spk, 2, seeds=seeds).clone()
        _BATCH[key] = (model, cond_ct, spk, seeds, mel)
    return _BATCH[key]


def _all_spans(halo):
    """Every span of the kept-frames test on B = 3, T = 200: tile-crossing, clamped at 0 and at T, not quad-aligned, and on utterance 2
    two spans with halo - 1 kept frames between them (one cluster) and two with halo (two windows)."""
    near = [(2, lo, hi) for _, lo, hi in gap_spans(halo, True)]
    far = [(2, lo + 90, hi + 90) for _, lo, hi in gap_spans(halo, False)]
    return SPAN_CASES["tile"] + SPAN_CASES["odd"] + SPAN_CASES["head"] + [(1, 191, 200)] + near + far


# ----------------------------------------------------------------------------- 1. the step kernel alone

@pytest.mark.parametrize("M", [80, 6])
def test_step_kernel_bits(M):
    """retake_step_kernel through its hook against numpy, bit for bit: x_T, a mid step and the last step (with and without a re-noise
    term), z taken from host.seeded_noise at each row's start frame."""
    host = _host()
    cfg = get_config("VCTK")
    Nw, Tw, T = 3, 37, 1040
    starts = (0, 1000, 7)
    seeds = SEEDS[:Nw]
    F = np.float32
    rs = np.random.RandomState(M)
    x0 = rs.standard_normal((Nw, Tw, M)).astype(F)
    known = rs.standard_normal((Nw, Tw, M)).astype(F)
    masks = {"none": np.zeros((Nw, Tw), bool), "all": np.ones((Nw, Tw), bool), "one": np.zeros((Nw, Tw), bool), "odd": np.zeros((Nw, Tw), bool)}
    masks["one"][1, 17] = True
    masks["odd"][:, 5:18] = True
    wins = torch.tensor([(n, starts[n], 0, Tw) for n in range(Nw)], dtype=torch.int32, device=DEV)
    sd = torch.from_numpy(seeds).to(DEV)
    tx0, tknown = torch.from_numpy(x0).to(DEV), torch.from_numpy(known).to(DEV)

    def z(draw):
        rows = [host.seeded_noise(seeds[n:n + 1], 1, Tw, M, DEV, first_draw=draw, t0=starts[n]) for n in range(Nw)]
        return torch.cat(rows, 1)[0, :, 0].cpu().numpy()

    def run(mode, draw, scale, mask, out):
        tm = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(DEV)
        assert _lib.internal_retake_step(_p(tx0), _p(tknown), _p(tm), _p(sd), _p(wins), Nw, Tw, M, T, draw, scale, mode, _p(out), _stream()) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def same(a, b):
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))

    sig, nstd = default_schedule(cfg, 4)
    got = run(0, 0, cfg.sigma_max, None, torch.zeros(Nw, Tw, M, device=DEV))
    assert same(got, z(0) * F(cfg.sigma_max)), "x_T"
    z2, z4 = z(2), z(4)
    for name, mask in masks.items():
        m3 = mask[:, :, None]
        got = run(1, 2, float(nstd[1]), mask, torch.zeros(Nw, Tw, M, device=DEV))
        assert same(got, np.where(m3, x0, known) + (z2 * nstd[1]) * F(0.85)), ("mid", name)
        for scale in (float(nstd[3]), -1.0):
            ref = np.full((Nw, T, M), 7.5, F)
            val = x0 + (z4 * F(scale)) * F(0.85) if scale >= 0 else x0
            for n in range(Nw):
                ref[n, starts[n]:starts[n] + Tw][mask[n]] = val[n][mask[n]]
            got = run(2, 4, scale, mask, torch.full((Nw, T, M), 7.5, device=DEV))
            assert same(got, ref), ("last", name, scale)
    assert 0 < nstd[3] < 1e-6 and nstd[1] > 79


# ----------------------------------------------------------------------------- 2. kept frames

@pytest.mark.parametrize("windowed", [True, False])
@pytest.mark.parametrize("n_steps", [1, 2, 4])
def test_kept_frames_bitwise(conv_form, n_steps, windowed):
    host = _host()
    model, cond_ct, spk, seeds, mel = _batch("VCTK", 3, T_GPU)
    spans = _all_spans(model.config.res_layers)
    mask = torch.from_numpy(R.regen_mask(spans, 3, T_GPU)).to(DEV)
    out = host.retake(model, mel, cond_ct, spk, spans, N.utterance_seeds(77, np.arange(3)), n_steps=n_steps, windowed=windowed)
    host.synchronize()
    assert out.shape == mel.shape and out.data_ptr() != mel.data_ptr()
    assert torch.equal(out[~mask].view(torch.int32), mel[~mask].view(torch.int32))
    assert torch.isfinite(out).all()
    assert bool((out != mel).any(-1)[mask].all()), "a regenerated frame kept its old values"


# ----------------------------------------------------------------------------- 3. against the float64 oracle

ORACLE_SPANS = [(0, 44, 50), (1, 0, 9), (1, 90, 96)]
SCHEDULES = {"n2": (2, None), "n4": (4, None), "ts": (3, (0, 13, 26, 39))}


def _oracle_case(variant, sched):
    """(GPU retake, e_retake, e_plain) at B = 2, T = 96 on one schedule: both errors are max|GPU - float64 oracle| on the same conditioning
    and the same noise values (the device's seeded noise, fed to the oracle as it is)."""
    key = (variant, sched)
    if key in _ORACLE:
        return _ORACLE[key]
    host = _host()
    B, T = 2, 96
    model, cond_ct, spk, seeds, mel = _batch(variant, B, T)
    cfg, lib = model.config, model.lib
    n_steps, ts = SCHEDULES[sched]
    if ts is None:
        sig, std = (C.c_float * n_steps)(), (C.c_float * n_steps)()
        _lib.check(lib.cmtts_schedule(model._h, n_steps, sig, std))
        sig, std = np.asarray(list(sig), np.float32), np.asarray(list(std), np.float32)
    else:
        sig, std = R.schedule_from_ts(ts, 40, cfg.sigma_min, cfg.sigma_max, cfg.rho)
    take = N.utterance_seeds(55, np.arange(B))
    got = host.retake(model, mel, cond_ct, spk, ORACLE_SPANS, take, n_steps=n_steps, ts=ts, steps=40)
    # the plain sampler on the same schedule and the same kind of noise
    noise = host.seeded_noise(take, n_steps + 1, T, cfg.n_mels, DEV)
    plain = torch.empty(B, T, cfg.n_mels, device=DEV)
    nb = lib.cmtts_denoiser_workspace_bytes(model._h, B, T)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_sample(model._h, _p(noise), _p(cond_ct), _p(spk), B, T, n_steps, (C.c_float * n_steps)(*sig.tolist()),
                                (C.c_float * n_steps)(*std.tolist()), _p(plain), _p(ws), nb, _stream()))
    host.synchronize()
    sd = {k: np.asarray(v) for k, v in _sd(variant).items()}
    cond = np.ascontiguousarray(cond_ct.cpu().numpy().transpose(0, 2, 1))
    spk_np = None if spk is None else spk.cpu().numpy()
    z = noise.cpu().numpy()
    known = mel.cpu().numpy()[:, None]
    mask = R.regen_mask(ORACLE_SPANS, B, T)
    with O.precision("f64"):
        ref = R.retake_reference(lambda x, s: O.karras_denoise(sd, cfg, x, s, cond, spk_np), known, mask, z, sig, std, cfg.sigma_max, np.float64)
        ref_plain = O.karras_sample_tts(sd, cfg, cond, spk_np, n_steps, list(z), ts=ts, steps=40 if ts else 2)
    e_retake = float(np.abs(got.cpu().numpy() - ref[:, 0]).max())
    e_plain = float(np.abs(plain.cpu().numpy() - ref_plain).max())
    _ORACLE[key] = (got, e_retake, e_plain, mask, mel)
    return _ORACLE[key]


@pytest.mark.parametrize("sched", sorted(SCHEDULES))
@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
def test_against_oracle(variant, sched):
    got, e_retake, e_plain, mask, mel = _oracle_case(variant, sched)
    report(f"RETAKE {variant} {sched}: max|retake - float64 definition| {e_retake:.2e}; the plain sampler against float64 on the same "
           f"schedule and noise {e_plain:.2e}")
    m = torch.from_numpy(mask).to(DEV)
    assert torch.equal(got[~m].view(torch.int32), mel[~m].view(torch.int32))
    assert e_retake <= max(4 * e_plain, 1e-4) and e_retake < 1e-3, (e_retake, e_plain)


# ----------------------------------------------------------------------------- 4. windows against the whole utterance

@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
def test_windowed_equals_whole(conv_form, variant):
    host = _host()
    model, cond_ct, spk, seeds, mel = _batch(variant, 3, T_GPU)
    spans = _all_spans(model.config.res_layers)
    take = N.utterance_seeds(78, np.arange(3))
    prev = model.set_option("batch_invariant", 1)
    try:
        win = host.retake(model, mel, cond_ct, spk, spans, take, n_steps=4, windowed=True).clone()
        whole = host.retake(model, mel, cond_ct, spk, spans, take, n_steps=4, windowed=False).clone()
    finally:
        model.set_option("batch_invariant", prev)
    host.synchronize()
    report(f"RETAKE windows {variant} {conv_form}: max|windowed - whole| {float((win - whole).abs().max()):.2e}")
    assert same_trimmed(win, whole, conv_form), float((win - whole).abs().max())
    assert not torch.equal(win, mel)


# ----------------------------------------------------------------------------- 5. row independence

def test_row_independent():
    host = _host()
    model, cond_ct, spk, seeds, mel = _batch("VCTK", 3, T_GPU)
    spans = _all_spans(model.config.res_layers)
    take = N.utterance_seeds(79, np.arange(3))
    prev = model.set_option("batch_invariant", 1)
    try:
        full = host.retake(model, mel, cond_ct, spk, spans, take, n_steps=4).clone()
        alone = host.retake(model, mel[1:2].contiguous(), cond_ct[1:2].contiguous(), spk[1:2].contiguous(),
                            [(0, lo, hi) for b, lo, hi in spans if b == 1], take[1:2], n_steps=4).clone()
    finally:
        model.set_option("batch_invariant", prev)
    host.synchronize()
    assert torch.equal(alone[0], full[1]), float((alone[0] - full[1]).abs().max())
    assert not torch.equal(full[1], mel[1])


# ----------------------------------------------------------------------------- 6. everything regenerated

@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
def test_all_regenerated_is_the_plain_sampler(variant):
    """With every frame regenerated the masked sampler is the plain one, up to the re-noise arithmetic (the fused tail adds the noise with
    an fmaf, the step kernel with a product and a sum): bounded by the plain sampler's own distance from float64 (test 3's yardstick)."""
    host = _host()
    B, T = 2, 96
    model, cond_ct, spk, seeds, mel = _batch(variant, B, T)
    e_plain = _oracle_case(variant, "n4")[2]
    take = N.utterance_seeds(55, np.arange(B))
    got = host.retake(model, mel, cond_ct, spk, [(b, 0, T) for b in range(B)], take, n_steps=4)
    plain = host.sample_with_cond(model, cond_ct, spk, 4, seeds=take)
    host.synchronize()
    e = float((got - plain).abs().max())
    report(f"RETAKE all frames {variant}: max|retake - sample_with_cond(seeds)| {e:.2e} (plain sampler against float64 {e_plain:.2e}); "
           f"bitwise equal: {torch.equal(got, plain)}")
    assert torch.isfinite(got).all()
    assert e <= max(4 * e_plain, 1e-4) and e < 1e-3, (e, e_plain)


# ----------------------------------------------------------------------------- 7. the audio

def test_retake_pcm(voc_form):
    host = _host()
    model, cond_ct, spk, seeds, mel = _batch("VCTK", 3, T_GPU)
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    spans = [(0, 60, 70), (1, 0, 9)]
    mel_new = host.retake(model, mel, cond_ct, spk, spans, N.utterance_seeds(80, np.arange(3)), n_steps=2)
    pcm_old = host.vocoder_infer(mel.transpose(1, 2), voc)
    got = host.retake_pcm(mel_new.transpose(1, 2), voc, pcm_old, spans)
    whole = host.vocoder_infer(mel_new.transpose(1, 2), voc)
    H = 13
    assert host.vocoder_halo_frames(hcfg) == H
    changed = np.zeros((3, T_GPU * HOP), bool)
    for b, lo, hi in spans:
        changed[b, HOP * max(lo - H, 0):HOP * (hi + H)] = True
    for b in range(3):
        assert got[b].dtype == np.int16 and got[b].shape == (T_GPU * HOP,)
        assert same_pcm(got[b], whole[b], voc_form), b
        assert np.array_equal(got[b][~changed[b]], np.asarray(pcm_old[b])[~changed[b]]), b
    assert not np.array_equal(got[0], np.asarray(pcm_old[0])) and np.array_equal(got[2], np.asarray(pcm_old[2]))
    short = host.retake_pcm(mel_new.transpose(1, 2), voc, pcm_old, spans, lengths=[T_GPU * HOP - 100, 64 * HOP + 5, 10])
    assert [len(w) for w in short] == [T_GPU * HOP - 100, 64 * HOP + 5, 10]
    assert all(np.array_equal(s, g[:len(s)]) for s, g in zip(short, got))
    for kw in ({"sample_rate": 8000}, {"encoding": "mulaw"}, {"gain_db": -3.0}):
        with pytest.raises(ValueError):
            host.retake_pcm(mel_new.transpose(1, 2), voc, pcm_old, spans, **kw)


# ----------------------------------------------------------------------------- 8. validation

def test_validation_launches_nothing():
    host = _host()
    model, cond_ct, spk, seeds, mel = _batch("VCTK", 3, T_GPU)
    lib, cfg = model.lib, model.config
    B, T, Tw, n = 3, T_GPU, 52, 2
    sig, std = (C.c_float * n)(), (C.c_float * n)()
    _lib.check(lib.cmtts_schedule(model._h, n, sig, std))
    good = [(0, 40, 20, 10), (1, 0, 0, 9)]
    regen = torch.from_numpy(R.regen_mask([(0, 60, 70), (1, 0, 9)], B, T).astype(np.uint8)).to(DEV)
    sd = torch.from_numpy(seeds).to(DEV)
    out = torch.full_like(mel, -123.0)
    nb = lib.cmtts_retake_workspace_bytes(model._h, 3, Tw)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)

    def call(wins=good, **kw):
        tab = np.ascontiguousarray(np.asarray(wins, np.int32).reshape(-1, 4))
        a = dict(m=model._h, known=_p(mel), regen=_p(regen), cond=_p(cond_ct), spk=_p(spk), seeds=_p(sd), B=B, T=T, win=C.c_void_p(tab.ctypes.data),
                 N=len(wins), Tw=Tw, n=n, sig=sig, std=std, out=_p(out), ws=_p(ws), nb=nb)
        a.update(kw)
        return lib.cmtts_retake(a["m"], a["known"], a["regen"], a["cond"], a["spk"], a["seeds"], a["B"], a["T"], a["win"], a["N"], a["Tw"], a["n"],
                                a["sig"], a["std"], a["out"], a["ws"], a["nb"], _stream())

    bad_std = (C.c_float * n)(-1.0, 0.0)
    null = C.c_void_p(0)
    cases = {
        "known": dict(known=null), "regen": dict(regen=null), "cond": dict(cond=null), "seeds": dict(seeds=null), "windows": dict(win=null),
        "sigmas": dict(sig=None), "std": dict(std=None), "ws": dict(ws=null), "speaker": dict(spk=null),
        "B": dict(B=0), "T": dict(T=0), "N": dict(N=0), "Tw": dict(Tw=0), "n_steps": dict(n=0), "Tw > T": dict(Tw=T + 4),
        "start < 0": dict(wins=[(0, -1, 20, 10)]), "past T": dict(wins=[(0, T - Tw + 1, 20, 10)]),
        "core_off": dict(wins=[(0, 40, -1, 10)]), "core_len": dict(wins=[(0, 40, 20, 0)]), "core past window": dict(wins=[(0, 40, 45, 10)]),
        "b = B": dict(wins=[(3, 40, 20, 10)]), "b < 0": dict(wins=[(-1, 40, 20, 10)]),
        "overlap": dict(wins=[(0, 40, 20, 10), (0, 30, 35, 5)]), "mid std < 0": dict(std=bad_std),
    }
    for name, kw in cases.items():
        assert call(**kw) == -1, name
    assert call(out=null) == -1
    assert call(nb=lib.cmtts_retake_workspace_bytes(model._h, len(good), Tw) - 1) == -4          # CMTTS_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -123.0).all()), "a refused call wrote to mel_out"
    assert call(wins=[(0, 40, 20, 10), (0, 30, 25, 5), (1, 0, 0, 9)]) == 0          # cores that touch do not overlap
    host.synchronize()
    m = regen.bool()
    assert torch.equal(out[~m], mel[~m]) and bool((out != mel).any(-1)[m].all())
    # in place: mel_out = mel_known
    inplace = mel.clone()
    assert call(known=_p(inplace), out=_p(inplace)) == 0
    host.synchronize()
    assert torch.equal(inplace[~regen.bool()], mel[~regen.bool()]) and torch.isfinite(inplace).all()


# ----------------------------------------------------------------------------- 9. 16-bit models

def test_bf16_kept_frames():
    host = _host()
    model, cond_ct, spk, seeds, mel = _batch("VCTK", 3, T_GPU)
    spans = _all_spans(model.config.res_layers)
    mask = torch.from_numpy(R.regen_mask(spans, 3, T_GPU)).to(DEV)
    model.set_precision("bf16")
    try:
        out = host.retake(model, mel, cond_ct, spk, spans, N.utterance_seeds(81, np.arange(3)), n_steps=2).clone()
        host.synchronize()
    finally:
        model.set_precision("fp32")
    assert torch.isfinite(out).all()
    assert torch.equal(out[~mask].view(torch.int32), mel[~mask].view(torch.int32))
    assert bool((out != mel).any(-1)[mask].all())
