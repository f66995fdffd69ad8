"""Mixed step counts in one batch (cmtts_sample_mixed): every utterance of a mixed call has the bits of its row in the
uniform entry points on the same full batch — on the per-layer routes, in the persistent tail's table form (fp32 and bf16), across the
chunked launch, with per-utterance sigmas inside one evaluation — finished utterances really leave, and the host surface puts every
utterance back where the caller had it."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmtts_amd import _lib, noise as N, retake as R, steps as S
from cmtts_amd.config import get_config, HifiGanConfig
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict
from conftest import WINO_TOL, conv_form, report, same_pcm, same_result, voc_form  # noqa: F401  (fixtures)
from oracle import cmtts_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = 256
_MODELS = {}
TS = ((0, 13, 26, 39), (0, 20, 39), (0, 39), (0, 39))        # tests/test_mixed_steps_cpu.py: 3, 2, 1, 1 evaluations, steps = 40


def _host():
    from cmtts_amd import host
    return host


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _model(variant, dur=None):
    key = (variant, dur)
    if key not in _MODELS:
        cfg = get_config(variant)
        sd = synth_cmtts_state_dict(cfg, seed=5) if dur is None else synth_cmtts_state_dict(cfg, seed=5, dur_frames=dur, dur_spread=0.0)
        _MODELS[key] = (_host().CMTotalTTS(cfg, DEV).load_state_dict(sd), sd)
    return _MODELS[key][0]


def _cond(variant, B, T, with_factors, seed, perm=None):
    """Conditioning of a (B, T) batch in the order `perm` of its inputs: from the duration net (with its factors; T = 8 frames per phoneme)
    or random."""
    g = torch.Generator().manual_seed(seed)
    perm = np.arange(B) if perm is None else np.asarray(perm)
    if with_factors:
        model = _model(variant, 8.0)
        cfg = model.config
        assert T % 8 == 0
        L = T // 8
        rs = np.random.RandomState(seed)
        texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)[perm]).to(DEV)
        lens = torch.full((B,), L, dtype=torch.int64, device=DEV)
        spk = torch.randn(B, cfg.external_speaker_dim, generator=g)[torch.from_numpy(perm)].to(DEV) if cfg.multi_speaker else None
        out = model.duration_pitch_energy_net(None, texts, lens, spker_embeds=spk)
        assert out["cond_ct"].shape[2] == T, out["cond_ct"].shape
        return model, out["cond_ct"], out["speaker_emb"], out["cond_factors"]
    model = _model(variant)
    cfg = model.config
    cond_ct = torch.randn(B, cfg.hidden, T, generator=g)[torch.from_numpy(perm)].contiguous().to(DEV)
    spk = torch.randn(B, cfg.hidden, generator=g)[torch.from_numpy(perm)].contiguous().to(DEV) if cfg.multi_speaker else None
    return model, cond_ct, spk, None


def _uniform_rows(model, cond_ct, spk, counts, f=None, seeds=None, noise=None):
    """Row b of sample_with_cond(n_steps=counts[b]) on the same full batch: one uniform call per distinct count."""
    host = _host()
    ref = torch.empty(cond_ct.shape[0], cond_ct.shape[2], model.config.n_mels, device=DEV)
    for n in sorted(set(counts)):
        nz = None if noise is None else noise[:1 if n == 1 else n + 1]
        full = host.sample_with_cond(model, cond_ct, spk, n, nz, factors=f, seeds=seeds)
        rows = torch.tensor([b for b, c in enumerate(counts) if c == n], device=DEV)
        ref[rows] = full[rows]
    return ref


def _nan_mel(model, cond_ct):
    return torch.full((cond_ct.shape[0], cond_ct.shape[2], model.config.n_mels), float("nan"), device=DEV)


# ----------------------------------------------------------------------------- 1. forms

@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
@pytest.mark.parametrize("with_factors", [False, True])
def test_forms(variant, with_factors, conv_form):
    """B = 40, T = 200: prefixes of 40 / 24 / 12 / 12 utterances of 4 tiles — the first evaluation takes the persistent stack, the later ones
    the per-layer kernels."""
    host, lib = _host(), _lib.load()
    B, T = 40, 200
    caller = np.random.RandomState(3).permutation([4] * 12 + [2] * 12 + [1] * 16)
    perm = S.order(caller)
    counts = [int(caller[k]) for k in perm]
    assert S.active(counts) == [40, 24, 12, 12] and sorted(perm.tolist()) == list(range(B)) and perm.tolist() != list(range(B))
    model, cond_ct, spk, f = _cond(variant, B, T, with_factors, 50, perm)
    seeds = N.utterance_seeds(31, np.arange(B))[perm]
    ref = _uniform_rows(model, cond_ct, spk, counts, f, seeds)
    mel = _nan_mel(model, cond_ct)
    got = host.sample_mixed(model, cond_ct, spk, counts, factors=f, seeds=seeds, out=mel)
    host.synchronize()
    assert got is mel and torch.isfinite(mel).all() and lib.cmtts_poll_error() == 0
    d = float((mel - ref).abs().max())
    report(f"MIXED forms {variant} factors={with_factors} {conv_form}: max|mixed - uniform| {d:.2e}")
    assert same_result(mel, ref, conv_form), d
    prev = model.set_option("batch_invariant", 1)
    try:
        ref_i = _uniform_rows(model, cond_ct, spk, counts, f, seeds)
        mel_i = _nan_mel(model, cond_ct)
        host.sample_mixed(model, cond_ct, spk, counts, factors=f, seeds=seeds, out=mel_i)
        host.synchronize()
    finally:
        model.set_option("batch_invariant", prev)
    assert torch.isfinite(mel_i).all() and lib.cmtts_poll_error() == 0
    assert torch.equal(mel_i, ref_i), float((mel_i - ref_i).abs().max())


# ----------------------------------------------------------------------------- 2. the persistent tail with tables

@pytest.mark.parametrize("mode", ["fp32-direct", "fp32-default", "bf16"])
def test_persistent_tail_tables_smallest(mode):
    """Every evaluation through the persistent stack: B = 5, T = 100 (two tiles, the last one partial), counts (4, 4, 2, 1, 1) — rows that
    re-noise, rows that do not, rows whose last evaluation writes the result, all in one launch."""
    host, lib = _host(), _lib.load()
    counts = [4, 4, 2, 1, 1]
    model, cond_ct, spk, _ = _cond("VCTK", 5, 100, False, 60)
    seeds = N.utterance_seeds(32, np.arange(5))
    prev_p = lib.cmtts_set_persistent_denoiser(2)
    prev_w = _lib.internal_set("persist_wino", 0) if mode == "fp32-direct" else None
    try:
        if mode == "bf16":
            model.set_precision("bf16")
        ref = _uniform_rows(model, cond_ct, spk, counts, None, seeds)
        mel = _nan_mel(model, cond_ct)
        host.sample_mixed(model, cond_ct, spk, counts, seeds=seeds, out=mel)
        rows = _lib.internal_sample_rows()
        host.synchronize()
    finally:
        if mode == "bf16":
            model.set_precision("fp32")
        if prev_w is not None:
            _lib.internal_set("persist_wino", prev_w)
        lib.cmtts_set_persistent_denoiser(prev_p)
    assert rows == sum(counts)
    assert torch.isfinite(mel).all() and lib.cmtts_poll_error() == 0
    assert torch.equal(mel, ref), float((mel - ref).abs().max())
    assert not torch.equal(mel[2], mel[0])


# ----------------------------------------------------------------------------- 3. chunked launch

def test_chunked_launch():
    """B = 70, T = 250: 280 tiles, two launches of 35 utterances; counts 36 x 2 then 34 x 1 put rows with different flags on both sides of
    the chunk boundary."""
    host, lib = _host(), _lib.load()
    B, T = 70, 250
    counts = [2] * 36 + [1] * 34
    model, cond_ct, spk, _ = _cond("LJSpeech", B, T, False, 70)
    seeds = N.utterance_seeds(33, np.arange(B))
    assert C.CDLL(_lib.LIB_PATH).cmtts_persist_chunks(B, T, 256) == 2          # csrc/persist_args.h: launches of one evaluation
    prev_w = _lib.internal_set("persist_wino", 0)
    try:
        ref = _uniform_rows(model, cond_ct, spk, counts, None, seeds)
        mel = _nan_mel(model, cond_ct)
        host.sample_mixed(model, cond_ct, spk, counts, seeds=seeds, out=mel)
        host.synchronize()
    finally:
        _lib.internal_set("persist_wino", prev_w)
    assert torch.isfinite(mel).all() and lib.cmtts_poll_error() == 0
    assert torch.equal(mel, ref), float((mel - ref).abs().max())


# ----------------------------------------------------------------------------- 4. per-utterance sigmas in one evaluation

def _sample_schedule(model, cond_ct, spk, noise, sig, std):
    """cmtts_sample on the full batch with one schedule's arrays."""
    lib = model.lib
    B, _, T = cond_ct.shape
    n = len(sig)
    a, d = (C.c_float * n)(*[float(v) for v in sig]), (C.c_float * n)(*[float(v) for v in std])
    mel = torch.empty(B, T, model.config.n_mels, device=DEV)
    nb = lib.cmtts_denoiser_workspace_bytes(model._h, B, T)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_sample(model._h, noise.data_ptr(), cond_ct.data_ptr(), spk.data_ptr() if spk is not None else None, B, T, n, a, d,
                                mel.data_ptr(), ws.data_ptr(), nb, _stream()))
    torch.cuda.synchronize()
    return mel


def test_per_utterance_sigmas():
    host, lib = _host(), _lib.load()
    variant, B, T = "VCTK", 4, 70
    model, cond_ct, spk, _ = _cond(variant, B, T, False, 80)
    cfg = model.config
    scheds = [R.schedule_from_ts(ts, 40, cfg.sigma_min, cfg.sigma_max, cfg.rho) for ts in TS]
    counts, sig, std = S.plan_from_schedules(scheds)
    noise = torch.randn(4, B, 1, T, cfg.n_mels, generator=torch.Generator().manual_seed(4)).to(DEV)
    prev_w = _lib.internal_set("persist_wino", 0)
    try:
        refs = [_sample_schedule(model, cond_ct, spk, noise, *sc) for sc in scheds]
        mel = _nan_mel(model, cond_ct)
        host.sample_mixed(model, cond_ct, spk, counts.tolist(), noise, sigmas=sig, renoise_std=std, out=mel)
        host.synchronize()
    finally:
        _lib.internal_set("persist_wino", prev_w)
    assert torch.isfinite(mel).all() and lib.cmtts_poll_error() == 0
    for b in range(B):
        assert torch.equal(mel[b], refs[b][b]), (b, float((mel[b] - refs[b][b]).abs().max()))
    assert not torch.equal(refs[0][0], refs[1][0])          # the schedules matter
    # one spot check against the float64 oracle: utterance 0 on its own schedule
    sd = {k: np.asarray(v) for k, v in _MODELS[(variant, None)][1].items()}
    cond = cond_ct[:1].transpose(1, 2).contiguous().cpu().numpy()
    with O.precision("f64"):
        ora = O.karras_sample_tts(sd, cfg, cond, spk[:1].cpu().numpy(), 3, list(noise[:, :1].cpu().numpy()), ts=TS[0], steps=40)
    e_mixed = float(np.abs(mel[0].cpu().numpy().astype(np.float64) - ora[0]).max())
    e_uniform = float(np.abs(refs[0][0].cpu().numpy().astype(np.float64) - ora[0]).max())
    report(f"MIXED sigmas ts={TS[0]}: max|mixed - float64| {e_mixed:.3e}, max|uniform - float64| {e_uniform:.3e}")
    assert e_mixed <= e_uniform          # direct form: the same bits, so the two measured numbers are equal


# ----------------------------------------------------------------------------- 5. explicit noise tensor

def test_noise_tensor():
    host, lib = _host(), _lib.load()
    B, T = 6, 64
    counts = [4, 2, 2, 1, 1, 1]
    model, cond_ct, spk, _ = _cond("VCTK", B, T, False, 90)
    noise = torch.randn(5, B, 1, T, model.config.n_mels, generator=torch.Generator().manual_seed(5)).to(DEV)
    prev_w = _lib.internal_set("persist_wino", 0)
    try:
        ref = _uniform_rows(model, cond_ct, spk, counts, None, None, noise)
        mel = _nan_mel(model, cond_ct)
        host.sample_with_cond(model, cond_ct, spk, counts, noise)          # the sequence form of the existing entry
        host.sample_mixed(model, cond_ct, spk, counts, noise, out=mel)
        host.synchronize()
    finally:
        _lib.internal_set("persist_wino", prev_w)
    assert torch.isfinite(mel).all() and lib.cmtts_poll_error() == 0
    assert torch.equal(mel, ref), float((mel - ref).abs().max())


# ----------------------------------------------------------------------------- 6. uniform plan, 7. work shrinks

def test_uniform_plan_is_the_seeded_sampler(conv_form):
    host = _host()
    B, T = 40, 200
    model, cond_ct, spk, _ = _cond("LJSpeech", B, T, False, 100)
    seeds = N.utterance_seeds(34, np.arange(B))
    ref = host.sample_with_cond(model, cond_ct, spk, 4, seeds=seeds).clone()
    rows_u = _lib.internal_sample_rows()
    got = host.sample_with_cond(model, cond_ct, spk, [4] * B, seeds=seeds).clone()
    rows_m = _lib.internal_sample_rows()
    host.synchronize()
    assert torch.isfinite(ref).all() and torch.equal(got, ref)
    assert rows_u == B * 4 and rows_m == B * 4


def test_work_shrinks():
    host = _host()
    B, T = 7, 40
    counts = [4, 4, 2, 2, 1, 1, 1]
    model, cond_ct, spk, _ = _cond("LJSpeech", B, T, False, 110)
    seeds = N.utterance_seeds(35, np.arange(B))
    host.sample_with_cond(model, cond_ct, spk, counts, seeds=seeds)
    assert _lib.internal_sample_rows() == sum(counts) == 15
    host.sample_with_cond(model, cond_ct, spk, 4, seeds=seeds)
    assert _lib.internal_sample_rows() == B * 4
    host.sample_with_cond(model, cond_ct, spk, 1, seeds=seeds)
    assert _lib.internal_sample_rows() == B
    host.synchronize()
    with pytest.raises(ValueError, match="steps.order"):
        host.sample_with_cond(model, cond_ct, spk, counts[::-1], seeds=seeds)
    with pytest.raises(ValueError):
        host.sample_with_cond(model, cond_ct, spk, counts[:-1], seeds=seeds)
    with pytest.raises(NotImplementedError):
        host.sample_ragged(model, [], counts)
    with pytest.raises(NotImplementedError):
        host.synthesize_sharded(model, torch.zeros(7, 4, dtype=torch.int64), torch.full((7,), 4), n_steps=counts)


# ----------------------------------------------------------------------------- 8. validation on a finalized model

def test_validation_leaves_mel_alone():
    lib = _lib.load()
    B, T = 3, 32
    model, cond_ct, spk, _ = _cond("VCTK", B, T, False, 120)
    cfg = model.config
    seeds = torch.from_numpy(N.utterance_seeds(36, np.arange(B))).to(DEV)
    noise = torch.randn(3, B, 1, T, cfg.n_mels, device=DEV)
    nb = lib.cmtts_sample_mixed_workspace_bytes(model._h, B, T, 2)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    mel = torch.full((B, T, cfg.n_mels), 7.0, device=DEV)
    sig0, std0 = S.default_plan([2, 2, 1], cfg.sigma_min, cfg.sigma_max, cfg.rho)

    def call(counts, sig=sig0, std=std0, sd=seeds, nz=None, nbytes=nb, speaker=spk):
        ns = np.asarray(counts, np.int32)
        plan = _lib.StepPlanStruct(2, ns.ctypes.data, np.ascontiguousarray(sig).ctypes.data, np.ascontiguousarray(std).ctypes.data)
        return lib.cmtts_sample_mixed(model._h, sd.data_ptr() if sd is not None else None, nz.data_ptr() if nz is not None else None,
                                      cond_ct.data_ptr(), speaker.data_ptr() if speaker is not None else None, B, T, C.byref(plan), mel.data_ptr(),
                                      ws.data_ptr(), nbytes, _stream(), None, None, 0, 0, None, None)

    assert call([1, 2, 2]) == -1 and b"max_steps" in lib.cmtts_last_error()
    assert call([2, 1, 2]) == -1 and b"steps.py" in lib.cmtts_last_error()          # increasing: the message names the remedy
    assert call([2, 2, 0]) == -1 and call([2, 2, 3]) == -1 and call([1, 1, 1]) == -1          # out of range; n_steps[0] != max_steps
    assert call([2, 2, 1], nz=noise) == -1 and call([2, 2, 1], sd=None) == -1          # both, neither
    mid = std0.copy()
    mid[0, 0] = -1.0
    assert call([2, 2, 1], std=mid) == -1 and b"last evaluation" in lib.cmtts_last_error()
    for v in (0.0, float("nan"), float("inf")):
        bs = sig0.copy()
        bs[1, 1] = v
        assert call([2, 2, 1], sig=bs) == -1
    assert call([2, 2, 1], speaker=None) == -1          # a multi-speaker model
    assert call([2, 2, 1], nbytes=nb - 1) == -4          # CMTTS_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((mel == 7.0).all())
    assert call([2, 2, 1]) == 0
    _host().synchronize()
    assert torch.isfinite(mel).all() and not bool((mel == 7.0).any())


# ----------------------------------------------------------------------------- 9. host surface

def _texts(cfg, seed, B=5, L=14):
    """Utterances of 14, 9, 12, 5, 11 phonemes; the models below give every phoneme 5 frames (T = 70, lengths 70, 45, 60, 25, 55)."""
    rs = np.random.RandomState(seed)
    src = np.asarray([L, 9, 12, 5, 11], np.int64)[:B]
    texts = np.zeros((B, L), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = torch.from_numpy(rs.standard_normal((B, cfg.external_speaker_dim)).astype(np.float32))
    return torch.from_numpy(texts), torch.from_numpy(src), spk


def test_synthesize_sequence_in_caller_order():
    host = _host()
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=2, dur_frames=5.0, dur_spread=0.0))
    texts, src, spk = _texts(cfg, 2)
    B = texts.shape[0]
    counts = [1, 4, 2, 4, 1]          # scrambled: steps.order gives (1, 3, 2, 0, 4)
    seeds = N.utterance_seeds(37, np.arange(B))
    batch = (None, None, None, texts, src, int(src.max()), spk)
    syn = host.CMTotalTTSSynthesize.from_model(model, T=4)
    prev_w = _lib.internal_set("persist_wino", 0)
    try:
        got = syn.synthesize(batch, seeds=seeds, n_steps=counts)
        uni = {n: host.CMTotalTTSSynthesize.from_model(model, T=n).synthesize(batch, seeds=seeds) for n in (1, 2, 4)}
        same = syn.synthesize(batch, seeds=seeds, n_steps=None)
        host.synchronize()
    finally:
        _lib.internal_set("persist_wino", prev_w)
    assert torch.equal(same[0], uni[4][0])
    assert torch.equal(torch.as_tensor(got[11]).cpu(), torch.as_tensor(uni[4][11]).cpu())          # lengths in the caller's order
    assert torch.equal(torch.as_tensor(got[10]).cpu(), src)
    assert torch.isfinite(got[0]).all()
    for b, n in enumerate(counts):
        assert torch.equal(got[0][b], uni[n][0][b]), (b, n, float((got[0][b] - uni[n][0][b]).abs().max()))
    assert not torch.equal(got[0][0], uni[4][0][0])
    with pytest.raises(ValueError):
        syn.synthesize(batch, seeds=seeds, n_steps=[1, 4, 3, 4, 1])


def test_synthesize_stream_sequence(voc_form):
    host = _host()
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=2, dur_frames=5.0, dur_spread=0.0))
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    texts, src, spk = _texts(cfg, 2, B=3)
    counts = [1, 4, 2]
    seeds = N.utterance_seeds(38, np.arange(3))
    batch = (None, None, None, texts, src, int(src.max()), spk)
    out = host.CMTotalTTSSynthesize.from_model(model, T=4).synthesize(batch, seeds=seeds, n_steps=counts)
    mel, lens = out[0], [int(v) for v in torch.as_tensor(out[11]).cpu().tolist()]
    ref = host.vocoder_infer(mel.transpose(1, 2), voc, lengths=[n * HOP for n in lens])
    chunks = {b: [] for b in range(3)}
    for b, off, pcm, last in host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=counts, seeds=seeds, chunk_frames=(8, 16)):
        assert off == sum(len(c) for c in chunks[b]) and pcm.dtype == np.int16
        chunks[b].append(pcm)
    host.synchronize()
    for b in range(3):
        got = np.concatenate(chunks[b])
        assert len(got) == lens[b] * HOP
        assert same_pcm(got, np.asarray(ref[b]), voc_form), b
