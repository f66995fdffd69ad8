"""Recorded speech in on the GPU (include/cmtts_hip.h: cmtts_mel_analysis, cmtts_phoneme_energy, cmtts_pcm_crossfade; csrc/mel_analysis.hip;
host.mel_from_audio / energy_targets / retake_recording_pcm): mel and energy against the float64 definition with the
definition's own float32 arm as the yardstick, the exact cases (silence, batch, input type, layout), phoneme energy, copy synthesis and the
retake of a recording end to end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cmtts_amd import _lib, analysis as A, noise as N
from cmtts_amd.config import get_config, HifiGanConfig
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict
from conftest import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = 256
LENGTHS = {"reference": (513, 1809, 4000), "vocoder": (385, 1809, 4000)}

# The bound of test_mel_and_energy_against_float64.  Yardstick: analysis.mel_from_audio(dtype=float32) — numpy's float32 FFT, matrix product and
# sums — against its float64 arm on the inputs of _signal(), worst over both pad modes and the three lengths (measured with numpy 2.2: 6.54e-6 on
# the log-mel at (reference, 4000), 8.68e-8 relative on the energy at (reference, 1809); the test prints the live figures).  The kernel gets 4 x
# that: its radix-2 FFT, split step and sparse sums associate differently from numpy's.
YARDSTICK_MEL, YARDSTICK_ENERGY = 6.6e-6, 8.7e-8
BOUND_MEL, BOUND_ENERGY = 4 * YARDSTICK_MEL, 4 * YARDSTICK_ENERGY
# cmtts_phoneme_energy accumulates in double and rounds (m - mean) / std to float once: one rounding of the result, plus what the float
# energies' exact double sum loses against the definition's (nothing visible).  Allowed: 2 float32 ulps of max(|m|, |mean|) / std.
PHONEME_ULPS = 2

_CACHE = {}


def _host():
    from cmtts_amd import host
    return host


def _an():
    if "an" not in _CACHE:
        _CACHE["an"] = _host().get_analyzer(device=DEV)
    return _CACHE["an"]


def _voc():
    if "voc" not in _CACHE:
        hcfg = HifiGanConfig()
        _CACHE["voc"] = _host().Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    return _CACHE["voc"]


def _model():
    if "model" not in _CACHE:
        cfg = get_config("VCTK")
        _CACHE["model"] = _host().CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=5))
    return _CACHE["model"]


def _signal(n, seed):
    """Four sinusoids and white noise 30 dB under them: every mel channel of every frame stays far above the 1e-5 clamp."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 22050.0
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in [(0.25, 220.0, 0.3), (0.2, 1330.0, 1.1), (0.15, 3900.0, 2.0), (0.1, 7100.0, 0.5)])
    x = x + rs.standard_normal(n) * (np.sqrt((x ** 2).mean()) * 10 ** (-30 / 20))
    return x.astype(np.float32)


def _batch(pad):
    """(wavs [3, 4000] float32, lengths, the float64 definition) — computed once, shared, never written."""
    if pad not in _CACHE:
        lens = LENGTHS[pad]
        wavs = np.zeros((3, max(lens)), np.float32)
        for b, n in enumerate(lens):
            wavs[b, :n] = _signal(n, b)
        _CACHE[pad] = (wavs, list(lens), A.mel_from_audio(wavs, lens, pad))
    return _CACHE[pad]


def _valid(lens, T):
    return np.arange(T)[None, :] < np.asarray(lens)[:, None]


# ----------------------------------------------------------------------------- 1. against the definition

@pytest.mark.parametrize("pad", ["reference", "vocoder"])
def test_mel_and_energy_against_float64(pad):
    host = _host()
    wavs, lens, ref = _batch(pad)
    T = ref["mel"].shape[1]
    ok = _valid(ref["mel_lens"], T)
    assert list(ref["mel_lens"]) == [A.frame_count(n, pad) for n in lens] and T == max(ref["mel_lens"])
    assert ref["mel"][ok].min() > math.log(1e-5) + 3.0        # no cell near the clamp: the bound below is never met trivially
    f32 = A.mel_from_audio(wavs, lens, pad, dtype=np.float32)
    y_mel = float(np.abs(f32["mel"].astype(np.float64) - ref["mel"])[ok].max())
    y_en = float((np.abs(f32["energy"].astype(np.float64) - ref["energy"])[ok] / ref["energy"][ok]).max())
    got = host.mel_from_audio(_an(), wavs, lens, pad=pad)
    mel, energy = got["mel"].cpu().numpy().astype(np.float64), got["energy"].cpu().numpy().astype(np.float64)
    e_mel = float(np.abs(mel - ref["mel"])[ok].max())
    e_en = float((np.abs(energy - ref["energy"])[ok] / ref["energy"][ok]).max())
    report(f"ANALYSIS {pad}: max|mel - f64| kernel {e_mel:.2e}, numpy float32 {y_mel:.2e} (bound {BOUND_MEL:.2e}); "
           f"energy rel. kernel {e_en:.2e}, numpy float32 {y_en:.2e} (bound {BOUND_ENERGY:.2e})")
    assert got["mel"].shape == (3, T, 80) and got["energy"].shape == (3, T) and got["mel_lens"].dtype == torch.int64
    assert got["mel_lens"].cpu().tolist() == list(ref["mel_lens"])
    assert not mel[~ok].any() and not energy[~ok].any()
    assert e_mel <= BOUND_MEL and e_en <= BOUND_ENERGY, (e_mel, e_en)


# ----------------------------------------------------------------------------- 2. the exact cases

@pytest.mark.parametrize("pad", ["reference", "vocoder"])
def test_silence(pad):
    host = _host()
    lens = [3000, 1000]
    got = host.mel_from_audio(_an(), np.zeros((2, 3000), np.float32), lens, pad=pad)
    F = [A.frame_count(n, pad) for n in lens]
    ok = torch.from_numpy(_valid(F, max(F))).to(DEV)
    floor = torch.tensor(np.float32(np.log(1e-5)), device=DEV)
    assert got["mel_lens"].cpu().tolist() == F
    assert torch.equal(got["mel"][ok], floor.expand(int(ok.sum()), 80))
    assert torch.equal(got["mel"][~ok], torch.zeros(int((~ok).sum()), 80, device=DEV))
    assert torch.equal(got["energy"], torch.zeros(2, max(F), device=DEV))


@pytest.mark.parametrize("pad", ["reference", "vocoder"])
def test_batch_independence_input_type_and_layout(pad):
    host, an = _host(), _an()
    wavs, lens, _ = _batch(pad)
    full = host.mel_from_audio(an, wavs, lens, pad=pad)
    for b, n in enumerate(lens):
        alone = host.mel_from_audio(an, wavs[b:b + 1, :n].copy(), pad=pad)
        F = A.frame_count(n, pad)
        assert alone["mel"].shape == (1, F, 80)
        assert torch.equal(alone["mel"][0], full["mel"][b, :F]) and torch.equal(alone["energy"][0], full["energy"][b, :F]), b
    # the two layouts hold the same bits
    ct = host.mel_from_audio(an, wavs, lens, pad=pad, layout="ct")
    assert ct["mel"].shape == (3, 80, full["mel"].shape[1])
    assert torch.equal(ct["mel"].transpose(1, 2), full["mel"]) and torch.equal(ct["energy"], full["energy"])
    # int16 against the same samples as float (x / 32768 is exact); a list of rows against the padded matrix
    pcm = np.round(wavs * 30000.0).astype(np.int16)
    as_int = host.mel_from_audio(an, pcm, lens, pad=pad)
    as_float = host.mel_from_audio(an, pcm.astype(np.float32) / np.float32(32768.0), lens, pad=pad)
    as_list = host.mel_from_audio(an, [pcm[b, :n] for b, n in enumerate(lens)], pad=pad)
    for k in ("mel", "energy", "mel_lens"):
        assert torch.equal(as_int[k], as_float[k]) and torch.equal(as_int[k], as_list[k]), k
    # float input is clipped to [-1, 1]
    loud = host.mel_from_audio(an, wavs * 40.0, lens, pad=pad)
    clipped = host.mel_from_audio(an, np.clip(wavs * 40.0, -1.0, 1.0), lens, pad=pad)
    assert torch.equal(loud["mel"], clipped["mel"])


# ----------------------------------------------------------------------------- 3. phoneme energy

def test_phoneme_energy_and_energy_targets():
    host, an = _host(), _an()
    wavs = np.stack([_signal(20 * HOP, 11) * np.linspace(0.2, 1.0, 20 * HOP, dtype=np.float32), _signal(20 * HOP, 12)])
    feat = host.mel_from_audio(an, wavs, [20 * HOP, 15 * HOP])
    energy = feat["energy"]
    assert feat["mel_lens"].cpu().tolist() == [21, 16]
    d = np.asarray([[3, 0, 2, 5, 0, 1, 1, 4, 2, 2], [2, 2, 0, 7, 1, 0, 3, 0, 0, 0]], np.int64)
    mean, std = 21.7, 9.3
    e = host.energy_targets(an, energy, torch.from_numpy(d), mean, std)
    assert e.shape == (2, 10) and e.dtype == torch.float32 and e.is_cuda
    en = energy.cpu().numpy()

    def close(got, durations):
        ref = A.phoneme_energy(en, durations, mean, std)
        m = ref * std + mean
        tol = PHONEME_ULPS * np.finfo(np.float32).eps * np.maximum(np.abs(m), abs(mean)) / std
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        assert (err <= tol).all(), (err / tol).max()
        return m

    m = close(e, d)
    assert float(e[0, 1]) == np.float32((0.0 - mean) / std) and (m[0, [0, 2, 3]] > 0).all()
    # durations that run past T: frames beyond count as zero
    long = d.copy()
    long[0, 9] = 50
    e2 = host.energy_targets(an, energy, long, mean, std)
    close(e2, long)
    assert torch.equal(e2[1], e[1]) and not torch.equal(e2[0, 9], e[0, 9])
    # accepted unchanged as e_targets=: the same conditioning as the same numbers handed over from the host
    model = _model()
    cfg = model.config
    rs = np.random.RandomState(4)
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(2, 10)).astype(np.int64))
    texts[1, 7:] = 0
    src = torch.tensor([10, 7])
    spk = torch.from_numpy(rs.standard_normal(size=(2, cfg.external_speaker_dim)).astype(np.float32))
    dt = torch.from_numpy(d.astype(np.float32))
    a = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, d_targets=dt, e_targets=e)
    a = {k: a[k].clone() for k in ("cond_ct", "mel_lens")}
    b = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, d_targets=dt, e_targets=torch.from_numpy(e.cpu().numpy()))
    assert a["mel_lens"].cpu().tolist() == [20, 15] and torch.equal(a["cond_ct"], b["cond_ct"])
    c = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, d_targets=dt)
    assert not torch.equal(a["cond_ct"], c["cond_ct"])        # the targets were used


# ----------------------------------------------------------------------------- 4. copy synthesis

def test_copy_synthesis():
    host = _host()
    lens = [16 * HOP + 100, 11 * HOP]
    wavs = np.zeros((2, lens[0]), np.float32)
    for b, n in enumerate(lens):
        wavs[b, :n] = _signal(n, 20 + b)
    feat = host.mel_from_audio(_an(), wavs, lens, pad="vocoder", layout="ct")
    frames = feat["mel_lens"].cpu().tolist()
    assert frames == [16, 11] and feat["mel"].shape == (2, 80, 16)
    out = host.vocoder_infer(feat["mel"], _voc(), lengths=[f * HOP for f in frames])
    assert [w.shape for w in out] == [(16 * HOP,), (11 * HOP,)] and all(w.dtype == np.int16 for w in out)
    assert all(np.abs(w.astype(np.int32)).max() > 0 for w in out)


# ----------------------------------------------------------------------------- 5. a retake of a recording

def _whole_f32(voc, mel_ct):
    """cmtts_vocoder_forward_windows_f32 on one whole-utterance window per row: fp32 [B, T * hop]."""
    lib = voc.lib
    B, _, T = mel_ct.shape
    tab = torch.tensor([(b, 0, 0, T) for b in range(B)], dtype=torch.int32, device=DEV)
    rows = torch.empty(B, T * HOP, dtype=torch.float32, device=DEV)
    nb = lib.cmtts_vocoder_windows_workspace_bytes(voc._h, B, T)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.cmtts_vocoder_forward_windows_f32(voc._h, p(mel_ct), B, T, p(tab), B, T, T, 0, p(rows), p(ws), nb, st))
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def test_retake_of_a_recording():
    host, an, model, voc = _host(), _an(), _model(), _voc()
    cfg = model.config
    T = 40
    lens = [39 * HOP + 100, 33 * HOP + 17]
    rec = [np.round(_signal(n, 30 + b) * 30000.0).astype(np.int16) for b, n in enumerate(lens)]
    feat = host.mel_from_audio(an, rec)
    mel_rec = feat["mel"]
    assert mel_rec.shape == (2, T, 80) and feat["mel_lens"].cpu().tolist() == [40, 34]
    g = torch.Generator().manual_seed(6)
    cond_ct = torch.randn(2, cfg.hidden, T, generator=g).to(DEV)
    spk = torch.randn(2, cfg.hidden, generator=g).to(DEV)
    spans = [(0, 0, 5), (0, 20, 26), (1, 10, 14), (1, 30, 33)]
    new = host.retake(model, mel_rec, cond_ct, spk, spans, N.utterance_seeds(9, np.arange(2)), n_steps=2).clone()
    inside = np.zeros((2, T), bool)
    for b, lo, hi in spans:
        inside[b, lo:hi] = True
    keep = torch.from_numpy(~inside).to(DEV)
    assert torch.equal(new[keep], mel_rec[keep]) and not torch.equal(new[~keep], mel_rec[~keep])
    mel_ct = new.transpose(1, 2).contiguous()
    prev = _lib.internal_set("voc_wino", 0)                   # the direct conv form: windows are bit for bit the whole utterance
    try:
        wav = _whole_f32(voc, mel_ct)
        got1 = host.retake_recording_pcm(mel_ct, voc, rec, spans, xfade_frames=1)
        # fades that touch merge their spans: (0, 8, 10) and (0, 14, 16) at X = 3 are one span [8, 16)
        got3 = host.retake_recording_pcm(mel_ct, voc, rec, [(0, 8, 10), (0, 14, 16)], xfade_frames=3)
        got0 = host.retake_recording_pcm(mel_ct, voc, rec, [(1, 30, 33)], xfade_frames=0)
    finally:
        _lib.internal_set("voc_wino", prev)

    def check(got, merged, X):
        want = [r.copy() for r in rec]
        touched = [np.zeros(len(r), bool) for r in rec]
        core = [np.zeros(len(r), bool) for r in rec]
        for b, lo, hi in merged:
            want[b] = A.crossfade_splice(want[b], wav[b], lo, hi, X)
            touched[b][max(lo - X, 0) * HOP:(hi + X) * HOP] = True
            core[b][lo * HOP:hi * HOP] = True
        for b in range(2):
            assert got[b].dtype == np.int16 and got[b].shape == rec[b].shape
            assert np.array_equal(got[b][~touched[b]], rec[b][~touched[b]]), b
            pcm = np.clip(np.rint(wav[b][:len(rec[b])].astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
            assert np.array_equal(got[b][core[b]], pcm[core[b]]), b
            assert np.abs(got[b].astype(np.int32) - want[b].astype(np.int32)).max() <= 1, b

    check(got1, spans, 1)
    check(got3, [(0, 8, 16)], 3)
    check(got0, [(1, 30, 33)], 0)
    # a span that touches frame 0 has no leading fade (there is nothing before it); one whose fade would pass the end has no trailing fade
    assert np.array_equal(got1[1][33 * HOP:], rec[1][33 * HOP:])
    assert not np.array_equal(got1[0][5 * HOP:6 * HOP], rec[0][5 * HOP:6 * HOP])          # the trailing fade of (0, 0, 5)
    assert not np.array_equal(got1[1][9 * HOP:10 * HOP], rec[1][9 * HOP:10 * HOP])        # the leading fade of (1, 10, 14)
    assert np.array_equal(got3[1], rec[1])
    with pytest.raises(ValueError):
        host.retake_recording_pcm(mel_ct, voc, rec, [(0, 38, 41)])
    with pytest.raises(ValueError):
        host.retake_recording_pcm(mel_ct, voc, rec, spans, xfade_frames=-1)
