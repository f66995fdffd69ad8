"""Streamed PCM (windowed HiFi-GAN vocoding, include/cmtts_hip.h: cmtts_vocoder_forward_windows; host.vocoder_infer_stream,
host.synthesize_stream): the window gather and the windowed conv_post / int16 tail bitwise against their whole-mel counterparts,
stitched window cores against the one-shot vocoder in every form, text -> streamed PCM end to end, and argument validation."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd.config import HifiGanConfig, get_config
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict
from conftest import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = HifiGanConfig().hop


def _host():
    from cmtts_amd import host
    return host


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _voc(seed=3, **over):
    hcfg = HifiGanConfig()
    hsd = synth_hifigan_state_dict(hcfg, seed=seed)
    for k, v in over.items():
        hsd[k] = np.full_like(hsd[k], v)
    return _host().Generator(hcfg, DEV).load_state_dict(hsd), hsd, hcfg


def _mels(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 80, T, generator=g) * 0.8 - 1.0).to(DEV)


def _forward_windows(voc, mel, windows, Tw, core, max_wav=32768.0):
    """cmtts_vocoder_forward_windows with a DEVICE table -> int16 [N, core * hop] on the device."""
    lib = voc.lib
    B, _, T = mel.shape
    tab = torch.tensor(windows, dtype=torch.int32, device=DEV)
    N = len(windows)
    pcm = torch.empty(N, core * HOP, dtype=torch.int16, device=DEV)
    nb = lib.cmtts_vocoder_windows_workspace_bytes(voc._h, N, Tw)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_vocoder_forward_windows(voc._h, mel.data_ptr(), B, T, tab.data_ptr(), N, Tw, core, pcm.data_ptr(), max_wav,
                                                 ws.data_ptr(), nb, _stream()))
    return pcm


def _stitch(stream_iter, lens):
    """(utterance, sample_offset, pcm, is_last) chunks -> one array per utterance; checks order, offsets and is_last."""
    out = [[] for _ in lens]
    pos = [0] * len(lens)
    done = [False] * len(lens)
    first = {}
    for b, off, pcm, last in stream_iter:
        assert not done[b] and off == pos[b] and pcm.dtype == np.int16
        first.setdefault(b, (len(pcm), last))
        out[b].append(pcm)
        pos[b] += len(pcm)
        done[b] = last
        assert last == (pos[b] == lens[b] * HOP)
    assert all(done[b] for b in range(len(lens)) if lens[b] > 0)
    return [np.concatenate(o) if o else np.zeros(0, np.int16) for o in out], first


def _whole(voc, mel, lens):
    return _host().vocoder_infer(mel, voc, lengths=[n * HOP for n in lens])


def test_mel_window_gather_bitwise():
    mel = torch.randn(3, 80, 40, device=DEV)
    cases = [(16, [(0, 0, 0, 4), (1, 4, 0, 4), (2, 24, 0, 4), (1, 8, 2, 3)]),     # 16-byte rows
             (21, [(2, 19, 0, 1), (0, 3, 0, 1), (1, 0, 0, 1)]),                   # dword copies, odd width
             (40, [(0, 0, 0, 1), (2, 0, 0, 1)])]                                  # whole tensor
    for Tw, win in cases:
        tab = torch.tensor(win, dtype=torch.int32, device=DEV)
        out = torch.full((len(win), 80, Tw), float("nan"), device=DEV)
        _lib.check(C.CDLL(_lib.LIB_PATH).cmtts_internal_mel_window_gather(
            C.c_void_p(mel.data_ptr()), 3, 40, C.c_void_p(tab.data_ptr()), len(win), Tw, C.c_void_p(out.data_ptr()), _stream()))
        ref = torch.stack([mel[b, :, s:s + Tw] for b, s, _, _ in win])
        torch.cuda.synchronize()
        assert torch.equal(out, ref), Tw
    mel2 = torch.randn(2, 80, 33, device=DEV)[:, :, :32].contiguous()             # T % 4 == 0: aligned starts take float4
    tab = torch.tensor([(1, 4, 0, 1), (0, 8, 0, 1), (1, 5, 0, 1)], dtype=torch.int32, device=DEV)
    out = torch.empty(3, 80, 24, device=DEV)
    _lib.check(C.CDLL(_lib.LIB_PATH).cmtts_internal_mel_window_gather(C.c_void_p(mel2.data_ptr()), 2, 32, C.c_void_p(tab.data_ptr()), 3, 24,
                                                                      C.c_void_p(out.data_ptr()), _stream()))
    assert torch.equal(out, torch.stack([mel2[1, :, 4:28], mel2[0, :, 8:32], mel2[1, :, 5:29]]))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_conv_post_windows_bitwise(precision):
    """Whole-tensor windows (the generator sees exactly the whole mel batch): the windowed tail must equal conv_post + tanh
    followed by cmtts_wav_to_int16 on the same columns, zeros after a short core."""
    voc, _, _ = _voc()
    voc.set_precision(precision)
    B, T = 2, 24
    mel = _mels(B, T, 1)
    whole = _host().vocoder_infer_device(mel, voc)
    core = 11
    win = [(0, 0, 5, 11), (1, 0, 13, 7)]
    pcm = _forward_windows(voc, mel, win, T, core)
    torch.cuda.synchronize()
    for n, (b, s, off, cl) in enumerate(win):
        assert torch.equal(pcm[n, : cl * HOP], whole[b, off * HOP:(off + cl) * HOP]), n
        assert not pcm[n, cl * HOP:].any()
    # +1.0 wraps to -32768: a conv_post bias that saturates tanh
    voc2, _, _ = _voc(**{"conv_post.bias": 20.0})
    whole2 = _host().vocoder_infer_device(mel, voc2)
    pcm2 = _forward_windows(voc2, mel, [(1, 0, 3, 9)], T, 9)
    torch.cuda.synchronize()
    assert (whole2 == -32768).all() and torch.equal(pcm2[0], whole2[1, 3 * HOP:12 * HOP])


DIRECT_CASES = [  # (B, T, lens, chunk_frames)
    (3, 200, [200, 151, 1], (32, 64, 128, 256)),
    (2, 37, [37, 20], (32, 64, 128, 256)),         # odd T; Tw > T: one whole-tensor window
    (3, 90, [90, 61, 30], (30, 14)),               # cores not divisible by 4, edges clamped at 0 and T
    (2, 64, [64, 47], (5, 9, 13)),
]


@pytest.mark.parametrize("B,T,lens,chunks", DIRECT_CASES)
def test_stream_fp32_direct_bitwise(B, T, lens, chunks):
    voc, _, _ = _voc()
    assert voc.set_option("winograd", 0) == 1
    mel = _mels(B, T, T)
    ref = _whole(voc, mel, lens)
    got, first = _stitch(_host().vocoder_infer_stream(mel, voc, lens, chunks), lens)
    for b in range(B):
        assert np.array_equal(got[b], ref[b]), f"utterance {b}: {np.count_nonzero(got[b] != ref[b])} samples differ"
    for b, (n0, last) in first.items():
        assert last == (lens[b] * HOP == n0)


def test_stream_fp32_default_forms():
    """The default (Winograd-capable) forms: the window batch and the whole batch may take different conv forms, and a dilated
    conv's Winograd quads sit at another phase in a window; within the vocoder's existing tolerance (<= 1 LSB, few samples)."""
    voc, _, _ = _voc()
    B, T = 32, 512
    g = torch.Generator().manual_seed(7)
    lens = [T] + torch.randint(200, T + 1, (B - 1,), generator=g).tolist()
    mel = _mels(B, T, 11)
    ref = _whole(voc, mel, lens)
    got, _ = _stitch(_host().vocoder_infer_stream(mel, voc, lens), lens)
    d = np.concatenate([np.abs(got[b].astype(np.int32) - ref[b]) for b in range(B)])
    report(f"STREAM fp32 default forms, 32 x 512: {np.count_nonzero(d)} of {d.size} samples differ, max {d.max()} LSB")
    # the forms differ by <= 1.4e-6 on the waveform (include/cmtts_hip.h, "winograd"), ~0.05 LSB: a truncation toward zero flips
    # only where a sample sits that close to an integer (measured on MI355X: 5262 of 3041024, 0.17 %)
    assert d.max() <= 1 and np.count_nonzero(d) <= 1e-2 * d.size


def test_stream_bf16_against_whole_and_oracle():
    from oracle import cmtts_oracle as O
    voc, hsd, hcfg = _voc()
    voc.set_precision("bf16")
    B, T, lens = 2, 64, [64, 45]
    mel = _mels(B, T, 5)
    ref = _whole(voc, mel, lens)
    got, _ = _stitch(_host().vocoder_infer_stream(mel, voc, lens, (8, 16)), lens)
    with O.operands16("bf16"):
        orc = O.wav_to_int16(O.hifigan_generator(hsd, hcfg, mel.cpu().numpy())[:, 0])
    d_sw = max(int(np.abs(got[b].astype(np.int32) - ref[b]).max()) for b in range(B))
    e_s = max(int(np.abs(got[b].astype(np.int32) - orc[b, : lens[b] * HOP]).max()) for b in range(B))
    e_w = max(int(np.abs(ref[b].astype(np.int32) - orc[b, : lens[b] * HOP]).max()) for b in range(B))
    report(f"STREAM bf16: stitched vs whole max {d_sw} LSB; vs the bf16-operand oracle: stitched {e_s}, whole {e_w} LSB")
    assert d_sw <= max(2 * e_w, 4)
    assert e_s <= 1.5 * e_w + 2


def _e2e(voc, chunks, seed=2):
    host = _host()
    cfg = get_config("VCTK")
    sd = synth_cmtts_state_dict(cfg, seed=seed, dur_frames=5.0, dur_spread=0.3)
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(sd)
    rs = np.random.RandomState(seed)
    B, L = 3, 14
    src = np.asarray([L, 9, 5], np.int64)
    texts = np.zeros((B, L), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = torch.from_numpy(rs.standard_normal((B, cfg.external_speaker_dim)).astype(np.float32))
    texts, src = torch.from_numpy(texts), torch.from_numpy(src)
    out = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk)
    T = out["cond"].shape[1]
    noise = torch.randn(5, B, 1, T, cfg.n_mels, generator=torch.Generator().manual_seed(seed)).to(DEV)
    mel = host.sample_with_cond(model, out["cond_ct"], out["speaker_emb"], 4, noise, factors=out.get("cond_factors"))
    lens = out["mel_lens"].cpu().tolist()
    ref = host.vocoder_infer(mel.transpose(1, 2), voc, lengths=[n * HOP for n in lens])
    got, first = _stitch(host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=4, noise=noise, chunk_frames=chunks), lens)
    return got, ref, lens, first


def test_synthesize_stream_end_to_end():
    voc, _, _ = _voc()
    voc.set_option("winograd", 0)
    got, ref, lens, first = _e2e(voc, (8, 16))
    assert max(lens) > 8
    for b in range(len(lens)):
        assert np.array_equal(got[b], ref[b]), b
        if lens[b] > 8:
            assert first[b] == (8 * HOP, False), "the first round's chunk is not the last one"
    voc.set_option("winograd", 1)
    got, ref, lens, _ = _e2e(voc, (8, 16))
    d = max(int(np.abs(got[b].astype(np.int32) - ref[b]).max()) for b in range(len(lens)))
    assert d <= 1


def test_forward_windows_argument_validation():
    voc, _, _ = _voc()
    lib = voc.lib
    B, T, Tw, core = 2, 40, 30, 4
    mel = _mels(B, T, 3)
    N = 2
    nb = lib.cmtts_vocoder_windows_workspace_bytes(voc._h, N, Tw)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    pcm = torch.full((N, core * HOP), 0x5A5A, dtype=torch.int16, device=DEV)
    good = [(0, 0, 0, 4), (1, 10, 13, 4)]

    def call(win=good, mel_p=mel.data_ptr(), Bc=B, Tc=T, Nc=N, Twc=Tw, corec=core, pcm_p=pcm.data_ptr(), ws_p=ws.data_ptr(), nbc=nb, handle=voc._h):
        tab = torch.tensor(win, dtype=torch.int32, device=DEV) if win is not None else None
        return lib.cmtts_vocoder_forward_windows(handle, mel_p, Bc, Tc, None if tab is None else tab.data_ptr(), Nc, Twc, corec, pcm_p, 32768.0,
                                                 ws_p, nbc, _stream())

    bad = {
        "null vocoder": call(handle=None), "null mel": call(mel_p=None), "null table": call(win=None), "null pcm": call(pcm_p=None),
        "null ws": call(ws_p=None), "N = 0": call(Nc=0), "N < 0": call(Nc=-1), "Tw > T": call(Twc=T + 1), "core 0": call(corec=0),
        "window past T": call(win=[(0, 11, 0, 4), (1, 0, 0, 4)]), "negative start": call(win=[(0, -1, 1, 4), (1, 0, 0, 4)]),
        "utterance >= B": call(win=[(2, 0, 0, 4), (1, 0, 0, 4)]), "core_off + core_len > Tw": call(win=[(0, 0, 27, 4), (1, 0, 0, 4)]),
        "core_len > core": call(win=[(0, 0, 0, 5), (1, 0, 0, 4)]), "core_len 0": call(win=[(0, 0, 0, 0), (1, 0, 0, 4)]),
        "short workspace": call(nbc=nb - 1),
    }
    torch.cuda.synchronize()
    for what, rc in bad.items():
        assert rc < 0, what
        if what != "short workspace":
            assert rc == -1, what
    assert lib.cmtts_vocoder_forward_windows(voc._h, mel.data_ptr(), B, T, (C.c_int32 * 8)(*[0] * 8), N, Tw, core, pcm.data_ptr(), 32768.0,
                                             ws.data_ptr(), nb, _stream()) == -1, "pageable host table"
    torch.cuda.synchronize()
    assert (pcm == 0x5A5A).all(), "a rejected call wrote the output"
    assert call() == 0
    torch.cuda.synchronize()
    assert not (pcm == 0x5A5A).all()
