"""Speaker embeddings from reference audio on the device (include/cmtts_hip.h: cmtts_spkenc_*; host.speaker_embedding): the Conv2D kernel
alone, the trim, the fbank and the whole path against the float64 definition (cmtts_amd/speaker.py), batch independence, the embedding as
spker_embeds= end to end, and the invalid-argument paths of the C ABI.

Tolerances are not fixed numbers: each comparison runs the same computation in float32 on the CPU (torch for the conv, the numpy definition
elsewhere) and takes ITS error against float64 as the yardstick; the kernel's error must be <= 4 x that."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import speaker as sp
from conftest import report
from speaker_cases import (CONV_CASES, FRAME_LEN, FRAME_STEP, FS, conv_case, conv_float32, fbank_signals, reference_embeddings, trim_signals,
                           utterances, weights)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GARBAGE = 1.0e30
RULE = 4.0


@pytest.fixture(autouse=True, scope="module")
def _symbols():
    if not hasattr(C.CDLL(_lib.LIB_PATH), "cmtts_spkenc_forward"):
        pytest.skip("this libcmtts_hip.so has no speaker encoder (cmtts_spkenc_*)")


def _host():
    from cmtts_amd import host
    return host


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def enc():
    return _host().get_speaker_encoder(weights(), DEV)


def _rows(xs, pad=37):
    """rows xs -> (device [rows, ld] with GARBAGE behind every row's samples, lengths)."""
    ld = max(len(x) for x in xs) + pad
    buf = np.full((len(xs), ld), GARBAGE, np.float32)
    for i, x in enumerate(xs):
        buf[i, :len(x)] = x
    return torch.from_numpy(buf).to(DEV), [len(x) for x in xs]


# ---------------------------------------------------------------------------------------------------- a. the conv kernel alone

@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_kernel_against_float64(name):
    k, s, cin, cout, H, W, B, residual = CONV_CASES[name]
    x, kernel, bias, res, want = conv_case(name)
    assert (want == 0).any() and (want == 20).any(), "the expected output must sit on both clips"
    frag, b = _lib.internal_spkenc_pack(kernel, bias, None)
    xd, fd, bd = (torch.from_numpy(v).to(DEV) for v in (x, frag, b))
    rd = None if res is None else torch.from_numpy(res).to(DEV)
    y = torch.full(want.shape, float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.internal_spkenc_conv(xd.data_ptr(), fd.data_ptr(), bd.data_ptr(), None if rd is None else rd.data_ptr(), B, H, W, cin, cout, k, s,
                                         y.data_ptr(), _stream()))
    got = y.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    yard = float(np.abs(conv_float32(name).astype(np.float64) - want).max())
    report(f"SPEAKER conv ({name}) k{k}/s{s} {cin}->{cout} {H}x{W} B={B}: max error {err:.3e}, torch CPU float32 {yard:.3e}, ratio {err / yard:.2f}")
    assert np.isfinite(got).all() and err <= RULE * yard


@pytest.mark.parametrize("name,big", [("f", 64), ("c", 1400)])
def test_conv_bits_do_not_depend_on_the_launch_size(name, big):
    """Image 0 of a large launch has the bits of the batch of one (the instance, and with it the K split, follows (cin, cout) alone): 64 and 1400
    images reach 2560 and 8400 pixels, many workgroups and a last, partly filled tile."""
    k, s, cin, cout, H, W, B, residual = CONV_CASES[name]
    x, kernel, bias, _, want = conv_case(name)
    frag, b = _lib.internal_spkenc_pack(kernel, bias, None)
    fd, bd = torch.from_numpy(frag).to(DEV), torch.from_numpy(b).to(DEV)
    outs = []
    for n in (1, big // 2, big):
        xs = torch.from_numpy(x[:1]).to(DEV).repeat(n, 1, 1, 1)
        xs[1:] *= 0.5
        y = torch.full((n,) + want.shape[1:], float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(_lib.internal_spkenc_conv(xs.data_ptr(), fd.data_ptr(), bd.data_ptr(), None, n, H, W, cin, cout, k, s, y.data_ptr(), _stream()))
        outs.append(y)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[2][0]) and bool(torch.isfinite(outs[2]).all())
    assert torch.equal(outs[2][1], outs[2][big - 1])


# ---------------------------------------------------------------------------------------------------- b. batch independence

def test_window_does_not_depend_on_the_batch(enc):
    host = _host()
    win, info = host.speaker_features(enc, list(utterances()))
    assert win.shape == (3, 160, 64) and info[:, 3].tolist() == [1, 1, 1]
    three = host.speaker_forward(enc, win, [0, 1, 2], 3)
    one = host.speaker_forward(enc, win[:1].clone(), [0], 1)
    assert torch.equal(three[0], one[0])
    assert not torch.equal(three[0], three[1])


# ---------------------------------------------------------------------------------------------------- c. trim

def test_trim_indices_and_the_silent_row(enc):
    host = _host()
    sig = trim_signals()
    names = ["ramp", "silence", "ties", "two", "square"]
    wav, lens = _rows([sig[n] for n in names])
    win, info = host.speaker_features(enc, wav, lens)
    for i, n in enumerate(names):
        first, last = sp.trim_indices(sig[n])
        F = sp.num_frames(last - first, FRAME_LEN, FRAME_STEP) if first >= 0 else 0
        assert info[i].tolist() == [first, last, F, 1 if F else 0], n
    assert info[0, 2] > 0 and info[2, 2] > 0 and info[1, 2] == 0 and info[3, 2] == 0 and info[4, 2] == 0
    assert win.shape[0] == 2 and bool(torch.isfinite(win).all())
    # the rows that keep something are not affected by the ones that do not
    alone, info1 = host.speaker_features(enc, *_rows([sig["ramp"]], pad=5))
    assert info1[0].tolist() == info[0].tolist() and torch.equal(alone[0], win[0])
    emb = host.speaker_forward(enc, win, [0, 2], len(names))
    assert bool((emb[[1, 3, 4]] == 0).all()) and abs(float(emb[0].norm()) - 1.0) < 1e-5 and abs(float(emb[2].norm()) - 1.0) < 1e-5
    with pytest.raises(ValueError, match=r"rows \[1, 3, 4\]"):
        host.speaker_embedding(enc, wav, lens)
    with pytest.raises(ValueError, match="sample rate"):
        host.speaker_embedding(enc, wav, lens, sample_rate=16000)


# ---------------------------------------------------------------------------------------------------- d. fbank

@pytest.mark.parametrize("name", ["frames1", "frames2", "frames163", "tone", "impulse"])
def test_fbank_against_definition(name):
    x = fbank_signals()[name]
    f64, f32 = sp.fbank_features(x, FS, 1024, np.float64), sp.fbank_features(x, FS, 1024, np.float32)
    F = f64.shape[0]
    assert F == {"frames1": 1, "frames2": 2, "frames163": 163}.get(name, F)
    offs = sp.window_offsets(F, "all")
    want = np.stack([sp.cut_window(f64, o) for o in offs])
    yard = float(np.abs(np.stack([sp.cut_window(f32, o) for o in offs]).astype(np.float64) - want).max())
    wav, _ = _rows([x])
    info = torch.tensor([[0, len(x), -7, -7]], dtype=torch.int32, device=DEV)
    win = torch.full((4, 160, 64), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.internal_spkenc_fbank(wav.data_ptr(), 1, wav.shape[1], FS, 1024, 1, None, 4, win.data_ptr(), info.data_ptr(), _stream()))
    assert info.cpu().tolist() == [[0, len(x), F, len(offs)]]
    got = win[:len(offs)].cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    report(f"SPEAKER fbank {name}: {F} frames, max error {err:.3e}, numpy float32 definition {yard:.3e}, ratio {err / max(yard, 1e-30):.2f}")
    assert np.isfinite(got).all() and err <= RULE * yard
    if F < 160:
        assert not got[0, F:].any()                          # zero rows behind the utterance's end, exactly
    assert bool(torch.isnan(win[len(offs):]).all())           # slots beyond the row's windows are not written


# ---------------------------------------------------------------------------------------------------- e. the whole path

@pytest.mark.parametrize("windows", ["center", "all"])
def test_whole_path_against_definition(enc, windows):
    host = _host()
    utts = list(utterances())
    want = reference_embeddings(windows, "float64")
    yard = float(np.abs(reference_embeddings(windows, "float32").astype(np.float64) - want).max())
    emb = host.speaker_embedding(enc, utts, windows=windows)
    assert emb.device.type == "cuda" and emb.dtype == torch.float32 and tuple(emb.shape) == (3, 512)
    got = emb.cpu().numpy().astype(np.float64)
    nw = [len(sp.window_offsets(sp.utterance_windows(u)[0][2], windows)) for u in utts]
    assert sp.utterance_windows(utts[1])[0][2] < 160 and (windows == "center" or max(nw) > 1)
    err = float(np.abs(got - want).max())
    report(f"SPEAKER whole path windows={windows} {nw}: max error {err:.3e}, float32 definition {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= RULE * yard
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-5


def test_explicit_offsets(enc):
    host = _host()
    utts = list(utterances())
    F = [sp.utterance_windows(u)[0][2] for u in utts]
    assert F[0] > 167 and F[1] < 160
    offs = [F[0] - 160, 0, max(F[2] - 160, 0)]
    emb = host.speaker_embedding(enc, utts, windows=offs).cpu().numpy().astype(np.float64)
    want = sp.speaker_embedding(weights(), utts, windows=offs)
    yard = float(np.abs(sp.speaker_embedding(weights(), utts, windows=offs, dtype=np.float32).astype(np.float64) - want).max())
    assert np.abs(emb - want).max() <= RULE * yard
    with pytest.raises(ValueError, match="outside"):
        host.speaker_embedding(enc, utts, windows=[F[0] - 159, 0, 0])


# ---------------------------------------------------------------------------------------------------- f. end to end

def test_embedding_feeds_synthesize_unchanged(enc):
    from cmtts_amd.config import get_config
    from cmtts_amd.weights import synth_cmtts_state_dict
    host = _host()
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, device=DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=3, dur_frames=4.0, dur_spread=0.0))
    emb = host.speaker_embedding(enc, list(utterances())[:2])
    assert emb.is_cuda and tuple(emb.shape) == (2, cfg.external_speaker_dim)
    rs = np.random.RandomState(0)
    L = 6
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(2, L)).astype(np.int64))
    src = torch.tensor([L, L - 2])
    texts[1, L - 2:] = 0
    syn = host.CMTotalTTSSynthesize.from_model(model, T=2)
    seeds = torch.tensor([11, 12], dtype=torch.int64)
    a = syn.synthesize((None, None, None, texts, src, L, emb), seeds=seeds)
    b = syn.synthesize((None, None, None, texts, src, L, emb.cpu().numpy()), seeds=seeds)
    assert torch.equal(a[0], b[0]) and torch.equal(torch.as_tensor(a[11]), torch.as_tensor(b[11]))
    assert bool(torch.isfinite(a[0]).all())


# ---------------------------------------------------------------------------------------------------- g. C ABI

def test_invalid_arguments_are_refused_before_any_launch(enc):
    lib = _lib.load()
    INV = -1
    wav, lens = _rows([trim_signals()["ramp"]])
    ld = wav.shape[1]
    nv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    win = torch.full((1, 160, 64), 5.0, device=DEV)
    info = torch.full((1, 4), 9, dtype=torch.int32, device=DEV)
    emb = torch.full((1, 512), 5.0, device=DEV)
    rm = torch.zeros(1, dtype=torch.int32, device=DEV)
    nb = lib.cmtts_spkenc_workspace_bytes(1, ld, 1)
    assert nb > 0 and lib.cmtts_spkenc_workspace_bytes(0, ld, 1) == 0 and lib.cmtts_spkenc_workspace_bytes(1, 0, 1) == 0
    assert lib.cmtts_spkenc_workspace_bytes(1, ld, 65) == 0 and lib.cmtts_spkenc_workspace_bytes(1, ld, 0) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    h, s = enc._h, _stream()

    def feat(e=h, w=wav.data_ptr(), rows=1, ld_=ld, n=nv.data_ptr(), fs=FS, wl=1024, mode=0, offs=None, mw=1, out=win.data_ptr(), inf=info.data_ptr()):
        return lib.cmtts_spkenc_features(e, w, rows, ld_, n, fs, wl, mode, offs, mw, out, inf, s)

    def fwd(e=h, w=win.data_ptr(), W=1, r=rm.data_ptr(), rows=1, out=emb.data_ptr(), wsp=ws.data_ptr(), nbytes=nb):
        return lib.cmtts_spkenc_forward(e, w, W, r, rows, out, wsp, nbytes, s)

    bad = [feat(e=None), feat(w=None), feat(n=None), feat(out=None), feat(inf=None), feat(rows=0), feat(ld_=0), feat(fs=48000), feat(fs=4000),
           feat(wl=512), feat(wl=2048), feat(mode=3), feat(mode=2), feat(mw=2), feat(mode=1, mw=65), feat(mode=1, mw=0),
           fwd(e=None), fwd(w=None), fwd(r=None), fwd(out=None), fwd(wsp=None), fwd(rows=0), fwd(W=-1), fwd(nbytes=nb - 1)]
    assert bad == [INV] * len(bad), bad
    assert b"workspace too small" in lib.cmtts_last_error()
    fresh = C.c_void_p()
    assert lib.cmtts_spkenc_create(None) == INV and lib.cmtts_spkenc_create(C.byref(fresh)) == 0
    try:
        assert feat(e=fresh) == INV and b"finalize" in lib.cmtts_last_error() and fwd(e=fresh) == INV
        assert lib.cmtts_spkenc_finalize(fresh) == INV and b"missing tensor" in lib.cmtts_last_error()
        assert lib.cmtts_spkenc_set_tensor(fresh, None, None, None, 0) == INV and lib.cmtts_spkenc_finalize(None) == INV
    finally:
        lib.cmtts_spkenc_destroy(fresh)
    torch.cuda.synchronize()
    # nothing was launched: the outputs hold what they held
    assert bool((win == 5.0).all()) and bool((emb == 5.0).all()) and bool((info == 9).all())
    assert feat() == 0 and fwd() == 0
    torch.cuda.synchronize()
    assert abs(float(emb[0].norm()) - 1.0) < 1e-5
