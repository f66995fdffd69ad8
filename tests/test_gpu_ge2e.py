"""GE2E speaker embeddings from reference audio on the device (include/cmtts_hip.h: cmtts_ge2e_*; host.ge2e_embedding): one LSTM layer alone
through its hook, the front end alone, the whole path against the float64 definition (cmtts_amd/ge2e.py), batch independence bitwise, the
embedding as spker_embeds= end to end, and the invalid-argument paths of the C ABI.

Tolerances are not fixed numbers: each comparison runs the same computation in float32 on the CPU (torch.nn.LSTM for the recurrence, the
numpy definition elsewhere) and takes ITS error against float64 as the yardstick; the kernel's error must be <= 4 x that."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import ge2e as g2
from conftest import report
from ge2e_cases import (FS, GARBAGE, LSTM_CASES, TILE, clips, layer_tensors, lstm_case, lstm_float32, mel_reference, mel_rows, reference_embeddings,
                        weights)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RULE = 4.0


@pytest.fixture(autouse=True, scope="module")
def _symbols():
    if not hasattr(C.CDLL(_lib.LIB_PATH), "cmtts_ge2e_forward"):
        pytest.skip("this libcmtts_hip.so has no GE2E encoder (cmtts_ge2e_*)")


def _host():
    from cmtts_amd import host
    return host


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def enc():
    return _host().get_ge2e_encoder(weights(), DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_layer(layer, x, lens, tile=TILE):
    """One LSTM layer through its hook: (hseq [N, T, 256], hlast [N, 256]) as device tensors; hseq starts as NaN."""
    w_ih, w_hh, b_ih, b_hh = layer_tensors(layer)
    fi, bias = _lib.ge2e_pack_lstm(w_ih, b_ih, b_hh)
    fh = _lib.ge2e_pack_lstm(w_hh)
    N, T, K = x.shape
    xd, fid, fhd, bd = (x if isinstance(x, torch.Tensor) else _dev(x)), _dev(fi), _dev(fh), _dev(bias)
    ld = None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device=DEV)
    pre = torch.empty(N, T, 1024, dtype=torch.float32, device=DEV)
    hseq = torch.full((N, T, 256), float("nan"), dtype=torch.float32, device=DEV)
    hlast = torch.full((N, 256), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.internal_ge2e_layer(xd.data_ptr(), N, T, K, fid.data_ptr(), fhd.data_ptr(), bd.data_ptr(), None if ld is None else ld.data_ptr(),
                                        tile, pre.data_ptr(), hseq.data_ptr(), hlast.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return hseq, hlast


# ---------------------------------------------------------------------------------------------------- a. the recurrence alone

@pytest.mark.parametrize("name", sorted(LSTM_CASES))
def test_lstm_layer_against_float64(name):
    """Rule: max error <= 4 x the error of torch.nn.LSTM in float32 on the CPU, both against the float64 definition."""
    layer, N, T, scale, lens = LSTM_CASES[name]
    x, _, want, want_h = lstm_case(name)
    o32, h32 = lstm_float32(name)
    hseq, hlast = _run_layer(layer, x, lens)
    got, got_h = hseq.cpu().numpy().astype(np.float64), hlast.cpu().numpy().astype(np.float64)
    # the outputs are written up to the longest window of a window's TILE (the workgroup stops there); behind that they keep what they held
    tmax = np.asarray([T if lens is None else max(lens[i // TILE * TILE:i // TILE * TILE + TILE]) for i in range(N)])
    live = np.arange(T)[None, :] < tmax[:, None]
    assert np.isfinite(got[live]).all() and np.isfinite(got_h).all() and np.isnan(got[~live]).all()
    err = max(float(np.abs(got - want)[live].max()), float(np.abs(got_h - want_h).max()))
    yard = max(float(np.abs(o32.astype(np.float64) - want)[live].max()), float(np.abs(h32.astype(np.float64) - want_h).max()))
    report(f"GE2E lstm ({name}) K={x.shape[2]} N={N} T={T}: max error {err:.3e}, torch CPU float32 {yard:.3e}, ratio {err / yard:.2f}")
    assert err <= RULE * yard
    if lens is not None:
        for i, l in enumerate(lens):                          # the frozen state is repeated behind a window's frames, bit for bit
            assert torch.equal(hseq[i, l - 1], hlast[i]) and bool((hseq[i, l:tmax[i]] == hlast[i]).all())


def test_layer_hook_refuses_what_no_instance_covers():
    x = torch.zeros(1, 2, 40, device=DEV)
    out = torch.full((1, 2, 1024 + 256 + 256), 7.0, device=DEV)
    p = x.data_ptr()
    for N, T, K, tile in ((1, 2, 40, 32), (1, 2, 64, TILE), (1, 0, 40, TILE)):      # the 32-window tile was measured and dropped (profiles/ge2e.md)
        assert _lib.internal_ge2e_layer(p, N, T, K, p, p, p, None, tile, out.data_ptr(), out.data_ptr(), out.data_ptr(), _stream()) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------- b. the front end alone

def test_front_end_against_definition():
    rows = mel_rows()
    ld = max(len(r) for r in rows) + 37
    buf = np.full((len(rows), ld), GARBAGE, np.float32)
    for i, r in enumerate(rows):
        buf[i, :len(r)] = r
    wav, nv = _dev(buf), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)
    T = 163                                                   # beyond the longest row's 161 frames: zero rows, and a last tile that is cut
    win = torch.full((3, T, 40), float("nan"), dtype=torch.float32, device=DEV)
    wl = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    info = torch.full((3, 4), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.internal_ge2e_mel(wav.data_ptr(), 3, ld, nv.data_ptr(), 0, 1, T, win.data_ptr(), wl.data_ptr(), info.data_ptr(), _stream()))
    assert info.cpu().tolist() == [[35200, 35200, 160, 1], [35201, 35201, 161, 1], [221, 221, 2, 1]] and wl.cpu().tolist() == [160, 161, 2]
    for i in range(3):
        want, f32 = mel_reference(i, "float64"), mel_reference(i, "float32")
        F = want.shape[0]
        got = win[i].cpu().numpy().astype(np.float64)
        err, yard = float(np.abs(got[:F] - want).max()), float(np.abs(f32.astype(np.float64) - want).max())
        report(f"GE2E mel row {i} ({len(rows[i])} samples, {F} frames, peak {want.max():.1f}): max error {err:.3e}, numpy float32 definition {yard:.3e}, "
               f"ratio {err / yard:.2f}")
        assert np.isfinite(got).all() and not got[F:].any() and err <= RULE * yard
    # partials: one window each (the second one of 35 201 samples covers half a window and is dropped); the 221-sample row is zero-padded to 35 200
    win2 = torch.full((6, 160, 40), float("nan"), dtype=torch.float32, device=DEV)
    wl2 = torch.full((6,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.internal_ge2e_mel(wav.data_ptr(), 3, ld, nv.data_ptr(), 1, 2, 0, win2.data_ptr(), wl2.data_ptr(), info.data_ptr(), _stream()))
    assert info.cpu().tolist() == [[35200, 35200, 160, 1], [35201, 35201, 161, 1], [221, 35200, 160, 1]] and wl2.cpu().tolist() == [160] * 3 + [-7] * 3
    short = np.concatenate([rows[2], np.zeros(35200 - 221, np.float32)])
    padded = g2.mel_power(short)
    yard = float(np.abs(g2.mel_power(short, np.float32).astype(np.float64) - padded).max())
    assert np.abs(win2[2].cpu().numpy().astype(np.float64) - padded).max() <= RULE * yard
    assert torch.equal(win2[0], win[0, :160]) and torch.equal(win2[1], win[1, :160]) and bool(torch.isnan(win2[3:]).all())


# ---------------------------------------------------------------------------------------------------- c. batch independence, bitwise

def test_window_does_not_depend_on_the_launch():
    x, _, _, _ = lstm_case("l0_n35_t160")
    many, many_h = _run_layer(0, x, None)
    one, one_h = _run_layer(0, x[:1], None)
    assert torch.equal(one[0], many[0]) and torch.equal(one_h[0], many_h[0]) and not torch.equal(many_h[0], many_h[1])


def test_row_does_not_depend_on_the_batch(enc):
    host = _host()
    three = host.ge2e_embedding(enc, list(clips()))
    for i in (0, 2):
        assert torch.equal(host.ge2e_embedding(enc, [clips()[i]])[0], three[i])
    whole = host.ge2e_embedding(enc, list(clips()), using_partials=False)
    assert torch.equal(host.ge2e_embedding(enc, [clips()[0]], using_partials=False)[0], whole[0])


# ---------------------------------------------------------------------------------------------------- d. the whole path

@pytest.mark.parametrize("using_partials", [True, False])
def test_whole_path_against_definition(enc, using_partials):
    want = reference_embeddings(using_partials, "float64")
    yard = float(np.abs(reference_embeddings(using_partials, "float32").astype(np.float64) - want).max())
    emb = _host().ge2e_embedding(enc, list(clips()), using_partials=using_partials)
    assert emb.device.type == "cuda" and emb.dtype == torch.float32 and tuple(emb.shape) == (3, 256)
    got = emb.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    cos = (got * want).sum(axis=1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    report(f"GE2E whole path using_partials={using_partials}: max error {err:.3e}, float32 definition {yard:.3e}, ratio {err / yard:.2f}, "
           f"min cosine {cos.min():.8f}")
    assert cos.min() >= 1 - 1e-5
    assert err <= RULE * yard
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------- e. end to end

def test_embedding_feeds_synthesize_unchanged(enc):
    import dataclasses
    from cmtts_amd.config import get_config
    from cmtts_amd.weights import synth_cmtts_state_dict
    host = _host()
    cfg = dataclasses.replace(get_config("VCTK"), external_speaker_dim=256)
    model = host.CMTotalTTS(cfg, device=DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=3, dur_frames=4.0, dur_spread=0.0))
    emb = host.ge2e_embedding(enc, list(clips())[:2])
    assert emb.is_cuda and tuple(emb.shape) == (2, 256)
    rs = np.random.RandomState(0)
    L = 6
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(2, L)).astype(np.int64))
    src = torch.tensor([L, L - 2])
    texts[1, L - 2:] = 0
    syn = host.CMTotalTTSSynthesize.from_model(model, T=2)
    seeds = torch.tensor([11, 12], dtype=torch.int64)
    a = syn.synthesize((None, None, None, texts, src, L, emb), seeds=seeds)
    b = syn.synthesize((None, None, None, texts, src, L, emb.cpu().numpy()), seeds=seeds)
    assert torch.equal(a[0], b[0]) and bool(torch.isfinite(a[0]).all())
    with pytest.raises(ValueError, match="external_speaker_dim = 256"):
        syn.synthesize((None, None, None, texts, src, L, torch.zeros(2, 512)), seeds=seeds)


def test_predefined_embedder_forward(enc):
    host = _host()
    cfg = {"preprocessing": {"audio": {"sampling_rate": 22050}, "stft": {"win_length": 1024}, "speaker_embedder": "GE2E"}}
    out = host.PreDefinedEmbedder(cfg, weights=weights(), device=DEV).forward(torch.from_numpy(clips()[0]))
    assert isinstance(out, np.ndarray) and out.shape == (1, 256)
    assert np.array_equal(out[0], host.ge2e_embedding(enc, [clips()[0]])[0].cpu().numpy())


# ---------------------------------------------------------------------------------------------------- f. C ABI

def test_invalid_arguments_are_refused_before_any_launch(enc):
    lib = _lib.load()
    INV = -1
    wav = _dev(clips()[0][None])
    ld = wav.shape[1]
    nv = torch.tensor([ld], dtype=torch.int32, device=DEV)
    win = torch.full((1, 160, 40), 5.0, device=DEV)
    wl = torch.full((1,), 9, dtype=torch.int32, device=DEV)
    info = torch.full((1, 4), 9, dtype=torch.int32, device=DEV)
    emb = torch.full((1, 256), 5.0, device=DEV)
    rm = np.zeros(1, np.int32)
    nb = lib.cmtts_ge2e_workspace_bytes(1, 160)
    assert nb > 0 and lib.cmtts_ge2e_workspace_bytes(0, 160) == 0 and lib.cmtts_ge2e_workspace_bytes(1, 0) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    h, s = enc._h, _stream()

    def feat(e=h, w=wav.data_ptr(), rows=1, ld_=ld, n=nv.data_ptr(), fs=FS, mode=1, mw=1, T=160, out=win.data_ptr(), l=wl.data_ptr(), inf=info.data_ptr()):
        return lib.cmtts_ge2e_features(e, w, rows, ld_, n, fs, mode, mw, T, out, l, inf, s)

    def fwd(e=h, w=win.data_ptr(), W=1, T=160, ln=None, r=rm.ctypes.data, rows=1, out=emb.data_ptr(), wsp=ws.data_ptr(), nbytes=nb):
        return lib.cmtts_ge2e_forward(e, w, W, T, ln, r, rows, out, wsp, nbytes, s)

    bad = [feat(e=None), feat(w=None), feat(n=None), feat(out=None), feat(l=None), feat(inf=None), feat(rows=0), feat(ld_=0), feat(fs=16000),
           feat(fs=44100), feat(mode=2), feat(mw=0), feat(mode=0, mw=2), feat(mode=0, T=0),
           fwd(e=None), fwd(w=None), fwd(out=None), fwd(wsp=None), fwd(rows=0), fwd(W=-1), fwd(T=0), fwd(nbytes=nb - 1), fwd(r=None, rows=2),
           fwd(r=np.asarray([1], np.int32).ctypes.data), fwd(r=np.asarray([-1], np.int32).ctypes.data)]
    assert bad == [INV] * len(bad), bad
    assert b"row_map" in lib.cmtts_last_error()
    fresh = C.c_void_p()
    assert lib.cmtts_ge2e_create(None) == INV and lib.cmtts_ge2e_create(C.byref(fresh)) == 0
    try:
        assert feat(e=fresh) == INV and b"finalize" in lib.cmtts_last_error() and fwd(e=fresh) == INV
        assert lib.cmtts_ge2e_finalize(fresh) == INV and b"missing tensor" in lib.cmtts_last_error()
        assert lib.cmtts_ge2e_set_tensor(fresh, None, None, None, 0) == INV and lib.cmtts_ge2e_finalize(None) == INV
    finally:
        lib.cmtts_ge2e_destroy(fresh)
    torch.cuda.synchronize()
    # nothing was launched: the outputs hold what they held
    assert bool((win == 5.0).all()) and bool((emb == 5.0).all()) and bool((info == 9).all()) and bool((wl == 9).all())
    assert feat() == 0 and fwd() == 0
    torch.cuda.synchronize()
    assert abs(float(emb[0].norm()) - 1.0) < 1e-5 and info.cpu().tolist() == [[11025, 35200, 160, 1]]
    with pytest.raises(ValueError, match="22050"):
        _host().ge2e_embedding(enc, wav, sample_rate=16000)
