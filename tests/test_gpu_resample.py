"""Output sample rates and G.711 on the device (include/cmtts_hip.h: cmtts_resample_encode, cmtts_vocoder_forward_windows_f32;
host.vocoder_infer / vocoder_infer_stream / synthesize_stream with sample_rate / encoding): the kernel against the numpy definition
(cmtts_amd/resample.py), pieces bitwise equal to the whole, the float windowed last layer bitwise against the one-shot waveform, the
stream bitwise against the one-shot call, the native path untouched, and argument validation."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import resample as rs
from cmtts_amd.config import HifiGanConfig, get_config
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict
from conftest import report
from resample_cases import GARBAGE, RATES, definition_and_bound, filt, reference, waves

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = HifiGanConfig().hop
TORCH_DTYPE = {"f32": torch.float32, "s16": torch.int16, "mulaw": torch.uint8, "alaw": torch.uint8}


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
    return _host().Generator(hcfg, DEV).load_state_dict(hsd)


def _mels(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 80, T, generator=g) * 0.8 - 1.0).to(DEV)


class _Resampler:
    def __init__(self, rate):
        self.lib = _lib.load()
        self.L, self.M, self.taps, self.half, self.R = filt(rate)
        self.h = C.c_void_p()
        _lib.check(self.lib.cmtts_resampler_create(self.L, self.M, self.taps.ctypes.data_as(C.c_void_p), self.half, C.byref(self.h)))
        assert self.lib.cmtts_resampler_half_width(self.h) == self.R

    def __del__(self):
        self.lib.cmtts_resampler_destroy(self.h)

    def encode(self, wav, segs, encoding, out_ld, max_wav=32768.0, fill=None):
        """cmtts_resample_encode with a DEVICE table -> [N, out_ld] numpy."""
        tab = torch.tensor(segs, dtype=torch.int32, device=DEV)
        out = torch.empty(len(segs), out_ld, dtype=TORCH_DTYPE[encoding], device=DEV)
        if fill is not None:
            out.fill_(fill)
        _lib.check(self.lib.cmtts_resample_encode(self.h, wav.data_ptr(), wav.shape[0], wav.shape[1], tab.data_ptr(), len(segs),
                                                  rs.ENCODINGS[encoding], max_wav, out.data_ptr(), out_ld, _stream()))
        return out.cpu().numpy()


def _rows(xs, ld):
    """Waves as the rows of one fp32 buffer; GARBAGE after each row's valid samples."""
    buf = np.full((len(xs), ld), GARBAGE, np.float32)
    for i, x in enumerate(xs):
        buf[i, : len(x)] = x
    return torch.from_numpy(buf).to(DEV)


def _check_f32(got, y, bound, what):
    d = np.abs(got.astype(np.float64) - y)
    assert (d <= bound).all(), f"{what}: output {int(np.argmax(d - bound))} is {d.max():.3e} off, bound {bound[np.argmax(d - bound)]:.3e}"


# ---------------------------------------------------------------------------------------------------- a. kernel vs definition

@pytest.mark.parametrize("rate", RATES)
def test_kernel_against_definition(rate):
    r = _Resampler(rate)
    xs, ref = waves(rate), reference(rate)
    assert [len(x) for x in xs] == [1000, 257, 1, r.R - 1]
    wav = _rows(xs, 1000)
    nout = [rs.out_len(len(x), r.L, r.M) for x in xs]
    segs = [(i, 0, 0, nout[i], len(x)) for i, x in enumerate(xs)]
    out_ld = max(nout) + 3
    got = {enc: r.encode(wav, segs, enc, out_ld, fill=1) for enc in rs.ENCODINGS}
    ndiff = total = 0
    for i, (y, bound) in enumerate(ref):
        n = nout[i]
        assert len(y) == n
        for enc in rs.ENCODINGS:
            assert not got[enc][i, n:].any(), f"row {i} {enc}: no zeros after the segment"
        _check_f32(got["f32"][i, :n], y, bound, f"{rate} Hz row {i}")
        d = np.abs(got["s16"][i, :n].astype(np.int64) - rs.to_s16(y))
        assert d.max(initial=0) <= 1, f"{rate} Hz row {i}: s16 {d.max()} LSB from the definition"
        ndiff += int(np.count_nonzero(d))
        total += n
        # G.711 of the kernel's OWN s16 output, bit for bit
        assert np.array_equal(got["mulaw"][i, :n], rs.lin2ulaw(got["s16"][i, :n]))
        assert np.array_equal(got["alaw"][i, :n], rs.lin2alaw(got["s16"][i, :n]))
    report(f"RESAMPLE {rate} Hz: s16 {ndiff} of {total} samples 1 LSB from the float64 definition")
    assert ndiff <= 0.01 * total


def test_saturation_and_g711_codes_on_device():
    """The saturating cast (+-1.2 through the DC gain of a 2x up-sampler) and every G.711 segment: a ramp over the whole int16 range."""
    r = _Resampler(44100)
    n = 4096
    x = np.concatenate([np.full(200, 1.2), np.full(200, -1.2), np.linspace(-1.0, 1.0, n - 400)]).astype(np.float32)
    wav = _rows([x], n)
    nout = rs.out_len(n, r.L, r.M)
    seg = [(0, 0, 0, nout, n)]
    s16 = r.encode(wav, seg, "s16", nout)[0]
    f32 = r.encode(wav, seg, "f32", nout)[0]
    assert s16[100:300].tolist() == [32767] * 200 and s16[500:700].tolist() == [-32768] * 200          # no wrap
    assert np.array_equal(s16, rs.to_s16(f32))                      # the cast, exactly, on the kernel's own float output
    assert len(np.unique(s16)) > 3000
    for enc, f in (("mulaw", rs.lin2ulaw), ("alaw", rs.lin2alaw)):
        c = r.encode(wav, seg, enc, nout)[0]
        assert np.array_equal(c, f(s16)) and len(np.unique(c)) >= 200
    half = r.encode(wav, seg, "s16", nout, max_wav=16384.0)[0]
    assert np.array_equal(half, rs.to_s16(f32, 16384.0))


# ---------------------------------------------------------------------------------------------------- b. segments

@pytest.mark.parametrize("rate", RATES)
def test_pieces_bitwise_equal_to_the_whole(rate):
    r = _Resampler(rate)
    x = waves(rate)[0]
    n = len(x)
    whole_seg = [(0, 0, 0, rs.out_len(n, r.L, r.M), n)]
    nout = whole_seg[0][3]
    assert nout > 256                                                # the whole crosses a workgroup tile edge
    cuts = [0, 3, 130, 131, 131, 131 + r.R - 1, 515, n]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    plan = rs.plan_segments(pieces, n, r.L, r.M, r.half)
    assert any(m0 == m1 for m0, m1, _, _ in plan)
    # every piece in a row of its own whose element 0 is another absolute sample: 1, 2 or 3 samples before what the piece needs
    # (origins that are no multiples of 4: rows not 16-byte aligned to the wave), and no wider than the widest piece needs
    origins = [lo - 1 - i % 3 for i, (_, _, lo, _) in enumerate(plan)]
    ld = max(hi - o for o, (_, _, _, hi) in zip(origins, plan))
    buf = np.full((len(plan), ld), GARBAGE, np.float32)
    for i, o in enumerate(origins):
        a, b = max(o, 0), min(o + ld, n)
        buf[i, a - o:b - o] = x[a:b]
    assert any(o % 4 for o in origins) and origins[0] < 0
    segs = [(i, o, m0, m1, n) for i, (o, (m0, m1, _, _)) in enumerate(zip(origins, plan))]
    out_ld = max(m1 - m0 for m0, m1, _, _ in plan) + 5
    for enc in ("f32", "s16", "mulaw"):
        whole = r.encode(_rows([x], n), whole_seg, enc, nout)[0]
        got = r.encode(torch.from_numpy(buf).to(DEV), segs, enc, out_ld, fill=1)
        for i, (m0, m1, _, _) in enumerate(plan):
            assert not got[i, m1 - m0:].any(), f"{enc} piece {i}: no zeros after the segment"
        stitched = np.concatenate([got[i, : m1 - m0] for i, (m0, m1, _, _) in enumerate(plan)])
        assert stitched.tobytes() == whole.tobytes(), f"{rate} Hz {enc}: pieces differ from the whole"


# ---------------------------------------------------------------------------------------------------- c. float windows

def _forward_windows_f32(voc, mel, windows, Tw, core, margin):
    lib = voc.lib
    B, _, T = mel.shape
    tab = torch.tensor(windows, dtype=torch.int32, device=DEV)
    N = len(windows)
    rows = torch.full((N, (core + 2 * margin) * HOP), float("nan"), device=DEV)
    nb = lib.cmtts_vocoder_windows_workspace_bytes(voc._h, N, Tw)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_vocoder_forward_windows_f32(voc._h, mel.data_ptr(), B, T, tab.data_ptr(), N, Tw, core, margin, rows.data_ptr(),
                                                     ws.data_ptr(), nb, _stream()))
    return rows


def test_float_windows_bitwise():
    voc = _voc()
    assert voc.set_option("winograd", 0) == 1
    B, T, core, Tw = 2, 45, 8, 36
    mel = _mels(B, T, 4)
    wav = voc(mel)[:, 0]
    # clamped at frame 0 (no left margin), interior (14 = H + 1 frames on both sides), clamped at T (no right margin), a short core
    win = [(0, 0, 0, 8), (1, 9, 14, 8), (0, 9, 28, 8), (1, 5, 14, 5)]
    rows = _forward_windows_f32(voc, mel, win, Tw, core, 1)
    torch.cuda.synchronize()
    for n, (b, start, off, cl) in enumerate(win):
        lo, hi = start + max(off - 1, 0), start + min(off + cl + 1, Tw)
        assert torch.equal(rows[n, : (hi - lo) * HOP], wav[b, lo * HOP:hi * HOP]), n
        assert not rows[n, (hi - lo) * HOP:].any(), n
    assert [start + min(off + cl + 1, Tw) for _, start, off, cl in win][2] == T
    # margin 0: the core columns alone
    rows0 = _forward_windows_f32(voc, mel, win[1:2], Tw, core, 0)
    assert torch.equal(rows0[0], wav[1, 23 * HOP:31 * HOP])


# ---------------------------------------------------------------------------------------------------- d. stream == one-shot

def _stitch(stream_iter, out_lens, dtype):
    """(utterance, offset in output samples, chunk, is_last) -> one array per utterance; checks order, offsets, dtype and is_last."""
    out = [[] for _ in out_lens]
    pos = [0] * len(out_lens)
    done = [False] * len(out_lens)
    for b, off, chunk, last in stream_iter:
        assert not done[b] and off == pos[b] and chunk.dtype == dtype and len(chunk) > 0
        out[b].append(chunk)
        pos[b] += len(chunk)
        done[b] = last
        assert last == (pos[b] == out_lens[b])
    assert all(done[b] for b in range(len(out_lens)) if out_lens[b] > 0)
    assert all(not out[b] for b in range(len(out_lens)) if out_lens[b] == 0)
    return [np.concatenate(o) if o else np.zeros(0, dtype) for o in out]


STREAM_CASES = [(8000, "mulaw"), (8000, "s16"), (48000, "s16"), (48000, "f32")]


@pytest.fixture(scope="module")
def stream_setup():
    voc = _voc()
    B, T, lens = 3, 61, [61, 37, 5]
    return voc, _mels(B, T, 9), lens


@pytest.mark.parametrize("rate,enc", STREAM_CASES)
def test_stream_equals_one_shot_bitwise(stream_setup, rate, enc):
    voc, mel, lens = stream_setup
    host = _host()
    L, M = rs.ratio(rs.NATIVE_RATE, rate)
    out_lens = [rs.out_len(n * HOP, L, M) for n in lens]
    prev = voc.set_option("winograd", 0)
    try:
        ref = host.vocoder_infer(mel, voc, lengths=[n * HOP for n in lens], sample_rate=rate, encoding=enc)
        got = _stitch(host.vocoder_infer_stream(mel, voc, lens, (8, 16), sample_rate=rate, encoding=enc), out_lens, rs.DTYPES[enc])
    finally:
        voc.set_option("winograd", prev)
    for b in range(len(lens)):
        assert ref[b].dtype == rs.DTYPES[enc] and len(ref[b]) == out_lens[b]
        assert got[b].tobytes() == ref[b].tobytes(), f"utterance {b}: {np.count_nonzero(got[b] != ref[b])} samples differ"
    # the default conv forms: the window batch may take another form than the whole batch — lengths, offsets and dtype only
    ref = host.vocoder_infer(mel, voc, lengths=[n * HOP for n in lens], sample_rate=rate, encoding=enc)
    got = _stitch(host.vocoder_infer_stream(mel, voc, lens, (8, 16), sample_rate=rate, encoding=enc), out_lens, rs.DTYPES[enc])
    d = max(float(np.abs(got[b].astype(np.float64) - ref[b].astype(np.float64)).max()) for b in range(len(lens)))
    report(f"RESAMPLE stream vs one-shot, default conv forms, {rate} Hz {enc}: max |difference| {d:g}")


def test_stream_zero_length_utterance():
    voc = _voc()
    lens = [20, 0]
    got = list(_host().vocoder_infer_stream(_mels(2, 20, 2), voc, lens, (8, 16), sample_rate=8000, encoding="mulaw"))
    assert got and all(b == 0 for b, _, _, _ in got)
    _stitch(iter(got), [rs.out_len(20 * HOP, 160, 441), 0], np.uint8)


# ---------------------------------------------------------------------------------------------------- e. one-shot vs definition

def test_one_shot_against_definition():
    voc = _voc()
    mel = _mels(2, 12, 6)
    lens = [12 * HOP, 7 * HOP + 13]
    wav = voc(mel)[:, 0].cpu().numpy()
    got = _host().vocoder_infer(mel, voc, lengths=lens, sample_rate=16000, encoding="f32")
    L, M, taps, half, _ = filt(16000)
    for b, n in enumerate(lens):
        y, bound = definition_and_bound(wav[b, :n], L, M, taps, half)
        assert got[b].dtype == np.float32 and len(got[b]) == len(y) == rs.out_len(n, L, M)
        _check_f32(got[b], y, bound, f"utterance {b}")


# ---------------------------------------------------------------------------------------------------- f. native path untouched

def test_native_path_untouched():
    host = _host()
    mel = _mels(2, 10, 8)
    voc = _voc()
    plain = host.vocoder_infer(mel, voc, lengths=[10 * HOP, 777])
    native = host.vocoder_infer(mel, voc, lengths=[10 * HOP, 777], sample_rate=22050, encoding="s16")
    dev = host.vocoder_infer_device(mel, voc).cpu().numpy()
    for b, n in enumerate((10 * HOP, 777)):
        assert plain[b].dtype == np.int16 and np.array_equal(plain[b], dev[b, :n]) and np.array_equal(native[b], plain[b])
    # +1.0 still wraps to -32768 on the native path (a conv_post bias that saturates tanh); a resampled output saturates instead
    voc2 = _voc(**{"conv_post.bias": 20.0})
    for out in (host.vocoder_infer(mel, voc2), host.vocoder_infer(mel, voc2, sample_rate=None, encoding="s16"),
                host.vocoder_infer(mel, voc2, sample_rate=22050)):
        assert all((w == -32768).all() for w in out)
    chunks = list(host.vocoder_infer_stream(mel, voc2, [10, 3], (4,), sample_rate=22050, encoding="s16"))
    assert all(c.dtype == np.int16 and (c == -32768).all() for _, _, c, _ in chunks)
    up = host.vocoder_infer(mel, voc2, sample_rate=44100, encoding="s16")
    assert all(w.dtype == np.int16 and w.min() >= 0 and w[100:-100].min() >= 32000 for w in up)


# ---------------------------------------------------------------------------------------------------- g. text -> 8 kHz mu-law

def test_synthesize_stream_mulaw():
    host = _host()
    voc = _voc()
    voc.set_option("winograd", 0)
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=2, dur_frames=5.0, dur_spread=0.3))
    g = np.random.RandomState(2)
    B, Lt = 3, 14
    src = np.asarray([Lt, 9, 5], np.int64)
    texts = np.zeros((B, Lt), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = g.randint(1, cfg.n_symbols, size=s)
    spk = torch.from_numpy(g.standard_normal((B, cfg.external_speaker_dim)).astype(np.float32))
    texts, src = torch.from_numpy(texts), torch.from_numpy(src)
    seeds = torch.tensor([11, 12, 13], dtype=torch.int64)
    out = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk)
    mel = host.sample_with_cond(model, out["cond_ct"], out["speaker_emb"], 4, None, factors=out.get("cond_factors"), seeds=seeds)
    lens = out["mel_lens"].cpu().tolist()
    assert max(lens) > 8
    ref = host.vocoder_infer(mel.transpose(1, 2), voc, lengths=[n * HOP for n in lens], sample_rate=8000, encoding="mulaw")
    got = _stitch(host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=4, chunk_frames=(8, 16), seeds=seeds,
                                         sample_rate=8000, encoding="mulaw"), [rs.out_len(n * HOP, 160, 441) for n in lens], np.uint8)
    for b in range(B):
        assert np.array_equal(got[b], ref[b]), b


# ---------------------------------------------------------------------------------------------------- h. argument validation

def test_argument_validation():
    lib = _lib.load()
    L, M, taps, half, R = filt(8000)
    tp = taps.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert lib.cmtts_resampler_create(L, M, None, half, C.byref(h)) == -1
    assert lib.cmtts_resampler_create(L, M, tp, half, None) == -1
    assert lib.cmtts_resampler_create(0, M, tp, half, C.byref(h)) == -1 and lib.cmtts_resampler_create(-3, M, tp, half, C.byref(h)) == -1
    assert lib.cmtts_resampler_create(L, 0, tp, half, C.byref(h)) == -1 and lib.cmtts_resampler_create(L, M, tp, -1, C.byref(h)) == -1
    assert lib.cmtts_resampler_create(2 * L, 2 * M, tp, half, C.byref(h)) == -1          # not reduced
    assert lib.cmtts_resampler_create(48001, 22050, tp, half, C.byref(h)) == -2          # the tap table would not fit
    assert not h.value and lib.cmtts_resampler_half_width(None) == -1
    r = _Resampler(8000)
    n, rows = 1000, 2
    wav = torch.zeros(rows, n, device=DEV)
    nout = rs.out_len(n, L, M)
    out = torch.full((2, nout), 0x5A5A, dtype=torch.int16, device=DEV)
    good = [(0, 0, 0, nout, n), (1, 0, 10, 20, n)]

    def call(segs=good, rh=r.h, wav_p=wav.data_ptr(), rows_c=rows, ld=n, N=2, enc=1, mw=32768.0, out_p=out.data_ptr(), old=nout):
        tab = torch.tensor(segs, dtype=torch.int32, device=DEV) if segs is not None else None
        return lib.cmtts_resample_encode(rh, wav_p, rows_c, ld, None if tab is None else tab.data_ptr(), N, enc, mw, out_p, old, _stream())

    bad = {
        "null resampler": call(rh=None), "null wav": call(wav_p=None), "null table": call(segs=None), "null out": call(out_p=None),
        "N = 0": call(N=0), "rows = 0": call(rows_c=0), "ld = 0": call(ld=0), "out_ld = 0": call(old=0),
        "unknown encoding": call(enc=4), "negative encoding": call(enc=-1), "max_wav 0": call(mw=0.0),
        "m1 < m0": call(segs=[(0, 0, 5, 4, n), good[1]]), "m0 < 0": call(segs=[(0, 0, -1, 4, n), good[1]]),
        "row >= rows": call(segs=[(2, 0, 0, nout, n), good[1]]), "row < 0": call(segs=[(-1, 0, 0, nout, n), good[1]]),
        "m1 beyond the utterance": call(segs=[(0, 0, 0, nout + 1, n), good[1]]), "negative n": call(segs=[(0, 0, 0, 0, -1), good[1]]),
        "more outputs than out_ld": call(old=nout - 1),
        "row starts after the samples needed": call(segs=[(0, 300, 100, 120, n), good[1]]),
        "row ends before the samples needed": call(segs=[(0, 0, 0, nout, n), good[1]], ld=n - 1),
    }
    torch.cuda.synchronize()
    for what, rc in bad.items():
        assert rc == -1, what
    assert lib.cmtts_resample_encode(r.h, wav.data_ptr(), rows, n, (C.c_int32 * 10)(*[0] * 10), 2, 1, 32768.0, out.data_ptr(), nout,
                                     _stream()) == -1, "pageable host table"
    torch.cuda.synchronize()
    assert (out == 0x5A5A).all(), "a rejected call wrote the output"
    assert call() == 0
    pinned = torch.tensor(good, dtype=torch.int32).pin_memory()
    assert lib.cmtts_resample_encode(r.h, wav.data_ptr(), rows, n, pinned.data_ptr(), 2, 1, 32768.0, out.data_ptr(), nout, _stream()) == 0
    torch.cuda.synchronize()
    assert not out.any()

    # the float windows: the int16 entry point's checks, the margin, the workspace
    voc = _voc()
    B, T, Tw, core = 2, 40, 30, 4
    mel = _mels(B, T, 3)
    nb = lib.cmtts_vocoder_windows_workspace_bytes(voc._h, 2, Tw)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    rows_f = torch.full((2, (core + 2) * HOP), 3.0, device=DEV)
    gwin = [(0, 0, 0, 4), (1, 10, 13, 4)]

    def wcall(win=gwin, mel_p=mel.data_ptr(), Twc=Tw, corec=core, margin=1, rows_p=rows_f.data_ptr(), ws_p=ws.data_ptr(), nbc=nb, handle=voc._h):
        tab = torch.tensor(win, dtype=torch.int32, device=DEV) if win is not None else None
        return lib.cmtts_vocoder_forward_windows_f32(handle, mel_p, B, T, None if tab is None else tab.data_ptr(), 2, Twc, corec, margin,
                                                     rows_p, ws_p, nbc, _stream())

    wbad = {
        "null vocoder": wcall(handle=None), "null mel": wcall(mel_p=None), "null table": wcall(win=None), "null rows": wcall(rows_p=None),
        "null ws": wcall(ws_p=None), "Tw > T": wcall(Twc=T + 1), "core 0": wcall(corec=0), "negative margin": wcall(margin=-1),
        "margin wider than the window allows": wcall(margin=14), "window past T": wcall(win=[(0, 11, 0, 4), (1, 0, 0, 4)]),
        "utterance >= B": wcall(win=[(2, 0, 0, 4), (1, 0, 0, 4)]), "core_len > core": wcall(win=[(0, 0, 0, 5), (1, 0, 0, 4)]),
    }
    torch.cuda.synchronize()
    for what, rc in wbad.items():
        assert rc == -1, what
    assert wcall(nbc=nb - 1) == -4, "short workspace"
    torch.cuda.synchronize()
    assert (rows_f == 3.0).all(), "a rejected call wrote the output"
    assert wcall() == 0
    torch.cuda.synchronize()
    assert not (rows_f == 3.0).any()
