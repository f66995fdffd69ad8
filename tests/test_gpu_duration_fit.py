"""Duration targets and phoneme marks on the GPU (include/cmtts_hip.h: cmtts_set_duration_targets, cmtts_phoneme_marks;
csrc/duration_fit.hip) against the definition in cmtts_amd/timing.py: the fitted durations exactly, a fitted run against teacher
forcing with the numpy-fitted durations bit for bit, an utterance inside a batch against the utterance alone, the fit behind a
duration table, the refusals, nothing left installed, the marks, streamed PCM of an exact length, and virtual sharded worlds.
Fixture and batches are those of tests/test_gpu_controls.py (dur_frames = 4.0: many equal durations, so remainders tie)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib, resample, shard, timing
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from conftest import load_golden
from test_gpu_controls import N_STEPS, _batch, _run, _virtual_world

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = 256


def _host():
    from cmtts_amd import host
    return host


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def fixture():
    g = load_golden("cmtts_VCTK")
    cfg = get_config("VCTK")
    sd = synth_cmtts_state_dict(cfg, seed=int(g["seed"]), dur_frames=4.0, dur_spread=0.03)
    model = _host().CMTotalTTS(cfg, DEV).load_state_dict(sd)
    return g, cfg, sd, model


def _batch70(cfg):
    """B = 4, L = 70: src_len exactly 64 (one full 64-wide pass), 70 (a second, partial pass), and two shorter ones."""
    rs = np.random.RandomState(70)
    src = np.asarray([64, 70, 37, 23], np.int64)
    texts = np.zeros((4, 70), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = rs.standard_normal(size=(4, cfg.external_speaker_dim)).astype(np.float32)
    return torch.from_numpy(texts), torch.from_numpy(src), torch.from_numpy(spk)


def _shapes(fixture):
    g, cfg, _, _ = fixture
    return {"3x20": (torch.from_numpy(g["texts"]), torch.from_numpy(g["src_lens"]), torch.from_numpy(g["spker_embeds"])),
            "6x33": _batch(cfg, 6, 33, seed=33), "4x70": _batch70(cfg)}


def _text(model, batch, max_mel_len=None, **kw):
    """Text side + frame side only -> the integer outputs (numpy)."""
    texts, src, spk = batch
    out = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, max_mel_len=max_mel_len, **kw)
    torch.cuda.synchronize()
    res = {"log_d": _np(out["log_d_predictions"]), "d_rounded": _np(out["d_rounded"]), "mel_len": _np(out["mel_lens"]),
           "mel2ph": _np(out["mel2ph"]), "out": out}
    if "unmet_targets" in out:
        res["unmet"] = _np(out["unmet_targets"])
    return res


_PLAIN = {}


def _plain(fixture, tag):
    """The plain run of a shape, computed once: n = int(d_rounded) is what every fit starts from."""
    if tag not in _PLAIN:
        r = _text(fixture[3], _shapes(fixture)[tag])
        n = r["d_rounded"].astype(np.int64)
        src = _np(_shapes(fixture)[tag][1])
        assert (n >= 0).all() and not n[np.arange(n.shape[1])[None] >= src[:, None]].any()
        assert (n.sum(1) >= 1).all() and np.array_equal(n.sum(1), r["mel_len"])
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _PLAIN[tag] = (r, n)
    return _PLAIN[tag]


def _segments(src, L):
    """Three segments and one unsegmented tail per utterance: [0, 3s/7) [3s/7, 6s/7) [6s/7, max(6s/7 + 1, s - 2)) and the rest -1.
    s = 70: the third segment is [60, 68) and straddles phonemes 63 / 64."""
    seg = -np.ones((len(src), L), np.int64)
    for b, s in enumerate(int(v) for v in src):
        c1, c2 = s * 3 // 7, s * 6 // 7
        c3 = max(c2 + 1, s - 2)
        assert 0 < c1 < c2 < c3 < s
        seg[b, :c1], seg[b, c1:c2], seg[b, c2:c3] = 0, 1, 2
    return seg


def _mel2ph(d, T):
    B, L = d.shape
    want = np.zeros((B, T), np.int64)
    for b in range(B):
        rep = np.repeat(np.arange(1, L + 1), d[b])[:T]
        want[b, :len(rep)] = rep
    return want


def _tied_at_cut(n, t):
    """Does the largest-remainder cut of this segment pass between two equal remainders?"""
    S = int(n.sum())
    if t < 0 or S == 0:
        return False
    q = n * t
    r = np.sort(q % S)[::-1]
    R = t - int((q // S).sum())
    return 0 < R < len(n) and r[R - 1] == r[R]


def _check_against_definition(got, plain, n, want, what):
    np.testing.assert_array_equal(got["d_rounded"], want.astype(np.float32), err_msg=what)
    np.testing.assert_array_equal(got["mel_len"], want.sum(1), err_msg=what)
    np.testing.assert_array_equal(got["mel2ph"], _mel2ph(want, got["mel2ph"].shape[1]), err_msg=what)      # cum, through mel2ph
    assert np.array_equal(got["log_d"].view(np.int32), plain["log_d"].view(np.int32)), what
    assert "unmet" not in got or not got["unmet"].any(), what


# ---- 1. the kernel equals the definition

@pytest.mark.parametrize("tag", ["3x20", "6x33", "4x70"])
def test_fit_equals_the_definition(fixture, tag):
    model, batch = fixture[3], _shapes(fixture)[tag]
    plain, n = _plain(fixture, tag)
    B, L = n.shape
    src = _np(batch[1])
    if tag == "4x70":
        assert src[0] == 64 and src[1] == 70
    S = n.sum(1)
    nz = (n > 0).sum(1)
    assert (nz >= 2).all()
    mixed = np.where(np.arange(B) % 2 == 1, -1, S + 5)
    ties = 0
    for what, tf in (("S", S), ("S + 1", S + 1), ("2 S + 3", 2 * S + 3), ("below the non-zero count", np.maximum(1, nz // 2)),
                     ("-1 mixed in", mixed)):
        got = _text(model, batch, target_frames=torch.from_numpy(tf.astype(np.int64)))
        want = np.stack([timing.fit_segments(n[b], None, [tf[b]])[0] for b in range(B)])
        assert all(want[b].sum() == tf[b] for b in range(B) if tf[b] >= 0)
        _check_against_definition(got, plain, n, want, (tag, what))
        ties += sum(_tied_at_cut(n[b, :src[b]], int(tf[b])) for b in range(B))
        if what == "S":
            np.testing.assert_array_equal(got["d_rounded"], plain["d_rounded"])
    # three segments and one unsegmented tail
    seg = _segments(src, L)
    Sg = np.stack([[n[b][seg[b] == g].sum() for g in range(3)] for b in range(B)])
    assert (Sg > 0).all()
    tg = np.stack([Sg[:, 0] + 2, np.maximum(1, Sg[:, 1] // 2), 2 * Sg[:, 2] + 3], 1)
    tg[B - 1, 1] = -1
    got = _text(model, batch, target_frames=torch.from_numpy(tg), segments=torch.from_numpy(seg).to(torch.int32))
    want = np.stack([timing.fit_segments(n[b], seg[b], tg[b])[0] for b in range(B)])
    _check_against_definition(got, plain, n, want, (tag, "segments"))
    for b in range(B):
        assert np.array_equal(want[b][seg[b] == -1], n[b][seg[b] == -1])
        ties += sum(_tied_at_cut(n[b][seg[b] == g], int(tg[b, g])) for g in range(3))
    assert ties > 0, "no case cut between tied remainders: the index rule went untested"


# ---- 2. a fitted run is teacher forcing with the fitted durations, bit for bit

@pytest.mark.parametrize("tag,T", [("3x20", 256), ("4x70", 640)])
def test_fit_equals_teacher_forcing_bitwise(fixture, tag, T):
    model, (texts, src, spk) = fixture[3], _shapes(fixture)[tag]
    _, n = _plain(fixture, tag)
    B, L = n.shape
    seg = _segments(_np(src), L)
    Sg = np.stack([[n[b][seg[b] == g].sum() for g in range(3)] for b in range(B)])
    tg = np.stack([2 * Sg[:, 0] + 1, np.maximum(1, Sg[:, 1] - 3), Sg[:, 2] + 4], 1)
    fitted = np.stack([timing.fit_segments(n[b], seg[b], tg[b])[0] for b in range(B)])
    assert fitted.sum(1).max() <= T and not np.array_equal(fitted, n)
    got = _run(model, texts, src, spk, 7, T, target_frames=torch.from_numpy(tg), segments=torch.from_numpy(seg))
    ref = _run(model, texts, src, spk, 7, T, d_targets=torch.from_numpy(fitted.astype(np.float32)))
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (tag, k)


# ---- 3. an utterance with its target inside a batch is that utterance alone

def test_target_inside_a_batch_equals_alone_bitwise(fixture):
    model = fixture[3]
    frame_keys = ("mel2ph", "cwt_out", "f0_denorm", "p_idx", "cond", "mel")
    for tag, T in (("3x20", 256), ("6x33", 512)):
        texts, src, spk = _shapes(fixture)[tag]
        _, n = _plain(fixture, tag)
        B = n.shape[0]
        S = n.sum(1)
        tf = np.asarray([S[b] + (b + 1) * 7 if b % 2 == 0 else max(1, S[b] - 5 - b) for b in range(B)], np.int64)
        got = _run(model, texts, src, spk, 11, T, target_frames=torch.from_numpy(tf))
        assert np.array_equal(got["mel_len"], tf) and tf.max() <= T
        for b in range(B):
            only = -np.ones(B, np.int64)
            only[b] = tf[b]                   # the same batch, this utterance's target alone
            one = _run(model, texts, src, spk, 11, T, target_frames=torch.from_numpy(only))
            assert one["mel_len"][b] == tf[b]
            for k in ("log_d", "d_rounded", "e_pred", "e_idx"):
                assert np.array_equal(got[k][b], one[k][b]), (tag, b, k)
            for k in frame_keys:
                assert np.array_equal(got[k][b, :tf[b]], one[k][b, :tf[b]]), (tag, b, k)
            # ... and as a batch of one: the integer outputs of the text side
            solo = _text(model, (texts[b:b + 1], src[b:b + 1], spk[b:b + 1]), target_frames=torch.from_numpy(tf[b:b + 1]))
            assert np.array_equal(solo["d_rounded"][0], got["d_rounded"][b]) and solo["mel_len"][0] == tf[b], (tag, b)
            assert np.array_equal(solo["mel2ph"][0], got["mel2ph"][b, :tf[b]]), (tag, b)


# ---- 4. behind a duration table: the fit apportions the controlled integers

def test_fit_behind_a_duration_table(fixture):
    model, batch = fixture[3], _shapes(fixture)["3x20"]
    B, L = batch[0].shape
    D = torch.from_numpy(np.random.RandomState(4).uniform(0.5, 2.0, size=(B, L)).astype(np.float32))
    table = _text(model, batch, d_control=D)
    assert (table["d_rounded"] != np.floor(table["d_rounded"])).any()          # fractional: the fit takes int()
    n = table["d_rounded"].astype(np.int64)
    assert not np.array_equal(n, _plain(fixture, "3x20")[1])
    tf = n.sum(1) * 3 // 2 + 1
    got = _text(model, batch, d_control=D, target_frames=torch.from_numpy(tf))
    want = np.stack([timing.fit_segments(n[b], None, [tf[b]])[0] for b in range(B)])
    _check_against_definition(got, table, n, want, "table")
    # relative emphasis survives: a phoneme the table stretched stays longer than one it shrank
    b = 0
    hi, lo = int(np.argmax(n[b])), int(np.argmin(np.where(n[b] > 0, n[b], 1 << 30)))
    assert want[b, hi] > want[b, lo]


# ---- 5. refusals

def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_c_abi_refusals(fixture):
    g, cfg, _, model = fixture
    lib = model.lib
    texts, src, spk = (torch.from_numpy(g[k]).to(DEV) for k in ("texts", "src_lens", "spker_embeds"))
    B, L = texts.shape
    tgt = torch.full((B,), 50, dtype=torch.int32, device=DEV)
    dtg = torch.full((B, L), 2.0, device=DEV)
    nb = lib.cmtts_text_workspace_bytes(model._h, B, L)
    tws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    mel_len = torch.empty(B, dtype=torch.int64, device=DEV)
    call = lambda: lib.cmtts_text_forward(model._h, texts.data_ptr(), src.data_ptr(), spk.data_ptr(), None, B, L, 1.0, None, None,
                                          mel_len.data_ptr(), None, None, None, None, tws.data_ptr(), nb, _stream())
    dt = _lib.DurationTargetsStruct(seg=None, target=tgt.data_ptr(), unmet=None, ld=L, n_seg=1)
    try:
        _lib.check(lib.cmtts_set_duration_targets(model._h, C.byref(dt)))
        assert call() == 0
        torch.cuda.synchronize()
        assert mel_len.tolist() == [50] * B
        vc = _lib.VarianceControlsStruct(p_control=1.0, e_control=1.0, d_target=dtg.data_ptr())
        _lib.check(lib.cmtts_set_variance_controls(model._h, C.byref(vc)))
        assert call() == -1 and b"nothing to fit" in lib.cmtts_last_error()
        lib.cmtts_set_variance_controls(model._h, None)
        dt.ld = L + 1
        _lib.check(lib.cmtts_set_duration_targets(model._h, C.byref(dt)))
        assert call() == -1 and b"row pitch" in lib.cmtts_last_error()
        _lib.check(lib.cmtts_set_duration_targets(model._h, None))
        assert call() == 0
        torch.cuda.synchronize()
        assert mel_len.tolist() == _plain(fixture, "3x20")[0]["mel_len"].tolist()
    finally:
        lib.cmtts_set_variance_controls(model._h, None)
        lib.cmtts_set_duration_targets(model._h, None)
        torch.cuda.synchronize()
    with pytest.raises(ValueError, match="d_targets"):
        model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, target_frames=tgt, d_targets=dtg)


def test_unmet_segment_raises_and_spares_the_others(fixture):
    model, batch = fixture[3], _shapes(fixture)["3x20"]
    _, n = _plain(fixture, "3x20")
    B, L = n.shape
    src = _np(batch[1])
    seg = _segments(src, L)
    D = torch.ones(B, L)
    D[1][torch.from_numpy(seg[1] == 1)] = 0.0          # utterance 1, segment 1: durations of 0 frames only
    n0 = n.copy()
    n0[1][seg[1] == 1] = 0
    tg = np.stack([[int(n0[b][seg[b] == 0].sum()) + 3, 5, int(n0[b][seg[b] == 2].sum()) + 1] for b in range(B)])
    kw = dict(d_control=D, target_frames=torch.from_numpy(tg), segments=torch.from_numpy(seg))
    with pytest.raises(ValueError, match="utterance 1"):
        _text(model, batch, **kw)
    got = _text(model, batch, max_mel_len=256, **kw)          # T fixed: no read-back, the counts come back instead
    assert got["unmet"].tolist() == [0, 1, 0]
    fits = [timing.fit_segments(n0[b], seg[b], tg[b]) for b in range(B)]
    assert [u for _, u in fits] == [0, 1, 0]
    want = np.stack([f for f, _ in fits])
    assert not want[1][seg[1] == 1].any() and want[1][seg[1] == 0].sum() == tg[1, 0]
    np.testing.assert_array_equal(got["d_rounded"], want.astype(np.float32))
    np.testing.assert_array_equal(got["mel_len"], want.sum(1))
    np.testing.assert_array_equal(got["mel2ph"], _mel2ph(want, 256))


# ---- 6. nothing sticks

def test_nothing_sticks(fixture):
    model = fixture[3]
    for tag, T in (("3x20", 256), ("4x70", 640)):
        texts, src, spk = _shapes(fixture)[tag]
        _, n = _plain(fixture, tag)
        before = _run(model, texts, src, spk, 5, T)
        np.testing.assert_array_equal(before["d_rounded"].astype(np.int64), n)
        fitted = _run(model, texts, src, spk, 5, T, target_frames=torch.from_numpy(n.sum(1) + 9))
        assert np.array_equal(fitted["mel_len"], n.sum(1) + 9)
        after = _run(model, texts, src, spk, 5, T)
        for k in before:
            assert np.array_equal(before[k], after[k]), (tag, k)


# ---- 7. marks

@pytest.mark.parametrize("tag", ["3x20", "4x70"])
def test_marks(fixture, tag):
    host, model, batch = _host(), fixture[3], _shapes(fixture)[tag]
    _, n = _plain(fixture, tag)
    B, L = n.shape
    src = _np(batch[1])
    seg = _segments(src, L)
    tg = np.stack([[int(n[b][seg[b] == g].sum()) + 2 * g + 1 for g in range(3)] for b in range(B)])
    got = _text(model, batch, target_frames=torch.from_numpy(tg), segments=torch.from_numpy(seg))
    out, d, T = got["out"], got["d_rounded"], got["mel2ph"].shape[1]
    Tclip = int(got["mel_len"].min()) - 3
    assert 0 < Tclip < got["mel_len"].min()
    clipped = _text(model, batch, max_mel_len=Tclip, target_frames=torch.from_numpy(tg), segments=torch.from_numpy(seg))
    for rate in (22050, 8000):
        up, down = resample.ratio(22050, rate)
        assert (up, down) == ((1, 1) if rate == 22050 else (160, 441))
        for Tm, mel2ph in ((None, got["mel2ph"]), (T, got["mel2ph"]), (Tclip, clipped["mel2ph"])):
            marks = _np(host.phoneme_marks(out, T=Tm, sample_rate=None if rate == 22050 else rate))
            assert marks.dtype == np.int32 and marks.shape == (B, L, 4)
            for b in range(B):
                np.testing.assert_array_equal(marks[b], timing.phoneme_marks(d[b], src[b], Tm or 0, HOP, up, down), err_msg=str((rate, Tm, b)))
                # frame t lies in [start_l, end_l) exactly when the device's mel2ph[t] - 1 == l
                width = mel2ph.shape[1]
                want = np.zeros(width, np.int64)
                for l in range(L):
                    assert not want[marks[b, l, 0]:marks[b, l, 1]].any()
                    want[marks[b, l, 0]:marks[b, l, 1]] = l + 1
                np.testing.assert_array_equal(mel2ph[b], want)
                end = min(int(got["mel_len"][b]), Tm) if Tm else int(got["mel_len"][b])
                assert marks[b, -1, 1] == end and marks[b, -1, 3] == resample.out_len(end * HOP, up, down)
    # the definition's sample columns at the two ratios, spelled out
    assert timing.phoneme_marks(np.asarray([3.0]), 1, 0, HOP, 160, 441)[0].tolist() == [0, 3, 0, -(-3 * HOP * 160 // 441)]


# ---- 8. streamed PCM of an exact length, with marks

def test_stream_hits_the_target_and_reports_marks():
    from test_gpu_stream import _stitch, _voc
    host = _host()
    cfg = get_config("VCTK")
    seed = 2
    sd = synth_cmtts_state_dict(cfg, seed=seed, dur_frames=5.0, dur_spread=0.3)
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(sd)
    rs = np.random.RandomState(seed)
    B, L = 2, 14
    src = np.asarray([L, 9], np.int64)
    texts = np.zeros((B, L), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = torch.from_numpy(rs.standard_normal((B, cfg.external_speaker_dim)).astype(np.float32))
    texts, src = torch.from_numpy(texts), torch.from_numpy(src)
    plain = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk)["mel_lens"].cpu().tolist()
    tf = [timing.frames_for_seconds(1.0), 37]
    assert tf[0] == 86 and tf != plain
    target = torch.tensor(tf)

    class Gen:
        def __init__(self):
            self.g = torch.Generator().manual_seed(seed)

        def randn(self, *shape, **kw):
            return torch.randn(*shape, generator=self.g).to(DEV)

        def randn_like(self, x):
            return self.randn(*x.shape)

    voc, _, _ = _voc()
    voc.set_option("winograd", 0)          # the direct fp32 form: streamed chunks are bitwise the one-shot output (tests/test_gpu_stream.py)
    res = host.CMTotalTTSSynthesize.from_model(model, T=N_STEPS, generator=Gen()).synthesize((None, None, None, texts, src, L, spk), target_frames=target)
    assert res[11].cpu().tolist() == tf
    ref = host.vocoder_infer(res[0].transpose(1, 2), voc, lengths=[n * HOP for n in tf])
    events = []
    it = host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=N_STEPS, generator=Gen(), chunk_frames=(8, 16),
                                target_frames=target, on_marks=lambda m: events.append(("marks", m)))

    def tap():
        for item in it:
            events.append(("chunk", item[0]))
            yield item
    got, _ = _stitch(tap(), tf)
    assert [e[0] for e in events].count("marks") == 1 and events[0][0] == "marks"          # once, before the first chunk
    marks = events[0][1]
    assert isinstance(marks, np.ndarray) and marks.dtype == np.int32 and marks.shape == (B, L, 4)
    for b in range(B):
        assert len(got[b]) == resample.out_len(tf[b] * HOP, 1, 1) == tf[b] * HOP
        assert np.array_equal(got[b], ref[b]), b
        assert marks[b, -1, 3] == len(got[b]) and marks[b, -1, 1] == tf[b]
    # another output rate: the marks are in the stream's own samples
    up, down = resample.ratio(22050, 8000)
    seen, total = [], [0] * B
    for b, off, pcm, last in host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=N_STEPS, generator=Gen(),
                                                    chunk_frames=(8, 16), target_frames=target, sample_rate=8000, on_marks=seen.append):
        assert len(seen) == 1 and off == total[b]
        total[b] += len(pcm)
    for b in range(B):
        assert total[b] == resample.out_len(tf[b] * HOP, up, down) == seen[0][b, -1, 3]
        np.testing.assert_array_equal(seen[0][b], timing.phoneme_marks(marks[b, :, 1] - marks[b, :, 0], int(src[b]), 0, HOP, up, down))


# ---- 9. virtual sharded worlds: the fitted lengths travel in the records

def test_sharded_targets_travel_with_the_utterance(fixture):
    _, cfg, _, model = fixture
    host = _host()
    n, L = 10, 24
    texts, src, spk = _batch(cfg, n, L, seed=41)
    assert int(src.max()) == L
    buckets = (128, 256)
    plain = _text(model, (texts, src, spk))
    nd = plain["d_rounded"].astype(np.int64)
    S = nd.sum(1)
    tf = np.where(np.arange(n) % 3 == 2, -1, S + (np.arange(n) % 5) * 4 - 6)
    assert (tf[tf >= 0] >= 1).all() and max(tf.max(), S.max()) <= max(buckets)          # nothing is truncated at the largest bucket
    ctl = {"target_frames": torch.from_numpy(tf)}
    want_len = np.where(tf >= 0, tf, S).tolist()
    ref = _virtual_world(model, texts, src, spk, 1, buckets, ctl)
    assert ref["mel_len"] == want_len and want_len != S.tolist()
    fitted = np.stack([timing.fit_segments(nd[i], None, [tf[i]])[0] for i in range(n)])
    for i in range(n):
        assert np.array_equal(_np(ref["mel2ph"][i])[:want_len[i]], _mel2ph(fitted[i:i + 1], want_len[i])[0]), i
    got = _virtual_world(model, texts, src, spk, 2, buckets, ctl)
    assert torch.equal(got["records"], ref["records"]) and got["mel_len"] == ref["mel_len"]
    for i in range(n):
        for k in ("mel2ph", "cwt", "p_idx", "mels"):
            assert torch.equal(got[k][i], ref[k][i]), (i, k)
    out = host.synthesize_sharded(model, texts, src, spker_embeds=spk, n_steps=N_STEPS, seed=5, buckets=buckets, **ctl)
    assert out["mel_len"] == want_len
    for i in range(n):
        assert out["mels"][i].shape[0] == want_len[i] and torch.equal(out["mels"][i], ref["mels"][i]), i


# ---- 10. the kernel alone at the lengths the text side accepts (the reference's max_seq_len is 1000): a lane per phoneme at
# L = 1000, more phonemes than lanes at L = 1500; many segments, zeros mixed in, empty and unmeetable segments

@pytest.mark.parametrize("L,G", [(1000, 1), (1000, 37), (1500, 200)])
def test_kernel_alone_at_long_lengths(L, G):
    rs = np.random.RandomState(L + G)
    B = 3
    n = rs.randint(0, 12, size=(B, L)).astype(np.int64)
    n[rs.rand(B, L) < 0.25] = 0
    src = np.asarray([L, L - 1, L // 2 + 1], np.int64)
    seg = None if G == 1 else rs.randint(-1, G, size=(B, L)).astype(np.int32)
    if G > 1:
        seg[:, :64][seg[:, :64] == 3] = 4          # segment 3 starts behind the first wave
        n[1][seg[1] == 5] = 0                      # utterance 1, segment 5: only zeros
        seg[2][seg[2] == 7] = -1                   # utterance 2, segment 7: no phoneme at all
    tgt = np.stack([[rs.randint(0, 3 * max(1, int(n[b, :src[b]][(seg[b, :src[b]] == g) if G > 1 else slice(None)].sum())) + 3) for g in range(G)]
                    for b in range(B)]).astype(np.int32)
    tgt[rs.rand(B, G) < 0.15] = -1
    if G > 1:
        tgt[1, 5], tgt[2, 7] = 9, 4
    d = torch.from_numpy(n.astype(np.float32)).to(DEV)
    cum = torch.empty(B, L, dtype=torch.int32, device=DEV)
    mel_len = torch.empty(B, dtype=torch.int64, device=DEV)
    sl, tg = torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV)
    sg = None if seg is None else torch.from_numpy(seg).to(DEV)
    unmet = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.internal_duration_fit(d.data_ptr(), cum.data_ptr(), mel_len.data_ptr(), sl.data_ptr(), None if sg is None else sg.data_ptr(),
                                          tg.data_ptr(), unmet.data_ptr(), B, L, G, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for b in range(B):
        s = np.full(L, -1, np.int64)
        s[:src[b]] = 0 if seg is None else seg[b, :src[b]]          # entries at l >= src_len are ignored
        want, want_unmet = timing.fit_segments(n[b], s, tgt[b])
        np.testing.assert_array_equal(_np(d[b]), want.astype(np.float32), err_msg=str(b))
        np.testing.assert_array_equal(_np(cum[b]), np.cumsum(want), err_msg=str(b))
        assert int(mel_len[b]) == want.sum() and int(unmet[b]) == want_unmet, b
    if G > 1:
        assert int(unmet[1]) >= 1 and int(unmet[2]) >= 1
