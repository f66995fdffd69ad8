"""Duration targets and phoneme marks, CPU side (no compute calls): the definition in cmtts_amd/timing.py — its four properties over
random cases, the segment form against an independent one-frame-at-a-time apportionment, the tie rule, the marks against the
oracle's dur_to_mel2ph — the host's refusals before anything launches, and the two entry points (cmtts_set_duration_targets,
cmtts_phoneme_marks).  The GPU tests in tests/test_gpu_duration_fit.py hold the kernels to this definition."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib, resample, timing
from cmtts_amd.config import get_config
from oracle import cmtts_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_durations(rs, L):
    n = rs.randint(0, 12, size=L).astype(np.int64)
    n[rs.rand(L) < 0.25] = 0          # zeros mixed in
    return n


# ---- 1. the four properties

def test_fit_properties_over_random_cases():
    rs = np.random.RandomState(0)
    nonzero_total = 0
    for _ in range(20000):
        L = rs.randint(1, 130)
        n = _random_durations(rs, L)
        S = int(n.sum())
        t = rs.randint(0, 4 * S + 5)
        out = timing.fit_durations(n, t)
        assert out.dtype == np.int64 and out.shape == n.shape
        if S == 0:
            assert np.array_equal(out, n)
            continue
        nonzero_total += 1
        assert int(out.sum()) == t
        assert not out[n == 0].any()
        assert (out >= 0).all()
        # |result - n t / S| < 1, exactly: |result S - n t| < S
        assert (np.abs(out * S - n * t) < S).all()
        assert np.array_equal(timing.fit_durations(n, S), n)
    assert nonzero_total > 19000
    n = np.asarray([3, 0, 5], np.int64)
    assert np.array_equal(timing.fit_durations(n, -1), n) and timing.fit_durations(n, -1) is not n
    assert np.array_equal(timing.fit_durations(np.zeros(4, np.int64), 7), np.zeros(4, np.int64))
    assert timing.fit_durations(n, 0).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        timing.fit_durations(np.asarray([1, -1]), 3)


# ---- 2. the segment form against an independent apportionment

def _brute_force(n, t):
    """Frames handed out one at a time to the phoneme with the largest deficit n t / S - given (ties to the lower index), starting
    from the floors: Hamilton's method without remainders or sorting, in exact fractions."""
    S = int(n.sum())
    quota = [Fraction(int(v) * t, S) for v in n]
    out = [q.numerator // q.denominator for q in quota]
    while sum(out) < t:
        deficit = [q - o for q, o in zip(quota, out)]
        out[max(range(len(n)), key=lambda i: (deficit[i], -i))] += 1
    return np.asarray(out, np.int64)


def test_segments_against_brute_force():
    rs = np.random.RandomState(1)
    unmet_seen = left_alone = 0
    for _ in range(300):
        L = rs.randint(1, 60)
        G = rs.randint(1, 6)
        n = _random_durations(rs, L)
        seg = rs.randint(-1, G, size=L)
        targets = np.asarray([rs.randint(0, 3 * max(1, int(n[seg == g].sum())) + 3) for g in range(G)], np.int64)
        targets[rs.rand(G) < 0.2] = -1
        got, unmet = timing.fit_segments(n, seg, targets)
        want, want_unmet = n.copy(), 0
        for g in range(G):
            idx = np.flatnonzero(seg == g)
            if targets[g] < 0:
                left_alone += 1
            elif n[idx].sum() == 0:
                want_unmet += int(targets[g] > 0)
            else:
                want[idx] = _brute_force(n[idx], int(targets[g]))
        assert np.array_equal(got, want) and unmet == want_unmet
        assert np.array_equal(got[seg == -1], n[seg == -1])
        unmet_seen += unmet
    assert unmet_seen > 0 and left_alone > 0
    # the utterance-level form: one segment that holds every phoneme
    n = np.asarray([4, 0, 3, 5], np.int64)
    got, unmet = timing.fit_segments(n, None, [30])
    assert np.array_equal(got, timing.fit_durations(n, 30)) and unmet == 0 and got.sum() == 30
    assert timing.fit_segments(np.zeros(3, np.int64), None, [2]) [1] == 1
    assert timing.fit_segments(np.zeros(3, np.int64), None, [0])[1] == 0
    assert timing.fit_segments(n, np.asarray([0, 0, -1, -1]), [8, 5])[1] == 1          # segment 1 holds no phoneme at all
    with pytest.raises(ValueError):
        timing.fit_segments(n, None, [3, 4])
    with pytest.raises(ValueError):
        timing.fit_segments(n, np.asarray([0, 1, 2, 0]), [3, 4])


def test_ties_go_to_the_lower_index():
    n = np.full(5, 4, np.int64)          # S = 20
    assert timing.fit_durations(n, 22).tolist() == [5, 5, 4, 4, 4]          # r = 8 everywhere, R = 2
    assert timing.fit_durations(n, 19).tolist() == [4, 4, 4, 4, 3]          # r = 16 everywhere, R = 4
    n = np.asarray([4, 2, 4, 0, 2], np.int64)          # S = 12, t = 15: q = 60 30 60 0 30, a = 5 2 5 0 2, r = 0 6 0 0 6, R = 1
    assert timing.fit_durations(n, 15).tolist() == [5, 3, 5, 0, 2]
    seg = np.asarray([1, 0, 1, 0, 1, 0])
    got, _ = timing.fit_segments(np.full(6, 2, np.int64), seg, [7, 8])       # each: S = 6; t = 7: r = 2, R = 1; t = 8: r = 4, R = 2
    assert got.tolist() == [3, 3, 3, 2, 2, 2]


# ---- 3. marks

def test_marks_against_dur_to_mel2ph():
    rs = np.random.RandomState(2)
    for case in range(40):
        L = rs.randint(1, 40)
        src_len = rs.randint(1, L + 1)
        d = _random_durations(rs, L).astype(np.float32)
        d[src_len:] = 0
        total = int(d.sum())
        up, down = resample.ratio(22050, (22050, 8000, 16000, 48000)[case % 4])
        for T in (0, max(1, total // 2), total + 3):
            marks = timing.phoneme_marks(d, src_len, T, 256, up, down)
            assert marks.dtype == np.int32 and marks.shape == (L, 4)
            width = T if T > 0 else max(total, 1)
            mask = (np.arange(L) >= src_len)[None]
            mel2ph = O.dur_to_mel2ph(d[None], mask, width)[0]
            for t in range(width):
                inside = [l for l in range(L) if marks[l, 0] <= t < marks[l, 1]]
                assert inside == ([int(mel2ph[t]) - 1] if mel2ph[t] > 0 else []), (case, T, t)
            end = min(total, T) if T > 0 else total
            assert (marks[src_len - 1:, 1] == end).all() and (marks[src_len:, 0] == end).all()
            assert marks[0, 0] == 0 and (marks[1:, 0] == marks[:-1, 1]).all()
            for col in (0, 1):
                want = [resample.out_len(int(f) * 256, up, down) for f in marks[:, col]]
                assert marks[:, col + 2].tolist() == want
    # fractional durations: the integer part counts, like the length regulator
    m = timing.phoneme_marks(np.asarray([2.6, 1.5, 0.9], np.float32), 3)
    assert m[:, :2].tolist() == [[0, 2], [2, 3], [3, 3]] and m[:, 3].tolist() == [512, 768, 768]


def test_frames_for_seconds():
    assert timing.frames_for_seconds(3.2) == round(3.2 * 22050 / 256) == 276
    assert timing.frames_for_seconds(1.0, 16000, 200) == 80
    assert timing.frames_for_seconds(1e-4) == 1
    for sec in np.random.RandomState(3).uniform(0.05, 20.0, 200):
        f = timing.frames_for_seconds(sec)
        assert abs(f * 256 / 22050 - sec) <= 0.5 * 256 / 22050 + 1e-12          # within half a frame
    assert "half a frame" in timing.frames_for_seconds.__doc__.lower().replace("\n", " ")
    with pytest.raises(ValueError):
        timing.frames_for_seconds(0)


def test_timing_imports_no_torch_at_module_level():
    src = open(os.path.join(ROOT, "cm-tts_amd", "timing.py")).read()
    assert not re.search(r"^\s*(import|from)\s+torch", src, flags=re.M)


# ---- 4. the entry points

def test_entry_points_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "cmtts_hip.h")).read()
    assert re.search(r"int cmtts_set_duration_targets\(cmtts_model\* m, const cmtts_duration_targets\* t\);", text)
    assert re.search(r"int cmtts_phoneme_marks\(const float\* d_rounded, const int64_t\* src_lens, int B, int L, int T,?\s+int hop, int up, "
                     r"int down,\s+int32_t\* marks, void\* stream\);", text)
    body = re.search(r"typedef struct cmtts_duration_targets \{(.*?)\} cmtts_duration_targets;", text, flags=re.S).group(1)
    names = [n for decl in re.findall(r"(?:const int32_t\*|int32_t\*|int)\s+([a-z_, ]+);", body) for n in re.split(r",\s*", decl)]
    assert names == [n for n, _ in _lib.DurationTargetsStruct._fields_] == ["seg", "target", "unmet", "ld", "n_seg"]
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cmtts_set_duration_targets", "cmtts_phoneme_marks"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cmtts_abi_version() == 8 and _lib.ABI_VERSION == 8          # entry points only: the revision stays
    assert lib.cmtts_set_duration_targets(None, None) == -1
    assert b"cmtts_set_duration_targets" in lib.cmtts_last_error() and b"null" in lib.cmtts_last_error()
    assert lib.cmtts_phoneme_marks(None, None, 1, 1, 0, 256, 1, 1, None, None) == -1
    assert b"cmtts_phoneme_marks" in lib.cmtts_last_error()
    assert lib.cmtts_phoneme_marks(0x1000, 0x1000, 1, 1, 0, 256, 1, 0, 0x1000, None) == -1          # down = 0


def test_targets_on_a_created_model():
    from cmtts_amd import host
    model = host.CMTotalTTS(get_config("VCTK"), "cpu")          # cmtts_create only: the targets live on the handle
    lib = model.lib
    mk = lambda **kw: _lib.DurationTargetsStruct(**{**dict(seg=None, target=0x1000, unmet=None, ld=20, n_seg=1), **kw})
    assert lib.cmtts_set_duration_targets(model._h, C.byref(mk())) == 0
    assert lib.cmtts_set_duration_targets(model._h, C.byref(mk(seg=0x1000, n_seg=5))) == 0
    for bad, word in ((mk(target=None), b"target"), (mk(ld=0), b"ld"), (mk(n_seg=0), b"n_seg"), (mk(n_seg=3), b"n_seg")):
        assert lib.cmtts_set_duration_targets(model._h, C.byref(bad)) == -1 and word in lib.cmtts_last_error()
    assert lib.cmtts_set_duration_targets(model._h, None) == 0               # NULL clears


# ---- 5. host validation, before anything launches (a create-only model cannot launch anything)

def _bad_targets(B, L):
    seg = torch.zeros(B, L, dtype=torch.int64)
    high = seg.clone(); high[1, 3] = 2
    low = seg.clone(); low[0, 0] = -2
    return [
        ("segments without targets", dict(segments=seg)),
        ("wrong shape [B + 1]", dict(target_frames=torch.ones(B + 1, dtype=torch.int64))),
        ("[B, G] without segments", dict(target_frames=torch.ones(B, 2, dtype=torch.int64))),
        ("[B] beside segments", dict(target_frames=torch.ones(B, dtype=torch.int64), segments=seg)),
        ("segments [B, L + 1]", dict(target_frames=torch.ones(B, 2, dtype=torch.int64), segments=torch.zeros(B, L + 1, dtype=torch.int64))),
        ("float targets", dict(target_frames=torch.ones(B))),
        ("float segments", dict(target_frames=torch.ones(B, 2, dtype=torch.int64), segments=seg.float())),
        ("a Python list", dict(target_frames=[10] * B)),
        ("target < -1", dict(target_frames=torch.tensor([10, -2, 10]))),
        ("target > 2^24", dict(target_frames=torch.tensor([10, (1 << 24) + 1, 10]))),
        ("segment >= G", dict(target_frames=torch.ones(B, 2, dtype=torch.int64), segments=high)),
        ("segment < -1", dict(target_frames=torch.ones(B, 2, dtype=torch.int64), segments=low)),
        ("beside d_targets", dict(target_frames=torch.full((B,), 50), d_targets=torch.ones(B, L))),
    ]


def test_host_refusals_raise_value_error():
    from cmtts_amd import host
    model = host.CMTotalTTS(get_config("VCTK"), "cpu")
    B, L = 3, 20
    texts = torch.ones(B, L, dtype=torch.int64)
    src = torch.tensor([20, 14, 9])
    spk = torch.zeros(B, model.config.external_speaker_dim)
    for what, kw in _bad_targets(B, L):
        with pytest.raises(ValueError):
            model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, **kw)
        if "d_targets" in kw:
            continue
        with pytest.raises(ValueError):
            next(host.synthesize_stream(model, None, texts, src, spker_embeds=spk, **kw))
        with pytest.raises(ValueError):
            host.synthesize_sharded(model, texts, src, spker_embeds=spk, **kw)
        with pytest.raises(ValueError):
            host.text_state_records(model, texts, src, 0, 2, spker_embeds=spk, **kw)
        with pytest.raises(ValueError):
            host.CMTotalTTSSynthesize.from_model(model, T=2).synthesize((None, None, None, texts, src, L, spk), **kw)
    with pytest.raises(ValueError):
        next(host.synthesize_stream(model, None, texts, src, spker_embeds=spk, on_marks=3))
    # valid targets pass validation and reach the model, which has no weights: the launch is what is refused
    ok = dict(target_frames=torch.tensor([[40, -1], [0, 1 << 24], [7, 7]]), segments=torch.randint(-1, 2, (B, L)))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, **ok)
    with pytest.raises(RuntimeError, match="load_state_dict"):
        host.CMTotalTTSSynthesize.from_model(model, T=2).synthesize((None, None, None, texts, src, L, spk), target_frames=torch.tensor([40, 41, -1]))
    tgt, seg = host._resolve_targets(B, L, np.asarray([40, -1, 12]), None)
    assert seg is None and tgt.dtype == torch.int32 and tgt.tolist() == [[40], [-1], [12]]
    tgt, seg = host._resolve_targets(B, L, **ok)
    assert tgt.shape == (B, 2) and seg.dtype == torch.int32 and seg.shape == (B, L) and seg.is_contiguous()
    assert host._resolve_targets(B, L) is None
