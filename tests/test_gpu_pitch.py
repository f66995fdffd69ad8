"""Pitch of a recording on the GPU (include/cmtts_hip.h: cmtts_pitch_nacf, cmtts_pitch_track, cmtts_pitch_targets; csrc/pitch.hip;
host.pitch_from_audio / pitch_targets): the autocorrelation against the float64 definition with the definition's own float32
arm as the yardstick; the tracker's path bit for bit the definition, on the device's own r and on hand-made matrices, NaN and infinities
included, across the frames the Viterbi kernel loads ahead and at 4096 frames; the targets against the definition; and the targets of
recordings teacher-forced into the model end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmtts_amd import _lib, pitch as P
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from conftest import load_golden, report
from oracle import cmtts_oracle as O
import pitch_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = P.default_geometry()

# The bounds of test_nacf_against_float64.  Yardstick: pitch.nacf(dtype=float32) — numpy's float32 mean, products and sums — against its float64
# arm on the rows of pitch_cases.rows(), absolute on r (which is normalised) and relative on pk, worst over the rows (measured with numpy 2.2:
# r 1.03e-6 / 2.43e-6 / 2.18e-6 / 0 / 2.27e-6, pk 3.5e-8 / 3.9e-8 / 4.3e-8 / 0 / 5.7e-8; the test prints the live figures).  The kernel gets 4 x
# that: its sums associate differently (fused chains of eight products, added up in double).  Measured on MI355X: see DESIGN §3.5k.
YARDSTICK_NACF = 2.43e-6
YARDSTICK_PK = 5.67e-8
# The bound of test_targets_against_the_definition.  Yardstick: pitch.cwt_direct(dtype=float32) — x, table and sums in float32 — against its
# float64 arm on the normalised contours of pitch_cases.contours(), relative to the row's largest |cwt|, worst over the rows (measured with
# numpy 2.2: 4.8e-8 .. 1.07e-7, the largest at 257 frames; the test prints the live figure).  The kernel gets 4 x that.
YARDSTICK_CWT = 1.07e-7

_CACHE = {}


def _host():
    from cmtts_amd import host
    return host


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _handle():
    if "h" not in _CACHE:
        h = C.c_void_p()
        _lib.check(_lib.load().cmtts_pitch_create(P.SAMPLE_RATE, P.HOP, P.FLOOR_HZ, P.CEILING_HZ, C.byref(h)))
        _CACHE["h"] = h
    return _CACHE["h"]


def _ws(B, T):
    nb = _lib.load().cmtts_pitch_workspace_bytes(B, T)
    assert nb > 0
    return torch.empty(nb, dtype=torch.uint8, device=DEV), nb


def _nacf_dev(wav, lens, T):
    """cmtts_pitch_nacf into NaN-filled buffers: (r, pk, frames) on the device."""
    wav = torch.from_numpy(np.ascontiguousarray(wav)).to(DEV)
    B, ld = wav.shape
    n_valid = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    r = torch.full((B, T, G.LMAX + 2), float("nan"), dtype=torch.float32, device=DEV)
    pk = torch.full((B, T), float("nan"), dtype=torch.float32, device=DEV)
    frames = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws, nb = _ws(B, T)
    _lib.check(_lib.load().cmtts_pitch_nacf(_handle(), _p(wav), int(wav.dtype == torch.int16), B, ld, _p(n_valid), T, _p(r), _p(pk), _p(frames), _p(ws),
                                            nb, _st()))
    torch.cuda.synchronize()
    _host().check_async_error()
    return r, pk, frames


def _track_dev(r, pk, frames):
    """cmtts_pitch_track into buffers filled with -7 / NaN: (lag, f0) on the device."""
    B, T, _ = r.shape
    lag = torch.full((B, T), -7, dtype=torch.int32, device=DEV)
    f0 = torch.full((B, T), float("nan"), dtype=torch.float32, device=DEV)
    fr = torch.as_tensor(np.asarray(frames, np.int32)).to(DEV) if not isinstance(frames, torch.Tensor) else frames
    ws, nb = _ws(B, T)
    ws.fill_(0xff)
    _lib.check(_lib.load().cmtts_pitch_track(_handle(), _p(r), _p(pk), _p(fr), B, T, _p(lag), _p(f0), _p(ws), nb, _st()))
    torch.cuda.synchronize()
    _host().check_async_error()
    return lag, f0


def _float_batch():
    """Rows 0-3 of pitch_cases.rows() in one NaN-padded batch, one frame more than the longest row has; the float64 definition once."""
    if "fb" not in _CACHE:
        rows = PC.rows()[:4]
        wav, lens = PC.batch(rows)
        T = max(r.T for r in rows) + 1
        ref = [P.nacf(r.wav) for r in rows]
        _CACHE["fb"] = (rows, wav, lens, T, ref)
    return _CACHE["fb"]


def _device_nacf():
    if "dn" not in _CACHE:
        rows, wav, lens, T, _ = _float_batch()
        _CACHE["dn"] = _nacf_dev(wav, lens, T)
    return _CACHE["dn"]


def _ulps(got, want):
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(1e-30))).astype(np.float64)


def _rel(got, want):
    """|got - want| / want where want > 0; where want is 0 (silence) got must be 0 too."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not got[want == 0].any()
    nz = want > 0
    return float((np.abs(got[nz] - want[nz]) / want[nz]).max()) if nz.any() else 0.0


def test_nacf_against_float64():
    rows, wav, lens, T, ref = _float_batch()
    r, pk, frames = (t.cpu().numpy() for t in _device_nacf())
    assert frames.tolist() == [row.T for row in rows]
    assert not np.isnan(r).any() and not np.isnan(pk).any()                # nothing of the NaN beyond n_valid comes out
    worst_r = worst_pk = yard_r = yard_pk = 0.0
    for b, row in enumerate(rows):
        r64, pk64 = ref[b]
        r32, pk32 = P.nacf(row.wav, dtype=np.float32)
        assert not r[b, row.T:].any() and not pk[b, row.T:].any()           # zeros at and beyond the row's frames
        worst_r = max(worst_r, float(np.abs(r[b, :row.T] - r64).max()))
        yard_r = max(yard_r, float(np.abs(r32 - r64).max()))
        worst_pk = max(worst_pk, _rel(pk[b, :row.T], pk64))
        yard_pk = max(yard_pk, _rel(pk32, pk64))
        if not pk64.any():
            assert not r[b].any()
    report(f"PITCH nacf vs float64: r {worst_r:.3e} (float32 definition {yard_r:.3e}, bound {4 * YARDSTICK_NACF:.3e}), "
           f"pk {worst_pk:.3e} (float32 definition {yard_pk:.3e}, bound {4 * YARDSTICK_PK:.3e})")
    assert worst_r <= 4 * YARDSTICK_NACF and worst_pk <= 4 * YARDSTICK_PK


def test_nacf_row_alone_and_int16():
    rows, wav, lens, T, _ = _float_batch()
    r, pk, _ = _device_nacf()
    row = rows[2]
    r1, pk1, f1 = _nacf_dev(wav[2:3, :row.n + 3], [row.n], row.T)          # another T, another ld, another batch: the same bits
    assert f1.tolist() == [row.T]
    assert torch.equal(r1[0], r[2, :row.T]) and torch.equal(pk1[0], pk[2, :row.T])
    i16 = PC.rows()[4]
    pcm = np.zeros((1, i16.n + 5), np.int16)
    pcm[0, :i16.n] = i16.pcm
    pcm[0, i16.n:] = 32767
    ri, pki, _ = _nacf_dev(pcm, [i16.n], i16.T)
    flt = np.full((1, i16.n + 5), np.nan, np.float32)
    flt[0, :i16.n] = i16.pcm.astype(np.float32) / np.float32(32768.0)
    rf, pkf, _ = _nacf_dev(flt, [i16.n], i16.T)
    assert torch.equal(ri, rf) and torch.equal(pki, pkf)
    r64, pk64 = P.nacf(i16.pcm)
    assert np.abs(ri[0].cpu().numpy() - r64).max() <= 4 * YARDSTICK_NACF
    assert _rel(pki[0].cpu().numpy(), pk64) <= 4 * YARDSTICK_PK


def _same_path(r_host, pk_host, frames, lag, f0, tag):
    lag, f0 = lag.cpu().numpy(), f0.cpu().numpy()
    for b, n in enumerate(frames):
        want_lag, want_f0 = P.track(np.ascontiguousarray(r_host[b, :n]), np.ascontiguousarray(pk_host[b, :n]))
        np.testing.assert_array_equal(lag[b, :n], want_lag, err_msg=f"{tag} row {b}")
        assert not lag[b, n:].any() and not f0[b, n:].any(), f"{tag} row {b}: not zero beyond its frames"
        assert ((f0[b, :n] > 0) == (want_lag > 0)).all() and not np.isnan(f0[b]).any()
        v = want_lag > 0
        if v.any():
            assert _ulps(f0[b, :n][v], want_f0[v]).max() <= 2, f"{tag} row {b}"


def test_track_on_the_device_r_is_the_definition():
    rows, wav, lens, T, _ = _float_batch()
    r, pk, frames = _device_nacf()
    lag, f0 = _track_dev(r, pk, frames)
    _same_path(r.cpu().numpy(), pk.cpu().numpy(), [row.T for row in rows], lag, f0, "rows")
    # and what it found: the rows' own f0 (the CPU test's bound is on the float64 r; the path is the same)
    f0 = f0.cpu().numpy()
    for b, row in enumerate(rows):
        want = P.track(*(a.astype(np.float32) for a in P.nacf(row.wav)))[0]
        np.testing.assert_array_equal(lag[b, :row.T].cpu().numpy(), want, err_msg=row.name)
    # a row alone equals the row in the batch
    l1, f1 = _track_dev(r[2:3, :rows[2].T].contiguous(), pk[2:3, :rows[2].T].contiguous(), [rows[2].T])
    assert torch.equal(l1[0], lag[2, :rows[2].T]) and np.array_equal(f1[0].cpu().numpy(), f0[2, :rows[2].T])


@pytest.mark.parametrize("name", sorted(PC.handmade()))
def test_track_handmade_is_the_definition(name):
    r, pk = PC.handmade()[name]
    T = r.shape[0]
    rb = np.full((2, T + 3, r.shape[1]), np.nan, np.float32)                # the same matrix twice, once shortened by a frame
    pb = np.full((2, T + 3), np.nan, np.float32)
    rb[:, :T], pb[:, :T] = r, pk
    frames = [T, max(T - 1, 0)]
    lag, f0 = _track_dev(torch.from_numpy(rb).to(DEV), torch.from_numpy(pb).to(DEV), frames)
    _same_path(rb, pb, frames, lag, f0, name)


def test_track_long_rows():
    """More frames than the Viterbi kernel loads ahead (8) and than a wave has lanes, a length that is no multiple of either, and the most
    a row may have; the shorter row alone equals the row in the batch."""
    T = P.MAX_FRAMES
    ra, pa = PC.long_r(T, 1)
    rb_, pb_ = PC.long_r(701, 2)
    r = np.full((2, T, G.LMAX + 2), np.nan, np.float32)
    pk = np.full((2, T), np.nan, np.float32)
    r[0], pk[0] = ra, pa
    r[1, :701], pk[1, :701] = rb_, pb_
    frames = [T, 701]
    lag, f0 = _track_dev(torch.from_numpy(r).to(DEV), torch.from_numpy(pk).to(DEV), frames)
    _same_path(r, pk, frames, lag, f0, "long")
    assert 0.3 < float((lag[0] > 0).float().mean()) < 0.9                   # both voiced and unvoiced stretches were walked
    l1, f1 = _track_dev(torch.from_numpy(rb_[None]).to(DEV), torch.from_numpy(pb_[None]).to(DEV), [701])
    assert torch.equal(l1[0], lag[1, :701]) and torch.equal(f1[0], f0[1, :701])


def _targets_dev(f0, frames):
    B, T = f0.shape
    f0 = torch.from_numpy(f0).to(DEV)
    fr = torch.from_numpy(np.asarray(frames, np.int32)).to(DEV)
    cwt = torch.full((B, T, 10), float("nan"), dtype=torch.float32, device=DEV)
    mean = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    std = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    uv = torch.full((B, T), 7, dtype=torch.uint8, device=DEV)
    status = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ws, nb = _ws(B, T)
    _lib.check(_lib.load().cmtts_pitch_targets(_handle(), _p(f0), _p(fr), B, T, _p(cwt), _p(mean), _p(std), _p(uv), _p(status), _p(ws), nb, _st()))
    torch.cuda.synchronize()
    _host().check_async_error()
    return cwt.cpu().numpy(), mean.cpu().numpy(), std.cpu().numpy(), uv.cpu().numpy(), status.cpu().numpy()


def test_targets_against_the_definition():
    cs = PC.contours()
    frames = [c.shape[0] for c in cs]
    assert frames[:6] == list(PC.CONTOUR_FRAMES)
    T = max(frames) + 3
    f0 = np.full((len(cs), T), np.nan, np.float32)
    for b, c in enumerate(cs):
        f0[b, :c.shape[0]] = c
    cwt, mean, std, uv, status = _targets_dev(f0, frames)
    assert not np.isnan(cwt).any() and not np.isnan(mean).any() and not np.isnan(std).any()
    worst = yard = 0.0
    for b, c in enumerate(cs):
        n = frames[b]
        want = P.targets(c)
        assert status[b] == want["status"], b
        np.testing.assert_array_equal(uv[b, :n], want["uv"].astype(np.uint8))
        assert int((uv[b, :n] == 0).sum()) == int((c != 0).sum())            # the voiced count
        assert not uv[b, n:].any() and not cwt[b, n:].any()                   # zeros at and beyond the row's frames
        assert _ulps(mean[b], np.float32(want["f0_mean"])).max() <= 2 and _ulps(std[b], np.float32(want["f0_std"])).max() <= 2, b
        if want["status"] != 0:
            assert not cwt[b].any() and std[b] == 1.0
            continue
        x = (np.log(P.convert_continuos_f0(c)) - want["f0_mean"]) / want["f0_std"]
        d64 = P.cwt_direct(x)
        peak = np.abs(want["cwt_spec"]).max()
        worst = max(worst, float(np.abs(cwt[b, :n] - want["cwt_spec"]).max() / peak))
        yard = max(yard, float(np.abs(P.cwt_direct(x, np.float32) - d64).max() / np.abs(d64).max()))
    assert status.tolist()[6:] == [1, 2, 3]
    report(f"PITCH cwt vs float64: {worst:.3e} of the row's peak (float32 definition {yard:.3e}, bound {4 * YARDSTICK_CWT:.3e})")
    assert worst <= 4 * YARDSTICK_CWT
    # a row alone, in a buffer of its own length, equals the row in the batch
    c1, m1, s1, u1, st1 = _targets_dev(np.ascontiguousarray(f0[4:5, :33]), [33])
    assert np.array_equal(c1[0], cwt[4, :33]) and m1[0] == mean[4] and s1[0] == std[4] and np.array_equal(u1[0], uv[4, :33]) and st1[0] == 0


def test_targets_longest_row():
    """4096 frames: the largest table, every thread with 16 frames of its own."""
    n = P.MAX_FRAMES
    rng = np.random.default_rng(3)
    c = (150.0 * np.exp(0.3 * np.sin(np.arange(n) / 40.0) + 0.02 * rng.standard_normal(n))).astype(np.float32)
    c[:7] = 0
    c[1000:1300] = 0
    c[-1] = 0
    cwt, mean, std, uv, status = _targets_dev(c[None], [n])
    want = P.targets(c)
    assert status[0] == 0 and np.array_equal(uv[0], want["uv"].astype(np.uint8))
    assert _ulps(mean[0], np.float32(want["f0_mean"])).max() <= 2 and _ulps(std[0], np.float32(want["f0_std"])).max() <= 2
    assert np.abs(cwt[0] - want["cwt_spec"]).max() <= 4 * YARDSTICK_CWT * np.abs(want["cwt_spec"]).max()


def _model():
    if "model" not in _CACHE:
        g = load_golden("cmtts_VCTK")
        cfg = get_config("VCTK")
        sd = synth_cmtts_state_dict(cfg, seed=int(g["seed"]), dur_frames=4.0, dur_spread=0.03)
        _CACHE["model"] = (g, cfg, sd, _host().CMTotalTTS(cfg, DEV).load_state_dict(sd))
    return _CACHE["model"]


@pytest.mark.parametrize("which", [1, 2])
def test_pitch_targets_teacher_forced_end_to_end(which):
    """pitch_targets(wavs) goes unchanged into duration_pitch_energy_net(d_targets=, p_targets=) on the golden weights: f0_denorm is the
    oracle's on the same targets (the existing parity tolerance), 0 on the unvoiced frames, and on the voiced frames the tracked contour to
    within the reconstruction bound of the CPU test (asserted on the fully voiced glide; the mixed row's jump of an octave across an
    interpolated gap is beyond what ten scales give back)."""
    host = _host()
    g, cfg, sd, model = _model()
    assert cfg.use_uv
    row = PC.rows()[which]
    pt = host.get_pitch_tracker(device=DEV)
    wav = np.full((1, row.n + 9), np.nan, np.float32)
    wav[0, :row.n] = row.wav
    tg = host.pitch_targets(pt, wav, lengths=[row.n])
    T = row.T
    assert tuple(tg["cwt_spec"].shape) == (1, T, 10) and tg["uv"].dtype == torch.bool and tg["status"].tolist() == [0]
    f0 = tg["f0"][0].cpu().numpy()
    want = P.track(*(a.astype(np.float32) for a in P.nacf(row.wav)))
    np.testing.assert_array_equal(tg["uv"][0].cpu().numpy(), want[0] == 0)
    texts, lens, spk = g["texts"][:1], g["src_lens"][:1], g["spker_embeds"][:1]
    L = int(lens[0])
    d = np.zeros((1, texts.shape[1]), np.int64)
    d[0, :L] = T // L
    d[0, :T - L * (T // L)] += 1
    assert d.sum() == T
    out = model.duration_pitch_energy_net(None, torch.from_numpy(texts), torch.from_numpy(lens), spker_embeds=torch.from_numpy(spk),
                                          d_targets=torch.from_numpy(d), p_targets={k: tg[k] for k in ("cwt_spec", "f0_mean", "f0_std", "uv")})
    torch.cuda.synchronize()
    got = out["p_predictions"]["f0_denorm"][0].cpu().numpy()
    pt_np = {k: tg[k].cpu().numpy() for k in ("cwt_spec", "f0_mean", "f0_std", "uv")}
    st = O.duration_pitch_speaker_net(sd, cfg, texts, lens, spk, max_mel_len=T, d_target=d.astype(np.float32), pitch_target=pt_np)
    np.testing.assert_allclose(got, st["f0_denorm"][0], rtol=3e-4, atol=2e-3)
    uv = want[0] == 0
    assert not got[uv].any() and (got[~uv] > 0).all()
    err = float(np.abs(got[~uv] / f0[~uv] - 1).max())
    report(f"PITCH end to end ({row.name}): f0_denorm vs the tracked f0 on {int((~uv).sum())} voiced frames {err:.3e} (bound {2 * PC.RECON_ERR_MEASURED:.3e})")
    if which == 1:
        assert err <= 2 * PC.RECON_ERR_MEASURED


def test_pitch_targets_check_raises_on_a_silent_row():
    host = _host()
    pt = host.get_pitch_tracker(device=DEV)
    rows = PC.rows()
    wavs = [rows[1].wav, rows[3].wav]
    with pytest.raises(ValueError, match=r"rows 1 \(no voiced frame\)"):
        host.pitch_targets(pt, wavs)
    tg = host.pitch_targets(pt, wavs, check=False)
    assert tg["status"].tolist() == [0, 1] and not tg["cwt_spec"][1].any() and float(tg["f0_std"][1]) == 1.0
    p = host.pitch_from_audio(pt, wavs)
    assert p["frames"].tolist() == [17, 17] and not p["f0"][1].any() and p["uv"][1].all()
    edited = host.pitch_targets_from_f0(pt, p["f0"][:1] * 2.0 ** (2 / 12), p["frames"][:1])      # the melody, two semitones up
    assert abs(float(edited["f0_mean"][0]) - float(tg["f0_mean"][0]) - 2.0 / 12.0 * float(np.log(2.0))) < 1e-5
    assert torch.allclose(edited["cwt_spec"], tg["cwt_spec"][:1], atol=1e-4)

