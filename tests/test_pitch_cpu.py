"""Pitch of a recording, the definition (cmtts_amd/pitch.py) and what the C ABI checks without a GPU: the CWT pinned
analytically (direct = FFT form, the closed form on a cosine, the scales), convert_continuos_f0's semantics and the status codes, the tracker
on synthetic rows with known f0, its tie rules on hand-made autocorrelations, the model's reconstruction of the contour from the targets,
the host tables of the library against numpy's, and the arguments the entry points refuse before the GPU is touched."""
import ctypes as C
import math

import numpy as np
import pytest

from cmtts_amd import _lib, pitch as P
import pitch_cases as PC

G = P.default_geometry()

F0_ERR_MEASURED, RECON_ERR_MEASURED = PC.F0_ERR_MEASURED, PC.RECON_ERR_MEASURED


def _tracked(row, dtype=np.float64):
    src = row.pcm if hasattr(row, "pcm") else row.wav
    r, pk = P.nacf(src, dtype=dtype)
    return P.track(r.astype(np.float32), pk.astype(np.float32))


def test_geometry_of_the_reference_constants():
    assert (G.W, G.LMIN, G.LMAX) == (828, 30, 275)
    assert G.frame_count(513) == 3 and G.frame_count(4200) == 17 and G.frame_count(8300) == 33 and G.frame_count(0) == 1
    assert G.r_w[0] == 1.0 and 0.45 < G.r_w[-1] < 0.5 and np.all(np.diff(G.r_w) < 0)
    assert G.lg[0] == 0 and G.lg[1] == 0 and G.lg[64] == 6 and G.lg.dtype == np.float32
    for bad in ((22050, 256, 20.0, 750.0), (22050, 256, 80.0, 12000.0), (22050, 256, 800.0, 750.0), (0, 256, 80.0, 750.0), (48000, 256, 80.0, 750.0)):
        with pytest.raises(ValueError):
            P.Geometry(*bad)


@pytest.mark.parametrize("T", [3, 4, 16, 17, 33, 257])
def test_cwt_direct_is_the_fft_form(T):
    x = np.random.default_rng(T).standard_normal(T)
    a, b = P.cwt_fft(x), P.cwt_direct(x)
    assert a.shape == b.shape == (T, 10)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


def test_cwt_of_a_cosine_is_the_closed_form():
    """T = N, the cosine on an FFT bin: W_j[t] = sqrt(2 pi s_j / dt) psi^(s_j w0) cos(w0 t) — pins the normalisation."""
    N, k = 64, 5
    t = np.arange(N)
    w0 = 2 * np.pi * k / (N * P.CWT_DT)
    x = np.cos(2 * np.pi * k * t / N)
    want = np.stack([math.sqrt(2 * np.pi * s / P.CWT_DT) * P.psi_ft(s * w0) * x for s in P.cwt_scales()], axis=1)
    assert np.abs(P.cwt_fft(x) - want).max() <= 1e-12
    assert np.abs(P.cwt_direct(x) - want).max() <= 1e-12


def test_cwt_scales_and_table():
    np.testing.assert_array_equal(P.cwt_scales(), [0.01 * 2 ** j for j in range(10)])
    assert [P.cwt_length(T) for T in (3, 4, 5, 16, 17, 4096)] == [4, 4, 8, 16, 32, 4096]
    h = P.cwt_table(32)
    assert h.shape == (10, 32)
    np.testing.assert_allclose(h[:, 1:], h[:, :0:-1], rtol=0, atol=1e-15)        # even
    with pytest.raises(ValueError):
        P.cwt_fft(np.ones(2))                                                      # pycwt's own omega_1 is negative at N = 2


def test_convert_continuos_f0_semantics():
    f0 = np.array([0, 0, 100.0, 0, 0, 0, 200.0, 150.0, 0, 0])
    c = P.convert_continuos_f0(f0)
    np.testing.assert_allclose(c, [100, 100, 100, 125, 150, 175, 200, 150, 150, 150], rtol=1e-15)
    np.testing.assert_array_equal(P.convert_continuos_f0(np.array([120.0, 130.0, 140.0])), [120.0, 130.0, 140.0])
    with pytest.raises(ValueError):
        P.convert_continuos_f0(np.zeros(4))


def test_targets_statuses():
    t = P.targets(np.array([0, 0, 100.0, 0, 0, 0, 200.0, 150.0, 0, 0]))
    lf0 = np.log([100, 100, 100, 125, 150, 175, 200, 150, 150, 150])
    assert t["status"] == 0 and t["f0_mean"] == np.mean(lf0) and t["f0_std"] == np.std(lf0)
    np.testing.assert_array_equal(t["uv"], [1, 1, 0, 1, 1, 1, 0, 0, 1, 1])
    np.testing.assert_allclose(t["cwt_spec"], P.cwt_fft((lf0 - lf0.mean()) / lf0.std()), rtol=0, atol=1e-12)
    one = P.targets(np.array([0, 0, 0, 187.5, 0, 0, 0]))                           # a single voiced frame: a constant contour
    assert one["status"] == 2 and one["f0_mean"] == math.log(187.5) and one["f0_std"] == 1.0 and not one["cwt_spec"].any()
    flat = P.targets(np.full(9, 0.1 * 3))                                          # max == min, whatever the mean of equal values rounds to
    assert flat["status"] == 2
    none = P.targets(np.zeros(6))
    assert none["status"] == 1 and none["f0_mean"] == 0.0 and none["f0_std"] == 1.0 and not none["cwt_spec"].any() and none["uv"].all()
    assert P.targets(np.array([100.0, 110.0]))["status"] == 3


def test_tracker_follows_the_rows():
    worst = 0.0
    for row in PC.rows():
        lag, f0 = _tracked(row)
        kinds = row.frame_kinds()
        assert len(kinds) == row.T == f0.shape[0]
        # the frames left out straddle a boundary (or reach outside the clip): at most 4 per boundary, so the exclusion cannot hide a failure
        runs = [len(s) for s in "".join(kinds).replace("v", " ").replace("u", " ").split()]
        assert max(runs, default=0) <= 4 and len(runs) <= len(row.stretches) + 1, (row.name, "".join(kinds))
        truth = row.truth[np.minimum(np.arange(row.T) * PC.HOP, row.n - 1)]
        v = np.array([k == "v" for k in kinds])
        u = np.array([k == "u" for k in kinds])
        assert (f0[u] == 0).all() and (lag[u] == 0).all(), (row.name, f0)
        assert (f0[v] > 0).all(), (row.name, f0)
        if v.any():
            err = float(np.abs(f0[v] / truth[v] - 1).max())
            print(f"{row.name}: worst relative f0 error on {int(v.sum())} voiced frames {err:.3e}")
            worst = max(worst, err)
    assert worst <= 2 * F0_ERR_MEASURED, worst
    short = _tracked(PC.rows()[0])[1]                          # every frame reaches outside the clip: still the right octave
    assert np.all(np.abs(short / 200.0 - 1) < 0.01), short
    assert not _tracked(PC.rows()[3])[0].any()


def test_float32_arm_takes_the_same_path():
    for row in PC.rows():
        lag64, f64 = _tracked(row)
        lag32, f32 = _tracked(row, np.float32)
        np.testing.assert_array_equal(lag64, lag32, err_msg=row.name)
        np.testing.assert_allclose(f32, f64, rtol=1e-4)


def test_int16_row_is_the_float_row_it_was_made_from():
    row = PC.rows()[4]
    a = P.nacf(row.pcm)
    b = P.nacf(row.pcm.astype(np.float32) / np.float32(32768.0))
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_tie_rules_on_handmade_r():
    hm = PC.handmade()
    lag, stren = P.candidates(hm["plateaus"][0])
    assert lag[0].tolist() == [100, 0, 0, 0, 0, 0, 0, 0]              # of a plateau only the first cell is > its left and >= its right
    assert lag[3].tolist() == [50, 100, 0, 0, 0, 0, 0, 0] and stren[3, 0] > stren[3, 1] and stren[0, 1] == -np.inf      # listed by ascending lag
    # more than 8 maxima of one height: the octave cost favours the shorter lags, so the 8 shortest stay
    r, pk = hm["many"]
    peaks = np.arange(G.LMIN + 1, G.LMAX, 9)
    lag, stren = P.candidates(r)
    assert lag[4].tolist() == peaks[:8].tolist()
    for f in (0, 1, 2, 3, 5, 6):                                       # the 8 strongest, listed by ascending lag
        s = r[f, peaks] - np.float32(P.OC) * (G.lg[peaks] - G.lg_floor)
        keep = np.sort(peaks[np.argsort(-s, kind="stable")[:8]])
        assert lag[f].tolist() == keep.tolist()
    # equal strengths (+inf ties exactly): ties go to the smaller lag
    r = np.zeros((1, G.LMAX + 2), np.float32)
    r[0, 40:240:20] = np.inf
    lag, stren = P.candidates(r)
    assert lag[0].tolist() == list(range(40, 200, 20)) and np.all(stren[0] == np.inf)
    # a NaN is never a candidate, and a cell beside a NaN is not one either (its comparison is false)
    lag, _ = P.candidates(hm["nan"][0])
    assert lag[:, 0].tolist() == [120, 0, 0, 0, 0, 120]
    got = P.track(*hm["nan"])
    assert got[0].tolist() == [120, 0, 0, 0, 0, 120] and not np.isnan(got[1]).any()
    # nothing to choose from
    for name in ("zero", "zero_pk"):
        lag, f0 = P.track(*hm[name])
        assert not lag.any() and not f0.any()
    # T = 1 and 2; the final state is the first maximum, the walk back starts there
    assert P.track(*hm["T1"])[0].tolist() == [200]
    assert P.track(*hm["T2"])[0].tolist() == [90, 90]
    # two states of equal (infinite) total: the first one wins at the end, and a later predecessor does not replace an equal earlier one
    assert P.track(*hm["inf"])[0].tolist() == [70, 0, 0, 0]
    lag, f0 = P.track(*hm["random"])
    assert lag.shape == (40,) and ((lag == 0) | ((lag >= G.LMIN) & (lag <= G.LMAX))).all() and ((f0 > 0) == (lag > 0)).all()
    with pytest.raises(ValueError):
        P.track(hm["zero"][0].astype(np.float64), hm["zero"][1])


def test_unvoiced_strength_terms():
    pk = np.array([0.5, 0.005, 0.0, np.nan], np.float32)
    u = P.unvoiced_strength(pk)
    K = (np.float32(1) + np.float32(P.VT)) / np.float32(P.ST)
    assert u.dtype == np.float32 and u[0] == np.float32(P.VT) and u[3] == np.float32(P.VT)
    assert u[1] == np.float32(P.VT) + (np.float32(2) - (np.float32(0.005) / np.float32(0.5)) * K)
    assert u[2] == np.float32(P.VT) + np.float32(2)
    assert np.all(P.unvoiced_strength(np.zeros(3, np.float32)) == np.float32(P.VT))           # gpk == 0: the term is 0


def test_reconstruction_gives_the_contour_back():
    worst = 0.0
    for row in PC.rows()[:2]:
        _, f0 = _tracked(row)
        t = P.targets(f0)
        assert t["status"] == 0
        rec = PC.cwt2f0(t["cwt_spec"], t["f0_mean"], t["f0_std"])
        v = f0 > 0
        err = float(np.abs(rec[v] / f0[v] - 1).max())
        print(f"{row.name}: worst relative error of the reconstructed f0 {err:.3e}")
        worst = max(worst, err)
    assert worst <= 2 * RECON_ERR_MEASURED, worst


# ---- the library without a GPU -----------------------------------------------------------------------------------------------------------
NAMES = ("cmtts_pitch_tables", "cmtts_pitch_create", "cmtts_pitch_destroy", "cmtts_pitch_workspace_bytes", "cmtts_pitch_nacf", "cmtts_pitch_track",
         "cmtts_pitch_targets")


def _tables(fs=22050, hop=256, floor=80.0, ceiling=750.0, cwt_n=64):
    lib = _lib.load()
    geo = np.zeros(3, np.int32)
    assert lib.cmtts_pitch_tables(fs, hop, floor, ceiling, geo.ctypes.data, None, None, None, None, 0, None) == 0
    W, lmax = int(geo[0]), int(geo[2])
    window, rw, lg = np.zeros(W, np.float32), np.zeros(lmax + 2, np.float64), np.zeros(lmax + 2, np.float32)
    lgf, cwt = np.zeros(1, np.float32), np.zeros((10, cwt_n), np.float32)
    assert lib.cmtts_pitch_tables(fs, hop, floor, ceiling, geo.ctypes.data, window.ctypes.data, rw.ctypes.data, lg.ctypes.data, lgf.ctypes.data, cwt_n,
                                  cwt.ctypes.data) == 0
    return geo, window, rw, lg, lgf[0], cwt


def test_library_tables_are_the_definitions():
    """The tables a handle holds (csrc/pitch_tables.cpp, made in double) against numpy's: the log2 table and the floor's log2 bit for bit — the
    tracker's path depends on them —, the window to a float32 rounding, r_w and the periodised wavelets to the double arithmetic."""
    for name in NAMES:
        assert name in _lib.SIGNATURES
    geo, window, rw, lg, lgf, cwt = _tables()
    assert geo.tolist() == [G.W, G.LMIN, G.LMAX]
    np.testing.assert_array_equal(lg, G.lg)
    assert lgf == G.lg_floor
    np.testing.assert_allclose(window, G.window, rtol=1.2e-7, atol=1e-9)
    np.testing.assert_allclose(rw, G.r_w, rtol=1e-12)
    for n in (4, 64, 4096):
        cwt = _tables(cwt_n=n)[5]
        h = P.cwt_table(n)
        assert np.abs(cwt - h).max() <= 1.2e-7 * np.abs(h).max(), n
    g2 = P.Geometry(16000, 200, 60.0, 500.0)
    geo, window, rw, lg, lgf, _ = _tables(16000, 200, 60.0, 500.0, 4)
    assert geo.tolist() == [g2.W, g2.LMIN, g2.LMAX] and lgf == g2.lg_floor
    np.testing.assert_array_equal(lg, g2.lg)


def test_arguments_refused_before_the_gpu():
    lib = _lib.load()
    geo = np.zeros(3, np.int32)
    h = C.c_void_p()
    for bad in ((22050, 256, 20.0, 750.0), (22050, 256, 80.0, 12000.0), (22050, 0, 80.0, 750.0), (22050, 2048, 80.0, 750.0), (48000, 256, 80.0, 750.0),
                (0, 256, 80.0, 750.0), (22050, 256, 800.0, 750.0)):
        assert lib.cmtts_pitch_tables(*bad, geo.ctypes.data, None, None, None, None, 0, None) == -1 and b"unsupported geometry" in lib.cmtts_last_error()
        assert lib.cmtts_pitch_create(*bad, C.byref(h)) == -1 and b"unsupported geometry" in lib.cmtts_last_error() and not h.value
    assert lib.cmtts_pitch_tables(22050, 256, 80.0, 750.0, None, None, None, None, None, 0, None) == -1 and b"null" in lib.cmtts_last_error()
    buf = np.zeros((10, 8), np.float32)
    assert lib.cmtts_pitch_tables(22050, 256, 80.0, 750.0, geo.ctypes.data, None, None, None, None, 6, buf.ctypes.data) == -1
    assert b"cwt_n" in lib.cmtts_last_error()
    assert lib.cmtts_pitch_create(22050, 256, 80.0, 750.0, None) == -1 and b"null" in lib.cmtts_last_error()
    lib.cmtts_pitch_destroy(None)
    assert lib.cmtts_pitch_workspace_bytes(1, 1) > 0
    assert lib.cmtts_pitch_workspace_bytes(32, 512) >= 32 * 512 * 8 * 8
    assert lib.cmtts_pitch_workspace_bytes(1, 4096) > 0
    for bad in ((0, 16), (65536, 16), (1, 0), (1, 4097)):
        assert lib.cmtts_pitch_workspace_bytes(*bad) == 0, bad
    # a null handle or buffer: refused, nothing launched (the other pointers are never dereferenced)
    assert lib.cmtts_pitch_nacf(None, 1, 0, 1, 4000, 1, 16, 1, 1, 1, 1, 1 << 20, None) == -1 and b"null" in lib.cmtts_last_error()
    assert lib.cmtts_pitch_track(None, 1, 1, 1, 1, 16, 1, 1, 1, 1 << 20, None) == -1 and b"null" in lib.cmtts_last_error()
    assert lib.cmtts_pitch_targets(None, 1, 1, 1, 16, 1, 1, 1, 1, 1, 1, 1 << 20, None) == -1 and b"null" in lib.cmtts_last_error()
    for k in (1, 2, 5, 6, 7, 8, 9):                           # every pointer of cmtts_pitch_targets
        a = [1, 1, 1, 1, 16, 1, 1, 1, 1, 1, 1, 1 << 20, None]
        a[k] = None
        assert lib.cmtts_pitch_targets(*a) == -1 and b"null" in lib.cmtts_last_error(), k
    # a handle that is not null, sizes out of range: refused on the sizes (1 stands for pointers that are never dereferenced)
    assert lib.cmtts_pitch_nacf(1, 1, 0, 0, 4000, 1, 16, 1, 1, 1, 1, 1 << 20, None) == -1 and b"rows" in lib.cmtts_last_error()
    assert lib.cmtts_pitch_nacf(1, 1, 0, 1, 4000, 1, 4097, 1, 1, 1, 1, 1 << 20, None) == -1 and b"T" in lib.cmtts_last_error()
    assert lib.cmtts_pitch_nacf(1, 1, 0, 1, 1 << 30, 1, 16, 1, 1, 1, 1, 1 << 20, None) == -1 and b"ld" in lib.cmtts_last_error()
    assert lib.cmtts_pitch_track(1, 1, 1, 1, 70000, 16, 1, 1, 1, 1 << 20, None) == -1
    assert lib.cmtts_pitch_targets(1, 1, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1 << 20, None) == -1 and b"3 <= T" in lib.cmtts_last_error()
    assert lib.cmtts_pitch_targets(1, 1, 1, 1, 16, 1, 1, 1, 1, 1, None, 1 << 20, None) == -4                      # CMTTS_E_WORKSPACE
    assert lib.cmtts_pitch_track(1, 1, 1, 1, 4, 512, 1, 1, 1, 16, None) == -4


def test_host_surface_refuses_before_a_device_is_asked_for():
    from cmtts_amd import host
    for bad in ({"pitch_type": "frame"}, {"pitch_type": "ph"}, {"pitch_norm": "standard"}):
        with pytest.raises(ValueError):
            host.get_pitch_tracker({"preprocessing": {"pitch": bad}}, device="cpu")
    with pytest.raises(ValueError):
        host.get_pitch_tracker({"preprocessing": {"audio": {"sampling_rate": 16000}}}, device="cpu")
    pt = host.get_pitch_tracker({"preprocessing": {"pitch": {"pitch_type": "cwt", "pitch_norm": "log"}}}, device="cpu")
    assert pt.lags == G.LMAX + 2 and pt.hop == 256
    with pytest.raises(ValueError):
        host.pitch_targets(pt, np.zeros((2, 511), np.float32))                     # 2 frames
    with pytest.raises(ValueError):
        host.pitch_targets(pt, np.zeros((1, 4096 * 256), np.float32))              # 4097 frames
    with pytest.raises(ValueError):
        host.pitch_from_audio(pt, np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        host.pitch_from_audio(pt, np.zeros((2, 4000), np.float32), lengths=[4000, 4001])
    with pytest.raises(ValueError):
        host.pitch_targets_from_f0(pt, np.zeros((2, 2), np.float32), [2, 2])
    with pytest.raises(ValueError):
        host.pitch_targets_from_f0(pt, np.zeros((2, 8), np.float32), [8])
    with pytest.raises(ValueError):
        host.pitch_track(pt, np.zeros((1, 4, 100), np.float32), np.zeros((1, 4), np.float32), [4])
