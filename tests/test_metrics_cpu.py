"""The definition of the objective metrics (cmtts_amd/metrics.py), pinned analytically: the DCT table and the cepstra against
scipy, the MCD, F0 and SSIM identities, the host-only table of the library against the definition bit for bit, and every refusal the entry
points make before the GPU is touched.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.fft

from cmtts_amd import _lib, align as A, metrics as M
import metrics_cases as MC

K = M.MCD_CONST


def _mel(T, seed=0):
    rs = np.random.RandomState(seed)
    return (MC.LOG_LO + (MC.LOG_HI - MC.LOG_LO) * rs.rand(T, 80)).astype(np.float32)


# ----------------------------------------------------------------------------- cepstra

def test_dct_table_is_orthogonal():
    n = np.arange(80)[:, None]
    k = np.arange(80)[None, :]
    D = math.sqrt(2.0 / 80) * np.cos(math.pi * (n + 0.5) * k / 80)
    D[:, 0] = math.sqrt(1.0 / 80)
    assert np.abs(D.T @ D - np.eye(80)).max() <= 1e-12
    tab = M.dct_table(80, 80)
    assert tab.dtype == np.float32 and tab.shape == (80, 80) and np.array_equal(tab, D.astype(np.float32))
    assert np.array_equal(M.dct_table(80, 13), tab[:, :13])
    for bad in ((79, 20), (80, 0), (80, 81)):
        with pytest.raises(ValueError):
            M.dct_table(*bad)


def test_cepstra_equal_scipy_dct():
    mel = _mel(37).astype(np.float64)
    ref = scipy.fft.dct(mel, type=2, norm="ortho", axis=1)
    n = np.arange(80)[:, None]
    k = np.arange(80)[None, :]
    D = math.sqrt(2.0 / 80) * np.cos(math.pi * (n + 0.5) * k / 80)
    D[:, 0] = math.sqrt(1.0 / 80)
    assert np.abs(mel @ D - ref).max() <= 1e-12 * np.abs(ref).max()
    got = M.cepstra(mel, 30, 20)                     # on the float32 table: off by the table's rounding, 2^-24 relative per entry
    assert got.shape == (30, 20) and got.dtype == np.float64
    assert np.abs(got - ref[:30, :20]).max() <= 2.0 ** -24 * np.abs(mel).sum(axis=1).max()
    assert M.cepstra(mel, 30, 20, dtype=np.float32).dtype == np.float32


def test_library_table_has_the_definitions_bits():
    lib = _lib.load()
    for n_cep in (1, 13, 20, 80):
        tab = np.full((80, n_cep), np.nan, np.float32)
        assert lib.cmtts_metric_dct_table(80, n_cep, C.c_void_p(tab.ctypes.data)) == 0
        assert tab.tobytes() == M.dct_table(80, n_cep).tobytes(), n_cep


# ----------------------------------------------------------------------------- MCD

def test_mcd_of_a_pair_with_itself_is_zero():
    mel = _mel(40, 1)
    for align in ("dtw", "frame"):
        s = M.score(mel, 40, mel, 40, align=align)
        assert s["mcd"] == 0.0 and s["path_len"] == 40 and np.array_equal(s["row"], np.arange(40))


def test_one_shifted_coefficient_gives_the_constant_times_the_shift():
    mel = _mel(25, 2)
    cx = (np.round(M.cepstra(mel, 25, 20) * 4096.0) / 4096.0).astype(np.float32)      # multiples of 2^-12 below 2^7: the shift is exact
    assert np.abs(cx).max() < 128.0
    for delta in (0.5, -0.25):
        cy = cx.copy()
        cy[:, 3] = cx[:, 3] + np.float32(delta)
        assert np.array_equal(cy[:, 3] - cx[:, 3], np.full(25, np.float32(delta)))
        c = M.cost(cx, 25, cy, 25).astype(np.float32)
        total, n = M.diagonal(c)
        assert abs(float(M.mcd(total, n)) - K * abs(delta)) <= 1e-6 * K * abs(delta)
        t, n, row = A.dtw(c)
        assert float(t) / n <= abs(delta) * (1 + 1e-6)      # the DTW cannot do worse than the diagonal
    cy = cx.copy()
    cy[:, 0] += np.float32(3.0)                       # c0 is excluded by default
    assert not M.cost(cx, 25, cy, 25).diagonal().any()
    assert M.cost(cx, 25, cy, 25, k_lo=0, k_hi=0).diagonal().tolist() == [3.0] * 25


def test_repeated_frames_give_zero_and_the_known_row():
    mel = _mel(30, 3)
    reps = np.random.RandomState(4).randint(1, 4, size=30)
    rec = np.repeat(mel, reps, axis=0)
    s = M.score(mel, 30, rec, len(rec))
    assert s["mcd"] == 0.0 and np.array_equal(s["row"], np.repeat(np.arange(30), reps))
    assert s["path_len"] == len(rec)
    f = M.score(mel, 30, rec, len(rec), align="frame")
    assert f["mcd"] > 0.0 and f["path_len"] == 30 and np.array_equal(f["row"], np.minimum(np.arange(len(rec)), 29))
    with pytest.raises(ValueError):
        M.score(mel, 30, rec, len(rec), align="band")


# ----------------------------------------------------------------------------- F0

def test_f0_counts_on_a_hand_made_table():
    #            at 1.2   above    below   vde      vde     both unvoiced   fine
    syn = [MC.F_AT, MC.F_OVER, 79.0, 0.0, 150.0, 0.0, 200.0]
    rec = [MC.F_REC, MC.F_REC, 100.0, 100.0, 0.0, 0.0, 200.0]
    s = M.f0_stats(syn, rec)
    assert (s["n"], s["n_vv"], s["n_gpe"], s["n_vde"]) == (7, 4, 2, 2)
    assert s["ffe"] == np.float32(4 / 7) and s["gpe"] == np.float32(2 / 4) and s["vde"] == np.float32(2 / 7)
    assert M.f0_stats([MC.F_AT], [MC.F_REC])["n_gpe"] == 0 and M.f0_stats([MC.F_OVER], [MC.F_REC])["n_gpe"] == 1
    assert M.f0_stats([np.float32(80.0)], [MC.F_REC])["n_gpe"] == 0      # |80 - 100| = 20 as well
    assert M.f0_stats([np.nextafter(np.float32(80.0), np.float32(0))], [MC.F_REC])["n_gpe"] == 1
    # a row: the rendering's frames 2, 2, 0 against the recording's three
    r = M.f0_stats([100.0, 0.0, 130.0], [130.0, 131.0, 0.0], row=[2, 2, 0])
    assert (r["n"], r["n_vv"], r["n_gpe"], r["n_vde"]) == (3, 2, 0, 1)
    # row entries are clamped, and the identity is clamped to the rendering's last frame
    assert M.f0_stats([100.0, 200.0], [100.0, 200.0, 200.0, 0.0])["n_vde"] == 1
    assert M.f0_stats([100.0, 200.0], [100.0, 200.0], row=[-3, 9])["n_gpe"] == 0


def test_f0_undefined_values_are_nan_and_counts_stay_valid():
    s = M.f0_stats(np.zeros(9), np.zeros(9))
    assert (s["n"], s["n_vv"], s["n_gpe"], s["n_vde"]) == (9, 0, 0, 0) and s["ffe"] == 0.0 and s["vde"] == 0.0
    assert all(np.isnan(s[k]) for k in ("gpe", "rmse_cents", "mae_cents", "corr"))
    s = M.f0_stats([0, 100, 0], [100, 0, 0])
    assert (s["n_vv"], s["n_vde"]) == (0, 2) and np.isnan(s["corr"]) and s["ffe"] == np.float32(2 / 3)
    c = M.f0_stats([150.0] * 70, np.linspace(100, 200, 70))      # a constant track: no variance, no correlation
    assert np.isnan(c["corr"]) and not np.isnan(c["rmse_cents"])


def test_a_semitone_is_a_hundred_cents():
    rec = np.linspace(90.0, 390.0, 200)
    syn = rec * 2.0 ** (1.0 / 12.0)
    assert np.abs(M.cents(syn, rec) - 100.0).max() <= 1e-9      # in double, before the tracks are rounded to float32
    x, y = syn.astype(np.float32).astype(np.float64), rec.astype(np.float32).astype(np.float64)
    e = 1200.0 * np.log2(x / y)                      # the float32 tracks' own cents: 100 up to the rounding of the inputs
    assert np.abs(e - 100.0).max() <= 1200.0 / math.log(2.0) * 2.0 ** -23 * 1.01
    s = M.f0_stats(syn, rec)
    assert abs(float(s["mae_cents"]) - e.mean()) <= 1e-9 * 100 + 100 * 2.0 ** -24
    assert abs(float(s["rmse_cents"]) - math.sqrt((e * e).mean())) <= 1e-9 * 100 + 100 * 2.0 ** -24
    assert abs(float(s["corr"]) - np.corrcoef(x, y)[0, 1]) <= 2.0 ** -23
    # exact inputs: powers of two, an octave is 1200 cents to 1e-9
    o = M.f0_stats([256.0, 512.0, 128.0], [128.0, 256.0, 64.0])
    assert abs(float(o["mae_cents"]) - 1200.0) <= 1e-9 and abs(float(o["rmse_cents"]) - 1200.0) <= 1e-9 and o["n_gpe"] == 3
    # the fixed order: the sum of many equal terms does not depend on it, the definition's own order is reproducible
    assert M._lane_sum(np.ones(4096)) == 4096.0 and M._lane_sum(np.arange(130.0)) == 130 * 129 / 2


# ----------------------------------------------------------------------------- SSIM

def _images(T, C, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(T, C).astype(np.float32) - 0.5, rs.rand(T, C).astype(np.float32) - 0.5


def test_ssim_of_an_image_with_itself_is_one():
    u, _ = _images(40, 20, 5)
    assert M.ssim(u, u, 1.0) == 1.0 and (M.ssim_map(u, u, 0.37) == 1.0).all()


def test_separable_evaluation_equals_the_direct_double_loop():
    u, v = _images(19, 14, 6)
    a, b = M.ssim_map(u, v, 0.8), M.ssim_map_direct(u, v, 0.8)
    assert a.shape == (9, 4) and np.abs(a - b).max() <= 1e-12
    assert abs(float(M.ssim(u, v, 0.8)) - b.mean()) <= 2.0 ** -24
    g = M.gaussian_window()
    assert len(g) == 11 and abs(g.sum() - 1.0) <= 1e-15 and np.array_equal(g, g[::-1]) and abs(g[5] / g[4] - math.exp(1 / 4.5)) <= 1e-15


def test_constant_images_give_the_luminance_term():
    a, b, L = 0.25, -0.5, 1.5
    c1 = (0.01 * L) ** 2
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    got = M.ssim_map(np.full((13, 12), a), np.full((13, 12), b), L)
    assert got.shape == (3, 2) and np.abs(got - want).max() <= 1e-12
    assert abs(float(M.ssim(np.full((13, 12), a), np.full((13, 12), b), L)) - want) <= 2.0 ** -24 * abs(want) * 1.01


def test_window_counts():
    u, v = _images(11, 11, 7)
    assert M.ssim_map(u, v, 1.0).shape == (1, 1) and not np.isnan(M.ssim(u, v, 1.0))
    assert np.isnan(M.ssim(u[:10], v[:10], 1.0)) and np.isnan(M.ssim(u[:, :10], v[:, :10], 1.0))
    with pytest.raises(ValueError):
        M.ssim(u, v[:10], 1.0)


def test_images_are_unit_columns_on_the_recordings_axis():
    rs = np.random.RandomState(8)
    cx, cy = rs.standard_normal((9, 20)).astype(np.float32), rs.standard_normal((14, 20)).astype(np.float32)
    cy[:, 4] = 0.0
    row = np.minimum(np.arange(14) * 9 // 14, 8)
    u, v, (lo, hi) = M.ssim_images(cx, cy, row, 12)
    assert u.shape == v.shape == (14, 12) and u.dtype == np.float32
    assert np.abs(np.linalg.norm(u.astype(np.float64), axis=0) - 1.0).max() <= 14 * 2.0 ** -24
    assert not v[:, 4].any() and np.abs(np.linalg.norm(np.delete(v, 4, axis=1).astype(np.float64), axis=0) - 1.0).max() <= 14 * 2.0 ** -24
    a = cx[row, :12].astype(np.float64)
    assert np.abs(u - a / np.linalg.norm(a, axis=0)).max() <= 2.0 ** -24
    assert lo == min(u.min(), v.min()) and hi == max(u.max(), v.max())


def test_score_and_summarise():
    x, y, fx, fy = MC.inputs()
    scores = []
    for b, (xl, yl) in enumerate(MC.PAIRS[:5]):
        s = M.score(x[b], xl, y[b], yl, f0_syn=fx[b], f0_rec=fy[b])
        assert s["row"].shape == (yl,) and s["path_len"] >= max(xl, yl) and s["mcd"] > 0 and s["n"] == yl
        assert -1.0 <= s["ssim"] <= 1.0
        scores.append(s)
    assert scores[0]["n_gpe"] > 0 and scores[0]["n_vde"] > 0 and scores[0]["n_vv"] > 20
    m = M.summarise(scores)
    assert m["pairs"] == 5 and abs(m["mcd"] - np.mean([float(s["mcd"]) for s in scores])) <= 1e-12
    assert set(m) >= {"mcd", "ssim", "ffe", "gpe", "vde", "f0_rmse_cents", "f0_mae_cents", "f0_corr"} and "row" not in m
    one = M.score(x[6], 1, y[6], 1)
    assert np.isnan(one["ssim"]) and M.summarise([one])["pairs"] == 1 and np.isnan(M.summarise([one])["ssim"])
    assert M.summarise([]) == {"pairs": 0}


# ----------------------------------------------------------------------------- the entry points' refusals

def test_entry_points_refuse_before_the_gpu_is_touched():
    lib = _lib.load()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)          # stands for a device pointer: every call below returns before it would be read
    E_INVALID, E_WORKSPACE = -1, lib.cmtts_metric_ssim(p, p, p, 1, 64, 20, p, p, p, 0, None)
    assert E_WORKSPACE not in (0, E_INVALID) and b"workspace" in lib.cmtts_last_error()

    def refused(rc, word):
        assert rc == E_INVALID and word in lib.cmtts_last_error(), (rc, lib.cmtts_last_error())

    refused(lib.cmtts_metric_dct_table(80, 20, None), b"null")
    refused(lib.cmtts_metric_dct_table(64, 20, p), b"n_mels")
    refused(lib.cmtts_metric_dct_table(80, 0, p), b"n_cep")
    refused(lib.cmtts_metric_dct_table(80, 81, p), b"n_cep")
    # null device pointers
    refused(lib.cmtts_metric_cepstra(None, None, None, 1, 8, 80, 20, None, None), b"null")
    refused(lib.cmtts_metric_cost(None, None, 8, None, None, 8, 1, 20, 1, 13, None, None), b"null")
    refused(lib.cmtts_metric_diagonal(None, None, None, 1, 8, 8, None, None, None), b"null")
    refused(lib.cmtts_metric_f0(None, None, 8, None, None, 8, None, 1, None, None, None), b"null")
    refused(lib.cmtts_metric_ssim_prepare(None, None, 8, None, None, 8, None, 1, 20, 20, None, None, None, None), b"null")
    refused(lib.cmtts_metric_ssim(None, None, None, 1, 8, 20, None, None, None, 0, None), b"null")
    # shapes
    refused(lib.cmtts_metric_cepstra(p, p, p, 1, 8, 64, 20, p, None), b"n_mels")
    refused(lib.cmtts_metric_cepstra(p, p, p, 1, 8, 80, 81, p, None), b"n_cep")
    refused(lib.cmtts_metric_cepstra(p, p, p, 0, 8, 80, 20, p, None), b"B")
    refused(lib.cmtts_metric_cepstra(p, p, p, 1, 4097, 80, 20, p, None), b"4096")
    for B, Ts, Tr in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 4097)):
        refused(lib.cmtts_metric_cost(p, p, Ts, p, p, Tr, B, 20, 1, 13, p, None), b"4096")
        refused(lib.cmtts_metric_diagonal(p, p, p, B, Ts, Tr, p, p, None), b"4096")
        refused(lib.cmtts_metric_f0(p, p, Ts, p, p, Tr, None, B, p, p, None), b"4096")
        refused(lib.cmtts_metric_ssim_prepare(p, p, Ts, p, p, Tr, None, B, 20, 20, p, p, p, None), b"4096")
    for n_cep, k_lo, k_hi in ((20, 5, 4), (20, -1, 4), (20, 1, 20), (81, 1, 13), (0, 0, 0)):
        refused(lib.cmtts_metric_cost(p, p, 8, p, p, 8, 1, n_cep, k_lo, k_hi, p, None), b"k_lo")
    refused(lib.cmtts_metric_ssim_prepare(p, p, 8, p, p, 8, None, 1, 20, 21, p, p, p, None), b"n_cep")
    refused(lib.cmtts_metric_ssim_prepare(p, p, 8, p, p, 8, None, 1, 20, 0, p, p, p, None), b"n_cep")
    refused(lib.cmtts_metric_ssim(p, p, p, 1, 8, 81, p, p, p, 1 << 20, None), b"C")
    refused(lib.cmtts_metric_ssim(p, p, p, 1, 4097, 20, p, p, p, 1 << 20, None), b"4096")
    refused(lib.cmtts_metric_ssim(p, p, p, 0, 8, 20, p, p, p, 1 << 20, None), b"B")
    # the workspace
    assert lib.cmtts_metric_workspace_bytes(0, 8, 20) == 0 and lib.cmtts_metric_workspace_bytes(1, 4097, 20) == 0
    assert lib.cmtts_metric_workspace_bytes(1, 8, 81) == 0 and lib.cmtts_metric_workspace_bytes(1, 1, 20) == 256
    nb = lib.cmtts_metric_workspace_bytes(32, 600, 20)
    assert nb >= 32 * ((600 - 10 + 7) // 8) * 8 and nb % 256 == 0
    assert lib.cmtts_metric_ssim(p, p, p, 32, 600, 20, p, p, p, nb - 1, None) == E_WORKSPACE
    assert lib.cmtts_metric_ssim(p, p, p, 1, 64, 20, p, p, None, 1 << 20, None) == E_WORKSPACE


def test_host_surface_refuses_before_a_device_is_asked_for():
    import torch
    from cmtts_amd import host
    mel = torch.zeros(2, 12, 80)
    ok = dict(mel_syn=mel, syn_lens=[12, 11], mel_rec=mel, rec_lens=[12, 12])
    for change in (dict(mel_syn=torch.zeros(2, 12, 79)), dict(mel_rec=torch.zeros(3, 12, 80)), dict(syn_lens=[12, 13]), dict(rec_lens=[0, 12]),
                   dict(rec_lens=[12]), dict(align="band"), dict(f0_syn=torch.zeros(2, 12)), dict(f0_syn=torch.zeros(2, 11), f0_rec=torch.zeros(2, 12)),
                   dict(mcd_coefs=(5, 4)), dict(mcd_coefs=(1, 80)), dict(ssim_coefs=0), dict(ssim_coefs=81), dict(data_range=0.0),
                   dict(emb_syn=torch.zeros(2, 8)), dict(emb_syn=torch.zeros(2, 8), emb_rec=torch.zeros(2, 9)),
                   dict(mel_syn=torch.zeros(2, 4097, 80), syn_lens=[12, 12])):
        with pytest.raises(ValueError):
            host.score_pairs(**{**ok, **change})
    with pytest.raises(ValueError):
        host.mel_cepstra(mel, [12, 13])
    with pytest.raises(ValueError):
        host.mel_cepstra(mel, [12, 12], n_cep=81)
