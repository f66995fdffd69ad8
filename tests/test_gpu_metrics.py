"""Objective metrics on the GPU (include/cmtts_hip.h: cmtts_metric_*; csrc/metrics.hip; host.mel_cepstra / score_pairs / score_audio; DESIGN.md
§3.5m): every kernel alone against the float64 definition under a derived bound or bit for bit, the padding untouched, a pair alone against
the pair in its batch, and the host surface end to end.  No tolerance below is taken from the code under test."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmtts_amd import _lib, align as A, metrics as M
from conftest import report
import metrics_cases as MC
import pitch_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS, TS, TR = MC.PAIRS, MC.TS, MC.TR
B = len(PAIRS)
U24, U23 = 2.0 ** -24, 2.0 ** -23

_CACHE = {}


def _host():
    from cmtts_amd import host
    return host


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _dev_lens(pairs=PAIRS):
    return (torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=DEV), torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=DEV))


def _table(n_cep):
    return torch.from_numpy(M.dct_table(80, n_cep)).to(DEV)


def _cepstra_dev(mel, lens, n_cep):
    """cmtts_metric_cepstra into a NaN-filled buffer."""
    lib = _lib.load()
    Bm, T, _ = mel.shape
    out = _nan(Bm, T, n_cep)
    _lib.check(lib.cmtts_metric_cepstra(_p(mel), _p(lens), _p(_table(n_cep)), Bm, T, 80, n_cep, _p(out), _st()))
    torch.cuda.synchronize()
    return out


def _cost_dev(cx, cy, xl, yl, k_lo, k_hi):
    lib = _lib.load()
    cost = _nan(cx.shape[0], cx.shape[1], cy.shape[1])
    _lib.check(lib.cmtts_metric_cost(_p(cx), _p(xl), cx.shape[1], _p(cy), _p(yl), cy.shape[1], cx.shape[0], cx.shape[2], k_lo, k_hi, _p(cost), _st()))
    torch.cuda.synchronize()
    return cost


def _dtw_dev(cost, pairs):
    """The existing cmtts_align_dtw on a cost matrix: (row with -7 where nothing is written, total, path_len) on the device."""
    lib = _lib.load()
    Bc, Ts, Tr = cost.shape
    xl = np.asarray([p[0] for p in pairs], np.int32)
    yl = np.asarray([p[1] for p in pairs], np.int32)
    row = torch.full((Bc, Tr), -7, dtype=torch.int32, device=DEV)
    total = torch.empty(Bc, dtype=torch.float32, device=DEV)
    n = torch.empty(Bc, dtype=torch.int32, device=DEV)
    nb = lib.cmtts_align_workspace_bytes(Bc, Ts, Tr)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_align_dtw(_p(cost), C.c_void_p(xl.ctypes.data), C.c_void_p(yl.ctypes.data), Bc, Ts, Tr, _p(row), _p(total), _p(n), _p(ws), nb,
                                   _st()))
    torch.cuda.synchronize()
    return row, total, n


def _prepare_dev(cx, cy, xl, yl, row, Cimg):
    lib = _lib.load()
    Bc, Ts, n_cep = cx.shape
    Tr = cy.shape[1]
    u, v, mm = _nan(Bc, Tr, Cimg), _nan(Bc, Tr, Cimg), _nan(Bc, 2)
    _lib.check(lib.cmtts_metric_ssim_prepare(_p(cx), _p(xl), Ts, _p(cy), _p(yl), Tr, _p(row), Bc, n_cep, Cimg, _p(u), _p(v), _p(mm), _st()))
    torch.cuda.synchronize()
    return u, v, mm


def _ssim_dev(u, v, yl, rng):
    lib = _lib.load()
    Bc, Tr, Cimg = u.shape
    out = torch.full((Bc,), -9.0, dtype=torch.float32, device=DEV)
    nb = lib.cmtts_metric_workspace_bytes(Bc, Tr, Cimg)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_metric_ssim(_p(u), _p(v), _p(yl), Bc, Tr, Cimg, _p(rng), _p(out), _p(ws), nb, _st()))
    torch.cuda.synchronize()
    return out


def _f0_dev(fx, fy, xl, yl, row):
    lib = _lib.load()
    Bc, Ts = fx.shape
    counts = torch.full((Bc, 4), -7, dtype=torch.int32, device=DEV)
    vals = torch.full((Bc, 3), -9.0, dtype=torch.float32, device=DEV)
    _lib.check(lib.cmtts_metric_f0(_p(fx), _p(xl), Ts, _p(fy), _p(yl), fy.shape[1], _p(row), Bc, _p(counts), _p(vals), _st()))
    torch.cuda.synchronize()
    return counts.cpu().numpy(), vals.cpu().numpy()


def _shared():
    """The device's cepstra (n_cep = 20), cost (coefficients 1 .. 13) and DTW of the shared pairs: made once, never written."""
    if "s" not in _CACHE:
        x, y, fx, fy = MC.inputs()
        xl, yl = _dev_lens()
        cx = _cepstra_dev(torch.from_numpy(x).to(DEV), xl, 20)
        cy = _cepstra_dev(torch.from_numpy(y).to(DEV), yl, 20)
        cost = _cost_dev(cx, cy, xl, yl, 1, 13)
        row, total, n = _dtw_dev(cost, PAIRS)
        _CACHE["s"] = dict(cx=cx, cy=cy, cost=cost, row=row, total=total, n=n, xl=xl, yl=yl, fx=torch.from_numpy(fx).to(DEV),
                           fy=torch.from_numpy(fy).to(DEV))
    return _CACHE["s"]


def _within_ulps(got, ref64, ulps, tag):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), (tag, got, ref64)          # NaN exactly where the definition has NaN
    err = np.abs(got - ref64)[~nan]
    lim = ulps * MC.ulp32(ref64[~nan])
    assert (err <= lim).all(), (tag, got, ref64)
    return float((err / MC.ulp32(ref64[~nan])).max()) if err.size else 0.0


# ----------------------------------------------------------------------------- 1. cepstra

@pytest.mark.parametrize("n_cep", [13, 20])
def test_cepstra_against_float64(n_cep):
    x, y, _, _ = MC.inputs()
    worst = 0.0
    for mel, lens, T in ((x, _dev_lens()[0], TS), (y, _dev_lens()[1], TR)):
        got = _cepstra_dev(torch.from_numpy(mel).to(DEV), lens, n_cep).cpu().numpy()
        for b, n in enumerate(lens.cpu().tolist()):
            assert np.isnan(got[b, n:]).all(), b                      # the NaN the buffer was filled with: padding rows not written
            ref = M.cepstra(mel[b], n, n_cep)                         # float64 on the same float32 table
            bound = MC.cepstra_error_bound(mel[b], n, n_cep)
            err = np.abs(got[b, :n].astype(np.float64) - ref)
            assert np.isfinite(got[b, :n]).all() and (err <= bound).all(), (b, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    report(f"METRICS cepstra n_cep={n_cep}: max |c - f64| / (82 * 2^-24 * sum |mel||D|) = {worst:.3f}")


# ----------------------------------------------------------------------------- 2. cost, and the existing DTW on it

@pytest.mark.parametrize("n_cep,k_lo,k_hi", [(20, 1, 13), (40, 1, 39), (20, 0, 0)])
def test_cost_against_float64_on_the_devices_cepstra(n_cep, k_lo, k_hi):
    x, y, _, _ = MC.inputs()
    xl, yl = _dev_lens()
    cx = _cepstra_dev(torch.from_numpy(x).to(DEV), xl, n_cep)
    cy = _cepstra_dev(torch.from_numpy(y).to(DEV), yl, n_cep).clone()
    cy[0, 3] = cx[0, 70]                                              # equal frames: in another tile row, and on the single-frame pair
    cy[2, 64 - 1] = cx[2, 64]
    cy[6, 0] = cx[6, 0]
    got = _cost_dev(cx, cy, xl, yl, k_lo, k_hi).cpu().numpy()
    cxh, cyh = cx.cpu().numpy(), cy.cpu().numpy()
    K = k_hi - k_lo + 1
    bound = (K / 2 + 2) * U24
    worst = 0.0
    for b, (a, r) in enumerate(PAIRS):
        valid = np.zeros((TS, TR), bool)
        valid[:a, :r] = True
        assert np.isnan(got[b][~valid]).all() and np.isfinite(got[b][valid]).all(), b
        ref = M.cost(cxh[b], a, cyh[b], r, k_lo, k_hi)                # float64 on the device's own cepstra
        err = np.abs(got[b, :a, :r].astype(np.float64) - ref)
        assert (err <= bound * ref).all(), (b, float((err / np.maximum(ref, 1e-300)).max()))
        if (ref > 0).any():                                           # the single-frame pair holds the planted zero alone
            worst = max(worst, float((err[ref > 0] / ref[ref > 0]).max()))
    assert got[0, 70, 3] == 0.0 and got[2, 64, 63] == 0.0 and got[6, 0, 0] == 0.0
    report(f"METRICS cost K={K}: max relative |c - f64| = {worst:.2e} (bound (K/2 + 2) 2^-24 = {bound:.2e})")


def test_dtw_on_the_cepstral_cost_is_the_definition():
    s = _shared()
    cost = s["cost"].cpu().numpy()
    row, total, n = s["row"].cpu().numpy(), s["total"].cpu().numpy(), s["n"].cpu().numpy()
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    for b, (a, r) in enumerate(PAIRS):
        t_ref, n_ref, row_ref = A.dtw(np.ascontiguousarray(cost[b, :a, :r]))
        assert torch.equal(f(row[b, :r]), f(row_ref)) and (row[b, r:] == -7).all(), b
        assert torch.equal(f(total[b:b + 1]), f(np.asarray([t_ref], np.float32))) and n[b] == n_ref, b


def test_diagonal_is_the_float32_sum_in_order():
    s = _shared()
    lib = _lib.load()
    total = torch.full((B,), -9.0, dtype=torch.float32, device=DEV)
    n = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.cmtts_metric_diagonal(_p(s["cost"]), _p(s["xl"]), _p(s["yl"]), B, TS, TR, _p(total), _p(n), _st()))
    torch.cuda.synchronize()
    cost = s["cost"].cpu().numpy()
    for b, (a, r) in enumerate(PAIRS):
        t_ref, n_ref = M.diagonal(np.ascontiguousarray(cost[b, :a, :r]))
        assert total[b].cpu().numpy().tobytes() == np.float32(t_ref).tobytes() and int(n[b]) == n_ref == min(a, r), b


# ----------------------------------------------------------------------------- 3. F0 statistics

@pytest.mark.parametrize("with_row", [True, False])
def test_f0_counts_bit_for_bit_and_values_within_four_ulp(with_row):
    s = _shared()
    _, _, fx, fy = MC.inputs()
    counts, vals = _f0_dev(s["fx"], s["fy"], s["xl"], s["yl"], s["row"] if with_row else None)
    row = s["row"].cpu().numpy()
    worst, seen_nan = 0.0, False
    for b, (a, r) in enumerate(PAIRS):
        ref = M.f0_stats(fx[b, :a], fy[b, :r], row[b, :r] if with_row else None)
        want = np.asarray([ref["n"], ref["n_vv"], ref["n_gpe"], ref["n_vde"]], np.int32)
        assert torch.equal(torch.from_numpy(counts[b]), torch.from_numpy(want)), (b, counts[b], want)
        r64 = [float(ref[k]) for k in ("rmse_cents", "mae_cents", "corr")]
        worst = max(worst, _within_ulps(vals[b], r64, 4, b))
        seen_nan = seen_nan or bool(np.isnan(r64).any())
    if not with_row:                                                  # the planted boundary ratios meet each other on the identity row
        ref = M.f0_stats(fx[0, :130], fy[0, :67])
        one = M.f0_stats(fx[0, 15:17], fy[0, 15:17])
        assert (one["n_vv"], one["n_gpe"]) == (2, 1) and ref["n_gpe"] >= 1
    assert counts[:, 2].sum() > 0 and counts[:, 3].sum() > 0
    report(f"METRICS f0 (row={'dtw' if with_row else 'NULL'}): values within {worst:.2f} fp32 ulp of the definition; NaN rows seen: {seen_nan}")


def test_f0_all_unvoiced_and_constant_tracks():
    fx = torch.zeros(3, 70, device=DEV)
    fy = torch.zeros(3, 70, device=DEV)
    fx[1], fy[1] = 150.0, torch.linspace(100, 200, 70, device=DEV)       # a constant track: no correlation
    fx[2, :5], fy[2, 5:9] = 120.0, 130.0                                  # voiced on one side only
    xl = torch.tensor([70, 70, 70], dtype=torch.int32, device=DEV)
    counts, vals = _f0_dev(fx, fy, xl, xl, None)
    for b in range(3):
        ref = M.f0_stats(fx[b].cpu().numpy(), fy[b].cpu().numpy())
        assert counts[b].tolist() == [ref["n"], ref["n_vv"], ref["n_gpe"], ref["n_vde"]], b
        _within_ulps(vals[b], [float(ref[k]) for k in ("rmse_cents", "mae_cents", "corr")], 4, b)
    assert np.isnan(vals[0]).all() and np.isnan(vals[2]).all() and counts[2].tolist() == [70, 0, 0, 9]
    assert np.isnan(vals[1, 2]) and not np.isnan(vals[1, :2]).any()


# ----------------------------------------------------------------------------- 4. the images and their SSIM

@pytest.mark.parametrize("with_row", [True, False])
@pytest.mark.parametrize("Cimg", [11, 20])
def test_ssim_prepare_and_ssim(Cimg, with_row):
    s = _shared()
    row_d = s["row"] if with_row else None
    u, v, mm = _prepare_dev(s["cx"], s["cy"], s["xl"], s["yl"], row_d, Cimg)
    cx, cy, row = s["cx"].cpu().numpy(), s["cy"].cpu().numpy(), s["row"].cpu().numpy()
    uh, vh, mmh = u.cpu().numpy(), v.cpu().numpy(), mm.cpu().numpy()
    for b, (a, r) in enumerate(PAIRS):
        ur, vr, _ = M.ssim_images(cx[b, :a], cy[b, :r], row[b, :r] if with_row else None, Cimg)
        assert np.isnan(uh[b, r:]).all() and np.isnan(vh[b, r:]).all(), b               # padding rows untouched
        assert (np.abs(uh[b, :r].astype(np.float64) - ur) <= MC.ulp32(ur)).all() and (np.abs(vh[b, :r].astype(np.float64) - vr) <= MC.ulp32(vr)).all(), b
        both = np.concatenate([uh[b, :r].ravel(), vh[b, :r].ravel()])
        assert mmh[b, 0] == both.min() and mmh[b, 1] == both.max(), b                   # of the device's own u, v
    rng = (mm[:, 1].max() - mm[:, 0].min()).reshape(1)
    L = np.float32(mmh[:, 1].max() - mmh[:, 0].min())
    assert rng.cpu().numpy()[0] == L
    got = _ssim_dev(u, v, s["yl"], rng).cpu().numpy()
    worst = 0.0
    for b, (a, r) in enumerate(PAIRS):
        ref = M.ssim(uh[b, :r], vh[b, :r], L)                         # float64 on the device's own images
        if r < 11:
            assert np.isnan(ref) and np.isnan(got[b]), b
            continue
        m = M.ssim_map(uh[b, :r], vh[b, :r], L)
        assert m.shape == (r - 10, Cimg - 10)
        err = abs(float(got[b]) - float(m.sum() / m.size))
        assert err <= U23, (b, err)
        worst = max(worst, err)
    assert PAIRS[4][1] == 11 and PAIRS[5][1] == 12 and np.isnan(got[6])
    # a pair alone, in buffers of its own size, has the bits of the pair in the batch
    for b in (0, 1, 4, 5):
        a, r = PAIRS[b]
        alone = _ssim_dev(u[b:b + 1, :r].contiguous(), v[b:b + 1, :r].contiguous(), s["yl"][b:b + 1], rng).cpu().numpy()
        assert alone.tobytes() == got[b:b + 1].tobytes(), b
        xl1, yl1 = s["xl"][b:b + 1], s["yl"][b:b + 1]
        r1 = s["row"][b:b + 1, :r].contiguous() if with_row else None
        u1, v1, mm1 = _prepare_dev(s["cx"][b:b + 1, :a].contiguous(), s["cy"][b:b + 1, :r].contiguous(), xl1, yl1, r1, Cimg)
        assert torch.equal(u1[0], u[b, :r]) and torch.equal(v1[0], v[b, :r]) and torch.equal(mm1[0], mm[b]), b
    report(f"METRICS ssim C={Cimg} (row={'dtw' if with_row else 'NULL'}): max |ssim - f64| = {worst:.2e} (bound 2^-23 = {U23:.2e})")


def test_ssim_of_images_with_themselves_and_below_eleven_columns():
    s = _shared()
    u, _, mm = _prepare_dev(s["cy"], s["cy"], s["yl"], s["yl"], None, 20)
    rng = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
    got = _ssim_dev(u, u, s["yl"], rng).cpu().numpy()
    assert (got[:6] == 1.0).all() and np.isnan(got[6])
    u10 = u[:, :, :10].contiguous()
    assert np.isnan(_ssim_dev(u10, u10, s["yl"], rng).cpu().numpy()).all()


# ----------------------------------------------------------------------------- 5. the host surface

def test_score_pairs_is_the_definition_for_all_pairs_in_one_call():
    host = _host()
    s = _shared()
    x, y, fx, fy = MC.inputs()
    xl, yl = MC.lens()
    emb = torch.from_numpy(np.random.RandomState(3).standard_normal((2, B, 16)).astype(np.float32)).to(DEV)
    out = host.score_pairs(torch.from_numpy(x).to(DEV), xl, torch.from_numpy(y).to(DEV), yl, f0_syn=s["fx"], f0_rec=s["fy"], emb_syn=emb[0],
                           emb_rec=emb[1])
    for k in ("mcd", "ssim", "ffe", "gpe", "vde", "f0_rmse_cents", "f0_mae_cents", "f0_corr", "path_len", "speaker_cos"):
        assert out[k].shape == (B,) and out[k].is_cuda, k
    assert out["row"].shape == (B, TR) and out["row"].dtype == torch.int32 and out["counts"].shape == (B, 4)
    assert torch.equal(host.mel_cepstra(torch.from_numpy(x).to(DEV), xl, 20)[0, :130], s["cx"][0, :130])
    cx, cy, cost = s["cx"].cpu().numpy(), s["cy"].cpu().numpy(), s["cost"].cpu().numpy()
    L = float(out["data_range"].cpu()[0])
    row = out["row"].cpu().numpy()
    u, v, _ = _prepare_dev(s["cx"], s["cy"], s["xl"], s["yl"], out["row"], 20)
    uh, vh = u.cpu().numpy(), v.cpu().numpy()
    o = {k: t.cpu().numpy() for k, t in out.items()}
    for b, (a, r) in enumerate(PAIRS):
        ref = M.score(x[b], a, y[b], r, f0_syn=fx[b], f0_rec=fy[b], data_range=L, cepstra_syn=cx[b], cepstra_rec=cy[b],
                      cost_matrix=cost[b, :a, :r])
        assert o["mcd"][b].tobytes() == ref["mcd"].tobytes() and o["path_len"][b] == ref["path_len"] and np.array_equal(row[b, :r], ref["row"]), b
        assert o["counts"][b].tolist() == [ref["n"], ref["n_vv"], ref["n_gpe"], ref["n_vde"]], b
        for k in ("ffe", "gpe", "vde"):
            assert o[k][b].tobytes() == ref[k].tobytes() or (np.isnan(o[k][b]) and np.isnan(ref[k])), (b, k)
        _within_ulps([o["f0_rmse_cents"][b], o["f0_mae_cents"][b], o["f0_corr"][b]],
                     [float(ref[k]) for k in ("f0_rmse_cents", "f0_mae_cents", "f0_corr")], 4, b)
        if r < 11:
            assert np.isnan(o["ssim"][b]) and np.isnan(ref["ssim"]), b
        else:
            m = M.ssim_map(uh[b, :r], vh[b, :r], np.float32(L))       # on the device's own images, as in test_ssim_prepare_and_ssim
            assert abs(float(o["ssim"][b]) - float(m.sum() / m.size)) <= U23, b
        cos = float(np.dot(emb[0, b].cpu().numpy().astype(np.float64), emb[1, b].cpu().numpy().astype(np.float64))
                    / np.linalg.norm(emb[0, b].cpu().numpy().astype(np.float64)) / np.linalg.norm(emb[1, b].cpu().numpy().astype(np.float64)))
        assert abs(float(o["speaker_cos"][b]) - cos) <= 64 * U24, b      # an fp32 dot product of 16 terms and two norms: (16 + 2 * 9 + a few) roundings
    # the frame-by-frame mode: the diagonal of the same cost
    fr = host.score_pairs(torch.from_numpy(x).to(DEV), xl, torch.from_numpy(y).to(DEV), yl, align="frame")
    for b, (a, r) in enumerate(PAIRS):
        t_ref, n_ref = M.diagonal(np.ascontiguousarray(cost[b, :a, :r]))
        assert fr["mcd"][b].cpu().numpy().tobytes() == M.mcd(t_ref, n_ref).tobytes() and int(fr["path_len"][b]) == n_ref, b
        assert fr["row"][b, :r].cpu().tolist() == np.minimum(np.arange(r), a - 1).tolist(), b
    assert "ffe" not in fr and "speaker_cos" not in fr


def test_a_stretched_log_mel_scores_zero_and_gives_the_known_row():
    host = _host()
    rs = np.random.RandomState(9)
    lens = [50, 37]
    mel = torch.from_numpy((MC.LOG_LO + (MC.LOG_HI - MC.LOG_LO) * rs.rand(2, 50, 80)).astype(np.float32)).to(DEV)
    reps = [rs.randint(1, 4, size=n) for n in lens]
    rec_lens = [int(r.sum()) for r in reps]
    rec = torch.zeros(2, max(rec_lens), 80, device=DEV)
    for b in range(2):
        rec[b, :rec_lens[b]] = torch.repeat_interleave(mel[b, :lens[b]], torch.from_numpy(reps[b]).to(DEV), dim=0)
    out = host.score_pairs(mel, lens, rec, rec_lens)
    assert out["mcd"].cpu().tolist() == [0.0, 0.0] and out["path_len"].cpu().tolist() == rec_lens
    for b in range(2):
        assert out["row"][b, :rec_lens[b]].cpu().tolist() == np.repeat(np.arange(lens[b]), reps[b]).tolist(), b
        assert abs(float(out["ssim"][b]) - 1.0) <= U23
    frame = host.score_pairs(mel, lens, rec, rec_lens, align="frame")
    assert (frame["mcd"] > 0).all() and frame["path_len"].cpu().tolist() == lens


def test_score_audio_of_a_signal_with_itself():
    host = _host()
    n = 2 * PC.FS
    f = np.linspace(120.0, 220.0, n)
    w = PC.harmonic(f).astype(np.float32)
    w[n // 2:n // 2 + 6000] = 0.0                                     # a stretch without voice
    an, pt = host.get_analyzer(device=DEV), host.get_pitch_tracker(device=DEV)
    out = host.score_audio(an, pt, w[None], w[None])
    T = 1 + n // 256
    assert out["row"].shape == (1, T) and out["row"][0].cpu().tolist() == list(range(T)) and int(out["path_len"][0]) == T
    assert float(out["mcd"][0]) == 0.0 and float(out["ffe"][0]) == 0.0 and abs(float(out["ssim"][0]) - 1.0) <= U23
    c = out["counts"][0].cpu().tolist()
    assert c[0] == T and 0 < c[1] < T and c[2] == 0 and c[3] == 0
    assert float(out["f0_rmse_cents"][0]) == 0.0 and abs(float(out["f0_corr"][0]) - 1.0) <= U23
    with pytest.raises(ValueError):
        host.score_audio(an, pt, w[None], np.stack([w, w]))
