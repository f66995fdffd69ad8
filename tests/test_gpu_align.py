"""Alignment of a recording to its phonemes on the GPU (include/cmtts_hip.h: cmtts_align_cost, cmtts_align_dtw, cmtts_align_durations;
csrc/align.hip; host.dtw_align / align_recording): the cost against the float64 definition with the definition's own float32
arm as the yardstick and the padding untouched; the DP, the walk back and the durations bit for bit the definition, on the device's own cost
and on tie-heavy integer matrices, across wave, strip and band edges; a rendering stretched by known counts aligned end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmtts_amd import _lib, align as A, noise as N
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from conftest import report

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Side lengths from {1, 2, 63, 64, 65, 130, 257}: below, at and above a strip of 64 rows / a tile of 64 columns, several strips, both Ts > Tr
# and Tr > Ts.  The buffers are wider than the longest pair (260 x 259), so every pair has padding.
PAIRS = [(257, 130), (130, 257), (65, 64), (64, 65), (63, 2), (2, 63), (1, 257), (257, 1), (1, 1), (257, 257), (64, 64), (130, 63)]
TS, TR, L = 260, 259, 12

# The bound of test_cost_against_float64.  Yardstick: align.cost(dtype=float32) — numpy's float32 mean, differences and sums — against its
# float64 arm on the inputs of _inputs(), relative to the pair's largest cost, worst over PAIRS (measured with numpy 2.2: 1.508e-7 at pair
# (64, 65), 7.6e-8 to 1.2e-7 on the others; the issue's 9.6e-8 was one 65 x 64 pair; the test prints the live figure).  The kernel gets 4 x that: its sums associate differently
# (ten fused chains of eight terms, added in order).  Measured on MI355X: 1.73e-7.  BOUND_COST = 6.04e-7.
YARDSTICK_COST = 1.51e-7
BOUND_COST = 4 * YARDSTICK_COST

_CACHE = {}


def _host():
    from cmtts_amd import host
    return host


def _inputs():
    """x ~ N(0, 1) [B, TS, 80]; y: x resampled to the pair's recording length + 5 % noise (a rendering of one or two
    frames: N(0, 1), so that no side is constant); NaN beyond the lengths; d_syn [B, L] with zeros.
    Computed once, shared, never written."""
    if "in" not in _CACHE:
        rs = np.random.RandomState(7)
        B = len(PAIRS)
        x = np.full((B, TS, 80), np.nan, np.float32)
        y = np.full((B, TR, 80), np.nan, np.float32)
        d = np.zeros((B, L), np.int32)
        for b, (xl, yl) in enumerate(PAIRS):
            x[b, :xl] = rs.standard_normal((xl, 80))
            y[b, :yl] = x[b, (np.arange(yl) * xl) // yl] + 0.05 * rs.standard_normal((yl, 80)) if xl > 2 else rs.standard_normal((yl, 80))
            cuts = np.sort(rs.randint(0, xl + 1, size=L - 1))
            d[b] = np.diff(np.concatenate([[0], cuts, [xl]]))
        c64 = [A.cost(x[b], xl, y[b], yl) for b, (xl, yl) in enumerate(PAIRS)]
        _CACHE["in"] = (x, y, d, c64)
    return _CACHE["in"]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _hp(a):
    return C.c_void_p(a.ctypes.data)


def _lens(pairs):
    return np.asarray([p[0] for p in pairs], np.int32), np.asarray([p[1] for p in pairs], np.int32)


def _ws(B, Ts, Tr):
    nb = _lib.load().cmtts_align_workspace_bytes(B, Ts, Tr)
    return torch.empty(nb, dtype=torch.uint8, device=DEV), nb


def _cost_dev(x, y, pairs, normalise=True):
    """cmtts_align_cost into a NaN-filled buffer."""
    lib = _lib.load()
    B, Ts, Tr = x.shape[0], x.shape[1], y.shape[1]
    xl, yl = _lens(pairs)
    cost = torch.full((B, Ts, Tr), float("nan"), dtype=torch.float32, device=DEV)
    ws, nb = _ws(B, Ts, Tr)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.cmtts_align_cost(_p(x), _hp(xl), Ts, _p(y), _hp(yl), Tr, B, 80, int(normalise), _p(cost), _p(ws), nb, st))
    torch.cuda.synchronize()
    return cost


def _dtw_dev(cost, pairs, d_syn):
    """cmtts_align_dtw + cmtts_align_durations on a cost matrix of the test's choice: (row with -7 where nothing is written, total, path_len,
    d_rec, phoneme_cost) as host arrays."""
    lib = _lib.load()
    B, Ts, Tr = cost.shape
    xl, yl = _lens(pairs)
    d_host = np.ascontiguousarray(d_syn, np.int32)
    d_dev = torch.from_numpy(d_host).to(DEV)
    row = torch.full((B, Tr), -7, dtype=torch.int32, device=DEV)
    total = torch.empty(B, dtype=torch.float32, device=DEV)
    n = torch.empty(B, dtype=torch.int32, device=DEV)
    d_rec = torch.empty(B, d_host.shape[1], dtype=torch.int32, device=DEV)
    pc = torch.empty(B, d_host.shape[1], dtype=torch.float32, device=DEV)
    ws, nb = _ws(B, Ts, Tr)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.cmtts_align_dtw(_p(cost), _hp(xl), _hp(yl), B, Ts, Tr, _p(row), _p(total), _p(n), _p(ws), nb, st))
    _lib.check(lib.cmtts_align_durations(_p(row), _p(cost), _p(d_dev), _hp(d_host), _hp(xl), _hp(yl), B, Ts, Tr, d_host.shape[1], _p(d_rec), _p(pc),
                                         _p(ws), nb, st))
    torch.cuda.synchronize()
    _host().check_async_error()
    return row.cpu().numpy(), total.cpu().numpy(), n.cpu().numpy(), d_rec.cpu().numpy(), pc.cpu().numpy()


def _same_as_definition(cost_host, pairs, d_syn, got, tag):
    """row, total, path length, durations and phoneme cost of every pair: the definition's bits."""
    row, total, n, d_rec, pc = got
    for b, (xl, yl) in enumerate(pairs):
        c = np.ascontiguousarray(cost_host[b, :xl, :yl])
        t_ref, n_ref, row_ref = A.dtw(c)
        d_ref, pc_ref = A.durations(row_ref, c, d_syn[b])
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        assert torch.equal(f(row[b, :yl]), f(row_ref)), (tag, b, xl, yl)
        assert (row[b, yl:] == -7).all(), (tag, b)
        assert torch.equal(f(total[b:b + 1]), f(np.asarray([t_ref], np.float32))) and n[b] == n_ref, (tag, b, total[b], t_ref, n[b], n_ref)
        assert torch.equal(f(d_rec[b].astype(np.int64)), f(d_ref)) and torch.equal(f(pc[b]), f(pc_ref)), (tag, b)
        assert d_rec[b].sum() == yl


# ----------------------------------------------------------------------------- 1. the cost

def test_cost_against_float64():
    x, y, _, c64 = _inputs()
    yard = max(float(np.abs(A.cost(x[b], xl, y[b], yl, dtype=np.float32) - c64[b]).max() / c64[b].max())
               for b, (xl, yl) in enumerate(PAIRS) if c64[b].max() > 0)
    cost = _cost_dev(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), PAIRS)
    got = cost.cpu().numpy()
    err = 0.0
    for b, (xl, yl) in enumerate(PAIRS):
        valid = np.zeros((TS, TR), bool)
        valid[:xl, :yl] = True
        assert np.isnan(got[b][~valid]).all(), b               # the NaN the buffer was filled with: nothing written beyond the lengths
        assert np.isfinite(got[b][valid]).all(), b             # and no NaN of the inputs' padding read
        if c64[b].max() > 0:
            err = max(err, float(np.abs(got[b, :xl, :yl].astype(np.float64) - c64[b]).max() / c64[b].max()))
        else:
            assert not got[b, :xl, :yl].any()                  # one frame a side: both are their own mean
    report(f"ALIGN cost: max|c - f64| / max c: kernel {err:.2e}, numpy float32 {yard:.2e} (pinned {YARDSTICK_COST:.2e}, bound {BOUND_COST:.2e})")
    assert err <= BOUND_COST, err


def test_cost_without_normalisation_and_alone():
    x, y, _, _ = _inputs()
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    full = _cost_dev(xd, yd, PAIRS)
    for b in (0, 1, 4, 8):
        xl, yl = PAIRS[b]
        alone = _cost_dev(xd[b:b + 1, :xl].contiguous(), yd[b:b + 1, :yl].contiguous(), [PAIRS[b]])
        assert torch.equal(alone[0], full[b, :xl, :yl]), b      # a pair's cost does not depend on its batch or on the buffers' widths
    raw = _cost_dev(xd, yd, PAIRS, normalise=False).cpu().numpy()
    for b in (0, 3, 8):
        xl, yl = PAIRS[b]
        ref = A.cost(x[b], xl, y[b], yl, normalise=False)
        assert np.abs(raw[b, :xl, :yl] - ref).max() <= BOUND_COST * ref.max()


# ----------------------------------------------------------------------------- 2. DP, walk back, durations: bit for bit

def test_dtw_on_the_device_cost():
    x, y, d, _ = _inputs()
    cost = _cost_dev(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), PAIRS)
    got = _dtw_dev(cost, PAIRS, d)
    _same_as_definition(cost.cpu().numpy(), PAIRS, d, got, "device cost")
    # a row alone, in buffers of its own size (another number of waves), equals the row inside the batch
    for b in (0, 1, 3, 6, 9):
        xl, yl = PAIRS[b]
        alone = _dtw_dev(cost[b:b + 1, :xl, :yl].contiguous(), [PAIRS[b]], d[b:b + 1])
        assert np.array_equal(alone[0][0], got[0][b, :yl]) and alone[1][0].tobytes() == got[1][b].tobytes() and alone[2][0] == got[2][b], b
        assert np.array_equal(alone[3][0], got[3][b]) and alone[4][0].tobytes() == got[4][b].tobytes(), b


@pytest.mark.parametrize("kind", ["zeros", "small_integers", "plateaus"])
def test_dtw_on_tie_heavy_integer_costs(kind):
    _, _, d, _ = _inputs()
    rs = np.random.RandomState(11)
    c = np.full((len(PAIRS), TS, TR), np.nan, np.float32)
    for b, (xl, yl) in enumerate(PAIRS):
        if kind == "zeros":
            c[b, :xl, :yl] = 0.0
        elif kind == "small_integers":
            c[b, :xl, :yl] = rs.randint(0, 4, size=(xl, yl))
        else:                                                   # blocks of equal cost, 0 along a staircase: ties on every side of the path
            c[b, :xl, :yl] = np.abs(np.arange(xl)[:, None] // 7 - (np.arange(yl)[None, :] * max(xl, 1) // max(yl, 1)) // 7)
    got = _dtw_dev(torch.from_numpy(c).to(DEV), PAIRS, d)
    _same_as_definition(c, PAIRS, d, got, kind)


def test_dtw_across_bands_and_with_nan():
    """More than 16 strips of 64 rows: the second band of strips takes the first band's last row from LDS.  And a matrix with NaN cells: a NaN
    never wins a comparison, and the walk ends."""
    rs = np.random.RandomState(13)
    pairs = [(1100, 70), (1030, 129)]
    Ts, Tr = 1100, 130
    c = np.full((2, Ts, Tr), np.nan, np.float32)
    d = np.zeros((2, L), np.int32)
    for b, (xl, yl) in enumerate(pairs):
        c[b, :xl, :yl] = rs.randint(0, 6, size=(xl, yl)) + (rs.rand(xl, yl) < 0.5) * rs.rand(xl, yl)
        d[b] = np.diff(np.concatenate([[0], np.sort(rs.randint(0, xl + 1, size=L - 1)), [xl]]))
    got = _dtw_dev(torch.from_numpy(c).to(DEV), pairs, d)
    _same_as_definition(c, pairs, d, got, "bands")
    cn = rs.rand(1, 70, 90).astype(np.float32)
    cn[0, rs.rand(70, 90) < 0.1] = np.nan
    cn[0, -1, -1] = 1.0
    dn = np.asarray([[70] + [0] * (L - 1)], np.int32)
    row, total, n, d_rec, _ = _dtw_dev(torch.from_numpy(cn).to(DEV), [(70, 90)], dn)
    t_ref, n_ref, row_ref = A.dtw(cn[0])
    assert np.array_equal(row[0], row_ref) and n[0] == n_ref and d_rec[0].tolist() == [90] + [0] * (L - 1)
    assert total[0].tobytes() == np.float32(t_ref).tobytes() or (np.isnan(total[0]) and np.isnan(t_ref))


def test_dtw_align_returns_the_definition():
    host = _host()
    x, y, d, _ = _inputs()
    sub = [0, 1, 3, 5]
    pairs = [PAIRS[b] for b in sub]
    xl, yl = _lens(pairs)
    out = host.dtw_align(torch.from_numpy(x[sub]).to(DEV), xl, torch.from_numpy(d[sub]), torch.from_numpy(y[sub]).to(DEV), yl)
    assert out["d_targets"].dtype == torch.int64 and out["d_targets"].shape == (4, L) and out["d_targets"].is_cuda
    assert out["phoneme_cost"].dtype == torch.float32 and out["row"].dtype == torch.int32 and out["row"].shape == (4, TR) and out["cost"].shape == (4,)
    assert out["d_targets"].sum(1).cpu().tolist() == yl.tolist()
    cost = _cost_dev(torch.from_numpy(x[sub]).to(DEV), torch.from_numpy(y[sub]).to(DEV), pairs).cpu().numpy()
    for k, (a, b) in enumerate(pairs):
        c = np.ascontiguousarray(cost[k, :a, :b])
        t_ref, n_ref, row_ref = A.dtw(c)
        d_ref, pc_ref = A.durations(row_ref, c, d[sub[k]])
        assert out["d_targets"][k].cpu().tolist() == d_ref.tolist() and np.array_equal(out["row"][k, :b].cpu().numpy(), row_ref)
        assert np.array_equal(out["phoneme_cost"][k].cpu().numpy(), pc_ref)
        assert abs(float(out["cost"][k]) - float(t_ref) / n_ref) <= 1e-6 * float(t_ref) / n_ref
    assert A.spans_of(out["d_targets"], [(0, 0, L)]) == [(0, 0, int(yl[0]))]


# ----------------------------------------------------------------------------- 3. end to end

def test_align_recording_recovers_a_known_stretch():
    host = _host()
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=5))
    rs = np.random.RandomState(4)
    B, Lp = 2, 10
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, Lp)).astype(np.int64))
    texts[1, 7:] = 0
    src = torch.tensor([10, 7])
    spk = torch.from_numpy(rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32))
    seeds = N.utterance_seeds(9, np.arange(B))
    out = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk)
    d_syn = out["d_rounded"].to(torch.int64).cpu().numpy()
    lens = out["mel_lens"].cpu().tolist()
    assert d_syn.sum(1).tolist() == lens and min(lens) >= 8 and (d_syn[1, 7:] == 0).all()
    mel = host.sample_with_cond(model, out["cond_ct"], out["speaker_emb"], 4, seeds=seeds).clone()
    for b in range(B):
        m = mel[b, :lens[b]]
        assert not (m[1:] == m[:-1]).all(dim=1).any(), b          # no two neighbouring frames bitwise equal: the stretch below can be told
    reps = [rs.randint(1, 4, size=n) for n in lens]
    rec_lens = [int(r.sum()) for r in reps]
    mel_rec = torch.zeros(B, max(rec_lens), cfg.n_mels, device=DEV)
    for b in range(B):
        mel_rec[b, :rec_lens[b]] = torch.repeat_interleave(mel[b, :lens[b]], torch.from_numpy(reps[b]).to(DEV), dim=0)
    res = host.align_recording(model, texts, src, mel_rec, rec_lens, spker_embeds=spk, seeds=seeds)
    assert torch.equal(res["mel_syn"], mel) and res["d_syn"].cpu().tolist() == d_syn.tolist()
    want = np.zeros((B, Lp), np.int64)
    for b in range(B):
        want[b] = np.bincount(np.repeat(np.arange(Lp), d_syn[b]), weights=reps[b], minlength=Lp)
    assert res["d_targets"].cpu().tolist() == want.tolist()
    assert res["row"][0, :rec_lens[0]].cpu().tolist() == np.repeat(np.arange(lens[0]), reps[0]).tolist()
    # the alignment is what the teacher-forced calls take: unchanged, still on the device
    tf = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, d_targets=res["d_targets"])
    assert tf["mel_lens"].cpu().tolist() == rec_lens
    an = host.get_analyzer(device=DEV)
    energy = torch.rand(B, max(rec_lens), device=DEV) * 30.0
    e = host.energy_targets(an, energy, res["d_targets"], 21.7, 9.3)
    assert e.shape == (B, Lp) and bool(torch.isfinite(e).all())
    spans = A.spans_of(res["d_targets"], [(0, 2, 5)])
    assert spans == [(0, int(want[0, :2].sum()), int(want[0, :5].sum()))]
