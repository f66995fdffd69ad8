"""Alignment of a recording to its phonemes, CPU side: the numpy definition (cmtts_amd/align.py) on the cases whose answer is known — a pure
stretch is recovered exactly, deleted frames keep the invariants, the tie-breaks are pinned on integer matrices — spans_of, the bound entry
points, and the refusals of the entry points and of the host layer, which leave a message and touch no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import align as A


def _case(seed, lo=1):
    """x ~ N(0, 1) [Ts, 80], d_syn in 0 .. 5 (first and last >= 1), every frame repeated lo .. 3 times (0 only in the interior), 5 % noise."""
    rs = np.random.RandomState(seed)
    L = 3 + seed % 9
    d = rs.randint(0, 6, size=L)
    d[0], d[-1] = max(d[0], 1), max(d[-1], 1)
    Ts = int(d.sum())
    x = rs.standard_normal((Ts, 80)).astype(np.float32)
    rep = rs.randint(lo, 4, size=Ts)
    rep[0], rep[-1] = max(rep[0], 1), max(rep[-1], 1)
    y = (np.repeat(x, rep, axis=0) + 0.05 * rs.standard_normal((int(rep.sum()), 80))).astype(np.float32)
    return x, y, d, rep


def _plain_dtw(c):
    """The recurrence and the walk written cell by cell, rows outermost: another evaluation order than align.accumulate's anti-diagonals."""
    Ts, Tr = c.shape
    D = np.zeros((Ts, Tr), np.float32)
    S = np.zeros((Ts, Tr), np.uint8)
    for i in range(Ts):
        for j in range(Tr):
            if i == 0 and j == 0:
                D[i, j] = c[i, j]
                continue
            if i == 0:
                best, s = D[i, j - 1], A.LEFT
            elif j == 0:
                best, s = D[i - 1, j], A.UP
            else:
                best, s = D[i - 1, j - 1], A.DIAG
                if D[i - 1, j] < best:
                    best, s = D[i - 1, j], A.UP
                if D[i, j - 1] < best:
                    best, s = D[i, j - 1], A.LEFT
            D[i, j] = np.float32(c[i, j] + best)
            S[i, j] = s
    i, j = Ts - 1, Tr - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        s = S[i, j]
        i, j = i - (s != A.LEFT), j - (s != A.UP)
        path.append((i, j))
    row = np.zeros(Tr, np.int32)
    for j in range(Tr):
        pts = sorted(i for i, jj in path if jj == j)
        row[j] = min(pts, key=lambda i: (c[i, j], i))
    return D[-1, -1], len(path), row, path


# ----------------------------------------------------------------------------- what the alignment must recover

@pytest.mark.parametrize("seed", range(20))
def test_pure_stretch_is_recovered_exactly(seed):
    x, y, d, rep = _case(seed)
    Ts, Tr = len(x), len(y)
    got = A.align(x, Ts, y, Tr, d)
    owner = np.repeat(np.arange(len(d)), d)
    want = np.bincount(owner, weights=rep, minlength=len(d)).astype(np.int64)
    assert np.array_equal(got["d_rec"], want), (got["d_rec"], want)
    assert np.array_equal(got["row"], np.repeat(np.arange(Ts), rep))
    assert got["d_rec"].sum() == Tr and got["path_len"] == Tr and got["cost"] == np.float32(got["total"] / np.float32(Tr))
    # the float32 cost gives the path of the float64 cost
    c32 = A.cost(x, Ts, y, Tr, dtype=np.float32)
    c64 = A.cost(x, Ts, y, Tr)
    assert c32.dtype == np.float32 and c64.dtype == np.float64 and c32.shape == (Ts, Tr)
    _, n32, row32 = A.dtw(c32)
    _, n64, row64 = A.dtw(c64.astype(np.float32))
    assert n32 == n64 and np.array_equal(row32, row64)
    # the phoneme cost is the mean of the matched cells, and small against an unmatched cell
    assert (got["phoneme_cost"][d == 0] == 0).all() and (got["phoneme_cost"][d > 0] < 0.05 * np.median(c64)).all()


@pytest.mark.parametrize("seed", range(20))
def test_deleted_frames_keep_the_invariants(seed):
    x, y, d, rep = _case(100 + seed, lo=0)
    got = A.align(x, len(x), y, len(y), d)
    assert got["d_rec"].sum() == len(y)
    assert (np.diff(got["row"]) >= 0).all() and got["row"][0] == 0 and got["row"][-1] == len(x) - 1
    assert (got["d_rec"][d == 0] == 0).all() and (got["phoneme_cost"][got["d_rec"] == 0] == 0).all()
    assert max(len(x), len(y)) <= got["path_len"] <= len(x) + len(y) - 1


def test_cost_normalisation_and_lengths():
    rs = np.random.RandomState(3)
    x, y = rs.standard_normal((9, 80)).astype(np.float32), rs.standard_normal((12, 80)).astype(np.float32)
    c = A.cost(x, 7, y, 10)
    xm, ym = x[:7].astype(np.float64) - x[:7].mean(0, dtype=np.float64), y[:10].astype(np.float64) - y[:10].mean(0, dtype=np.float64)
    np.testing.assert_allclose(c, ((xm[:, None] - ym[None]) ** 2).sum(-1), rtol=1e-13)
    # a level or microphone difference (a constant per channel) drops out; without normalise it does not
    shift = rs.standard_normal(80).astype(np.float32)
    np.testing.assert_allclose(A.cost(x + shift, 7, y, 10), c, atol=1e-4)
    raw = A.cost(x, 7, y, 10, normalise=False)
    np.testing.assert_allclose(raw, ((x[:7, None].astype(np.float64) - y[None, :10]) ** 2).sum(-1), rtol=1e-13)
    assert np.abs(A.cost(x + shift, 7, y, 10, normalise=False) - raw).max() > 1.0
    for bad in ((x, 0, y, 10), (x, 10, y, 10), (x, 7, y, 13), (x[:, :79], 7, y, 10)):
        with pytest.raises(ValueError):
            A.cost(*bad)


# ----------------------------------------------------------------------------- the tie-breaks, on integer-valued matrices

def test_all_zero_cost_walks_the_diagonal_then_the_edge():
    tot, n, row = A.dtw(np.zeros((3, 5), np.float32))         # (2,4) (1,3) (0,2) then left along row 0
    assert tot == 0 and n == 5 and row.tolist() == [0, 0, 0, 1, 2]
    tot, n, row = A.dtw(np.zeros((5, 3), np.float32))         # (4,2) (3,1) (2,0) then up along column 0: its run 2, 1, 0 ties to the smallest row
    assert tot == 0 and n == 5 and row.tolist() == [0, 3, 4]
    tot, n, row = A.dtw(np.zeros((4, 4), np.float32))
    assert n == 4 and row.tolist() == [0, 1, 2, 3]


def test_small_integer_costs_pinned():
    c = np.asarray([[0, 1, 3, 2],
                    [2, 0, 0, 3],
                    [1, 2, 0, 0],
                    [3, 1, 2, 0],
                    [2, 2, 1, 0]], np.float32)
    D, step = A.accumulate(c)
    assert D.tolist() == [[0, 1, 4, 6], [2, 0, 0, 3], [3, 2, 0, 0], [6, 3, 2, 0], [8, 5, 3, 0]]
    # (1,2): diagonal 1, up 4, left 0 -> left; (2,3): diagonal 0, up 3, left 0 -> the diagonal keeps the tie; (4,3): diagonal 2, up 0 -> up
    assert step[1, 2] == A.LEFT and step[2, 3] == A.DIAG and step[4, 3] == A.UP and step[2, 2] == A.DIAG
    tot, n, row = A.dtw(c)
    # the path: (4,3) up to (3,3), whose diagonal keeps the tie with up, then (2,2) (1,1) (0,0); column 3 holds rows 3 and 4 at cost 0: the smaller wins
    assert step[3, 3] == A.DIAG and tot == 0 and n == 5 and row.tolist() == [0, 1, 2, 3]
    rs = np.random.RandomState(5)
    for Ts, Tr in ((7, 9), (9, 7), (1, 6), (6, 1), (12, 12)):
        c = rs.randint(0, 4, size=(Ts, Tr)).astype(np.float32)
        tot, n, row = A.dtw(c)
        ptot, pn, prow, path = _plain_dtw(c)
        assert tot == ptot and n == pn and np.array_equal(row, prow), (Ts, Tr)
        assert path[0] == (Ts - 1, Tr - 1) and path[-1] == (0, 0)


def test_single_row_and_single_column():
    c = np.asarray([[3, 1, 2, 5]], np.float32)
    tot, n, row = A.dtw(c)
    assert tot == 11 and n == 4 and row.tolist() == [0, 0, 0, 0]
    d_rec, pc = A.durations(row, c, [0, 1, 0])
    assert d_rec.tolist() == [0, 4, 0] and pc.tolist() == [0, 11 / 4, 0]
    tot, n, row = A.dtw(c.T.copy())
    assert tot == 11 and n == 4 and row.tolist() == [1]       # the cheapest of the column's four rows
    tot, n, row = A.dtw(np.asarray([[7]], np.float32))
    assert tot == 7 and n == 1 and row.tolist() == [0]
    # a NaN never wins a comparison and the walk still ends
    c = np.full((4, 5), np.nan, np.float32)
    tot, n, row = A.dtw(c)
    assert np.isnan(tot) and n == 5 and (np.diff(row) >= 0).all()


def test_durations():
    c = np.arange(20, dtype=np.float32).reshape(4, 5)
    row = np.asarray([0, 0, 1, 3, 3], np.int32)
    d_rec, pc = A.durations(row, c, [1, 0, 2, 1])              # phoneme 2 owns rendering frames 1 and 2, phoneme 3 frame 3
    assert d_rec.tolist() == [2, 0, 1, 2] and d_rec.dtype == np.int64 and pc.dtype == np.float32
    assert pc.tolist() == [(0 + 1) / 2, 0, 7.0, (18 + 19) / 2]
    for bad_d in ([1, 1, 1], [2, -1, 2, 1]):
        with pytest.raises(ValueError, match="sum"):
            A.durations(row, c, bad_d)
    with pytest.raises(ValueError, match="non-decreasing"):
        A.durations(np.asarray([0, 1, 0, 3, 3]), c, [1, 0, 2, 1])


def test_spans_of():
    d = np.asarray([[2, 0, 3, 1, 4], [1, 1, 0, 0, 5]])
    assert A.spans_of(d, [(0, 0, 1), (0, 2, 4), (1, 1, 5), (0, 1, 3)]) == [(0, 0, 2), (0, 2, 6), (1, 1, 7), (0, 2, 5)]
    assert A.spans_of(torch.from_numpy(d), [(1, 0, 2)]) == [(1, 0, 2)]
    with pytest.raises(ValueError, match="no frame"):
        A.spans_of(d, [(1, 2, 4)])
    for bad in ((2, 0, 1), (0, 3, 3), (0, 4, 6), (0, -1, 2)):
        with pytest.raises(ValueError, match="outside"):
            A.spans_of(d, [bad])


# ----------------------------------------------------------------------------- the entry points

NAMES = ("cmtts_align_workspace_bytes", "cmtts_align_cost", "cmtts_align_dtw", "cmtts_align_durations")


def test_signatures_bound_and_abi_unchanged():
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.cmtts_abi_version() == 8 == _lib.ABI_VERSION
    assert lib.cmtts_set_option(b"align", 1) == -1            # no public option came with it


def test_workspace_bytes():
    lib = _lib.load()
    assert lib.cmtts_align_workspace_bytes(1, 1, 1) > 0
    assert lib.cmtts_align_workspace_bytes(32, 512, 512) >= 32 * 512 * 512          # one byte per cell for the walk back, at the least
    assert lib.cmtts_align_workspace_bytes(1, 4096, 4096) > 0
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 4097, 8), (1, 8, 4097), (1, -3, 8)):
        assert lib.cmtts_align_workspace_bytes(*bad) == 0, bad


def test_entry_points_refuse_before_the_gpu():
    """Every pointer below is either null or host memory the kernels could not read: a call that got as far as the device would not return
    CMTTS_E_INVALID with its message."""
    lib = _lib.load()
    B, Ts, Tr, L = 2, 8, 9, 3
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    xl, yl = np.asarray([8, 5], np.int32), np.asarray([9, 4], np.int32)
    hp = lambda a: a.ctypes.data
    nb = lib.cmtts_align_workspace_bytes(B, Ts, Tr)
    cost = lambda *a: lib.cmtts_align_cost(*a)
    ok = [p, hp(xl), Ts, p, hp(yl), Tr, B, 80, 1, p, p, nb, None]
    for k in (0, 1, 3, 4, 9):
        a = list(ok)
        a[k] = None
        assert cost(*a) == -1 and b"null" in lib.cmtts_last_error(), k
    a = list(ok); a[7] = 64
    assert cost(*a) == -1 and b"n_mels" in lib.cmtts_last_error()
    for bad_x, bad_y in (([9, 5], [9, 4]), ([8, 0], [9, 4]), ([8, 5], [10, 4]), ([8, 5], [9, -1])):
        a = list(ok); bx, by = np.asarray(bad_x, np.int32), np.asarray(bad_y, np.int32); a[1], a[4] = hp(bx), hp(by)
        assert cost(*a) == -1 and b"lengths" in lib.cmtts_last_error(), (bad_x, bad_y)
    for sides in ((0, Ts, Tr), (B, 4097, Tr), (B, Ts, 0)):
        a = list(ok); a[6], a[2], a[5] = sides
        assert cost(*a) == -1 and b"4096" in lib.cmtts_last_error(), sides
    a = list(ok); a[11] = nb - 1
    assert cost(*a) == -4 and b"workspace" in lib.cmtts_last_error()
    a = list(ok); a[10] = None
    assert cost(*a) == -4
    dtw_ok = [p, hp(xl), hp(yl), B, Ts, Tr, p, p, p, p, nb, None]
    for k in (0, 1, 2, 6, 7, 8):
        a = list(dtw_ok)
        a[k] = None
        assert lib.cmtts_align_dtw(*a) == -1 and b"null" in lib.cmtts_last_error(), k
    a = list(dtw_ok); bx = np.asarray([8, 9], np.int32); a[1] = hp(bx)
    assert lib.cmtts_align_dtw(*a) == -1 and b"lengths" in lib.cmtts_last_error()
    a = list(dtw_ok); a[10] = 16
    assert lib.cmtts_align_dtw(*a) == -4
    d = np.asarray([[3, 0, 5], [1, 2, 2]], np.int32)
    dur_ok = [p, p, p, hp(d), hp(xl), hp(yl), B, Ts, Tr, L, p, p, p, nb, None]
    for k in (0, 1, 2, 4, 5, 10, 11):
        a = list(dur_ok)
        a[k] = None
        assert lib.cmtts_align_durations(*a) == -1 and b"null" in lib.cmtts_last_error(), k
    for bad_d in ([[3, 0, 4], [1, 2, 2]], [[3, 0, 5], [1, 2, 3]], [[4, -1, 5], [1, 2, 2]]):
        a = list(dur_ok); bd = np.asarray(bad_d, np.int32); a[3] = hp(bd)
        assert lib.cmtts_align_durations(*a) == -1 and b"sum to x_len" in lib.cmtts_last_error(), bad_d
    a = list(dur_ok); a[9] = 0
    assert lib.cmtts_align_durations(*a) == -1 and b"L" in lib.cmtts_last_error()


def test_host_refuses_before_the_gpu():
    from cmtts_amd import host
    from cmtts_amd.config import get_config
    z = lambda *s: torch.zeros(*s)
    d = torch.tensor([[3, 0, 5], [1, 2, 2]])
    good = dict(mel_syn=z(2, 8, 80), syn_lens=[8, 5], d_syn=d, mel_rec=z(2, 9, 80), rec_lens=[9, 4])
    for change, match in ((dict(mel_syn=z(2, 8, 64)), "80"), (dict(mel_rec=z(3, 9, 80)), "recordings"), (dict(syn_lens=[8, 9]), "syn_lens"),
                          (dict(rec_lens=[9]), "rec_lens"), (dict(rec_lens=[9, 0]), "rec_lens"), (dict(d_syn=d[:, :2]), "sum to syn_lens"),
                          (dict(d_syn=torch.tensor([[3, 0, 5], [1, 3, 2]])), "sum to syn_lens"), (dict(d_syn=d.float() + 0.5), "integers"),
                          (dict(mel_rec=z(2, 4097, 80)), "4096"), (dict(mel_syn=z(8, 80)), "80")):
        with pytest.raises(ValueError, match=match):
            host.dtw_align(**{**good, **change})
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, device="cpu")                # no weights, no device: a call that passed its checks would raise RuntimeError
    texts, src = torch.ones(2, 6, dtype=torch.int64), torch.tensor([6, 4])
    for args, match in (((texts[0], src, z(2, 9, 80), [9, 4]), "texts"), ((texts, src, z(3, 9, 80), [9, 4, 2]), "recordings"),
                        ((texts, src, z(2, 9, 40), [9, 4]), "80"), ((texts, src, z(2, 9, 80), [9, 10]), "rec_lens"),
                        ((texts, torch.tensor([6, 7]), z(2, 9, 80), [9, 4]), "src_lens"), ((texts, src, z(2, 5000, 80), [9, 4]), "4096")):
        with pytest.raises(ValueError, match=match):
            host.align_recording(model, *args)
    with pytest.raises(ValueError, match="n_steps"):
        host.align_recording(model, texts, src, z(2, 9, 80), [9, 4], n_steps=0)
    with pytest.raises(RuntimeError):
        host.align_recording(model, texts, src, z(2, 9, 80), [9, 4])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU"):
            host.dtw_align(**good)
