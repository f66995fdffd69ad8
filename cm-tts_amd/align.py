"""Alignment of a recording to its phonemes by dynamic time warping: the definition in executable form.

numpy only — no torch, no GPU.  Like analysis.py, timing.py and retake.py this file is what the kernels (csrc/align.hip: cmtts_align_cost,
cmtts_align_dtw, cmtts_align_durations) are tested against; it is not a fallback.

The model renders the recording's phonemes in the recording's voice (host.align_recording); the rendering's integer durations say which of
ITS frames belong to which phoneme.  DTW of the rendering's log-mel x [Ts, 80] against the recording's y [Tr, 80] carries those
boundaries over to the recording's frames:

    cost       c[i, j] = sum_k (x[i, k] - y[j, k])^2 in the difference form, each side with its own per-channel mean over its valid frames
               removed first (cepstral-mean style: microphone and level differences drop out).
    dtw        D[0, 0] = c[0, 0], D[i, j] = c[i, j] + min(D[i-1, j-1], D[i-1, j], D[i, j-1]) in float32, both ends fixed, no band, no slope
               constraint.  Ties: diagonal, then (i-1, j), then (i, j-1) — a later candidate wins only if it is strictly smaller.  Every cell
               is ONE rounded add of already rounded values, so D does not depend on the order in which the cells are evaluated and a
               device kernel reproduces it bit for bit.  row[j]: among the path's points in column j the one with the smallest c[i, j],
               ties to the smallest i (the midpoint of the column's run puts a recording frame into the wrong phoneme when the path
               passes a deleted rendering frame at a phoneme boundary; the minimum-cost row does not).
    durations  recording frame j belongs to the phoneme that owns rendering frame row[j]; d_rec[p] counts them (sum d_rec = Tr, a phoneme
               of 0 rendered frames gets 0); phoneme_cost[p] is the float32 sum of c[row[j], j] over the phoneme's frames, j ascending,
               divided by the count (0 for no frames): which phonemes of the recording do not sound like their text.

Limits: a phoneme rendered with 0 frames gets 0 frames; leading or trailing silence the text does not name goes to the first or last
phoneme; no band, no open ends, nothing streamed or sharded."""
import numpy as np

N_MELS = 80
MAX_SIDE = 4096                   # frames per side the device path takes (cmtts_align_workspace_bytes)
DIAG, UP, LEFT = 0, 1, 2          # the step that LED to a cell: from (i-1, j-1), (i-1, j), (i, j-1)


def _side(a, n, normalise, dtype, what):
    a = np.asarray(a)
    n = int(n)
    if a.ndim != 2 or a.shape[1] != N_MELS:
        raise ValueError(f"align.cost: {what} must be [T, {N_MELS}], not {a.shape}")
    if not 1 <= n <= a.shape[0]:
        raise ValueError(f"align.cost: {what}_len = {n} outside [1, {a.shape[0]}]")
    a = a[:n].astype(dtype)
    if normalise:
        a = a - a.mean(axis=0, dtype=dtype)
    return a


def cost(x, x_len, y, y_len, normalise=True, dtype=np.float64):
    """x [>= x_len, 80] (the rendering), y [>= y_len, 80] (the recording), both log-mel -> c [x_len, y_len] in `dtype`.  float64 is the
    definition; float32 — numpy's float32 mean, differences and sums — is the yardstick arm the kernel's bound is derived from."""
    x = _side(x, x_len, normalise, dtype, "x")
    y = _side(y, y_len, normalise, dtype, "y")
    c = np.empty((x.shape[0], y.shape[0]), dtype)
    for i in range(x.shape[0]):             # row by row: [Ts, Tr, 80] at once is 1.3 GB at 4096 x 4096
        d = x[i][None, :] - y
        c[i] = (d * d).sum(axis=1, dtype=dtype)
    return c


def accumulate(c):
    """(D, step) of the recurrence on float32 c [Ts, Tr]: D float32, step uint8 (DIAG / UP / LEFT; DIAG at (0, 0)).  Evaluated by
    anti-diagonals; any other order gives the same bits."""
    c = np.asarray(c)
    if c.dtype != np.float32 or c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
        raise ValueError(f"align.dtw: a float32 cost matrix [Ts, Tr] expected, not {c.dtype} {c.shape}")
    Ts, Tr = c.shape
    D = np.empty((Ts, Tr), np.float32)
    step = np.zeros((Ts, Tr), np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        D[0, 0] = c[0, 0]
        if Tr > 1:
            D[0, 1:] = np.add.accumulate(c[0], dtype=np.float32)[1:]         # sequential float32 adds
            step[0, 1:] = LEFT
        if Ts > 1:
            D[1:, 0] = np.add.accumulate(c[:, 0], dtype=np.float32)[1:]
            step[1:, 0] = UP
        for k in range(2, Ts + Tr - 1):
            i = np.arange(max(1, k - (Tr - 1)), min(Ts - 1, k - 1) + 1)
            j = k - i
            best, s = D[i - 1, j - 1].copy(), np.zeros(len(i), np.uint8)
            for cand, code in ((D[i - 1, j], UP), (D[i, j - 1], LEFT)):
                less = cand < best                                            # strictly smaller; a NaN never wins and never loses its place
                best[less], s[less] = cand[less], code
            D[i, j] = c[i, j] + best
            step[i, j] = s
    return D, step


def dtw(c):
    """float32 c [Ts, Tr] -> (D[Ts-1, Tr-1] as float32, the path's number of points, row int32 [Tr]).  The walk back from (Ts-1, Tr-1) takes
    at most Ts + Tr - 2 steps whatever c holds: on row 0 it goes left, on column 0 up."""
    c = np.asarray(c)
    D, step = accumulate(c)
    Ts, Tr = c.shape
    i, j, n = Ts - 1, Tr - 1, 1
    row = np.zeros(Tr, np.int32)
    row[j], best = i, c[i, j]
    while i > 0 or j > 0:
        s = LEFT if i == 0 else UP if j == 0 else step[i, j]
        if s != LEFT:
            i -= 1
        if s != UP:
            j -= 1
            row[j], best = i, c[i, j]           # a column's first point, met at its largest i
        elif c[i, j] <= best:                   # the same column, a smaller i: it wins a tie
            row[j], best = i, c[i, j]
        n += 1
    return D[Ts - 1, Tr - 1], n, row


def durations(row, c, d_syn):
    """row int [Tr] (non-decreasing, as dtw returns it), float32 c [Ts, Tr], d_syn int [L] with sum Ts -> (d_rec int64 [L], phoneme_cost
    float32 [L])."""
    row, c, d_syn = np.asarray(row), np.asarray(c), np.asarray(d_syn)
    Ts, Tr = c.shape
    if d_syn.ndim != 1 or (d_syn < 0).any() or int(d_syn.sum()) != Ts:
        raise ValueError(f"align.durations: d_syn must be non-negative and sum to the rendering's {Ts} frames, not {int(d_syn.sum())}")
    if row.shape != (Tr,) or (row < 0).any() or (row >= Ts).any() or (np.diff(row) < 0).any():
        raise ValueError("align.durations: row must hold one non-decreasing rendering frame per recording frame")
    if c.dtype != np.float32:
        raise ValueError("align.durations: a float32 cost matrix expected")
    L = len(d_syn)
    owner = np.searchsorted(np.cumsum(d_syn), row, side="right")
    d_rec = np.bincount(owner, minlength=L).astype(np.int64)
    pc = np.zeros(L, np.float32)
    for p in np.nonzero(d_rec)[0]:
        js = np.nonzero(owner == p)[0]
        s = np.float32(0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            for j in js:
                s = np.float32(s + c[row[j], j])
            pc[p] = s / np.float32(len(js))
    return d_rec, pc


def align(x, x_len, y, y_len, d_syn, normalise=True):
    """The whole chain on one pair, through the float32 cost: {"d_rec", "phoneme_cost", "row", "total", "path_len", "cost"} with cost =
    total / path_len."""
    c = cost(x, x_len, y, y_len, normalise).astype(np.float32)
    total, n, row = dtw(c)
    d_rec, pc = durations(row, c, d_syn)
    return {"d_rec": d_rec, "phoneme_cost": pc, "row": row, "total": total, "path_len": n, "cost": np.float32(total / np.float32(n))}


def spans_of(d, phoneme_spans):
    """d int [B, L] (frames per phoneme: d_targets of an alignment), [(b, p_lo, p_hi)] phonemes p_lo .. p_hi - 1 of row b -> [(b, lo, hi)] in
    frames: what retake and retake_recording_pcm take.  An empty frame span (only phonemes of 0 frames) raises ValueError."""
    d = np.asarray(d.cpu() if hasattr(d, "cpu") else d)
    if d.ndim != 2 or (d < 0).any():
        raise ValueError("align.spans_of: d must be [B, L] and non-negative")
    B, L = d.shape
    cum = np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(d.astype(np.int64), axis=1)], axis=1)
    out = []
    for b, p_lo, p_hi in phoneme_spans:
        b, p_lo, p_hi = int(b), int(p_lo), int(p_hi)
        if not 0 <= b < B or not 0 <= p_lo < p_hi <= L:
            raise ValueError(f"align.spans_of: span ({b}, {p_lo}, {p_hi}) outside [{B}, {L}]")
        lo, hi = int(cum[b, p_lo]), int(cum[b, p_hi])
        if lo == hi:
            raise ValueError(f"align.spans_of: phonemes {p_lo} .. {p_hi - 1} of row {b} hold no frame")
        out.append((b, lo, hi))
    return out
