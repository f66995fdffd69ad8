"""Duration targets and phoneme marks: the definition (csrc/duration_fit.hip) in executable form.

Pure numpy.  This is what the HIP kernels are tested against, NOT a fallback: DurationPitchSpeakerNet.forward(target_frames=...,
segments=...) runs duration_fit_kernel behind the durations kernel and host.phoneme_marks runs phoneme_marks_kernel; nothing here
runs on that path.

    fit        the integer durations n[0..k) of one segment (after the duration control and int() truncation, S = sum n) are
               apportioned to a target of t frames by largest remainder:
                   q = n t,  a = q // S,  r = q % S,  R = t - sum a
               and the R entries with the largest r take one more frame, ties to the lower index.  Exact 64-bit integer arithmetic.
               sum(result) = t;  n[l] = 0 stays 0 (R never exceeds the count of non-zero remainders);  |result[l] - n[l] t / S| < 1;
               t = S returns n.  t < 0 ("leave alone") or S = 0 returns n.
    segments   seg[l] in [-1, G) names the segment of phoneme l (-1: in none, left alone), targets[g] the frame count of segment g
               (-1: left alone); each segment is fitted on its own, phonemes in index order.  A segment with S = 0 and a target > 0
               cannot be met and is counted.
    marks      phoneme l occupies the frames [cum[l - 1], cum[l]) of the cumulative sum of max(int(d), 0), clipped to T when T > 0,
               and the samples [out_len(start hop), out_len(end hop)) at the output rate up / down (resample.out_len: the mapping of
               vocoder_infer_stream's chunk offsets, so a mark and a chunk offset are on one scale).
"""
import numpy as np

from . import resample

MAX_TARGET = 1 << 24          # include/cmtts_hip.h: a fitted duration is returned as fp32, which holds integers up to 2^24 exactly


def fit_durations(n, target):
    """The durations n (non-negative integers) of ONE segment fitted to `target` frames -> int64 array of n's shape.
    target < 0 or sum(n) == 0: n itself (as int64)."""
    n = np.asarray(n, dtype=np.int64)
    if n.ndim != 1 or (n < 0).any():
        raise ValueError("fit_durations: n must be a vector of non-negative integers")
    t = int(target)
    S = int(n.sum())
    if t < 0 or S == 0:
        return n.copy()
    q = n * np.int64(t)
    a = q // S
    r = q % S
    R = t - int(a.sum())
    order = np.lexsort((np.arange(len(n)), -r))          # largest remainder first, ties to the lower index
    out = a.copy()
    out[order[:R]] += 1
    return out


def fit_segments(n, seg, targets):
    """One utterance: durations n [L], seg int [L] in [-1, G) or None (the utterance-level form: one segment holding every
    phoneme, G = 1), targets int [G] (-1 = leave alone).  Returns (fitted int64 [L], the number of segments that could not be
    met: S == 0 and target > 0)."""
    n = np.asarray(n, dtype=np.int64)
    targets = np.atleast_1d(np.asarray(targets, dtype=np.int64))
    G = len(targets)
    if seg is None:
        if G != 1:
            raise ValueError("fit_segments: the utterance-level form takes one target")
        seg = np.zeros(len(n), np.int64)
    seg = np.asarray(seg, dtype=np.int64)
    if seg.shape != n.shape or (seg < -1).any() or (seg >= G).any():
        raise ValueError(f"fit_segments: seg must be [{len(n)}] with values in [-1, {G})")
    out = n.copy()
    unmet = 0
    for g in range(G):
        idx = np.flatnonzero(seg == g)
        t = int(targets[g])
        if t < 0:
            continue
        if int(n[idx].sum()) == 0:
            unmet += t > 0
            continue
        out[idx] = fit_durations(n[idx], t)
    return out, int(unmet)


def phoneme_marks(d, src_len, T=0, hop=resample.HOP, up=1, down=1):
    """d [L] durations (fp32 as d_rounded, or integers) of one utterance with src_len phonemes -> int32 [L, 4]: start frame, end
    frame, start sample, end sample of every phoneme.  T > 0 clips the frames to T (a mel cut at a bucket).  Rows l >= src_len repeat
    the utterance's end."""
    d = np.asarray(d)
    L, src_len = len(d), int(src_len)
    n = np.maximum(d.astype(np.int64), 0)
    n[src_len:] = 0
    end = np.cumsum(n)
    if T > 0:
        end = np.minimum(end, int(T))
    start = np.concatenate([[0], end[:-1]])
    marks = np.empty((L, 4), np.int32)
    for l in range(L):
        marks[l] = (start[l], end[l], resample.out_len(int(start[l]) * hop, up, down), resample.out_len(int(end[l]) * hop, up, down))
    return marks


def frames_for_seconds(sec, sampling_rate=resample.NATIVE_RATE, hop=resample.HOP):
    """The frame count closest to `sec` seconds, at least 1: max(1, round(sec * sampling_rate / hop)).  A frame is the model's unit
    (hop / sampling_rate seconds, 11.6 ms at 22050 Hz and hop 256), so the achieved length target * hop / sampling_rate is within
    HALF A FRAME of the request (5.8 ms), not sample exact."""
    if not sec > 0:
        raise ValueError(f"frames_for_seconds: {sec!r} seconds")
    return max(1, int(round(float(sec) * float(sampling_rate) / float(hop))))
