"""Speaker embedding from reference audio (DeepSpeaker: fbank features + ResCNN): the definition (DESIGN.md §3.5h,
csrc/speaker_encoder.hip) in executable form.

Pure numpy, float64 capable.  This is what the HIP kernels are tested against, NOT a fallback: host.speaker_embedding runs
speaker_encoder.hip and nothing here.  It restates the reference's model/speaker_embedder.py -> deepspeaker/embedding.py ->
deepspeaker/audio_ds.py + deepspeaker/conv_models.py; TensorFlow, python_speech_features and the pretrained .h5 are not available,
so the recipes are spelled out here and this file is the definition.

    trim      deepspeaker/audio_ds.py:34-41.  e = |x|; thr = the 95th percentile with linear interpolation, p = 0.95 (n - 1), k = floor(p),
              thr = e_(k) + (p - k)(e_(k+1) - e_(k)) in float64 from the float32 order statistics (e_(k+1) = e_(k) when k = n - 1); keep
              x[first:last], first / last = the first / last index with e > thr — `last` is EXCLUSIVE, as in the reference.  Where no sample
              exceeds thr (silence, constant magnitude) the reference dies with an IndexError; where first == last its fbank dies on the
              empty signal: here both give first = last = -1, frame count 0 and an all-zero embedding (the host raises ValueError).
    fbank     audio_ds.py:17-31,126-137 -> python_speech_features.fbank(signal, fs, nfilt=64, nfft): pre-emphasis 0.97 (first sample kept);
              frame_len = round_half_up(0.025 fs), frame_step = round_half_up(0.01 fs) (551 / 221 at 22 050 Hz); numframes =
              1 + ceil((n - frame_len) / frame_step) if n > frame_len else 1, zero padded to fit; rectangular window; nfft = smallest power
              of two >= win_length; |rfft|^2 / nfft; 64 triangular filters with corners floor((nfft + 1) mel2hz(linspace(hz2mel(0),
              hz2mel(fs / 2), 66)) / fs), hz2mel = 2595 log10(1 + f / 700); zero energies replaced by float64 eps; NO logarithm (fbank, not
              logfbank); then per frame (v - mean) / max(std, 1e-12) over the 64 values, population std (audio_ds.py:136-137).
    windows   deepspeaker/batcher.py:23-29: 160 frames; shorter utterances padded with zero rows AFTER the normalisation.  The reference
              draws the crop offset at random; here it is a parameter: "center" (offset (F - 160) // 2), an integer offset, or "all"
              (hop 80, the last window aligned to the end, the first MAX_WINDOWS of that list).  A row's embedding is the L2-normalised
              mean of its windows' embeddings — with one window too, so every mode runs the same arithmetic.
    ResCNN    deepspeaker/conv_models.py:50-135, channels-last: four stages of Conv2D(k = 5, s = 2, 'same') + BN + clip(0, 20), each followed
              by three identity blocks (conv3-BN-clip, conv3-BN-clip, add, clip); Reshape(-1, 2048): (10, 4, 512) -> index freq * 512 + ch;
              mean over the 10 time rows; Dense(512); x / sqrt(max(sum x^2, 1e-12)).  Keras semantics: convs have a bias; BN epsilon 1e-3
              (inference: moving statistics); TensorFlow's 'same' padding for stride s is total = max((ceil(n / s) - 1) s + k - n, 0) with
              total // 2 before and the rest after (k = 5, s = 2, even n: 1 before, 2 after); kernels are (kh, kw, cin, cout).
"""
import math

import numpy as np

NUM_FBANKS = 64
NUM_FRAMES = 160
EMB_DIM = 512
WINDOW_HOP = 80
MAX_WINDOWS = 64
PREEMPH = 0.97
BN_EPS = 1e-3
CLIP = 20.0
STAGES = (64, 128, 256, 512)


# ---- trim -------------------------------------------------------------------------------------------------------------------------
def trim_threshold(x):
    """float64 threshold of the trim from the float32 samples x[0:n] (n >= 1)."""
    e = np.sort(np.abs(np.asarray(x, np.float32)))
    n = e.size
    p = 0.95 * float(n - 1)
    k = int(math.floor(p))
    ek = float(e[k])
    ek1 = float(e[min(k + 1, n - 1)])
    return ek + (p - k) * (ek1 - ek)


def trim_indices(x):
    """(first, last) with x[first:last] the kept span, or (-1, -1) where the reference cannot go on (see the module text)."""
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return -1, -1
    idx = np.nonzero(np.abs(x).astype(np.float64) > trim_threshold(x))[0]
    if idx.size == 0 or idx[0] == idx[-1]:
        return -1, -1
    return int(idx[0]), int(idx[-1])


# ---- fbank ------------------------------------------------------------------------------------------------------------------------
def round_half_up(v):
    return int(math.floor(v + 0.5))


def frame_geometry(fs, win_length):
    """(frame_len, frame_step, nfft)."""
    nfft = 1
    while nfft < win_length:
        nfft *= 2
    return round_half_up(0.025 * fs), round_half_up(0.01 * fs), nfft


def num_frames(n, frame_len, frame_step):
    if n <= 0:
        return 0
    return 1 + int(math.ceil((n - frame_len) / float(frame_step))) if n > frame_len else 1


def hz2mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def mel2hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def filter_bins(fs, nfft, nfilt=NUM_FBANKS):
    """The nfilt + 2 corner bins of the triangular filters (int64)."""
    mel = np.linspace(hz2mel(0.0), hz2mel(fs / 2.0), nfilt + 2)
    return np.floor((nfft + 1) * mel2hz(mel) / fs).astype(np.int64)


def filterbank(fs, nfft, nfilt=NUM_FBANKS):
    """[nfilt, nfft // 2 + 1] float64: row j rises over [bin[j], bin[j+1]) and falls over [bin[j+1], bin[j+2])."""
    b = filter_bins(fs, nfft, nfilt)
    fb = np.zeros((nfilt, nfft // 2 + 1), np.float64)
    for j in range(nfilt):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / float(b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / float(b[j + 2] - b[j + 1])
    return fb


def fbank_features(sig, fs=22050, win_length=1024, dtype=np.float64):
    """Normalised filterbank energies [F, 64] of the (already trimmed) signal, every step in `dtype`."""
    sig = np.asarray(sig, np.float32).astype(dtype)
    frame_len, frame_step, nfft = frame_geometry(fs, win_length)
    F = num_frames(sig.size, frame_len, frame_step)
    if F == 0:
        return np.zeros((0, NUM_FBANKS), dtype)
    pre = np.empty_like(sig)
    pre[0] = sig[0]
    pre[1:] = sig[1:] - dtype(PREEMPH) * sig[:-1]
    padded = np.zeros((F - 1) * frame_step + frame_len, dtype)
    padded[:sig.size] = pre
    idx = np.arange(frame_len)[None, :] + frame_step * np.arange(F)[:, None]
    frames = padded[idx]
    if dtype == np.float32:
        spec = np.fft.rfft(frames.astype(np.float32), nfft).astype(np.complex64)
    else:
        spec = np.fft.rfft(frames, nfft)
    pspec = ((spec.real.astype(dtype) ** 2 + spec.imag.astype(dtype) ** 2) / dtype(nfft)).astype(dtype)
    feat = pspec @ filterbank(fs, nfft).astype(dtype).T
    feat = np.where(feat == 0, dtype(np.finfo(np.float64).eps), feat).astype(dtype)
    mean = feat.mean(axis=1, keepdims=True, dtype=dtype)
    std = np.sqrt(((feat - mean) ** 2).mean(axis=1, keepdims=True, dtype=dtype))
    return ((feat - mean) / np.maximum(std, dtype(1e-12))).astype(dtype)


# ---- windows ----------------------------------------------------------------------------------------------------------------------
def window_offsets(F, windows="center"):
    """Frame offsets of the 160-frame windows of an utterance of F frames ([] when F == 0)."""
    if F <= 0:
        return []
    if isinstance(windows, str):
        if windows == "center":
            return [max(F - NUM_FRAMES, 0) // 2]
        if windows == "all":
            if F <= NUM_FRAMES:
                return [0]
            return (list(range(0, F - NUM_FRAMES, WINDOW_HOP)) + [F - NUM_FRAMES])[:MAX_WINDOWS]
        raise ValueError(f"windows = {windows!r}: expected 'center', 'all' or an integer offset")
    off = int(windows)
    if off < 0 or off > max(F - NUM_FRAMES, 0):
        raise ValueError(f"window offset {off} outside [0, {max(F - NUM_FRAMES, 0)}]")
    return [off]


def cut_window(feat, off):
    """[160, 64]: frames off .. off + 159 of feat, zero rows behind its end."""
    w = np.zeros((NUM_FRAMES, NUM_FBANKS), feat.dtype)
    part = feat[off:off + NUM_FRAMES]
    w[:part.shape[0]] = part
    return w


# ---- ResCNN -----------------------------------------------------------------------------------------------------------------------
def same_pad(n, k, s):
    """(before, after, out) of TensorFlow's 'same' padding."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2, out


def conv2d_same(x, kernel, bias, stride):
    """x [B, H, W, Cin], kernel (kh, kw, cin, cout), bias [cout] -> [B, ceil(H / s), ceil(W / s), cout], in x's dtype."""
    kh, kw, cin, cout = kernel.shape
    B, H, W, _ = x.shape
    pt, pb, Ho = same_pad(H, kh, stride)
    pl, pr, Wo = same_pad(W, kw, stride)
    xp = np.zeros((B, H + pt + pb, W + pl + pr, cin), x.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    y = np.zeros((B, Ho, Wo, cout), x.dtype)
    k = kernel.astype(x.dtype)
    for i in range(kh):
        for j in range(kw):
            y += xp[:, i:i + (Ho - 1) * stride + 1:stride, j:j + (Wo - 1) * stride + 1:stride] @ k[i, j]
    return y + bias.astype(x.dtype)


def clip(x):
    return np.minimum(np.maximum(x, 0), x.dtype.type(CLIP))


def _get(sd, name):
    v = sd[name] if name in sd else sd[name + ":0"]
    return np.asarray(v)


def layer_names():
    """Conv layers of the ResCNN in execution order: (name, kernel size, stride, cin, cout)."""
    out, cin = [], 1
    for s, c in enumerate(STAGES, start=1):
        out.append((f"conv{c}-s", 5, 2, cin, c))
        for b in range(3):
            out.append((f"res{s}_{b}_branch_2a", 3, 1, c, c))
            out.append((f"res{s}_{b}_branch_2b", 3, 1, c, c))
        cin = c
    return out


def conv_bn(sd, name, x, stride):
    dt = x.dtype
    y = conv2d_same(x, _get(sd, name + "/kernel"), _get(sd, name + "/bias"), stride)
    g, b = _get(sd, name + "_bn/gamma").astype(dt), _get(sd, name + "_bn/beta").astype(dt)
    m, v = _get(sd, name + "_bn/moving_mean").astype(dt), _get(sd, name + "_bn/moving_variance").astype(dt)
    return g * (y - m) / np.sqrt(v + dt.type(BN_EPS)) + b


def fold_bn(sd, name):
    """(kernel, bias) in float64 of conv `name` with its BatchNorm folded in: what the importer rounds to float32."""
    k, b = _get(sd, name + "/kernel").astype(np.float64), _get(sd, name + "/bias").astype(np.float64)
    s = _get(sd, name + "_bn/gamma").astype(np.float64) / np.sqrt(_get(sd, name + "_bn/moving_variance").astype(np.float64) + BN_EPS)
    return k * s, (b - _get(sd, name + "_bn/moving_mean").astype(np.float64)) * s + _get(sd, name + "_bn/beta").astype(np.float64)


def rescnn_features(sd, x, taps=None):
    """x [B, 160, 64, 1] -> [B, 10, 4, 512].  taps: an optional list that receives every stage's output."""
    for s, c in enumerate(STAGES, start=1):
        x = clip(conv_bn(sd, f"conv{c}-s", x, 2))
        for b in range(3):
            t = clip(conv_bn(sd, f"res{s}_{b}_branch_2a", x, 1))
            t = clip(conv_bn(sd, f"res{s}_{b}_branch_2b", t, 1))
            x = clip(t + x)
        if taps is not None:
            taps.append(x)
    return x


def l2_normalize(x):
    return x / np.sqrt(np.maximum((x * x).sum(axis=-1, keepdims=True), x.dtype.type(1e-12)))


def rescnn(sd, windows, dtype=np.float64):
    """windows [W, 160, 64] -> unit-norm embeddings [W, 512]."""
    x = np.asarray(windows).astype(dtype)[..., None]
    f = rescnn_features(sd, x)
    v = f.reshape(f.shape[0], f.shape[1], -1).mean(axis=1, dtype=dtype)          # Reshape(-1, 2048), mean over time
    y = v @ _get(sd, "affine/kernel").astype(dtype) + _get(sd, "affine/bias").astype(dtype)
    return l2_normalize(y)


# ---- the whole path ----------------------------------------------------------------------------------------------------------------
def utterance_windows(wav, fs=22050, win_length=1024, windows="center", dtype=np.float64):
    """((first, last, frames, n_windows), [n_windows, 160, 64]) of one utterance."""
    first, last = trim_indices(wav)
    if first < 0:
        return (-1, -1, 0, 0), np.zeros((0, NUM_FRAMES, NUM_FBANKS), dtype)
    feat = fbank_features(np.asarray(wav, np.float32)[first:last], fs, win_length, dtype)
    offs = window_offsets(feat.shape[0], windows)
    return (first, last, feat.shape[0], len(offs)), np.stack([cut_window(feat, o) for o in offs])


def speaker_embedding(sd, wavs, lengths=None, fs=22050, win_length=1024, windows="center", dtype=np.float64):
    """[B, 512]: per row the L2-normalised mean of its windows' embeddings; all zeros for a row with frame count 0.
    windows: "center", "all", one integer offset or one per row."""
    B = len(wavs)
    out = np.zeros((B, EMB_DIM), dtype)
    for b in range(B):
        w = np.asarray(wavs[b], np.float32)
        if lengths is not None:
            w = w[:int(lengths[b])]
        mode = windows if isinstance(windows, (str, int)) else windows[b]
        info, win = utterance_windows(w, fs, win_length, mode, dtype)
        if info[3]:
            out[b] = l2_normalize(rescnn(sd, win, dtype).mean(axis=0, dtype=dtype)[None])[0]
    return out
