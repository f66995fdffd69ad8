"""Speaker embedding from reference audio, the GE2E way (40-channel power mel + 3-layer LSTM): the definition (DESIGN.md §3.5l,
csrc/ge2e.hip) in executable form.

Pure numpy, float64 by default with a `dtype=` switch.  This is what the HIP kernels are tested against, NOT a fallback:
host.ge2e_embedding runs ge2e.hip and nothing here.  It restates the reference's speakerembedder/speaker_embedder.py (embedder "GE2E") ->
ge2e_encoder/inference.py: embed_utterance -> ge2e_encoder/audio.py: wav_to_mel_spectrogram + ge2e_encoder/model.py: SpeakerEncoder.forward.
The reference hands embed_utterance the RAW 22 050 Hz waveform: preprocess_wav (volume normalisation to -30 dBFS, the webrtcvad silence
trim) is NOT applied on this path, and is not built here.

    slices    inference.py: compute_partial_slices.  220 samples per frame (int(22050 * 10 / 1000)), n_frames = ceil((n + 1) / 220), partials
              of 160 frames every 80 frames, i = 0, 80, ... < max(1, n_frames - 160 + 80 + 1); the last one is dropped when
              (n - start) / 35200 < 0.75 and it is not the only one.  embed_utterance zero-pads the waveform to the last slice's stop when
              that stop >= n.
    mel       audio.py: librosa.feature.melspectrogram(y, sr=22050, n_fft=551, hop_length=220, n_mels=40) with the defaults of the
              reference's era, written out: centred frames, REFLECT padding of 275 samples per side (numpy.pad: repeated reflection for a
              signal shorter than the pad), periodic Hann of 551, |rfft|^2 (276 bins), Slaney mel scale with Slaney-normalised triangles
              between 0 and 11 025 Hz sampled on linspace(0, fs / 2, 276), NO logarithm.  1 + (n - 1) // 220 frames (n_fft is odd).
              librosa is not available where this project is developed: this is the public recipe restated, not librosa bit for bit.
    float32   the dtype=float32 arm — the yardstick of the kernel's error — forms the spectrum the way the kernel does, as the contraction of
              the frames with the windowed cos / sin table (made in double, angle reduced as k n mod 551, rounded once), every operation in
              float32; the float64 arm uses numpy's rfft.
    LSTM      model.py: SpeakerEncoder.forward.  torch.nn.LSTM(40, 256, 3, batch_first=True): gates in the order i, f, g, o, both biases,
              zero initial state; c = sigmoid(f) c + sigmoid(i) tanh(g), h = sigmoid(o) tanh(c); hidden[-1] -> Linear(256, 256) -> ReLU ->
              x / (||x||_2 + 1e-5).  `lengths` freezes a window's state after its last frame.
    utterance the mean of the partials' embeddings divided by its L2 norm (no epsilon, as the reference); using_partials=False: the whole
              spectrogram as one window, its embedding as it is.
"""
import functools

import numpy as np

from . import analysis as _an

SAMPLE_RATE = 22050
N_FFT = 551                         # int(22050 * 25 / 1000)
HOP = 220                           # int(22050 * 10 / 1000)
N_MELS = 40
N_BINS = N_FFT // 2 + 1             # 276
PAD = N_FFT // 2                    # 275
PARTIAL_FRAMES = 160
HIDDEN = 256
EMB_DIM = 256
LAYERS = 3


# ---- slices -------------------------------------------------------------------------------------------------------------------------
def partial_slices(n_samples, partial_frames=PARTIAL_FRAMES, min_pad_coverage=0.75, overlap=0.5):
    """(wave slices, mel slices) as lists of (start, stop): inference.py: compute_partial_slices."""
    if not (0 <= overlap < 1) or not (0 < min_pad_coverage <= 1):
        raise ValueError("partial_slices: 0 <= overlap < 1 and 0 < min_pad_coverage <= 1")
    n_samples = int(n_samples)
    n_frames = -(-(n_samples + 1) // HOP)
    step = max(int(np.round(partial_frames * (1 - overlap))), 1)
    starts = list(range(0, max(1, n_frames - partial_frames + step + 1), step))
    last = starts[-1] * HOP
    coverage = (n_samples - last) / float(partial_frames * HOP)
    if coverage < min_pad_coverage and len(starts) > 1:
        starts = starts[:-1]
    mel = [(i, i + partial_frames) for i in starts]
    return [(a * HOP, b * HOP) for a, b in mel], mel


def padded_length(n_samples, **kw):
    """Length of the waveform embed_utterance computes the spectrogram of: zero-padded to the last slice's stop when that stop >= n."""
    stop = partial_slices(n_samples, **kw)[0][-1][1]
    return max(int(n_samples), stop)


# ---- mel ----------------------------------------------------------------------------------------------------------------------------
def frame_count(n):
    return 0 if n <= 0 else 1 + (int(n) - 1) // HOP


@functools.lru_cache(maxsize=None)
def mel_basis():
    """[40, 276] float32: analysis.mel_basis (the Slaney filterbank, also csrc/mel_basis.cpp) at the odd transform length."""
    return _an.mel_basis(SAMPLE_RATE, N_FFT, N_MELS, 0.0, SAMPLE_RATE / 2.0)


def hann_window(dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


@functools.lru_cache(maxsize=None)
def dft_table():
    """(cos, sin) [276, 551] float64 with the window folded in: w[n] cos(2 pi (k n mod 551) / 551), likewise sin."""
    kn = (np.arange(N_BINS, dtype=np.int64)[:, None] * np.arange(N_FFT, dtype=np.int64)[None, :]) % N_FFT
    ang = 2.0 * np.pi * kn.astype(np.float64) / N_FFT
    w = hann_window()
    return np.cos(ang) * w, np.sin(ang) * w


def frames_of(wav):
    """[F, 551] reflect-padded centred frames of a float waveform (no window), in its dtype."""
    x = np.asarray(wav).reshape(-1)
    F = frame_count(x.size)
    if F == 0:
        return np.zeros((0, N_FFT), x.dtype)
    xp = np.pad(x, PAD, mode="reflect") if x.size > 1 else np.full(x.size + 2 * PAD, x[0], x.dtype)
    return xp[HOP * np.arange(F)[:, None] + np.arange(N_FFT)[None, :]]


def power_spectrum(wav, dtype=np.float64):
    """[F, 276] |STFT|^2 of one row in `dtype` (see the module text for the float32 arm)."""
    fr = frames_of(np.asarray(wav, np.float32).astype(dtype))
    if dtype == np.float32:
        c, s = (t.astype(np.float32) for t in dft_table())
        re, im = fr @ c.T, fr @ s.T
    else:
        spec = np.fft.rfft(fr * hann_window(dtype), axis=1)
        re, im = spec.real, spec.imag
    return (re * re + im * im).astype(dtype)


def mel_power(wav, dtype=np.float64):
    """[F, 40] power mel spectrogram of one row, no logarithm: audio.py: wav_to_mel_spectrogram (the public recipe restated, not librosa bit
    for bit)."""
    return (power_spectrum(wav, dtype) @ mel_basis().astype(dtype).T).astype(dtype)


# ---- LSTM ---------------------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_layer(w_ih, w_hh, b_ih, b_hh, x, lengths=None):
    """One layer: x [N, T, K] -> (outputs [N, T, 256], h [N, 256]) in x's dtype.  Beyond a window's length its state stays as it is (and
    the outputs repeat it); what x holds there is not read."""
    dt = x.dtype
    N, T, _ = x.shape
    H = w_hh.shape[1]
    w_ih, w_hh, b = w_ih.astype(dt), w_hh.astype(dt), (b_ih.astype(dt) + b_hh.astype(dt))
    lens = np.full(N, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    h, c = np.zeros((N, H), dt), np.zeros((N, H), dt)
    out = np.zeros((N, T, H), dt)
    for t in range(T):
        live = lens > t
        xt = np.where(live[:, None], x[:, t], 0).astype(dt)
        g = (xt @ w_ih.T + b) + h @ w_hh.T
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c_new = f * c + i * gg
        h_new = o * np.tanh(c_new)
        c = np.where(live[:, None], c_new, c).astype(dt)
        h = np.where(live[:, None], h_new, h).astype(dt)
        out[:, t] = h
    return out, h


def lstm(sd, x, lengths=None, dtype=np.float64):
    """hidden[-1] [N, 256] of the three layers on x [N, T, 40]."""
    x = np.asarray(x).astype(dtype)
    h = None
    for l in range(LAYERS):
        x, h = lstm_layer(*(np.asarray(sd[f"lstm.{p}_l{l}"]) for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")), x, lengths)
    return h


def project(sd, h):
    """relu(linear(h)) / (||.||_2 + 1e-5) per row."""
    dt = h.dtype
    y = np.maximum(h @ np.asarray(sd["linear.weight"]).astype(dt).T + np.asarray(sd["linear.bias"]).astype(dt), 0)
    return (y / (np.sqrt((y * y).sum(axis=1, keepdims=True, dtype=dt)) + dt.type(1e-5))).astype(dt)


def embed_frames(sd, frames, lengths=None, dtype=np.float64):
    """model.py: SpeakerEncoder.forward — frames [N, T, 40] -> [N, 256]."""
    return project(sd, lstm(sd, frames, lengths, dtype))


def utterance_windows(wav, using_partials=True, dtype=np.float64):
    """([W, T, 40] windows, padded length) of one utterance: its partials (T = 160), or the whole spectrogram as one window."""
    wav = np.asarray(wav, np.float32).reshape(-1)
    if not using_partials:
        return mel_power(wav, dtype)[None], wav.size
    _, mel_slices = partial_slices(wav.size)
    n_eff = padded_length(wav.size)
    frames = mel_power(np.concatenate([wav, np.zeros(n_eff - wav.size, np.float32)]), dtype)
    return np.stack([frames[a:b] for a, b in mel_slices]), n_eff


def embed_utterance(sd, wav, using_partials=True, dtype=np.float64):
    """inference.py: embed_utterance — [256]."""
    win, _ = utterance_windows(wav, using_partials, dtype)
    e = embed_frames(sd, win, None, dtype)
    if not using_partials:
        return e[0]
    raw = e.mean(axis=0, dtype=dtype)
    return (raw / np.sqrt((raw * raw).sum(dtype=dtype))).astype(dtype)


# ---- the packed weight stream (csrc/weight_pack.cpp: to_lstm_fragments) -----------------------------------------------------------------
def packed_row(q):
    """The PyTorch gate row (gate * 256 + unit) that packed row q holds: q = 64 (unit // 16) + 16 gate + unit % 16, so the four 16-row MFMA
    tiles 4 g .. 4 g + 3 are i, f, g, o of hidden units 16 g .. 16 g + 15."""
    q = np.asarray(q)
    return ((q % 64) // 16) * HIDDEN + 16 * (q // 64) + q % 16


def unpack_lstm_fragments(stream, K):
    """The [1024, K] matrix (PyTorch row order) a fragment stream [ceil(K / 16)][64 row tiles][64 lanes][4] holds."""
    nc = -(-K // 16)
    s = np.asarray(stream, np.float32).reshape(nc, 64, 64, 4)
    w = np.zeros((4 * HIDDEN, nc * 16), np.float32)
    for lane in range(64):
        rows = packed_row(16 * np.arange(64) + (lane & 15))
        for j in range(4):
            w[rows[None, :], (16 * np.arange(nc) + 4 * (lane >> 4) + j)[:, None]] = s[:, :, lane, j]
    assert not w[:, K:].any()
    return w[:, :K]
