"""Recorded speech in: the log-mel / energy analysis of a waveform, phoneme-level energy targets and the crossfade that joins a vocoded span
back into a recording — the DEFINITION the kernels of csrc/mel_analysis.hip are tested against (numpy, float64 by default; dtype=np.float32
runs the same steps in float32 as a yardstick for the kernels' rounding).  Not a fallback: host.py never calls it.

What it restates (preprocessor/preprocessor.py:291-305, 180-189, 426-437 of the reference):

    mel, energy   Audio.tools.get_mel_from_wav(wav, STFT): the public TacotronSTFT recipe at filter_length = win_length = 1024, hop 256,
                  80 Slaney mel channels over 0-8000 Hz at 22050 Hz — reflect padding, periodic Hann window, 1024-point real DFT, magnitude
                  sqrt(re^2 + im^2) over 513 bins, energy = sqrt(sum mag^2) per frame, mel = log(max(basis @ mag, 1e-5)).  The reference's `audio`
                  package is not part of its tree, so the recipe is restated here and pinned against torch.stft (tests/test_analysis_cpu.py).
    framing       pad="reference": 512 reflected samples on both sides, 1 + n // 256 frames (n > 512) — what the acoustic model's mels were
                  made with.  pad="vocoder": 384 reflected samples on both sides and no centring, n // 256 frames (n > 384): frame f covers
                  samples [256 f, 256 (f + 1)), the cell the generator emits for it (HiFi-GAN's mel_spectrogram framing).  The magnitude has
                  the same form in both modes: HiFi-GAN's + 1e-9 under the root is NOT reproduced.
    phoneme_energy  the phoneme-level average (296-305) and the normalisation (normalize: (e - mean) / std, zeros included).
    crossfade_splice  no reference counterpart: the join of a vocoded span into a recording (host.retake_recording_pcm).

Input: float audio in [-1, 1] (clipped to that range) or int16 taken as x / 32768, at 22050 Hz; no resampling.  Any other STFT geometry is
refused (check_geometry).  Beyond a row's frame count mel and energy are zero (the reference's pad_2D / pad_1D)."""
import numpy as np

SAMPLE_RATE = 22050
N_FFT = 1024
HOP = 256
N_BINS = N_FFT // 2 + 1
N_MELS = 80
FMIN = 0.0
FMAX = 8000.0
MEL_FLOOR = 1e-5
PAD = {"reference": N_FFT // 2, "vocoder": (N_FFT - HOP) // 2}          # reflected samples on either side


def check_geometry(filter_length=N_FFT, hop_length=HOP, win_length=N_FFT, n_mels=N_MELS):
    """The one STFT instance every reference config uses; anything else raises ValueError."""
    if (int(filter_length), int(hop_length), int(win_length), int(n_mels)) != (N_FFT, HOP, N_FFT, N_MELS):
        raise ValueError(f"analysis: filter_length / hop_length / win_length / n_mel_channels = {filter_length} / {hop_length} / {win_length} / "
                         f"{n_mels} is not supported (only {N_FFT} / {HOP} / {N_FFT} / {N_MELS})")


def _pad_of(pad):
    if pad not in PAD:
        raise ValueError(f"pad = {pad!r}: expected 'reference' or 'vocoder'")
    return PAD[pad]


def min_samples(pad="reference"):
    """A row needs MORE than this many samples (one reflection must reach)."""
    return _pad_of(pad)


def frame_count(n, pad="reference"):
    """Frames of an n-sample row; 0 for a row at or below the minimum length."""
    if n <= _pad_of(pad):
        return 0
    return 1 + n // HOP if pad == "reference" else n // HOP


# ---- the Slaney filterbank ---------------------------------------------------------------------------------------------------------------
_F_SP = 200.0 / 3.0
_BREAK_HZ = 1000.0
_BREAK_MEL = _BREAK_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= _BREAK_HZ, _BREAK_MEL + np.log(np.maximum(f, _BREAK_HZ) / _BREAK_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= _BREAK_MEL, _BREAK_HZ * np.exp(_LOGSTEP * (m - _BREAK_MEL)), _F_SP * m)


def mel_corners(n_mels=N_MELS, fmin=FMIN, fmax=FMAX):
    """The n_mels + 2 corner frequencies in Hz: equally spaced in mel between fmin and fmax."""
    return mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))


def mel_basis(fs=SAMPLE_RATE, n_fft=N_FFT, n_mels=N_MELS, fmin=FMIN, fmax=FMAX):
    """[n_mels, n_fft // 2 + 1] float32: triangles on linspace(0, fs / 2, bins), filter i rising over [f[i], f[i+1]] and falling over
    [f[i+1], f[i+2]], scaled by 2 / (f[i+2] - f[i]); computed in float64, stored as float32 (cmtts_mel_basis computes the same)."""
    f = mel_corners(n_mels, fmin, fmax)
    bins = np.linspace(0.0, fs / 2.0, n_fft // 2 + 1)
    fdiff = np.diff(f)
    ramps = f[:, None] - bins[None, :]
    w = np.zeros((n_mels, bins.size), np.float64)
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (f[2:] - f[:-2]))[:, None]
    return w.astype(np.float32)


def hann_window(dtype=np.float64):
    """Periodic Hann over 1024 samples, computed in double; the float32 arm (and the kernel) use it rounded to float32."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


# ---- mel and energy ------------------------------------------------------------------------------------------------------------------------
def to_float(wav, dtype=np.float64):
    """int16 -> x / 32768; float -> float32 clipped to [-1, 1]; then `dtype`."""
    wav = np.asarray(wav)
    if wav.dtype == np.int16:
        return wav.astype(dtype) / dtype(32768.0)
    if wav.dtype.kind != "f":
        raise ValueError(f"analysis: float or int16 audio expected, not {wav.dtype}")
    return np.clip(wav.astype(np.float32), -1.0, 1.0).astype(dtype)


def stft_magnitude(wav, pad="reference", dtype=np.float64):
    """|STFT| [frames, 513] of one row, every step in `dtype`."""
    P = _pad_of(pad)
    x = to_float(np.asarray(wav).reshape(-1), dtype)
    F = frame_count(x.size, pad)
    if F == 0:
        raise ValueError(f"analysis: a row of {x.size} samples is too short for pad={pad!r} (more than {P} needed)")
    xp = np.pad(x, P, mode="reflect")
    frames = xp[HOP * np.arange(F)[:, None] + np.arange(N_FFT)[None, :]] * hann_window(dtype)
    spec = np.fft.rfft(frames.astype(dtype), axis=1)
    re, im = spec.real.astype(dtype), spec.imag.astype(dtype)
    return np.sqrt(re * re + im * im).astype(dtype)


def mel_from_wav(wav, pad="reference", dtype=np.float64, basis=None):
    """One row -> (mel [frames, 80], energy [frames]) in `dtype`."""
    mag = stft_magnitude(wav, pad, dtype)
    basis = (mel_basis() if basis is None else np.asarray(basis, np.float32)).astype(dtype)
    energy = np.sqrt((mag * mag).sum(axis=1, dtype=dtype))
    mel = np.log(np.maximum(mag @ basis.T, dtype(MEL_FLOOR)))
    return mel.astype(dtype), energy.astype(dtype)


def mel_from_audio(wavs, lengths=None, pad="reference", layout="tc", T=None, dtype=np.float64, basis=None):
    """A batch: wavs [B, n] (or a list of rows), lengths per row -> {"mel": [B, T, 80] ("tc") or [B, 80, T] ("ct"), "mel_lens": int [B],
    "energy": [B, T]}; T defaults to the longest row's frame count; zeros beyond a row's frames."""
    if layout not in ("tc", "ct"):
        raise ValueError(f"layout = {layout!r}: expected 'tc' or 'ct'")
    rows = [np.asarray(w).reshape(-1) for w in wavs]
    lens = [r.size for r in rows] if lengths is None else [int(v) for v in lengths]
    if len(lens) != len(rows) or any(n > r.size for n, r in zip(lens, rows)):
        raise ValueError("analysis: one length per row, none beyond the row")
    out = [mel_from_wav(r[:n], pad, dtype, basis) for r, n in zip(rows, lens)]
    F = [m.shape[0] for m, _ in out]
    T = max(F) if T is None else int(T)
    mel = np.zeros((len(rows), T, N_MELS), dtype)
    energy = np.zeros((len(rows), T), dtype)
    for b, (m, e) in enumerate(out):
        k = min(F[b], T)
        mel[b, :k], energy[b, :k] = m[:k], e[:k]
    return {"mel": mel if layout == "tc" else np.ascontiguousarray(mel.transpose(0, 2, 1)), "mel_lens": np.minimum(F, T).astype(np.int64),
            "energy": energy}


# ---- phoneme-level energy --------------------------------------------------------------------------------------------------------------------
def phoneme_energy(energy, durations, mean, std, dtype=np.float64):
    """energy [B, T] (frames), durations int [B, L] -> [B, L]: entry l is the mean of that phoneme's d frames (frames sum(d[:l]) ... + d), 0
    when d == 0; then every entry, the zeros included, becomes (e - mean) / std with stats.json's "energy"[2:4].  Frames at or beyond T count
    as zero.  The reference's loop (preprocessor.py:296-305) writes its means into the array it reads from; it equals this wherever it has not
    yet overwritten a frame it goes on to read, i.e. while sum(d[:l]) >= l — any alignment whose phonemes average a frame or more."""
    e = np.asarray(energy).astype(dtype)
    d = np.asarray(durations).astype(np.int64)
    if e.ndim != 2 or d.ndim != 2 or e.shape[0] != d.shape[0]:
        raise ValueError(f"phoneme_energy: energy {e.shape} and durations {d.shape} do not fit [B, T] / [B, L]")
    if (d < 0).any():
        raise ValueError("phoneme_energy: negative duration")
    B, T = e.shape
    out = np.zeros(d.shape, dtype)
    for b in range(B):
        pos = 0
        for l, n in enumerate(d[b]):
            if n > 0:
                seg = e[b, min(pos, T):min(pos + n, T)]
                out[b, l] = seg.sum(dtype=dtype) / dtype(n)
            pos += int(n)
    return ((out - dtype(mean)) / dtype(std)).astype(dtype)


# ---- joining a vocoded span into a recording -------------------------------------------------------------------------------------------------
def to_pcm16(v):
    """Round to nearest (ties to even) and saturate to int16."""
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def crossfade_splice(rec, voc, lo, hi, X=1, hop=HOP, dtype=np.float64):
    """rec int16 [n]: the recording; voc float [>= n]: the vocoded audio of the same utterance in [-1, 1], sample-aligned with rec.  The output
    samples of frames [lo, hi) are the vocoded audio, to_pcm16(voc * 32768).  Over X frames on either side, out = to_pcm16(rec + w (voc * 32768 -
    rec)) with w = (i + 0.5) / (X hop) for the i-th sample counted from the fade's outer end, so w rises towards the core.  A side whose X frames
    are clipped by the utterance's start (lo - X < 0) or end ((hi + X) hop > n) gets no fade.  Every other sample keeps rec's bits."""
    rec = np.asarray(rec)
    if rec.dtype != np.int16 or rec.ndim != 1:
        raise ValueError("crossfade_splice: rec must be a 1-D int16 array")
    n = rec.size
    lo, hi, X = int(lo), int(hi), int(X)
    if not (0 <= lo < hi and (hi - 1) * hop < n) or X < 0:
        raise ValueError(f"crossfade_splice: frames [{lo}, {hi}) outside the {n} samples or X < 0")
    v = np.asarray(voc).astype(dtype)[:n] * dtype(32768.0)
    r = rec.astype(dtype)
    out = rec.copy()
    out[lo * hop:hi * hop] = to_pcm16(v[lo * hop:hi * hop])
    w = ((np.arange(X * hop) + 0.5) / (X * hop)).astype(dtype) if X > 0 else None
    if X > 0 and lo - X >= 0:
        s = slice((lo - X) * hop, lo * hop)
        out[s] = to_pcm16(r[s] + w * (v[s] - r[s]))
    if X > 0 and (hi + X) * hop <= n:
        s = slice(hi * hop, (hi + X) * hop)
        out[s] = to_pcm16(r[s] + w[::-1] * (v[s] - r[s]))
    return out
