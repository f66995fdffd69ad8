"""Recorded speech in, CPU side: the numpy definition (cmtts_amd/analysis.py) pinned against torch.stft, its frame counts and filterbank, the
host-only filterbank entry point (csrc/mel_basis.cpp) against it, phoneme_energy against the reference's loop, crossfade_splice's three
regions, the bound entry points, and the refusals, which leave a message and touch no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import analysis as A


def _signal(n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 22050.0
    x = 0.3 * np.sin(2 * np.pi * 311.0 * t) + 0.2 * np.sin(2 * np.pi * 2750.0 * t + 1.0) + 0.05 * rs.standard_normal(n)
    return x.astype(np.float32)


# ----------------------------------------------------------------------------- the STFT

@pytest.mark.parametrize("pad", ["reference", "vocoder"])
@pytest.mark.parametrize("n", [1024, 4000])
def test_magnitude_against_torch_stft(pad, n):
    x = _signal(n, n)
    mag = A.stft_magnitude(x, pad)
    tx = torch.from_numpy(x.astype(np.float64))
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    if pad == "reference":
        spec = torch.stft(tx, 1024, hop_length=256, win_length=1024, window=win, center=True, pad_mode="reflect", return_complex=True)
    else:
        padded = torch.nn.functional.pad(tx[None, None], (384, 384), mode="reflect")[0, 0]
        spec = torch.stft(padded, 1024, hop_length=256, win_length=1024, window=win, center=False, return_complex=True)
    ref = spec.abs().numpy().T
    assert mag.shape == ref.shape == (A.frame_count(n, pad), 513)
    err = np.abs(mag - ref).max(axis=1) / ref.max(axis=1)
    assert err.max() <= 1e-10, err.max()


@pytest.mark.parametrize("pad,cases", [("reference", {513: 3, 767: 3, 768: 4, 1024: 5, 4000: 16}),
                                       ("vocoder", {385: 1, 767: 2, 768: 3, 1024: 4, 4000: 15})])
def test_frame_counts(pad, cases):
    for n, frames in cases.items():
        assert A.frame_count(n, pad) == frames == (1 + n // 256 if pad == "reference" else n // 256)
        mel, energy = A.mel_from_wav(_signal(n, 1), pad)
        assert mel.shape == (frames, 80) and energy.shape == (frames,)
    assert A.frame_count(A.min_samples(pad), pad) == 0
    with pytest.raises(ValueError, match="too short"):
        A.stft_magnitude(_signal(A.min_samples(pad), 0), pad)


def test_energy_and_mel_follow_the_magnitude():
    x = _signal(3000, 5)
    mag = A.stft_magnitude(x)
    mel, energy = A.mel_from_wav(x)
    np.testing.assert_allclose(energy, np.linalg.norm(mag, axis=1), rtol=1e-14)
    np.testing.assert_allclose(mel, np.log(np.maximum(mag @ A.mel_basis().astype(np.float64).T, 1e-5)), rtol=0, atol=1e-14)
    # int16 is x / 32768; float is clipped to [-1, 1]
    pcm = (x * 20000).astype(np.int16)
    assert np.array_equal(A.to_float(pcm), pcm / 32768.0)
    assert np.array_equal(A.to_float(np.asarray([-2.0, 0.5, 3.0], np.float32)), [-1.0, 0.5, 1.0])
    out = A.mel_from_audio([x, x[:1000]], pad="vocoder", layout="ct")
    assert out["mel"].shape == (2, 80, 11) and list(out["mel_lens"]) == [11, 3]
    assert not out["mel"][1, :, 3:].any() and not out["energy"][1, 3:].any() and out["mel"][1, :, :3].all()


# ----------------------------------------------------------------------------- the filterbank

def test_basis_properties():
    basis = A.mel_basis()
    f = A.mel_corners()
    bins = np.linspace(0.0, 22050 / 2.0, 513)
    assert basis.dtype == np.float32 and basis.shape == (80, 513) and (basis >= 0).all()
    assert f.shape == (82,) and f[0] == 0.0 and abs(f[-1] - 8000.0) < 1e-9 and (np.diff(f) > 0).all()
    # the 1000 Hz break: linear at 200 / 3 Hz per mel below it, a constant ratio exp(step * ln(6.4) / 27) above
    step = float(A.hz_to_mel(8000.0)) / 81
    below, above = f[f <= 1000.0], f[f >= 1000.0]
    np.testing.assert_allclose(np.diff(below), step * 200.0 / 3.0, rtol=1e-12)
    np.testing.assert_allclose(above[1:] / above[:-1], np.exp(step * np.log(6.4) / 27.0), rtol=1e-12)
    assert abs(float(A.hz_to_mel(1000.0)) - 15.0) < 1e-12 and abs(float(A.mel_to_hz(A.hz_to_mel(4321.0))) - 4321.0) < 1e-9
    df = bins[1]
    for i in range(80):
        nz = np.nonzero(basis[i])[0]
        assert nz.size and (np.diff(nz) == 1).all()                              # one run of bins
        assert f[i] < bins[nz[0]] and bins[nz[-1]] < f[i + 2]                    # inside its corners
        assert f[i] <= bins[basis[i].argmax()] <= f[i + 2]
        assert abs(bins[basis[i].argmax()] - f[i + 1]) <= df                     # the peak is the bin next to the centre corner
        # unit area: 2 / (f[i+2] - f[i]) times the triangle's area (f[i+2] - f[i]) / 2, sampled every df — to within one bin of the peak height
        assert abs(basis[i].astype(np.float64).sum() * df - 1.0) <= df * 2.0 / (f[i + 2] - f[i])
    # a bin feeds at most two filters
    assert ((basis > 0).sum(axis=0) <= 2).all()


@pytest.mark.parametrize("args", [(22050, 1024, 80, 0.0, 8000.0), (22050, 1024, 80, 0.0, 11025.0), (16000, 512, 40, 50.0, 7600.0)])
def test_basis_entry_point_matches_the_definition(args):
    lib = _lib.load()
    fs, n_fft, n_mels, fmin, fmax = args
    out = np.empty((n_mels, n_fft // 2 + 1), np.float32)
    assert lib.cmtts_mel_basis(fs, n_fft, n_mels, fmin, fmax, out.ctypes.data) == 0
    np.testing.assert_allclose(out, A.mel_basis(fs, n_fft, n_mels, fmin, fmax), rtol=1e-6, atol=0)


# ----------------------------------------------------------------------------- phoneme energy

def _reference_loop(energy, duration, mean, std):
    """preprocessor/preprocessor.py:293-305 and normalize (426-437), line for line."""
    energy = np.array(energy[: sum(duration)])
    pos = 0
    for i, d in enumerate(duration):
        if d > 0:
            energy[i] = np.mean(energy[pos: pos + d])
        else:
            energy[i] = 0
        pos += d
    energy = energy[: len(duration)]
    return (energy - mean) / std


def test_phoneme_energy_against_the_reference_loop():
    """Durations with zeros, placed so that the loop (which writes into the array it reads) has not yet overwritten a frame it goes on to read:
    sum(d[:l]) >= l throughout — see analysis.phoneme_energy."""
    rs = np.random.RandomState(3)
    durs = np.asarray([[3, 0, 2, 5, 0, 0, 1, 4], [2, 2, 0, 7, 1, 0, 3, 0]])
    energy = rs.uniform(0.5, 40.0, size=(2, 18))
    energy[1, 15:] = 0.0                                      # row 1 has 15 frames
    mean, std = 21.7, 9.3
    got = A.phoneme_energy(energy, durs, mean, std)
    for b in range(2):
        assert all(durs[b, :l].sum() >= l for l in range(durs.shape[1]))
        np.testing.assert_allclose(got[b], _reference_loop(energy[b], list(durs[b]), mean, std), rtol=1e-13, atol=1e-13)
    assert got[0, 1] == (0.0 - mean) / std                    # the zeros are normalised too
    with pytest.raises(ValueError):
        A.phoneme_energy(energy, durs[:1], mean, std)
    with pytest.raises(ValueError):
        A.phoneme_energy(energy, -durs, mean, std)


# ----------------------------------------------------------------------------- the crossfade

def test_crossfade_splice_regions():
    rs = np.random.RandomState(9)
    hop, T = 256, 12
    rec = rs.randint(-20000, 20000, size=T * hop).astype(np.int16)
    voc = rs.uniform(-0.9, 0.9, size=T * hop)
    out = A.crossfade_splice(rec, voc, 4, 7, X=2)
    assert np.array_equal(out[:2 * hop], rec[:2 * hop]) and np.array_equal(out[9 * hop:], rec[9 * hop:])
    assert np.array_equal(out[4 * hop:7 * hop], np.rint(voc[4 * hop:7 * hop] * 32768).astype(np.int16))
    # the fades rise towards the core: nearly the recording at the outer end, nearly the vocoded audio next to the core
    w = (np.arange(2 * hop) + 0.5) / (2 * hop)
    lead = rec[2 * hop:4 * hop] + w * (voc[2 * hop:4 * hop] * 32768 - rec[2 * hop:4 * hop])
    trail = rec[7 * hop:9 * hop] + w[::-1] * (voc[7 * hop:9 * hop] * 32768 - rec[7 * hop:9 * hop])
    assert np.array_equal(out[2 * hop:4 * hop], np.rint(lead).astype(np.int16)) and np.array_equal(out[7 * hop:9 * hop], np.rint(trail).astype(np.int16))
    assert abs(int(out[2 * hop]) - int(rec[2 * hop])) <= 1 + 65536 // (4 * hop)
    # a clipped side gets no fade: the span touches frame 0 / the fade would pass the end
    head = A.crossfade_splice(rec, voc, 0, 3, X=2)
    assert np.array_equal(head[:3 * hop], np.rint(voc[:3 * hop] * 32768).astype(np.int16)) and not np.array_equal(head[3 * hop:5 * hop], rec[3 * hop:5 * hop])
    assert np.array_equal(head[5 * hop:], rec[5 * hop:])
    tail = A.crossfade_splice(rec, voc, 1, 3, X=2)             # lo - X < 0
    assert np.array_equal(tail[:hop], rec[:hop])
    end = A.crossfade_splice(rec, voc, 8, 11, X=2)             # (hi + X) hop > n
    assert np.array_equal(end[11 * hop:], rec[11 * hop:]) and np.array_equal(end[:6 * hop], rec[:6 * hop])
    # saturation, and X = 0 is a hard cut
    loud = A.crossfade_splice(rec, np.full(T * hop, 1.0), 4, 7, X=0)
    assert (loud[4 * hop:7 * hop] == 32767).all() and np.array_equal(loud[:4 * hop], rec[:4 * hop]) and np.array_equal(loud[7 * hop:], rec[7 * hop:])
    with pytest.raises(ValueError):
        A.crossfade_splice(rec, voc, 5, 5)
    with pytest.raises(ValueError):
        A.crossfade_splice(rec.astype(np.int32), voc, 1, 2)


# ----------------------------------------------------------------------------- the entry points

NAMES = ("cmtts_mel_basis", "cmtts_analysis_create", "cmtts_analysis_destroy", "cmtts_analysis_workspace_bytes", "cmtts_mel_analysis",
         "cmtts_phoneme_energy", "cmtts_pcm_crossfade")


def test_signatures_bound_and_abi_unchanged():
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert lib.cmtts_abi_version() == 8 == _lib.ABI_VERSION
    assert lib.cmtts_set_option(b"analysis", 1) == -1         # no public option came with it


def test_entry_points_refuse_before_the_gpu():
    lib = _lib.load()
    h = C.c_void_p()
    for geo in ((22050, 2048, 256, 1024, 80), (22050, 1024, 200, 1024, 80), (22050, 1024, 256, 800, 80), (22050, 1024, 256, 1024, 64)):
        assert lib.cmtts_analysis_create(*geo, 0.0, 8000.0, C.byref(h)) == -1 and b"unsupported geometry" in lib.cmtts_last_error()
        assert not h.value
    assert lib.cmtts_analysis_create(4000, 1024, 256, 1024, 80, 0.0, 2000.0, C.byref(h)) == -1 and b"fs" in lib.cmtts_last_error()
    assert lib.cmtts_analysis_create(22050, 1024, 256, 1024, 80, 0.0, 12000.0, C.byref(h)) == -1
    assert lib.cmtts_analysis_create(22050, 1024, 256, 1024, 80, 0.0, 8000.0, None) == -1 and b"null" in lib.cmtts_last_error()
    lib.cmtts_analysis_destroy(None)
    out = np.empty((80, 513), np.float32)
    assert lib.cmtts_mel_basis(22050, 1024, 80, 0.0, 12000.0, out.ctypes.data) == -1 and b"fmax" in lib.cmtts_last_error()
    assert lib.cmtts_mel_basis(22050, 1023, 80, 0.0, 8000.0, out.ctypes.data) == -1
    assert lib.cmtts_mel_basis(22050, 1024, 80, 0.0, 8000.0, None) == -1
    assert lib.cmtts_analysis_workspace_bytes(3, 16) > 0
    assert lib.cmtts_analysis_workspace_bytes(0, 16) == 0 and lib.cmtts_analysis_workspace_bytes(3, 0) == 0 and lib.cmtts_analysis_workspace_bytes(70000, 16) == 0
    assert lib.cmtts_mel_analysis(None, 1, 0, 1, 4000, 1, 0, 16, 0, 1, 1, 1, 1, 256, None) == -1 and b"null" in lib.cmtts_last_error()
    assert lib.cmtts_phoneme_energy(None, 1, 8, 1, 4, 0.0, 1.0, 1, None) == -1 and b"null" in lib.cmtts_last_error()
    assert lib.cmtts_phoneme_energy(1, 1, 8, 1, 4, 0.0, 0.0, 1, None) == -1 and b"std" in lib.cmtts_last_error()
    assert lib.cmtts_phoneme_energy(1, 0, 8, 1, 4, 0.0, 1.0, 1, None) == -1
    assert lib.cmtts_pcm_crossfade(None, 1, 1, 1, 4, 1, 256, 1, None) == -1 and b"null" in lib.cmtts_last_error()
    assert lib.cmtts_pcm_crossfade(1, 1, 1, 1, 0, 1, 256, 1, None) == -1 and b"core" in lib.cmtts_last_error()
    assert lib.cmtts_pcm_crossfade(1, 1, 1, 1, 4, -1, 256, 1, None) == -1


def test_host_refuses_before_the_gpu():
    """Another geometry, a row at or below the minimum length and mismatched shapes raise from the host layer before it asks for a device."""
    from cmtts_amd import host
    bad = {"preprocessing": {"stft": {"filter_length": 1024, "hop_length": 300, "win_length": 1024}, "mel": {"n_mel_channels": 80}}}
    with pytest.raises(ValueError, match="not supported"):
        host.get_analyzer(bad, device="cpu")
    with pytest.raises(ValueError, match="sample rate"):
        host.get_analyzer({"preprocessing": {"audio": {"sampling_rate": 16000}}}, device="cpu")
    an = host.get_analyzer(device="cpu")                      # loads, cannot run
    assert not an._ready and an.fmax == 8000.0
    with pytest.raises(ValueError, match="too short"):
        host.mel_from_audio(an, np.zeros((2, 4000), np.float32), lengths=[4000, 512])
    with pytest.raises(ValueError, match="too short"):
        host.mel_from_audio(an, [np.zeros(4000, np.int16), np.zeros(384, np.int16)], pad="vocoder")
    with pytest.raises(ValueError, match="pad"):
        host.mel_from_audio(an, np.zeros((1, 4000), np.float32), pad="center")
    with pytest.raises(ValueError, match="layout"):
        host.mel_from_audio(an, np.zeros((1, 4000), np.float32), layout="bt")
    with pytest.raises(ValueError, match="length"):
        host.mel_from_audio(an, np.zeros((2, 4000), np.float32), lengths=[4000])
    with pytest.raises(ValueError, match="int16"):
        host.mel_from_audio(an, np.zeros((1, 4000), np.int32))
    with pytest.raises(ValueError, match="do not fit"):
        host.energy_targets(an, np.zeros((2, 16), np.float32), np.ones((3, 4), np.int64), 0.0, 1.0)
    with pytest.raises(ValueError, match="std"):
        host.energy_targets(an, np.zeros((2, 16), np.float32), np.ones((2, 4), np.int64), 0.0, 0.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no GPU"):
            host.mel_from_audio(an, np.zeros((1, 4000), np.float32))
