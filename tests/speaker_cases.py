"""Cases shared by tests/test_speaker_cpu.py and tests/test_gpu_speaker.py: the conv shapes, the trim and fbank signals, the utterances of
the whole path and the synthetic ResCNN, each made once."""
import functools

import numpy as np

from cmtts_amd import speaker as sp
from cmtts_amd.weights import synth_deepspeaker_state_dict

FS = 22050
FRAME_LEN, FRAME_STEP, NFFT = sp.frame_geometry(FS, 1024)
SEED = 0

# name: (k, stride, cin, cout, H, W, B, residual)
CONV_CASES = {
    "a": (5, 2, 1, 64, 6, 8, 2, False),          # first layer, even sizes
    "b": (5, 2, 1, 64, 5, 7, 2, False),          # first layer, odd sizes
    "c": (5, 2, 64, 128, 6, 4, 1, False),        # strided stage, small even size
    "d": (5, 2, 64, 128, 5, 3, 1, False),        # strided stage, small odd size
    "e": (3, 1, 64, 64, 5, 3, 3, True),          # residual path; 45 pixels: no multiple of a tile
    "f": (3, 1, 512, 512, 10, 4, 1, False),      # long K, last-stage shape
    "g": (3, 1, 512, 512, 3, 4, 1, False),       # 12 pixels: fewer than one tile
}


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """(x [B,H,W,cin], kernel, bias, res or None, expected float64) of one conv case.  Inputs are non-negative like the activations the net
    feeds its convs, weights are N(0, 2 / sqrt(fan_in)) and the bias is spread over +-3, which puts outputs on both clips
    (tests/test_speaker_cpu.py asserts it for every case)."""
    k, s, cin, cout, H, W, B, residual = CONV_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 17)
    x = np.abs(rs.standard_normal((B, H, W, cin))).astype(np.float32) * 6.0
    kernel = (rs.standard_normal((k, k, cin, cout)) * 2.0 / np.sqrt(k * k * cin)).astype(np.float32)
    bias = (rs.standard_normal(cout) * 3.0).astype(np.float32)
    y = sp.clip(sp.conv2d_same(x.astype(np.float64), kernel, bias, s))
    res = None
    if residual:
        res = (np.maximum(rs.standard_normal(y.shape), 0) * 6.0).astype(np.float32)       # like a clipped activation: zeros included
        y = sp.clip(y + res.astype(np.float64))
    return x, kernel, bias, res, y


def conv_float32(name):
    """The same layer in torch CPU float32: the yardstick of the kernel's error."""
    import torch
    import torch.nn.functional as F
    k, s, cin, cout, H, W, B, residual = CONV_CASES[name]
    x, kernel, bias, res, _ = conv_case(name)
    y = torch_conv_same(torch.from_numpy(x), torch.from_numpy(kernel), torch.from_numpy(bias), s).clamp(0, 20)
    if res is not None:
        y = (y + torch.from_numpy(res)).clamp(0, 20)
    return y.numpy()


def torch_conv_same(x, kernel, bias, stride):
    """NHWC in / out through F.conv2d with TensorFlow's asymmetric 'same' padding written out as an explicit F.pad."""
    import torch.nn.functional as F
    kh, kw = kernel.shape[:2]
    pt, pb, _ = sp.same_pad(x.shape[1], kh, stride)
    pl, pr, _ = sp.same_pad(x.shape[2], kw, stride)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, kernel.permute(3, 2, 0, 1), bias, stride=stride).permute(0, 2, 3, 1)


# ---- trim -----------------------------------------------------------------------------------------------------------------------------
def trim_signals():
    """name -> float32 signal.  "silence" and "square" keep nothing; "two" (n = 2) keeps nothing either: one sample above the threshold."""
    rs = np.random.RandomState(3)
    n = 5000
    ramp = (np.arange(n, dtype=np.float32) - 1800.0) / 4096.0                   # distinct magnitudes, sign change inside
    ties = np.round(rs.standard_normal(n) * 3.0).astype(np.float32) / 4.0        # a handful of distinct magnitudes: ties around the threshold
    return {"ramp": ramp, "ties": ties, "two": np.asarray([0.25, -0.5], np.float32), "silence": np.zeros(777, np.float32),
            "square": np.where(np.arange(600) % 7 < 3, 0.5, -0.5).astype(np.float32)}


# ---- fbank ----------------------------------------------------------------------------------------------------------------------------
def fbank_signals():
    """name -> float32 signal handed to the fbank alone (no trim): lengths of 1, 2 and 163 frames, a pure tone and an impulse."""
    rs = np.random.RandomState(4)

    def noise(n):
        return (rs.standard_normal(n) * 0.1).astype(np.float32)
    t = np.arange(3 * FRAME_LEN) / FS
    imp = np.zeros(2 * FRAME_LEN, np.float32)
    imp[300] = 1.0
    return {"frames1": noise(FRAME_LEN), "frames2": noise(FRAME_LEN + 1), "frames163": noise(FRAME_LEN + FRAME_STEP * 162),
            "tone": (0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32), "impulse": imp}


# ---- the whole path -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def utterances():
    """Three utterances of different lengths (the second shorter than 160 frames): amplitude-modulated tones over noise, so that the trim
    cuts inside them."""
    rs = np.random.RandomState(5)
    out = []
    for n, f0 in ((60000, 180.0), (21000, 240.0), (44000, 130.0)):
        t = np.arange(n) / FS
        env = np.clip(np.sin(np.pi * t / t[-1]) * 1.5, 0, 1) * (1 + 0.5 * np.sin(2 * np.pi * 3.1 * t))
        out.append(((0.3 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 3.7 * f0 * t)) * env + 0.02 * rs.standard_normal(n)).astype(np.float32))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def weights():
    return synth_deepspeaker_state_dict(SEED)


@functools.lru_cache(maxsize=None)
def reference_embeddings(windows, dtype_name):
    """The definition on utterances() in float64 / float32, computed once per mode."""
    return sp.speaker_embedding(weights(), list(utterances()), windows=windows, dtype=np.dtype(dtype_name).type)
