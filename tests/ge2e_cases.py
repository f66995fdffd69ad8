"""Cases shared by tests/test_ge2e_cpu.py and tests/test_gpu_ge2e.py: the synthetic GE2E encoder, the recurrence cases with their float64
expectations and torch float32 yardsticks, the front-end rows and the clips of the whole path, each made once."""
import functools
import os

import numpy as np

from cmtts_amd import ge2e as g2
from cmtts_amd.weights import synth_ge2e_state_dict

FS = g2.SAMPLE_RATE
SEED = 0
TILE = 16                                     # windows per recurrence workgroup (csrc/ge2e.hip; profiles/ge2e.md)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ge2e.npz")
SLICE_COUNTS = (1, 1000, 35199, 35200, 35201, 43999, 44000, 52800, 52801, 61599, 61600, 220500)


@functools.lru_cache(maxsize=None)
def weights():
    return synth_ge2e_state_dict(SEED)


def layer_tensors(layer):
    sd = weights()
    return tuple(sd[f"lstm.{p}_l{layer}"] for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


# name: (layer whose matrices are used (0: K = 40, 1: K = 256), N windows, T steps, input scale, lengths or None)
def _lens(N, T):
    return tuple([T, 1, max(T - 1, 1)][i % 3] if i % 5 else T for i in range(N))


LSTM_CASES = {
    "l0_n1_t160": (0, 1, 160, 1.0, None),
    "l0_n15_t2": (0, TILE - 1, 2, 1.0, None),
    "l0_n17_t1": (0, TILE + 1, 1, 1.0, None),
    "l0_n35_t160": (0, 2 * TILE + 3, 160, 1.0, None),
    "l1_n1_t2": (1, 1, 2, 1.0, None),
    "l1_n17_t160": (1, TILE + 1, 160, 1.0, None),
    "l1_n35_t1": (1, 2 * TILE + 3, 1, 1.0, None),
    "l0_lengths": (0, 2 * TILE + 3, 160, 1.0, _lens(2 * TILE + 3, 160)),
    "l1_lengths": (1, TILE + 1, 160, 1.0, _lens(TILE + 1, 160)),
    "l0_saturated": (0, TILE + 1, 160, 100.0, None),      # power mels are not log-compressed and reach the hundreds: gates saturate
    "l0_default_scale": (0, TILE + 1, 160, 0.05, None),   # torch's default initialisation and small inputs: h stays near 0.08
}
GARBAGE = 1.0e30


@functools.lru_cache(maxsize=None)
def lstm_case(name):
    """(x float32 [N, T, K] with GARBAGE behind each window's frames, lengths or None, expected outputs float64 [N, T, 256], expected h
    float64 [N, 256]) of one recurrence case.  Layer 0 inputs are non-negative like power mels; inner inputs lie in (-1, 1) like an h."""
    layer, N, T, scale, lens = LSTM_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 31)
    K = 40 if layer == 0 else 256
    x = rs.standard_normal((N, T, K)).astype(np.float32)
    x = (np.abs(x) * scale).astype(np.float32) if layer == 0 else np.tanh(x).astype(np.float32)
    if lens is not None:
        for i, l in enumerate(lens):
            x[i, l:] = GARBAGE
    out, h = g2.lstm_layer(*layer_tensors(layer), x.astype(np.float64), lens)
    return x, lens, out, h


@functools.lru_cache(maxsize=None)
def lstm_float32(name):
    """The same layer through torch.nn.LSTM in float32 on the CPU: (outputs, h) — the yardstick of the kernel's error.  A window with a
    length runs alone on its own frames (torch has no freeze); its outputs beyond the length repeat the last one."""
    import torch
    layer, N, T, scale, lens = LSTM_CASES[name]
    x, _, _, _ = lstm_case(name)
    m = torch_lstm(40 if layer == 0 else 256, 1, {k.replace(f"_l{layer}", "_l0"): v for k, v in weights().items() if k.endswith(f"_l{layer}")})
    with torch.no_grad():
        if lens is None:
            o, (h, _) = m(torch.from_numpy(x))
            return o.numpy(), h[0].numpy()
        outs, hs = np.zeros((N, T, 256), np.float32), np.zeros((N, 256), np.float32)
        for i, l in enumerate(lens):
            o, (h, _) = m(torch.from_numpy(x[i:i + 1, :l]))
            outs[i, :l], outs[i, l:], hs[i] = o[0].numpy(), o[0, -1].numpy(), h[0, 0].numpy()
        return outs, hs


def torch_lstm(K, layers, sd, dtype=None):
    """torch.nn.LSTM(K, 256, layers, batch_first=True) loaded from the `lstm.*` entries of sd."""
    import torch
    m = torch.nn.LSTM(K, 256, layers, batch_first=True)
    m.load_state_dict({k[len("lstm."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if k.startswith("lstm.")})
    return (m.double() if dtype == "float64" else m).eval()


# ---- the front end --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mel_rows():
    """Rows of 35 200 (160 frames), 35 201 (161) and 221 samples (one hop + 1: 2 frames, shorter than the reflect padding): a tone over noise."""
    rs = np.random.RandomState(9)
    out = []
    for n in (35200, 35201, 221):
        t = np.arange(n) / FS
        out.append((0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 3100.0 * t + 1.0) + 0.05 * rs.standard_normal(n)).astype(np.float32))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mel_reference(i, dtype_name):
    return g2.mel_power(mel_rows()[i], np.dtype(dtype_name).type)


# ---- the whole path -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clips():
    """Three clips of 0.5 s (one padded partial), 2.0 s and 2.8 s, off the boundaries at which the last partial is dropped."""
    rs = np.random.RandomState(5)
    out = []
    for n, f0 in ((11025, 180.0), (44100, 240.0), (61740, 130.0)):
        t = np.arange(n) / FS
        env = 1 + 0.5 * np.sin(2 * np.pi * 3.1 * t)
        out.append(((0.3 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 3.7 * f0 * t)) * env + 0.02 * rs.standard_normal(n)).astype(np.float32))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_embeddings(using_partials, dtype_name):
    dt = np.dtype(dtype_name).type
    return np.stack([g2.embed_utterance(weights(), c, using_partials, dt) for c in clips()])
