"""Loudness measurement and output gain on the device (include/cmtts_hip.h: cmtts_loudness_measure, cmtts_resample_encode_gain;
host.vocoder_loudness, vocoder_infer with loudness / gain_db / stats, vocoder_infer_stream with gain_db): the kernels against the float64
definition (cmtts_amd/loudness.py), row independence, the gain rules, the gained resampler against cmtts_amd/resample.py, the one-shot
call end to end and the stream bitwise against it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import loudness as ld
from cmtts_amd import resample as rs
from cmtts_amd.config import HifiGanConfig
from cmtts_amd.weights import synth_hifigan_state_dict
from conftest import report
from loudness_cases import BLOCK, FS, GATE_MARGIN, LENGTHS, SIGNALS, gate_margin, pin, reference, signal
from resample_cases import GARBAGE, definition_and_bound, filt, waves

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = HifiGanConfig().hop
TORCH_DTYPE = {"f32": torch.float32, "s16": torch.int16, "mulaw": torch.uint8, "alaw": torch.uint8}
HARD_CAP = 0.1          # LU: the meter tolerance of EBU Tech 3341


def _host():
    from cmtts_amd import host
    return host


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _measure(xs, ld_, target=None, ceiling_db=-1.0, fs=FS):
    """cmtts_loudness_measure on rows xs (GARBAGE after each row's valid samples) -> stats float32 numpy [rows, 4]."""
    lib = _lib.load()
    buf = np.full((len(xs), ld_), GARBAGE, np.float32)
    for i, x in enumerate(xs):
        buf[i, : len(x)] = x
    wav = torch.from_numpy(buf).to(DEV)
    n_valid = torch.tensor([len(x) for x in xs], dtype=torch.int32, device=DEV)
    tgt = None if target is None else torch.tensor(target, dtype=torch.float32, device=DEV)
    stats = torch.full((len(xs), 4), 777.0, device=DEV)
    nb = lib.cmtts_loudness_workspace_bytes(len(xs), ld_, fs)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_loudness_measure(wav.data_ptr(), len(xs), ld_, n_valid.data_ptr(), fs, None if tgt is None else tgt.data_ptr(),
                                          ceiling_db, stats.data_ptr(), ws.data_ptr(), nb, _stream()))
    return stats.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- a. kernel vs definition

@pytest.mark.parametrize("name", SIGNALS)
def test_kernel_against_definition(name):
    x = signal(name)
    ld_ = len(x) + 37
    assert ld_ % (FS // 10) and max(LENGTHS) == len(x)
    xs = [x[:n] for n in LENGTHS]
    st = _measure(xs, ld_)
    worst = (0.0, 0.0, 0)
    for i, n in enumerate(LENGTHS):
        L, nb, ng = reference(name, n)
        assert gate_margin(name, n) >= GATE_MARGIN, f"{name} n = {n}: a block within {GATE_MARGIN} LU of a gate"
        Ld, pk, g, blocks = (float(v) for v in st[i])
        assert np.float32(pk) == np.float32(ld.sample_peak(xs[i])), f"{name} n = {n}: peak {pk}"
        assert blocks == ng, f"{name} n = {n}: {blocks} gated blocks, the definition has {ng} of {nb}"
        assert g == 1.0
        if math.isinf(L):
            assert Ld == -math.inf, f"{name} n = {n}: L = {Ld}, the definition has -inf"
            continue
        bound, d32 = pin(name, n)
        d = abs(Ld - L)
        print(f"LOUDNESS {name} n = {n}: L = {Ld:.6f}, definition {L:.6f}, |d| = {d:.2e}, d32 = {d32:.2e}, pin {bound:.2e}")
        if d / bound > worst[0]:
            worst = (d / bound, d, n)
        assert d <= HARD_CAP, f"{name} n = {n}: {d:.3e} LU off"
        assert d <= bound, f"{name} n = {n}: {d:.3e} LU off, pin {bound:.3e} (d32 = {d32:.3e})"
    report(f"LOUDNESS {name}: largest deviation from the float64 definition {worst[1]:.2e} LU at n = {worst[2]} ({worst[0]:.2f} of its pin)")


def test_other_sample_rate():
    """48 kHz: another chunk, run and matrix set (the 3 s full-scale sine of BS.1770: -3.01 LKFS)."""
    fs = 48000
    x = np.sin(2 * np.pi * 997 * np.arange(3 * fs) / fs).astype(np.float32)
    L, nb, ng = ld.integrated_loudness(x, fs)
    st = _measure([x, x[: fs // 2]], len(x) + 11, fs=fs)
    d32 = abs(ld.integrated_loudness(x, fs, np.float32)[0] - L)
    assert abs(float(st[0, 0]) - L) <= max(10 * d32, 2e-4) and st[0, 3] == ng and abs(float(st[0, 0]) + 3.01) <= 0.01
    assert st[1, 3] == 2 and st[0, 1] == np.float32(ld.sample_peak(x))


# ---------------------------------------------------------------------------------------------------- b. row independence

def test_row_independence():
    a, b, c = signal("modulated"), signal("gating"), signal("dc")
    ld_ = len(a) + 37
    rows = [b[:20000], a[:31337], c[:9000], a]
    tgt = [-16.0, -23.0, -20.0, -30.0]
    batch = _measure(rows, ld_, tgt)
    for i in (1, 3):
        alone = _measure([rows[i]], ld_, [tgt[i]])
        assert alone[0].tobytes() == batch[i].tobytes(), i


# ---------------------------------------------------------------------------------------------------- c. gain on the device

def test_gain_on_device():
    x = signal("modulated")
    targets = [-16.0, -23.0, math.nan, -5.0]
    st = _measure([x, x[:40000], x, x], len(x) + 37, targets, ceiling_db=-1.0)
    # rtol 2e-6: float32 rounding of an exponent of at most 3 (1.8e-7 absolute) times ln 10, plus two ulps of the exponential
    for i in (0, 1):
        want = 10.0 ** ((targets[i] - float(st[i, 0])) / 20.0)
        assert float(st[i, 1]) * want <= 10 ** (-1 / 20)
        assert abs(float(st[i, 2]) - want) <= 2e-6 * want, i
    assert st[2, 2] == 1.0 and st[2, 0] == st[0, 0]
    # the ceiling takes over: g = ceiling / peak, two float32 roundings (the ceiling, the division)
    assert float(st[3, 1]) * 10.0 ** ((targets[3] - float(st[3, 0])) / 20.0) > 10 ** (-1 / 20)
    want = 10 ** (-1 / 20) / float(st[3, 1])
    assert abs(float(st[3, 2]) - want) <= 2.0 ** -22 * want
    assert abs(float(st[3, 2]) - ld.gain_for(reference("modulated", len(x))[0], ld.sample_peak(x), -5.0, -1.0)) <= 2.0 ** -22 * want
    # no target table at all, silence and an empty row with a target: gain 1
    z = _measure([x[:1000]], 5000)
    assert z[0, 2] == 1.0
    s = _measure([np.zeros(30000, np.float32), x[:0]], 30011, [-16.0, -16.0])
    assert s[0].tolist() == [-math.inf, 0.0, 1.0, 0.0] and s[1].tolist() == [-math.inf, 0.0, 1.0, 0.0]


# ---------------------------------------------------------------------------------------------------- d. the gained resampler

class _Resampler:
    def __init__(self, rate):
        self.lib = _lib.load()
        self.L, self.M, self.taps, self.half, self.R = filt(rate)
        self.h = C.c_void_p()
        _lib.check(self.lib.cmtts_resampler_create(self.L, self.M, self.taps.ctypes.data_as(C.c_void_p), self.half, C.byref(self.h)))

    def __del__(self):
        self.lib.cmtts_resampler_destroy(self.h)

    def encode(self, wav, segs, encoding, out_ld, gains="plain"):
        """cmtts_resample_encode (gains "plain") or cmtts_resample_encode_gain (a tensor or None) -> [N, out_ld] numpy."""
        tab = torch.tensor(segs, dtype=torch.int32, device=DEV)
        out = torch.full((len(segs), out_ld), 1, dtype=TORCH_DTYPE[encoding], device=DEV)
        args = (self.h, wav.data_ptr(), wav.shape[0], wav.shape[1], tab.data_ptr(), len(segs), rs.ENCODINGS[encoding], 32768.0,
                out.data_ptr(), out_ld)
        if isinstance(gains, str):
            _lib.check(self.lib.cmtts_resample_encode(*args, _stream()))
        else:
            _lib.check(self.lib.cmtts_resample_encode_gain(*args, None if gains is None else gains.data_ptr(), _stream()))
        return out.cpu().numpy()


GAINS = (0.37, 1.9, 1.0, 2.5)


@pytest.mark.parametrize("rate", [8000, 22050])
def test_resample_encode_gain(rate):
    """Against cmtts_amd/resample.py applied to fl32(g x), with the bounds and bit-exactness rules of test_gpu_resample.py."""
    r = _Resampler(rate)
    assert (rate != 22050) or (r.L, r.M) == (1, 1)
    xs = waves(rate)
    buf = np.full((len(xs), 1000), GARBAGE, np.float32)
    for i, x in enumerate(xs):
        buf[i, : len(x)] = x
    wav = torch.from_numpy(buf).to(DEV)
    gains = torch.tensor(GAINS, dtype=torch.float32, device=DEV)
    nout = [rs.out_len(len(x), r.L, r.M) for x in xs]
    segs = [(i, 0, 0, nout[i], len(x)) for i, x in enumerate(xs)]
    out_ld = max(nout) + 3
    got = {enc: r.encode(wav, segs, enc, out_ld, gains) for enc in rs.ENCODINGS}
    ndiff = total = 0
    for i, x in enumerate(xs):
        gx = ld.apply_gain(x, GAINS[i])
        y, bound = definition_and_bound(gx, r.L, r.M, r.taps, r.half)
        n = nout[i]
        for enc in rs.ENCODINGS:
            assert not got[enc][i, n:].any(), f"row {i} {enc}: no zeros after the segment"
        d = np.abs(got["f32"][i, :n].astype(np.float64) - y)
        assert (d <= bound).all(), f"{rate} Hz row {i}: {d.max():.3e} off"
        d = np.abs(got["s16"][i, :n].astype(np.int64) - rs.to_s16(y))
        assert d.max(initial=0) <= 1, f"{rate} Hz row {i}: s16 {d.max()} LSB from the definition"
        ndiff += int(np.count_nonzero(d))
        total += n
        assert np.array_equal(got["mulaw"][i, :n], rs.lin2ulaw(got["s16"][i, :n]))
        assert np.array_equal(got["alaw"][i, :n], rs.lin2alaw(got["s16"][i, :n]))
    assert np.abs(got["s16"].astype(np.int32)).max() == 32768 or np.abs(got["s16"].astype(np.int32)).max() == 32767          # 2.5 x saturates
    report(f"RESAMPLE with gain {rate} Hz: s16 {ndiff} of {total} samples 1 LSB from the float64 definition")
    assert ndiff <= 0.01 * total
    # gains = NULL is cmtts_resample_encode, and a gain of 1 changes no bit either
    ones = torch.ones(len(xs), device=DEV)
    for enc in rs.ENCODINGS:
        plain = r.encode(wav, segs, enc, out_ld)
        assert r.encode(wav, segs, enc, out_ld, None).tobytes() == plain.tobytes(), enc
        assert r.encode(wav, segs, enc, out_ld, ones).tobytes() == plain.tobytes(), enc


# ---------------------------------------------------------------------------------------------------- e. end to end

def _voc(seed=3):
    hcfg = HifiGanConfig()
    voc = _host().Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=seed))
    assert voc.set_option("winograd", 0) in (0, 1)
    return voc


def _mels(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 80, T, generator=g) * 0.8 - 1.0).to(DEV)


@pytest.fixture(scope="module")
def e2e():
    voc = _voc()
    frames = [40, 35, 12]
    return voc, _mels(3, 40, 21), [f * HOP for f in frames]


def test_vocoder_infer_loudness(e2e):
    voc, mel, lens = e2e
    host = _host()
    assert lens[2] < BLOCK <= lens[1]
    wav = voc(mel)[:, 0].cpu().numpy()
    s = []
    out = host.vocoder_infer(mel, voc, lengths=lens, loudness=-23, encoding="f32", stats=s)
    assert len(s) == 3 and all(set(d) == {"lufs", "peak", "gain_db", "blocks"} for d in s)
    fixed = host.vocoder_infer(mel, voc, lengths=lens, gain_db=[d["gain_db"] for d in s], encoding="f32")
    L, M, taps, half = 1, 1, np.ones(1, np.float32), 0          # the native rate with a gain: the single tap 1, nothing is filtered
    for b, n in enumerate(lens):
        assert out[b].dtype == np.float32 and len(out[b]) == n
        assert out[b].tobytes() == fixed[b].tobytes(), f"utterance {b}: loudness= and its own gain_db differ"
        x = wav[b, :n]
        Ldef, _, ng = ld.integrated_loudness(x, FS)
        d32 = abs(ld.integrated_loudness(x, FS, np.float32)[0] - Ldef)
        bound = max(10 * d32, 2e-4)
        g = 10.0 ** (s[b]["gain_db"] / 20.0)
        assert s[b]["blocks"] == ng and np.float32(s[b]["peak"]) == np.float32(ld.sample_peak(x))
        assert abs(s[b]["lufs"] - Ldef) <= bound, f"utterance {b}: measured {s[b]['lufs']}, definition {Ldef}"
        want = ld.gain_for(Ldef, ld.sample_peak(x), -23.0, -1.0)
        limited = ld.sample_peak(x) * 10.0 ** ((-23.0 - Ldef) / 20.0) > 10 ** (-1 / 20)
        # the delivered row is the definition's resampling of fl32(g x)
        y, ybound = definition_and_bound(ld.apply_gain(x, g), L, M, taps, half)
        assert (np.abs(out[b].astype(np.float64) - y) <= ybound).all(), b
        Lout = ld.integrated_loudness(out[b], FS)[0]
        print(f"LOUDNESS e2e utterance {b}: L = {s[b]['lufs']:.5f} (definition {Ldef:.5f}), gain {s[b]['gain_db']:.4f} dB, "
              f"ceiling {'on' if limited else 'off'}, delivered row {Lout:.5f} LKFS, pin {bound:.2e}")
        if n < BLOCK:
            # no 0.4 s block: the gain against gain_for of the definition's single-block L (an error of the bound in L, in the exponent)
            assert abs(g / want - 1.0) <= bound * math.log(10) / 20 + 2e-6, f"utterance {b}: gain {g}, gain_for {want}"
        elif not limited:
            assert abs(Lout - (-23.0)) <= bound, f"utterance {b}: the delivered row has {Lout} LKFS"
    # measured only: the same stats, gain 1
    m = host.vocoder_loudness(mel, voc, lengths=lens)
    assert m.dtype == np.float32 and m.shape == (3, 4) and (m[:, 2] == 1.0).all()
    for b in range(3):
        assert float(m[b, 0]) == s[b]["lufs"] and float(m[b, 1]) == s[b]["peak"] and int(m[b, 3]) == s[b]["blocks"]
    # NaN leaves an utterance alone; s16 saturates on the float path
    part = host.vocoder_infer(mel, voc, lengths=lens, loudness=[-23.0, math.nan, -23.0], encoding="f32")
    unity = host.vocoder_infer(mel, voc, lengths=lens, gain_db=0.0, encoding="f32")
    assert part[0].tobytes() == out[0].tobytes() and part[1].tobytes() == unity[1].tobytes() == wav[1, : lens[1]].tobytes()
    loud = host.vocoder_infer(mel, voc, lengths=lens, gain_db=40.0)
    assert all(w.dtype == np.int16 and w.max() == 32767 and w.min() == -32768 for w in loud)


def test_vocoder_infer_unchanged_without_the_keywords(e2e):
    voc, mel, lens = e2e
    host = _host()
    dev = host.vocoder_infer_device(mel, voc).cpu().numpy()
    plain = host.vocoder_infer(mel, voc, lengths=lens)
    s = []
    measured = host.vocoder_infer(mel, voc, lengths=lens, stats=s)
    m = host.vocoder_loudness(mel, voc, lengths=lens)
    for b, n in enumerate(lens):
        assert plain[b].dtype == np.int16 and np.array_equal(plain[b], dev[b, :n]) and np.array_equal(measured[b], plain[b])
        assert s[b]["gain_db"] == 0.0 and s[b]["lufs"] == float(m[b, 0])


def test_keyword_validation(e2e):
    voc, mel, lens = e2e
    host = _host()
    with pytest.raises(ValueError, match="not both"):
        host.vocoder_infer(mel, voc, lengths=lens, loudness=-23, gain_db=1.0)
    with pytest.raises(ValueError):
        host.vocoder_infer(mel, voc, lengths=lens, gain_db=[1.0, 2.0])
    with pytest.raises(ValueError):
        host.vocoder_infer(mel, voc, lengths=lens, gain_db=math.inf)
    with pytest.raises(ValueError, match="whole utterance.*vocoder_loudness.*gain_db"):
        next(host.vocoder_infer_stream(mel, object(), loudness=-23))          # refused before the vocoder is touched
    with pytest.raises(ValueError, match="whole utterance"):
        next(host.synthesize_stream(None, voc, None, None, loudness=-16))


# ---------------------------------------------------------------------------------------------------- f. stream

def _collect(stream_iter, out_lens, dtype):
    """(utterance, offset, chunk, is_last) -> one array per utterance; checks offsets, dtype and is_last."""
    parts = [[] for _ in out_lens]
    pos = [0] * len(out_lens)
    for b, off, chunk, last in stream_iter:
        assert off == pos[b] and chunk.dtype == dtype
        parts[b].append(chunk)
        pos[b] += len(chunk)
        assert last == (pos[b] == out_lens[b])
    return [np.concatenate(p) for p in parts]


def test_stream_with_gain_equals_one_shot_bitwise():
    voc = _voc()
    host = _host()
    T, lens, gains = 70, [70, 41], [-3.0, 2.5]
    mel = _mels(2, T, 13)
    Lr, Mr = rs.ratio(rs.NATIVE_RATE, 8000)
    ref = host.vocoder_infer(mel, voc, lengths=[n * HOP for n in lens], gain_db=gains, sample_rate=8000, encoding="mulaw")
    ungained = host.vocoder_infer(mel, voc, lengths=[n * HOP for n in lens], sample_rate=8000, encoding="mulaw")
    assert not np.array_equal(ref[0], ungained[0]) and not np.array_equal(ref[1], ungained[1])
    got = _collect(host.vocoder_infer_stream(mel, voc, lens, (32, 64), gain_db=gains, sample_rate=8000, encoding="mulaw"),
                   [rs.out_len(n * HOP, Lr, Mr) for n in lens], np.uint8)
    for b in range(2):
        assert got[b].tobytes() == ref[b].tobytes(), f"utterance {b}: {np.count_nonzero(got[b] != ref[b])} samples differ"
    # the native format with a gain takes the float path in both forms
    ref = host.vocoder_infer(mel, voc, lengths=[n * HOP for n in lens], gain_db=-6.0)
    got = _collect(host.vocoder_infer_stream(mel, voc, lens, (32, 64), gain_db=-6.0), [n * HOP for n in lens], np.int16)
    assert all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
