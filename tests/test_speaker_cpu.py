"""The speaker encoder's definition (cmtts_amd/speaker.py), its synthetic weights and its host-side weight packer, on the CPU: the numpy
'same' convolution pinned by torch float64, the shapes of the net, the fbank and trim rules, the BatchNorm fold and the fragment stream
against the unfolded float64 layer, and the condition on the synthetic weights that makes the GPU comparisons meaningful."""
import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import speaker as sp
from cmtts_amd.weights import import_deepspeaker, synth_deepspeaker_state_dict
from speaker_cases import (CONV_CASES, FRAME_LEN, FRAME_STEP, FS, NFFT, conv_case, conv_float32, torch_conv_same, trim_signals, utterances,
                           weights)


@pytest.mark.parametrize("k,s,H,W", [(5, 2, 6, 8), (5, 2, 5, 7), (3, 1, 5, 3)])
def test_same_conv_against_torch_float64(k, s, H, W):
    rs = np.random.RandomState(k * 100 + H)
    x = rs.standard_normal((2, H, W, 3))
    kernel, bias = rs.standard_normal((k, k, 3, 4)), rs.standard_normal(4)
    got = sp.conv2d_same(x, kernel, bias, s)
    ref = torch_conv_same(torch.from_numpy(x), torch.from_numpy(kernel), torch.from_numpy(bias), s).numpy()
    assert got.shape == ref.shape == (2, -(-H // s), -(-W // s), 4)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    if s == 2 and H % 2 == 0:
        assert sp.same_pad(H, k, s)[:2] == (1, 2)            # even size: 1 before, 2 after


@pytest.mark.parametrize("name", sorted(CONV_CASES))
def test_conv_cases_sit_on_both_clips(name):
    k, s, cin, cout, H, W, B, residual = CONV_CASES[name]
    x, kernel, bias, res, want = conv_case(name)
    assert want.shape == (B, -(-H // s), -(-W // s), cout) and (res is not None) == residual
    assert (want == 0).any() and (want == 20).any() and 0.05 <= ((want > 0) & (want < 20)).mean() <= 0.95
    assert np.abs(conv_float32(name) - want).max() < 1e-3          # the torch float32 yardstick computes the same layer


def test_network_shapes_and_unit_norm():
    sd = weights()
    win = sp.utterance_windows(utterances()[1])[1]
    assert win.shape == (1, 160, 64)
    taps = []
    f = sp.rescnn_features(sd, win[..., None], taps)
    assert [t.shape[1:] for t in taps] == [(80, 32, 64), (40, 16, 128), (20, 8, 256), (10, 4, 512)] and f.shape == (1, 10, 4, 512)
    e = sp.rescnn(sd, win)
    assert e.shape == (1, 512) and abs(np.linalg.norm(e[0]) - 1.0) < 1e-12
    # Reshape(-1, 2048): index freq * 512 + ch
    assert np.array_equal(f.reshape(1, 10, 2048)[0, 3, 2 * 512 + 7], f[0, 3, 2, 7])


def test_filterbank():
    b = sp.filter_bins(FS, NFFT)
    fb = sp.filterbank(FS, NFFT)
    assert (FRAME_LEN, FRAME_STEP, NFFT) == (551, 221, 1024)
    assert fb.shape == (64, 513) and b.size == 66 and b[0] == 0 and b[-1] == 512
    assert np.all(np.diff(b) >= 0) and np.all(fb >= 0) and fb.max() <= 1.0
    assert all(fb[j, :b[j]].sum() == 0 and fb[j, b[j + 2]:].sum() == 0 for j in range(64))


def test_frame_count_rule():
    assert sp.num_frames(551, 551, 221) == 1 and sp.num_frames(552, 551, 221) == 2
    assert sp.num_frames(551 + 221 * 162 + 1, 551, 221) == 164 and sp.num_frames(551 + 221 * 162, 551, 221) == 163
    x = np.random.RandomState(0).standard_normal(552).astype(np.float32)
    assert sp.fbank_features(x).shape == (2, 64) and sp.fbank_features(x[:551]).shape == (1, 64)
    assert sp.window_offsets(163, "all") == [0, 3] and sp.window_offsets(400, "all") == [0, 80, 160, 240] and sp.window_offsets(100, "all") == [0]
    assert sp.window_offsets(163, "center") == [1] and len(sp.window_offsets(80 * 100, "all")) == sp.MAX_WINDOWS


def test_trim_follows_numpy_percentile():
    sig = dict(trim_signals())
    for i, u in enumerate(utterances()):
        sig[f"utt{i}"] = u
    for name, x in sig.items():
        e = np.abs(x)
        idx = np.where(e > np.percentile(e, 95))[0]
        want = (int(idx[0]), int(idx[-1])) if idx.size and idx[0] != idx[-1] else (-1, -1)
        assert sp.trim_indices(x) == want, name
    assert sp.trim_indices(sig["ramp"])[0] >= 0 and sp.trim_indices(sig["ties"])[0] >= 0
    # the threshold really is interpolated between two order statistics on the ramp, and falls on tied values on "ties"
    e = np.sort(np.abs(sig["ramp"]))
    k = int(0.95 * (e.size - 1))
    assert e[k] < sp.trim_threshold(sig["ramp"]) < e[k + 1]
    e = np.sort(np.abs(sig["ties"]))
    assert e[int(0.95 * (e.size - 1))] == e[int(0.95 * (e.size - 1)) + 1] == sp.trim_threshold(sig["ties"])


def test_nothing_kept_gives_zero_frames():
    sig = trim_signals()
    for name in ("silence", "square", "two"):
        info, win = sp.utterance_windows(sig[name])
        assert info == (-1, -1, 0, 0) and win.shape[0] == 0, name
    emb = sp.speaker_embedding(weights(), [sig["silence"]])
    assert emb.shape == (1, 512) and not emb.any()


def _unpack(frag, taps, cin, cout):
    """Invert weight_pack.h: to_conv2d_fragments -> [ceil(taps cin / 16) * 16][cout]."""
    nchunk = (taps * cin + 15) // 16
    f = frag.reshape(nchunk, cout // 16, 64, 4)
    w = np.zeros((nchunk * 16, cout), np.float32)
    lane = np.arange(64)
    for j in range(4):
        for c in range(nchunk):
            for mt in range(cout // 16):
                w[16 * c + 4 * (lane >> 4) + j, 16 * mt + (lane & 15)] = f[c, mt, :, j]
    return w


@pytest.mark.parametrize("name", ["conv64-s", "res1_1_branch_2b", "conv128-s"])
def test_bn_fold_and_fragments_against_the_unfolded_layer(name):
    sd = weights()
    kernel = sd[name + "/kernel"]
    kh, kw, cin, cout = kernel.shape
    bn = np.stack([sd[name + "_bn/" + p] for p in ("gamma", "beta", "moving_mean", "moving_variance")])
    frag, bias = _lib.internal_spkenc_pack(kernel, sd[name + "/bias"], bn)
    w = _unpack(frag, kh * kw, cin, cout)
    k64, b64 = sp.fold_bn(sd, name)
    assert not w[kh * kw * cin:].any()                          # the padded tail of K is zero
    wk = w[:kh * kw * cin].reshape(kernel.shape)
    assert np.array_equal(wk, k64.astype(np.float32)) and np.array_equal(bias, b64.astype(np.float32))      # folded in double, rounded once
    # the folded layer is the unfolded float64 layer up to that one rounding
    x = np.abs(np.random.RandomState(1).standard_normal((1, 6, 5, cin)))
    stride = 2 if kh == 5 else 1
    ref = sp.conv_bn(sd, name, x, stride)
    got = sp.conv2d_same(x, wk.astype(np.float64), bias.astype(np.float64), stride)
    assert np.abs(got - ref).max() <= 4 * 2.0 ** -24 * (np.abs(x).max() * np.abs(k64).sum(axis=(0, 1, 2)).max() + np.abs(b64).max())
    # without a BatchNorm the stream holds the kernel itself
    frag0, bias0 = _lib.internal_spkenc_pack(kernel, None, None)
    assert np.array_equal(_unpack(frag0, kh * kw, cin, cout)[:kh * kw * cin].reshape(kernel.shape), kernel) and not bias0.any()
    assert np.array_equal(frag0, _lib.internal_pack_weights("conv2d_fragments", kernel.reshape(kh * kw, cin, cout)).view(np.float32))


def test_weight_names_and_import(tmp_path):
    sd = synth_deepspeaker_state_dict(2, suffix=":0")
    assert "conv64-s/kernel:0" in sd and "res3_1_branch_2b/kernel:0" in sd and sd["affine/bias:0"].shape == (512,)
    assert sd["conv64-s/kernel:0"].shape == (5, 5, 1, 64) and sd["res4_2_branch_2a_bn/moving_variance:0"].min() > 0
    assert len(sd) == 28 * 6 + 2
    plain = import_deepspeaker(sd)
    assert "conv64-s/kernel" in plain and len(plain) == len(sd)
    np.savez(tmp_path / "w.npz", **{k: v for k, v in plain.items()})
    again = import_deepspeaker(str(tmp_path / "w.npz"))
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
    del sd["affine/bias:0"]
    with pytest.raises(KeyError):
        import_deepspeaker(sd)


def test_synthetic_weights_exercise_both_clips():
    """In the float64 definition on the test windows every stage keeps between 5 % and 95 % of its activations strictly inside (0, 20), and
    the net puts activations on each clip: otherwise neither the clip nor the residual path would be exercised."""
    win = np.concatenate([sp.utterance_windows(u)[1] for u in utterances()])
    taps = []
    sp.rescnn_features(weights(), win[..., None], taps)
    for s, x in enumerate(taps):
        inside = float(((x > 0) & (x < 20)).mean())
        assert 0.05 <= inside <= 0.95, f"stage {s + 1}: {inside:.3f} inside (0, 20)"
    assert any((x == 0).any() for x in taps) and any((x == 20).any() for x in taps)
