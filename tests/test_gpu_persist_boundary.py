"""The layer boundary of the persistent denoiser stack (csrc/denoiser_persist.hip): the epilogue's row vectors through LDS, the halo entry's dp
loaded ahead of the neighbour wait, the skip sum formed in the epilogue, x' stored without a wait in front of the layer barrier.  Small shapes forced
onto the persistent path; the reference is never the kernel under test: the per-layer F(4,3) form (model option "batch_invariant",
csrc/resblock_split_w43.hip), the factors expanded first, the per-layer direct form, each bucket's uniform launch.

Shapes: (1, 64) one tile without a neighbour, (1, 65) a second tile of one frame, (2, 130) a middle tile with both neighbours, (3, 192) full tiles
only.  One residual layer: nothing is published; two: published once, the last layer's path right behind it; three: a middle layer."""
import dataclasses

import numpy as np
import pytest
import torch

from cmtts_amd import _lib
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from conftest import WINO_TRIM_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 64), (1, 65), (2, 130), (3, 192)]
_MODELS = {}


def _host():
    from cmtts_amd import host
    return host


def _model(layers, variant="VCTK", **synth):
    """One model per (variant, depth); layers = None keeps the variant's own depth."""
    key = (variant, layers, tuple(sorted(synth.items())))
    if key not in _MODELS:
        cfg = get_config(variant)
        if layers is not None:
            cfg = dataclasses.replace(cfg, res_layers=layers)
        _MODELS[key] = _host().CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=7 + (layers or 0), **synth))
    return _MODELS[key]


class _switches:
    """Process-wide switches and model options for the duration of a block; everything restored on exit."""

    def __init__(self, model, batch_invariant=None, winograd=None):
        self.model, self.bi, self.wg = model, batch_invariant, winograd

    def __enter__(self):
        lib = _lib.load()
        self.prev_p = lib.cmtts_set_persistent_denoiser(-1)
        self.prev_s = lib.cmtts_set_option(b"resblock_split", -1)
        self.prev_k = _lib.internal_set("cond_inkernel", 1)
        self.prev_bi = self.model.set_option("batch_invariant", self.bi) if self.bi is not None else None
        self.prev_wg = self.model.set_option("winograd", self.wg) if self.wg is not None else None
        return self

    def persistent(self):
        _lib.load().cmtts_set_persistent_denoiser(2)

    def per_layer(self, split=None):
        lib = _lib.load()
        lib.cmtts_set_persistent_denoiser(0)
        if split is not None:
            lib.cmtts_set_option(b"resblock_split", split)

    def __exit__(self, *exc):
        lib = _lib.load()
        if self.prev_wg is not None:
            self.model.set_option("winograd", self.prev_wg)
        if self.prev_bi is not None:
            self.model.set_option("batch_invariant", self.prev_bi)
        _lib.internal_set("cond_inkernel", self.prev_k)
        lib.cmtts_set_option(b"resblock_split", self.prev_s)
        lib.cmtts_set_persistent_denoiser(self.prev_p)


def _inputs(cfg, B, T, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 1, T, cfg.n_mels, generator=gen).to(DEV)
    cond = torch.randn(B, T, cfg.hidden, generator=gen).to(DEV)
    spk = torch.randn(B, cfg.hidden, generator=gen).to(DEV) if cfg.multi_speaker else None
    noise = torch.randn(3, B, 1, T, cfg.n_mels, generator=gen).to(DEV)
    return x, cond, spk, noise, torch.full((B,), 1095.5, device=DEV)


def _eval_and_sample(model, x, t, cond, spk, noise):
    """One network evaluation and a T = 2 sample."""
    cond_ct = cond.transpose(1, 2).contiguous()
    return model.net(x, t, cond, spk).clone(), _host().sample_with_cond(model, cond_ct, spk, 2, noise).clone()


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("B,T", SHAPES)
def test_boundary_f43_vs_per_layer_bitwise(B, T, layers):
    """The persistent F(4,3) stack against the per-layer F(4,3) form, bit for bit: one evaluation and a T = 2 sample."""
    model = _model(layers)
    x, cond, spk, noise, t = _inputs(model.config, B, T, 100 * layers + T)
    with _switches(model, batch_invariant=1) as s:
        s.persistent()
        got = _eval_and_sample(model, x, t, cond, spk, noise)
        s.per_layer(split=2)
        ref = _eval_and_sample(model, x, t, cond, spk, noise)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(a).all() and torch.equal(a, b), (i, float((a - b).abs().max()))


def _factored(model, lens, T, seed):
    """The duration net's conditioning and factors for utterances of `lens` phonemes, padded to T frames."""
    cfg = model.config
    lens = np.asarray(lens, np.int64)
    B, L = len(lens), int(lens.max())
    rs = np.random.RandomState(seed)
    texts = rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)
    texts[np.arange(L)[None, :] >= lens[:, None]] = 0
    out = model.duration_pitch_energy_net(None, torch.from_numpy(texts).to(DEV), torch.from_numpy(lens).to(DEV), max_mel_len=T)
    assert out["cond_factors"] is not None and out["cond_factors"].matches(out["cond_ct"])
    return out


@pytest.mark.parametrize("layers", [1, 2, 3, None])
def test_boundary_factors_inkernel_vs_expanded_bitwise(layers):
    """Factors gathered in-kernel against factors expanded first, bit for bit.  32, 11 and 20 phonemes of four frames in 192 frames: the second
    utterance ends in its first tile, its other two tiles are all padding frames (mel2ph = 0: the `ph > 0` select), like the last tile of the others."""
    host = _host()
    model = _model(layers, "LJSpeech", dur_frames=4.0, dur_spread=0.0)
    T = 192
    out = _factored(model, [32, 11, 20], T, 3)
    assert int(out["mel_lens"].max()) <= 128 and not out["mel2ph"][:, 128:].any(), "the last tile is meant to be padding only"
    noise = torch.randn(3, 3, 1, T, model.config.n_mels, generator=torch.Generator().manual_seed(9)).to(DEV)
    with _switches(model) as s:
        s.persistent()
        got = [host.sample_with_cond(model, out["cond_ct"], None, n, noise, factors=out["cond_factors"]).clone() for n in (1, 2)]
        _lib.internal_set("cond_inkernel", 0)
        ref = [host.sample_with_cond(model, out["cond_ct"], None, n, noise, factors=out["cond_factors"]).clone() for n in (1, 2)]
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("layers", [2, 3])
def test_boundary_back_to_back(layers):
    """The same call twice, then two different shapes one after the other on one model: nothing of a launch (row vectors, index table, z flags in LDS;
    halo granules, the residual stream's buffer in memory) reaches the next one.  Every result against the per-layer F(4,3) form, bit for bit."""
    model = _model(layers)
    order = [(2, 130), (2, 130), (1, 65), (3, 192), (2, 130)]
    data = {bt: _inputs(model.config, bt[0], bt[1], 31 * layers + bt[1]) for bt in set(order)}
    with _switches(model, batch_invariant=1) as s:
        s.per_layer(split=2)
        ref = {bt: _eval_and_sample(model, d[0], d[4], d[1], d[2], d[3]) for bt, d in data.items()}
        s.persistent()
        got = [(bt, _eval_and_sample(model, data[bt][0], data[bt][4], data[bt][1], data[bt][2], data[bt][3])) for bt in order]
    torch.cuda.synchronize()
    for i, (bt, g) in enumerate(got):
        for a, b in zip(g, ref[bt]):
            assert torch.equal(a, b), (i, bt, float((a - b).abs().max()))


def test_boundary_ragged_trimmed_shard():
    """One small ragged shard through host.sample_ragged (two buckets in ONE launch, 130 padded tiles: the smallest the one-launch form takes), an
    utterance of the 256-frame bucket trimmed to two of its four tiles: every kept frame within WINO_TRIM_TOL of its bucket's uniform launch,
    the untrimmed run of the same shard bit for bit."""
    host = _host()
    model = _model(None, "LJSpeech", dur_frames=4.0, dur_spread=0.0)
    cfg = model.config
    lens_a = [32] * 33                                # 33 x 128 frames: two full tiles each
    lens_b = [64, 20] + [48] * 14                     # 16 x 256 frames; utterance 1: 80 frames + 16 + 20 layers = 116 -> two tiles of four
    groups = []
    with _switches(model) as s:
        s.persistent()
        for lens, T, seed in ((lens_a, 128, 1), (lens_b, 256, 2)):
            out = _factored(model, lens, T, seed)
            nz = torch.randn(1, len(lens), 1, T, cfg.n_mels, generator=torch.Generator().manual_seed(seed)).to(DEV)
            ref = host.sample_with_cond(model, out["cond_ct"], None, 1, nz, factors=out["cond_factors"]).clone()
            groups.append((out, nz, ref))
        mel_lens = [g[0]["mel_lens"].tolist() for g in groups]
        assert (mel_lens[1][1] + 16 + cfg.res_layers + 63) // 64 < 4, "nothing is trimmed: the test is vacuous"
        full = host.sample_ragged(model, [(o["cond_ct"], None, nz, None, o["cond_factors"]) for o, nz, _ in groups], 1)
        trim = host.sample_ragged(model, [(o["cond_ct"], None, nz, ml, o["cond_factors"]) for (o, nz, _), ml in zip(groups, mel_lens)], 1, tail_frames=16)
    host.synchronize()
    for gi, (_, _, ref) in enumerate(groups):
        assert torch.isfinite(ref).all() and torch.equal(full[gi], ref), (gi, float((full[gi] - ref).abs().max()))
        for b, n in enumerate(mel_lens[gi]):
            keep = min(n + 16, ref.shape[1])
            d = float((trim[gi][b, :keep] - ref[b, :keep]).abs().max())
            assert d <= WINO_TRIM_TOL, (gi, b, n, d)
    cut = (mel_lens[1][1] + 16 + cfg.res_layers + 63) // 64 * 64
    assert not trim[1][1, cut:].any()                 # the trimmed tiles were not computed


def test_boundary_direct_form_bitwise():
    """winograd = 0 at (2, 130): the persistent direct form against the per-layer kernels, bit for bit — the pieces in the code it shares with the
    Winograd instances have not changed it."""
    model = _model(3)
    x, cond, spk, noise, t = _inputs(model.config, 2, 130, 5)
    with _switches(model, winograd=0) as s:
        s.persistent()
        got = _eval_and_sample(model, x, t, cond, spk, noise)
        s.per_layer()
        ref = _eval_and_sample(model, x, t, cond, spk, noise)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())
