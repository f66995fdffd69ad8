"""Seeded per-utterance sampler noise on the device (csrc/noise_philox.hip): the kernel against the numpy statement of the definition
(cmtts_amd/noise.py), the pure-function property in every launch shape, the seeded sampler against the sampler on a noise tensor, and
what it buys end to end — one request (conditioning, seed) gives one mel and one PCM whatever it is batched with."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmtts_amd import _lib, noise as N
from cmtts_amd.config import get_config, HifiGanConfig
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict
from conftest import report, same_pcm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP = 256
_MODELS = {}
SEEDS = np.asarray([0, -1, -(1 << 63) + 12345, 0x0123456789ABCDEF], np.int64)          # 0, all ones, bit 63 set, ordinary


def _host():
    from cmtts_amd import host
    return host


def _model(variant):
    if variant not in _MODELS:
        cfg = get_config(variant)
        _MODELS[variant] = _host().CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=5))
    return _MODELS[variant]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _moment_z(z):
    z = np.asarray(z, np.float64).reshape(-1)
    n = z.size
    return np.sqrt(n) * z.mean(), np.sqrt(2 * n) * (z.std() - 1.0), ((z ** 4).mean() - 3.0) / np.sqrt(96.0 / n)


@pytest.mark.parametrize("M", [80, 6])
@pytest.mark.parametrize("t0", [0, 1000])
def test_bits(M, t0):
    """The raw Philox blocks (internal hook) equal noise.reference_bits bit for bit."""
    T, nd, B = 37, 5, len(SEEDS)
    Q = (M + 3) // 4
    sd = torch.from_numpy(SEEDS).to(DEV)
    bits = torch.zeros(nd, B, T, Q, 4, dtype=torch.int32, device=DEV)
    assert _lib.internal_noise_bits(C.c_void_p(sd.data_ptr()), B, T, M, 0, nd, t0, C.c_void_p(bits.data_ptr()), _stream()) == 0
    torch.cuda.synchronize()
    got = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, N.reference_bits(SEEDS, nd, T, M, 0, t0))


@pytest.mark.parametrize("M", [80, 6])
@pytest.mark.parametrize("T,t0", [(37, 0), (37, 1000), (1, 0)])
def test_normals(M, T, t0):
    """cmtts_noise_fill against the float64 normals of the same bits.  Bound (derived, not measured): r <= 5.77 times the fp32 rounding of
    the argument 2 pi u2 (<= 2.4e-7), plus a few ulp of logf / sqrtf / sincospif and the product's rounding: ~4e-6; 2.5 x that."""
    host = _host()
    z = host.seeded_noise(SEEDS, 5, T, M, DEV, t0=t0)
    torch.cuda.synchronize()
    assert z.shape == (5, len(SEEDS), 1, T, M) and z.dtype == torch.float32
    got = z.cpu().numpy().astype(np.float64)
    ref = N.reference_normals(SEEDS, 5, T, M, 0, t0)
    err = float(np.abs(got - ref).max())
    report(f"NOISE normals M={M} T={T} t0={t0}: max|device - float64| {err:.2e} (bound 1e-5), max|z| {np.abs(got).max():.3f}")
    assert np.isfinite(got).all()
    assert np.abs(got).max() <= 5.78
    assert err <= 1e-5


def test_pure_function_bitwise():
    host = _host()
    seeds = N.utterance_seeds(11, np.arange(40))
    big = host.seeded_noise(seeds, 5, 200, 80, DEV)
    assert big.shape == (5, 40, 1, 200, 80)
    for b in (0, 17, 39):          # a row = the B = 1 fill of its seed
        assert torch.equal(big[:, b:b + 1], host.seeded_noise(seeds[b:b + 1], 5, 200, 80, DEV)), b
    long = host.seeded_noise(seeds, 5, 512, 80, DEV)          # T = 200 = the first 200 frames of T = 512
    assert torch.equal(big, long[:, :, :, :200])
    assert torch.equal(host.seeded_noise(seeds, 5, 136, 80, DEV, t0=64), big[:, :, :, 64:])          # a window = the slice
    assert torch.equal(host.seeded_noise(seeds, 3, 200, 80, DEV, first_draw=2), big[2:5])          # draws 2..4
    perm = np.random.RandomState(0).permutation(40)
    assert torch.equal(host.seeded_noise(seeds[perm], 5, 200, 80, DEV), big[:, torch.from_numpy(perm).to(DEV)])
    # the element-store form (n_mels not a multiple of 4, or a tensor that is not 16-byte aligned) writes the same values
    z6 = host.seeded_noise(seeds[:3], 2, 9, 6, DEV)
    z8 = host.seeded_noise(seeds[:3], 2, 9, 8, DEV)
    assert torch.equal(z6[..., :4], z8[..., :4])          # block 0 of every row; block 1 differs in nothing but the cut
    assert torch.equal(z6[..., 4:], z8[..., 4:6])
    lib = _lib.load()
    buf = torch.zeros(2 * 3 * 9 * 80 + 1, device=DEV)
    sd = torch.from_numpy(seeds[:3]).to(DEV)
    _lib.check(lib.cmtts_noise_fill(sd.data_ptr(), 3, 9, 80, 0, 2, 0, buf.data_ptr() + 4, _stream()))
    assert torch.equal(buf[1:].view(2, 3, 1, 9, 80), host.seeded_noise(seeds[:3], 2, 9, 80, DEV))
    # the groups launch = per-group fills
    shapes = [(3, 64), (7, 200), (1, 37)]
    gs = [(N.utterance_seeds(5 + k, np.arange(B)), T) for k, (B, T) in enumerate(shapes)]
    outs = host.seeded_noise_groups(gs, 5, 80, DEV)
    for (sv, T), o in zip(gs, outs):
        assert torch.equal(o, host.seeded_noise(sv, 5, T, 80, DEV)), T
    many = [(N.utterance_seeds(k, np.arange(2)), 5 + k) for k in range(35)]          # more groups than one launch's table holds
    for (sv, T), o in zip(many, host.seeded_noise_groups(many, 2, 80, DEV, first_draw=1)):
        assert torch.equal(o, host.seeded_noise(sv, 2, T, 80, DEV, first_draw=1)), T


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_moments_device(seed):
    host = _host()
    z = host.seeded_noise(N.utterance_seeds(seed, np.arange(8)), 5, 512, 80, DEV).cpu().numpy().astype(np.float64)
    zs = _moment_z(z)
    n = z[0, 0].size
    a, b, c = z[0, 0].reshape(-1), z[1, 0].reshape(-1), z[0, 1].reshape(-1)
    r_draw = float(np.corrcoef(a, b)[0, 1]) * np.sqrt(n)
    r_seed = float(np.corrcoef(a, c)[0, 1]) * np.sqrt(n)
    report(f"NOISE moments (device), seed {seed}: z(mean) {zs[0]:+.2f} z(sd) {zs[1]:+.2f} z(m4) {zs[2]:+.2f}; "
           f"r sqrt(n): two draws {r_draw:+.2f}, two seeds {r_seed:+.2f}")
    assert all(abs(v) <= 4 for v in zs), zs
    assert abs(r_draw) <= 4 and abs(r_seed) <= 4


def _cond(variant, B, T, with_factors, seed):
    """Conditioning of a (B, T) batch: from the duration net (with its factors) or random."""
    model = _model(variant)
    cfg = model.config
    g = torch.Generator().manual_seed(seed)
    if with_factors:
        L = 22
        rs = np.random.RandomState(seed)
        texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)).to(DEV)
        lens = torch.full((B,), L, dtype=torch.int64, device=DEV)
        spk = torch.randn(B, cfg.external_speaker_dim, generator=g).to(DEV) if cfg.multi_speaker else None
        out = model.duration_pitch_energy_net(None, texts, lens, spker_embeds=spk)
        return model, out["cond_ct"], out["speaker_emb"], out["cond_factors"]
    cond_ct = torch.randn(B, cfg.hidden, T, generator=g).to(DEV)
    spk = torch.randn(B, cfg.hidden, generator=g).to(DEV) if cfg.multi_speaker else None
    return model, cond_ct, spk, None


@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
@pytest.mark.parametrize("with_factors", [False, True])
@pytest.mark.parametrize("B", [1, 40])
def test_seeded_sampler_bitwise(variant, with_factors, B):
    """cmtts_sample_seeded = cmtts_sample_factored_t on seeded_noise(...), bit for bit, at the default stack form."""
    host = _host()
    model, cond_ct, spk, f = _cond(variant, B, 130, with_factors, 100 + B)
    T = cond_ct.shape[2]
    seeds = N.utterance_seeds(21, np.arange(B))
    for n_steps in (1, 2, 4):
        noise = host.seeded_noise(seeds, 1 if n_steps == 1 else n_steps + 1, T, model.config.n_mels, DEV)
        ref = host.sample_with_cond(model, cond_ct, spk, n_steps, noise, factors=f).clone()
        got = host.sample_with_cond(model, cond_ct, spk, n_steps, factors=f, seeds=seeds).clone()
        again = host.sample_with_cond(model, cond_ct, spk, n_steps, factors=f, seeds=torch.from_numpy(seeds)).clone()
        host.synchronize()
        assert torch.isfinite(ref).all()
        assert torch.equal(got, ref), (n_steps, float((got - ref).abs().max()))
        assert torch.equal(again, ref), n_steps
    with pytest.raises(ValueError):
        host.sample_with_cond(model, cond_ct, spk, 1)
    with pytest.raises(ValueError):
        host.sample_with_cond(model, cond_ct, spk, 1, seeds=seeds[: B - 1] if B > 1 else np.zeros(2, np.int64))


@pytest.mark.parametrize("variant", ["LJSpeech", "VCTK"])
def test_request_determinism(variant):
    """Both batch_invariant options at 1: utterance 17 of a B = 40, T = 200 batch through sample_with_cond(seeds=...) has the mel bits and the
    PCM bits of the same utterance alone with its seed (same conditioning, same padded T).  With torch noise drawn for the two batch
    shapes the mels differ."""
    host = _host()
    B, T, b = 40, 200, 17
    model, cond_ct, spk, _ = _cond(variant, B, T, False, 7)
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    seeds = N.utterance_seeds(99, np.arange(B))
    sl = slice(b, b + 1)
    cond1 = cond_ct[sl].contiguous()
    spk1 = spk[sl].contiguous() if spk is not None else None
    prev_m, prev_v = model.set_option("batch_invariant", 1), voc.set_option("batch_invariant", 1)
    try:
        mel_b = host.sample_with_cond(model, cond_ct, spk, 4, seeds=seeds).clone()
        mel_1 = host.sample_with_cond(model, cond1, spk1, 4, seeds=seeds[sl]).clone()
        pcm_b = host.vocoder_infer(mel_b.transpose(1, 2), voc)
        pcm_1 = host.vocoder_infer(mel_1.transpose(1, 2), voc)
        tn_b = torch.randn(5, B, 1, T, 80, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
        tn_1 = torch.randn(5, 1, 1, T, 80, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
        ctl_b = host.sample_with_cond(model, cond_ct, spk, 4, tn_b).clone()
        ctl_1 = host.sample_with_cond(model, cond1, spk1, 4, tn_1).clone()
    finally:
        model.set_option("batch_invariant", prev_m)
        voc.set_option("batch_invariant", prev_v)
    host.synchronize()
    assert torch.isfinite(mel_b).all()
    assert torch.equal(mel_1[0], mel_b[b]), float((mel_1[0] - mel_b[b]).abs().max())
    assert np.array_equal(np.asarray(pcm_1[0]), np.asarray(pcm_b[b]))
    assert not torch.equal(ctl_1[0], ctl_b[b])


def _text_batch(cfg, B, L, seed, lo):
    rs = np.random.RandomState(seed)
    src = rs.randint(lo, L + 1, size=B)
    src[rs.randint(B)] = L
    texts = np.zeros((B, L), np.int64)
    for i, s in enumerate(src):
        texts[i, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32)
    return torch.from_numpy(texts), torch.from_numpy(src.astype(np.int64)), torch.from_numpy(spk)


def test_sharded_order_independent():
    """synthesize_sharded, one rank, batch_invariant 1: a batch and its permutation, seeds permuted alike, give the same mel bits per
    utterance; with seeds=None (noise keyed by position) they do not."""
    host = _host()
    cfg = get_config("LibriTTS")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=9, dur_frames=4.0, dur_spread=0.0))
    B = 24
    texts, src, spk = _text_batch(cfg, B, 40, seed=3, lo=5)
    buckets = (64, 128, 256)
    seeds = N.utterance_seeds(2024, np.arange(B))
    perm = np.random.RandomState(1).permutation(B)
    pt = torch.from_numpy(perm)
    prev = model.set_option("batch_invariant", 1)
    try:
        a = host.synthesize_sharded(model, texts, src, spker_embeds=spk, n_steps=4, buckets=buckets, seeds=seeds)
        p = host.synthesize_sharded(model, texts[pt], src[pt], spker_embeds=spk[pt], n_steps=4, buckets=buckets, seeds=seeds[perm])
        a0 = host.synthesize_sharded(model, texts, src, spker_embeds=spk, n_steps=4, buckets=buckets, seed=5)
        p0 = host.synthesize_sharded(model, texts[pt], src[pt], spker_embeds=spk[pt], n_steps=4, buckets=buckets, seed=5)
        c = host.synthesize_sharded(model, texts, src, spker_embeds=spk, n_steps=4, buckets=buckets, seeds=2024)
    finally:
        model.set_option("batch_invariant", prev)
    host.synchronize()
    assert len(a["plan"]) >= 2, a["plan"]          # predicted lengths over at least two buckets
    assert [a["mel_len"][int(i)] for i in perm] == list(p["mel_len"])
    diff = []
    for k, i in enumerate(perm):
        x, y = a["mels"][int(i)], p["mels"][k]
        assert x.shape == y.shape and bool(torch.isfinite(x).all())
        if not torch.equal(x, y):
            diff.append((int(i), k, float((x - y).abs().max())))
    assert not diff, diff
    assert any(not torch.equal(a0["mels"][int(i)], p0["mels"][k]) for k, i in enumerate(perm))
    assert all(torch.equal(x, y) for x, y in zip(a["mels"], c["mels"]))          # one int = utterance_seeds(int, arange(B))


def _stitch(chunks, lens):
    out = [np.zeros(n * HOP, np.int16) for n in lens]
    done = [0] * len(lens)
    for b, off, pcm, is_last in chunks:
        out[b][off:off + len(pcm)] = pcm
        done[b] += len(pcm)
    assert done == [n * HOP for n in lens]
    return out


def test_stream_seeded(voc_form):
    """synthesize_stream(seeds=...) chunk by chunk = vocoder_infer of synthesize(seeds=...)'s mel."""
    host = _host()
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=2, dur_frames=5.0, dur_spread=0.3))
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=3))
    B, L = 3, 14
    texts, src, spk = _text_batch(cfg, B, L, seed=2, lo=5)
    seeds = N.utterance_seeds(8, np.arange(B))
    res = host.CMTotalTTSSynthesize.from_model(model, T=4).synthesize((None, None, None, texts, src, L, spk), seeds=seeds)
    lens = res[11].cpu().tolist()
    ref = host.vocoder_infer(res[0].transpose(1, 2), voc, lengths=[n * HOP for n in lens])
    got = _stitch(host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=4, chunk_frames=(8, 16), seeds=seeds), lens)
    assert max(lens) > 8
    for b in range(B):
        assert same_pcm(got[b], ref[b], voc_form), b
    with pytest.raises(ValueError):
        next(host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=4, seeds=seeds, noise=torch.zeros(1)))


def test_generator_surface():
    host = _host()
    B, T = 6, 50
    gen = host.get_generator("determ-indiv", 100, 3)
    x = gen.randn(B, 1, T, 80, device=DEV)
    y = gen.randn_like(x)
    ids = np.arange(B)
    assert x.shape == (B, 1, T, 80) and x.device.type == "cuda"
    assert torch.equal(x, host.seeded_noise(N.utterance_seeds(3, ids), 1, T, 80, DEV)[0])
    assert torch.equal(y, host.seeded_noise(N.utterance_seeds(3, ids), 1, T, 80, DEV, first_draw=1)[0])          # randn_like: the next draw
    gen.set_done_samples(97)          # moves the ids (clamped to num_samples - 1) and restarts the draws
    z = gen.randn(B, 1, T, 80, device=DEV)
    assert torch.equal(z, host.seeded_noise(N.utterance_seeds(3, [97, 98, 99, 99, 99, 99]), 1, T, 80, DEV)[0])
    with pytest.raises(NotImplementedError):
        gen.randn(B, 2, T, 80, device=DEV)
    # CMTotalTTSSynthesize with the generator = the explicit seeds= call; all draws in one fill = call-by-call draws
    cfg = get_config("VCTK")
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=2, dur_frames=5.0, dur_spread=0.3))
    texts, src, spk = _text_batch(cfg, 3, 14, seed=2, lo=5)
    batch = (None, None, None, texts, src, 14, spk)
    for steps in (1, 4):
        g = host.get_generator("determ-indiv", 100, 3)
        a = host.CMTotalTTSSynthesize.from_model(model, T=steps, generator=g).synthesize(batch)[0].clone()
        b = host.CMTotalTTSSynthesize.from_model(model, T=steps).synthesize(batch, seeds=N.utterance_seeds(3, np.arange(3)))[0].clone()
        assert g.draw == (1 if steps == 1 else steps + 1)
        host.synchronize()
        assert torch.isfinite(a).all() and torch.equal(a, b), steps

        class CallByCall:          # the same generator behind the plain randn / randn_like surface
            def __init__(self):
                self.g = host.get_generator("determ-indiv", 100, 3)

            def randn(self, *a, **k):
                return self.g.randn(*a, **k)

            def randn_like(self, t):
                return self.g.randn_like(t)
        c = host.CMTotalTTSSynthesize.from_model(model, T=steps, generator=CallByCall()).synthesize(batch)[0].clone()
        host.synchronize()
        assert torch.equal(c, a), steps
