"""Per-utterance and per-phoneme prosody controls on the GPU (include/cmtts_hip.h: cmtts_set_control_tables; the table forms of the
duration, energy and pitch kernels): a constant table against the scalar control and a per-utterance vector against the utterance
alone, both bit for bit; per-phoneme tables against the numpy oracle; the pitch rows inside text-state records across virtual
worlds; streamed PCM with per-utterance vectors."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib, shard
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from conftest import FLIP_MARGIN, load_golden, pitch_margin_mask, report
from oracle import cmtts_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_STEPS = 4


def _host():
    from cmtts_amd import host
    return host


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def fixture():
    """Model and inputs of tests/test_oracle_golden.py::_setup(golden, "VCTK"): B = 3, L = 20, src_lens 20 / 14 / 9."""
    g = load_golden("cmtts_VCTK")
    cfg = get_config("VCTK")
    sd = synth_cmtts_state_dict(cfg, seed=int(g["seed"]), dur_frames=4.0, dur_spread=0.03)
    model = _host().CMTotalTTS(cfg, DEV).load_state_dict(sd)
    return g, cfg, sd, model


def _batch(cfg, B, L, seed):
    rs = np.random.RandomState(seed)
    src = rs.randint(max(1, L // 3), L + 1, size=B)
    src[rs.randint(B)] = L
    texts = np.zeros((B, L), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32)
    return torch.from_numpy(texts), torch.from_numpy(src.astype(np.int64)), torch.from_numpy(spk)


def _run(model, texts, src, spk, noise_seed, max_mel_len=None, **ctl):
    """Text side, frame side and the 4-step mel -> every returned array (numpy)."""
    host = _host()
    out = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, max_mel_len=max_mel_len, **ctl)
    B, T, _ = out["cond"].shape
    noise = torch.randn(N_STEPS + 1, B, 1, T, model.config.n_mels, generator=torch.Generator().manual_seed(noise_seed)).to(DEV)
    mel = host.sample_with_cond(model, out["cond_ct"], out["speaker_emb"], N_STEPS, noise, factors=out.get("cond_factors"))
    torch.cuda.synchronize()
    pp = out["p_predictions"]
    return {"log_d": _np(out["log_d_predictions"]), "d_rounded": _np(out["d_rounded"]), "mel_len": _np(out["mel_lens"]),
            "e_pred": _np(out["e_predictions"]), "e_idx": _np(out["e_idx"]), "mel2ph": _np(out["mel2ph"]), "cwt_out": _np(pp["cwt"]),
            "f0_denorm": _np(pp["f0_denorm"]), "p_idx": _np(pp["p_idx"]), "f0_mean": _np(pp["f0_mean"]), "f0_std": _np(pp["f0_std"]),
            "cond": _np(out["cond"]), "speaker_emb": _np(out["speaker_emb"]), "enc_out": _np(out["enc_out"]), "mel": _np(mel)}


def _shapes(fixture):
    g, cfg, _, _ = fixture
    yield "3x20", (torch.from_numpy(g["texts"]), torch.from_numpy(g["src_lens"]), torch.from_numpy(g["spker_embeds"])), None
    yield "32x85", _batch(cfg, 32, 85, seed=85), 512


# ---- 5. a table that holds one value is the scalar: the same multiply on the same operands

def test_constant_table_equals_scalar_bitwise(fixture):
    model = fixture[3]
    p, e, d = 1.3, 0.8, 1.25
    for tag, (texts, src, spk), T in _shapes(fixture):
        B, L = texts.shape
        ref = _run(model, texts, src, spk, 7, T, p_control=p, e_control=e, d_control=d)
        full = lambda v: torch.full((B, L), v, dtype=torch.float32)
        vec = lambda v: torch.full((B,), v, dtype=torch.float32)
        for form, kw in (("[B, L]", dict(p_control=full(p), e_control=full(e), d_control=full(d))),
                         ("[B]", dict(p_control=vec(p), e_control=vec(e), d_control=vec(d))),
                         ("mixed", dict(p_control=full(p).to(DEV), e_control=e, d_control=vec(d)))):
            got = _run(model, texts, src, spk, 7, T, **kw)
            for k in ref:
                assert np.array_equal(got[k], ref[k]), (tag, form, k)
        # ... and the tables do not stick: a plain call afterwards is the plain call
        plain = _run(model, texts, src, spk, 7, T)
        assert not np.array_equal(plain["d_rounded"], ref["d_rounded"])
        again = _run(model, texts, src, spk, 7, T)
        for k in plain:
            assert np.array_equal(plain[k], again[k]), (tag, k)


# ---- 6. an utterance with its own factors inside a batch is the utterance with those factors as the batch's scalars

def test_per_utterance_equals_alone_bitwise(fixture):
    g, cfg, _, model = fixture
    cases = [("3x20", (torch.from_numpy(g["texts"]), torch.from_numpy(g["src_lens"]), torch.from_numpy(g["spker_embeds"])), 256,
              (0.8, 1.0, 1.3), (1.2, 0.7, 1.0), (0.75, 1.0, 1.5))]
    rs = np.random.RandomState(6)
    B2 = 6
    cases.append(("6x33", _batch(cfg, B2, 33, seed=33), 512, tuple(rs.uniform(0.7, 1.4, B2).round(2)),
                  tuple(rs.uniform(0.5, 1.5, B2).round(2)), tuple(rs.uniform(0.5, 2.0, B2).round(2))))
    frame_keys = ("mel2ph", "cwt_out", "f0_denorm", "p_idx", "cond", "mel")
    for tag, (texts, src, spk), T, P, E, D in cases:
        B = texts.shape[0]
        t32 = lambda v: torch.tensor(v, dtype=torch.float32)
        got = _run(model, texts, src, spk, 11, T, p_control=t32(P), e_control=t32(E), d_control=t32(D))
        assert got["mel_len"].min() < T and len(set(got["mel_len"].tolist())) > 1          # padding frames exist
        for b in range(B):
            one = _run(model, texts, src, spk, 11, T, p_control=float(np.float32(P[b])), e_control=float(np.float32(E[b])),
                       d_control=float(np.float32(D[b])))
            assert got["mel_len"][b] == one["mel_len"][b]
            n = min(int(one["mel_len"][b]), T)
            for k in ("log_d", "d_rounded", "e_pred", "e_idx"):
                assert np.array_equal(got[k][b], one[k][b]), (tag, b, k)
            for k in frame_keys:
                assert np.array_equal(got[k][b, :n], one[k][b, :n]), (tag, b, k)
            # the padding frames too: they take the factor of the utterance's last frame, a constant row's value
            for k in ("cwt_out", "f0_denorm", "p_idx"):
                assert np.array_equal(got[k][b], one[k][b]), (tag, b, k, "padding")


# ---- 7. per-phoneme tables against the oracle

def _frame_factors(P, d_rounded, T):
    """The [B, T, 1] pitch factors of the oracle: phoneme l repeated int(d_rounded[b, l]) times; a padding frame takes the factor of
    the utterance's last frame (include/cmtts_hip.h, cmtts_set_control_tables)."""
    B = P.shape[0]
    pf = np.ones((B, T, 1), np.float32)
    for b in range(B):
        rep = np.repeat(P[b], d_rounded[b].astype(np.int64))
        pf[b, :len(rep), 0] = rep
        if len(rep):
            pf[b, len(rep):, 0] = rep[-1]
    return pf


@pytest.mark.parametrize("seed", [0])
def test_per_phoneme_against_oracle(fixture, seed):
    """Seed-0 tables D ~ U(0.5, 2), E ~ U(0.5, 1.5), P ~ U(0.7, 1.4) on the 3 x 20 fixture.  The integer stages must be exact: the
    duration factor multiplies an integer-valued float on both sides, and the closest a scaled energy comes to a bucket edge (3.2e-4)
    is more than the e_pred tolerance times the largest factor (1.5e-4).  The float outputs take the tolerances the scalar controls
    are held to (tests/test_gpu_parity.py::_check_variance_gpu), times the largest factor where the quantity is multiplied.  The
    oracle has no frame within FLIP_MARGIN of a pitch-bucket boundary on this fixture, so 0 pitch buckets are expected to differ."""
    g, cfg, sd, model = fixture
    texts, src, spk = g["texts"], g["src_lens"], g["spker_embeds"]
    B, L = texts.shape
    rs = np.random.RandomState(seed)
    D = rs.uniform(0.5, 2.0, size=(B, L)).astype(np.float32)
    E = rs.uniform(0.5, 1.5, size=(B, L)).astype(np.float32)
    P = rs.uniform(0.7, 1.4, size=(B, L)).astype(np.float32)
    first = O.duration_pitch_speaker_net(sd, cfg, texts, src, spk, e_control=E, d_control=D)
    T = int(first["mel_len"].max())
    assert first["mel_len"].tolist() == [111, 80, 156] and T == 156
    ref = O.duration_pitch_speaker_net(sd, cfg, texts, src, spk, max_mel_len=T, e_control=E, d_control=D,
                                       p_control=_frame_factors(P, first["d_rounded"], T))
    got = _run(model, torch.from_numpy(texts), torch.from_numpy(src), torch.from_numpy(spk), 3,
               p_control=torch.from_numpy(P), e_control=torch.from_numpy(E), d_control=torch.from_numpy(D))
    valid_l = np.arange(L)[None, :] < src[:, None]
    valid_t = np.arange(T)[None, :] < ref["mel_len"][:, None]
    err = lambda a, b: float(np.abs(a - b).max())
    same = got["p_idx"] == ref["p_idx"]
    n_diff = int((~same & valid_t).sum())
    report(f"CONTROL_TABLES seed {seed}: |dlog_d| {err(got['log_d'], ref['log_d']):.2e} |de_pred| {err(got['e_pred'], ref['e_pred']):.2e} "
           f"|dcwt| {err(got['cwt_out'], ref['cwt_out']):.2e} |df0| {err(got['f0_denorm'], ref['f0_denorm']):.2e} "
           f"pitch buckets differing {n_diff}/{int(valid_t.sum())} |dcond| {float(np.abs(got['cond'] - ref['cond'])[same].max()):.2e}")
    np.testing.assert_array_equal(got["d_rounded"][valid_l], ref["d_rounded"][valid_l])
    np.testing.assert_array_equal(got["mel_len"], ref["mel_len"])
    # mel2ph follows the INTEGER parts of the durations, like the length regulator (a non-integer factor leaves d_rounded fractional,
    # and the oracle's dur_to_mel2ph accumulates the fractions, which nothing downstream reads)
    for b in range(B):
        want = np.zeros(T, np.int64)
        rep = np.repeat(np.arange(1, L + 1), ref["d_rounded"][b].astype(np.int64))
        want[:len(rep)] = rep
        np.testing.assert_array_equal(got["mel2ph"][b], want)
    np.testing.assert_array_equal(got["e_idx"][valid_l], ref["e_idx"][valid_l])
    np.testing.assert_allclose(got["log_d"], ref["log_d"], atol=5e-5)
    np.testing.assert_allclose(got["e_pred"], ref["e_pred"], atol=1e-4 * float(E.max()))
    np.testing.assert_allclose(got["cwt_out"], ref["cwt_out"], atol=3e-4 * float(P.max()))
    np.testing.assert_allclose(got["f0_denorm"], ref["f0_denorm"], rtol=3e-4, atol=2e-3)
    # pitch buckets: a differing frame sits on a bucket boundary of the oracle's f0 and is one bucket off; at most 1 % of the frames
    on_boundary = ~pitch_margin_mask(ref["f0_denorm"], FLIP_MARGIN)
    assert not (~same & ~on_boundary).any(), "a pitch bucket differs away from a rounding boundary"
    assert (np.abs(got["p_idx"] - ref["p_idx"]) <= 1).all()
    assert n_diff <= 0.01 * valid_t.sum()
    assert float(np.abs(got["cond"] - ref["cond"])[same].max()) < 1e-3


# ---- 8. the pitch rows travel inside the text-state records

def _stream():
    return torch.cuda.current_stream().cuda_stream


def _virtual_world(model, texts, src, spk, world, buckets, ctl):
    """synthesize_sharded's per-rank body for every rank of `world`, one after the other on this GPU (tests/test_gpu_text_state.py)."""
    host = _host()
    n, L_all = texts.shape[0], int(src.max())
    recs, lens = [], []
    for r in range(world):
        lo, hi = shard.shard_range(n, r, world)
        rec, ml = host.text_state_records(model, texts, src, lo, hi, spker_embeds=spk, **ctl)
        recs.append(rec)
        lens.append(ml)
    records = torch.cat(recs)
    mel_len = torch.cat(lens).tolist()
    planned, _ = shard.planned_lengths(mel_len, buckets)
    plan = shard.plan_shards(planned, world, buckets)
    slots, need = shard.route_records(plan, n, world)
    res = {"records": records, "mel_len": mel_len, "mel2ph": [None] * n, "cwt": [None] * n, "p_idx": [None] * n, "mels": [None] * n}
    for r in range(world):
        recv = records.index_select(0, torch.tensor(need[r], device=DEV))
        row = {i: k for k, i in enumerate(need[r])}
        groups = [(b, recv.index_select(0, torch.tensor([row[i] for i in slots[b][r]], device=DEV)), slots[b][r],
                   [planned[i] for i in slots[b][r]]) for b in sorted(slots)]
        det = []
        outs = host.frame_side_from_records(model, groups, L_all, N_STEPS, 5, details=det, p_control=ctl.get("p_control", 1.0))
        for (b, _, ids, _), (mel, _), d in zip(groups, outs, det):
            for k, i in enumerate(plan[b][r]):
                if i >= 0:
                    res["mel2ph"][i], res["cwt"][i], res["p_idx"][i] = d["mel2ph"][k].clone(), d["cwt"][k].clone(), d["p_idx"][k].clone()
                    res["mels"][i] = mel[k, :planned[i]].clone()
    torch.cuda.synchronize()
    return res


def test_sharded_pitch_rows_travel_with_the_utterance(fixture):
    _, cfg, _, model = fixture
    host, lib = _host(), model.lib
    n, L = 24, 32
    texts, src, spk = _batch(cfg, n, L, seed=40)
    assert int(src.max()) == L
    buckets = (128, 256, 512)
    rs = np.random.RandomState(8)
    ctl = {"d_control": torch.from_numpy(rs.uniform(0.4, 1.2, size=n).astype(np.float32)),
           "e_control": torch.from_numpy(rs.uniform(0.5, 1.5, size=(n, L)).astype(np.float32)),
           "p_control": torch.from_numpy(rs.uniform(0.7, 1.4, size=(n, L)).astype(np.float32))}
    ref = _virtual_world(model, texts, src, spk, 1, buckets, ctl)
    lay = shard.text_state_layout(cfg.hidden, cfg.cwt_hidden, L, with_p=True)
    assert ref["records"].shape[1] == lay["record_bytes"]
    h = shard.text_state_header(ref["records"])
    assert (h["layout"] == shard.TEXT_STATE_LAYOUT_P).all() and h["index"].tolist() == list(range(n))
    assert torch.equal(shard.text_state_region(ref["records"], lay, "pctl").cpu(), ctl["p_control"])
    plain = _virtual_world(model, texts, src, spk, 1, buckets, {})
    assert plain["mel_len"] != ref["mel_len"]
    for world in (2, 4):
        got = _virtual_world(model, texts, src, spk, world, buckets, ctl)
        assert torch.equal(got["records"], ref["records"]) and got["mel_len"] == ref["mel_len"]
        for i in range(n):
            for k in ("mel2ph", "cwt", "p_idx", "mels"):
                assert torch.equal(got[k][i], ref[k][i]), (world, i, k)
    # the whole path: synthesize_sharded (one rank) gives the virtual worlds' mels
    out = host.synthesize_sharded(model, texts, src, spker_embeds=spk, n_steps=N_STEPS, seed=5, buckets=buckets, **ctl)
    assert out["mel_len"] == ref["mel_len"]
    for i in range(n):
        assert torch.equal(out["mels"][i], ref["mels"][i]), i
    # without a pitch table a record is the revision-1 record: its size, its layout word and its bytes, whatever else is installed
    lay1 = shard.text_state_layout(cfg.hidden, cfg.cwt_hidden, L)
    no_p = {k: v for k, v in ctl.items() if k != "p_control"}
    rec_de, _ = host.text_state_records(model, texts, src, 0, n, spker_embeds=spk, **no_p)
    assert rec_de.shape[1] == lay1["record_bytes"] == lib.cmtts_text_state_record_bytes(model._h, L)
    h = shard.text_state_header(rec_de)
    assert (h["layout"] == shard.TEXT_STATE_LAYOUT).all()
    assert (rec_de[:, 36:40].contiguous().view(torch.int32) == 4).all()          # n_regions
    # ... and the revision-2 record of the same text side is that record + the row (header words layout / n_regions aside)
    rec_p = ref["records"]
    body = slice(shard.TEXT_STATE_HEADER_BYTES, lay1["record_bytes"])
    assert torch.equal(rec_p[:, body], rec_de[:, body])
    assert torch.equal(rec_p[:, :20], rec_de[:, :20]) and torch.equal(rec_p[:, 24:36], rec_de[:, 24:36])
    assert (rec_p[:, 36:40].contiguous().view(torch.int32) == 5).all() and torch.equal(rec_p[:, 40:64], rec_de[:, 40:64])
    # plain records (no tables at all) against a pack through the C ABI with nothing installed: byte for byte
    rec_plain, _ = host.text_state_records(model, texts, src, 0, n, spker_embeds=spk)
    assert torch.equal(rec_plain, plain["records"]) and rec_plain.shape[1] == lay1["record_bytes"]


def test_c_abi_refuses_table_with_scalar(fixture):
    g, cfg, _, model = fixture
    lib = model.lib
    texts, src, spk = (torch.from_numpy(g[k]).to(DEV) for k in ("texts", "src_lens", "spker_embeds"))
    B, L = texts.shape
    tab = torch.ones(B, L, device=DEV)
    nb = lib.cmtts_text_workspace_bytes(model._h, B, L)
    tws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    call = lambda d, Lc=L: lib.cmtts_text_forward(model._h, texts.data_ptr(), src.data_ptr(), spk.data_ptr(), None, B, Lc, d, None, None, None,
                                                  None, None, None, None, tws.data_ptr(), nb, _stream())
    ct = _lib.ControlTablesStruct(d=tab.data_ptr(), e=None, p=None, ld=L)
    try:
        _lib.check(lib.cmtts_set_control_tables(model._h, C.byref(ct)))
        assert call(1.5) == -1 and b"replaces d_control" in lib.cmtts_last_error()
        assert call(1.0) == 0
        ct.ld = L + 1
        _lib.check(lib.cmtts_set_control_tables(model._h, C.byref(ct)))
        assert call(1.0) == -1 and b"row pitch" in lib.cmtts_last_error()
        ct = _lib.ControlTablesStruct(d=None, e=tab.data_ptr(), p=None, ld=L)
        _lib.check(lib.cmtts_set_control_tables(model._h, C.byref(ct)))
        vc = _lib.VarianceControlsStruct(p_control=1.0, e_control=1.2)
        _lib.check(lib.cmtts_set_variance_controls(model._h, C.byref(vc)))
        assert call(1.0) == -1 and b"replaces e_control" in lib.cmtts_last_error()
    finally:
        lib.cmtts_set_variance_controls(model._h, None)
        lib.cmtts_set_control_tables(model._h, None)
        torch.cuda.synchronize()


# ---- 9. streamed PCM with per-utterance vectors

def test_stream_with_per_utterance_controls():
    from test_gpu_stream import HOP, _stitch, _voc
    host = _host()
    cfg = get_config("VCTK")
    seed = 2
    sd = synth_cmtts_state_dict(cfg, seed=seed, dur_frames=5.0, dur_spread=0.3)
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(sd)
    rs = np.random.RandomState(seed)
    B, L = 3, 14
    src = np.asarray([L, 9, 5], np.int64)
    texts = np.zeros((B, L), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = torch.from_numpy(rs.standard_normal((B, cfg.external_speaker_dim)).astype(np.float32))
    texts, src = torch.from_numpy(texts), torch.from_numpy(src)
    ctl = {"p_control": torch.tensor([0.8, 1.0, 1.3]), "e_control": torch.tensor([1.2, 0.7, 1.0]), "d_control": torch.tensor([0.75, 1.0, 1.5])}

    class Gen:
        def __init__(self):
            self.g = torch.Generator().manual_seed(seed)

        def randn(self, *shape, **kw):
            return torch.randn(*shape, generator=self.g).to(DEV)

        def randn_like(self, x):
            return self.randn(*x.shape)

    voc, _, _ = _voc()
    plain_lens = None
    for wino, tol in ((0, 0), (1, 1)):
        voc.set_option("winograd", wino)
        res = host.CMTotalTTSSynthesize.from_model(model, T=N_STEPS, generator=Gen(), **ctl).synthesize((None, None, None, texts, src, L, spk))
        lens = res[11].cpu().tolist()
        ref = host.vocoder_infer(res[0].transpose(1, 2), voc, lengths=[n * HOP for n in lens])
        got, _ = _stitch(host.synthesize_stream(model, voc, texts, src, spker_embeds=spk, n_steps=N_STEPS, generator=Gen(),
                                                chunk_frames=(8, 16), **ctl), lens)
        for b in range(B):
            if tol == 0:
                assert np.array_equal(got[b], ref[b]), b
            else:
                assert int(np.abs(got[b].astype(np.int32) - ref[b]).max()) <= tol
        if plain_lens is None:
            plain_lens = model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk)["mel_lens"].cpu().tolist()
        assert lens != plain_lens and lens[1] == plain_lens[1]          # the controls arrived; utterance 1 has d = 1
