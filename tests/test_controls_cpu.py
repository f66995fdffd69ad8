"""Per-utterance and per-phoneme prosody controls, CPU side (no compute calls): the entry point cmtts_set_control_tables, the
host's validation of control tensors, what the numpy oracle says about per-utterance vectors (the ground the GPU tests in
tests/test_gpu_controls.py stand on), and the routing of per-utterance controls through shard.two_phase on gloo worlds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib, shard
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from oracle import cmtts_oracle as O
from test_shard_gloo import _free_port, _join_gloo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the entry point

def test_entry_point_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "cmtts_hip.h")).read()
    assert re.search(r"int cmtts_set_control_tables\(cmtts_model\* m, const cmtts_control_tables\* t\);", text)
    body = re.search(r"typedef struct cmtts_control_tables \{(.*?)\} cmtts_control_tables;", text, flags=re.S).group(1)
    names = re.findall(r"(?:const float\*|int)\s+([a-z]+);", body)
    assert names == [n for n, _ in _lib.ControlTablesStruct._fields_] == ["d", "e", "p", "ld"]
    for line in ("model/modules.py:270", ":326", ":369"):
        assert line in text[text.index("Per-utterance and per-phoneme controls"):text.index("} cmtts_control_tables;")]
    assert hasattr(C.CDLL(_lib.LIB_PATH), "cmtts_set_control_tables")
    assert "cmtts_set_control_tables" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.cmtts_abi_version() == 8 and _lib.ABI_VERSION == 8          # entry points only: the revision stays
    assert lib.cmtts_set_control_tables(None, None) == -1
    assert b"cmtts_set_control_tables" in lib.cmtts_last_error() and b"null" in lib.cmtts_last_error()


def test_tables_on_a_created_model():
    from cmtts_amd import host
    model = host.CMTotalTTS(get_config("VCTK"), "cpu")          # cmtts_create only: the tables live on the handle
    lib = model.lib
    ct = _lib.ControlTablesStruct(d=None, e=None, p=0x1000, ld=0)
    assert lib.cmtts_set_control_tables(model._h, C.byref(ct)) == -1 and b"ld" in lib.cmtts_last_error()
    # the record size follows "a pitch table is installed", nothing else
    R0 = lib.cmtts_text_state_record_bytes(model._h, 37)
    cfg = model.config
    assert R0 == shard.text_state_layout(cfg.hidden, cfg.cwt_hidden, 37)["record_bytes"]
    ct = _lib.ControlTablesStruct(d=0x1000, e=0x1000, p=None, ld=37)
    assert lib.cmtts_set_control_tables(model._h, C.byref(ct)) == 0
    assert lib.cmtts_text_state_record_bytes(model._h, 37) == R0
    ct.p = 0x1000
    assert lib.cmtts_set_control_tables(model._h, C.byref(ct)) == 0
    lay = shard.text_state_layout(cfg.hidden, cfg.cwt_hidden, 37, with_p=True)
    assert lib.cmtts_text_state_record_bytes(model._h, 37) == lay["record_bytes"] == R0 + (37 * 4 + 15) // 16 * 16
    assert lay["pctl"] == (R0, 37 * 4) and lay["pctl"][0] % 16 == 0
    assert lib.cmtts_set_control_tables(model._h, None) == 0               # NULL clears
    assert lib.cmtts_text_state_record_bytes(model._h, 37) == R0


# ---- 2. host validation, before anything launches (a create-only model cannot launch anything)

def _bad_controls(B, L):
    ok = torch.ones(B, L)
    nan = ok.clone(); nan[1, 2] = float("nan")
    zero = ok.clone(); zero[0, 0] = 0.0
    neg = ok.clone(); neg[2, 1] = -0.5
    return [
        ("wrong shape [B, L + 1]", dict(p_control=torch.ones(B, L + 1))),
        ("wrong shape [B + 1]", dict(e_control=torch.ones(B + 1))),
        ("wrong shape [B, L, 1]", dict(d_control=torch.ones(B, L, 1))),
        ("wrong dtype", dict(e_control=torch.ones(B, L, dtype=torch.float64))),
        ("P <= 0", dict(p_control=zero)),
        ("P < 0", dict(p_control=neg)),
        ("D < 0", dict(d_control=neg)),
        ("NaN in P", dict(p_control=nan)),
        ("NaN in E", dict(e_control=nan)),
        ("NaN in D", dict(d_control=nan)),
        ("NaN in a [B] vector", dict(e_control=nan[:, 2].contiguous())),
    ]


def test_host_validation_raises_value_error():
    from cmtts_amd import host
    model = host.CMTotalTTS(get_config("VCTK"), "cpu")
    B, L = 3, 20
    texts = torch.ones(B, L, dtype=torch.int64)
    src = torch.tensor([20, 14, 9])
    spk = torch.zeros(B, model.config.external_speaker_dim)
    for what, kw in _bad_controls(B, L):
        with pytest.raises(ValueError):
            model.duration_pitch_energy_net(None, texts, src, spker_embeds=spk, **kw)
        with pytest.raises(ValueError):
            model(torch.zeros(B, 1, 8, 80), torch.zeros(B), texts=texts, src_lens=src, spker_embeds=spk, **kw)
        with pytest.raises(ValueError):
            next(host.synthesize_stream(model, None, texts, src, spker_embeds=spk, **kw))
        with pytest.raises(ValueError):
            host.synthesize_sharded(model, texts, src, spker_embeds=spk, **kw)
        with pytest.raises(ValueError):
            host.text_state_records(model, texts, src, 0, 2, spker_embeds=spk, **kw)
        syn = host.CMTotalTTSSynthesize.from_model(model, T=2, **kw)
        with pytest.raises(ValueError):
            syn.synthesize((None, None, None, texts, src, L, spk))
    with pytest.raises(ValueError):
        host.frame_side_from_records(model, [], L, p_control=torch.ones(B, L + 1))
    with pytest.raises(ValueError):
        host.frame_side_from_records(model, [], L, p_control=-torch.ones(B, L))
    # a table replaces the scalar of its control: both at once is refused
    for name in ("p_control", "e_control", "d_control"):
        syn = host.CMTotalTTSSynthesize.from_model(model, T=2, **{name: 1.2})
        with pytest.raises(ValueError, match="replaces the scalar"):
            syn.synthesize((None, None, None, texts, src, L, spk), **{name: torch.ones(B, L)})
    # valid tables pass validation and reach the model, which has no weights: the launch is what is refused
    syn = host.CMTotalTTSSynthesize.from_model(model, T=2, p_control=torch.full((B,), 1.1))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        syn.synthesize((None, None, None, texts, src, L, spk), d_control=torch.ones(B, L))
    (p, e, d), tabs = host._resolve_controls(B, L, torch.tensor([0.8, 1.0, 1.3]), 1.2, torch.full((B, L), 0.5))
    assert (p, e, d) == (1.0, 1.2, 1.0) and sorted(tabs) == ["d", "p"]
    assert tabs["p"].shape == (B, L) and tabs["p"].is_contiguous() and tabs["p"][2].tolist() == [np.float32(1.3)] * L


# ---- 3. the oracle on per-utterance vectors: row b of one call with vectors == the call with row b's scalars, bit for bit

def _fixture():
    from conftest import load_golden
    g = load_golden("cmtts_VCTK")
    cfg = get_config("VCTK")
    sd = synth_cmtts_state_dict(cfg, seed=int(g["seed"]), dur_frames=4.0, dur_spread=0.03)
    return g, cfg, sd


def test_oracle_per_utterance_equals_scalar_calls():
    g, cfg, sd = _fixture()
    P, E, D = (0.8, 1.0, 1.3), (1.2, 0.7, 1.0), (0.75, 1.0, 1.5)
    B = len(g["src_lens"])
    col = lambda v: np.asarray(v, np.float32)[:, None]
    first = O.duration_pitch_speaker_net(sd, cfg, g["texts"], g["src_lens"], g.get("spker_embeds"),
                                         e_control=col(E), d_control=col(D))
    T = int(first["mel_len"].max())
    vec = O.duration_pitch_speaker_net(sd, cfg, g["texts"], g["src_lens"], g.get("spker_embeds"), max_mel_len=T,
                                       p_control=np.asarray(P, np.float32)[:, None, None], e_control=col(E), d_control=col(D))
    for b in range(B):
        one = O.duration_pitch_speaker_net(sd, cfg, g["texts"], g["src_lens"], g.get("spker_embeds"), max_mel_len=T,
                                           p_control=P[b], e_control=E[b], d_control=D[b])
        for k in ("log_d", "e_pred", "e_idx", "d_rounded"):
            assert np.array_equal(vec[k][b], one[k][b]), (k, b)
        assert vec["mel_len"][b] == one["mel_len"][b]


def test_oracle_takes_per_phoneme_tables():
    """The fixture of tests/test_gpu_controls.py::test_per_phoneme_against_oracle: seed-0 tables give mel_len 111 / 80 / 156."""
    g, cfg, sd = _fixture()
    B, L = g["texts"].shape
    rs = np.random.RandomState(0)
    D = rs.uniform(0.5, 2.0, size=(B, L)).astype(np.float32)
    E = rs.uniform(0.5, 1.5, size=(B, L)).astype(np.float32)
    st = O.duration_pitch_speaker_net(sd, cfg, g["texts"], g["src_lens"], g.get("spker_embeds"), e_control=E, d_control=D)
    assert st["mel_len"].tolist() == [111, 80, 156]


# ---- 4. gloo worlds: a per-utterance control indexed by GLOBAL utterance reaches the rank that runs the utterance

H, CWT, M, SEED, N_ITEMS = 8, 4, 80, 11, 13
BUCKETS = (16, 32, 48)


def _texts():
    rs = np.random.RandomState(7)
    src = rs.randint(3, 12, size=N_ITEMS)
    L = int(src.max())
    texts = np.zeros((N_ITEMS, L), np.int64)
    for i, s in enumerate(src):
        texts[i, :s] = rs.randint(1, 60, size=s)
    return texts, src


def _controls(L):
    rs = np.random.RandomState(3)
    d = rs.choice([0.5, 1.0, 1.5, 2.0], size=N_ITEMS).astype(np.float32)           # per utterance
    p = rs.uniform(0.7, 1.4, size=(N_ITEMS, L)).astype(np.float32)                 # per phoneme
    return d, p


def _text_side(texts, src, d_ctl, p_ctl, served):
    """Stand-in text side: durations = (token id % 7) * D[i], the pitch row of utterance i packed into its record (layout
    revision 2), both taken from the GLOBAL tables by global index."""
    L = texts.shape[1]
    lay = shard.text_state_layout(H, CWT, L, with_p=True)

    def run(lo, hi):
        rec = torch.zeros(hi - lo, lay["record_bytes"], dtype=torch.uint8)
        lens = []
        for k, i in enumerate(range(lo, hi)):
            d = np.zeros(L, np.float32)
            d[:src[i]] = (texts[i, :src[i]] % 7).astype(np.float32) * d_ctl[i]
            cum = np.cumsum(d.astype(np.int64)).astype(np.int32)
            hdr = np.zeros(64, np.uint8)
            hdr[:16].view(np.int64)[:] = [i, int(cum[-1])]
            hdr[16:28].view(np.int32)[:] = [int(src[i]), shard.TEXT_STATE_LAYOUT_P, L]
            rec[k, :64] = torch.from_numpy(hdr)
            off, nb = lay["cum"]
            rec[k, off:off + nb] = torch.from_numpy(cum).view(torch.uint8)
            off, nb = lay["pctl"]
            rec[k, off:off + nb] = torch.from_numpy(p_ctl[i].copy()).view(torch.uint8)
            lens.append(int(cum[-1]))
            served.append(i)
        return rec, torch.tensor(lens, dtype=torch.int64)
    return run, lay


def _frame_side(lay, p_ctl, seen):
    def run(groups):
        out = []
        for bucket, rec, ids, planned in groups:
            h = shard.text_state_header(rec)
            assert h["index"].tolist() == list(ids) and (h["layout"] == shard.TEXT_STATE_LAYOUT_P).all()
            rows = shard.text_state_region(rec, lay, "pctl")
            # the row that arrived is the row of the utterance's GLOBAL index, whichever rank packed it
            assert torch.equal(rows, torch.from_numpy(p_ctl[list(ids)]))
            seen.append((bucket, list(ids)))
            mels = []
            for k, i in enumerate(ids):
                g = torch.Generator().manual_seed(SEED * 1000003 + i)
                mels.append(torch.randn(bucket, M, generator=g) * rows[k].mean() + 1000.0 * i)
            out.append((torch.stack(mels), torch.tensor(planned, dtype=torch.int64)))
        return out
    return run


def _run(group=None):
    texts, src = _texts()
    d_ctl, p_ctl = _controls(texts.shape[1])
    served, seen = [], []
    text_side, lay = _text_side(texts, src, d_ctl, p_ctl, served)
    res = shard.two_phase(N_ITEMS, text_side, _frame_side(lay, p_ctl, seen), group=group, buckets=BUCKETS)
    return res, served, seen


def _worker(rank, world, port, q):
    _join_gloo(rank, world, port)
    res, served, seen = _run()
    q.put((rank, [m.numpy() for m in res["mels"]], res["mel_len"], served, seen))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("world", [2, 4])
def test_controls_follow_the_utterance_across_ranks(world):
    texts, src = _texts()
    d_ctl, _ = _controls(texts.shape[1])
    ref, served, _ = _run()
    assert served == list(range(N_ITEMS))
    want = [int(((texts[i, :src[i]] % 7).astype(np.float32) * d_ctl[i]).astype(np.int64).sum()) for i in range(N_ITEMS)]
    assert ref["mel_len"] == want
    assert len(set(d_ctl.tolist())) > 1
    for rank, mels, mel_len, served_r, seen in _spawn(world):
        lo, hi = shard.shard_range(N_ITEMS, rank, world)
        assert served_r == list(range(lo, hi))                       # the text side took the rows of its own slice
        assert mel_len == want                                       # ... and applied the factors of those global rows
        assert len(mels) == N_ITEMS
        for a, b in zip(mels, ref["mels"]):                          # the same order and bits as world 1
            assert np.array_equal(a, b.numpy())
