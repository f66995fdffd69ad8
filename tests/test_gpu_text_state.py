"""Text-state records (cmtts_text_state_pack / _unpack, include/cmtts_hip.h) and the two-phase sharded synthesis built on them
(host.synthesize_sharded, shard.two_phase): bitwise round trips, a virtual multi-rank world on one GPU, the oracle, and the record
exchange on a 1-rank RCCL communicator."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib, shard
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from conftest import near_flip_mask, report, WINO_TOL
from test_gpu_parity import KNOWN_ORACLE_FLIPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(variant="LibriTTS", dur_frames=3.0, dur_spread=0.05, seed=5):
    from cmtts_amd import host
    cfg = get_config(variant)
    sd = synth_cmtts_state_dict(cfg, seed=seed, dur_frames=dur_frames, dur_spread=dur_spread)
    return host.CMTotalTTS(cfg, device=DEV).load_state_dict(sd), sd, cfg


def _batch(cfg, B, L, seed, lo=None):
    rs = np.random.RandomState(seed)
    src = rs.randint(lo or max(1, L // 4), L + 1, size=B)
    src[rs.randint(B)] = L
    texts = np.zeros((B, L), np.int64)
    for b, s in enumerate(src):
        texts[b, :s] = rs.randint(1, cfg.n_symbols, size=s)
    spk = rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32)
    return torch.from_numpy(texts), torch.from_numpy(src.astype(np.int64)), torch.from_numpy(spk)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _frame(model, tws, B_all, L, b0, B, T):
    """cmtts_frame_forward_sub_t on [b0, b0 + B) -> dict of every output that is compared."""
    lib, cfg = model.lib, model.config
    p1_ld = (L + 3) // 4 * 4
    out = {"cond_ct": torch.empty(B, cfg.hidden, T, device=DEV), "mel2ph": torch.empty(B, T, dtype=torch.int64, device=DEV),
           "p_idx": torch.empty(B, T, dtype=torch.int64, device=DEV), "f0_stats": torch.empty(B, 2, device=DEV),
           "cond_p1": torch.empty(B, cfg.res_layers * cfg.res_channels, p1_ld, device=DEV),
           "cond_p1t": torch.empty(B, cfg.res_layers, p1_ld, cfg.res_channels, device=DEV)}
    nf = lib.cmtts_frame_workspace_bytes(model._h, B, T)
    fws = torch.empty(nf, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_frame_forward_sub_t(model._h, tws.data_ptr(), B_all, L, b0, B, T, out["cond_ct"].data_ptr(),
                                             out["mel2ph"].data_ptr(), None, None, out["p_idx"].data_ptr(), out["f0_stats"].data_ptr(),
                                             out["cond_p1"].data_ptr(), out["cond_p1t"].data_ptr(), fws.data_ptr(), nf, _stream()))
    del out["cond_p1"]
    return out


@pytest.mark.parametrize("B,L,n_rows", [(32, 171, 13), (3, 37, 3)])
def test_pack_unpack_round_trip_bitwise(B, L, n_rows):
    model, _, cfg = _model()
    lib = model.lib
    texts, src, spk = _batch(cfg, B, L, seed=B + L)
    texts, src, spk = texts.to(DEV), src.to(DEV), spk.to(DEV)
    nb = lib.cmtts_text_workspace_bytes(model._h, B, L)
    tws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    mel_len = torch.empty(B, dtype=torch.int64, device=DEV)
    spk_out = torch.empty(B, cfg.hidden, device=DEV)
    _lib.check(lib.cmtts_text_forward(model._h, texts.data_ptr(), src.data_ptr(), spk.data_ptr(), None, B, L, 1.0, None, None,
                                      mel_len.data_ptr(), None, None, None, spk_out.data_ptr(), tws.data_ptr(), nb, _stream()))
    order = list(range(B))[::-1]
    rows = (order[0::2] + order[1::2])[:n_rows]                 # reversed and interleaved
    R = lib.cmtts_text_state_record_bytes(model._h, L)
    lay = shard.text_state_layout(cfg.hidden, cfg.cwt_hidden, L)
    assert R == lay["record_bytes"]
    rows_d = torch.tensor(rows, dtype=torch.int32, device=DEV)
    gidx = torch.tensor([1000 + r for r in rows], dtype=torch.int64, device=DEV)
    rec = torch.full((n_rows, R), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_text_state_pack(model._h, tws.data_ptr(), B, L, rows_d.data_ptr(), n_rows, gidx.data_ptr(), src.data_ptr(),
                                         rec.data_ptr(), _stream()))
    h = shard.text_state_header(rec)
    assert h["index"].tolist() == [1000 + r for r in rows]
    assert h["mel_len"].tolist() == [int(mel_len[r]) for r in rows]
    assert h["src_len"].tolist() == [int(src[r]) for r in rows]
    assert (h["layout"] == shard.TEXT_STATE_LAYOUT).all() and (h["L_all"] == L).all()
    assert torch.equal(shard.text_state_region(rec, lay, "spk"), spk_out[rows])
    nb2 = lib.cmtts_text_workspace_bytes(model._h, n_rows, L)
    tws2 = torch.full((nb2,), 0xCD, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_text_state_unpack(model._h, rec.data_ptr(), n_rows, L, tws2.data_ptr(), nb2, _stream()))
    assert lib.cmtts_text_state_unpack(model._h, rec.data_ptr(), n_rows, L, tws2.data_ptr(), nb2 - 1, _stream()) == -4
    T = int(mel_len.max())
    for k, r in enumerate(rows):
        a = _frame(model, tws, B, L, r, 1, T)
        b = _frame(model, tws2, n_rows, L, k, 1, T)
        for name in a:
            assert torch.equal(a[name], b[name]), (name, r)
    # a contiguous run of rows: the batched call on both workspaces
    n = min(4, B)
    rows_c = torch.arange(n, dtype=torch.int32, device=DEV)
    rec_c = torch.empty(n, R, dtype=torch.uint8, device=DEV)
    _lib.check(lib.cmtts_text_state_pack(model._h, tws.data_ptr(), B, L, rows_c.data_ptr(), n, None, None, rec_c.data_ptr(), _stream()))
    assert shard.text_state_header(rec_c)["index"].tolist() == list(range(n))
    _lib.check(lib.cmtts_text_state_unpack(model._h, rec_c.data_ptr(), n, L, tws2.data_ptr(), nb2, _stream()))
    a, b = _frame(model, tws, B, L, 0, n, T), _frame(model, tws2, n, L, 0, n, T)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def _virtual_world(model, texts, src, spk, world, n_steps, seed, buckets):
    """synthesize_sharded's per-rank body for every rank of a `world`, one rank after the other on this GPU; the record exchange is
    host-side routing of the packed records (shard.route_records)."""
    from cmtts_amd import host
    n = texts.shape[0]
    L_all = int(src.max())
    recs, lens = [], []
    for r in range(world):
        lo, hi = shard.shard_range(n, r, world)
        rec, ml = host.text_state_records(model, texts, src, lo, hi, spker_embeds=spk)
        recs.append(rec)
        lens.append(ml)
    records = torch.cat(recs)                       # the slices are contiguous: global order
    mel_len = torch.cat(lens).tolist()
    planned, truncated = shard.planned_lengths(mel_len, buckets)
    plan = shard.plan_shards(planned, world, buckets)
    slots, need = shard.route_records(plan, n, world)
    mels, mel2ph = [None] * n, [None] * n
    sizes = []
    for r in range(world):
        recv = records.index_select(0, torch.tensor(need[r], device=DEV))
        row = {i: k for k, i in enumerate(need[r])}
        groups = [(b, recv.index_select(0, torch.tensor([row[i] for i in slots[b][r]], device=DEV)), slots[b][r],
                   [planned[i] for i in slots[b][r]]) for b in sorted(slots)]
        det = []
        outs = host.frame_side_from_records(model, groups, L_all, n_steps, seed, details=det)
        sizes.append([(b, len(ids)) for b, _, ids, _ in groups])
        for (b, _, ids, _), (mel, ml), d in zip(groups, outs, det):
            for k, i in enumerate(plan[b][r]):
                if i >= 0:
                    mels[i] = mel[k, :planned[i]]
                    mel2ph[i] = d["mel2ph"][k]
    torch.cuda.synchronize()
    return {"records": records, "mel_len": mel_len, "mels": mels, "mel2ph": mel2ph, "plan": plan, "sizes": sizes}


def test_virtual_world_matches_world_one():
    model, _, cfg = _model()
    n, L = 64, 48
    texts, src, spk = _batch(cfg, n, L, seed=21, lo=8)
    buckets = (128, 256, 512)
    ref = _virtual_world(model, texts, src, spk, 1, 2, 3, buckets)
    lay = shard.text_state_layout(cfg.hidden, cfg.cwt_hidden, L)
    cum = shard.text_state_region(ref["records"], lay, "cum", torch.int32)
    assert len(set(ref["mel_len"])) > 4, "durations are not predicted"
    assert len(ref["plan"]) >= 2
    for world in (2, 4):
        got = _virtual_world(model, texts, src, spk, world, 2, 3, buckets)
        report(f"TEXT_STATE virtual world {world}: bucket-group sizes per rank {got['sizes']} (world 1: {ref['sizes']})")
        assert got["mel_len"] == ref["mel_len"]
        assert torch.equal(shard.text_state_region(got["records"], lay, "cum", torch.int32), cum)       # d_rounded = its differences
        diff = (got["records"] != ref["records"]).sum(1)
        report(f"TEXT_STATE virtual world {world}: records differing from world 1: {int((diff > 0).sum())} of {n}")
        assert torch.equal(got["records"], ref["records"]), "the text side is not batch-size invariant"
        err = 0.0
        for i in range(n):
            assert torch.equal(got["mel2ph"][i], ref["mel2ph"][i]) or got["mel2ph"][i].shape != ref["mel2ph"][i].shape
            assert torch.equal(got["mel2ph"][i][:ref["mel_len"][i]], ref["mel2ph"][i][:ref["mel_len"][i]])
            err = max(err, float((got["mels"][i] - ref["mels"][i]).abs().max()))
        report(f"TEXT_STATE virtual world {world}: max |dmel| vs world 1 = {err:.2e}")
        assert err <= WINO_TOL


def test_sharded_against_oracle():
    from cmtts_amd import host
    from oracle import cmtts_oracle as O
    model, sd, cfg = _model(dur_frames=4.0, dur_spread=0.0, seed=9)
    texts, src, spk = _batch(cfg, 4, 20, seed=2, lo=4)
    src[:] = torch.tensor([6, 20, 8, 19])
    for b in range(4):
        texts[b, src[b]:] = 0
    buckets = (64, 128)
    res = host.synthesize_sharded(model, texts, src, spker_embeds=spk, n_steps=2, seed=4, buckets=buckets)
    assert len(res["plan"]) == 2 and res["truncated"] == []
    flips = 0
    for b, ranks in res["plan"].items():
        ids = [i for i in ranks[0] if i >= 0]
        st = O.duration_pitch_speaker_net(sd, cfg, texts.numpy(), src.numpy(), spk.numpy(), max_mel_len=b)
        assert [int(st["mel_len"][i]) for i in ids] == [res["mel_len"][i] for i in ids]
        noise = torch.stack([host.utterance_noise(4, i, 3, b, cfg.n_mels, DEV) for i in ids], 1).cpu().numpy()
        ref = O.karras_sample_tts(sd, cfg, st["cond"][ids], st["speaker_emb"][ids], 2, list(noise))
        # the frame side's integer stages against the oracle: rerun from the records of this bucket on the GPU
        det = []
        recs, _ = host.text_state_records(model, texts, src, 0, 4, spker_embeds=spk)
        host.frame_side_from_records(model, [(b, recs[ids], ids, [res["mel_len"][i] for i in ids])], int(src.max()), 2, 4, details=det)
        m2p = det[0]["mel2ph"].cpu().numpy()
        ref_m2p = st["mel2ph"][ids]                # the oracle's mel2ph is as wide as the batch's longest utterance
        W = min(ref_m2p.shape[1], b)
        assert np.array_equal(m2p[:, :W], ref_m2p[:, :W]) and not m2p[:, W:].any() and not ref_m2p[:, W:].any()
        same = det[0]["p_idx"].cpu().numpy() == st["p_idx"][ids]
        for k, i in enumerate(ids):
            got = res["mels"][i].cpu().numpy()
            ml = got.shape[0]
            ok = near_flip_mask(same)[k, :ml]
            assert np.abs(got - ref[k, :ml])[ok].max() < 1e-3, i
        flips += int((~same).sum())
    assert flips <= KNOWN_ORACLE_FLIPS["pitch"]


def test_exchange_records_one_rank_communicator():
    lib = _lib.load()
    torch.cuda.set_device(0)
    uid = (C.c_char * 128)()
    _lib.check(lib.cmtts_comm_unique_id(C.cast(uid, C.c_void_p)))
    comm = C.c_void_p()
    _lib.check(lib.cmtts_comm_init_rank(C.byref(comm), 1, 0, C.cast(uid, C.c_void_p)))
    try:
        R, n = 4160, 7
        g = torch.Generator().manual_seed(3)
        rec = torch.randint(0, 256, (n, R), generator=g, dtype=torch.int32).to(torch.uint8).to(DEV)
        counts = (C.c_int64 * 1)(n)
        for use_comm in (True, False):
            out = torch.zeros(n, R, dtype=torch.uint8, device=DEV)
            _lib.check(lib.cmtts_exchange_records(comm if use_comm else None, 1, rec.data_ptr(), counts, out.data_ptr(), counts, R, _stream()))
            torch.cuda.synchronize()
            assert torch.equal(out, rec)
        assert lib.cmtts_exchange_records(None, 2, rec.data_ptr(), counts, rec.data_ptr(), counts, R, None) < 0
    finally:
        _lib.check(lib.cmtts_comm_destroy(comm))
