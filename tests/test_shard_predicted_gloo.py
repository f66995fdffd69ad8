"""Sharding a batch that starts from text, on CPU: world-2 and world-4 gloo runs of shard.two_phase (text side per slice, length
agreement, plan, record exchange, frame side per bucket, all-gather of mels) with a stand-in model whose "duration predictor"
derives each utterance's frame count from its text — the planner learns the lengths only from the text side.  The records are real
byte buffers of the text-state record layout (include/cmtts_hip.h, cmtts_text_state_*)."""
import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cmtts_amd  # noqa: F401
from cmtts_amd import shard
from test_shard_gloo import _free_port, _join_gloo

H, CWT, M, SEED = 8, 4, 80, 11
BUCKETS = (16, 32, 48)


def _texts(n_items, overflow):
    rs = np.random.RandomState(7)
    src = rs.randint(3, 12, size=n_items)
    if overflow:
        src[1] = 11
    L = int(src.max())
    texts = np.zeros((n_items, L), np.int64)
    for i, s in enumerate(src):
        texts[i, :s] = rs.randint(1, 60, size=s)
    if overflow:
        texts[1, :src[1]] = 55          # 11 x 6 frames: longer than the largest bucket
    return texts, src


def _durations(text_row, s):
    """Stand-in duration predictor: 0..6 frames per phoneme, from the token ids."""
    d = np.zeros(len(text_row), np.int64)
    d[:s] = text_row[:s] % 7
    return d


def _text_side(texts, src):
    L = texts.shape[1]
    lay = shard.text_state_layout(H, CWT, L)

    def run(lo, hi):
        R = lay["record_bytes"]
        rec = torch.zeros(hi - lo, R, dtype=torch.uint8)
        lens = []
        for k, i in enumerate(range(lo, hi)):
            d = _durations(texts[i], int(src[i]))
            cum = np.cumsum(d).astype(np.int32)
            hdr = np.zeros(64, np.uint8)
            hdr[:16].view(np.int64)[:] = [i, int(cum[-1])]
            hdr[16:28].view(np.int32)[:] = [int(src[i]), shard.TEXT_STATE_LAYOUT, L]
            rec[k, :64] = torch.from_numpy(hdr)
            off, nb = lay["out1"]
            rec[k, off:off + nb] = torch.full((nb // 4,), float(i), dtype=torch.float32).view(torch.uint8)
            off, nb = lay["cum"]
            rec[k, off:off + nb] = torch.from_numpy(cum).view(torch.uint8)
            lens.append(int(cum[-1]))
        return rec, torch.tensor(lens, dtype=torch.int64)
    return run, lay


def _frame_side(lay, seen):
    def run(groups):
        out = []
        for bucket, rec, ids, planned in groups:
            h = shard.text_state_header(rec)
            assert h["index"].tolist() == list(ids)
            assert (h["layout"] == shard.TEXT_STATE_LAYOUT).all()
            assert torch.equal(shard.text_state_region(rec, lay, "out1")[:, 0], torch.tensor(ids, dtype=torch.float32))
            cum = shard.text_state_region(rec, lay, "cum", torch.int32)
            assert [min(int(c), BUCKETS[-1]) for c in cum[:, -1]] == list(planned)
            seen.append((bucket, list(ids)))
            mels = []
            for i in ids:       # the global-index noise rule: utterance i's noise is the same on any rank of any world
                g = torch.Generator().manual_seed(SEED * 1000003 + i)
                mels.append(torch.randn(bucket, M, generator=g) + 1000.0 * i)
            out.append((torch.stack(mels), torch.tensor(planned, dtype=torch.int64)))
        return out
    return run


def _run(n_items, overflow, group=None):
    texts, src = _texts(n_items, overflow)
    text_side, lay = _text_side(texts, src)
    seen = []
    res = shard.two_phase(n_items, text_side, _frame_side(lay, seen), group=group, buckets=BUCKETS)
    return res, seen


def _worker(rank, world, port, n_items, overflow, q):
    _join_gloo(rank, world, port)
    res, seen = _run(n_items, overflow)
    got = shard.text_state_header(res["records"])["index"].tolist()
    q.put((rank, [m.numpy() for m in res["mels"]], res["mel_len"], res["plan"], res["truncated"], got, seen))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, n_items, overflow):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_items, overflow, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def _check_world(world, n_items, overflow, ref):
    texts, src = _texts(n_items, overflow)
    lens = [int(_durations(texts[i], int(src[i])).sum()) for i in range(n_items)]
    res = _spawn(world, n_items, overflow)
    plans = [r[3] for r in res]
    assert all(p == plans[0] for p in plans), "ranks disagree on the plan"
    planned, trunc = shard.planned_lengths(lens, BUCKETS)
    assert plans[0] == shard.plan_shards(planned, world, BUCKETS)
    for rank, mels, mel_len, plan, truncated, got, seen in res:
        assert mel_len == lens and truncated == trunc
        assert len(mels) == n_items
        for i, m in enumerate(mels):            # restored to the input order, trimmed to the planned length
            assert m.shape == (planned[i], M) and np.allclose(m.mean(), 1000.0 * i, atol=1.0)
        # world-size independence: the same bits as world 1
        for a, b in zip(mels, ref["mels"]):
            assert np.array_equal(a, b.numpy())
    # every utterance's record reached exactly its planned rank (plus the filler stand-ins that rank needs), nothing else
    slots, need = shard.route_records(plans[0], n_items, world)
    home = {}
    for b, ranks in plans[0].items():
        for r, ids in enumerate(ranks):
            for i in ids:
                if i >= 0:
                    assert i not in home
                    home[i] = r
    assert sorted(home) == list(range(n_items))
    for rank, *_rest, got, seen in res:
        assert got == need[rank]
        mine = sorted(i for i, r in home.items() if r == rank)
        assert set(mine) <= set(got)
        assert set(got) - set(mine) <= {i for b in slots for i in slots[b][rank]}
        assert sorted(b for b, _ in seen) == sorted(plans[0])
    return res


def test_two_phase_world_size_independent():
    n_items = 13
    ref, _ = _run(n_items, False)
    assert ref["truncated"] == []
    for world in (2, 4):
        _check_world(world, n_items, False, ref)


def test_two_phase_overflow_is_truncated_and_reported():
    n_items = 9
    ref, _ = _run(n_items, True)
    assert ref["truncated"] == [1] and ref["mel_len"][1] > BUCKETS[-1]
    assert ref["mels"][1].shape[0] == BUCKETS[-1]
    _check_world(2, n_items, True, ref)


def test_route_records_fillers():
    plan = shard.plan_shards([5, 40, 41, 3], 4, BUCKETS)
    slots, need = shard.route_records(plan, 4, 4)
    for b, ranks in slots.items():
        assert all(i >= 0 for r in ranks for i in r)
        assert len({len(r) for r in ranks}) == 1
    assert sorted(set(i for n in need for i in n)) == [0, 1, 2, 3]
    lay = shard.text_state_layout(256, 128, 171)
    assert lay["record_bytes"] % 16 == 0 and all(lay[r][0] % 16 == 0 for r in shard.TEXT_STATE_REGIONS)
    assert lay["record_bytes"] == 64 + 256 * 172 * 4 + 128 * 172 * 4 + 256 * 4 + 171 * 4 + 4
