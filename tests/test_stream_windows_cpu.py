"""Streamed vocoding, host side (no GPU): the generator's receptive radius from its config, the window planner's invariants,
and — on the numpy oracle — that stitching window cores reproduces the whole-mel waveform with a halo of H frames and not
with H - 1."""
import dataclasses

import numpy as np
import pytest

from cmtts_amd import host
from cmtts_amd.config import HifiGanConfig
from cmtts_amd.weights import synth_hifigan_state_dict
from oracle import cmtts_oracle as O


def _conv_support(a, k, d):
    """Positions of a stride-1 'same' conv (kernel k, dilation d) that read an affected input position."""
    p = d * (k - 1) // 2
    out = np.zeros_like(a)
    for j in range(k):
        s = j * d - p                       # out[t] reads in[t + s]
        if s >= 0:
            out[: len(a) - s] |= a[s:]
        else:
            out[-s:] |= a[: len(a) + s]
    return out


def _brute_halo(h: HifiGanConfig, T=160):
    """Mark one mel frame as 'affected' and push the mark through every layer of the generator as a set of positions
    (conv, ConvTranspose1d, ResBlock residuals, MRF union); the radius is the farthest output frame reached."""
    m = T // 2
    a = np.zeros(T, bool)
    a[m] = True
    a = _conv_support(a, 7, 1)                                  # conv_pre
    for u, k in zip(h.upsample_rates, h.upsample_kernel_sizes):
        p = (k - u) // 2
        y = np.zeros(len(a) * u, bool)
        for i in np.nonzero(a)[0]:                              # y[i u + j - p] += x[i] w[j]
            for j in range(k):
                t = i * u + j - p
                if 0 <= t < len(y):
                    y[t] = True
        xs = np.zeros_like(y)
        for rk, dils in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
            xr = y
            for d in dils:
                xr = xr | _conv_support(_conv_support(xr, rk, d), rk, 1)
            xs |= xr
        a = xs
    a = _conv_support(a, 7, 1)                                  # conv_post
    frames = np.nonzero(a.reshape(T, h.hop).any(1))[0]
    return int(max(m - frames.min(), frames.max() - m))


def test_halo_is_13_for_v1_and_matches_brute_force():
    h = HifiGanConfig()
    assert h.halo_frames == 13 == host.vocoder_halo_frames(h) == host.vocoder_halo_frames()
    assert _brute_halo(h) == 13
    for mod in (dict(resblock_dilation_sizes=((1, 2, 3),) * 3),
                dict(resblock_dilation_sizes=((1, 3, 9), (1, 3, 5), (2, 2, 2))),
                dict(resblock_kernel_sizes=(3, 5, 13)),
                dict(upsample_rates=(8, 4, 4, 2), upsample_kernel_sizes=(16, 8, 8, 4))):
        hm = dataclasses.replace(h, **mod)
        assert hm.halo_frames == _brute_halo(hm), mod
    assert dataclasses.replace(h, resblock_dilation_sizes=((1, 3, 9),) * 3).halo_frames > 13


def _check_plan(T, lens, chunks, H):
    rounds = host.plan_stream_windows(T, lens, chunks, H)
    pos = [0] * len(lens)
    last = [None] * len(lens)
    for ri, r in enumerate(rounds):
        assert 0 < r.Tw <= T and r.core > 0
        c = min(chunks[min(ri, len(chunks) - 1)], max(lens[b] - pos[b] for b in range(len(lens)) if last[b] is None and lens[b] > 0))
        if r.Tw == T:
            assert r.core == T and c + 2 * H >= T
        else:
            assert (r.Tw, r.core) == (c + 2 * H, c)
        seen = set()
        for b, start, off, n in r.windows:
            assert b not in seen and last[b] is None, "one window per live utterance per round"
            seen.add(b)
            assert 0 <= start and start + r.Tw <= T, "window inside [0, T)"
            cs = start + off
            assert cs == pos[b], "cores tile without gaps or overlaps"
            assert 1 <= n <= r.core and off + n <= r.Tw
            assert off >= H or start == 0, "left context"
            assert start + r.Tw - (cs + n) >= H or start + r.Tw == T, "right context"
            pos[b] = cs + n
            if pos[b] == lens[b]:
                last[b] = ri
        assert seen == {b for b in range(len(lens)) if lens[b] > 0 and (ri == 0 or last[b] is None or last[b] == ri)}
    assert pos == list(lens)
    return rounds


@pytest.mark.parametrize("T", [1, 13, 26, 27, 37, 200, 512])
@pytest.mark.parametrize("chunks", [(32, 64, 128, 256), (5,), (13, 30), (1, 2)])
def test_planner_properties(T, chunks):
    H = 13
    rs = np.random.RandomState(T)
    lens = sorted({1, T, max(1, T // 2), max(1, T - 1)} | set(rs.randint(1, T + 1, size=3).tolist()))
    _check_plan(T, lens, chunks, H)
    _check_plan(T, lens + [0], chunks, 0)


def test_planner_rounds_and_edges():
    r = host.plan_stream_windows(512, [512], halo=13)
    assert [x.core for x in r] == [32, 64, 128, 256, 32] and sum(w[3] for x in r for w in x.windows) == 512
    assert sum(x.Tw for x in r) == 642                            # 1.25x the whole mel's generator frames
    assert r[0].windows == [(0, 0, 0, 32)]                        # clamped at 0: the core starts the window
    assert r[1].windows == [(0, 32 - 13, 13, 64)]
    tail = r[-1].windows[0]
    assert tail[1] + r[-1].Tw == 512                              # clamped at T: shifted inwards, core offset grows
    one = host.plan_stream_windows(30, [30, 7], halo=13)           # T < core + 2H: one whole-tensor window each
    assert len(one) == 1 and one[0].Tw == one[0].core == 30 and one[0].windows == [(0, 0, 0, 30), (1, 0, 0, 7)]
    with pytest.raises(ValueError):
        host.plan_stream_windows(10, [11], halo=13)
    with pytest.raises(ValueError):
        host.plan_stream_windows(10, [5], chunk_frames=(0,), halo=13)


def _stitched(hsd, hcfg, mel_ct, lens, chunks, halo):
    hop = hcfg.hop
    out = [np.zeros(n * hop, np.float64) for n in lens]      # holds float32 and float64 results exactly
    for r in host.plan_stream_windows(mel_ct.shape[2], lens, chunks, halo):
        win = np.stack([mel_ct[b, :, s:s + r.Tw] for b, s, _, _ in r.windows])
        wav = O.hifigan_generator(hsd, hcfg, win)[:, 0]
        for n, (b, s, off, cl) in enumerate(r.windows):
            out[b][(s + off) * hop:(s + off + cl) * hop] = wav[n, off * hop:(off + cl) * hop]
    return out


def test_oracle_stitched_windows_equal_whole_mel():
    hcfg = HifiGanConfig()
    H = hcfg.halo_frames
    hsd = synth_hifigan_state_dict(hcfg, seed=5)
    rs = np.random.RandomState(1)
    T, lens, chunks = 40, [40, 29], (6, 10)
    mel_ct = rs.standard_normal((2, 80, T)).astype(np.float32)

    def gap(halo):
        whole = O.hifigan_generator(hsd, hcfg, mel_ct)[:, 0]
        st = _stitched(hsd, hcfg, mel_ct, lens, chunks, halo)
        return max(float(np.abs(s - whole[b, : n * hcfg.hop]).max()) for b, (s, n) in enumerate(zip(st, lens)))

    d_h, d_h1 = gap(H), gap(H - 1)
    with O.precision("f64"):
        e_h, e_h1 = gap(H), gap(H - 1)
    print(f"stitched vs whole: float32 halo {H}: {d_h:.2e}, halo {H - 1}: {d_h1:.2e}; float64 {e_h:.2e} / {e_h1:.2e}")
    assert d_h <= 2e-6, "H frames of context reproduce the whole-mel waveform to float32 rounding"
    # The oracle's arithmetic does not depend on the window shape (with H frames the stitched samples come out identical), so any
    # gap at H - 1 is the dependence on the frame left out — small (~3e-13 in float64, ~3e-8 in float32) because only the outermost
    # tap of every layer reaches that far, but far above float64 rounding: H is the true bound, not merely a sufficient one.
    assert e_h == 0.0
    assert d_h1 > 0 and e_h1 > 1e-14, "with H - 1 frames some sample differs: H is the true bound"


def test_c_abi_halo_and_workspace():
    import ctypes as C
    from cmtts_amd import _lib
    lib = _lib.load()
    v = C.c_void_p()
    assert lib.cmtts_vocoder_create(C.byref(v)) == 0
    try:
        assert lib.cmtts_vocoder_halo_frames(v) == HifiGanConfig().halo_frames == 13
        assert lib.cmtts_vocoder_windows_workspace_bytes(v, 0, 58) == 0
        assert lib.cmtts_vocoder_windows_workspace_bytes(v, 4, 58) > lib.cmtts_vocoder_workspace_bytes(v, 4, 58) + 4 * 80 * 58 * 4
        # an unfinalized vocoder launches nothing
        assert lib.cmtts_vocoder_forward_windows(v, None, 1, 58, None, 1, 58, 32, None, 32768.0, None, 0, None) == -1
    finally:
        lib.cmtts_vocoder_destroy(v)
    assert lib.cmtts_vocoder_halo_frames(None) == -1
