"""The text side's kernels called ALONE through their launch hooks against the float64 definition (tests/text_kernel_cases.py):
attention.hip (attention_kernel, attention_qb_kernel, attention_long_kernel) and conv_xres.hip (the three launches of an FFT block, the
fused FFN launch in its direct, F(2,3) and F(4,3) forms) — at the score regime a trained checkpoint produces, with padding that dominates
the result if it leaks — and the expected flip rate of the integer stages (durations, energy and pitch buckets) for the four
(ffn_wino, pred_wino) arms against the float64 oracle.

Bounds are M x d32: d32 = the deviation of the definition's own float32 evaluation on the same case, M = twice the worst ratio measured
on MI355X, rounded up (the kernels sum in MFMA order, numpy pairwise: a ratio of a few is a reordered fp32 sum; above 10 it is a finding)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from conftest import report, FLIP_MARGIN, pitch_margin_mask
import text_kernel_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# M = twice the worst measured ratio, rounded up.  Measured on MI355X (every ratio of the module is in the parity report):
# max |kernel - float64| / max(d32, 4 ulps), worst of all L, row strides and score regimes: attention_kernel 1.09 (L = 97, unit),
# attention_qb_kernel 1.09 (the same bits), attention_long_kernel 1.49 (L = 320, unit); peaky / first / overflow <= 1.11, flat <= 0.15 of the floor
ATTN_M = {"plain": 3, "qb": 3, "long": 3}
# conv_xres launches: |kernel - float64| / d32 (d32 = the DIRECT form's float32 evaluation for all three FFN arms: one yardstick, so the
# arms' ratios compare).  Measured worst: in-projection 4.88 and out-projection 3.80 (both at N = 1, where d32 is the maximum over one column
# only; <= 1.26 / 1.16 at every other N), fused FFN launch direct 1.72, F(2,3) 1.14, F(4,3) 3.72 (all three at N = 97)
XRES_M = {"qkv": 10, "out": 8, "ffn_direct": 4, "ffn_f23": 3, "ffn_f43": 8}
# |kernel - float32 restatement of the form's own products| / d32.  Measured worst: direct 1.94 (N = 31), F(2,3) 1.54, F(4,3) 4.23 (N = 97)
XRES_M_OWN = {"ffn_direct": 4, "ffn_f23": 4, "ffn_f43": 9}
# flip rates: every arm's expected rate <= FLIP_R x the float32 oracle's.  Measured worst ratio 1.44 (LJSpeech energy, ffn_wino = 0: 63.0 against 43.7 per million)
FLIP_R = 3
# boundary margins in buckets, set as conftest.FLIP_MARGIN was (pitch: 2e-3; largest pitch error measured here 5.5e-4): 4 x the largest error of the
# pre-rounding value over both variants and all four arms — durations 5.35e-5, energy 3.14e-4
DUR_MARGIN = 2.2e-4
ENERGY_MARGIN = 1.3e-3


def _clib():
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    for f in ("cmtts_launch_attention", "cmtts_attention_set_qb", "cmtts_launch_conv_xres", "cmtts_launch_conv_xresq", "cmtts_xres_set_nt"):
        getattr(lib, f).restype = C.c_int
    return lib


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cases are read-only arrays)


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------- attention.hip

def _attention(lib, qkv, lens, L, ld):
    """One launch on qkv [B][768][ld] -> out float32 [B + 2][256][ld] (the launch's rows are 1 .. B; SENTINEL everywhere before it)."""
    Bn = qkv.shape[0]
    qd, ln = _dev(qkv), _dev(lens)
    out = torch.full((Bn + 2, TC.ATTN_H * TC.DH, ld), TC.SENTINEL, device=DEV)
    a = TC.AttnArgs(qd.data_ptr(), out[1:].data_ptr(), ln.data_ptr(), 3 * TC.ATTN_H * TC.DH * ld, TC.ATTN_H * TC.DH * ld,
                    Bn, TC.ATTN_H, TC.DH, L, ld, 1.0 / math.sqrt(TC.DH))
    assert lib.cmtts_launch_attention(C.byref(a), None) == 0
    torch.cuda.synchronize()
    got = _np(out)
    assert (got[0] == TC.SENTINEL).all() and (got[-1] == TC.SENTINEL).all(), "written outside the launch's rows"
    assert (got[:, :, L:] == TC.SENTINEL).all(), "written beyond L"
    assert np.isfinite(got[1:-1, :, :L]).all()
    return got[1:-1, :, :L]


ATTN_PARAMS = ([("plain", L) for L in TC.ATTN_L_SHORT] + [("qb", L) for L in TC.ATTN_L_SHORT if L <= 128] + [("long", L) for L in TC.ATTN_L_LONG])


@pytest.mark.parametrize("kernel,L", ATTN_PARAMS)
def test_attention_vs_f64(kernel, L):
    """attention_kernel<1..6> (attn_qb = 0), attention_qb_kernel<1..4> (attn_qb = 1, L <= 128) and attention_long_kernel (L > 192) alone
    against the float64 definition in the five score regimes of text_kernel_cases.attn_input: lens = [L, inside a tile / chunk, 1], padded
    keys that would win the softmax with V = +-100 behind them, junk in [L, ld), a second row stride at L = 33 / 129 / 257; nothing is
    written outside [0, L) of the launch's rows; an utterance alone gets the bits it has in the batch; a row with lens = 0 is all zeros."""
    lib = _clib()
    prev = lib.cmtts_attention_set_qb(1 if kernel == "qb" else 0)
    try:
        worst = 0.0
        for case in TC.ATTN_CASES:
            d, d32, ratio = 0.0, 0.0, 0.0
            for ld in TC.attn_lds(L):
                qkv, lens = TC.attn_input(L, ld, case)
                ref, c32, floor = TC.attn_reference(L, ld, case)
                got = _attention(lib, qkv, lens, L, ld)
                one = _attention(lib, qkv[1:2], lens[1:2], L, ld)
                assert np.array_equal(one[0], got[1]), (case, ld, "utterance 1 alone differs from its rows in the batch")
                e = float(np.abs(got - ref).max())
                if e / max(c32, floor) >= ratio:
                    d, d32, ratio = e, c32, e / max(c32, floor)
            report(f"ATTN_F64 {kernel} L={L} {case}: |d| {d:.2e}, d32 {d32:.2e}, ratio {ratio:.2f}")
            worst = max(worst, ratio)
            assert ratio <= ATTN_M[kernel], (case, d, d32, ratio)
        # a row without a valid key: zeros, the other rows as before
        ld = TC.attn_lds(L)[0]
        qkv, lens = TC.attn_input(L, ld, "unit", True)
        ref, d32, floor = TC.attn_reference(L, ld, "unit", True)
        got = _attention(lib, qkv, lens, L, ld)
        assert not got[2].any(), "lens = 0: the row is not all zeros"
        assert np.abs(got - ref).max() <= ATTN_M[kernel] * max(d32, floor)
    finally:
        lib.cmtts_attention_set_qb(prev)


# ----------------------------------------------------------------------------------------------------------------- conv_xres.hip

@pytest.fixture(scope="module")
def packed():
    """The weights of the three launches as the packers behind cmtts_internal_pack_weights lay them out, on the device."""
    def pack(layout, p):
        s = _lib.internal_pack_weights(layout, p)
        assert s is not None, layout
        return _dev(s.view(np.float32))
    out = {}
    for name, (M, taps, seed) in {"qkv": (768, 1, 11), "out": (256, 1, 12), "ffn": (1024, 9, 13)}.items():
        w, b = TC.xres_weights(M, taps, seed)
        out[name] = {"kmajor": _dev(TC.kmajor(w)), "iter": pack("fragment_iter_order", TC.kmajor(w)), "bias": _dev(b)}
    w, _ = TC.xres_weights(1024, 9, 13)
    out["ffn"]["f23"] = pack("wino23_xres_fragments", TC.kmajor(w))
    out["ffn"]["f43"] = pack("wino43_xres_fragments", TC.kmajor(w))
    out["w2"] = pack("fragment_iter_order", np.ascontiguousarray(TC.ffn2_weights().T)[None])      # [1][K = 1024][M2 = 256]
    g, be = TC.ln_params()
    out["ln"] = (_dev(g), _dev(be))
    return out


class _ForcedTiles:
    def __init__(self, lib, nt):
        self.lib, self.nt = lib, nt

    def __enter__(self):
        self.prev = self.lib.cmtts_xres_set_nt(self.nt)

    def __exit__(self, *exc):
        self.lib.cmtts_xres_set_nt(self.prev)
        return False


def _guarded(rows, ld, fill=None):
    """[B + 2][rows][ld] holding SENTINEL (or `fill` [B][rows][ld] in rows 1 .. B): the launch writes rows 1 .. B."""
    t = torch.full((TC.XRES_B + 2, rows, ld), TC.SENTINEL, device=DEV)
    if fill is not None:
        t[1:-1] = _dev(fill)
    return t


def _untouched(t, N, before=None):
    got = _np(t)
    assert (got[0] == TC.SENTINEL).all() and (got[-1] == TC.SENTINEL).all(), "written outside the launch's rows"
    assert np.array_equal(got[1:-1, ..., N:], np.full_like(got[1:-1, ..., N:], TC.SENTINEL) if before is None else before[..., N:]), "written beyond N"
    return got[1:-1, ..., :N]


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("N", TC.XRES_N)
def test_xres_qkv_vs_f64(packed, N, nt):
    """Launch 1 of an FFT block: the QKV in-projection (K = 256, M = 768, one tap) with LayerNorm1 as the prologue, with and without
    ln_lens (columns >= ln_lens[z] come out as the projection of 0), 32- and 96-column tiles."""
    lib = _clib()
    P = packed["qkv"]
    lens = TC.xres_lens(N)
    lens_d = _dev(lens)
    worst = (0.0, 0.0, 0.0)
    with _ForcedTiles(lib, nt):
        for ld in TC.xres_lds(N):
            x = TC.xres_input(N, ld)
            xd = _dev(x)
            for masked in (False, True):
                y = _guarded(768, ld)
                a = TC.conv_args(xd.data_ptr(), N, ld, TC.XRES_K * ld, y[1:].data_ptr(), ld, 768 * ld, N, 768, TC.XRES_K, 1, P["bias"].data_ptr())
                a.A = P["kmajor"].data_ptr()
                a.ln_g, a.ln_b, a.ln_eps = packed["ln"][0].data_ptr(), packed["ln"][1].data_ptr(), TC.LN_EPS
                a.ln_lens = lens_d.data_ptr() if masked else None
                assert lib.cmtts_launch_conv_xres(C.byref(a), C.c_void_p(P["iter"].data_ptr()), TC.XRES_B, None) == 0
                torch.cuda.synchronize()
                got = _untouched(y, N)
                for b in range(TC.XRES_B):
                    n = int(lens[b]) if masked else None
                    ref = TC.qkv_def(x[b], N, np.float64, n)
                    d32 = TC.yardstick(ref, TC.qkv_def(x[b], N, np.float32, n))
                    e = float(np.abs(got[b] - ref).max())
                    worst = max(worst, (e / d32, e, d32))
                    if masked:
                        assert np.array_equal(got[b][:, n:], np.broadcast_to(_np(P["bias"])[:, None], (768, N - n))), "masked columns are not the projection of 0"
    report(f"XRES_F64 qkv N={N} nt={nt}: |d| {worst[1]:.2e}, d32 {worst[2]:.2e}, ratio {worst[0]:.2f}")
    assert worst[0] <= XRES_M["qkv"], worst


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("N", TC.XRES_N)
def test_xres_outproj_vs_f64(packed, N, nt):
    """Launch 2: the out-projection (K = 256, M = 256) with bias, alpha, the residual in place (res == Y) and out of place, and lens
    (columns >= lens are written as 0)."""
    lib = _clib()
    P = packed["out"]
    lens = TC.xres_lens(N)
    lens_d = _dev(lens)
    worst = (0.0, 0.0, 0.0)
    with _ForcedTiles(lib, nt):
        for ld in TC.xres_lds(N):
            x = TC.xres_input(N, ld)
            res = np.ascontiguousarray(x[::-1]) * np.float32(0.5)
            xd = _dev(x)
            for in_place in (False, True):
                y = _guarded(256, ld, res if in_place else None)
                rd = y[1:] if in_place else _dev(res)
                a = TC.conv_args(xd.data_ptr(), N, ld, TC.XRES_K * ld, y[1:].data_ptr(), ld, 256 * ld, N, 256, TC.XRES_K, 1, P["bias"].data_ptr())
                a.A = P["kmajor"].data_ptr()
                o = a.out[0]
                o.alpha, o.res, o.r_zs0, o.ldr, o.lens = TC.OUT_ALPHA, rd.data_ptr(), 256 * ld, ld, lens_d.data_ptr()
                assert lib.cmtts_launch_conv_xres(C.byref(a), C.c_void_p(P["iter"].data_ptr()), TC.XRES_B, None) == 0
                torch.cuda.synchronize()
                got = _untouched(y, N, res if in_place else None)
                for b in range(TC.XRES_B):
                    ref = TC.outproj_def(x[b], res[b], N, np.float64, lens[b])
                    d32 = TC.yardstick(ref, TC.outproj_def(x[b], res[b], N, np.float32, lens[b]))
                    e = float(np.abs(got[b] - ref).max())
                    worst = max(worst, (e / d32, e, d32))
                    assert not got[b][:, int(lens[b]):].any(), "columns >= lens are not 0"
    report(f"XRES_F64 out N={N} nt={nt}: |d| {worst[1]:.2e}, d32 {worst[2]:.2e}, ratio {worst[0]:.2f}")
    assert worst[0] <= XRES_M["out"], worst


FFN_ARMS = (("direct", "iter", 0), ("f23", "f23", 2), ("f43", "f43", 1))      # (definition's form, packed stream, cmtts_launch_conv_xresq's form)


def _ffn_args(packed, xd, N, ld, scratch, part):
    P = packed["ffn"]
    a = TC.conv_args(xd.data_ptr(), N, ld, TC.XRES_K * ld, scratch.data_ptr(), ld, 1024 * ld, N, 1024, TC.XRES_K, 9, P["bias"].data_ptr())
    a.A = P["kmajor"].data_ptr()
    a.out[0].alpha, a.out[0].act = TC.FFN_ALPHA, TC.ACT_GELU_ERF
    a.ln_g, a.ln_b, a.ln_eps = packed["ln"][0].data_ptr(), packed["ln"][1].data_ptr(), TC.LN_EPS
    a.w2frag, a.part = packed["w2"].data_ptr(), part[1:].data_ptr()
    a.part_zs0, a.part_zs1, a.part_ld, a.M2 = 8 * 256 * ld, 256 * ld, ld, 256
    return a


def _ffn_launch(lib, packed, a, stream_name, form):
    wf = C.c_void_p(packed["ffn"][stream_name].data_ptr())
    if form == 0:
        return lib.cmtts_launch_conv_xres(C.byref(a), wf, TC.XRES_B, None)
    return lib.cmtts_launch_conv_xresq(C.byref(a), wf, TC.XRES_B, None, form)


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("N", TC.XRES_N)
def test_xres_ffn_vs_f64(packed, N, nt):
    """Launch 3: the fused FFN launch (k = 9 conv behind LayerNorm2, k^-1/2, GELU, the FFN linear's eight K-segment partials) in its three
    forms — direct, F(2,3) pairs, F(4,3) quads — against W2 gelu((conv + b) k^-1/2) in float64 (the partials added in float64: the reduction
    kernel is not under test) and against the float32 restatement of each form's own products; once (N = 130) with ln_lens and
    ln_skip_tiles: tiles wholly beyond ln_lens[z] keep the sentinel, every other column matches."""
    lib = _clib()
    lens = TC.xres_lens(N)
    lens_d = _dev(lens)
    worst = {arm: (0.0, 0.0, 0.0) for arm, _, _ in FFN_ARMS}
    own = {arm: 0.0 for arm, _, _ in FFN_ARMS}
    with _ForcedTiles(lib, nt):
        for ld in TC.xres_lds(N):
            x = TC.xres_input(N, ld)
            xd = _dev(x)
            scratch = torch.zeros((TC.XRES_B, 1024, ld), device=DEV)
            for skip in ((False, True) if N == 130 else (False,)):
                refs = [TC.ffn_def(x[b], N, np.float64, "direct", int(lens[b]) if skip else None) for b in range(TC.XRES_B)]
                d32 = [TC.yardstick(refs[b], TC.ffn_def(x[b], N, np.float32, "direct", int(lens[b]) if skip else None)) for b in range(TC.XRES_B)]
                for arm, stream_name, form in FFN_ARMS:
                    part = torch.full((TC.XRES_B + 2, 8, 256, ld), TC.SENTINEL, device=DEV)
                    a = _ffn_args(packed, xd, N, ld, scratch, part)
                    if skip:
                        a.ln_lens, a.ln_skip_tiles = lens_d.data_ptr(), 1
                    assert _ffn_launch(lib, packed, a, stream_name, form) == 0
                    torch.cuda.synchronize()
                    parts = _untouched(part, N)                                   # [B][8][256][N]
                    for b in range(TC.XRES_B):
                        n_live = N
                        if skip:      # column tiles of 32 nt that start beyond ln_lens[b] (and not at 0) are not written
                            bn = 32 * nt
                            n_live = min(N, -(-int(lens[b]) // bn) * bn)
                            assert (parts[b][:, :, n_live:] == TC.SENTINEL).all(), "a skipped tile was written"
                        got = parts[b][:, :, :n_live].astype(np.float64).sum(0)
                        assert np.isfinite(got).all()
                        e = float(np.abs(got - refs[b][:, :n_live]).max())
                        worst[arm] = max(worst[arm], (e / d32[b], e, d32[b]))
                        mine = TC.ffn_def(x[b], N, np.float32, arm, int(lens[b]) if skip else None)[:, :n_live]
                        own[arm] = max(own[arm], float(np.abs(got - mine).max()) / d32[b])
    report(f"XRES_F64 ffn N={N} nt={nt}: ratio direct / F(2,3) / F(4,3) " + " / ".join(f"{worst[arm][0]:.2f}" for arm, _, _ in FFN_ARMS) +
           f" (|d| " + " / ".join(f"{worst[arm][1]:.2e}" for arm, _, _ in FFN_ARMS) + f", d32 {max(w[2] for w in worst.values()):.2e}); vs own fp32 products " +
           " / ".join(f"{own[arm]:.2f}" for arm, _, _ in FFN_ARMS))
    for arm, _, _ in FFN_ARMS:
        assert worst[arm][0] <= XRES_M["ffn_" + arm], (arm, worst[arm])
        assert own[arm] <= XRES_M_OWN["ffn_" + arm], (arm, own[arm])


def test_xres_refusals(packed):
    """Shapes the X-resident kernels do not take are refused (-2) by both launchers, not mangled."""
    lib = _clib()
    N, ld = 33, 36
    xd = _dev(TC.xres_input(N, ld))
    scratch = torch.zeros((TC.XRES_B, 1024, ld), device=DEV)
    part = torch.full((TC.XRES_B + 2, 8, 256, ld), TC.SENTINEL, device=DEV)

    def both(a):
        return (_ffn_launch(lib, packed, a, "iter", 0), _ffn_launch(lib, packed, a, "f23", 2))

    a = _ffn_args(packed, xd, N, ld, scratch, part)
    a.dil = 2                                   # nine taps at dilation 2: a halo of 16 columns
    assert both(a) == (-2, -2)
    a = _ffn_args(packed, xd, N, ld, scratch, part)
    a.K = 288
    assert both(a) == (-2, -2)
    a = _ffn_args(packed, xd, N, ld, scratch, part)
    a.part = None                               # w2frag without a place for the partials
    assert both(a) == (-2, -2)
    torch.cuda.synchronize()
    assert (_np(part) == TC.SENTINEL).all()


# ----------------------------------------------------------------------------------------------------------------- flip rates

ARMS = ((0, 0), (0, 1), (1, 0), (1, 1))         # (ffn_wino, pred_wino); (1, 1) is the default


@pytest.mark.parametrize("variant", TC.FLIP_VARIANTS)
def test_flip_rate_of_the_four_arms(variant):
    """VERDICT r06 Next #2: the text and frame side (no denoiser) with the FFN conv direct / F(2,3) and the pitch predictor direct / F(4,3)
    against the FLOAT64 oracle on 4096 unsearched frames.  Per arm: every disagreeing duration, energy bucket and pitch bucket is off by one
    and sits on a boundary of the float64 pre-rounding value; the expected flip rate (mean |pre-rounding value - float64's| in buckets: for
    an error far below a bucket, the probability of landing in the other one) is at most FLIP_R x the float32 oracle's own."""
    from cmtts_amd import host
    cfg, sd, texts, lens, spk = TC.flip_inputs(variant)
    ref = TC.flip_oracle(variant, "f64")
    base = TC.flip_stats(variant, TC.flip_oracle(variant, "f32"))
    model = host.CMTotalTTS(cfg, DEV).load_state_dict(sd)
    stats = {}
    prev = (_lib.internal_set("ffn_wino", 1), _lib.internal_set("pred_wino", 1))
    try:
        for arm in ARMS:
            _lib.internal_set("ffn_wino", arm[0])
            _lib.internal_set("pred_wino", arm[1])
            out = model.duration_pitch_energy_net(None, torch.from_numpy(texts), torch.from_numpy(lens),
                                                  spker_embeds=None if spk is None else torch.from_numpy(spk), max_mel_len=TC.FLIP_T)
            torch.cuda.synchronize()
            got = {"log_d": _np(out["log_d_predictions"]), "d_rounded": _np(out["d_rounded"]), "e_pred": _np(out["e_predictions"]),
                   "e_idx": _np(out["e_idx"]), "f0_denorm": _np(out["p_predictions"]["f0_denorm"]), "p_idx": _np(out["p_predictions"]["p_idx"])}
            stats[arm] = TC.flip_stats(variant, got)
            # pitch: on a boundary as conftest.pitch_margin_mask defines it
            _, fr = TC.flip_masks(variant, got["d_rounded"], got["e_idx"])
            differs = (got["p_idx"] != ref["p_idx"]) & fr
            assert not (differs & pitch_margin_mask(ref["f0_denorm"], FLIP_MARGIN)).any(), (arm, "a pitch bucket differs away from a rounding boundary")
    finally:
        _lib.internal_set("ffn_wino", prev[0])
        _lib.internal_set("pred_wino", prev[1])
    for stage, margin in (("dur", DUR_MARGIN), ("energy", ENERGY_MARGIN), ("pitch", FLIP_MARGIN)):
        b = base[stage]
        report(f"FLIP_RATE {variant} {stage}: fp32 oracle {1e6 * b['rate']:.1f}, arms 00 / 01 / 10 / 11 " +
               " / ".join(f"{1e6 * stats[arm][stage]['rate']:.1f}" for arm in ARMS) + f" per million; observed fp32 oracle {b['n']}, arms " +
               " / ".join(str(stats[arm][stage]["n"]) for arm in ARMS) + f" of {b['of']}; largest error " +
               f"{max(s[stage]['max_err'] for s in stats.values()):.2e} buckets; {int((b['margins'] < margin).sum())} elements within {margin:g} of a boundary")
    for arm in ARMS:
        for stage, margin in (("dur", DUR_MARGIN), ("energy", ENERGY_MARGIN), ("pitch", FLIP_MARGIN)):
            s = stats[arm][stage]
            assert s["of"] == base[stage]["of"] or stage == "pitch"
            assert s["max_step"] <= 1, (arm, stage, "off by more than one")
            assert s["off_margin"] < margin, (arm, stage, s["off_margin"], "differs away from a boundary")
            assert s["rate"] <= FLIP_R * base[stage]["rate"], (arm, stage, s["rate"], base[stage]["rate"])
    for stage in ("dur", "energy", "pitch"):
        assert stats[(1, 1)][stage]["n"] <= base[stage]["n"] + 2, (stage, stats[(1, 1)][stage]["n"], base[stage]["n"])
