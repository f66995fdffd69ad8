"""CPU: what tests/test_gpu_denoiser_kernels.py measures the denoiser's kernels against (tests/denoiser_kernel_cases.py) is itself right — the
definitions against the oracle's arithmetic, the gate permutation against the tile layout the kernels use, the argument blocks against the headers,
the shape lists against the tile widths, the accounting of 16-bit rounding flips of z that the 16-bit block's bound rests on, and that three
plausible kernel mistakes move the definition by far more than the GPU module's bound."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from oracle import cmtts_oracle as O
import denoiser_kernel_cases as DC
import vocoder_kernel_cases as VC

F32, F64 = np.float32, np.float64
CH = DC.CH


def _layer(variant):
    cfg = dataclasses.replace(get_config(variant), res_layers=1)
    sd = synth_cmtts_state_dict(cfg, seed=7)
    p = "net.residual_layers.0."
    return cfg, {k[len(p):]: np.asarray(v) for k, v in sd.items() if k.startswith(p)}


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_block_def_is_the_oracles_arithmetic(mode):
    """block_def in float64 = one residual layer as O.denoiser_forward spells it (conv1d / quant16 / sigmoid / linear under precision("f64"), with and
    without operands16), to 1e-12, on a one-layer state dict of the multi-speaker model (dp = d + p); proj_def = its second half.  In the 16-bit modes
    the oracle's lines get the operand the kernels have — round16 of the float32 value of cp + (x + dp) — and that value is bit for bit the one the
    float32 oracle forms ((h + d) + cp, single speaker: the same two float32 additions)."""
    cfg, L = _layer("VCTK")
    T = 37
    rs = np.random.RandomState(11)
    h, cp = rs.standard_normal((1, CH, T)).astype(F32), rs.standard_normal((1, CH, T)).astype(F32)
    e, spk = rs.standard_normal((1, CH)).astype(F32), rs.standard_normal((1, cfg.hidden)).astype(F32)
    skip_old = rs.standard_normal((CH, T)).astype(F32)
    W3, b3, Wo3, bo = L["conv_layer.conv.weight"], L["conv_layer.conv.bias"], L["output_projection.conv.weight"], L["output_projection.conv.bias"]
    d32 = O.linear(e, L["diffusion_projection.linear.weight"]).astype(F32)
    p32 = O.linear(spk, L["speaker_projection.linear.weight"]).astype(F32)
    dp32 = (d32 + p32).astype(F32)
    dp_arg = dp32[0] if mode else d32[0].astype(F64) + p32[0].astype(F64)      # fp32 form: the exact d + p, as the oracle adds the two terms
    with O.precision("f64"), O.operands16(VC.MODES[mode]):
        d = d32.astype(F64)[:, :, None]
        r = h.astype(F64) + d
        if mode:
            u = (cp + (h + dp32[:, :, None])).astype(F32)      # float32 arithmetic: the kernels' operand
        else:
            u = r + cp.astype(F64) + p32.astype(F64)[:, :, None]
        y = O.conv1d(O.quant16(u), O.quant16(W3), b3, padding=1)
        z = O.sigmoid(y[:, :CH]) * np.tanh(y[:, CH:])
        o = O.conv1d(O.quant16(z), O.quant16(Wo3), bo)
        x_new = (o[:, :CH] + r) / F64(math.sqrt(2.0))
        skip = o[:, CH:]
    gy, gz, gx, gs = DC.block_def(h[0], cp[0], dp_arg, d32[0], W3, b3, Wo3[:, :, 0], bo, None, mode, F64)
    assert gy.dtype == F64 and gx.dtype == F64
    for got, ref in ((gy, y), (gz, z), (gx, x_new), (gs, skip)):
        assert np.abs(got - ref[0]).max() <= 1e-12
    assert np.abs(DC.block_def(h[0], cp[0], dp_arg, d32[0], W3, b3, Wo3[:, :, 0], bo, skip_old, mode, F64)[3] - (skip[0] + skip_old)).max() <= 1e-12
    px, ps, _ = DC.proj_def(DC.stage_z(gz, mode, F64), h[0], d32[0], Wo3[:, :, 0], bo, None, F64, mode)
    assert np.array_equal(px, gx) and np.array_equal(ps, gs)
    # the float32 oracle's own u (single speaker: dp = d) is the operand u_def rounds
    r32 = (h + d32[:, :, None]).astype(F32)
    assert np.array_equal((r32 + cp).astype(F32)[0], DC.u_def(h[0], cp[0], d32[0], 0, F32))
    if mode:
        assert np.array_equal(DC.u_def(h[0], cp[0], d32[0], mode, F64), VC.round16((r32 + cp)[0], mode).astype(F64))


def test_input_side_defs_are_the_oracles_arithmetic():
    """inproj_def = relu(conv1d(transpose(c_in x))) and cond_def = the conditioner projection with quant16 operands, as O.denoiser_forward spells them;
    expand_def against a loop over its elements with the kernel's stated clamps."""
    cfg, L = _layer("LJSpeech")
    sd = synth_cmtts_state_dict(dataclasses.replace(get_config("LJSpeech"), res_layers=1), seed=7)
    rs = np.random.RandomState(12)
    T = 29
    x_tm = rs.standard_normal((1, T, DC.MEL)).astype(F32)
    Wi, bi = np.asarray(sd["net.input_projection.0.conv.weight"]), np.asarray(sd["net.input_projection.0.conv.bias"])
    with O.precision("f64"):
        ref = np.maximum(O.conv1d((F64(F32(0.37)) * x_tm.astype(F64)).transpose(0, 2, 1), Wi, bi), 0)
    assert np.abs(DC.inproj_def(x_tm[0], F32(0.37), Wi[:, :, 0], bi, F64) - ref[0]).max() <= 1e-12
    c = rs.standard_normal((1, CH, T)).astype(F32)
    Wc, bc = L["conditioner_projection.conv.weight"], L["conditioner_projection.conv.bias"]
    for mode in (0, 1, 2, 3):
        with O.precision("f64"), O.operands16(VC.MODES[mode]):
            ref = O.conv1d(O.quant16(c.astype(F64)), O.quant16(Wc), bc)
        assert np.abs(DC.cond_def(c[0], Wc[:, :, 0], bc, mode, F64) - ref[0]).max() <= 1e-12
    for T in (1, 5, 64):
        p1, p2, m2p, pix = DC.expand_case(T)
        for b in range(DC.B):
            got = DC.expand_def(p1[b], p2, m2p[b], pix[b], DC.EXPAND_L, DC.EXPAND_LD2)
            for t in range(T):
                ph, ix = min(int(m2p[b, t]), DC.EXPAND_L), min(max(int(pix[b, t]), 0), DC.EXPAND_LD2 - 1)
                want = (p1[b][:, ph - 1] if ph > 0 else np.zeros(DC.EXPAND_M, F32)) + p2[:, ix]
                assert np.array_equal(got[:, t], want.astype(F32))
    for T in DC.EXPAND_T[1:]:
        _, _, m2p, pix = DC.expand_case(T)
        assert {0, 1, DC.EXPAND_L, DC.EXPAND_L + 5} <= set(m2p.ravel()) and {-1, 0, DC.EXPAND_LD2 - 1, DC.EXPAND_LD2 + 3} <= set(pix.ravel())


@pytest.mark.parametrize("n", [16, 32])
def test_gate_perm_is_the_tile_layout(n):
    """gate_perm(n) is a permutation of the 2 C rows, and packed 2 n-row tile w holds [n sigmoid rows | n tanh rows] of channels n w .. n w + n - 1 —
    what puts a channel's two gate operands into one lane (n = 16: registers r and r + 8 of a 32-row MFMA tile)."""
    perm = DC.gate_perm(n)
    assert np.array_equal(np.sort(perm), np.arange(2 * CH))
    assert np.array_equal(perm, [(r // n % 2) * CH + r // (2 * n) * n + r % n for r in range(2 * CH)])      # import.hip's expression
    for w in range(CH // n):
        tile = perm[2 * n * w:2 * n * (w + 1)]
        assert np.array_equal(tile[:n], np.arange(n * w, n * w + n)) and np.array_equal(tile[n:], CH + np.arange(n * w, n * w + n))
    km = DC.permuted_kmajor(DC.block_weights()[0], n)
    assert km.shape == (3, CH, 2 * CH) and km[2, 5, 3 * n + 1] == DC.block_weights()[0][perm[3 * n + 1], 5, 2]


def test_argument_blocks_match_the_headers():
    """The ctypes mirrors have the C structs' sizes and field offsets (LP64; resblock_args.h, cond_gemm.h and inproj.h have no packing pragma): the
    numbers a host-only sizeof / offsetof compile of the three headers prints."""
    R, G, I = DC.ResArgs, DC.CondGemmArgs, DC.InProjArgs
    assert C.sizeof(R) == 144
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 100, 104, 112, 120, 128, 136]
    assert C.sizeof(G) == 64
    assert [getattr(G, f).offset for f, _ in G._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56]
    assert C.sizeof(I) == 80
    assert [getattr(I, f).offset for f, _ in I._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 72]


def test_shape_lists_cover_the_tile_edges():
    """Every T list has a T below, at and above one and two tiles of its kernel, the one-, two- and three-column cases; the F(4,3) list has every residue
    mod 4 at the start and behind a full tile; nothing above 131 (cond_expand: 260, both vector widths and a ragged tile of each)."""
    for kn, Wt in DC.TILE.items():
        Ts = DC.t_list(kn)
        assert {1, 2, 3, Wt - 1, Wt, Wt + 1, 2 * Wt - 1, 2 * Wt, 2 * Wt + 1} <= set(Ts) and max(Ts) <= 131, (kn, Ts)
        assert set(DC.t_alone(kn)) <= set(Ts)
    q = DC.t_list("w43")
    assert {t % 4 for t in q} == {0, 1, 2, 3} and {1, 2, 3, 5, 6, 7} <= set(q)
    assert {t - 64 for t in q if 64 <= t <= 67} == {0, 1, 2, 3}
    for Ts, Wt in ((DC.INPROJ_T, 64), (DC.COND_T, 64)):
        assert {1, Wt - 1, Wt, Wt + 1, 2 * Wt + 1} <= set(Ts) and max(Ts) <= 131
    assert {1, 63, 64, 65} <= set(DC.EXPAND_T) and {256, 257, 260} <= set(DC.EXPAND_T) and max(DC.EXPAND_T) == 260
    assert any(t % 4 == 0 and t > 256 for t in DC.EXPAND_T) and any(t % 4 for t in DC.EXPAND_T)
    assert np.array_equal(DC.seam_columns(65, 32), [0, 31, 32, 63, 64]) and np.array_equal(DC.seam_columns(1, 32), [0])


def test_gate_grid():
    """The grid holds every ordered pair of the +- points as (g, f) of some (channel, frame), all finite, and the identity weights make y = u."""
    x = DC.gate_grid()
    assert x.shape == (CH, DC.GATE_T) and np.isfinite(x).all() and np.abs(x).max() == 1e4
    g, f = x[:CH // 2].ravel(), x[CH // 2:].ravel()
    have = set(zip(g.tolist(), f.tolist()))
    pts = [float(F32(s * p)) for p in DC.GATE_POINTS for s in (1.0, -1.0)]
    assert all((a, b) in have for a in pts for b in pts)
    assert ((np.abs(g) <= 8) & (np.abs(f) <= 8)).sum() >= 300
    W3, b3 = DC.gate_identity_weights()
    y = VC.conv_same(x.astype(F64), W3, 1, F64)
    assert np.array_equal(y[:CH], x) and np.array_equal(y[CH:], np.roll(x, -CH // 2, axis=0)) and not b3.any()


@pytest.mark.parametrize("mode", [1, 2])
def test_widening_is_small_against_the_output(mode):
    """The 16-bit block's bound is M d32 + widen (z elements that may round the other way on chip).  At every T of the list, with and without the
    skip accumulation: max(widen) <= 1 % of rms(o), on the reference alone — the widening cannot swallow an error of the size a wrong kernel makes."""
    for T in DC.t_list("lp"):
        for accum in (False, True):
            e, _ = DC.block_reference(T, mode, accum, max(DC.t_list("lp")))
            worst = max(e["widen_x"].max() * math.sqrt(2.0), e["widen_skip"].max())
            assert worst <= 0.01 * e["o_rms"], (mode, T, worst, e["o_rms"])
    assert (np.abs(DC.block_reference(65, mode, False, 129)[0]["z"]) < 0.9).mean() > 0.8      # the gate is mostly unsaturated on these weights


def test_wrong_kernels_move_the_definition_far_beyond_the_bound():
    """Three mistakes a kernel could make, restated through block_def at T = W + 1 (W = 32 and 64): the right halo not zeroed beyond T (the conv reads
    a clamped copy of column T - 1), d swapped for dp in the residual, C * T used as cp's batch stride (utterance 1 reads another layer's rows).  Each
    moves x_out or skip by more than 100 x the GPU module's bound M x yard."""
    W3, b3, Wo, bo = DC.block_weights()
    for T in (33, 65):
        x, cp_all, dp_all, d_all, _ = DC.block_inputs(T)
        cp, dp, d = DC.layer_slices(cp_all, dp_all, d_all)
        e, yard = DC.block_reference(T, 0, False, 129)
        bound = VC.M * max(yard["x"], yard["skip"])
        i = 1
        right = lambda a: np.concatenate([a, a[:, -1:]], axis=1)
        _, _, xh, sh = DC.block_def(right(x[i]), right(cp[i]), dp[i], d[i], W3, b3, Wo, bo, None, 0, F64)
        halo = max(np.abs(xh[:, :T] - e["x"][i]).max(), np.abs(sh[:, :T] - e["skip"][i]).max())
        _, _, xs, _ = DC.block_def(x[i], cp[i], dp[i], dp[i], W3, b3, Wo, bo, None, 0, F64)
        swap = np.abs(xs - e["x"][i]).max()
        cp_flat = cp_all.reshape(-1)[DC.LAYER * CH * T + i * CH * T:][:CH * T].reshape(CH, T)
        _, _, xc, _ = DC.block_def(x[i], cp_flat, dp[i], d[i], W3, b3, Wo, bo, None, 0, F64)
        stride = np.abs(xc - e["x"][i]).max()
        assert min(halo, swap, stride) > 100 * bound, (T, halo, swap, stride, bound)
