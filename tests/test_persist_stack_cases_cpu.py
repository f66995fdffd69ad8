"""CPU: what tests/test_gpu_persist_stack.py measures the persistent denoiser stack against (tests/persist_stack_cases.py) is itself right — the
ctypes mirrors of persist_args.h against the layout the built library reports, the chained definition and the tail against the oracle's residual
loop and skip head, the shape lists against the tile width, and that six plausible mistakes of a persistent kernel or its launcher move the
definition by far more than the GPU module's bound."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from cmtts_amd import _lib
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict
from oracle import cmtts_oracle as O
import denoiser_kernel_cases as DC
import persist_stack_cases as PC
import vocoder_kernel_cases as VC

F32, F64 = np.float32, np.float64
CH = PC.CH


def test_argument_blocks_match_the_built_library():
    """ctypes.sizeof and the field offsets of the PostRow / PersistGroup / PersistArgs mirrors equal sizeof / offsetof as the library's own compiler
    laid persist_args.h out (cmtts_internal_persist_args_layout: host only, the library loads without a GPU).  PersistArgs travels by value."""
    lib = C.CDLL(_lib.LIB_PATH)
    lib.cmtts_internal_persist_args_layout.restype = C.c_int
    lib.cmtts_internal_persist_args_layout.argtypes = [C.POINTER(C.c_size_t), C.c_int]
    want = PC.mirror_layout()
    n = lib.cmtts_internal_persist_args_layout(None, 0)
    assert n == len(want) == 3 + len(PC.LAYOUT_ARGS_FIELDS) + len(PC.LAYOUT_GROUP_FIELDS)
    out = (C.c_size_t * n)()
    assert lib.cmtts_internal_persist_args_layout(out, n) == n
    assert list(out) == want, (list(out), want)
    assert C.sizeof(PC.PostRow) == 16 and want[2] > 8 * PC.MAX_GROUPS * 8 + 4 * PC.MAX_WG      # grp[8] and desc[256] are inside
    short = (C.c_size_t * 2)(77, 77)
    assert lib.cmtts_internal_persist_args_layout(short, 1) == n and list(short) == [16, 77]     # writes no more than it is given room for


def test_descriptor_and_chunk_helpers():
    """desc_word's bit fields as persist_args.h states them; chunks_expected: the launchers' balanced chunks at the shapes of the chunk tests."""
    w = PC.desc_word(5, 700, 101, 200)
    assert (w & 7, w >> 3 & 1023, w >> 13 & 127, w >> 20 & 255) == (5, 700, 101, 200)
    assert PC.chunks_expected(3, 65, 2) == [1, 1, 1] and PC.chunks_expected(3, 65, 4) == [2, 1]
    assert PC.chunks_expected(3, 129, 7) == [2, 1] and PC.chunks_expected(3, 129, 256) == [3] and PC.chunks_expected(40, 512, 256) == [20, 20]


def test_shape_lists_cover_the_tile_edges():
    """Every instance runs T below, at and above one and two 64-frame tiles and the one-, two- and three-column cases at NL = 3; F(4,3) every residue
    mod 4 at the start and behind a full tile; NL = 1 and 2 at T = 1, 65, 129."""
    for inst in PC.INSTANCES:
        full = PC.t_list(inst, 3)
        assert {1, 2, 3, 63, 64, 65, 127, 128, 129} <= set(full) and max(full) == PC.T_MAX
        assert PC.t_list(inst, 1) == PC.t_list(inst, 2) == (1, 65, 129)
        assert len(PC.shapes(inst)) == len(full) + 6
    f43 = PC.t_list("f43", 3)
    assert {1, 2, 3, 5, 6, 7} <= set(f43) and {t % 4 for t in f43 if 64 <= t < 68} == {0, 1, 2, 3}
    for T in (1, 65, 129):
        _, _, m2p, pix = PC.fact_case(T)
        if T > 8:
            assert {0, 1, PC.EXPAND_L, PC.EXPAND_L + 5} <= set(m2p.ravel()) and {-1, 0, PC.EXPAND_LD2 - 1, PC.EXPAND_LD2 + 3} <= set(pix.ravel())
        p1n, p2n, p1t, p2t, _, _ = PC.fact_tables(T, PC.B, 2)
        assert p1n.shape == (PC.B, 2 * CH, PC.EXPAND_LDP) and p2n.shape == (3 * CH, PC.EXPAND_LD2) and (p2n[2 * CH:] == PC.GARBAGE).all()
        assert p1t[1, 1, 5, 9] == p1n[1, CH + 9, 5] and p2t[1, 3, 200] == p2n[CH + 200, 3]
        a = PC.alloc_layers(PC.stack_inputs(T)[1], 2)
        assert a.shape == (PC.B, 3 * CH, T) and (a[:, 2 * CH:] == PC.GARBAGE).all() and np.array_equal(a[:, :2 * CH], PC.stack_inputs(T)[1][:, :2 * CH])


def test_stack_and_tail_defs_are_the_oracles_arithmetic():
    """stack_def followed by tail_def (c_out = 1, nothing added) in float64 = O.denoiser_forward's residual loop and skip head under precision("f64")
    on a three-layer single-speaker state dict that carries stack_weights(3) and tail_weights(), to 1e-12 relative: the input projection, the
    step embedding and the conditioner projections are formed by the oracle's own functions and handed to stack_def as x0, d (= dp) and cp."""
    cfg = dataclasses.replace(get_config("LJSpeech"), res_layers=3)
    sd = {k: np.asarray(v) for k, v in synth_cmtts_state_dict(cfg, seed=7).items()}
    ws, (Ws, bs, Wp, bp) = PC.stack_weights(3), PC.tail_weights()
    for l, (W3, b3, Wo, bo) in enumerate(ws):
        p = f"net.residual_layers.{l}."
        for k, v in (("conv_layer.conv.weight", W3), ("conv_layer.conv.bias", b3), ("output_projection.conv.weight", Wo[:, :, None]),
                     ("output_projection.conv.bias", bo)):
            assert sd[p + k].shape == v.shape, (k, sd[p + k].shape)
            sd[p + k] = v
    for k, v in (("net.skip_projection.conv.weight", Ws[:, :, None]), ("net.skip_projection.conv.bias", bs),
                 ("net.output_projection.conv.weight", Wp[:, :, None]), ("net.output_projection.conv.bias", bp)):
        assert sd[k].shape == v.shape, (k, sd[k].shape)
        sd[k] = v
    T, Bn = 37, 2
    rs = np.random.RandomState(21)
    x, cond = rs.standard_normal((Bn, 1, T, PC.MEL)).astype(F32), rs.standard_normal((Bn, T, cfg.hidden)).astype(F32)
    t = np.asarray([300.0, -120.0], F32)
    with O.precision("f64"):
        want = O.denoiser_forward(sd, cfg, x, t, cond, None)[:, 0]
        h = np.maximum(O.conv1d(x[:, 0].transpose(0, 2, 1), sd["net.input_projection.0.conv.weight"], sd["net.input_projection.0.conv.bias"]), 0)
        e = O.diffusion_embedding(t, CH)
        e = O.linear(O.mish(O.linear(e, sd["net.mlp.0.linear.weight"])), sd["net.mlp.2.linear.weight"])
        d = np.concatenate([O.linear(e, sd[f"net.residual_layers.{l}.diffusion_projection.linear.weight"]) for l in range(3)], axis=1)
        cp = np.concatenate([O.conv1d(cond.transpose(0, 2, 1), sd[f"net.residual_layers.{l}.conditioner_projection.conv.weight"],
                                      sd[f"net.residual_layers.{l}.conditioner_projection.conv.bias"]) for l in range(3)], axis=1)
    assert want.dtype == F64 and h.dtype == F64 and d.shape == (Bn, 3 * CH) and cp.shape == (Bn, 3 * CH, T)
    skip = np.stack([PC.stack_def(h[b], cp[b], d[b], d[b], ws, 0, F64)[0] for b in range(Bn)])
    rows = np.asarray([[1.0, 0.0, 0.0, 0]] * Bn)
    # (div: under precision("f64") the oracle divides by the float64 sqrt(3); the kernels' and tail_def's divisor is the float32 one, 4e-8 away)
    got = PC.tail_def(skip, 3, Ws, bs, Wp, bp, None, None, rows, F64, div=np.sqrt(3.0))
    near = PC.tail_def(skip, 3, Ws, bs, Wp, bp, None, None, rows, F64)
    assert 0 < np.abs(near - got).max() < 1e-6
    assert got.shape == want.shape == (Bn, T, PC.MEL)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), np.abs(got - want).max()
    # the post-scaling on top of it: c_out F + c_skip xold + noise nstd 0.85 where bit 0 is set, and not where it is clear
    xold, noise = rs.standard_normal((Bn, T, PC.MEL)).astype(F32), rs.standard_normal((Bn, T, PC.MEL)).astype(F32)
    rows = np.asarray([[0.5, 0.25, 2.0, PC.POSTROW_RENOISE], [0.5, 0.25, 2.0, PC.POSTROW_FINAL]])
    got = PC.tail_def(skip, 3, Ws, bs, Wp, bp, xold, noise, rows, F64, div=np.sqrt(3.0))
    assert np.abs(got[0] - (0.5 * want[0] + 0.25 * xold[0] + noise[0].astype(F64) * 2.0 * F64(F32(0.85)))).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(got[1] - (0.5 * want[1] + 0.25 * xold[1])).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_the_16_bit_chain_is_block_def(mode):
    """stack_def's 16-bit layers take their weights rounded once per layer (persist_stack_cases._block16): the same bits as DC.block_def chained, in
    float64 and in float32."""
    T = 9
    x0, cp, dp, d = PC.stack_inputs(T)
    ws = PC.stack_weights(2)
    for dt in (F64, F32):
        got = PC.stack_def(x0[1], cp[1], dp[1], d[1], ws, mode, dt)
        x, skip = x0[1], None
        for l, (W3, b3, Wo, bo) in enumerate(ws):
            s = slice(l * CH, (l + 1) * CH)
            _, _, x, skip = DC.block_def(x, cp[1][s], dp[1][s], d[1][s], W3, b3, Wo, bo, skip, mode, dt)
        assert got[0].dtype == dt and np.array_equal(got[0], skip) and np.array_equal(got[1], x)
    assert not np.array_equal(got[0], PC.stack_def(x0[1], cp[1], dp[1], d[1], ws, 0, F32)[0])


def test_yardsticks_are_fp32_noise_on_outputs_of_a_few_units():
    """The yardsticks of the three-layer stack are a few 1e-6 on a skip sum of a few units for every instance (the bound M yard is a few 1e-5), the
    Winograd yardsticks are not below the direct one, fp16x3's carries the 22-bit operand model and is of the same size as fp32's."""
    yd = {}
    for inst in ("direct", "f43", "f23", "fp16x3"):
        ref, yard = PC.stack_reference(inst, 3, 65)
        assert 2.0 < np.abs(ref).max() < 10.0 and 1e-6 < yard < 2e-5, (inst, np.abs(ref).max(), yard)
        yd[inst] = yard
    assert yd["f43"] >= yd["direct"] and yd["f23"] >= yd["direct"]
    e = PC._stack_eval("fp16x3", 3, 65)
    assert 0.0 < e["model"] <= yd["fp16x3"] < 3 * yd["direct"]
    ref, yard = PC.tail_reference("direct", 3, 65, "full")
    assert ref.shape == (PC.B, 65, PC.MEL) and 1e-7 < yard < 2e-5


def _tile_conv(halo_of):
    """A k = 3 conv evaluated 64-frame tile by tile; halo_of(t0, n) -> (left, right) columns [C] next to the tile, or None for zeros."""
    def conv(u, w3):
        T = u.shape[1]
        outs = []
        for t0 in range(0, T, PC.FN):
            n = min(PC.FN, T - t0)
            pad = np.zeros((u.shape[0], n + 2), F64)
            pad[:, 1:n + 1] = u[:, t0:t0 + n]
            lr = halo_of(t0, n)
            if lr is not None:
                pad[:, 0], pad[:, -1] = lr
            outs.append(VC.conv_same(pad, w3, 1, F64)[:, 1:n + 1])
        return np.concatenate(outs, axis=1)
    return conv


def _layers(x0, cp, dp, d, ws, conv_of):
    """stack_def in float64 with layer l's conv replaced by conv_of(l, us) (None: the right one); us = the conv operands u of the layers so far."""
    x, skip, us = x0, None, []
    for l, (W3, b3, Wo, bo) in enumerate(ws):
        s = slice(l * CH, (l + 1) * CH)
        us.append(DC.u_def(x, cp[s], dp[s], 0, F64))
        _, _, x, skip = DC.block_def(x, cp[s], dp[s], d[s], W3, b3, Wo, bo, skip, 0, F64, conv_of(l, us))
    return skip


@pytest.mark.parametrize("T", [65, 129])
def test_wrong_kernels_move_the_definition_far_beyond_the_bound(T):
    """Six mistakes of a persistent kernel or its launcher, restated through the definitions at NL = 3: the weights of layers 1 and 2 swapped; the
    neighbour's column lost at the tile seam in layers >= 1; a stale halo (layer 2 reads layer 0's edge columns: the granule slots alternate by layer
    parity); skip / NL for skip / sqrt(NL) in the tail; NL C T taken as cp's batch stride (utterance 1 then starts in utterance 0's garbage layer);
    a trim to one tile ignored (frames < 64 of the T-frame evaluation against the definition at T = 64).  Each moves the skip sum (the tail's
    output) by more than 100 x the GPU module's bound M x yard."""
    NL, i = 3, 1
    ws = PC.stack_weights(NL)
    x0, cp, dp, d = PC.stack_inputs(T)
    ref, yard = PC.stack_reference("direct", NL, T)
    bound = VC.M * yard
    right = PC.stack_def(x0[i], cp[i], dp[i], d[i], ws, 0, F64)[0]
    assert np.array_equal(right, ref[i])
    assert np.array_equal(_layers(x0[i], cp[i], dp[i], d[i], ws, lambda l, us: None), ref[i])
    moved = {}
    moved["weights swapped"] = np.abs(PC.stack_def(x0[i], cp[i], dp[i], d[i], (ws[0], ws[2], ws[1]), 0, F64)[0] - ref[i]).max()
    seam = _layers(x0[i], cp[i], dp[i], d[i], ws, lambda l, us: _tile_conv(lambda t0, n: None) if l >= 1 else None)
    moved["seam column lost"] = np.abs(seam - ref[i]).max()
    assert np.abs(seam - ref[i])[:, :60].max() < bound        # (and only near the seam: three layers reach three columns)

    def stale(l, us):
        if l < 2:
            return None
        old = us[l - 2]
        col = lambda t: old[:, t] if 0 <= t < T else np.zeros(CH)
        return _tile_conv(lambda t0, n: (col(t0 - 1), col(t0 + n)))
    moved["stale halo"] = np.abs(_layers(x0[i], cp[i], dp[i], d[i], ws, stale) - ref[i]).max()
    flat = PC.alloc_layers(cp, NL).reshape(-1)[i * NL * CH * T:][:NL * CH * T].reshape(NL * CH, T)
    moved["NL C T as the batch stride"] = np.abs(PC.stack_def(x0[i], flat, dp[i], d[i], ws, 0, F64)[0] - ref[i]).max()
    assert min(moved.values()) > 100 * bound, (T, moved, bound)

    tref, tyard = PC.tail_reference("direct", NL, T, "full")
    xold, noise = PC.post_inputs(T)
    rows = PC.tail_post("full", PC.B)[0]
    wrong = PC.tail_def(ref, NL, *PC.tail_weights(), xold, noise, rows, F64, div=float(NL))
    assert np.abs(wrong - tref).max() > 100 * VC.M * tyard, (T, "skip / NL", np.abs(wrong - tref).max(), tyard)

    cut, cyard = PC.stack_reference("direct", NL, T, PC.B, False, PC.FN)
    assert cut.shape == (PC.B, CH, PC.FN)
    assert np.abs(ref[:, :, :PC.FN] - cut).max() > 100 * VC.M * cyard, (T, "trimming ignored", np.abs(ref[:, :, :PC.FN] - cut).max(), cyard)
    assert np.abs(ref[:, :, :PC.FN - NL] - cut[:, :, :PC.FN - NL]).max() < VC.M * cyard     # frames further than NL from the cut do not see it
