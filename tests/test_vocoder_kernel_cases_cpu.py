"""CPU: what tests/test_gpu_vocoder_kernels.py measures the vocoder's kernels against (tests/vocoder_kernel_cases.py) is itself right — the
definitions against the oracle's arithmetic, the argument blocks against the headers, the shape lists against the tile widths, the two-tap
stacking of the upsampler weights, and the accounting of 16-bit rounding flips that the fused kernels' bound rests on."""
import ctypes as C

import numpy as np
import pytest

from oracle import cmtts_oracle as O
import vocoder_kernel_cases as VC

F32, F64 = np.float32, np.float64


def _nchw(v):
    return np.asarray(v)[None]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_resblock_def_is_the_oracles_arithmetic(mode):
    """resblock_def in float64 = ResBlock.forward as O.hifigan_generator spells it (conv1d / quant16 / leaky_relu under precision("f64"), with and
    without operands16), to 1e-12; one pair of it = pair_def; one conv of it = conv_def."""
    Cc, k, T = 32, 7, 61
    ws = [VC.pair_weights(Cc, k, m) for m in range(3)]
    x = VC.signal(Cc, T)[0]
    with O.precision("f64"), O.operands16(VC.MODES[mode]):
        xr = _nchw(x.astype(F64))
        for m, dil in enumerate(VC.RB_DILS):
            w1, b1, w2, b2 = ws[m]
            xt = O.quant16(O.leaky_relu(xr, VC.SLOPE))
            xt = O.conv1d(xt, O.quant16(w1), b1, padding=(k * dil - dil) // 2, dilation=dil)
            if m == 0:
                first_xt = xt[0].copy()
            xt = O.quant16(O.leaky_relu(xt, VC.SLOPE))
            xt = O.conv1d(xt, O.quant16(w2), b2, padding=(k - 1) // 2)
            xr = xt + xr
            if m == 0:
                first = xr[0].copy()
    got = VC.resblock_def(x, ws, mode, F64)
    assert got.dtype == F64 and np.abs(got - xr[0]).max() <= 1e-12
    y, xt = VC.pair_def(x, *ws[0], 1, mode, F64)
    assert np.abs(y - first).max() <= 1e-12 and np.abs(xt - first_xt).max() <= 1e-12
    assert np.abs(VC.conv_def(x, ws[0][0], ws[0][1], 1, mode, F64) - first_xt).max() <= 1e-12
    y_old = VC.signal(Cc, T, 2)[0]
    assert np.abs(VC.resblock_def(x, ws, mode, F64, y_old) - (xr[0] + y_old)).max() <= 1e-12


@pytest.mark.parametrize("mode,pre_div", [(0, 1.0), (0, 3.0), (1, 1.0), (2, 1.0)])
def test_convT_def_is_the_oracles_arithmetic(mode, pre_div):
    """convT_def in float64 = x = ups[i](leaky_relu(x / num_kernels)) as O.hifigan_generator spells it (the upsamplers' operands rounded in bf16 / fp16),
    to 1e-12 — and evaluated through the two-tap stacked array it is the same sum."""
    ci, co, s = 64, 32, 2
    w, b = VC.convT_weights(ci, co, s)
    x = VC.signal(ci, 37, 3)[0]
    with O.precision("f64"), O.operands16(VC.MODES[mode]):
        a = O.leaky_relu(_nchw(x.astype(F64)) / F64(pre_div), VC.SLOPE)
        qu = O.quant16 if mode else (lambda v: v)
        ref = O.conv_transpose1d(qu(a), qu(w), b, s, (2 * s - s) // 2)[0]
    got = VC.convT_def(x, w, b, s, pre_div, mode, F64)
    assert got.shape == (co, 37 * s) and np.abs(got - ref).max() <= 1e-12
    assert np.abs(VC.convT_def(x, w, b, s, pre_div, mode, F64, stacked=True) - ref).max() <= 1e-12


@pytest.mark.parametrize("stage", range(4))
def test_stacked_upsampler_weights(stage):
    """stack_two_tap is pack_conv_transpose's [2][Cin][s Cout] array, row = phase Cout + co, and convT_def through it equals the plain transposed conv
    for all four stages (stride 8 and 2), one-column input included."""
    ci, co, s = VC.CONVT_STAGES[stage]
    w, b = VC.convT_weights(ci, co, s)
    st = VC.stack_two_tap(w, s)
    assert st.shape == (2, ci, s * co)
    for q, c, r, o in ((0, 0, 0, 0), (1, 3, s - 1, co - 1), (1, ci - 1, 1, 5), (0, 7, s // 2, 2)):
        assert st[q, c, r * co + o] == w[c, o, r + s * q]
    for Ti in (1, 5):
        x = VC.signal(ci, Ti, 3)[0]
        for mode in (0, 1, 3):
            plain = VC.convT_def(x, w, b, s, 3.0, mode, F64)
            assert np.abs(VC.convT_def(x, w, b, s, 3.0, mode, F64, stacked=True) - plain).max() <= 1e-12 * max(1.0, np.abs(plain).max())


def test_rounding_and_decoders():
    rs = np.random.RandomState(5)
    v = (rs.standard_normal(4096) * np.exp(rs.uniform(-12, 3, 4096))).astype(F32)
    for mode in (1, 2):
        q = VC.round16(v, mode)
        assert q.dtype == F32
        bits = (q.view(np.uint32) >> np.uint32(16)).astype(np.uint16) if mode == 1 else q.astype(np.float16).view(np.uint16)
        assert np.array_equal(VC.decode16(bits, mode), q)                       # what the device writes decodes to what the definition rounds to
        assert (np.abs(q.astype(F64) - v) <= 0.5 * VC.ulp16(v, mode)).all()      # round to nearest
        assert np.array_equal(VC.round16(v.astype(F64), mode), q.astype(F64))
    hi = v.astype(np.float16).astype(F32)
    assert np.array_equal(VC.round16(v, 3), hi + (v - hi).astype(np.float16).astype(F32))
    assert VC.round16(v, 0) is not None and np.array_equal(VC.round16(v, 0), v)
    assert VC.ulp16(1.0, 1) == 2.0 ** -7 and VC.ulp16(1.5, 2) == 2.0 ** -10 and VC.ulp16(0.75, 2) == 2.0 ** -11 and VC.ulp16(1e-6, 2) == 2.0 ** -24


def test_argument_blocks_match_the_headers():
    """The ctypes mirrors have the C structs' sizes and field offsets (LP64: resblock_pair.h has no packing pragma)."""
    P, X = VC.PairArgs, VC.ConvXlArgs
    assert C.sizeof(P) == 96
    assert (P.bstride.offset, P.B.offset, P.ld.offset, P.k.offset, P.dil.offset, P.accum.offset, P.slope.offset, P.dbg.offset) == (48, 56, 68, 72, 76, 80, 84, 88)
    assert C.sizeof(X) == 128
    assert (X.res.offset, X.bstride.offset, X.B.offset, X.k.offset, X.accum.offset, X.slope.offset, X.relu.offset, X.cin.offset, X.xbstride.offset,
            X.wino_force.offset, X.ln_g.offset, X.ln_b.offset, X.ln_eps.offset, X.row_split.offset) == (32, 40, 48, 64, 72, 76, 80, 84, 88, 96, 104, 112, 120, 124)
    assert C.sizeof(VC.ConvArgs) == 504


INSTANCES = ([("conv_xl", c, k, d, 0) for c in (128, 256) for k in (3, 7, 11) for d in (1, 3, 5)] +
             [("conv_xlw", c, k, d, 0) for c in (128, 256) for k in (3, 7, 11) for d in (1, 3, 5)] + [("conv_xlw", 64, k, d, 0) for k in (7, 11) for d in (1, 3, 5)] +
             [(kn, c, k, d, 1) for kn, cs in (("conv16", (32, 64, 128)), ("conv_xl16", (128, 256)), ("resblock_pair", (32, 64)), ("resblock_pair16", (32, 64)),
                                             ("resblock_pairw16", (128,)), ("resblock_pair16x3", (32, 64, 128)), ("conv_xl16x3", (256,)))
              for c in cs for k in (3, 7, 11) for d in (1, 3, 5)] +
             [("resblock16", c, k, 1, 1) for c in (32, 64) for k in (3, 7, 11)])


def test_shape_lists_cover_the_tile_edges():
    """Every instance's T list holds W - 1, W, W + 1, a one-column case, the reach and a length of more than two tiles; nothing above ~900 columns.
    The Ts that also run with ld = T + 3 are in the list, and there the second stride differs from the aligned one and is no multiple of 4; one of them is
    odd (the row stride of the 16-bit images too) and one belongs to a ragged T."""
    for kn, c, k, d, mode in INSTANCES:
        Wt, Ts = VC.tile_width(kn, c, k, d, mode), VC.t_list(kn, c, k, d, mode)
        assert {1, Wt - 1, Wt, Wt + 1, VC.reach_of(kn, k, d)} <= set(Ts), (kn, c, k, d)
        assert max(Ts) > 2 * Wt and max(Ts) <= 900 and min(Ts) == 1, (kn, c, k, d, Ts)
        tes = VC.t_extra_lds(kn, c, k, d, mode)
        assert len(set(tes)) == 2 and set(tes) <= set(Ts) and any(te % Wt for te in tes), (kn, c, k, d, tes)
        for te in tes:
            aligned, extra = VC.lds_of(te, True)
            assert aligned % 4 == 0 and extra == te + 3 and extra != aligned and extra % 4 != 0, (kn, c, k, d, te)
        assert any(VC.lds_of(te, True)[1] % 2 for te in tes), (kn, c, k, d, tes)
        assert set(VC.t_alone(kn, c, k, d, mode)) <= set(Ts) and 1 in VC.t_alone(kn, c, k, d, mode)
        assert len(VC.lds_of(Wt + 2, False)) == 1
    assert [VC.tile_width("resblock16", 64, k) for k in (3, 7, 11)] == [360, 312, 264]
    assert VC.tile_width("resblock_pair", 32, 11) == 246 and VC.tile_width("resblock_pair", 64, 3) == 126
    assert VC.tile_width("resblock_pair16x3", 32, 7) == 122 and VC.tile_width("resblock_pair16x3", 128, 7) == 90
    for kn, ci, mode in (("convT", 512, 0), ("convT16", 512, 3), ("convT16", 64, 1)):
        tile = VC.tile_width(kn, ci, 0, 1, mode)
        assert set(VC.ti_list(tile)) >= {1, 2, tile - 1, tile, tile + 1}
        for Ti in VC.ti_extra_lds(tile):
            assert Ti in VC.ti_list(tile)
            for s_ in (2, 8):
                assert (Ti + 3) % 4 and (Ti * s_ + 3) % 4 and Ti + 3 != (Ti + 3) // 4 * 4
        assert any((Ti + 3) % 2 for Ti in VC.ti_extra_lds(tile))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("Cc,k,dil", [(32, 3, 1), (64, 11, 5), (128, 7, 3)])
def test_rounding_flip_accounting(Cc, k, dil, mode):
    """The fused 16-bit kernels round xt on chip, where it carries fp32 error: an element close to a rounding midpoint may round the other way and
    move conv2's operand by a whole 16-bit ulp — hundreds of times the fp32 yardstick.  The bound M d32 + widen allows exactly that, element by
    element, and nothing else: the float32 evaluation of pair_def (which has such flips: 1 - 62 of them here) sits inside it, and max(widen) stays
    below 1 % of rms(y), so that the widened bound cannot hide a structural error (a wrong tap, a wrong halo column: those are of the size of y)."""
    T = 300
    e, yard = VC.pair_reference(Cc, k, 0, dil, T, mode, 0, T)
    err = np.abs(e["v32"].astype(F64) - e["ref"])
    assert (err <= VC.M * yard + e["widen"]).all(), float((err - VC.M * yard - e["widen"]).max())
    rms = float(np.sqrt((e["ref"] ** 2).mean()))
    assert 0.5 < rms < 2.5
    assert e["widen"].max() <= 0.01 * rms, (float(e["widen"].max()), rms)
    assert e["near"] >= e["flips32"]                          # every flipped element was marked
    # the no-flip yardstick is fp32 rounding of a C k-term sum of O(1) values, not a 16-bit ulp
    assert yard < 1e-5 and e["d32_xt"] < 1e-5
    if e["flips32"]:
        assert err.max() > VC.M * yard                        # without `widen` the float32 evaluation itself would fail: the term is needed


def test_fp16x3_lolo_term_is_small_and_sufficient():
    """fp16x3: operands of 22 bits, the omitted lo x lo products bounded by 2^-21 (|w| conv |x|): a sum of absolute values (7e-5 here, where the
    products themselves cancel to far less), held to the same 1 % of rms(y) as the 16-bit widening."""
    e, yard = VC.pair_reference(64, 7, 0, 3, 200, 3, 0, 200)
    assert (np.abs(e["v32"].astype(F64) - e["ref"]) <= VC.M * yard + e["widen"]).all()
    assert 0 < e["widen"].max() <= 0.01 * float(np.sqrt((e["ref"] ** 2).mean()))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_the_bound_catches_structural_errors(mode):
    """What the issue names as able to hide in rounding noise does not fit under M d32 + widen: xt not zeroed outside [0, T) (conv2 then reads
    conv1's bias-driven values there), one tap of conv2 shifted by a column at a tile edge, and one halo column of x missing."""
    Cc, k, dil, T = 32, 3, 1, 300
    ws = VC.pair_weights(Cc, k, 0)
    e, yard = VC.pair_reference(Cc, k, 0, dil, T, mode, 0, T)
    bound = VC.M * yard + e["widen"][0]
    x = VC.signal(Cc, T)[0]
    # (1) the pair evaluated on a zero-extended x and cropped: xt outside [0, T) is conv1 of zeros + b1, not zero
    R = 4
    wide = VC.pair_def(np.pad(x, ((0, 0), (R, R))), *ws, dil, mode, F64)[0][:, R:R + T]
    # (2) conv2's last tap reads one column to the right for the outputs of the column before a 254-column tile edge
    xt = VC.pair_def(x, *ws, dil, mode, F64)[1]
    a2 = VC.round16(VC.leaky(xt, F64), mode)
    shifted = e["ref"][0].copy()
    w2q = VC.round16(np.asarray(ws[2], F64), mode)
    shifted[:, 253] += w2q[:, :, 2] @ (a2[:, 255] - a2[:, 254])
    # (3) x column 254 (the first halo column of the second tile) read as zero by conv1
    xz = x.copy()
    xz[:, 254] = 0
    halo = VC.pair_def(xz, *ws, dil, mode, F64)[0]
    halo[:, 254] += x[:, 254]                                 # (the residual read is another load: it stays right)
    for name, bad in (("xt outside [0, T)", wide), ("tap at a tile edge", shifted), ("halo column", halo)):
        over = np.abs(bad - e["ref"][0]) - bound
        assert over.max() > 100 * VC.M * yard, (name, float(over.max()))
