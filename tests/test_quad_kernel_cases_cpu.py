"""CPU: what tests/test_gpu_quad_kernels.py measures the F(4,3) quad kernels against (tests/quad_kernel_cases.py, oracle/winograd_ref.py) is itself
right — the restatements of the forms' own products against the plain conv in float64, the shape lists against the tile widths and residue classes,
the argument blocks against the header, that the bound M x yard catches the structural mistakes these kernels can make, and that the spiky case's
yardstick stays within 100 x the plain case's."""
import ctypes as C

import numpy as np
import pytest

from oracle import winograd_ref as W
import quad_kernel_cases as QC
import vocoder_kernel_cases as VC

F32, F64 = np.float32, np.float64


def _small(cout, cin, k, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((cout, cin, k)) / np.sqrt(cin * k), rs.standard_normal(cout)


@pytest.mark.parametrize("k,dil", [(k, d) for k in QC.XLQ_K for d in QC.DILS] + [(5, 1)])
def test_restatement_is_the_plain_conv_in_float64(k, dil):
    """conv1d_f43_taps_dil (every residue class through conv1d_f43_taps) = conv1d_direct to 1e-12 of the output, at every T of the instance's list:
    T = 1, T below the reach, ragged quads, a second tile with a partial set of classes."""
    w, _ = _small(6, 4, k, 10 * k + dil)
    kernel = "conv_k5q" if k == 5 else "conv_xlq"
    Ts = QC.t_list(kernel, k, dil)
    assert 1 in Ts and (QC.reach_of(kernel, k, dil) == 1 or any(1 < T <= QC.reach_of(kernel, k, dil) for T in Ts))
    for T in Ts:
        x = np.random.RandomState(T).standard_normal((4, T))
        ref = W.conv1d_direct(x, w, dil)
        got = W.conv1d_f43_taps_dil(x, w, dil)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (k, dil, T)


@pytest.mark.parametrize("dil", QC.DILS)
def test_pair_restatement_is_pair_def_in_float64(dil):
    """pair_f43 (the chain of the two restatements) = vocoder_kernel_cases.pair_def to 1e-12, xt too, at every T of the pair's list (T = 1, 2 and the
    reach: xt outside [0, T) decides the answer)."""
    w1, b1 = _small(8, 8, 3, 100 + dil)
    w2, b2 = _small(8, 8, 3, 200 + dil)
    for T in QC.t_list("conv_xlq_pair", 3, dil):
        x = np.random.RandomState(50 + T).standard_normal((8, T))
        y, xt = W.pair_f43(x, w1, b1, w2, b2, dil, VC.SLOPE)
        ry, rxt = VC.pair_def(x, w1, b1, w2, b2, dil, 0, F64)
        assert np.abs(xt - rxt).max() <= 1e-12 * max(1.0, np.abs(rxt).max()), (dil, T)
        assert np.abs(y - ry).max() <= 1e-12 * max(1.0, np.abs(ry).max()), (dil, T)


def test_k5q_def_is_layernorm_then_conv():
    """k5q_def in float64 = the older parity test's expression (numpy mean / var over the 256 channels, then conv1d_direct, bias, ReLU); its F(4,3)
    evaluation is the same function to 1e-12."""
    w, b = QC.k5q_weights(256)
    x = QC.k5q_input(256, 37)[0]
    g, be = QC.TC.ln_params()
    x64 = x.astype(F64)
    h = (x64 - x64.mean(0)) / np.sqrt(x64.var(0) + 1e-12) * g[:, None] + be[:, None]
    ref = np.maximum(W.conv1d_direct(h, w.astype(F64), 1) + b[:, None], 0.0)
    assert np.abs(QC.k5q_def(x, w, b, True, True, F64) - ref).max() <= 1e-12
    assert np.abs(QC.k5q_def(x, w, b, True, True, F64, f43=True) - ref).max() <= 1e-12
    plain = W.conv1d_direct(x64, w.astype(F64), 1) + b[:, None]
    assert np.abs(QC.k5q_def(x, w, b, False, False, F64) - plain).max() <= 1e-12


def test_shape_lists_cover_the_tile_edges():
    """Every instance's T list holds 1, 2, 3, the reach, W - 1, W, W + 1, more than two tiles, and all four residues mod 4 both in W - 1 .. W + 2 and in
    1 .. 4-column inputs or the reach; at dilation 3 / 5 second tiles that hold some residue classes and not others, and W + dil + 1, where class 0 has
    one entry more than the rest.  The T + 3 strides are unaligned, one of them odd."""
    inst = ([("conv_xlq", k, d) for k in QC.XLQ_K for d in QC.DILS] + [("conv_xlq_pair", 3, d) for d in QC.DILS] + [("conv_k5q", 5, 1)])
    for kn, k, d in inst:
        Wt, r, Ts = QC.tile_width(kn, d), QC.reach_of(kn, k, d), QC.t_list(kn, k, d)
        assert {1, 2, 3, r, Wt - 1, Wt, Wt + 1, 2 * Wt + r + 1} <= set(Ts), (kn, k, d)
        assert {T % 4 for T in Ts if Wt - 1 <= T <= Wt + 2} == {0, 1, 2, 3}, (kn, k, d)
        assert max(Ts) > 2 * Wt and max(Ts) <= 200 and min(Ts) == 1, (kn, k, d, Ts)
        if d > 1:
            assert any(0 < T - Wt < d for T in Ts), (kn, k, d, "no second tile with a partial set of classes")
            assert Wt + d + 1 in Ts
        tes = QC.t_extra_lds(kn, d)
        assert len(set(tes)) == 2 and set(tes) <= set(Ts) and any(te % Wt for te in tes)
        for te in tes:
            aligned, extra = QC.lds_of(te, True)
            assert aligned % 4 == 0 and extra == te + 3 and extra % 4 != 0
        assert any(QC.lds_of(te, True)[1] % 2 for te in tes)
        assert set(QC.t_alone(kn, d)) <= set(Ts) and QC.t_alone(kn, d) == (1, Wt + 1)
    assert [QC.tile_width("conv_xlq", d) for d in QC.DILS] == [64, 60, 60]
    assert [QC.tile_width("conv_xlq_pair", d) for d in QC.DILS] == [60, 56, 56]
    assert [QC.class_entries(d) for d in (3, 5)] == [20, 12] and all(QC.class_entries(d) % 4 == 0 for d in (3, 5))
    assert QC.reach_of("conv_xlq", 11, 5) == 25 and QC.reach_of("conv_xlq_pair", 3, 5) == 6 and QC.reach_of("conv_k5q", 5) == 2


def test_argument_blocks_match_the_header():
    """ConvXlArgs and PairArgs as resblock_pair.h declares them (LP64), ln_g .. row_split included."""
    X, P = QC.ConvXlArgs, QC.PairArgs
    assert C.sizeof(X) == 128 and C.sizeof(P) == 96
    assert [f[0] for f in X._fields_] == ["x", "y", "wf", "bias", "res", "bstride", "B", "C", "T", "ld", "k", "dil", "accum", "slope", "relu", "cin", "xbstride",
                                          "wino_force", "ln_g", "ln_b", "ln_eps", "row_split"]
    assert (X.cin.offset, X.xbstride.offset, X.wino_force.offset, X.ln_g.offset, X.ln_b.offset, X.ln_eps.offset, X.row_split.offset) == (84, 88, 96, 104, 112, 120, 124)
    assert (X.ln_g.size, X.ln_b.size, X.ln_eps.size, X.row_split.size) == (8, 8, 4, 4)
    assert [f[0] for f in P._fields_] == ["x", "y", "w1f", "b1", "w2f", "b2", "bstride", "B", "C", "T", "ld", "k", "dil", "accum", "slope", "dbg"]
    assert (P.w2f.offset, P.bstride.offset, P.dil.offset, P.accum.offset, P.slope.offset) == (32, 48, 76, 80, 84)


def test_the_bound_catches_structural_errors():
    """The four mistakes these kernels can make without the older checks noticing, restated on the definition at T = W + 1: each moves the output by more
    than 100 x M x yard.  (1) the class-major scatter at dilation 3 one entry off (every class's subsequence one entry late: x[t - dil] where x[t]
    belongs); (2) the pair's xt outside [0, T) taken as conv1(0) + b1; (3) k = 7's single tap accumulated into M3, which all four outputs of a quad
    read with weights 1, 2, 4, 8, where it belongs in M5, which y3 alone reads; (4) the LayerNorm prologue applied to a padding column (it then
    enters the conv as beta)."""
    # (1)
    Cc, k, dil = 64, 3, 3
    T, Tmax = QC.tile_width("conv_xlq", dil) + 1, QC.t_list("conv_xlq", k, dil)[-1]
    w, b = QC.weights(Cc, Cc, k, 0)
    x = QC.signal(Cc, T)[0]
    ref, yard = QC.xlq_reference(Cc, k, dil, T, False, False, Tmax)
    late = np.zeros_like(x)
    late[:, dil:] = x[:, :-dil]
    moved = {"class-major scatter": (np.abs(QC.conv_def(late, w, b, dil, 0, F64) - ref[0]).max(), yard)}
    # (2)
    dil = 1
    T, Tmax = QC.tile_width("conv_xlq_pair", dil) + 1, QC.t_list("conv_xlq_pair", 3, dil)[-1]
    ws = QC.pair_weights(Cc, 3, 0)
    x = QC.signal(Cc, T)[0]
    ref, yard = QC.pair_reference(Cc, dil, T, False, Tmax)
    wide = QC.pair_def(np.pad(x, ((0, 0), (4, 4))), *ws, dil, 0, F64)[0][:, 4:4 + T]
    moved["xt outside [0, T)"] = (np.abs(wide - ref[0]).max(), yard)
    # (3)
    k, dil = 7, 1
    T, Tmax = QC.tile_width("conv_xlq", dil) + 1, QC.t_list("conv_xlq", k, dil)[-1]
    w, b = QC.weights(Cc, Cc, k, 0)
    x = QC.signal(Cc, T)[0]
    ref, yard = QC.xlq_reference(Cc, k, dil, T, False, False, Tmax)
    Tq = -(-T // 4) * 4
    xp = np.pad(QC.leaky(x, F64), ((0, 0), (3, Tq - T + 8)))
    q0 = np.arange(0, Tq, 4)
    P = w[:, :, 6].astype(F64) @ (xp[:, q0 + 9] - xp[:, q0 + 7])      # g (x3 - x1), x_i = X[4 q + 6 + i]
    bad = np.zeros((Cc, Tq))
    bad[:, :T] = ref[0]
    for c, f in enumerate((1.0, 2.0, 4.0, 7.0)):                       # M3 reaches y0 .. y3 as 1, 2, 4, 8; y3 loses the 1 it had through M5
        bad[:, q0 + c] += f * P
    moved["k = 7's single tap in M3"] = (np.abs(bad[:, :T] - ref[0]).max(), yard)
    # (4)
    T, Tmax = QC.tile_width("conv_k5q") + 1, QC.t_list("conv_k5q", 5)[-1]
    w, b = QC.k5q_weights(256)
    x = QC.k5q_input(256, T)[0]
    ref, _, yard = QC.k5q_reference(256, True, True, T, Tmax)
    moved["LayerNorm of a padding column"] = (np.abs(QC.k5q_def(x, w, b, True, True, F64, ln_cols=T + 3) - ref[0]).max(), yard)
    for name, (d, yard) in moved.items():
        assert d > 100 * QC.M * yard, (name, d, yard)
        assert yard < 2e-5, (name, yard)


@pytest.mark.parametrize("k", QC.XLQ_K)
@pytest.mark.parametrize("Cc", QC.XLQ_C)
def test_spiky_yard_stays_within_100_plain_yards(Cc, k):
    """The spiky input (one sample in 64 times 100) at T = W + 1: its yardstick is at most 100 x the plain case's of the same instance, so that the
    yardstick cannot swallow a real error; the spikes are there (|x| > 100) and the plain signal has none."""
    for dil in QC.DILS:
        T = QC.tile_width("conv_xlq", dil) + 1
        x, ref, yard = QC.xlq_spiky_reference(Cc, k, dil, T)
        _, plain = QC.xlq_reference(Cc, k, dil, T, False, False, QC.t_list("conv_xlq", k, dil)[-1])
        assert np.abs(x).max() > 100 and np.abs(QC.signal(Cc, T)).max() < 10
        assert 0.5 / 64 < (np.abs(x) > 10).mean() < 2.0 / 64
        assert plain < yard <= 100 * plain, (Cc, k, dil, yard, plain)
