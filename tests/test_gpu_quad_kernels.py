"""The three Winograd F(4,3) kernels that work on output QUADS, called ALONE through their launch hooks (cm-tts_amd/csrc/resblock_pair.h) against the
float64 definition of the same operation (tests/quad_kernel_cases.py): conv_xlq_kernel (most ResBlock convs of the fp32 generator, 27 instances),
conv_xlq_pair3_kernel (its k = 3 pairs at C = 64 / 128, 6 instances) and conv_k5q_kernel (the frame-level pitch predictor's k = 5 convs, 3 instances
x ReLU on / off x four row splits).  The weight streams come from the production packer (weight_pack.cpp: to_wino43_iter_fragments through
_lib.internal_pack_weights); the Python restatement of that packing stays with the three older tests of tests/test_gpu_parity.py.

  A  conv_xlq: plain, with the residual, with y += and with both, against float64; plain launches also against the float32 restatement of the form's
     own products (oracle.winograd_ref.conv1d_f43_taps_dil); a spiky input (one sample in 64 times 100) once per instance
  B  conv_xlq_pair: with and without y +=, against pair_def in float64 and against the chain of two conv_xlq launches (fp32 Winograd rounding apart:
     the fused tile's conv1 quads start one frame earlier), both within the same bound
  C  conv_k5q: ReLU on and off, C_in = 128 as a slice of a wider allocation with its own xbstride; row splits 0 / 1 / 2 / 4 bit for bit; against
     float64 (LayerNorm over the frames inside [0, T) only) and against the float32 restatement
  D  refusals: what a launcher's header excludes returns -2 and writes nothing

at T in {1, 2, 3, reach, W - 1, W, W + 1, W + 2, 2 W + reach + 1} of every instance's own tile width W (W - 1 .. W + 2: every residue mod 4; dilation
3 / 5 also W + dil + 1), B = 2.  Output rows sit between sentinel rows, x between rows of GARBAGE, GARBAGE lies behind T in x and in the residual;
rows of T + 3 floats at W and at its ragged neighbour.  Utterance 1 alone, and the launch repeated behind one on inputs 1e4 times larger, at T = 1 and
T = W + 1 with aligned rows.

M = 10 for every kernel (vocoder_kernel_cases.M) — not set by what the kernels give.  yard = the largest of the d32 of the definition's direct
float32 evaluation, the d32 of the float32 F(4,3) restatement, both at the instance's largest T, and 4 ulps of the output.  That a wrong kernel
fails here is shown on the CPU (tests/test_quad_kernel_cases_cpu.py::test_the_bound_catches_structural_errors).  Every instance's worst ratio is in
the parity report (QUAD_F64 lines); the worst per kernel as measured on MI355X: below the imports."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from conftest import report
import quad_kernel_cases as QC
from test_gpu_vocoder_kernels import Worst, _alone_and_stale, _dev, _guard, _np, _rows, _untouched, _variants  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
M = QC.M
# Worst |kernel - float64| / yard per kernel over all its instances, T, row strides and epilogues, as measured on MI355X (the bound is M = 10 throughout;
# yard is 1.3e-6 .. 1.6e-5 on outputs of a few units, 2e-5 .. 2.6e-4 on the spiky input's outputs of up to a few hundred).  No launcher refused a T or a
# row stride of the lists.
#   conv_xlq 5.40 (C = 128, k = 11, d = 5, T = 146, ld = 148: |d| 7.51e-6 on a yard of 1.39e-6; 1.0 .. 2.9 at dilation 1, 1.0 .. 4.1 at dilation 3,
#   1.1 .. 5.4 at dilation 5; k = 3 at dilation 1 has ratio 1.00 at every C: there the largest error is the restatement's own); against the
#   restatement of its own products 5.61 (C = 128, k = 7, d = 5, T = 59, ld = 60); the spiky input 7.53 (C = 256, k = 11, d = 5, T = 61, ld = 64:
#   |d| 2.46e-4, yard 3.26e-5; 0.95 .. 5.8 at dilation 1 / 3, 2.2 .. 7.5 at dilation 5)
#   conv_xlq_pair 1.36 (C = 64, d = 1, T = 59, ld = 60); against the two conv_xlq launches 1.68 (C = 64, d = 3, T = 117, ld = 120, y +=)
#   conv_k5q 1.56 (C_in = 256 with LayerNorm, no ReLU, T = 131, ld = 132); against the restatement 1.51 (C_in = 256, T = 65, ld = 68); the four row
#   splits the same bits at every T
#   refusals: the 21 excluded arguments all return -2 — x == y in cmtts_launch_conv_xlq only since the guard that came with this module

LAUNCHERS = ("cmtts_launch_conv_xlq", "cmtts_launch_conv_xlq_pair", "cmtts_launch_conv_k5q")


def _clib():
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    for f in LAUNCHERS:
        getattr(lib, f).restype = C.c_int
    return lib


class WorstQ(Worst):
    def line(self, name):
        r, e, y, T, ld = self.w
        assert self.n >= len(self.core), (name, "nothing was compared")
        ref = f"; refused (-2): {self.refused}" if self.refused else ""
        report(f"QUAD_F64 {name}: |d| {e:.2e}, yard {y:.2e}, ratio {r:.2f} at T={T} ld={ld}{ref}")
        return r


def _core(kernel, dil=1):
    Wt = QC.tile_width(kernel, dil)
    return (Wt - 1, Wt, Wt + 1)


_CACHE = {}


def _frag43(cout, cin, k, seed):
    """The (cout, cin, k, seed) weights as weight_pack.cpp: to_wino43_iter_fragments streams them, on the device."""
    key = ("q", cout, cin, k, seed)
    if key not in _CACHE:
        s = _lib.internal_pack_weights("wino43_iter_fragments", QC.kmajor(QC.weights(cout, cin, k, seed)[0]), 0)
        assert s is not None, key
        _CACHE[key] = _dev(s)
    return _CACHE[key].data_ptr()


def _vec(key, make):
    if key not in _CACHE:
        _CACHE[key] = _dev(make())
    return _CACHE[key].data_ptr()


def _bias(cout, cin, k, seed):
    return _vec(("b", cout, cin, k, seed), lambda: QC.weights(cout, cin, k, seed)[1])


def _between(v, ld, rows=None, at=0):
    """v [Bn][C][T] -> a device buffer [Bn + 2][rows][ld] of GARBAGE with v in utterances 1 .. Bn, channels at .. at + C, columns 0 .. T; and the
    view of v's first element."""
    Bn, Cc, T = v.shape
    t = torch.full((Bn + 2, rows or Cc, ld), QC.GARBAGE, device=DEV)
    t[1:-1, at:at + Cc, :T] = _dev(v)
    return t, t[1:, at:]


def _finish(rc, y, y0, T, finite):
    torch.cuda.synchronize()
    if rc == -2:
        _untouched(y, y0)
        return None
    assert rc == 0, rc
    return _rows(y, T, finite)


def _xlq(lib, x, ld, k, dil, seed=0, res=None, y0=None, finite=True, force=1):
    """One cmtts_launch_conv_xlq on x [Bn][C][T] -> [Bn][C][T], or None if refused."""
    Bn, Cc, T = x.shape
    xd, xv = _between(x, ld)
    rd, rv = (None, None) if res is None else _between(res, ld)
    y = _guard(Bn, Cc, ld, y0)
    a = QC.ConvXlArgs(x=xv.data_ptr(), y=y[1:].data_ptr(), wf=_frag43(Cc, Cc, k, seed), bias=_bias(Cc, Cc, k, seed), res=None if rv is None else rv.data_ptr(),
                      bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, accum=int(y0 is not None), slope=0.1, wino_force=force)
    return _finish(lib.cmtts_launch_conv_xlq(C.byref(a), None), y, y0, T, finite)


def _pair(lib, x, ld, dil, y0=None, finite=True):
    """One cmtts_launch_conv_xlq_pair with the weights of pair 0 of the (C, 3) instance."""
    Bn, Cc, T = x.shape
    xd, xv = _between(x, ld)
    y = _guard(Bn, Cc, ld, y0)
    a = QC.PairArgs(x=xv.data_ptr(), y=y[1:].data_ptr(), w1f=_frag43(Cc, Cc, 3, 0), b1=_bias(Cc, Cc, 3, 0), w2f=_frag43(Cc, Cc, 3, 1), b2=_bias(Cc, Cc, 3, 1),
                    bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=3, dil=dil, accum=int(y0 is not None), slope=0.1)
    return _finish(lib.cmtts_launch_conv_xlq_pair(C.byref(a), None), y, y0, T, finite)


def _k5q(lib, x, ld, ln, relu, split, finite=True):
    """One cmtts_launch_conv_k5q on x [Bn][cin][T] -> [Bn][256][T].  C_in = 128: x is channels 64 .. 191 of a 256-channel allocation of GARBAGE and
    the launch gets that allocation's batch stride as xbstride."""
    Bn, cin, T = x.shape
    xd, xv = _between(x, ld, 256, 64 if cin == 128 else 0)
    y = _guard(Bn, 256, ld)
    g, be = QC.TC.ln_params()
    a = QC.ConvXlArgs(x=xv.data_ptr(), y=y[1:].data_ptr(), wf=_frag43(256, cin, 5, 0), bias=_bias(256, cin, 5, 0), bstride=256 * ld, B=Bn, C=256, T=T, ld=ld, k=5, dil=1,
                      slope=1.0, relu=int(relu), cin=0 if cin == 256 else cin, xbstride=256 * ld, wino_force=1, ln_g=_vec("ln_g", lambda: g) if ln else None,
                      ln_b=_vec("ln_b", lambda: be) if ln else None, ln_eps=QC.LN_EPS, row_split=split)
    return _finish(lib.cmtts_launch_conv_k5q(C.byref(a), None), y, None, T, finite)


# ----------------------------------------------------------------------------------------------------------------- A: conv_xlq

@pytest.mark.parametrize("k", QC.XLQ_K)
@pytest.mark.parametrize("Cc", QC.XLQ_C)
def test_conv_xlq_vs_f64(Cc, k):
    """conv_xlq_kernel<C, k, 1 / 3 / 5> alone: the four epilogue variants against float64; plain launches against the float32 restatement of the
    form's own products; one utterance alone and behind a launch 1e4 times larger; the spiky input at T = W + 1."""
    lib = _clib()
    for dil in QC.DILS:
        worst = WorstQ(_core("conv_xlq", dil))
        Ts = QC.t_list("conv_xlq", k, dil)
        for T in Ts:
            x, r, y0 = QC.signal(Cc, T), QC.signal(Cc, T, 1), QC.signal(Cc, T, 2)
            lds = QC.lds_of(T, T in QC.t_extra_lds("conv_xlq", dil))
            for ld in lds:
                run = lambda xx, rr=None, yy=None, finite=True: _xlq(lib, xx, ld, k, dil, 0, rr, yy, finite)
                for res, acc in _variants(r, y0):
                    got = run(x, res, acc)
                    if got is None:
                        worst.refuse(T, ld)
                        continue
                    ref, yard = QC.xlq_reference(Cc, k, dil, T, res is not None, acc is not None, Ts[-1])
                    worst.add(got - ref, yard, T, ld)
                    if res is None and acc is None:
                        own = float(np.abs(got - QC.xlq_own(Cc, k, dil, T)).max())
                        print(f"conv_xlq C={Cc} k={k} d={dil} T={T} ld={ld}: |own| {own:.2e} yard {yard:.2e}")
                        assert own <= M * yard, (dil, T, ld, own, yard, "differs from the restatement of its own products")
                    if T in QC.t_alone("conv_xlq", dil) and ld == lds[0]:
                        _alone_and_stale(run, x, got, res, acc)
            if T == QC.t_alone("conv_xlq", dil)[1]:
                xs, ref, yard = QC.xlq_spiky_reference(Cc, k, dil, T)
                got = _xlq(lib, xs, lds[0], k, dil)
                assert got is not None, (dil, T, "the spiky launch was refused")
                ratio = float(np.abs(got - ref).max()) / yard
                report(f"QUAD_F64 conv_xlq C={Cc} k={k} d={dil} spiky: |d| {ratio * yard:.2e}, yard {yard:.2e}, ratio {ratio:.2f} at T={T} ld={lds[0]}")
                assert ratio <= M, (dil, T, ratio, yard, "the spiky input")
        ratio = worst.line(f"conv_xlq C={Cc} k={k} d={dil}")
        assert ratio <= M, (dil, worst.w)


# ----------------------------------------------------------------------------------------------------------------- B: conv_xlq_pair

@pytest.mark.parametrize("dil", QC.DILS)
@pytest.mark.parametrize("Cc", QC.PAIR_C)
def test_conv_xlq_pair_vs_f64(Cc, dil):
    """conv_xlq_pair3_kernel<C, dil> alone, with and without y +=: against pair_def in float64 (T = 1, 2 and the reach: xt outside [0, T) decides the
    answer) and against the chain of two conv_xlq launches, both within M x yard."""
    lib = _clib()
    worst = WorstQ(_core("conv_xlq_pair", dil))
    Ts = QC.t_list("conv_xlq_pair", 3, dil)
    chain_worst = 0.0
    for T in Ts:
        x, y0 = QC.signal(Cc, T), QC.signal(Cc, T, 2)
        lds = QC.lds_of(T, T in QC.t_extra_lds("conv_xlq_pair", dil))
        for ld in lds:
            run = lambda xx, yy=None, finite=True: _pair(lib, xx, ld, dil, yy, finite)
            for acc in (None, y0):
                got = run(x, acc)
                if got is None:
                    worst.refuse(T, ld)
                    continue
                ref, yard = QC.pair_reference(Cc, dil, T, acc is not None, Ts[-1])
                worst.add(got - ref, yard, T, ld)
                xt = _xlq(lib, x, ld, 3, dil, 0)
                two = _xlq(lib, xt, ld, 3, 1, 1, res=x, y0=acc)
                assert xt is not None and two is not None, (T, ld, "conv_xlq refused a shape of the pair's list")
                d = float(np.abs(got - two).max())
                chain_worst = max(chain_worst, d / yard)
                print(f"conv_xlq_pair C={Cc} d={dil} T={T} ld={ld} accum={int(acc is not None)}: |pair - chain| {d:.2e} yard {yard:.2e}")
                assert d <= M * yard, (T, ld, d, yard, "differs from the two conv_xlq launches")
                if T in QC.t_alone("conv_xlq_pair", dil) and ld == lds[0]:
                    _alone_and_stale(run, x, got, acc)
    ratio = worst.line(f"conv_xlq_pair C={Cc} k=3 d={dil} (against the two-launch chain: ratio {chain_worst:.2f})")
    assert ratio <= M, worst.w


# ----------------------------------------------------------------------------------------------------------------- C: conv_k5q

@pytest.mark.parametrize("cin,ln", QC.K5Q_INSTANCES)
def test_conv_k5q_vs_f64(cin, ln):
    """conv_k5q_kernel<cin, ln> alone, ReLU on and off: the row splits 0 / 1 / 2 / 4 bit for bit at every T; against float64 (with GARBAGE behind T a
    LayerNorm taken over a padding column, or a column read past T, is far outside the bound) and against the float32 restatement."""
    lib = _clib()
    Ts = QC.t_list("conv_k5q", 5)
    for relu in (True, False):
        worst = WorstQ(_core("conv_k5q"))
        for T in Ts:
            x = QC.k5q_input(cin, T)
            lds = QC.lds_of(T, T in QC.t_extra_lds("conv_k5q"))
            for ld in lds:
                run = lambda xx, finite=True, split=0: _k5q(lib, xx, ld, ln, relu, split, finite)
                got = run(x)
                assert got is not None, (T, ld, "conv_k5q refused a shape of its list")
                for split in QC.K5Q_SPLITS[1:]:
                    assert np.array_equal(run(x, split=split), got), (relu, T, ld, split, "the row split changes the bits")
                ref, own, yard = QC.k5q_reference(cin, ln, relu, T, Ts[-1])
                worst.add(got - ref, yard, T, ld)
                d = float(np.abs(got - own).max())
                print(f"conv_k5q cin={cin} ln={int(ln)} relu={int(relu)} T={T} ld={ld}: |own| {d:.2e} yard {yard:.2e}")
                assert d <= M * yard, (relu, T, ld, d, yard, "differs from the restatement of its own products")
                if T in QC.t_alone("conv_k5q") and ld == lds[0]:
                    _alone_and_stale(run, x, got)
        ratio = worst.line(f"conv_k5q cin={cin} ln={int(ln)} relu={int(relu)}")
        assert ratio <= M, (relu, worst.w)


# ----------------------------------------------------------------------------------------------------------------- D: refusals

def test_refusals():
    """Every argument a launcher's header excludes returns -2 and the guarded buffer keeps its sentinel.  x == y: vocoder.hip: xl_pair never passes it
    (conv1 writes bT from x / bR, conv2 reads bT and writes bR / the MRF sum), and in place a tile would read the halo its neighbour has already
    overwritten, so cmtts_launch_conv_xlq refuses it as cmtts_launch_conv_xlw does."""
    lib = _clib()
    T, ld, Bn = 40, 40, QC.B
    xd = torch.zeros((Bn, 256, ld), device=DEV)
    y = _guard(Bn, 256, ld)
    w = torch.zeros(1 << 20, device=DEV)
    p, yp = w.data_ptr(), y[1:].data_ptr()

    def xl(Cc=128, k=3, dil=1, T=T, Bn=Bn, alias=False, force=1, **kw):
        return QC.ConvXlArgs(x=yp if alias else xd.data_ptr(), y=yp, wf=p, bias=p, bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, slope=0.1, wino_force=force, **kw)

    def pa(Cc=64, k=3, dil=1, w2f=p):
        return QC.PairArgs(x=xd.data_ptr(), y=yp, w1f=p, b1=p, w2f=w2f, b2=p, bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, slope=0.1)

    def k5(Cc=256, k=5, dil=1, slope=1.0, **kw):
        return QC.ConvXlArgs(x=xd.data_ptr(), y=yp, wf=p, bias=p, bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, slope=slope, xbstride=256 * ld, ln_eps=QC.LN_EPS, **kw)

    rcs = {}
    for name, a in (("k=5", xl(k=5)), ("dil=2", xl(dil=2)), ("C=32", xl(Cc=32)), ("cin!=C", xl(cin=64)), ("T=0", xl(T=0)), ("B=0", xl(Bn=0)),
                    ("small launch without wino_force", xl(force=0)), ("x==y", xl(alias=True))):
        rcs["conv_xlq " + name] = lib.cmtts_launch_conv_xlq(C.byref(a), None)
    for name, a in (("k=7", pa(k=7)), ("dil=2", pa(dil=2)), ("C=256", pa(Cc=256)), ("no w2f", pa(w2f=None))):
        rcs["conv_xlq_pair " + name] = lib.cmtts_launch_conv_xlq_pair(C.byref(a), None)
    for name, a in (("residual", k5(res=p)), ("accum", k5(accum=1)), ("slope!=1", k5(slope=0.1)), ("dil=3", k5(dil=3)), ("k=3", k5(k=3)), ("C=128", k5(Cc=128)),
                    ("cin=128 with LayerNorm", k5(cin=128, ln_g=p, ln_b=p)), ("ln_g without ln_b", k5(ln_g=p)), ("cin=64", k5(cin=64))):
        rcs["conv_k5q " + name] = lib.cmtts_launch_conv_k5q(C.byref(a), None)
    torch.cuda.synchronize()
    assert all(rc == -2 for rc in rcs.values()), {n: rc for n, rc in rcs.items() if rc != -2}
    assert (_np(y) == QC.SENTINEL).all(), "a refused launch wrote"
    report(f"QUAD_F64 refusals: {len(rcs)} excluded arguments over 3 launchers all returned -2")
