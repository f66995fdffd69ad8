"""The HiFi-GAN vocoder's kernels called ALONE through their launch hooks (cm-tts_amd/csrc/resblock_pair.h, conv_args.h) against the float64
definition of the same operation (tests/vocoder_kernel_cases.py): the element-wise check of the vocoder that the whole-wav criteria of
tests/test_gpu_precision.py and the kernel-against-kernel bit comparisons of tests/test_gpu_parity.py rest on.

  A  single convs, no on-chip rounding of an intermediate: conv_xl, conv_xlw, convT (fp32); conv16 / conv_xl16 with a 16-bit image out and in,
     convT16 (bf16, fp16, fp16x3); conv_xl16x3 — float64 on the operands the kernel itself has, bound M x d32
  B  fused kernels, anchored twice: resblock_pair (fp32), resblock_pair16, resblock_pairw16, resblock16, resblock_pair16x3 — bit for bit against the
     chain of single-conv launches their sources claim equality with, and against float64 with M x d32 + the rounding-flip widening (16-bit: xt is
     rounded on chip; fp16x3: the omitted lo x lo products)
  C  refusals: a shape a launcher's header does not cover returns -2 and writes nothing

at T in {1, reach, W - 1, W, W + 1, 2 W + reach + 1} of every instance's own tile width W, B = 2, into buffers that hold a sentinel around the launch's
rows.  Rows of T + 3 elements twice per instance: at T = W (an odd stride, of the 16-bit images too) and at the ragged neighbour of W whose T + 3 is no
multiple of 4 (vocoder_kernel_cases.t_extra_lds).  Utterance 1 alone, and the launch repeated behind one on inputs 1e4 times larger (stale on-chip
state), run at T = 1 and T = W + 1 with aligned rows for every epilogue variant — not at every T: two more launches each.  A launcher may refuse (-2,
buffer intact) a row stride of T + 3 or a T outside W - 1 .. W + 1; a refusal of an aligned W - 1 / W / W + 1 launch fails the test.

M = 10 for every kernel, set by the line the text-side module draws (a ratio of a few is a reordered fp32 sum, above 10 is a finding) — not by what
the kernels give.  d32 = the deviation of the definition's own float32 evaluation on the same case, floored by the instance's d32 at its largest T
and by 4 ulps of the output.  Measured worst ratios on MI355X: below the imports; every instance's is in the parity report (VOC_F64 lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from conftest import report
from oracle import winograd_ref as W
import vocoder_kernel_cases as VC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
M = VC.M
# Worst (|kernel - float64| - widening) / d32 per kernel over all its instances, T and row strides, as measured on MI355X (the bound is M = 10 throughout;
# d32 is mostly the 4-ulp floor, 1.9e-6 on outputs of 4 .. 8).  No launcher refused a T or a row stride of the lists.
#   conv_xl 9.21 (C = 256, k = 11, d = 1, T = 63: |d| 1.76e-5 on a 2816-term sum that the kernel adds in k-step order, numpy pairwise: the
#   ratio grows in proportion to the number of terms, 2.3 / 5.4 / 9.2 at k = 3 / 7 / 11, as a sequential fp32 sum's error does; C = 128: <= 6.72),
#   conv_xlw 5.79 (C = 256, k = 11, d = 1), convT 3.83 (512 -> 256), resblock_pair 2.07 (C = 64, k = 11, d = 3)
#   conv16 image out 0.30 bf16 / 0.62 fp16 (beyond half a 16-bit ulp), image in 1.53 / 1.36; conv_xl16 image out 0.82 / 1.22, image in 2.25 / 2.49
#   convT16 1.85 bf16 / 1.60 fp16 / 0.00 fp16x3; conv_xl16x3 1.63
#   resblock_pair16 0.22 bf16 / 0.08 fp16, resblock_pairw16 0.11 / 0.00, resblock16 0.26 / 0.04, resblock_pair16x3 0.00: beyond the widening, which at these
#   widths is non-zero for nearly every output (a few of the C k operands of an output sit near a midpoint) — the tight statement about the fused 16-bit
#   kernels is their bit equality with the conv16 chain, whose own bound is the bare M d32 above

LAUNCHERS = ("cmtts_launch_conv_xl", "cmtts_launch_conv_xlw", "cmtts_launch_convT", "cmtts_launch_conv_xl16", "cmtts_launch_resblock_pair",
             "cmtts_launch_resblock_pair16", "cmtts_launch_convT16", "cmtts_launch_resblock16", "cmtts_launch_resblock_pairw16",
             "cmtts_launch_resblock_pair16x3", "cmtts_launch_conv_xl16x3", "cmtts_launch_conv16", "cmtts_xl_set_split")
_VP, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float


def _clib():
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    for f in LAUNCHERS:
        getattr(lib, f).restype = C.c_int
    lib.cmtts_launch_convT.argtypes = [_VP, _VP, _VP, _VP, _L, _L, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _VP]
    lib.cmtts_launch_convT16.argtypes = [_VP, _VP, _VP, _VP, _L, _L, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _I, _VP]
    lib.cmtts_launch_resblock16.argtypes = [_VP, _VP, _VP, _VP, _VP, _VP, _L, _I, _I, _I, _I, _I, _I, _F, _I, _VP]
    return lib


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cases are read-only arrays)


def _np(t):
    return t.detach().cpu().numpy()


_CACHE = {}


def _frag(Cc, k, seed, mode, wino=False):
    """Conv weights (Cc, k, seed) as the launchers take them, on the device: fragment_iter_order (fp32), wino_iter_fragments (conv_xlw), fragment16 (bf16 / fp16), fragment16_split (fp16x3)."""
    key = ("w", Cc, k, seed, mode, wino)
    if key not in _CACHE:
        layout = "wino_iter_fragments" if wino else ("fragment_iter_order", "fragment16", "fragment16", "fragment16_split")[mode]
        s = _lib.internal_pack_weights(layout, VC.kmajor(VC.weights(Cc, Cc, k, seed)[0]), mode if mode in (1, 2) else 0)
        assert s is not None, key
        _CACHE[key] = _dev(s)
    return _CACHE[key].data_ptr()


def _bias(Cc, k, seed):
    key = ("b", Cc, k, seed)
    if key not in _CACHE:
        _CACHE[key] = _dev(VC.weights(Cc, Cc, k, seed)[1])
    return _CACHE[key].data_ptr()


def _guard(Bn, Cc, ld, fill=None, image=False):
    """[Bn + 2][C][ld] holding the sentinel (rows 1 .. Bn: `fill` [Bn][C][T] in the first T columns): the launch writes rows 1 .. Bn."""
    if image:
        return torch.full((Bn + 2, Cc, ld), VC.SENTINEL16, dtype=torch.int16, device=DEV)
    t = torch.full((Bn + 2, Cc, ld), VC.SENTINEL, device=DEV)
    if fill is not None:
        t[1:-1, :, :fill.shape[-1]] = _dev(fill)
    return t


def _rows(t, T, finite=True):
    """The launch's rows and columns; everything else still holds the sentinel."""
    got = _np(t)
    sent = VC.SENTINEL16 if got.dtype == np.int16 else VC.SENTINEL
    assert (got[0] == sent).all() and (got[-1] == sent).all(), "written outside the launch's rows"
    assert (got[1:-1, :, T:] == sent).all(), "written beyond T"
    if finite and got.dtype != np.int16:
        assert np.isfinite(got[1:-1, :, :T]).all()
    return got[1:-1, :, :T]


def _untouched(t, fill=None):
    """After a refusal: the buffer is as it was."""
    got = _np(t)
    sent = VC.SENTINEL16 if got.dtype == np.int16 else VC.SENTINEL
    if fill is not None:
        assert np.array_equal(got[1:-1, :, :fill.shape[-1]], fill), "a refused launch wrote"
        got = got.copy()
        got[1:-1, :, :fill.shape[-1]] = sent
    assert (got == sent).all(), "a refused launch wrote"


class Worst:
    """The worst ratio of an instance and where it was.  A refusal (-2, buffer intact) is accepted for a row stride of T + 3 or for a single T outside
    `core` — the aligned W - 1 / W / W + 1 launches every instance must take — and is listed in the report line."""

    def __init__(self, core):
        self.w, self.refused, self.core, self.n = (-1.0, 0.0, 0.0, 0, 0), [], set(core), 0

    def refuse(self, T, ld):
        assert not (T in self.core and ld % 4 == 0), (T, ld, "the launcher refused a shape it must take")
        self.refused.append((T, ld))

    def add(self, err, yard, T, ld, widen=None):
        over = np.abs(err) if widen is None else np.maximum(np.abs(err) - widen, 0.0)
        r = float(over.max()) / yard
        self.n += 1
        if r > self.w[0]:
            self.w = (r, float(np.abs(err).max()), yard, T, ld)

    def line(self, name):
        r, e, y, T, ld = self.w
        assert self.n >= len(self.core), (name, "nothing was compared")
        ref = f"; refused (-2): {self.refused}" if self.refused else ""
        report(f"VOC_F64 {name}: |d| {e:.2e}, d32 {y:.2e}, ratio {r:.2f} at T={T} ld={ld}{ref}")
        return r


def _core(kernel, Cc, k, dil=1, mode=0):
    Wt = VC.tile_width(kernel, Cc, k, dil, mode)
    return (Wt - 1, Wt, Wt + 1)


def _variants(r, y0):
    """The epilogue's operands: none, the residual alone, y += alone, both."""
    return ((None, None), (r, None), (None, y0), (r, y0))


def _alone_and_stale(run, x, got, *rest, big=None):
    """Utterance 1 launched alone has the bits it has in the batch; the launch repeated directly after one of the same kernel on inputs 1e4 times
    larger has the same bits (nothing of a previous launch's on-chip state reaches a result)."""
    one = run(x[1:2], *[None if r is None else r[1:2] for r in rest])
    assert np.array_equal(one[0], got[1]), "utterance 1 alone differs from its rows in the batch"
    run(x * F32(1e4) if big is None else big, *rest, finite=False)
    again = run(x, *rest)
    assert np.array_equal(again, got), "the launch depends on what ran before it"


# ----------------------------------------------------------------------------------------------------------------- launches

def _xl(lib, fn, x, ld, k, dil, mode=0, res=None, y0=None, finite=True, wino=False, seed=0, extra=()):
    """One ConvXlArgs launch (conv_xl, conv_xlw, conv_xl16x3) on x [Bn][C][T] -> [Bn][C][T], or None if refused."""
    Bn, Cc, T = x.shape
    xd = _dev(VC.padded(x, ld))
    rd = None if res is None else _dev(VC.padded(res, ld))
    y = _guard(Bn, Cc, ld, y0)
    a = VC.ConvXlArgs(x=xd.data_ptr(), y=y[1:].data_ptr(), wf=_frag(Cc, k, seed, mode, wino), bias=_bias(Cc, k, seed), res=None if rd is None else rd.data_ptr(),
                      bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, accum=int(y0 is not None), slope=0.1, wino_force=1)
    rc = getattr(lib, fn)(C.byref(a), *extra, None)
    torch.cuda.synchronize()
    if rc == -2:
        _untouched(y, y0)
        return None
    assert rc == 0, rc
    return _rows(y, T, finite)


def _conv16(lib, x, ld, k, dil, mode, seed, io, res=None, y0=None, finite=True, xl16=False):
    """cmtts_launch_conv16 (or cmtts_launch_conv_xl16) on x [Bn][C][T]: io 1 = fp32 in -> the activated 16-bit image out (uint16), io 2 = that image in
    (x: uint16) -> fp32 out, io 0 = fp32 in and out (fp16x3)."""
    Bn, Cc, T = x.shape
    if io == 2:
        xd = _dev(VC.padded(np.ascontiguousarray(x).view(np.int16), ld, np.int16(0x7BFF)))      # 65504 / a bf16 of 1e36 behind the valid columns
    else:
        xd = _dev(VC.padded(x, ld))
    rd = None if res is None else _dev(VC.padded(res, ld))
    y = _guard(Bn, Cc, ld, y0, image=io == 1)
    if xl16:
        a = VC.ConvXlArgs(x=xd.data_ptr(), y=y[1:].data_ptr(), wf=_frag(Cc, k, seed, mode), bias=_bias(Cc, k, seed), res=None if rd is None else rd.data_ptr(),
                          bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, accum=int(y0 is not None), slope=0.1)
        rc = lib.cmtts_launch_conv_xl16(C.byref(a), mode, io, None)
    else:
        a = VC.conv_args(xd.data_ptr(), T, ld, Cc * ld, y[1:].data_ptr(), ld, Cc * ld, T, Cc, Cc, k, _bias(Cc, k, seed))
        a.dil, a.pad, a.pre_slope = dil, dil * (k - 1) // 2, 0.1
        a.y16, a.y16_slope, a.x16 = int(io == 1), 0.1, int(io == 2)
        o = a.out[0]
        if rd is not None:
            o.res, o.r_zs0, o.ldr = rd.data_ptr(), Cc * ld, ld
        o.accum = int(y0 is not None)
        rc = lib.cmtts_launch_conv16(C.byref(a), C.c_void_p(_frag(Cc, k, seed, mode)), mode, Bn, None)
    torch.cuda.synchronize()
    if rc == -2:
        _untouched(y, y0)
        return None
    assert rc == 0, rc
    got = _rows(y, T, finite)
    return got.view(np.uint16) if io == 1 else got


def _pair(lib, kernel, x, ld, k, dil, mode, m=0, y0=None, finite=True):
    """One PairArgs launch (resblock_pair, resblock_pair16, resblock_pairw16, resblock_pair16x3) with the weights of pair m."""
    Bn, Cc, T = x.shape
    xd = _dev(VC.padded(x, ld))
    y = _guard(Bn, Cc, ld, y0)
    a = VC.PairArgs(x=xd.data_ptr(), y=y[1:].data_ptr(), w1f=_frag(Cc, k, 2 * m, mode), b1=_bias(Cc, k, 2 * m), w2f=_frag(Cc, k, 2 * m + 1, mode),
                    b2=_bias(Cc, k, 2 * m + 1), bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, accum=int(y0 is not None), slope=0.1)
    fn = getattr(lib, "cmtts_launch_" + kernel)
    rc = fn(C.byref(a), mode, None) if kernel in ("resblock_pair16", "resblock_pairw16") else fn(C.byref(a), None)
    torch.cuda.synchronize()
    if rc == -2:
        _untouched(y, y0)
        return None
    assert rc == 0, rc
    return _rows(y, T, finite)


def _pair_chain(lib, x, ld, k, dil, mode, m=0, y0=None):
    """The pair as the two single-conv launches the fused kernels claim bit equality with: conv16 writing the activated 16-bit image, conv16 reading
    it (bf16 / fp16); two fp32-in / fp32-out conv16 launches (fp16x3)."""
    if mode == 3:
        xt = _conv16(lib, x, ld, k, dil, 3, 2 * m, 0)
        return _conv16(lib, xt, ld, k, 1, 3, 2 * m + 1, 0, res=x, y0=y0)
    img = _conv16(lib, x, ld, k, dil, mode, 2 * m, 1)
    return _conv16(lib, img, ld, k, 1, mode, 2 * m + 1, 2, res=x, y0=y0)


def _resblock16(lib, x, ld, k, mode, y0=None, finite=True):
    Bn, Cc, T = x.shape
    xd = _dev(VC.padded(x, ld))
    y = _guard(Bn, Cc, ld, y0)
    arr = lambda ptrs: (C.c_void_p * 3)(*ptrs)
    w1, w2 = arr([_frag(Cc, k, 2 * m, mode) for m in range(3)]), arr([_frag(Cc, k, 2 * m + 1, mode) for m in range(3)])
    b1, b2 = arr([_bias(Cc, k, 2 * m) for m in range(3)]), arr([_bias(Cc, k, 2 * m + 1) for m in range(3)])
    rc = lib.cmtts_launch_resblock16(xd.data_ptr(), y[1:].data_ptr(), C.cast(w1, _VP), C.cast(w2, _VP), C.cast(b1, _VP), C.cast(b2, _VP), Cc * ld, Bn, Cc, T, ld, k,
                                     int(y0 is not None), 0.1, mode, None)
    torch.cuda.synchronize()
    if rc == -2:
        _untouched(y, y0)
        return None
    assert rc == 0, rc
    return _rows(y, T, finite)


def _convT(lib, stage, x, ldx, ldy, pre_div, mode, finite=True):
    """cmtts_launch_convT (mode 0) / cmtts_launch_convT16 on x [Bn][Cin][Ti] -> [Bn][Cout][Ti s]."""
    ci, co, s = VC.CONVT_STAGES[stage]
    Bn, _, Ti = x.shape
    key = ("T", stage, mode)
    if key not in _CACHE:
        w, b = VC.convT_weights(ci, co, s)
        layout = ("fragment_iter_order", "fragment16", "fragment16", "fragment16_split")[mode]
        p = _lib.internal_pack_weights(layout, VC.stack_two_tap(w, s), mode if mode in (1, 2) else 0)
        assert p is not None, key
        _CACHE[key] = (_dev(p), _dev(b))
    wf, bd = _CACHE[key]
    xd = _dev(VC.padded(x, ldx))
    y = _guard(Bn, co, ldy)
    args = (xd.data_ptr(), y[1:].data_ptr(), wf.data_ptr(), bd.data_ptr(), ci * ldx, co * ldy, Bn, ci, co, Ti, Ti * s, ldx, ldy, s, pre_div, 0.1)
    rc = lib.cmtts_launch_convT(*args, None) if mode == 0 else lib.cmtts_launch_convT16(*args, mode, None)
    torch.cuda.synchronize()
    if rc == -2:
        _untouched(y)
        return None
    assert rc == 0, rc
    return _rows(y, Ti * s, finite)


# ----------------------------------------------------------------------------------------------------------------- A: single convs

KS, DILS = (3, 7, 11), (1, 3, 5)


# conv_xlw at C = 64 (one wave per workgroup with both m-tiles; production: dilation 5 of the C = 64 stage): k = 7 and 11 are all its launcher accepts
# there.  cmtts_launch_conv_xl accepts C = 128 and 256 alone (C_in = 128 -> 256 at k = 5 apart): no instance below 128 to add.
FP32_CONVS = [(kn, Cc, k) for kn in ("conv_xl", "conv_xlw") for Cc in (128, 256) for k in KS] + [("conv_xlw", 64, 7), ("conv_xlw", 64, 11)]


@pytest.mark.parametrize("kernel,Cc,k", FP32_CONVS)
def test_fp32_conv_vs_f64(kernel, Cc, k):
    """conv_xl_kernel (the direct form: the whole C = 32 .. 256 fp32 generator below the Winograd launch sizes) and conv_xlw_kernel (F(2,3) tap groups,
    wino_force; C = 64 at k = 7 / 11 too) alone: plain, with the residual, with y += and with both; conv_xl with its m-tile split on and off (same bits); conv_xlw
    also against the float32 restatement of its own products (oracle.winograd_ref.conv1d_winograd)."""
    lib = _clib()
    wino = kernel == "conv_xlw"
    w, b = VC.weights(Cc, Cc, k, 0)
    for dil in DILS:
        worst = Worst(_core(kernel, Cc, k, dil))
        Ts = VC.t_list(kernel, Cc, k, dil)
        for T in Ts:
            x, r, y0 = VC.signal(Cc, T), VC.signal(Cc, T, 1), VC.signal(Cc, T, 2)
            lds = VC.lds_of(T, T in VC.t_extra_lds(kernel, Cc, k, dil))
            for ld in lds:
                for res, acc in _variants(r, y0):
                    run = lambda xx, rr=None, yy=None, finite=True: _xl(lib, "cmtts_launch_" + kernel, xx, ld, k, dil, 0, rr, yy, finite, wino)
                    got = run(x, res, acc)
                    if got is None:
                        worst.refuse(T, ld)
                        continue
                    ref, yard = VC.conv_reference(Cc, k, 0, dil, T, 0, res is not None, acc is not None, Ts[-1])
                    worst.add(got - ref, yard, T, ld)
                    if wino and res is None and acc is None:
                        own = np.stack([W.conv1d_winograd(VC.leaky(x[i], F32), w, dil) + b[:, None] for i in range(VC.B)])
                        assert np.abs(got - own).max() <= M * yard, (dil, T, ld, "differs from the restatement of its own products")
                    if not wino:
                        prev = lib.cmtts_xl_set_split(0)
                        try:
                            assert np.array_equal(run(x, res, acc), got), (dil, T, ld, "the m-tile split changes the bits")
                        finally:
                            lib.cmtts_xl_set_split(prev)
                    if T in VC.t_alone(kernel, Cc, k, dil) and ld == lds[0]:
                        _alone_and_stale(run, x, got, res, acc)
        ratio = worst.line(f"{kernel} C={Cc} k={k} d={dil} mode=fp32")
        assert ratio <= M, (dil, worst.w)


@pytest.mark.parametrize("stage", range(4))
@pytest.mark.parametrize("kernel", ["convT", "convT16"])
def test_upsampler_vs_f64(kernel, stage):
    """convT_xl_kernel (fp32) and convT_xl16_kernel (bf16, fp16, fp16x3: operands rounded from the fp32 value of leaky(x / pre_div), so the float64
    reference has the kernel's own operands) for the four stages, pre_div 1 and 3, Ti around the input tile, every phase of the first and of the
    last input column."""
    lib = _clib()
    ci, co, s = VC.CONVT_STAGES[stage]
    w, _ = VC.convT_weights(ci, co, s)
    for mode in ((0,) if kernel == "convT" else (1, 2, 3)):
        tile = VC.tile_width(kernel, ci, 0, 1, mode)
        worst = Worst((tile - 1, tile, tile + 1))
        Tis = VC.ti_list(tile)
        for Ti in Tis:
            for pre_div in (1.0, 3.0):
                x, ref, yard = VC.convT_reference(stage, Ti, pre_div, mode, max(Tis))
                To = Ti * s
                strides = [((Ti + 3) // 4 * 4, (To + 3) // 4 * 4)] + ([(Ti + 3, To + 3)] if Ti in VC.ti_extra_lds(tile) else [])
                for ldx, ldy in strides:
                    run = lambda xx, finite=True: _convT(lib, stage, xx, ldx, ldy, pre_div, mode, finite)
                    got = run(x)
                    if got is None:
                        worst.refuse(Ti, ldx)
                        continue
                    wd = np.stack([VC.convT_lolo(x[i], w, s, pre_div) for i in range(VC.B)]) if mode == 3 else None
                    worst.add(got - ref, yard, Ti, ldy, wd)
                    edge = np.abs(got - ref) - (0.0 if wd is None else wd)
                    assert edge[:, :, :s].max() <= M * yard, (mode, Ti, "a phase of the first input column")
                    assert edge[:, :, -s:].max() <= M * yard, (mode, Ti, "a phase of the last input column")
                    if Ti in (1, tile + 1) and ldx % 4 == 0:
                        _alone_and_stale(run, x, got)
        ratio = worst.line(f"{kernel} {ci}->{co} s={s} mode={VC.MODES[mode] or 'fp32'}")
        assert ratio <= M, (mode, worst.w)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kernel,Cc", [("conv16", 32), ("conv16", 64), ("conv16", 128), ("conv_xl16", 128), ("conv_xl16", 256)])
def test_conv16_image_out_and_in_vs_f64(kernel, Cc, k):
    """The root of the 16-bit chain: conv1d_mfma16_kernel (and its X-resident twin conv_xl16_kernel, which must give the same bits) as conv1 of a
    pair — fp32 in, convert(leaky(xt)) out as a 16-bit image: within half a 16-bit ulp + M d32 of leaky(xt) in float64 on rounded operands — and as
    conv2 on the DEVICE's own image, plain, with the residual, with y += and with both, at an odd row stride of the image too: the float64 reference then has exactly the kernel's operands and the bound is the bare M d32."""
    lib = _clib()
    xl16 = kernel == "conv_xl16"
    w2, b2 = VC.weights(Cc, Cc, k, 1)
    for mode in (1, 2):
        for dil in DILS:
            wo, wi = Worst(_core(kernel, Cc, k, dil, mode)), Worst(_core(kernel, Cc, k, dil, mode))
            Ts = VC.t_list(kernel, Cc, k, dil, mode)
            floor2 = {}
            for T in Ts[::-1]:
                x, y0 = VC.signal(Cc, T), VC.signal(Cc, T, 2)
                lds = VC.lds_of(T, T in VC.t_extra_lds(kernel, Cc, k, dil, mode))
                for ld in lds:
                    checks = T in VC.t_alone(kernel, Cc, k, dil, mode) and ld == lds[0]
                    run1 = lambda xx, finite=True: _conv16(lib, xx, ld, k, dil, mode, 0, 1, None, None, finite, xl16)
                    img = run1(x)
                    if img is None:
                        wo.refuse(T, ld)
                        continue
                    xt64, yard = VC.conv_reference(Cc, k, 0, dil, T, mode, False, False, Ts[-1])
                    a64 = VC.leaky(xt64, F64)
                    dec = VC.decode16(img, mode).astype(F64)
                    wo.add(dec - a64, yard, T, ld, 0.5 * VC.ulp16(np.maximum(np.abs(a64), np.abs(dec)), mode))
                    if xl16:
                        assert np.array_equal(_conv16(lib, x, ld, k, dil, mode, 0, 1), img), (mode, dil, T, ld, "conv_xl16 io 1 differs from conv16 y16")
                    for vi, (res, acc) in enumerate(_variants(x, y0)):
                        run2 = lambda ii, rr=None, yy=None, finite=True: _conv16(lib, ii, ld, k, 1, mode, 1, 2, rr, yy, finite, xl16)
                        got = run2(img, res, acc)
                        if got is None:
                            wi.refuse(T, ld)
                            continue
                        ev = lambda dt: np.stack([VC.conv_def(VC.decode16(img[i], mode), w2, b2, 1, mode, dt, None if res is None else res[i],
                                                              None if acc is None else acc[i], act=False) for i in range(VC.B)])
                        ref = ev(F64)
                        d32 = VC.dmax(ref, ev(F32))
                        if T == Ts[-1]:      # the floor of each epilogue variant: its own d32 at the instance's largest T
                            floor2[vi] = max(floor2.get(vi, 0.0), d32)
                        wi.add(got - ref, max(d32, floor2.get(vi, 0.0), VC.floor4(ref)), T, ld)
                        if xl16:
                            assert np.array_equal(_conv16(lib, img, ld, k, 1, mode, 1, 2, res, acc), got), (mode, dil, T, ld, "conv_xl16 io 2 differs from conv16 x16")
                        if checks:
                            _alone_and_stale(run2, img, got, res, acc, big=run1(x * F32(1e4), finite=False))
                    if checks:
                        _alone_and_stale(run1, x, img)
            name = f"C={Cc} k={k} d={dil} mode={VC.MODES[mode]}"
            r1, r2 = wo.line(f"{kernel} image out {name}"), wi.line(f"{kernel} image in {name}")
            assert r1 <= M and r2 <= M, (mode, dil, wo.w, wi.w)


@pytest.mark.parametrize("k", KS)
def test_conv_xl16x3_vs_f64(k):
    """conv_xl16x3_kernel (C = 256, fp16x3: (hi, lo) operands, three MFMAs per product) alone: bit for bit the generic kernel's mode-3 launch, and
    within M d32 + the omitted lo x lo products of float64 on the 22-bit operands."""
    lib = _clib()
    Cc = 256
    w, _ = VC.weights(Cc, Cc, k, 0)
    for dil in DILS:
        worst = Worst(_core("conv_xl16x3", Cc, k, dil, 3))
        Ts = VC.t_list("conv_xl16x3", Cc, k, dil, 3)
        for T in Ts:
            x, r, y0 = VC.signal(Cc, T), VC.signal(Cc, T, 1), VC.signal(Cc, T, 2)
            lds = VC.lds_of(T, T in VC.t_extra_lds("conv_xl16x3", Cc, k, dil, 3))
            lolo = np.stack([VC.lolo_term(VC.leaky(x[i], F64), w, dil) for i in range(VC.B)])
            for ld in lds:
                for res, acc in _variants(r, y0):
                    run = lambda xx, rr=None, yy=None, finite=True: _xl(lib, "cmtts_launch_conv_xl16x3", xx, ld, k, dil, 3, rr, yy, finite)
                    got = run(x, res, acc)
                    if got is None:
                        worst.refuse(T, ld)
                        continue
                    assert np.array_equal(_conv16(lib, x, ld, k, dil, 3, 0, 0, res, acc), got), (dil, T, ld, "differs from conv16 mode 3")
                    ref, yard = VC.conv_reference(Cc, k, 0, dil, T, 3, res is not None, acc is not None, Ts[-1])
                    worst.add(got - ref, yard, T, ld, lolo)
                    if T in VC.t_alone("conv_xl16x3", Cc, k, dil, 3) and ld == lds[0]:
                        _alone_and_stale(run, x, got, res, acc)
        assert worst.line(f"conv_xl16x3 C={Cc} k={k} d={dil} mode=fp16x3") <= M, (dil, worst.w)


# ----------------------------------------------------------------------------------------------------------------- B: fused kernels

PAIR_KERNELS = ([("resblock_pair", c, (0,)) for c in (32, 64)] + [("resblock_pair16", c, (1, 2)) for c in (32, 64)] + [("resblock_pairw16", 128, (1, 2))] +
                [("resblock_pair16x3", c, (3,)) for c in (32, 64, 128)])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kernel,Cc,modes", PAIR_KERNELS)
def test_pair_vs_f64(kernel, Cc, modes, k):
    """A ResBlock pair in one launch.  16-bit and fp16x3: bit for bit the two conv16 launches (ragged T and unaligned rows, which the whole-generator
    bit comparisons never present), and within M d32 + widen of pair_def in float64 on rounded operands, where max(widen) <= 1 % of rms(y); fp32: the
    bare M d32."""
    lib = _clib()
    for mode in modes:
        for dil in DILS:
            worst = Worst(_core(kernel, Cc, k, dil, mode))
            Ts = VC.t_list(kernel, Cc, k, dil, mode)
            for T in Ts:
                x, y0 = VC.signal(Cc, T), VC.signal(Cc, T, 2)
                lds = VC.lds_of(T, T in VC.t_extra_lds(kernel, Cc, k, dil, mode))
                for ld in lds:
                    for acc in (None, y0):
                        run = lambda xx, yy=None, finite=True: _pair(lib, kernel, xx, ld, k, dil, mode, 0, yy, finite)
                        got = run(x, acc)
                        if got is None:
                            worst.refuse(T, ld)
                            continue
                        if mode:
                            assert np.array_equal(_pair_chain(lib, x, ld, k, dil, mode, 0, acc), got), (mode, dil, T, ld, "differs from the two conv16 launches")
                        e, yard = VC.pair_reference(Cc, k, 0, dil, T, mode, acc is not None, Ts[-1])
                        assert e["widen"].max() <= 0.01 * np.sqrt((e["ref"] ** 2).mean()), (mode, dil, T, "the widening is no longer small against y")
                        worst.add(got - e["ref"], yard, T, ld, e["widen"] if mode else None)
                        if T in VC.t_alone(kernel, Cc, k, dil, mode) and ld == lds[0]:
                            _alone_and_stale(run, x, got, acc)
            assert worst.line(f"{kernel} C={Cc} k={k} d={dil} mode={VC.MODES[mode] or 'fp32'}") <= M, (mode, dil, worst.w)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("Cc", [32, 64])
def test_resblock16_vs_f64(Cc, k):
    """A whole ResBlock (three pairs) in one launch: bit for bit three resblock_pair16 launches, whose outputs are checked pair by pair against float64
    with each pair's reference starting from the DEVICE output of the pair before it (so rounding flips do not compound across the pairs)."""
    lib = _clib()
    for mode in (1, 2):
        worst = Worst(_core("resblock16", Cc, k, 1, mode))
        Ts = VC.t_list("resblock16", Cc, k, 1, mode)
        floors = {}
        for T in Ts[::-1]:
            x, y0 = VC.signal(Cc, T), VC.signal(Cc, T, 2)
            lds = VC.lds_of(T, T in VC.t_extra_lds("resblock16", Cc, k, 1, mode))
            for ld in lds:
                for acc in (None, y0):
                    xr = x      # the three-launch form first: its float64 checks do not depend on whether resblock16 takes the shape
                    for m, dil in enumerate(VC.RB_DILS):
                        ym = acc if m == 2 else None
                        nxt = _pair(lib, "resblock_pair16", xr, ld, k, dil, mode, m, ym)
                        assert nxt is not None, (mode, T, ld, m, "resblock_pair16 refused a shape of resblock16's list")
                        e, yard = VC.pair_reference_on(xr, ym, Cc, k, m, dil, mode, floors.get((m, acc is None), 0.0))
                        if T == Ts[-1]:
                            floors[(m, acc is None)] = max(floors.get((m, acc is None), 0.0), e["d32"])
                        assert e["widen"].max() <= 0.01 * np.sqrt((e["ref"] ** 2).mean()), (mode, m, T)
                        assert (np.maximum(np.abs(nxt - e["ref"]) - e["widen"], 0.0) <= M * yard).all(), (mode, T, ld, m, "pair of the three-launch form outside its bound")
                        last = (nxt - e["ref"], yard, e["widen"])
                        xr = nxt
                    run = lambda xx, yy=None, finite=True: _resblock16(lib, xx, ld, k, mode, yy, finite)
                    got = run(x, acc)
                    if got is None:
                        worst.refuse(T, ld)
                        continue
                    assert np.array_equal(got, xr), (mode, T, ld, "differs from three resblock_pair16 launches")
                    worst.add(last[0], last[1], T, ld, last[2])      # = resblock16's own output against the last pair's chained reference
                    if T in VC.t_alone("resblock16", Cc, k, 1, mode) and ld == lds[0]:
                        _alone_and_stale(run, x, got, acc)
        assert worst.line(f"resblock16 C={Cc} k={k} d=1,3,5 mode={VC.MODES[mode]}") <= M, (mode, worst.w)


# ----------------------------------------------------------------------------------------------------------------- C: refusals

def test_refusals():
    """One shape per launcher that its header does not cover — C = 96, k = 5, a dilation beyond the staged halo, x == y, mode 0 — returns -2 and the
    output buffer keeps its sentinel."""
    lib = _clib()
    T, ld, Bn = 40, 40, VC.B
    xd = torch.zeros((Bn, 256, ld), device=DEV)
    y = _guard(Bn, 256, ld)
    w = torch.zeros(1 << 20, device=DEV)

    def xl(Cc=128, k=3, dil=1, alias=False, **kw):
        return VC.ConvXlArgs(x=y[1:].data_ptr() if alias else xd.data_ptr(), y=y[1:].data_ptr(), wf=w.data_ptr(), bias=w.data_ptr(), bstride=Cc * ld, B=Bn, C=Cc, T=T,
                             ld=ld, k=k, dil=dil, slope=0.1, wino_force=1, **kw)

    def pa(Cc=64, k=3, dil=1, alias=False):
        return VC.PairArgs(x=y[1:].data_ptr() if alias else xd.data_ptr(), y=y[1:].data_ptr(), w1f=w.data_ptr(), b1=w.data_ptr(), w2f=w.data_ptr(), b2=w.data_ptr(),
                           bstride=Cc * ld, B=Bn, C=Cc, T=T, ld=ld, k=k, dil=dil, slope=0.1)

    rcs = {}
    for name, a in (("C=96", xl(Cc=96)), ("k=5", xl(k=5)), ("dil=7", xl(dil=7)), ("x==y", xl(alias=True))):
        rcs["conv_xl " + name] = lib.cmtts_launch_conv_xl(C.byref(a), None)
        rcs["conv_xl16 " + name] = lib.cmtts_launch_conv_xl16(C.byref(a), 1, 1, None)
    for name, a in (("C=96", xl(Cc=96)), ("k=5", xl(k=5)), ("dil=2", xl(dil=2)), ("x==y", xl(alias=True)), ("cin", xl(cin=64))):
        rcs["conv_xlw " + name] = lib.cmtts_launch_conv_xlw(C.byref(a), None)
    for name, a in (("C=128", xl(Cc=128)), ("k=5", xl(Cc=256, k=5)), ("dil=7", xl(Cc=256, dil=7)), ("x==y", xl(Cc=256, alias=True))):
        rcs["conv_xl16x3 " + name] = lib.cmtts_launch_conv_xl16x3(C.byref(a), None)
    rcs["conv_xl16 mode=0"] = lib.cmtts_launch_conv_xl16(C.byref(xl()), 0, 1, None)
    rcs["conv_xl16 io=0"] = lib.cmtts_launch_conv_xl16(C.byref(xl()), 1, 0, None)
    for name, a in (("C=96", pa(Cc=96)), ("k=5", pa(k=5)), ("dil=7,k=11", pa(k=11, dil=7)), ("x==y", pa(alias=True))):
        rcs["resblock_pair " + name] = lib.cmtts_launch_resblock_pair(C.byref(a), None)
        rcs["resblock_pair16 " + name] = lib.cmtts_launch_resblock_pair16(C.byref(a), 1, None)
        rcs["resblock_pair16x3 " + name] = lib.cmtts_launch_resblock_pair16x3(C.byref(a), None)
    for name, a in (("C=64", pa(Cc=64)), ("k=5", pa(Cc=128, k=5)), ("dil=7", pa(Cc=128, dil=7)), ("x==y", pa(Cc=128, alias=True))):
        rcs["resblock_pairw16 " + name] = lib.cmtts_launch_resblock_pairw16(C.byref(a), 1, None)
    rcs["resblock_pair16 mode=0"] = lib.cmtts_launch_resblock_pair16(C.byref(pa()), 0, None)
    rcs["resblock_pairw16 mode=0"] = lib.cmtts_launch_resblock_pairw16(C.byref(pa(Cc=128)), 0, None)
    ptrs = C.cast((C.c_void_p * 3)(w.data_ptr(), w.data_ptr(), w.data_ptr()), _VP)
    for name, (Cc, k, mode, alias) in (("C=96", (96, 3, 1, False)), ("k=5", (64, 5, 1, False)), ("mode=0", (64, 3, 0, False)), ("x==y", (64, 3, 1, True))):
        rcs["resblock16 " + name] = lib.cmtts_launch_resblock16(y[1:].data_ptr() if alias else xd.data_ptr(), y[1:].data_ptr(), ptrs, ptrs, ptrs, ptrs, Cc * ld, Bn, Cc, T, ld, k,
                                                                0, 0.1, mode, None)
    for name, (ci, co, s, To, mode) in (("C_in=96", (96, 48, 2, 80, 1)), ("s=3", (64, 32, 3, 120, 1)), ("To!=Ti s", (64, 32, 2, 81, 1)), ("mode=0", (64, 32, 2, 80, 0))):
        args = (xd.data_ptr(), y[1:].data_ptr(), w.data_ptr(), w.data_ptr(), ci * ld, co * To, Bn, ci, co, T, To, ld, To, s, 1.0, 0.1)
        if mode:
            rcs["convT " + name] = lib.cmtts_launch_convT(*args, None)
        rcs["convT16 " + name] = lib.cmtts_launch_convT16(*args, mode, None)
    a = VC.conv_args(xd.data_ptr(), T, ld, 64 * ld, y[1:].data_ptr(), ld, 64 * ld, T, 64, 64, 3, w.data_ptr())
    rcs["conv16 mode=0"] = lib.cmtts_launch_conv16(C.byref(a), C.c_void_p(w.data_ptr()), 0, Bn, None)
    a.K = 48
    rcs["conv16 K=48"] = lib.cmtts_launch_conv16(C.byref(a), C.c_void_p(w.data_ptr()), 1, Bn, None)
    a.K, a.x16, a.y16 = 64, 1, 1
    rcs["conv16 x16 and y16"] = lib.cmtts_launch_conv16(C.byref(a), C.c_void_p(w.data_ptr()), 1, Bn, None)
    torch.cuda.synchronize()
    assert all(rc == -2 for rc in rcs.values()), {n: rc for n, rc in rcs.items() if rc != -2}
    assert (_np(y) == VC.SENTINEL).all(), "a refused launch wrote"
    report(f"VOC_F64 refusals: {len(rcs)} uncovered shapes over 12 launchers all returned -2")
