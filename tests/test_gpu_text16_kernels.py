"""The opt-in 16-bit text side's kernels ("text16") called ALONE through their launch hooks (cm-tts_amd/csrc/conv_args.h) against the float64
definition of the same launch (tests/text16_kernel_cases.py): conv_xt16_kernel<1 / 3 / 5 / 9> (conv_xt16.hip: resident x^T tile, hand-issued weight
ring, no barrier in the K loop) and the text_epi branch of conv1d_mfma16_kernel with its 128x96, 128x128 and 64x128 tiles (conv_mfma16.hip) — the
element-wise check that the whole-model criteria of tests/test_gpu_precision.py and the kernel-against-kernel comparison
tests/test_gpu_parity.py::test_text16_xresident_bitwise rest on.

  A  every launch text_side.hip makes with text_epi = 1 (in- / out-projection, FFN conv and linear, predictor convs) and a small M = 64 / 48 one, bf16
     and fp16, against float64 on the operands the kernel itself has; bound M x yard, masked columns exactly 0
  B  bit for bit: cmtts_launch_conv_xt16 directly == cmtts_launch_conv16 with text_xt16 = 0 (the chunked kernel) == with text_xt16 = 1, at every N and
     row stride
  C  refusals: what a launcher's header does not cover returns -2 and writes nothing; empty launches write nothing

at N in (1, 31, 33, 95, 96, 97, 127, 128, 129, 130, 193), B = 2, lens = [N, 0.6 N], rows of round_up(N, 4) floats (N = 97: 8 more too), x between
GARBAGE, outputs between sentinel rows; the residual in place (res == Y) as production runs it, the out-projection also with a separate residual buffer
of rows 4 floats longer.  At N = 1 and 97: utterance 1 alone, and (bf16) the launch repeated behind one on inputs 1e4 times larger.

M = 10 (vocoder_kernel_cases.M), yard = max(d32 of the case, d32 of the instance at N = 193, 4 ulps of the output).  Measured worst ratios on MI355X:
below the imports; every instance's is in the parity report (TXT16_F64 lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from conftest import report
import text16_kernel_cases as T16
from test_gpu_vocoder_kernels import _alone_and_stale, _dev, _guard, _rows, _untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = T16.M
# Worst |kernel - float64| / yard per instance over all N, row strides and both residual forms, as measured on MI355X (the bound is M = 10):
#   qkv 0.67 bf16 / 0.36 fp16, out 0.79 / 0.38, ffn1 3.40 / 2.56 (N = 129 / 127: a 2304-term sum in (chunk, tap, k-group) order against numpy's pairwise one,
#   then GELU), pred3 1.62 / 0.86, pred5 1.30 / 1.19, ffn2 1.23 / 0.92, small M = 64 1.58 / 0.89, M = 48 1.14 / 0.89; yard is the 4-ulp floor (1.9e-6 on outputs
#   of 4 .. 8) in bf16 and mostly d32 (2.3e-6 .. 5.8e-6) in fp16, whose products keep more bits than an fp32 sum of them does.  The three calls of B agreed in
#   every bit at all 12 shapes of an instance (24 for `out`).  On the commit before the launcher's refusal list was completed, test_refusals failed with
#   cmtts_launch_conv_xt16 returning 0 and writing for rmul = 0.5 and split = 128, and test_empty_launches_write_nothing with -3 for M, N, nbatch = 0.


def _clib():
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    for f in ("cmtts_launch_conv16", "cmtts_launch_conv_xt16"):
        getattr(lib, f).restype = C.c_int
    return lib


_CACHE = {}


def _frag(name, mode):
    """The instance's weights as the launchers take them: the fragment16 stream of its rounded k-major array, on the device."""
    key = ("w", name, mode)
    if key not in _CACHE:
        s = _lib.internal_pack_weights("fragment16", T16.packer_input(name), mode)
        assert s is not None, key
        _CACHE[key] = _dev(s)
    return _CACHE[key].data_ptr()


def _bias(name):
    key = ("b", name)
    if key not in _CACHE:
        _CACHE[key] = _dev(T16.weights(name)[1])
    return _CACHE[key].data_ptr()


class _Switch:
    """The internal switch "text_xt16" (conv_xt16.hip's g_conv_xt16) for one launch, restored whatever happens."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.prev = _lib.internal_set("text_xt16", self.value)

    def __exit__(self, *exc):
        _lib.internal_set("text_xt16", self.prev)
        return False


def _launch(lib, how, name, mode, ld, x, res=None, lens=None, finite=True, sep=False):
    """One launch of instance `name` on x [Bn][K][N] -> [Bn][M][N], or None if refused (-2, buffers intact).  how: "xt16" = cmtts_launch_conv_xt16,
    "chunked" / "conv16" = cmtts_launch_conv16 with text_xt16 = 0 / 1.  res [Bn][M][N]: in place (res == Y, same strides), or sep: its own buffer with
    rows of ld + 4 floats.  x lies between utterances of GARBAGE, with GARBAGE in columns [N, ld)."""
    I = T16.INSTANCES[name]
    Bn, _, N = x.shape
    xd = _dev(T16.padded(x, ld, 1))
    in_place = res is not None and not sep
    y = _guard(Bn, I.M, ld, res if in_place else None)
    a = T16.conv_args(xd[1:].data_ptr(), N, ld, I.K * ld, y[1:].data_ptr(), ld, I.M * ld, N, I.M, I.K, I.taps, _bias(name))
    a.text_epi = 1
    o = a.out[0]
    o.alpha, o.act = I.alpha, I.act
    rd = ln = None
    if res is not None:
        rd = _dev(T16.padded(res, ld + 4)) if sep else y[1:]
        o.res, o.r_zs0, o.ldr = rd.data_ptr(), I.M * (ld + 4 if sep else ld), ld + 4 if sep else ld
    if lens is not None:
        ln = _dev(lens)
        o.lens = ln.data_ptr()
    wf = C.c_void_p(_frag(name, mode))
    if how == "xt16":
        rc = lib.cmtts_launch_conv_xt16(C.byref(a), wf, mode, Bn, None)
    else:
        with _Switch(0 if how == "chunked" else 1):
            rc = lib.cmtts_launch_conv16(C.byref(a), wf, mode, Bn, None)
    torch.cuda.synchronize()
    if rc == -2:
        _untouched(y, res if in_place else None)
        return None
    assert rc == 0, (how, rc)
    return _rows(y, N, finite)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(T16.INSTANCES))
def test_text16_conv_vs_f64(name, mode):
    """A and B of the module's header for one instance and operand type."""
    lib = _clib()
    I = T16.INSTANCES[name]
    worst = (-1.0, 0.0, 0.0, 0, 0, False)
    n = 0
    for N in T16.NS:
        x, lens = T16.x_input(I.K, N), T16.xres_lens(N)
        res = T16.residual(N) if I.res else None
        ln = lens if I.mask else None
        ref, yard = T16.reference(name, N, mode)
        lds = T16.lds_of(N)
        for ld in lds:
            for sep in ((False, True) if name == "out" else (False,)):
                def run(xx, rr=None, ll=None, finite=True, how="conv16"):
                    return _launch(lib, how, name, mode, ld, xx, rr, ll, finite, sep)
                got = run(x, res, ln)
                assert got is not None, (N, ld, "cmtts_launch_conv16 refused a launch of the text side")
                if I.mask:
                    for b in range(T16.B):
                        assert not got[b][:, int(lens[b]):].any(), (N, ld, b, "columns >= lens are not 0")
                e = float(np.abs(got - ref).max())
                n += 1
                if e / yard > worst[0]:
                    worst = (e / yard, e, yard, N, ld, sep)
                chunked = run(x, res, ln, how="chunked")
                assert chunked is not None and np.array_equal(chunked, got), (N, ld, sep, "text_xt16 = 0 and 1 differ")
                direct = run(x, res, ln, how="xt16")
                if name in T16.XT16:
                    assert direct is not None and np.array_equal(direct, got), (N, ld, sep, "cmtts_launch_conv_xt16 differs from cmtts_launch_conv16")
                else:
                    assert direct is None, (N, ld, "cmtts_launch_conv_xt16 took a shape outside its header")
                if N in T16.N_ALONE and ld == lds[0] and not sep:
                    for how in (("conv16", "chunked") if name in T16.XT16 else ("conv16",)):
                        runh = lambda xx, rr=None, ll=None, finite=True: run(xx, rr, ll, finite, how)
                        if mode == 1:
                            _alone_and_stale(runh, x, got, res, ln)
                        else:      # fp16 leaves its range on inputs 1e4 times larger
                            one = runh(x[1:2], None if res is None else res[1:2], None if ln is None else ln[1:2])
                            assert np.array_equal(one[0], got[1]), (how, "utterance 1 alone differs from its rows in the batch")
    r, e, yard, N, ld, sep = worst
    assert n >= len(T16.NS) + 1
    report(f"TXT16_F64 {name} K={I.K} M={I.M} k={I.taps} mode={T16.MODES[mode]}: |d| {e:.2e}, yard {yard:.2e}, ratio {r:.2f} at N={N} ld={ld}" +
           (" (separate residual)" if sep else "") + f"; {n} shapes, conv_xt16 / chunked / cmtts_launch_conv16 bit for bit")
    assert r <= M, worst


# ----------------------------------------------------------------------------------------------------------------- C: refusals

def _refusal_args(xd, y, w, N, ld, name="pred3"):
    """A launch both launchers take (the k = 3 predictor conv), to be spoilt in one field."""
    I = T16.INSTANCES[name]
    a = T16.conv_args(xd.data_ptr(), N, ld, I.K * ld, y[1:].data_ptr(), ld, I.M * ld, N, I.M, I.K, I.taps, w.data_ptr())
    a.text_epi, a.out[0].act = 1, I.act
    return a


def _spoil(a, **kw):
    for k, v in kw.items():
        setattr(a.out[0] if k in dict(T16.ConvOut._fields_) else a, k, v)
    return a


REFUSAL_N = 33
XT16_REFUSALS = {"text_epi = 0": dict(text_epi=0), "K = 128": dict(K=128), "M = 192": dict(M=192), "taps = 7": dict(taps=7, pad=3), "dil = 2": dict(dil=2),
                 "pad = 0": dict(pad=0), "pre_div = 2": dict(pre_div=2.0), "pre_slope = 0.1": dict(pre_slope=0.1), "zdiv = 2": dict(zdiv=2), "x16": dict(x16=1),
                 "y16": dict(y16=1), "ostride = 2": dict(ostride=2), "row_off = 1": dict(row_off=1), "div = 2": dict(div=2.0), "accum": dict(accum=1),
                 "bvec": dict(bvec=None), "Tout = N - 1": dict(Tout=REFUSAL_N - 1), "act = tanh": dict(act=T16.ACT_TANH), "rmul = 0.5": dict(rmul=0.5),
                 "split = 128": dict(split=128)}
CONV16_REFUSALS = {"rmul = 0.5": dict(rmul=0.5), "act = tanh": dict(act=T16.ACT_TANH), "accum": dict(accum=1)}


def test_refusals():
    """What cmtts_launch_conv_xt16's header (conv_args.h) does not cover, and what cmtts_launch_conv16 does not cover with text_epi = 1, returns -2
    and leaves the output as it was — never a result with a field silently ignored (epi_tile_simple has no rmul, the kernels have no second output)."""
    lib = _clib()
    N, ld, Bn = REFUSAL_N, 36, T16.B
    xd = torch.zeros((Bn, 256, ld), device=DEV)
    y = _guard(Bn, 256, ld)
    w = torch.zeros(1 << 20, device=DEV)
    wf = C.c_void_p(w.data_ptr())
    bad = {}

    def check(label, rc):
        torch.cuda.synchronize()
        wrote = not bool((y == T16.SENTINEL).all())
        if rc != -2 or wrote:
            bad[label] = (rc, "wrote" if wrote else "intact")
            y.fill_(T16.SENTINEL)

    assert lib.cmtts_launch_conv_xt16(C.byref(_refusal_args(xd, y, w, N, ld)), wf, 1, Bn, None) == 0      # unspoilt, both take it
    assert lib.cmtts_launch_conv16(C.byref(_refusal_args(xd, y, w, N, ld)), wf, 1, Bn, None) == 0
    torch.cuda.synchronize()
    assert not bool((y[1:-1, :, :N] == T16.SENTINEL).any())
    y.fill_(T16.SENTINEL)
    for label, kw in XT16_REFUSALS.items():
        if "bvec" in kw:
            kw = dict(bvec=w.data_ptr())      # (any valid device pointer)
        check("conv_xt16 " + label, lib.cmtts_launch_conv_xt16(C.byref(_spoil(_refusal_args(xd, y, w, N, ld), **kw)), wf, 1, Bn, None))
    for mode in (0, 3):
        check(f"conv_xt16 mode = {mode}", lib.cmtts_launch_conv_xt16(C.byref(_refusal_args(xd, y, w, N, ld)), wf, mode, Bn, None))
    check("conv16 mode = 3", lib.cmtts_launch_conv16(C.byref(_refusal_args(xd, y, w, N, ld)), wf, 3, Bn, None))
    for label, kw in CONV16_REFUSALS.items():
        check("conv16 " + label, lib.cmtts_launch_conv16(C.byref(_spoil(_refusal_args(xd, y, w, N, ld), **kw)), wf, 1, Bn, None))
    report(f"TXT16_F64 refusals: {len(XT16_REFUSALS) + 2 + 1 + len(CONV16_REFUSALS)} uncovered launches; not refused: {bad or 'none'}")
    assert not bad, bad


def test_empty_launches_write_nothing():
    """M = 0, N = 0 and nbatch = 0 on both launchers: nothing is launched (0 or -2) and nothing written."""
    lib = _clib()
    N, ld, Bn = REFUSAL_N, 36, T16.B
    xd = torch.zeros((Bn, 256, ld), device=DEV)
    y = _guard(Bn, 256, ld)
    w = torch.zeros(1 << 20, device=DEV)
    wf = C.c_void_p(w.data_ptr())
    rcs = {}
    for fn in ("cmtts_launch_conv_xt16", "cmtts_launch_conv16"):
        rcs[fn + " M = 0"] = getattr(lib, fn)(C.byref(_spoil(_refusal_args(xd, y, w, N, ld), M=0)), wf, 1, Bn, None)
        rcs[fn + " N = 0"] = getattr(lib, fn)(C.byref(_spoil(_refusal_args(xd, y, w, N, ld), N=0, Tout=0)), wf, 1, Bn, None)
        rcs[fn + " nbatch = 0"] = getattr(lib, fn)(C.byref(_refusal_args(xd, y, w, N, ld)), wf, 1, 0, None)
    torch.cuda.synchronize()
    assert all(rc in (0, -2) for rc in rcs.values()), rcs
    assert bool((y == T16.SENTINEL).all()), "an empty launch wrote"
