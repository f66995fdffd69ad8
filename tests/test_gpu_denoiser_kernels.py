"""The consistency denoiser's kernels called ALONE through their launch hooks (cm-tts_amd/csrc/resblock_args.h, cond_gemm.h, inproj.h) against the
float64 definition of the same operation (tests/denoiser_kernel_cases.py): the element-wise check of the denoiser that the whole-network criteria
of tests/test_gpu_precision.py and the kernel-against-kernel bit comparisons (fused = three-launch, split = fused, persistent = per-layer, F(4,3)
per-layer = persistent) rest on.  The persistent stack is called alone in tests/test_gpu_persist_stack.py, against its own float64 definition and bit
for bit against chains of the per-layer launches anchored here.

  A  the fp32 residual block, its two halves anchored separately: resblock_split_out on a given z; resblock_split (z, x', skip);
     resblock_fused_kernel<32> and <64> (cmtts_resblock_set_tile) bit for bit the split form and within the bound; resblock_w43 (F(4,3)) with and
     without a given u
  B  cmtts_gate alone: identity weights make z[c][t] = cmtts_gate(x[c][t], x[(c + 128) % 256][t]) on a grid up to +-1e4 — gate.h's 3e-7
  C  the 16-bit block resblock_fused_lp (bf16, fp16): float64 on rounded operands, M d32 + the rounding-flip widening of z; the fp16 overflow word
  D  the input side: inproj (scales, the cleared region), cond_gemm (flat / row_split forms: same bits), cond_gemm16 (bf16, fp16, fp16x3),
     cond_expand (bit for bit a gather and one add, both vector widths)
  E  refusals: what a launcher's header excludes returns -2 and writes nothing

at T in {1, 2, 3, W - 1, W, W + 1, 2 W - 1, 2 W, 2 W + 1} of every kernel's own tile width W (F(4,3): every residue mod 4 as well), B = 2, dense rows
(row stride T: odd T is the unaligned-row case).  The layer is a slice of a three-layer allocation (cp_bstride = 3 * 256 * T, vec_stride = 768),
outputs sit between sentinel rows, x and cp between rows of garbage.  Utterance 1 alone, and the launch repeated behind one on inputs 1e4 times
larger, at T = 1 and T = W + 1.

M = 10 for every kernel (vocoder_kernel_cases.M: a ratio of a few is a reordered fp32 sum, above 10 is a finding) — not set by what the kernels
give.  yard = max(d32 of the case, d32 of the instance at its largest T, 4 ulps of the output), d32 = the deviation of the definition's own
float32 evaluation.  That a wrong kernel fails here is shown on the CPU (tests/test_denoiser_kernel_cases_cpu.py::
test_wrong_kernels_move_the_definition_far_beyond_the_bound): a right halo not zeroed beyond T, d swapped for dp in the residual and C * T taken
as cp's batch stride each move block_def's output at T = W + 1 by more than 100 x M yard.  Measured worst ratios on MI355X: below the imports;
every instance's is in the parity report (DEN_F64 lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from conftest import report
import denoiser_kernel_cases as DC
import vocoder_kernel_cases as VC
from test_gpu_vocoder_kernels import _alone_and_stale, _dev, _guard, _np, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
M = VC.M
CH, NL, LAYER = DC.CH, DC.NL, DC.LAYER
# Worst (|kernel - float64| - widening) / d32 per kernel over its T list and epilogues, as measured on MI355X (the bound is M = 10 throughout; d32 is
# 1e-6 .. 6e-6 on outputs of a few units).  No ratio above 1.5: nothing to explain.
#   resblock_split_out 1.00, cond_gemm 1.00 (every form the same bits): K = 256 in ascending k with fused multiply-adds is also the order of the host
#   BLAS the float32 yardstick runs on, so the error IS d32; resblock_split z 1.36 (beyond the gate's 3e-7), x' / skip 1.43; resblock_fused<32> and <64>
#   1.14 (bit for bit the split form at all 14 T); resblock_w43 z 1.12, x' / skip 1.07 against the F(4,3) yardstick (d32 1.2e-5 on z: 5 x the direct
#   form's); inproj 0.92
#   cmtts_gate: worst |error| 2.57e-7 at (g, f) = (5.18, -3.44) over 16896 pairs — inside gate.h's 3e-7; saturated corners exact
#   resblock_fused_lp 0.00 bf16 / 0.00 fp16 beyond the widening (largest raw |d| in the report line), which is non-zero for every output: 4 .. 8 % (bf16) and
#   38 .. 46 % (fp16) of the z lie within M d32 + 3e-7 of a midpoint — the statement is "no error beyond rounding flips of z", 1 % of rms(o)
#   cond_gemm16 0.85 bf16 / 0.52 fp16 / 0.00 fp16x3 (beyond the lo x lo products); cond_expand bit for bit
#   refusals: the 29 excluded arguments all return -2 — ten of them (resblock_lp modes 0 and 3; x_out == x_in, four launchers; B = 0 and T = 0 in
#   resblock and resblock_lp) only since the guards that came with this module

LAUNCHERS = ("cmtts_launch_resblock", "cmtts_launch_resblock_split", "cmtts_launch_resblock_split_out", "cmtts_launch_resblock_w43",
             "cmtts_launch_resblock_lp", "cmtts_launch_cond_gemm", "cmtts_launch_cond_gemm16", "cmtts_launch_cond_expand", "cmtts_launch_inproj")
_VP, _I = C.c_void_p, C.c_int


def _clib():
    _lib.load()
    lib = C.CDLL(_lib.LIB_PATH)
    for f in LAUNCHERS:
        getattr(lib, f).restype = C.c_int
    lib.cmtts_launch_resblock_lp.argtypes = [_VP, _I, _VP]
    lib.cmtts_launch_cond_gemm16.argtypes = [_VP, _VP, _I, _VP]
    lib.cmtts_launch_cond_expand.argtypes = [_VP, _I, _I, _VP, _I, _VP, _VP, _VP, _I, _I, _I, _VP]
    lib.cmtts_resblock_set_tile.restype, lib.cmtts_resblock_set_tile.argtypes = None, [_I]
    return lib


_CACHE = {}


def _pack(key, layout, kmajor, mode=0):
    if key not in _CACHE:
        s = _lib.internal_pack_weights(layout, kmajor, mode)
        assert s is not None, key
        _CACHE[key] = _dev(s)
    return _CACHE[key].data_ptr()


def _vec(key, make):
    if key not in _CACHE:
        _CACHE[key] = _dev(np.ascontiguousarray(make(), F32))
    return _CACHE[key].data_ptr()


def _block_weights(wset, form, mode=0):
    """(W3f, b3, Wof, bo) device pointers of weight set `wset` ("case": DC.block_weights, "gate": the identity of part B) as launcher `form` takes them:
    W3 and b3 rows in gate_perm(16) order — fragment_order (fused, split), fragment16 (lp), wino43_fragments (w43); Wo fragment_order / fragment16."""
    if wset == "case":
        W3, b3, Wo, bo = DC.block_weights()
    else:
        (W3, b3), (_, _, Wo, bo) = DC.gate_identity_weights(), DC.block_weights()
    lay3 = {"w43": "wino43_fragments", "lp": "fragment16"}.get(form, "fragment_order")
    layo = "fragment16" if form == "lp" else "fragment_order"
    return (_pack((wset, "W3", lay3, mode), lay3, DC.permuted_kmajor(W3), mode), _vec((wset, "b3"), lambda: b3[DC.gate_perm(16)]),
            _pack(("Wo", layo, mode), layo, VC.kmajor(Wo[:, :, None]), mode), _vec(("bo",), lambda: bo))


def _between(v, fill):
    """[Bn][..] -> device [Bn + 2][..] with a row of `fill` before and after (a read outside the launch's rows meets it)."""
    t = torch.full((v.shape[0] + 2,) + v.shape[1:], float(fill), device=DEV)
    t[1:-1] = _dev(v)
    return t


FORMS = {"fused32": "cmtts_launch_resblock", "fused64": "cmtts_launch_resblock", "split": "cmtts_launch_resblock_split",
         "w43": "cmtts_launch_resblock_w43", "lp": "cmtts_launch_resblock_lp", "split_out": "cmtts_launch_resblock_split_out"}


def _block(lib, form, x, cp_all, dp_all, d_all, skip0=None, finite=True, mode=0, wset="case", z_in=None, u=None, flag=None):
    """One launch of `form` on the layer-LAYER slice of x [Bn][C][T], cp_all [Bn][NL C][T], dp_all / d_all [Bn][NL C] -> [Bn][2 C or 3 C][T]:
    x' | skip (| the z the launch left in a->z: split, w43).  skip0: skip's old content (accum_skip = 1).  z_in: split_out's input."""
    Bn, _, T = x.shape
    xg, cpg = _between(x, DC.GARBAGE), _between(cp_all, DC.GARBAGE)
    dpd, dd = _dev(dp_all), _dev(d_all)
    xo, sk, zb = _guard(Bn, CH, T), _guard(Bn, CH, T, skip0), _guard(Bn, CH, T, z_in)
    ud = None if u is None else _dev(u)
    w3f, b3, wof, bo = _block_weights(wset, "split" if form == "split_out" else form[:5] if form.startswith("fused") else form, mode)
    a = DC.ResArgs(x_in=xg[1:].data_ptr(), cp=cpg[1:].data_ptr() + 4 * LAYER * CH * T, dp=dpd.data_ptr() + 4 * LAYER * CH, d=dd.data_ptr() + 4 * LAYER * CH,
                   x_out=xo[1:].data_ptr(), skip=sk[1:].data_ptr(), W3f=w3f, b3=b3, Wof=wof, bo=bo, cp_bstride=NL * CH * T, vec_stride=NL * CH, B=Bn, T=T,
                   accum_skip=int(skip0 is not None), z=zb[1:].data_ptr(), flag=None if flag is None else flag.data_ptr(), u=None if ud is None else ud.data_ptr())
    fn = getattr(lib, FORMS[form])
    if form.startswith("fused"):
        lib.cmtts_resblock_set_tile(int(form[5:]))
    try:
        rc = fn(C.byref(a), mode, None) if form == "lp" else fn(C.byref(a), None)
        torch.cuda.synchronize()
    finally:
        if form.startswith("fused"):
            lib.cmtts_resblock_set_tile(0)      # (the setting before: automatic — nothing else in the suite forces a tile)
    assert rc == 0, (form, rc)
    outs = [_rows(xo, T, finite), _rows(sk, T, finite)]
    if form in ("split", "w43"):
        outs.append(_rows(zb, T, finite))
    elif z_in is None:
        assert (_np(zb) == VC.SENTINEL).all(), "a launch that has no use for a->z wrote it"
    return np.concatenate(outs, axis=1)


class Worst:
    """The worst ratio of an instance, where it fell, and the worst ratio on column 0, column T - 1 and the two columns at each tile seam."""

    def __init__(self, Wt):
        self.w, self.seam, self.Wt, self.n, self.raw = (-1.0, 0.0, 0.0, 0, ""), -1.0, Wt, 0, 0.0

    def add(self, err, yard, T, what, widen=None):
        over = np.abs(err) if widen is None else np.maximum(np.abs(err) - widen, 0.0)
        r = float(over.max()) / yard
        self.n += 1
        self.raw = max(self.raw, float(np.abs(err).max()))
        self.seam = max(self.seam, float(over[..., DC.seam_columns(T, self.Wt)].max()) / yard)
        if r > self.w[0]:
            self.w = (r, float(np.abs(err).max()), yard, T, what)
        return r

    def line(self, name):
        r, e, y, T, what = self.w
        assert self.n > 0, (name, "nothing was compared")
        report(f"DEN_F64 {name}: |d| {e:.2e}, d32 {y:.2e}, ratio {r:.2f} at T={T} ({what}); edge and seam columns {self.seam:.2f}; largest |d| of all {self.raw:.2e}")
        return r


def _split3(got):
    return got[:, :CH], got[:, CH:2 * CH], got[:, 2 * CH:]


# ----------------------------------------------------------------------------------------------------------------- A: the fp32 block

@pytest.mark.parametrize("accum", [0, 1])
def test_projection_alone_vs_f64(accum):
    """resblock_split_out_kernel alone on a z drawn uniform in (-1, 1): x' and skip (written, or added to a skip that holds a signal) within the bare M d32 of proj_def."""
    lib = _clib()
    worst = Worst(32)
    Ts = DC.t_list("split")
    for T in Ts:
        x, cp_all, dp_all, d_all, skip_old = DC.block_inputs(T)
        z, s0 = DC.proj_z(T), skip_old if accum else None
        run = lambda xx, zz, cc, pp, dd_, ss, finite=True: _block(lib, "split_out", xx, cc, pp, dd_, ss, finite, z_in=zz)
        got = run(x, z, cp_all, dp_all, d_all, s0)
        e, yard = DC.proj_reference(T, bool(accum), Ts[-1])
        worst.add(got[:, :CH] - e["x"], yard["x"], T, "x'")
        worst.add(got[:, CH:] - e["skip"], yard["skip"], T, "skip")
        if T in DC.t_alone("split"):
            _alone_and_stale(run, x, got, z, cp_all, dp_all, d_all, s0)
    assert worst.line(f"resblock_split_out accum={accum} mode=fp32") <= M, worst.w


@pytest.mark.parametrize("accum", [0, 1])
def test_split_block_vs_f64(accum):
    """resblock_split_conv_kernel + resblock_split_out_kernel: the z left in a->z within M d32 + 3e-7 (gate.h's figure: the float32 evaluation of the
    definition uses the exact exp) of block_def's, x' and skip within M d32."""
    lib = _clib()
    worst, wz = Worst(32), Worst(32)
    Ts = DC.t_list("split")
    for T in Ts:
        x, cp_all, dp_all, d_all, skip_old = DC.block_inputs(T)
        s0 = skip_old if accum else None
        run = lambda xx, cc, pp, dd_, ss, finite=True: _block(lib, "split", xx, cc, pp, dd_, ss, finite)
        got = run(x, cp_all, dp_all, d_all, s0)
        gx, gs, gz = _split3(got)
        e, yard = DC.block_reference(T, 0, bool(accum), Ts[-1])
        wz.add(gz - e["z"], yard["z"], T, "z", widen=DC.GATE_ABS)
        worst.add(gx - e["x"], yard["x"], T, "x'")
        worst.add(gs - e["skip"], yard["skip"], T, "skip")
        if T in DC.t_alone("split"):
            _alone_and_stale(run, x, got, cp_all, dp_all, d_all, s0)
    rz, r = wz.line(f"resblock_split z (beyond the gate's 3e-7) accum={accum} mode=fp32"), worst.line(f"resblock_split accum={accum} mode=fp32")
    assert rz <= M and r <= M, (wz.w, worst.w)


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("tile", [32, 64])
def test_fused_block_vs_f64_and_split(tile, accum):
    """resblock_fused_kernel<32> and <64> (cmtts_resblock_set_tile; <64> otherwise runs from 256 tiles up only): x' and skip bit for bit the split
    form's at every T of BOTH tile widths' lists, and within M d32 of block_def."""
    lib = _clib()
    form = f"fused{tile}"
    worst = Worst(tile)
    Ts = tuple(sorted(set(DC.t_list("fused32")) | set(DC.t_list("fused64"))))
    for T in Ts:
        x, cp_all, dp_all, d_all, skip_old = DC.block_inputs(T)
        s0 = skip_old if accum else None
        run = lambda xx, cc, pp, dd_, ss, finite=True: _block(lib, form, xx, cc, pp, dd_, ss, finite)
        got = run(x, cp_all, dp_all, d_all, s0)
        split = _block(lib, "split", x, cp_all, dp_all, d_all, s0)
        assert np.array_equal(got, split[:, :2 * CH]), (tile, T, "differs from the split form")
        e, yard = DC.block_reference(T, 0, bool(accum), Ts[-1])
        worst.add(got[:, :CH] - e["x"], yard["x"], T, "x'")
        worst.add(got[:, CH:] - e["skip"], yard["skip"], T, "skip")
        if T in DC.t_alone(form):
            _alone_and_stale(run, x, got, cp_all, dp_all, d_all, s0)
    assert worst.line(f"resblock_fused<{tile}> accum={accum} mode=fp32") <= M, worst.w


@pytest.mark.parametrize("accum", [0, 1])
def test_w43_block_vs_f64(accum):
    """resblock_w43_conv_kernel (F(4,3) over frame quads) + the split projection, as the launcher runs them: z against float64 with the yardstick of
    the F(4,3) restatement in float32 (oracle.winograd_ref.conv1d_f43 pushed through the gate; a transform is not a reordered sum), x' and skip
    likewise; with a->u = nullptr, and again with a->u = the float32 u: same bits."""
    lib = _clib()
    worst, wz = Worst(64), Worst(64)
    Ts = DC.t_list("w43")
    for T in Ts:
        x, cp_all, dp_all, d_all, skip_old = DC.block_inputs(T)
        cp, dp, _ = DC.layer_slices(cp_all, dp_all, d_all)
        s0 = skip_old if accum else None
        run = lambda xx, cc, pp, dd_, ss, finite=True: _block(lib, "w43", xx, cc, pp, dd_, ss, finite)
        got = run(x, cp_all, dp_all, d_all, s0)
        gx, gs, gz = _split3(got)
        e, yard = DC.block_reference(T, 0, bool(accum), Ts[-1], True)
        wz.add(gz - e["z"], yard["z"], T, "z", widen=DC.GATE_ABS)
        worst.add(gx - e["x"], yard["x"], T, "x'")
        worst.add(gs - e["skip"], yard["skip"], T, "skip")
        u = np.stack([DC.u_def(x[i], cp[i], dp[i], 0, F32) for i in range(x.shape[0])])
        assert np.array_equal(_block(lib, "w43", x, cp_all, dp_all, d_all, s0, u=u), got), (T, "a given u changes the bits")
        if T in DC.t_alone("w43"):
            _alone_and_stale(run, x, got, cp_all, dp_all, d_all, s0)
    rz, r = wz.line(f"resblock_w43 z (beyond the gate's 3e-7) accum={accum} mode=fp32"), worst.line(f"resblock_w43 accum={accum} mode=fp32")
    assert rz <= M and r <= M, (wz.w, worst.w)


# ----------------------------------------------------------------------------------------------------------------- B: the gate

def test_gate_alone():
    """cmtts_gate on a grid of (g, f) up to +-1e4, isolated by identity weights (y = u exactly, b3 = 0, cp = dp = 0): every z finite and in [-1, 1],
    within gate.h's 3e-7 of sigmoid(g) tanh(f) in float64, and the saturated corners exactly 0, +1 or -1 times the other factor."""
    lib = _clib()
    x1 = DC.gate_grid()
    x = np.stack([x1, x1[:, ::-1]])
    T = DC.GATE_T
    zero_cp, zero_v = np.zeros((2, NL * CH, T), F32), np.zeros((2, NL * CH), F32)
    got = _block(lib, "split", x, zero_cp, zero_v, zero_v, wset="gate")
    z = _split3(got)[2]
    g, f = x.astype(F64), np.roll(x, -CH // 2, axis=1).astype(F64)
    with np.errstate(over="ignore"):       # exp(1e4) = inf: sigmoid = 0 exactly
        ref = 1.0 / (1.0 + np.exp(-g)) * np.tanh(f)
    assert np.isfinite(z).all() and np.abs(z).max() <= 1.0
    err = np.abs(z - ref)
    i = np.unravel_index(err.argmax(), err.shape)
    report(f"DEN_F64 gate: worst |cmtts_gate - sigmoid(g) tanh(f)| {err.max():.3e} at g={g[i]:.6g} f={f[i]:.6g} over {err.size} pairs (gate.h: 3e-7)")
    big = 100.0                            # |v| >= 100: exp overflows or vanishes, the factor is exactly 0 or +-1
    gp, gn, fp, fn = g >= big, g <= -big, f >= big, f <= -big
    assert (z[gp & fp] == 1).all() and (z[gp & fn] == -1).all() and (z[gn] == 0).all()
    assert (z[gp & (f == 0)] == 0).all()
    for b in range(2):                     # sigmoid = 1 exactly: z is the tanh factor alone, the same for every saturated g; tanh = +-1: +-sigmoid alone
        zz, gg, ff = z[b][:CH // 2], g[b][:CH // 2], f[b][:CH // 2]      # (channels 128 .. 255 hold the same pairs the other way round)
        assert np.array_equal(_by(zz, ff, gg == 100.0), _by(zz, ff, gg == 1e4))
        assert np.array_equal(_by(zz, gg, ff == 100.0), _by(zz, gg, ff == 1e4))
        assert np.array_equal(_by(zz, gg, ff == -100.0), -_by(zz, gg, ff == 100.0))
    assert err.max() <= DC.GATE_ABS, (err.max(), g[i], f[i])


def _by(z, key, where):
    """z[where] ordered by key[where] (the grid holds every ordered pair of its points once)."""
    k = key[where]
    assert k.size == np.unique(k).size == 29
    return z[where][np.argsort(k)]


# ----------------------------------------------------------------------------------------------------------------- C: the 16-bit block

@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
def test_lp_block_vs_f64(mode, accum):
    """resblock_fused_lp_kernel (bf16, fp16) against block_def in float64 on rounded operands: |err| - widen <= M d32, where widen accounts for the z
    that may round the other way on chip and is itself at most 1 % of rms(o) (asserted here as on the CPU); the result differs from the fp32
    kernel's by more than 50 d32 (the operands really were rounded); the overflow word stays 0."""
    lib = _clib()
    worst = Worst(64)
    Ts = DC.t_list("lp")
    flag = torch.zeros(4, dtype=torch.int32, device=DEV)
    for T in Ts:
        x, cp_all, dp_all, d_all, skip_old = DC.block_inputs(T)
        s0 = skip_old if accum else None
        run = lambda xx, cc, pp, dd_, ss, finite=True: _block(lib, "lp", xx, cc, pp, dd_, ss, finite, mode=mode, flag=flag if finite else None)
        got = run(x, cp_all, dp_all, d_all, s0)
        e, yard = DC.block_reference(T, mode, bool(accum), Ts[-1])
        assert max(e["widen_x"].max() * np.sqrt(2.0), e["widen_skip"].max()) <= 0.01 * e["o_rms"], (mode, T, "the widening is no longer small against o")
        worst.add(got[:, :CH] - e["x"], yard["x"], T, "x'", e["widen_x"])
        worst.add(got[:, CH:] - e["skip"], yard["skip"], T, "skip", e["widen_skip"])
        fp32 = _block(lib, "fused64", x, cp_all, dp_all, d_all, s0)
        assert np.abs(got - fp32).max() > 50 * max(yard["x"], yard["skip"]), (mode, T, "the 16-bit launch gave the fp32 kernel's result")
        if T in DC.t_alone("lp"):
            _alone_and_stale(run, x, got, cp_all, dp_all, d_all, s0)
    assert int(flag[0]) == 0, "the overflow word was set on inputs inside the fp16 range"
    assert worst.line(f"resblock_fused_lp accum={accum} mode={VC.MODES[mode]}") <= M, (mode, worst.w)


def test_lp_fp16_overflow_word():
    """One u of 7e4 at frame T - 1 of the last tile (T = W + 1): the fp16 launch sets a->flag to 3, the bf16 launch leaves it 0 on the same input."""
    lib = _clib()
    T = DC.TILE["lp"] + 1
    x, cp_all, dp_all, d_all, _ = DC.block_inputs(T)
    x = x.copy()
    x[1, 77, T - 1] = 7e4
    for mode, want in ((2, 3), (1, 0)):
        flag = torch.zeros(4, dtype=torch.int32, device=DEV)
        _block(lib, "lp", x, cp_all, dp_all, d_all, None, mode == 1, mode=mode, flag=flag)
        assert _np(flag).tolist() == [want, 0, 0, 0], (mode, _np(flag))


# ----------------------------------------------------------------------------------------------------------------- D: the input side

def _inproj(lib, x, scales, zero_n=None, x_off=0):
    """cmtts_launch_inproj on x [Bn][T][80] -> (rc, h [Bn][C][T] or None, the zero region's buffer as bytes or None).  scales: a float, or [Bn] floats."""
    Bn, T, _ = x.shape
    xd = torch.full((Bn * T * DC.MEL + 8,), float(DC.GARBAGE), device=DEV)
    xd[x_off:x_off + Bn * T * DC.MEL] = _dev(x).reshape(-1)
    Wi, bi = DC.inproj_weights()
    wf = _pack(("Wi",), "fragment_order", VC.kmajor(Wi[:, :, None]))
    h = _guard(Bn, CH, T)
    sb = None if np.isscalar(scales) else _dev(np.asarray(scales, F32))
    zb = None
    if zero_n is not None:
        zb = torch.full((zero_n * 4 + 8,), VC.SENTINEL, device=DEV)
    a = DC.InProjArgs(x=xd.data_ptr() + 4 * x_off, scale_b=None if sb is None else sb.data_ptr(), scale=float(scales) if sb is None else 0.0, wf=wf,
                      bias=_vec(("bi",), lambda: bi), h=h[1:].data_ptr(), B=Bn, T=T, M=DC.MEL, C=CH, zero=None if zb is None else zb.data_ptr(),
                      zero_f4=0 if zb is None else zero_n)
    rc = lib.cmtts_launch_inproj(C.byref(a), None)
    torch.cuda.synchronize()
    if rc != 0:
        assert (_np(h) == VC.SENTINEL).all(), "a refused launch wrote"
        return rc, None, None
    return rc, _rows(h, T), None if zb is None else _np(zb)


@pytest.mark.parametrize("per_utt", [False, True])
def test_inproj_vs_f64(per_utt):
    """inproj_kernel alone: relu(W (s x)^T + b) within M d32 of float64 with the scalar scale and with one scale per utterance, exact zeros where the
    definition is negative beyond the bound; the region to clear is cleared and not one byte behind it (1, 255 and 256 * grid + 3 units, and none);
    x 4 bytes off a 16-byte line is refused (-2) with h intact."""
    lib = _clib()
    worst = Worst(64)
    scales = list(DC.INPROJ_SCALES) if per_utt else DC.INPROJ_SCALES[0]
    for T in DC.INPROJ_T:
        x = DC.inproj_input(T)
        grid = (T + 63) // 64 * x.shape[0]
        ref, yard = DC.inproj_reference(T, per_utt)
        first = None
        for n in (None, 1, 255, 256 * grid + 3):
            rc, h, zb = _inproj(lib, x, scales, n)
            assert rc == 0, (T, n, rc)
            if first is None:
                first = h
                worst.add(h - ref, yard, T, "h")
                assert (h[ref < -M * yard] == 0).all(), (T, "relu left a negative")
                assert (h >= 0).all()
            else:
                assert np.array_equal(h, first), (T, n, "the cleared region changes h")
                assert (zb[:4 * n] == 0).all() and (zb[4 * n:] == VC.SENTINEL).all(), (T, n, "the region to clear")
        run = lambda xx, finite=True: _inproj(lib, xx, scales if not per_utt or xx.shape[0] > 1 else scales[1:])[1]
        if T in (1, 65):
            _alone_and_stale(run, x, first)
    rc, h, _ = _inproj(lib, DC.inproj_input(5), DC.INPROJ_SCALES[0], None, x_off=1)
    assert rc == -2 and h is None
    assert worst.line(f"inproj scale={'per utterance' if per_utt else 'scalar'} mode=fp32") <= M, worst.w


def _cond(lib, X, Mr, mode=0, flat=0, row_split=1):
    """cmtts_launch_cond_gemm (mode 0) / cmtts_launch_cond_gemm16 on X [Bn][256][T] -> [Bn][M][T]."""
    Bn, _, T = X.shape
    Wc, bc = DC.cond_weights(Mr)
    xg = _between(X, DC.GARBAGE)
    y = _guard(Bn, Mr, T)
    km = VC.kmajor(Wc[:, :, None])
    a = DC.CondGemmArgs(X=xg[1:].data_ptr(), Wf=_pack(("Wc", Mr), "fragment_order", km), bias=_vec(("bc", Mr), lambda: bc), Y=y[1:].data_ptr(), B=Bn, T=T, M=Mr, K=CH,
                        force=1, flat=flat, row_split=row_split)
    if mode:
        lay = "fragment16_split" if mode == 3 else "fragment16"
        rc = lib.cmtts_launch_cond_gemm16(C.byref(a), _pack(("Wc16", Mr, mode), lay, km, mode if mode < 3 else 0), mode, None)
    else:
        rc = lib.cmtts_launch_cond_gemm(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0, (Mr, T, mode, flat, row_split, rc)
    return _rows(y, T)


@pytest.mark.parametrize("Mr", DC.COND_M)
def test_cond_gemm_vs_f64(Mr):
    """cond_gemm_kernel alone (force = 1): per-utterance tiles (B = 2) and the flat column axis (B = 3: at T = 65 a 64-column tile straddles two
    utterances), one, two and M / 512 workgroups per frame tile — every form the same bits, and within M d32 of W X + b in float64."""
    lib = _clib()
    worst = Worst(64)
    for T in DC.COND_T:
        for Bn, flat in ((DC.B, 0), (3, 1)):
            X = DC.cond_input(Bn, T)
            ref, yard, _ = DC.cond_reference(Bn, Mr, T, 0)
            got = _cond(lib, X, Mr, 0, flat, 1)
            worst.add(got - ref, yard, T, f"flat={flat}")
            for rs in sorted({2, Mr // 512} - {1}):
                assert np.array_equal(_cond(lib, X, Mr, 0, flat, rs), got), (T, flat, rs, "row_split changes the bits")
            if flat:
                assert np.array_equal(_cond(lib, X, Mr, 0, 0, 1), got), (T, "the flat form changes the bits")
            elif T in (1, 65):
                _alone_and_stale(lambda xx, finite=True: _cond(lib, xx, Mr), X, got)
    assert worst.line(f"cond_gemm M={Mr} mode=fp32") <= M, worst.w


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("Mr", DC.COND_M)
def test_cond_gemm16_vs_f64(Mr, mode):
    """cond_gemm16_kernel alone on rounded operands (bf16, fp16; fp16x3: (hi, lo) pairs, the widening is the omitted lo x lo products)."""
    lib = _clib()
    worst = Worst(64)
    for T in DC.COND_T:
        X = DC.cond_input(DC.B, T)
        ref, yard, wd = DC.cond_reference(DC.B, Mr, T, mode)
        got = _cond(lib, X, Mr, mode)
        worst.add(got - ref, yard, T, "y", wd)
        if T in (1, 65):
            _alone_and_stale(lambda xx, finite=True: _cond(lib, xx, Mr, mode), X, got)
    assert worst.line(f"cond_gemm16 M={Mr} mode={VC.MODES[mode]}") <= M, (mode, worst.w)


def _expand(lib, T, off=0):
    p1, p2, m2p, pix = DC.expand_case(T)
    Bn, Mr = p1.shape[0], DC.EXPAND_M
    buf = torch.full(((Bn + 2) * Mr * T + 4,), VC.SENTINEL, device=DEV)
    p1d, p2d, md, pd = _dev(p1), _dev(p2), _dev(m2p), _dev(pix)
    rc = lib.cmtts_launch_cond_expand(p1d.data_ptr(), DC.EXPAND_LDP, DC.EXPAND_L, p2d.data_ptr(), DC.EXPAND_LD2, md.data_ptr(), pd.data_ptr(),
                                      buf.data_ptr() + 4 * (Mr * T + off), Bn, Mr, T, None)
    torch.cuda.synchronize()
    assert rc == 0, (T, off, rc)
    got = _np(buf)
    body = got[Mr * T + off:Mr * T + off + Bn * Mr * T]
    assert (got[:Mr * T + off] == VC.SENTINEL).all() and (got[Mr * T + off + Bn * Mr * T:] == VC.SENTINEL).all(), "written outside cp"
    return body.reshape(Bn, Mr, T)


def test_cond_expand_bitwise():
    """cond_expand_kernel<4> and <1>: a gather and one add, bit for bit expand_def — T around the 64- and 256-frame tiles, mel2ph holding 0, 1, L and
    L + 5, pidx holding -1, 0, ld2 - 1 and ld2 + 3; T % 4 == 0 with cp 4 bytes off a 16-byte line takes the one-frame form."""
    lib = _clib()
    n = 0
    for T, off in [(T, 0) for T in DC.EXPAND_T] + [(64, 1), (260, 1)]:
        p1, p2, m2p, pix = DC.expand_case(T)
        got = _expand(lib, T, off)
        for b in range(p1.shape[0]):
            assert np.array_equal(got[b], DC.expand_def(p1[b], p2, m2p[b], pix[b], DC.EXPAND_L, DC.EXPAND_LD2)), (T, off, b)
        n += 1
    report(f"DEN_F64 cond_expand: {n} launches (V = 4 and V = 1) bit for bit the float32 definition")


# ----------------------------------------------------------------------------------------------------------------- E: refusals

def test_refusals():
    """What a launcher's header excludes returns -2 and leaves the output sentinels intact.  Every call carries complete, correctly sized, valid
    buffers: a launcher that wrongly accepted would run entirely in bounds and fail the assertion."""
    lib = _clib()
    T, Bn = 40, DC.B
    x, cp_all, dp_all, d_all, _ = (np.zeros(s, F32) for s in ((Bn, CH, T), (Bn, NL * CH, T), (Bn, NL * CH), (Bn, NL * CH), ()))
    xg, cpg, dpd, dd = _between(x, 0.0), _between(cp_all, 0.0), _dev(dp_all), _dev(d_all)
    outs = [_guard(Bn, CH, T) for _ in range(3)]
    ud = torch.zeros((Bn, CH, T), device=DEV)
    big = torch.zeros(1 << 20, device=DEV)          # 4 MiB of zeros: stands in for every packed weight stream (the largest, F(4,3), is 3.2 MiB)

    def ra(**kw):
        a = DC.ResArgs(x_in=xg[1:].data_ptr(), cp=cpg[1:].data_ptr(), dp=dpd.data_ptr(), d=dd.data_ptr(), x_out=outs[0][1:].data_ptr(), skip=outs[1][1:].data_ptr(),
                       W3f=big.data_ptr(), b3=big.data_ptr(), Wof=big.data_ptr(), bo=big.data_ptr(), cp_bstride=NL * CH * T, vec_stride=NL * CH, B=Bn, T=T,
                       z=outs[2][1:].data_ptr(), u=ud.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    four = {"resblock": lambda a: lib.cmtts_launch_resblock(C.byref(a), None), "resblock_lp": lambda a: lib.cmtts_launch_resblock_lp(C.byref(a), 1, None),
            "resblock_split": lambda a: lib.cmtts_launch_resblock_split(C.byref(a), None), "resblock_w43": lambda a: lib.cmtts_launch_resblock_w43(C.byref(a), None)}
    rcs = {}
    for mode in (0, 3):
        rcs[f"resblock_lp mode={mode}"] = lib.cmtts_launch_resblock_lp(C.byref(ra()), mode, None)
    for name, fn in four.items():
        rcs[name + " x_out==x_in"] = fn(ra(x_out=xg[1:].data_ptr()))
    for name in ("resblock", "resblock_lp", "resblock_split", "resblock_w43"):
        rcs[name + " B=0"] = four[name](ra(B=0))
        rcs[name + " T=0"] = four[name](ra(T=0))
    for name, fn in (("resblock_split", four["resblock_split"]), ("resblock_split_out", lambda a: lib.cmtts_launch_resblock_split_out(C.byref(a), None)),
                     ("resblock_w43", four["resblock_w43"])):
        rcs[name + " z=null"] = fn(ra(z=None))
    rcs["resblock_w43 W3f=null"] = four["resblock_w43"](ra(W3f=None))

    y = _guard(Bn, 512, T)
    Xd = torch.zeros((Bn, CH, T), device=DEV)

    def cg(**kw):
        a = DC.CondGemmArgs(X=Xd.data_ptr(), Wf=big.data_ptr(), bias=big.data_ptr(), Y=y[1:].data_ptr(), B=Bn, T=T, M=512, K=CH, force=1, flat=0, row_split=1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for name, a in (("K=128", cg(K=128)), ("M=256", cg(M=256)), ("force=0 at 2 tiles", cg(force=0))):
        rcs["cond_gemm " + name] = lib.cmtts_launch_cond_gemm(C.byref(a), None)
    for name, (a, wf, mode) in (("mode=0", (cg(), big.data_ptr(), 0)), ("mode=4", (cg(), big.data_ptr(), 4)), ("wf16=null", (cg(), None, 1))):
        rcs["cond_gemm16 " + name] = lib.cmtts_launch_cond_gemm16(C.byref(a), wf, mode, None)
    idx = torch.zeros((Bn, T), dtype=torch.int64, device=DEV)
    for name, (Mr, L) in (("M=96", (96, 4)), ("L=0", (128, 0))):
        rcs["cond_expand " + name] = lib.cmtts_launch_cond_expand(big.data_ptr(), 8, L, big.data_ptr(), 8, idx.data_ptr(), idx.data_ptr(), y[1:].data_ptr(), Bn, Mr, T, None)
    xin = torch.zeros((Bn, T, DC.MEL), device=DEV)
    for name, kw in (("M=64", dict(M=64)), ("C=128", dict(C=128)), ("wf=null", dict(wf=None))):
        a = DC.InProjArgs(x=xin.data_ptr(), scale=1.0, wf=big.data_ptr(), bias=big.data_ptr(), h=y[1:].data_ptr(), B=Bn, T=T, M=DC.MEL, C=CH)
        for k, v in kw.items():
            setattr(a, k, v)
        rcs["inproj " + name] = lib.cmtts_launch_inproj(C.byref(a), None)
    torch.cuda.synchronize()
    assert all(rc == -2 for rc in rcs.values()), {n: rc for n, rc in rcs.items() if rc != -2}
    for t in outs + [y]:
        assert (_np(t) == VC.SENTINEL).all(), "a refused launch wrote"
    report(f"DEN_F64 refusals: {len(rcs)} excluded arguments over 9 launchers all returned -2")
