"""The frame-side and small kernels of kernels.hip called ALONE through the launch hooks of kernel_hooks.hip (cmtts_internal_k_*: the
production wrappers, grid choice included), and the generic conv kernel (conv_mfma.hip) through cmtts_launch_conv, against the float64
definition of the same operation (tests/frame_kernel_cases.py) at the edges the end-to-end goldens do not reach: T one off a wave, tile or
256-thread segment, ld != T, masks inside a tile, a carry across the 64 lanes, variance far below mean^2, values exactly on a bucket edge.

Every buffer has a guard row of SENTINEL before and after; the alignment columns [T, ld) of inputs hold +-GARBAGE, those of outputs SENTINEL
(the energy head and energy_embed write 0 there: asserted); nothing outside a kernel's documented footprint may be written.  Every
comparison is a check_* of frame_kernel_cases.py (bounds: its BOUNDS, M x the definition's own float32 error); every measured ratio is
printed as `FRAME_F64 <kernel> <case>: |d| ..., d32 ..., ratio ...`."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from conftest import report
import frame_kernel_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# argument types of the hooks (internal_hooks.h): p = pointer, i = int, l = long, f = float; the stream is the last p
SIGNATURES = {
    "embed_tokens": "pppppipiiiifp", "layernorm_ct": "ppppfpiiip", "softmax_cols": "ppiiiilp", "pos_embed_add": "pppppiiiiipp",
    "pos_embed_add_lr": "pippppppiiiip", "chan_linear": "pppppiiiiip", "stats_mlp": "pllpppppppiiiiip", "dense_small": "pllppppiiiip",
    "energy_embed": "ppppfpipppiiiipp", "durations": "pfpppiip", "durations_serial": "pfpppiip", "durations_table": "pppppiip",
    "durations_table_serial": "pppppiip", "pitch_table_scale": "ppppiiiip", "reduce_partials": "pippppiiiip",
    "ln_linear_energy": "pppfpppppiiippfpipppppp", "ln_linear": "pppfpppppiiiip", "cumsum_durations": "pppiip", "mel2ph": "ppiiip",
    "length_regulate": "pppiiiipp", "pitch_index": "pippifpipfpppiip", "gather_add": "ppppiiip", "lr_gather_add": "ppipppiiip",
    "mel_prep": "ppfpiiip", "mel_post": "pppfffpiiipp", "mel_post_rows": "ppppppiiipp", "diff_embed": "pppiip", "conv_post": "pppffpiiiiip",
}
CTYPES = {"p": C.c_void_p, "i": C.c_int, "l": C.c_long, "f": C.c_float}
_LIB = []


def _clib():
    if not _LIB:
        _lib.load()
        lib = C.CDLL(_lib.LIB_PATH)
        for name, sig in SIGNATURES.items():
            f = getattr(lib, "cmtts_internal_k_" + name)
            f.restype, f.argtypes = C.c_int, [CTYPES[ch] for ch in sig]
        lib.cmtts_launch_conv.restype = C.c_int
        lib.cmtts_launch_conv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _LIB.append(lib)
    return _LIB[0]


SENT = {np.dtype(np.float32): FC.SENTINEL, np.dtype(np.int64): FC.ISENT, np.dtype(np.int32): FC.ISENT, np.dtype(np.uint8): 0xAB, np.dtype(np.uint32): 0xABABABAB}


class Buf:
    """A device buffer with a guard row of the sentinel before and after it: the contents `a`, or the sentinel everywhere (`shape`)."""

    def __init__(self, a=None, shape=None, dtype=np.float32):
        if a is not None:
            a = np.ascontiguousarray(a)
            shape, dtype = a.shape, a.dtype
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape))
        self.g = FC.ceil4(max(self.shape[-1] if self.shape else 1, 64))
        host = np.full(self.n + 2 * self.g, SENT[self.dtype], self.dtype)
        if a is not None:
            host[self.g:self.g + self.n] = a.reshape(-1)
        view = host.view(np.int32) if self.dtype == np.uint32 else host      # (torch has no uint32 arithmetic; the bits travel as int32)
        self.t = torch.from_numpy(view).to(DEV)
        self.ptr = self.t.data_ptr() + self.g * self.dtype.itemsize

    def at(self, elements):
        """The address `elements` into the buffer."""
        return self.ptr + elements * self.dtype.itemsize

    def get(self):
        """The contents after a launch; the guard rows must still hold the sentinel."""
        host = self.t.cpu().numpy().view(self.dtype)
        assert (host[:self.g] == SENT[self.dtype]).all() and (host[self.g + self.n:] == SENT[self.dtype]).all(), "written outside the buffer (guard rows)"
        return host[self.g:self.g + self.n].reshape(self.shape).copy()


def _p(b):
    return None if b is None else (b.ptr if isinstance(b, Buf) else int(b))


def _dev(a):
    return None if a is None else Buf(a)


def _run(name, *args):
    rc = getattr(_clib(), "cmtts_internal_k_" + name)(*[_p(a) if (a is None or isinstance(a, Buf)) else a for a in args], None)
    torch.cuda.synchronize()
    return rc


def _sentinel_beyond(got, T, what):
    assert (got[..., T:] == FC.SENTINEL).all(), (what, "written beyond T")
    return got[..., :T]


def _line(kernel, case, r):
    report(f"FRAME_F64 {kernel} {case}: |d| {r.d:.2e}, d32 {r.d32:.2e}, ratio {float(r):.2f}" + (f", pre-rounding error {r.err_units:.2e} buckets" if hasattr(r, "err_units") else ""))


# ----------------------------------------------------------------------------------------------------------------- the heads

def _head_dev(c):
    return {k: _dev(c[k]) for k in ("x", "g", "be", "W", "bias", "ln_lens", "out_lens")}


@pytest.mark.parametrize("T", FC.HEAD_T)
def test_layernorm_ct_vs_f64(T):
    """layernorm_ct_kernel: four input regimes, with and without lens, eps 1e-12 (and 1e-5 once); masked columns exactly 0, the dead column
    exactly beta, nothing written in [T, ld)."""
    for ld in FC.head_lds(T):
        for regime in FC.HEAD_REGIMES:
            for mask, eps in (("none", FC.LN_EPS), ("same", FC.LN_EPS)) + ((("none", FC.LN_EPS_ENC),) if regime == "unit" else ()):
                c = FC.head_case(T, ld, regime, mask, 1, eps)
                d = _head_dev(c)
                out = Buf(shape=(FC.HEAD_B, FC.HEAD_C, ld))
                assert _run("layernorm_ct", d["x"], out, d["g"], d["be"], eps, d["ln_lens"], FC.HEAD_B, T, ld) == 0
                _line("layernorm_ct", f"T={T} ld={ld} {regime} lens={mask} eps={eps:g}", FC.check_layernorm(_sentinel_beyond(out.get(), T, "layernorm_ct"), c))


@pytest.mark.parametrize("T", FC.HEAD_T)
def test_ln_linear_vs_f64(T):
    """ln_linear_kernel<1 | 10 | 11>: regimes x masks (ln_lens and out_lens null, equal, different) x row strides; any other O is declined
    (-2) with nothing written."""
    for O in FC.LN_O:
        for ld in FC.head_lds(T):
            for regime in FC.HEAD_REGIMES:
                for mask in FC.HEAD_MASKS:
                    c = FC.head_case(T, ld, regime, mask, O)
                    d = _head_dev(c)
                    out = Buf(shape=(FC.HEAD_B, T, O))
                    assert _run("ln_linear", d["x"], d["g"], d["be"], c["eps"], d["W"], d["bias"], out, d["ln_lens"], d["out_lens"], FC.HEAD_B, T, ld, O) == 0
                    _line(f"ln_linear<{O}>", f"T={T} ld={ld} {regime} masks={mask}", FC.check_ln_linear(out.get(), c))
    c = FC.head_case(T, FC.head_lds(T)[0], "unit", "none", 16)
    d = _head_dev(c)
    for O in (5, 16):
        out = Buf(shape=(FC.HEAD_B, T, 16))
        assert _run("ln_linear", d["x"], d["g"], d["be"], c["eps"], d["W"], d["bias"], out, None, None, FC.HEAD_B, T, c["ld"], O) == -2
        assert (out.get() == FC.SENTINEL).all()


@pytest.mark.parametrize("T", FC.HEAD_T)
def test_chan_linear_vs_f64(T):
    """chan_linear_kernel, C = 256, O in {1, 10, 11, 16}, with and without lens."""
    for O in FC.CHAN_O:
        for ld in FC.head_lds(T):
            for regime in ("unit", "relu", "offset"):
                for mask in ("none", "same"):
                    c = FC.head_case(T, ld, regime, mask, O)
                    d = _head_dev(c)
                    out = Buf(shape=(FC.HEAD_B, T, O))
                    assert _run("chan_linear", d["x"], d["W"], d["bias"], out, d["out_lens"], FC.HEAD_B, FC.HEAD_C, T, ld, O) == 0
                    _line(f"chan_linear O={O}", f"T={T} ld={ld} {regime} lens={mask}", FC.check_chan_linear(out.get(), c))


@pytest.mark.parametrize("T", FC.HEAD_T)
def test_energy_head_vs_f64(T):
    """ln_linear_kernel<1, EE 1 | 2> and energy_embed_kernel on the same cases: scalar control 1 and 1.3, a control table, teacher-forced
    targets on bin edges / outside the bins / NaN; the fused head has the bits of k_ln_linear + k_energy_embed."""
    for ld, mode in [(ld, mode) for t, ld, mode in FC.energy_cases() if t == T]:
        c = FC.energy_case(T, ld, mode)
        d = _head_dev(c)
        xin, bins, E, tab, tgt = (_dev(c[k]) for k in ("xin", "bins", "E", "e_table", "e_target"))
        res = []
        for fused in (True, False):
            out, out1 = Buf(shape=(FC.HEAD_B, T, 1)), Buf(shape=(FC.HEAD_B, FC.HEAD_C, ld))
            e_idx, e_scaled = Buf(shape=(FC.HEAD_B, T), dtype=np.int64), Buf(shape=(FC.HEAD_B, T))
            if fused:
                assert _run("ln_linear_energy", d["x"], d["g"], d["be"], c["eps"], d["W"], d["bias"], out, d["ln_lens"], d["out_lens"], FC.HEAD_B, T, ld,
                            xin, tgt, c["e_control"], bins, FC.NBINS, E, out1, e_idx, e_scaled, tab) == 0
            else:
                assert _run("ln_linear", d["x"], d["g"], d["be"], c["eps"], d["W"], d["bias"], out, d["ln_lens"], d["out_lens"], FC.HEAD_B, T, ld, 1) == 0
                assert _run("energy_embed", xin, out, e_scaled, tgt, c["e_control"], bins, FC.NBINS, E, out1, e_idx, FC.HEAD_B, FC.HEAD_C, T, ld, tab) == 0
            got = {"out": out.get(), "e_idx": e_idx.get(), "out1": out1.get(), "e_scaled": e_scaled.get()}
            r = FC.check_energy(got, c)
            _line("energy_head" if fused else "energy_embed", f"T={T} ld={ld} {mode}", r)
            res.append(got)
        for k in res[0]:
            FC.same_bits("energy_head", res[0][k], res[1][k], (T, ld, mode, k, "the fused head differs from k_ln_linear + k_energy_embed"))


# ----------------------------------------------------------------------------------------------------------------- the integer stages

def _durations(kernel, c, ctl):
    B, L = c["logd"].shape
    logd = _dev(c["logd"])
    d, cum, ml = Buf(shape=(B, L)), Buf(shape=(B, L), dtype=np.int32), Buf(shape=(B,), dtype=np.int64)
    assert _run(kernel, logd, _dev(ctl) if isinstance(ctl, np.ndarray) else float(ctl), d, cum, ml, B, L) == 0
    return {"d_rounded": d.get(), "cum": cum.get(), "mel_len": ml.get()}


@pytest.mark.parametrize("L", FC.DUR_L)
def test_durations_vs_f64(L):
    """The four durations kernels (wave, serial, table wave, table serial): wave == serial and a constant table == the scalar form bit for bit;
    cum and mel_len exactly the truncated sums of the kernel's own d_rounded; the clear set exactly float64's, the spread set off by one
    step only on a rounding boundary.  B = 65 once (the serial kernels put 64 utterances in a workgroup)."""
    flips, scalar = 0.0, {}
    for kind, ctl, table, B in FC.dur_cases(L):
        c = FC.dur_case(L, kind, ctl, table, B)
        arg = c["control"] if table is None else c["table"]
        wave, serial = ("durations", "durations_serial") if table is None else ("durations_table", "durations_table_serial")
        got = _durations(wave, c, arg)
        flips = max(flips, float(FC.check_durations(got, c)))
        other = _durations(serial, c, arg)
        for f in ("d_rounded", "cum", "mel_len"):
            FC.same_bits(serial, other[f], got[f], (L, B, kind, ctl, table, f, "serial differs from wave"))
            if table is None:
                scalar[(kind, B, ctl)] = got
            elif table == "const":
                FC.same_bits(wave, got[f], scalar[(kind, B, ctl)][f], (L, B, kind, ctl, f, "a constant table differs from the scalar form"))
    report(f"FRAME_F64 durations L={L}: exact; largest share of durations one step from float64's (all on a rounding boundary) {flips:.2e}")


@pytest.mark.parametrize("L", FC.CUM_L)
def test_cumsum_durations_and_mel2ph(L):
    """cumsum_durations_kernel (fractional, negative and zero entries, an utterance of all zeros) and mel2ph_kernel for T below the shortest
    mel_len, between the lengths and above the longest: exact."""
    for scale in FC.CUM_SCALES:
        c = FC.cumsum_case(L, scale)
        B = c["B"]
        cum, ml = Buf(shape=(B, L), dtype=np.int32), Buf(shape=(B,), dtype=np.int64)
        assert _run("cumsum_durations", _dev(c["dur"]), cum, ml, B, L) == 0
        FC.check_cumsum({"cum": cum.get(), "mel_len": ml.get()}, c)
        for T in FC.CUM_T:
            m2p = Buf(shape=(B, T), dtype=np.int64)
            assert _run("mel2ph", cum, m2p, B, L, T) == 0
            FC.check_mel2ph(m2p.get(), c, T)
    report(f"FRAME_F64 cumsum_durations / mel2ph L={L}: exact")


@pytest.mark.parametrize("T", FC.PITCH_T)
def test_pitch_index_vs_f64(T):
    """pitch_index_kernel: O = 11 with the uv logit in column 10 (0 and -0 voiced, the smallest positive normal unvoiced) and O = 10 with
    uv_mask bytes; statistics with stride 1 and 2; std_scale 1 and 1.3."""
    for O, stat_ld, std_scale in FC.PITCH_COMBOS:
        c = FC.pitch_case(T, O, stat_ld, std_scale)
        cwt = _dev(c["cwt"])
        if stat_ld == 2:
            st = _dev(c["stats"])
            mean_p, std_p = st.ptr, st.at(1)
        else:
            mean_b, std_b = _dev(c["mean"]), _dev(c["std"])
            mean_p, std_p = mean_b.ptr, std_b.ptr
        uv_mask = _dev(c["uv_mask"])
        r, idx, f0 = Buf(shape=(FC.PITCH_B, T)), Buf(shape=(FC.PITCH_B, T), dtype=np.int64), Buf(shape=(FC.PITCH_B, T))
        assert _run("pitch_index", cwt, O, mean_p, std_p, stat_ld, c["std_scale"], cwt.at(10) if O == 11 else None, O if O == 11 else 0, uv_mask, FC.PITCH_EPS,
                    r, idx, f0, FC.PITCH_B, T) == 0
        _line("pitch_index", f"T={T} O={O} stat_ld={stat_ld} std_scale={std_scale}", FC.check_pitch({"r_ws": r.get(), "p_idx": idx.get(), "f0_denorm": f0.get()}, c))


@pytest.mark.parametrize("T", FC.GATHER_T)
def test_pitch_table_scale_and_gathers(T):
    """pitch_table_scale_kernel (mel_len = T, > T, 0, T // 2), length_regulate_kernel with and without padv, lr_gather_add_kernel,
    gather_add_kernel with ldl != L: exact."""
    p = FC.pitch_table_case(T)
    cwt = Buf(p["cwt"])
    assert _run("pitch_table_scale", cwt, _dev(p["mel2ph"]), _dev(p["cum"]), _dev(p["ptab"]), p["B"], p["O"], p["L"], T) == 0
    FC.check_pitch_table(cwt.get(), p)
    g = FC.gather_case(T)
    B, Cn = g["B"], FC.GATHER_C
    out1, m2p, idx, E = (_dev(g[k]) for k in ("out1", "mel2ph", "idx", "E"))
    for padv in (None, g["padv"]):
        xlr = Buf(shape=(B, Cn, T))
        assert _run("length_regulate", out1, m2p, xlr, B, Cn, FC.GATHER_LDL, T, _dev(padv)) == 0
        FC.check_length_regulate(xlr.get(), g, padv is not None)
    out = Buf(shape=(B, Cn, T))
    assert _run("lr_gather_add", out1, m2p, FC.GATHER_LDL, idx, E, out, B, Cn, T) == 0
    FC.check_lr_gather_add(out.get(), g)
    out = Buf(shape=(B, Cn, T))
    assert _run("gather_add", _dev(g["x"]), idx, E, out, B, Cn, T) == 0
    FC.check_gather_add(out.get(), g)
    report(f"FRAME_F64 pitch_table_scale / length_regulate / lr_gather_add / gather_add T={T}: exact")


# ----------------------------------------------------------------------------------------------------------------- positions

@pytest.mark.parametrize("T", FC.POS_T)
def test_position_kernels_vs_f64(T):
    """pos_embed_add_kernel, pos_embed_add_lr_kernel, embed_tokens_kernel: false flags in the middle of the valid span, lens shorter than the
    flagged span, the table branch, the computed branch and both (tab_rows 0 / 100 / 700)."""
    alpha = _dev(np.asarray([FC.POS_ALPHA], np.float32))
    for Cn, kernels in ((FC.POS_C, ("pos_embed_add", "pos_embed_add_lr")), (FC.EMB_C, ("embed_tokens",))):
        omega = _dev(FC.pos_omega(Cn))
        for rows in FC.POS_TAB_ROWS:
            tab = _dev(FC.pos_table(rows, Cn))
            if "pos_embed_add" in kernels:
                c = FC.pos_case(T)
                x = _dev(c["x"])
                for masked in (False, True):
                    out = Buf(shape=(FC.POS_B, Cn, c["ld"]))
                    assert _run("pos_embed_add", x, out, alpha, omega, tab, rows, FC.POS_B, Cn, T, c["ld"], _dev(c["lens"]) if masked else None) == 0
                    _line("pos_embed_add", f"T={T} tab_rows={rows} lens={masked}", FC.check_pos_embed_add(_sentinel_beyond(out.get(), T, "pos_embed_add"), c, masked))
                for pad0_zero in (True, False):
                    p = FC.pos_lr_case(T, pad0_zero)
                    out = Buf(shape=(FC.POS_B, Cn, T))
                    assert _run("pos_embed_add_lr", _dev(p["src"]), FC.LR_LDL, _dev(p["mel2ph"]), _dev(p["padv"]), out, alpha, omega, tab, rows, FC.POS_B, Cn, T) == 0
                    _line("pos_embed_add_lr", f"T={T} tab_rows={rows} padv[0]{'=' if pad0_zero else '!='}0", FC.check_pos_embed_add_lr(out.get(), p))
            else:
                e = FC.embed_case(T)
                out = Buf(shape=(FC.POS_B, Cn, e["ld"]))
                assert _run("embed_tokens", _dev(e["texts"]), _dev(e["lens"]), _dev(e["E"]), omega, tab, rows, out, FC.POS_B, T, e["ld"], Cn, e["scale"]) == 0
                _line("embed_tokens", f"L={T} tab_rows={rows}", FC.check_embed_tokens(_sentinel_beyond(out.get(), T, "embed_tokens"), e))


# ----------------------------------------------------------------------------------------------------------------- small dense

@pytest.mark.parametrize("K", FC.DENSE_K)
def test_dense_small_vs_f64(K):
    """dense_small_kernel<4 | 16> (K = 1024 takes the 16-slice kernel at every B, N here; K = 3 is fewer rows than slices): no activation, ReLU,
    Mish over pre-activations in [-30, 30]; with and without bias / add; a strided input once per shape."""
    for B in FC.DENSE_B:
        for N in FC.DENSE_N:
            for in_ks, act, wb, wa in ((1, FC.DENSE_NONE, False, False), (1, FC.DENSE_RELU, True, False), (1, FC.DENSE_MISH, True, True), (3, FC.DENSE_MISH, True, False)):
                c = FC.dense_case(B, K, N, in_ks)
                out = Buf(shape=(B, N))
                assert _run("dense_small", _dev(c["raw"]), K * in_ks, in_ks, _dev(c["Wt"]), _dev(c["bias"]) if wb else None, _dev(c["add"]) if wa else None, out,
                            B, K, N, act) == 0
                _line(f"dense_small<{FC.dense_slices(B, K, N)}>", f"B={B} K={K} N={N} in_ks={in_ks} act={act} bias={wb} add={wa}", FC.check_dense(out.get(), c, act, wb, wa))


def test_stats_mlp_vs_f64_and_dense_small():
    """stats_mlp_kernel against float64 and bit for bit against three dense_small launches; a shape that needs more than 48 KB of LDS is
    declined (-2) with the output untouched."""
    for shape in FC.STATS_SHAPES:
        c = FC.stats_case(shape)
        K0, N0, N1, N2 = shape
        x, W, b = _dev(c["x"]), [_dev(w) for w in c["W"]], [_dev(v) for v in c["b"]]
        out = Buf(shape=(FC.STATS_B, N2))
        assert _run("stats_mlp", x, K0, 1, W[0], b[0], W[1], b[1], W[2], b[2], out, FC.STATS_B, K0, N0, N1, N2) == 0
        _line("stats_mlp", "x".join(map(str, shape)), FC.check_stats_mlp(out.get(), c))
        h1, h2, o3 = Buf(shape=(FC.STATS_B, N0)), Buf(shape=(FC.STATS_B, N1)), Buf(shape=(FC.STATS_B, N2))
        assert _run("dense_small", x, K0, 1, W[0], b[0], None, h1, FC.STATS_B, K0, N0, FC.DENSE_RELU) == 0
        assert _run("dense_small", h1, N0, 1, W[1], b[1], None, h2, FC.STATS_B, N0, N1, FC.DENSE_RELU) == 0
        assert _run("dense_small", h2, N1, 1, W[2], b[2], None, o3, FC.STATS_B, N1, N2, FC.DENSE_NONE) == 0
        FC.same_bits("stats_mlp", out.get(), o3.get(), (shape, "differs from three dense_small launches"))
    K0, N0, N1, N2 = FC.STATS_DECLINED
    out = Buf(shape=(FC.STATS_B, N2))
    assert _run("stats_mlp", x, K0, 1, W[0], b[0], W[1], b[1], W[2], b[2], out, FC.STATS_B, K0, N0, N1, N2) == -2
    assert (out.get() == FC.SENTINEL).all()


@pytest.mark.parametrize("L", FC.SOFTMAX_L)
def test_softmax_cols_vs_f64(L):
    """softmax_cols_kernel in place: lengths [L, mid, 1, 0], scores that overflow expf without the max subtraction; masked keys exactly 0, a
    len = 0 utterance all zeros, [L, ld) untouched."""
    for regime in FC.SOFTMAX_REGIMES:
        c = FC.softmax_case(L, regime)
        st = Buf(c["st"])
        nz = FC.SOFTMAX_B * FC.SOFTMAX_H
        assert _run("softmax_cols", st, _dev(c["lens"]), nz, FC.SOFTMAX_H, L, c["ld"], L * c["ld"]) == 0
        got = st.get()
        assert np.array_equal(got[:, :, L:], c["st"][:, :, L:]), "written beyond L"
        _line("softmax_cols", f"L={L} {regime}", FC.check_softmax(got[:, :, :L], c))


@pytest.mark.parametrize("Cn", FC.REDUCE_C)
def test_reduce_partials_exact_and_vs_f64(Cn):
    """reduce_partials_kernel: the fp32 left-to-right sum exactly, float64 by ratio; with and without bias, res, lens."""
    for L in FC.REDUCE_L:
        c = FC.reduce_case(Cn, L)
        part, bias, res, lens = (_dev(c[k]) for k in ("part", "bias", "res", "lens"))
        for wb, wr, wl in ((True, True, True), (False, True, False), (True, False, True), (False, False, False)):
            out = Buf(shape=(FC.REDUCE_B, Cn, c["ld"]))
            assert _run("reduce_partials", part, FC.REDUCE_NSEG, bias if wb else None, res if wr else None, lens if wl else None, out, FC.REDUCE_B, Cn, L, c["ld"]) == 0
            _line("reduce_partials", f"C={Cn} L={L} bias={wb} res={wr} lens={wl}", FC.check_reduce(_sentinel_beyond(out.get(), L, "reduce_partials"), c, wb, wr, wl))


@pytest.mark.parametrize("T", FC.POST_T)
def test_conv_post_vs_f64(T):
    """conv_post_kernel and conv_post_v4_kernel against tanh(conv(leaky(x / 3))) in float64 and each other bit for bit: C 32 and 30 (no
    multiple of the four channels in flight), KW 7 and 3, ld = T rounded up to 4 (the clamped neighbour loads at the row ends), and
    ld = T + 1 once (the scalar kernel by the launcher's rule)."""
    for Cn in FC.POST_C:
        for KW in FC.POST_KW:
            for ld in (FC.ceil4(T), T + 1) if (Cn, KW) == (32, 7) else (FC.ceil4(T),):
                c = FC.post_case(T, Cn, KW, ld)
                x, w, bias = _dev(c["x"]), _dev(c["w"]), _dev(c["bias"])
                assert x.ptr % 16 == 0
                got = []
                for v4 in (1, 0):
                    prev = _lib.internal_set("post_v4", v4)
                    try:
                        wav = Buf(shape=(FC.POST_B, T))
                        assert _run("conv_post", x, w, bias, FC.POST_DIV, FC.POST_SLOPE, wav, FC.POST_B, Cn, T, ld, KW) == 0
                    finally:
                        _lib.internal_set("post_v4", prev)
                    got.append(wav.get())
                    _line("conv_post" + ("_v4" if v4 and FC.post_takes_v4(T, ld, KW) else ""), f"T={T} C={Cn} KW={KW} ld={ld}", FC.check_conv_post(got[-1], c))
                FC.same_bits("conv_post", got[0], got[1], (T, Cn, KW, ld, "post_v4 on / off"))


@pytest.mark.parametrize("T", FC.MEL_T)
def test_mel_kernels_vs_f64(T):
    """mel_prep_kernel, mel_post_kernel, mel_post_rows_kernel (rows with and without the re-noise bit, the final bit routed to out_final),
    diff_embed_kernel; the flag word goes to 2 on a non-finite F only when it was 0."""
    c = FC.mel_case(T)
    B, M = FC.MEL_B, FC.MEL_M
    x, F, noise = _dev(c["x"]), _dev(c["F"]), _dev(c["noise"])
    for per_utt in (False, True):
        hin = Buf(shape=(B, M, T))
        assert _run("mel_prep", x, _dev(c["scale_b"]) if per_utt else None, c["scale"], hin, B, T, M) == 0
        _line("mel_prep", f"T={T} per-utterance={per_utt}", FC.check_mel_prep(hin.get(), c, per_utt))
    flag = Buf(np.zeros(1, np.uint32))
    for wx, wn in ((True, True), (True, False), (False, False)):
        out = Buf(shape=(B, T, M))
        assert _run("mel_post", F, x if wx else None, noise if wn else None, *c["c"], out, B, T, M, flag) == 0
        _line("mel_post", f"T={T} xold={wx} noise={wn}", FC.check_mel_post(out.get(), c, wx, wn))
    assert flag.get()[0] == 0
    rows = np.zeros(B, dtype=[("c", np.float32, 3), ("flags", np.uint32)])
    rows["c"], rows["flags"] = c["rows"][:, :3], c["rows"][:, 3].astype(np.uint32)
    out, fin = Buf(shape=(B, T, M)), Buf(shape=(B, T, M))
    assert _run("mel_post_rows", F, x, noise, _dev(rows.view(np.uint8).reshape(B, 16)), out, fin, B, T, M, flag) == 0
    _line("mel_post_rows", f"T={T}", FC.check_mel_post_rows(out.get(), fin.get(), c, FC.SENTINEL))
    assert flag.get()[0] == 0
    bad = c["F"].copy()
    bad[1, 3, 0] = np.inf
    rows_d = _dev(rows.view(np.uint8).reshape(B, 16))
    for before, after in ((0, 2), (1, 1)):
        flag = Buf(np.asarray([before], np.uint32))
        assert _run("mel_post", _dev(bad), x, None, *c["c"], Buf(shape=(B, T, M)), B, T, M, flag) == 0
        assert flag.get()[0] == after
        flag = Buf(np.asarray([before], np.uint32))
        assert _run("mel_post_rows", _dev(bad), x, noise, rows_d, Buf(shape=(B, T, M)), Buf(shape=(B, T, M)), B, T, M, flag) == 0
        assert flag.get()[0] == after
    emb = Buf(shape=(B, FC.DIFF_C))
    assert _run("diff_embed", _dev(c["t"]), _dev(FC.pos_omega(FC.DIFF_C)), emb, B, FC.DIFF_C) == 0
    _line("diff_embed", f"T={T}", FC.check_diff_embed(emb.get(), c))


# ----------------------------------------------------------------------------------------------------------------- conv_mfma.hip

def _conv_launch(c, override=None):
    """cmtts_launch_conv on the case's buffers -> (return code, name -> output contents after the launch)."""
    a, bufs = c["a"], c["bufs"]
    dev = {k: Buf(v) for k, v in bufs.items() if k != "W"}
    args = FC.ConvArgs()
    args.A, args.X = dev["A"].ptr, dev["X"].ptr
    for f in FC.CONV_FIELDS:
        setattr(args, f, a[f])
    for f, v in (override or {}).items():
        setattr(args, f, v)
    for o, spec in zip(args.out, c["out"]):
        for f in FC.OUT_FIELDS:
            setattr(o, f, spec[f])
        for f in ("Y", "bias", "bvec", "res", "lens"):
            setattr(o, f, dev[spec[f]].ptr if spec[f] is not None else None)
    rc = _clib().cmtts_launch_conv(C.addressof(args), c["epi"], c["nbatch"], None)
    torch.cuda.synchronize()
    return rc, {o["Y"]: dev[o["Y"]].get() for o in c["out"]}


@pytest.mark.parametrize("config", FC.CONV_CONFIGS)
def test_generic_conv_vs_f64(config):
    """conv1d_mfma_kernel through cmtts_launch_conv, one test per tile configuration (frame_kernel_cases.conv_case), N in {1, tile - 1, tile,
    tile + 1} and Tin < N once, with the epilogue operands the product uses that configuration with; the launcher's refusals (-2, nothing
    written): a gated M off 64, a split off 128, a halo above 64."""
    tile = FC.CONV_TILE_N[config]
    shapes = [(N, 0) for N in (2 if config == "convT" else 1, tile - 1, tile, tile + 1)]
    if config != "convT":
        shapes.append((tile + 1, 1))
    if config == "split":
        shapes.append((tile, 1))
    for N, variant in shapes:
        c = FC.conv_case(config, N, variant)
        rc, got = _conv_launch(c)
        assert rc == 0
        _line("conv_generic", f"{config} N={N}" + (" Tin<N" if variant else "") + (" accum" if variant and config == "split" else ""), FC.check_conv(got, c))
    refusals = {"gated": {"M": 96}, "split": {"split": 64}, "tb5": {"dil": 9}}
    if config in refusals:
        c = FC.conv_case(config, tile)
        rc, got = _conv_launch(c, refusals[config])
        assert rc == -2
        for name, v in got.items():
            assert np.array_equal(v, c["bufs"][name]), (config, name, "a refused launch wrote")
