"""Inputs, float64 definitions, yardsticks and argument-block mirrors shared by tests/test_vocoder_kernel_cases_cpu.py and
tests/test_gpu_vocoder_kernels.py (not a test module): the HiFi-GAN vocoder's kernels called ALONE through their launch hooks
(cm-tts_amd/csrc/resblock_pair.h, conv_args.h).  Every reference is the definition evaluated in float64 — in the 16-bit modes on operands
rounded from their fp32 value, oracle.cmtts_oracle.operands16's scheme — and the same function evaluated in float32 is the yardstick `d32`
the kernels' errors are measured in.  Nothing here is computed from a kernel.  Computed once per case and left unchanged."""
import ctypes as C
import functools

import numpy as np

from oracle import cmtts_oracle as O
from resample_cases import GARBAGE
from text_kernel_cases import ConvArgs, conv_args, kmajor  # noqa: F401  (cmtts_launch_conv16 takes the text side's ConvArgs)

F32, F64 = np.float32, np.float64

# ----------------------------------------------------------------------------------------------------------------- argument blocks


class PairArgs(C.Structure):
    """struct PairArgs (cm-tts_amd/csrc/resblock_pair.h)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("w1f", C.c_void_p), ("b1", C.c_void_p), ("w2f", C.c_void_p), ("b2", C.c_void_p),
                ("bstride", C.c_long), ("B", C.c_int), ("C", C.c_int), ("T", C.c_int), ("ld", C.c_int), ("k", C.c_int), ("dil", C.c_int),
                ("accum", C.c_int), ("slope", C.c_float), ("dbg", C.c_void_p)]


class ConvXlArgs(C.Structure):
    """struct ConvXlArgs (cm-tts_amd/csrc/resblock_pair.h)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("wf", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p),
                ("bstride", C.c_long), ("B", C.c_int), ("C", C.c_int), ("T", C.c_int), ("ld", C.c_int), ("k", C.c_int),
                ("dil", C.c_int), ("accum", C.c_int), ("slope", C.c_float), ("relu", C.c_int), ("cin", C.c_int), ("xbstride", C.c_long),
                ("wino_force", C.c_int), ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("ln_eps", C.c_float), ("row_split", C.c_int)]


# ----------------------------------------------------------------------------------------------------------------- operand rounding

MODES = {0: None, 1: "bf16", 2: "fp16", 3: "fp16x3"}      # cmtts_vocoder_set_precision's modes
SLOPE = float(F32(0.1))          # the float the launches are given (hifigan lrelu_slope)
M = 10                           # every bound of the GPU module is M x d32 (a ratio of a few is a reordered fp32 sum; above 10 it is a finding)
SENTINEL = 12345.0               # what an fp32 output buffer holds before a launch
SENTINEL16 = 0x7A7A              # and a 16-bit one
B = 2


def round16(a, mode):
    """a rounded as the kernels round an MFMA operand: from its fp32 value to bf16 (1), fp16 (2) or hi + lo fp16 (3); 0: unchanged.  In a's dtype."""
    a = np.asarray(a)
    if not mode:
        return a
    return np.asarray(O.quant16(a, MODES[mode])).astype(a.dtype)      # (quant16 answers in fp32, where all three are exact)


def decode16(u, mode):
    """The device's uint16 image -> float32: bf16 (1) shift left 16, fp16 (2) view as float16."""
    u = np.ascontiguousarray(u).view(np.uint16)
    if mode == 1:
        return (u.astype(np.uint32) << np.uint32(16)).view(F32)
    return u.view(np.float16).astype(F32)


def ulp16(v, mode):
    """Spacing of the 16-bit format (1 = bf16: 8 significant bits, 2 = fp16: 11, subnormals below 2^-14) at |v|."""
    e = np.frexp(np.abs(np.asarray(v, F64)))[1] - 1
    return np.ldexp(1.0, np.maximum(e, -126) - 7) if mode == 1 else np.ldexp(1.0, np.maximum(e, -14) - 10)


# ----------------------------------------------------------------------------------------------------------------- definitions

def leaky(v, dtype, slope=SLOPE):
    v = np.asarray(v, dtype)
    return np.where(v > 0, v, v * dtype(slope))


def conv_same(a, w, dil, dtype):
    """a [Cin][T]: the operand as staged (activated, rounded); zero outside [0, T), 'same' padding dil (k - 1) / 2 -> [Cout][T]."""
    co, ci, k = w.shape
    T = a.shape[1]
    pad = dil * (k - 1) // 2
    ap = np.zeros((ci, T + 2 * pad), dtype)
    ap[:, pad:pad + T] = a
    y = np.zeros((co, T), dtype)
    for tau in range(k):
        y += np.ascontiguousarray(w[:, :, tau], dtype) @ ap[:, tau * dil:tau * dil + T]
    return y


def conv_def(x, w, b, dil, mode, dtype, res=None, y_old=None, act=True):
    """One ResBlock conv (hifigan/models.py:96-103): ((W * round16(leaky(x)) + b) + res) + y_old; act = False: x is the staged operand already."""
    a = round16(leaky(x, dtype) if act else np.asarray(x, dtype), mode)
    y = conv_same(a, round16(np.asarray(w, dtype), mode), dil, dtype) + np.asarray(b, dtype)[:, None]
    if res is not None:
        y = y + np.asarray(res, dtype)
    if y_old is not None:
        y = y + np.asarray(y_old, dtype)
    return y


def pair_def(x, w1, b1, w2, b2, dil, mode, dtype, y_old=None, a2=None):
    """conv1 (dilation dil) -> LeakyReLU -> conv2 -> + x [+ y_old] -> (y, xt); a2: conv2's staged operand given instead of formed from xt."""
    xt = conv_def(x, w1, b1, dil, mode, dtype)
    if a2 is None:
        a2 = round16(leaky(xt, dtype), mode)
    y = conv_def(a2, w2, b2, 1, mode, dtype, res=x, y_old=y_old, act=False)
    return y, xt


RB_DILS = (1, 3, 5)


def resblock_def(x, ws, mode, dtype, y_old=None):
    """Three pairs, dilations 1, 3, 5; ws[m] = (w1, b1, w2, b2); y_old: the MRF sum the last pair adds to."""
    xr = np.asarray(x, dtype)
    for m, dil in enumerate(RB_DILS):
        xr, _ = pair_def(xr, *ws[m], dil, mode, dtype, y_old if m == 2 else None)
    return xr


def convT_operand(x, pre_div, mode, dtype):
    """leaky(x / pre_div) as the upsamplers stage it.  In the 16-bit modes the value that is rounded is the fp32 one (division, then slope, each rounded
    to fp32: convT_xl16_kernel), so it is formed in float32 whatever dtype."""
    if mode:
        return round16(leaky(np.asarray(x, F32) / F32(pre_div), F32), mode).astype(dtype)
    return leaky(np.asarray(x, dtype) / dtype(pre_div), dtype)


_TAPS_T = {}


def _convT_taps(w, mode, dtype):
    """round16(w) as contiguous per-tap matrices [K][Cout][Cin], kept per weight array (the rounding and the transposition are most of a small case's time)."""
    key = (id(w), mode, np.dtype(dtype).name)
    hit = _TAPS_T.get(key)
    if hit is None or hit[0] is not w:
        hit = _TAPS_T[key] = (w, np.ascontiguousarray(round16(np.asarray(w, dtype), mode).transpose(2, 1, 0)))
    return hit[1]


def convT_def(x, w, b, s, pre_div, mode, dtype, stacked=False):
    """ConvTranspose1d(kernel 2 s, stride s, padding s / 2) of leaky(x / pre_div): x [Cin][Ti], w [Cin][Cout][2 s] -> [Cout][Ti s].
    stacked: the same sum through stack_two_tap's array, as the kernels walk it."""
    ci, co, K = w.shape
    assert K == 2 * s
    Ti = x.shape[1]
    a = convT_operand(x, pre_div, mode, dtype)
    p = s // 2
    if stacked:      # y[co][s m + r - s/2] = sum_q W2[q][.][r Cout + co] . a[.][m - q], m = 0 .. Ti
        w2 = round16(stack_two_tap(w, s).astype(dtype), mode)
        ap = np.zeros((ci, Ti + 2), dtype)
        ap[:, 1:Ti + 1] = a                                        # column m + 1 <-> a[m]
        full = np.zeros((co, (Ti + 1) * s), dtype)                 # sample s m + r
        for q in range(2):
            z = np.ascontiguousarray(w2[q].T) @ np.ascontiguousarray(ap[:, 1 - q:Ti + 2 - q])      # [s Cout][Ti + 1]: a[m - q]
            full += z.reshape(s, co, Ti + 1).transpose(1, 2, 0).reshape(co, (Ti + 1) * s)
        y = full[:, p:p + Ti * s]
    else:
        full = np.zeros((co, (Ti - 1) * s + K), dtype)
        wt = _convT_taps(w, mode, dtype)
        for j in range(K):
            full[:, j:j + (Ti - 1) * s + 1:s] += wt[j] @ a
        y = full[:, p:p + Ti * s]
    return y + np.asarray(b, dtype)[:, None]


def convT_lolo(x, w, s, pre_div):
    """fp16x3 upsampler: the omitted lo x lo products, 2^-21 (|w| convT |leaky(x / pre_div)|)."""
    a = np.abs(convT_operand(x, pre_div, 0, F64))
    hit = _TAPS_T.get((id(w), "abs"))
    if hit is None or hit[0] is not w:
        hit = _TAPS_T[(id(w), "abs")] = (w, np.abs(np.asarray(w, F64)))
    return 2.0 ** -21 * convT_def(a, hit[1], np.zeros(w.shape[1]), s, 1.0, 0, F64)


def stack_two_tap(w, s):
    """ConvTranspose1d weights [Cin][Cout][2 s] -> the two-tap conv [2][Cin][s Cout] with row = phase Cout + co that pack_conv_transpose builds
    (cm-tts_amd/csrc/import.hip:65-72): element (q, ci, r Cout + co) = w[ci][co][r + s q].  k-major: the packers take it as it is."""
    ci, co, K = w.shape
    assert K == 2 * s
    return np.ascontiguousarray(w.reshape(ci, co, 2, s).transpose(2, 0, 3, 1).reshape(2, ci, s * co), F32)


# ----------------------------------------------------------------------------------------------------------------- yardsticks

def dmax(ref64, val):
    return float(np.abs(np.asarray(val, F64) - ref64).max())


def floor4(ref64):
    """4 float32 ulps of the output's magnitude."""
    return 4.0 * float(np.spacing(F32(np.abs(ref64).max())))


def widen_term(xt64, w2, mode, d32_xt):
    """Fused 16-bit kernels round xt on chip: an element whose activated float64 value lies within M d32_xt of a rounding midpoint may round the
    other way there, which moves conv2's operand by one 16-bit ulp.  widen[o][t] = sum |w2q[o][c][tau]| near[c][t + tau - R] ulp16(leaky(xt64)[c][.])."""
    a = leaky(xt64, F64)
    u = ulp16(a, mode)
    r = np.abs(a) / u
    near = np.abs(r - np.floor(r) - 0.5) * u <= M * d32_xt
    return conv_same(near * u, np.abs(round16(np.asarray(w2, F64), mode)), 1, F64), int(near.sum())


def lolo_term(a, w, dil):
    """fp16x3 omits the lo x lo product of every (hi, lo) pair: 2^-21 (|w| conv |a|)."""
    return 2.0 ** -21 * conv_same(np.abs(np.asarray(a, F64)), np.abs(np.asarray(w, F64)), dil, F64)


# ----------------------------------------------------------------------------------------------------------------- inputs

@functools.lru_cache(maxsize=None)
def weights(Cout, Cin, k, seed):
    """(w [Cout][Cin][k] float32, torch's Conv1d layout, bias [Cout]); rows differ in their mean: a transpose is not a symmetry."""
    rs = np.random.RandomState(9000 + 131 * Cout + 17 * k + seed)
    w = (rs.standard_normal((Cout, Cin, k)) / np.sqrt(Cin * k)).astype(F32)
    w += (np.arange(Cout)[:, None, None] * 2e-5).astype(F32)
    b = (0.3 * rs.standard_normal(Cout)).astype(F32)
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


def pair_weights(Cc, k, m=0):
    """(w1, b1, w2, b2) of pair m of the (C, k) instance."""
    return weights(Cc, Cc, k, 2 * m) + weights(Cc, Cc, k, 2 * m + 1)


@functools.lru_cache(maxsize=None)
def convT_weights(ci, co, s):
    rs = np.random.RandomState(7000 + ci + s)
    w = (rs.standard_normal((ci, co, 2 * s)) / np.sqrt(2 * ci)).astype(F32)
    w += (np.arange(co)[None, :, None] * 2e-5).astype(F32)
    b = (0.3 * rs.standard_normal(co)).astype(F32)
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


@functools.lru_cache(maxsize=None)
def signal(Cc, T, seed=0):
    """[B][C][T] float32, N(0, 1)."""
    x = np.random.RandomState(500 + 7 * Cc + 13 * T + seed).standard_normal((B, Cc, T)).astype(F32)
    x.setflags(write=False)
    return x


def padded(v, ld, fill=GARBAGE):
    """[..][T] -> [..][ld] with `fill` behind the valid columns: what must never reach an output."""
    out = np.full(v.shape[:-1] + (ld,), fill, v.dtype)
    out[..., :v.shape[-1]] = v
    return out


# ----------------------------------------------------------------------------------------------------------------- shapes

# Output-tile width W of every kernel instance, beside the source line that sets it (cm-tts_amd/csrc/)
def tile_width(kernel, Cc, k, dil=1, mode=0):
    R2 = k - 1
    return {
        "conv_xl": 64,                                    # resblock_pair.hip:338  constexpr int XL_BN = 64;
        "conv_xlw": 64 if dil == 1 else 60,               # resblock_pair.hip:606  constexpr int BN = DIL == 1 ? 64 : 60;
        "conv16": 128,                                    # conv_mfma16.hip:326-329  launch16<.., 128, ..>: 128-frame tiles everywhere
        "conv_xl16": 128,                                 # conv_xl16.hip:170  BN = (C == 128 || XL16_BN256 == 128) ? 128 : 64;
        "conv_xl16x3": 64,                                # resblock_pair16x3.inc:449  launch_xl3<256, P3_KT, 64>
        "resblock_pair": (256 if Cc == 32 else 128) - R2,  # resblock_pair.hip:51,194  N1_OF(C) ((C) == 32 ? 256 : 128); TT = N1 - 2 * R2;
        "resblock_pair16": 256 - R2,                      # resblock_pair16.hip:36  TT = N1 - 2 * R2;  (conv_loop16.h:16 N1 = 256)
        "resblock_pairw16": 256 - R2,                     # resblock_pairw16.inc:37,51  N1 = C == 128 ? 256 : 128; TT = N1 - 2 * R2;
        "resblock16": 384 - 12 * R2,                      # resblock16.hip:63  NOUT = W - 2 * H;  H = 12 * R: 360 / 312 / 264
        "resblock_pair16x3": (128 if Cc == 32 else 96) - R2,      # resblock_pair16x3.inc:150,288  NOUT = N1 - 2 * R2; N1 = 128 (C = 32) / 96 (:428-430)
        "convT": 64,                                      # resblock_pair.hip:759  tiles of XL_BN input columns over Ti + 1
        "convT16": 32 if (mode == 3 and Cc == 512) else 64,      # convT_xl16.hip:103,244  BN = 64; 32 for the fp16x3 C_in = 512 stage
    }[kernel]


def reach_of(kernel, k, dil):
    return 12 * (k - 1) // 2 if kernel == "resblock16" else dil * (k - 1) // 2


def t_list(kernel, Cc, k, dil=1, mode=0):
    """T in {1, reach, W - 1, W, W + 1, 2 W + reach + 1}."""
    Wt, r = tile_width(kernel, Cc, k, dil, mode), reach_of(kernel, k, dil)
    return tuple(sorted({1, r, Wt - 1, Wt, Wt + 1, 2 * Wt + r + 1}))


def t_extra_lds(kernel, Cc, k, dil=1, mode=0):
    """The Ts of an instance that also run with rows of T + 3 elements, so that rows do not start where 16-byte lines do: W itself (every W is even, so
    T + 3 is ODD: fp32 rows start at all four 4-byte phases of a line, the rows of a 16-bit image on odd half-words) and the ragged neighbour of W whose
    T + 3 is no multiple of 4 (W + 1, or W - 1 where W is a multiple of 4)."""
    Wt = tile_width(kernel, Cc, k, dil, mode)
    return (Wt, Wt - 1 if Wt % 4 == 0 else Wt + 1)


def t_alone(kernel, Cc, k, dil=1, mode=0):
    """The Ts at which utterance 1 is also launched alone and the launch is repeated behind one on inputs 1e4 times larger: one column, and a ragged second tile."""
    return (1, tile_width(kernel, Cc, k, dil, mode) + 1)


def lds_of(T, extra):
    ld = (T + 3) // 4 * 4
    return (ld, T + 3) if extra else (ld,)


def ti_list(tile):
    return (1, 2, tile - 1, tile, tile + 1)


def ti_extra_lds(tile):
    """The upsamplers' Ti that also run with rows of Ti + 3 floats in and Ti s + 3 out: the tile (both odd) and the ragged tile - 1 (tile is a multiple of 4)."""
    return (tile, tile - 1)


CONVT_STAGES = ((512, 256, 8), (256, 128, 8), (128, 64, 2), (64, 32, 2))      # (C_in, C_out, stride) of the four upsamplers

# ----------------------------------------------------------------------------------------------------------------- references


@functools.lru_cache(maxsize=None)
def _conv_base(Cc, k, seed, dil, T, mode):
    """(conv + bias in float64, in float32) of signal(C, T): what every epilogue variant of the case starts from."""
    w, b = weights(Cc, Cc, k, seed)
    x = signal(Cc, T)
    return tuple(np.stack([conv_def(x[i], w, b, dil, mode, dt) for i in range(B)]) for dt in (F64, F32))


@functools.lru_cache(maxsize=None)
def _conv_eval(Cc, k, seed, dil, T, mode, res, accum):
    ref, v32 = _conv_base(Cc, k, seed, dil, T, mode)
    for on, sig in ((res, 1), (accum, 2)):      # ((conv + b) + res) + y_old, each sum in the evaluation's own dtype: conv_def's expression
        if on:
            ref, v32 = ref + signal(Cc, T, sig), v32 + signal(Cc, T, sig)
    ref.setflags(write=False)
    return ref, dmax(ref, v32)


def conv_reference(Cc, k, seed, dil, T, mode, res, accum, Tmax):
    """One conv on signal(C, T) (residual signal(.., 1), old y signal(.., 2)) -> (ref float64 [B][C][T], yardstick = d32 floored by the instance's d32
    at its largest T and by 4 ulps of the output)."""
    ref, d32 = _conv_eval(Cc, k, seed, dil, T, mode, res, accum)
    return ref, max(d32, _conv_eval(Cc, k, seed, dil, Tmax, mode, res, accum)[1], floor4(ref))


@functools.lru_cache(maxsize=None)
def _pair_core(Cc, k, m, dil, T, mode):
    return _pair_eval_on(signal(Cc, T), None, pair_weights(Cc, k, m), dil, mode)


@functools.lru_cache(maxsize=None)
def _pair_eval(Cc, k, m, dil, T, mode, accum):
    e = _pair_core(Cc, k, m, dil, T, mode)
    if not accum:
        return e
    e, y0 = dict(e), signal(Cc, T, 2)       # ((conv2 + b2) + x) + y_old: the last sum alone differs, in each evaluation's dtype
    e["ref"], e["v32"], e["nf32"] = e["ref"] + y0, e["v32"] + y0, e["nf32"] + y0
    e["d32"] = dmax(e["ref"], e["nf32"])
    return e


def _pair_eval_on(x, y0, ws, dil, mode):
    """-> dict(ref [B][C][T], xt64, d32, d32_xt, widen [B][C][T], flips32: xt elements the float32 evaluation rounds the other way, v32: that evaluation,
    nf32: the float32 evaluation d32 is taken from).
    d32 is the NO-FLIP deviation: in bf16 / fp16 the float32 evaluation's conv2 runs on the float64 evaluation's rounded operand (rounding absorbs xt's
    fp32 error unless it crosses a midpoint, and that crossing is what `widen` accounts for); fp32 and fp16x3: the plain float32 evaluation."""
    coarse = mode in (1, 2)
    out = {k_: [] for k_ in ("ref", "xt", "widen", "v32", "nf32")}
    d32_xt = 0.0
    flips = near = 0
    for i in range(x.shape[0]):
        yo = None if y0 is None else y0[i]
        ref, xt = pair_def(x[i], *ws, dil, mode, F64, yo)
        v32, xt32 = pair_def(x[i], *ws, dil, mode, F32, yo)
        d32_xt = max(d32_xt, dmax(xt, xt32))
        nf32 = v32
        if coarse:
            a2 = round16(leaky(xt, F64), mode)
            flips += int((round16(leaky(xt32, F32), mode) != a2).sum())
            nf32 = conv_def(a2.astype(F32), ws[2], ws[3], 1, mode, F32, res=x[i], y_old=yo, act=False)
        for k_, v in (("ref", ref), ("xt", xt), ("v32", v32), ("nf32", nf32)):
            out[k_].append(v)
    for i in range(x.shape[0]):
        if coarse:
            wd, n = widen_term(out["xt"][i], ws[2], mode, d32_xt)
            near += n
        elif mode == 3:      # conv2's own omitted products and conv1's carried through conv2 (LeakyReLU scales by at most 1)
            l1 = lolo_term(leaky(x[i], F64), ws[0], dil)
            wd = lolo_term(leaky(out["xt"][i], F64), ws[2], 1) + conv_same(l1, np.abs(ws[2]).astype(F64), 1, F64)
        else:
            wd = np.zeros_like(out["ref"][i])
        out["widen"].append(wd)
    res = {k_: np.stack(v) for k_, v in out.items()}
    res.update(d32=dmax(res["ref"], res["nf32"]), d32_xt=d32_xt, flips32=flips, near=near)
    return res


def pair_reference(Cc, k, m, dil, T, mode, accum, Tmax):
    """A pair on signal(C, T) -> (_pair_eval_on's dict, yardstick = its d32 floored by the instance's at Tmax and by 4 ulps of the output)."""
    e = _pair_eval(Cc, k, m, dil, T, mode, accum)
    return e, max(e["d32"], _pair_eval(Cc, k, m, dil, Tmax, mode, accum)["d32"], floor4(e["ref"]))


def pair_reference_on(x, y0, Cc, k, m, dil, mode, d32_floor):
    """The same for a given input [B][C][T] (resblock16's chained reference: pair m starts from the device output of pair m - 1)."""
    e = _pair_eval_on(x, y0, pair_weights(Cc, k, m), dil, mode)
    return e, max(e["d32"], d32_floor, floor4(e["ref"]))


@functools.lru_cache(maxsize=None)
def _convT_eval(stage, Ti, pre_div, mode):
    ci, co, s = CONVT_STAGES[stage]
    w, b = convT_weights(ci, co, s)
    x = signal(ci, Ti, 3) * F32(2.0)
    ref = np.stack([convT_def(x[i], w, b, s, pre_div, mode, F64) for i in range(B)])
    v32 = np.stack([convT_def(x[i], w, b, s, pre_div, mode, F32) for i in range(B)])
    ref.setflags(write=False)
    return x, ref, dmax(ref, v32)


def convT_reference(stage, Ti, pre_div, mode, Timax):
    x, ref, d32 = _convT_eval(stage, Ti, pre_div, mode)
    return x, ref, max(d32, _convT_eval(stage, Timax, pre_div, mode)[2], floor4(ref))
