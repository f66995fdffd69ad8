"""Inputs, float64 definitions, yardsticks and argument-block mirrors shared by tests/test_denoiser_kernel_cases_cpu.py and
tests/test_gpu_denoiser_kernels.py (not a test module): the consistency denoiser's kernels called ALONE through their launch hooks
(cm-tts_amd/csrc/resblock_args.h, cond_gemm.h, inproj.h).  Every reference is the definition — one residual layer of
oracle.cmtts_oracle.denoiser_forward, its input projection, its stacked conditioner projection — evaluated in float64, in the 16-bit modes on
operands rounded from their fp32 value; the same function evaluated in float32 is the yardstick `d32` the kernels' errors are measured in.
Nothing here is computed from a kernel.  Computed once per case and left unchanged.

The layer is a SLICE of a larger allocation, as in the product: cp is layer LAYER of a [B][NL * 256][T] tensor (cp_bstride = NL * 256 * T), dp and
d point LAYER * 256 floats into [B][NL * 256] vectors (vec_stride = NL * 256): a kernel that strides a batch by C * T or by C reads another layer."""
import ctypes as C
import functools

import numpy as np

from oracle import winograd_ref as W
from resample_cases import GARBAGE  # noqa: F401  (the GPU module's guard rows)
import vocoder_kernel_cases as VC

F32, F64 = np.float32, np.float64
CH = 256                 # residual channels = encoder hidden
MEL = 80                 # mel channels (K of the input projection)
NL, LAYER = 3, 1         # the allocation holds three layers; the launches get the middle one
B = VC.B
GATE_ABS = 3e-7          # gate.h: cmtts_gate's absolute error on outputs in (-1, 1)

# ----------------------------------------------------------------------------------------------------------------- argument blocks


class ResArgs(C.Structure):
    """struct ResArgs (cm-tts_amd/csrc/resblock_args.h)."""
    _fields_ = [("x_in", C.c_void_p), ("cp", C.c_void_p), ("dp", C.c_void_p), ("d", C.c_void_p), ("x_out", C.c_void_p), ("skip", C.c_void_p),
                ("W3f", C.c_void_p), ("b3", C.c_void_p), ("Wof", C.c_void_p), ("bo", C.c_void_p), ("cp_bstride", C.c_long), ("vec_stride", C.c_long),
                ("B", C.c_int), ("T", C.c_int), ("accum_skip", C.c_int), ("z", C.c_void_p), ("dbg", C.c_void_p), ("flag", C.c_void_p), ("u", C.c_void_p)]


class CondGemmArgs(C.Structure):
    """struct CondGemmArgs (cm-tts_amd/csrc/cond_gemm.h)."""
    _fields_ = [("X", C.c_void_p), ("Wf", C.c_void_p), ("bias", C.c_void_p), ("Y", C.c_void_p), ("B", C.c_int), ("T", C.c_int), ("M", C.c_int),
                ("K", C.c_int), ("force", C.c_int), ("flat", C.c_int), ("row_split", C.c_int)]


class InProjArgs(C.Structure):
    """struct InProjArgs (cm-tts_amd/csrc/inproj.h)."""
    _fields_ = [("x", C.c_void_p), ("scale_b", C.c_void_p), ("scale", C.c_float), ("wf", C.c_void_p), ("bias", C.c_void_p), ("h", C.c_void_p),
                ("B", C.c_int), ("T", C.c_int), ("M", C.c_int), ("C", C.c_int), ("zero", C.c_void_p), ("zero_f4", C.c_long)]


# ----------------------------------------------------------------------------------------------------------------- gate permutation

def gate_perm(n, Cc=CH):
    """cm-tts_amd/csrc/import.hip: perm[r] = original row of packed row r; packed 2 n-row group g = [n sigmoid rows g n .. | n tanh rows C + g n ..]."""
    r = np.arange(2 * Cc)
    return (r // n % 2) * Cc + r // (2 * n) * n + r % n


def permuted_kmajor(w3, n=16):
    """W3 [2 C][C][3] -> the packers' k-major [3][C][2 C] with rows in gate_perm(n) order (fragment_order / fragment16 / wino43_fragments take this)."""
    return VC.kmajor(np.asarray(w3)[gate_perm(n, w3.shape[0] // 2)])


# ----------------------------------------------------------------------------------------------------------------- definitions

def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v)) if v.dtype == F64 else (F32(1.0) / (F32(1.0) + np.exp(-v))).astype(F32)


def gate_def(y, dtype):
    """z = sigmoid(y[:C]) * tanh(y[C:]) (model/blocks.py:678-679)."""
    y = np.asarray(y, dtype)
    Cc = y.shape[0] // 2
    return (sigmoid(y[:Cc]) * np.tanh(y[Cc:])).astype(dtype)


def u_def(x, cp, dp, mode, dtype):
    """The conv operand u = cp + (x + dp).  16-bit modes: round16 of the FLOAT32 value formed in that order (the kernels' own operand), whatever dtype."""
    if mode:
        u32 = np.asarray(cp, F32) + (np.asarray(x, F32) + np.asarray(dp, F32)[:, None])
        return VC.round16(u32, mode).astype(dtype)
    return np.asarray(cp, dtype) + (np.asarray(x, dtype) + np.asarray(dp, dtype)[:, None])


def proj_def(z, x, d, Wo, bo, skip_old, dtype, mode=0):
    """The second half on a given (staged) z [C][T]: o = Wo z + bo; x_new = (o[:C] + (x + d)) / sqrt(2); skip = o[C:] (+ skip_old) -> x_new, skip, o."""
    Cc = x.shape[0]
    o = VC.round16(np.asarray(Wo, dtype), mode) @ np.asarray(z, dtype) + np.asarray(bo, dtype)[:, None]
    x_new = (o[:Cc] + (np.asarray(x, dtype) + np.asarray(d, dtype)[:, None])) / dtype(np.sqrt(2.0))
    skip = o[Cc:] if skip_old is None else o[Cc:] + np.asarray(skip_old, dtype)
    return x_new.astype(dtype), skip.astype(dtype), o


def stage_z(z, mode, dtype):
    """z as the projection's operand: rounded from its FLOAT32 value in the 16-bit modes."""
    return VC.round16(np.asarray(z, F32), mode).astype(dtype) if mode else np.asarray(z, dtype)


def block_def(x, cp, dp, d, W3, b3, Wo, bo, skip_old, mode, dtype, conv=None):
    """One residual layer (ResidualBlock.forward, model/blocks.py:667-686, as O.denoiser_forward spells it) of one utterance: x, cp [C][T]; dp, d [C];
    W3 [2 C][C][3]; Wo [2 C][C] -> y [2 C][T], z [C][T] (before any rounding), x_new, skip.  conv: another evaluation of the k = 3 conv (the F(4,3)
    restatement) in place of the direct one."""
    u = u_def(x, cp, dp, mode, dtype)
    w3 = VC.round16(np.asarray(W3, dtype), mode)
    y = (VC.conv_same(u, w3, 1, dtype) if conv is None else conv(u, w3)) + np.asarray(b3, dtype)[:, None]
    z = gate_def(y, dtype)
    x_new, skip, _ = proj_def(stage_z(z, mode, dtype), x, d, Wo, bo, skip_old, dtype, mode)
    return y, z, x_new, skip


def inproj_def(x_tm, scale, Wi, bi, dtype):
    """x_tm [T][80] time-major -> relu(W (s x)^T + b) [C][T]."""
    xs = dtype(scale) * np.asarray(x_tm, dtype)
    return np.maximum(np.asarray(Wi, dtype) @ xs.T + np.asarray(bi, dtype)[:, None], dtype(0))


def cond_def(X, Wc, bias, mode, dtype):
    """X [K][T], Wc [M][K] -> Wc X + bias, operands rounded in the 16-bit modes (1 bf16, 2 fp16, 3 hi + lo fp16)."""
    return VC.round16(np.asarray(Wc, dtype), mode) @ VC.round16(np.asarray(X, dtype), mode) + np.asarray(bias, dtype)[:, None]


def expand_def(p1, p2, mel2ph, pidx, L, ld2):
    """cp[r][t] = (ph > 0 ? p1[r][ph - 1] : 0) + p2[r][idx], ph = min(mel2ph[t], L), idx = clamp(pidx[t], 0, ld2 - 1); p1 [M][ldp], p2 [M][ld2] — float32."""
    ph = np.minimum(np.asarray(mel2ph, np.int64), L)
    ix = np.clip(np.asarray(pidx, np.int64), 0, ld2 - 1)
    first = np.where(ph[None, :] > 0, np.asarray(p1, F32)[:, np.maximum(ph, 1) - 1], F32(0))
    return (first + np.asarray(p2, F32)[:, ix]).astype(F32)


# ----------------------------------------------------------------------------------------------------------------- shapes

TILE = {"fused32": 32, "fused64": 64, "split": 32, "w43": 64, "lp": 64, "cond_gemm": 64, "inproj": 64}      # frames per workgroup (FN of each .hip)


def t_list(kernel):
    """{1, 2, 3, W - 1, W, W + 1, 2 W - 1, 2 W, 2 W + 1} from the kernel's tile width W and the conv's reach 1; w43 (frame quads): every residue mod 4
    at the start and behind a full tile."""
    Wt = TILE[kernel]
    ts = {1, 2, 3, Wt - 1, Wt, Wt + 1, 2 * Wt - 1, 2 * Wt, 2 * Wt + 1}
    if kernel == "w43":
        ts |= {5, 6, 7, Wt + 2, Wt + 3}
    return tuple(sorted(ts))


def t_alone(kernel):
    return (1, TILE[kernel] + 1)


def seam_columns(T, Wt):
    """Column 0, column T - 1 and the two columns at each tile seam."""
    cols = {0, T - 1}
    for s in range(Wt, T, Wt):
        cols |= {s - 1, s}
    return np.asarray(sorted(cols))


INPROJ_T = (1, 5, 63, 64, 65, 129)
COND_T = (1, 63, 64, 65, 129)
COND_M = (512, 1024, 5120)
EXPAND_T = (1, 63, 64, 65, 256, 257, 260)

# ----------------------------------------------------------------------------------------------------------------- inputs


def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs if len(arrs) > 1 else arrs[0]


@functools.lru_cache(maxsize=None)
def block_weights():
    """W3 [512][256][3] ~ N(0, 1 / 768) and Wo [512][256] ~ N(0, 1 / 256), each row times its own gain in [0.5, 2] (a row permutation error moves every
    row); b3, bo ~ 0.3 N(0, 1).  The gate stays unsaturated: |y| is a few units."""
    rs = np.random.RandomState(4100)
    g3, go = np.exp2(rs.uniform(-1, 1, 2 * CH)), np.exp2(rs.uniform(-1, 1, 2 * CH))
    W3 = (rs.standard_normal((2 * CH, CH, 3)) / np.sqrt(3 * CH) * g3[:, None, None]).astype(F32)
    Wo = (rs.standard_normal((2 * CH, CH)) / np.sqrt(CH) * go[:, None]).astype(F32)
    b3, bo = (0.3 * rs.standard_normal(2 * CH)).astype(F32), (0.3 * rs.standard_normal(2 * CH)).astype(F32)
    return _ro(W3, b3, Wo, bo)


@functools.lru_cache(maxsize=None)
def block_inputs(T):
    """x [B][C][T], cp_all [B][NL C][T] ~ N(0, 1); dp_all, d_all [B][NL C] ~ 0.5 N(0, 1); skip_old [B][C][T] ~ N(0, 1)."""
    rs = np.random.RandomState(4200 + T)
    x, cp_all = rs.standard_normal((B, CH, T)).astype(F32), rs.standard_normal((B, NL * CH, T)).astype(F32)
    dp_all, d_all = (0.5 * rs.standard_normal((B, NL * CH))).astype(F32), (0.5 * rs.standard_normal((B, NL * CH))).astype(F32)
    skip_old = rs.standard_normal((B, CH, T)).astype(F32)
    return _ro(x, cp_all, dp_all, d_all, skip_old)


def layer_slices(cp_all, dp_all, d_all):
    lo = LAYER * CH
    return cp_all[:, lo:lo + CH], dp_all[:, lo:lo + CH], d_all[:, lo:lo + CH]


@functools.lru_cache(maxsize=None)
def proj_z(T):
    """z drawn uniform in (-1, 1) for the projection launch alone."""
    return _ro(np.random.RandomState(4300 + T).uniform(-1, 1, (B, CH, T)).astype(F32))


# ----------------------------------------------------------------------------------------------------------------- references

def _f43(u, w3):
    return W.conv1d_f43(u, w3)


def widen_z(z64, Wo, mode, d32_z):
    """The 16-bit block rounds z on chip: a z whose float64 value lies within M d32_z + the gate's 3e-7 of a rounding midpoint may round the other way
    there, which moves the projection's operand by one 16-bit ulp -> (widen [2 C][T], elements near a midpoint).  VC.widen_term takes the operand
    through LeakyReLU first; on max(z, 0) and on max(-z, 0) that is the identity, a zero is never near a midpoint, and the two sets are disjoint."""
    w2 = np.asarray(Wo)[:, :, None]
    thr = d32_z + GATE_ABS / VC.M
    wp, n_p = VC.widen_term(np.maximum(z64, 0.0), w2, mode, thr)
    wn, n_n = VC.widen_term(np.maximum(-z64, 0.0), w2, mode, thr)
    return wp + wn, n_p + n_n


@functools.lru_cache(maxsize=None)
def _block_eval(T, mode, accum, f43=False):
    """-> dict(z, x, skip: float64 [B]..; d32_z, d32_x, d32_skip; o_rms).  The 16-bit d32 of x / skip is the NO-FLIP
    deviation: the float32 evaluation's projection runs on the float64 evaluation's rounded z (vocoder_kernel_cases._pair_eval_on's construction)."""
    W3, b3, Wo, bo = block_weights()
    x, cp_all, dp_all, d_all, skip_old = block_inputs(T)
    cp, dp, d = layer_slices(cp_all, dp_all, d_all)
    out = {k: [] for k in ("z", "x", "skip", "z32", "x32", "skip32", "o")}
    for i in range(B):
        so = skip_old[i] if accum else None
        _, z, xn, sk = block_def(x[i], cp[i], dp[i], d[i], W3, b3, Wo, bo, so, mode, F64)
        _, z32, xn32, sk32 = block_def(x[i], cp[i], dp[i], d[i], W3, b3, Wo, bo, so, mode, F32, conv=_f43 if f43 else None)
        if mode:
            xn32, sk32, _ = proj_def(stage_z(z, mode, F32), x[i], d[i], Wo, bo, so, F32, mode)
        o = proj_def(stage_z(z, mode, F64), x[i], d[i], Wo, bo, None, F64, mode)[2]
        for k, v in (("z", z), ("x", xn), ("skip", sk), ("z32", z32), ("x32", xn32), ("skip32", sk32), ("o", o)):
            out[k].append(v)
    e = {k: np.stack(v) for k, v in out.items()}
    res = {k: e[k] for k in ("z", "x", "skip")}
    for k in ("z", "x", "skip"):
        res["d32_" + k] = VC.dmax(e[k], e[k + "32"])
        res[k].setflags(write=False)
    res["o_rms"] = float(np.sqrt((e["o"] ** 2).mean()))
    return res


@functools.lru_cache(maxsize=None)
def block_reference(T, mode, accum, Tmax, f43=False):
    """One layer on block_inputs(T) -> (_block_eval's dict + widen_x, widen_skip [B][C][T] and `near` in the 16-bit modes, yardsticks {z, x, skip}:
    each output's d32 floored by the instance's at its largest T and by 4 ulps of the output).  The widening counts the z within M yard[z] + 3e-7 of
    a midpoint: what a kernel inside its own bound on z may round the other way.  f43: the float32 evaluation's conv is the F(4,3) restatement
    (oracle.winograd_ref.conv1d_f43) and the yardstick of z is additionally floored by the direct form's."""
    e, top = dict(_block_eval(T, mode, accum, f43)), _block_eval(Tmax, mode, accum, f43)
    yard = {k: max(e["d32_" + k], top["d32_" + k], VC.floor4(e[k])) for k in ("z", "x", "skip")}
    if f43:
        yard["z"] = max(yard["z"], block_reference(T, mode, accum, Tmax)[1]["z"])
    if mode:
        Wo = block_weights()[2]
        wd = [widen_z(e["z"][i], Wo, mode, yard["z"]) for i in range(B)]
        full = np.stack([w_ for w_, _ in wd])
        e["widen_x"], e["widen_skip"], e["near"] = full[:, :CH] / np.sqrt(2.0), full[:, CH:], sum(n for _, n in wd)
    return e, yard


@functools.lru_cache(maxsize=None)
def _proj_eval(T, accum):
    _, _, Wo, bo = block_weights()
    x, _, _, d_all, skip_old = block_inputs(T)
    d, z = d_all[:, LAYER * CH:(LAYER + 1) * CH], proj_z(T)
    r64 = [proj_def(z[i], x[i], d[i], Wo, bo, skip_old[i] if accum else None, F64)[:2] for i in range(B)]
    r32 = [proj_def(z[i], x[i], d[i], Wo, bo, skip_old[i] if accum else None, F32)[:2] for i in range(B)]
    res = {"x": np.stack([r[0] for r in r64]), "skip": np.stack([r[1] for r in r64])}
    res["d32_x"] = VC.dmax(res["x"], np.stack([r[0] for r in r32]))
    res["d32_skip"] = VC.dmax(res["skip"], np.stack([r[1] for r in r32]))
    return res


def proj_reference(T, accum, Tmax):
    e, top = _proj_eval(T, accum), _proj_eval(Tmax, accum)
    return e, {k: max(e["d32_" + k], top["d32_" + k], VC.floor4(e[k])) for k in ("x", "skip")}


# ----------------------------------------------------------------------------------------------------------------- the gate's grid

GATE_T = 33
GATE_POINTS = (0.0, 1e-6, 1e-3, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 44.0, 87.0, 89.0, 100.0, 1e4)


@functools.lru_cache(maxsize=None)
def gate_grid():
    """x [C][GATE_T] float32 for the gate launch: z[c][t] = cmtts_gate(g = x[c][t], f = x[(c + 128) % 256][t]).  Channels 0 .. 127 of column t hold g,
    channels 128 .. 255 hold f of the pairs (c, c + 128) AND — read the other way round by channels 128 .. 255 — g and f swapped.  Every ordered pair of
    the +-GATE_POINTS occurs; the rest is uniform in [-8, 8].  All finite."""
    pts = np.asarray(sorted({s * p for p in GATE_POINTS for s in (1.0, -1.0)}), F32)
    gg, ff = np.meshgrid(pts, pts, indexing="ij")
    n = gg.size
    slots = (CH // 2) * GATE_T
    assert n <= slots
    rs = np.random.RandomState(4400)
    g = np.concatenate([gg.ravel(), rs.uniform(-8, 8, slots - n).astype(F32)]).astype(F32)
    f = np.concatenate([ff.ravel(), rs.uniform(-8, 8, slots - n).astype(F32)]).astype(F32)
    x = np.concatenate([g.reshape(CH // 2, GATE_T), f.reshape(CH // 2, GATE_T)]).astype(F32)
    return _ro(x)


def gate_identity_weights():
    """W3 [2 C][C][3]: centre tap only; sigmoid row c reads channel c, tanh row c reads channel (c + 128) % 256; b3 = 0."""
    W3 = np.zeros((2 * CH, CH, 3), F32)
    c = np.arange(CH)
    W3[c, c, 1] = 1.0
    W3[CH + c, (c + CH // 2) % CH, 1] = 1.0
    return W3, np.zeros(2 * CH, F32)


# ----------------------------------------------------------------------------------------------------------------- the input side

@functools.lru_cache(maxsize=None)
def inproj_weights():
    rs = np.random.RandomState(4500)
    Wi = (rs.standard_normal((CH, MEL)) / np.sqrt(MEL) * np.exp2(rs.uniform(-1, 1, CH))[:, None]).astype(F32)
    return _ro(Wi, (0.3 * rs.standard_normal(CH)).astype(F32))


@functools.lru_cache(maxsize=None)
def inproj_input(T):
    return _ro(np.random.RandomState(4600 + T).standard_normal((B, T, MEL)).astype(F32))


INPROJ_SCALES = (float(F32(1.7)), float(F32(0.3)))


@functools.lru_cache(maxsize=None)
def inproj_reference(T, per_utt):
    """-> (ref float64 [B][C][T], yard).  per_utt: utterance b is scaled by INPROJ_SCALES[b], else all by INPROJ_SCALES[0]."""
    def ev(Tt):
        Wi, bi = inproj_weights()
        x = inproj_input(Tt)
        sc = [INPROJ_SCALES[b if per_utt else 0] for b in range(B)]
        r64 = np.stack([inproj_def(x[b], sc[b], Wi, bi, F64) for b in range(B)])
        r32 = np.stack([inproj_def(x[b], sc[b], Wi, bi, F32) for b in range(B)])
        return r64, VC.dmax(r64, r32)
    ref, d32 = ev(T)
    return ref, max(d32, ev(max(INPROJ_T))[1], VC.floor4(ref))


@functools.lru_cache(maxsize=None)
def cond_weights(Mr):
    rs = np.random.RandomState(4700 + Mr)
    Wc = (rs.standard_normal((Mr, CH)) / np.sqrt(CH) * np.exp2(rs.uniform(-1, 1, Mr))[:, None]).astype(F32)
    return _ro(Wc, (0.3 * rs.standard_normal(Mr)).astype(F32))


@functools.lru_cache(maxsize=None)
def cond_input(Bn, T):
    return _ro(np.random.RandomState(4800 + 7 * Bn + T).standard_normal((Bn, CH, T)).astype(F32))


@functools.lru_cache(maxsize=None)
def _cond_eval(Bn, Mr, T, mode):
    Wc, bc = cond_weights(Mr)
    X = cond_input(Bn, T)
    r64 = np.stack([cond_def(X[b], Wc, bc, mode, F64) for b in range(Bn)])
    r32 = np.stack([cond_def(X[b], Wc, bc, mode, F32) for b in range(Bn)])
    return r64, VC.dmax(r64, r32)


def cond_reference(Bn, Mr, T, mode):
    """-> (ref float64 [Bn][M][T], yard, widen or None: fp16x3's omitted lo x lo products, 2^-21 |W| |X|)."""
    ref, d32 = _cond_eval(Bn, Mr, T, mode)
    wd = None
    if mode == 3:
        Wc, _ = cond_weights(Mr)
        wd = np.stack([VC.lolo_term(cond_input(Bn, T)[b], Wc[:, :, None], 1) for b in range(Bn)])
    return ref, max(d32, _cond_eval(Bn, Mr, max(COND_T), mode)[1], VC.floor4(ref)), wd


EXPAND_L, EXPAND_LDP, EXPAND_LD2, EXPAND_M = 11, 12, 9, 128


@functools.lru_cache(maxsize=None)
def expand_case(T):
    """p1 [B][M][ldp], p2 [M][ld2], mel2ph [B][T] holding 0, 1, L and L + 5 among 0 .. L, pidx [B][T] holding -1, 0, ld2 - 1 and ld2 + 3."""
    rs = np.random.RandomState(4900 + T)
    p1, p2 = rs.standard_normal((B, EXPAND_M, EXPAND_LDP)).astype(F32), rs.standard_normal((EXPAND_M, EXPAND_LD2)).astype(F32)
    m2p, pix = rs.randint(0, EXPAND_L + 1, (B, T)).astype(np.int64), rs.randint(0, EXPAND_LD2, (B, T)).astype(np.int64)
    edge_m, edge_p = (0, 1, EXPAND_L, EXPAND_L + 5), (-1, 0, EXPAND_LD2 - 1, EXPAND_LD2 + 3)
    for b in range(B):      # the edge values at both ends of the row (T = 1: one of them per utterance)
        for j in range(min(4, T)):
            m2p[b, (j + b) % T if T < 4 else j] = edge_m[(j + b) % 4]
            pix[b, (j + b) % T if T < 4 else j] = edge_p[(j + 2 * b + 1) % 4]
            if T >= 8:
                m2p[b, T - 1 - j] = edge_m[(j + b + 1) % 4]
                pix[b, T - 1 - j] = edge_p[(j + b) % 4]
    return _ro(p1, p2, m2p, pix)
