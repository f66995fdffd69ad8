"""Inputs, float64 definitions, yardsticks and argument-block mirrors shared by tests/test_persist_stack_cases_cpu.py and
tests/test_gpu_persist_stack.py (not a test module): the persistent denoiser stack (cm-tts_amd/csrc/denoiser_persist.hip, denoiser_persist_lp.hip,
persist_tail.h) called ALONE through its three launchers (persist_args.h).  The reference of the stack is denoiser_kernel_cases.block_def chained
over NL layers with the skip sum running — oracle.cmtts_oracle.denoiser_forward's residual loop —, the reference of the in-kernel tail is its
skip head followed by frame_kernel_cases.mel_post_def's post-scaling, both in float64; the same functions in float32 are the yardstick.  Nothing
here is computed from a kernel.  Computed once per case and left unchanged.

Every layer has its OWN weight set and its own rows of cp / dp / d: a kernel that reads layer l's weights, bias, bo, d or dp for another layer moves
the result.  cp, dp and d are held with NLA = NL + 1 layers (cp_bstride = NLA * 256 * T, vec_stride = NLA * 256), the last one garbage: a batch
stride taken as NL * 256 * T reads it."""
import ctypes as C
import functools

import numpy as np

from oracle import winograd_ref as W
import denoiser_kernel_cases as DC
import frame_kernel_cases as FK
import vocoder_kernel_cases as VC

F32, F64 = np.float32, np.float64
CH, MEL = DC.CH, DC.MEL
B = VC.B
M = VC.M
NL_MAX = 3
NLS = (1, 2, 3)                  # nothing published; published once; a middle layer
FN = 64                          # frames per workgroup
MAX_LAYERS, MAX_GROUPS, MAX_WG = 32, 8, 256
POSTROW_RENOISE, POSTROW_FINAL = FK.POSTROW_RENOISE, FK.POSTROW_FINAL
GARBAGE = DC.GARBAGE

# ----------------------------------------------------------------------------------------------------------------- argument blocks

_VP = C.c_void_p


class PostRow(C.Structure):
    """struct PostRow (cm-tts_amd/csrc/persist_args.h)."""
    _fields_ = [("c_out", C.c_float), ("c_skip", C.c_float), ("nstd", C.c_float), ("flags", C.c_uint)]


class PersistGroup(C.Structure):
    """struct PersistGroup (persist_args.h)."""
    _fields_ = [("x0", _VP), ("cp", _VP), ("dp", _VP), ("d", _VP), ("skip", _VP), ("halo", _VP), ("xold", _VP), ("noise", _VP), ("out", _VP),
                ("cp_bstride", C.c_long), ("B", C.c_int), ("T", C.c_int), ("tiles", C.c_int), ("pad_", C.c_int), ("p1", _VP), ("mel2ph", _VP),
                ("pidx", _VP), ("ldp", C.c_int), ("Lph", C.c_int), ("p1t", _VP), ("xst", _VP)]


class PersistArgs(C.Structure):
    """struct PersistArgs (persist_args.h): travels by value into the kernel, ~2.3 KB."""
    _fields_ = [("x0", _VP), ("cp", _VP), ("dp", _VP), ("d", _VP), ("skip", _VP), ("W3f", _VP * MAX_LAYERS), ("b3", _VP * MAX_LAYERS),
                ("Wof", _VP * MAX_LAYERS), ("bo", _VP * MAX_LAYERS), ("halo", _VP), ("tmo", _VP), ("cp_bstride", C.c_long), ("vec_stride", C.c_long),
                ("B", C.c_int), ("T", C.c_int), ("NL", C.c_int), ("tiles", C.c_int), ("tail", C.c_int), ("Wsf", _VP), ("bs", _VP), ("Wpf", _VP),
                ("bp", _VP), ("skip_div", C.c_float), ("n_mels", C.c_int), ("xold", _VP), ("noise", _VP), ("c_out", C.c_float), ("c_skip", C.c_float),
                ("nstd", C.c_float), ("out", _VP), ("post_rows", _VP), ("out_final", _VP), ("fact", C.c_int), ("p1", _VP), ("p2", _VP), ("mel2ph", _VP),
                ("pidx", _VP), ("ldp", C.c_int), ("Lph", C.c_int), ("ld2", C.c_int), ("p1t", _VP), ("p2t", _VP), ("wino", C.c_int), ("xst", _VP),
                ("halo_zeroed", C.c_int), ("dbg", _VP), ("n_groups", C.c_int), ("n_wg", C.c_int), ("grp", PersistGroup * MAX_GROUPS),
                ("desc", C.c_uint * MAX_WG)]


# what cmtts_internal_persist_args_layout reports, in its order (kernel_hooks.hip)
LAYOUT_ARGS_FIELDS = ("W3f", "halo", "cp_bstride", "tail", "skip_div", "post_rows", "fact", "p1t", "wino", "xst", "n_groups", "grp", "desc")
LAYOUT_GROUP_FIELDS = ("cp_bstride", "B", "p1", "ldp", "xst")


def mirror_layout():
    """The mirrors' sizes and offsets in the hook's order."""
    return ([C.sizeof(PostRow), C.sizeof(PersistGroup), C.sizeof(PersistArgs)] + [getattr(PersistArgs, f).offset for f in LAYOUT_ARGS_FIELDS]
            + [getattr(PersistGroup, f).offset for f in LAYOUT_GROUP_FIELDS])


def desc_word(group, b, tile, active):
    """One ragged tile descriptor (persist_args.h): group | utterance << 3 | tile << 13 | active tiles << 20."""
    assert 0 <= group < 8 and 0 <= b < 1024 and 0 <= tile < 128 and 0 <= active < 256
    return group | b << 3 | tile << 13 | active << 20


def chunks_expected(Bn, T, max_blocks):
    """The balanced utterance chunks of the uniform launchers -> the list of chunk sizes."""
    tiles = (T + FN - 1) // FN
    per = max_blocks // tiles
    n = (Bn + per - 1) // per
    bc = (Bn + n - 1) // n
    return [min(bc, Bn - b0) for b0 in range(0, Bn, bc)]


# ----------------------------------------------------------------------------------------------------------------- shapes

T_LIST = (1, 2, 3, 63, 64, 65, 127, 128, 129)
T_F43 = tuple(sorted(set(T_LIST) | {5, 6, 7, 66, 67}))      # every residue mod 4 at the start and behind a full tile
T_SHORT = (1, 65, 129)                                      # NL = 1 and 2
T_MAX = 129
INSTANCES = ("direct", "f43", "f23", "bf16", "fp16", "fp16x3")
WINO = {"direct": 0, "f23": 1, "f43": 3}                    # PersistArgs.wino of the fp32 instances
LP_MODE = {"bf16": 1, "fp16": 2, "fp16x3": 3}               # cmtts_launch_denoiser_persist_lp's mode


def t_list(inst, NL):
    return T_SHORT if NL < NL_MAX else T_F43 if inst == "f43" else T_LIST


def shapes(inst):
    """Every (NL, T) an instance runs at."""
    return [(NL, T) for NL in NLS for T in t_list(inst, NL)]


# ----------------------------------------------------------------------------------------------------------------- inputs

def _ro(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs if len(arrs) > 1 else arrs[0]


@functools.lru_cache(maxsize=None)
def layer_weights(l):
    """Layer l's own (W3, b3, Wo, bo), drawn like DC.block_weights."""
    rs = np.random.RandomState(5100 + l)
    g3, go = np.exp2(rs.uniform(-1, 1, 2 * CH)), np.exp2(rs.uniform(-1, 1, 2 * CH))
    W3 = (rs.standard_normal((2 * CH, CH, 3)) / np.sqrt(3 * CH) * g3[:, None, None]).astype(F32)
    Wo = (rs.standard_normal((2 * CH, CH)) / np.sqrt(CH) * go[:, None]).astype(F32)
    b3, bo = (0.3 * rs.standard_normal(2 * CH)).astype(F32), (0.3 * rs.standard_normal(2 * CH)).astype(F32)
    return _ro(W3, b3, Wo, bo)


def stack_weights(NL):
    return tuple(layer_weights(l) for l in range(NL))


@functools.lru_cache(maxsize=None)
def tail_weights():
    """skip_projection Ws [256][256], bs; output_projection Wp [80][256], bp — rows with their own gains."""
    rs = np.random.RandomState(5150)
    Ws = (rs.standard_normal((CH, CH)) / np.sqrt(CH) * np.exp2(rs.uniform(-1, 1, CH))[:, None]).astype(F32)
    Wp = (rs.standard_normal((MEL, CH)) / np.sqrt(CH) * np.exp2(rs.uniform(-1, 1, MEL))[:, None]).astype(F32)
    return _ro(Ws, (0.3 * rs.standard_normal(CH)).astype(F32), Wp, (0.3 * rs.standard_normal(MEL)).astype(F32))


@functools.lru_cache(maxsize=None)
def stack_inputs(T, Bn=B):
    """x0 [Bn][C][T], cp [Bn][3 C][T] ~ N(0, 1); dp, d [Bn][3 C] ~ 0.5 N(0, 1): three layers' worth, a stack of NL layers takes the first NL."""
    rs = np.random.RandomState(5200 + 1000 * Bn + T)
    x0, cp = rs.standard_normal((Bn, CH, T)).astype(F32), rs.standard_normal((Bn, NL_MAX * CH, T)).astype(F32)
    dp, d = (0.5 * rs.standard_normal((Bn, NL_MAX * CH))).astype(F32), (0.5 * rs.standard_normal((Bn, NL_MAX * CH))).astype(F32)
    return _ro(x0, cp, dp, d)


def alloc_layers(v, NL):
    """[Bn][>= NL C][..] -> [Bn][(NL + 1) C][..]: the stack's NL layers and one layer of garbage behind them."""
    g = np.full((v.shape[0], CH) + v.shape[2:], GARBAGE, F32)
    return np.ascontiguousarray(np.concatenate([v[:, :NL * CH], g], axis=1))


EXPAND_L, EXPAND_LDP, EXPAND_LD2 = DC.EXPAND_L, DC.EXPAND_LDP, DC.EXPAND_LD2


@functools.lru_cache(maxsize=None)
def fact_case(T, Bn=B):
    """The conditioner factors of a FACT launch, DC.expand_case's construction at the stack's row count: p1 [Bn][3 C][ldp], p2 [3 C][ld2], mel2ph
    [Bn][T] holding 0 (padding), 1, L and L + 5, pidx [Bn][T] holding -1, 0, ld2 - 1 and ld2 + 3."""
    rs = np.random.RandomState(5300 + 1000 * Bn + T)
    p1 = (rs.standard_normal((Bn, NL_MAX * CH, EXPAND_LDP)) * np.sqrt(0.5)).astype(F32)
    p2 = (np.random.RandomState(5300).standard_normal((NL_MAX * CH, EXPAND_LD2)) * np.sqrt(0.5)).astype(F32)      # the model's: one for every case (ragged groups share it)
    m2p, pix = rs.randint(0, EXPAND_L + 1, (Bn, T)).astype(np.int64), rs.randint(0, EXPAND_LD2, (Bn, T)).astype(np.int64)
    edge_m, edge_p = (0, 1, EXPAND_L, EXPAND_L + 5), (-1, 0, EXPAND_LD2 - 1, EXPAND_LD2 + 3)
    for b in range(Bn):
        for j in range(min(4, T)):
            m2p[b, (j + b) % T if T < 4 else j] = edge_m[(j + b) % 4]
            pix[b, (j + b) % T if T < 4 else j] = edge_p[(j + 2 * b + 1) % 4]
            if T >= 8:
                m2p[b, T - 1 - j] = edge_m[(j + b + 1) % 4]
                pix[b, T - 1 - j] = edge_p[(j + b) % 4]
        if T > FN:      # and at the tile seam, where the halo entries gather
            m2p[b, FN - 1], m2p[b, FN] = edge_m[b % 4], edge_m[(b + 3) % 4]
            pix[b, FN - 1], pix[b, FN] = edge_p[(b + 2) % 4], edge_p[(b + 3) % 4]
    return _ro(p1, p2, m2p, pix)


@functools.lru_cache(maxsize=None)
def fact_cp(T, Bn=B):
    """cp [Bn][3 C][T] float32 of fact_case: DC.expand_def per utterance (what cond_expand_kernel writes, bit for bit)."""
    p1, p2, m2p, pix = fact_case(T, Bn)
    return _ro(np.stack([DC.expand_def(p1[b], p2, m2p[b], pix[b], EXPAND_L, EXPAND_LD2) for b in range(Bn)]))


def fact_tables(T, Bn, NL):
    """(p1 [Bn][NL C][ldp] — persist_args.h: its batch stride is NL C ldp, there is no stride field —, p2 [(NL + 1) C][ld2] with a layer of garbage
    behind, p1t [Bn][NL][ldp][C], p2t [NL][ld2][C], mel2ph, pidx) as the launch takes them."""
    p1, p2, m2p, pix = fact_case(T, Bn)
    p1n = np.ascontiguousarray(p1[:, :NL * CH])
    p2n = np.ascontiguousarray(np.concatenate([p2[:NL * CH], np.full((CH, EXPAND_LD2), GARBAGE, F32)]))
    p1t = np.ascontiguousarray(p1n.reshape(Bn, NL, CH, EXPAND_LDP).transpose(0, 1, 3, 2))
    p2t = np.ascontiguousarray(p2[:NL * CH].reshape(NL, CH, EXPAND_LD2).transpose(0, 2, 1))
    return p1n, p2n, p1t, p2t, m2p, pix


@functools.lru_cache(maxsize=None)
def post_inputs(T, Bn=B):
    """xold, noise [Bn][T][80] ~ N(0, 1)."""
    rs = np.random.RandomState(5400 + 1000 * Bn + T)
    return _ro(rs.standard_normal((Bn, T, MEL)).astype(F32), rs.standard_normal((Bn, T, MEL)).astype(F32))


POST_SCALARS = (float(F32(0.7)), float(F32(0.4)), float(F32(1.3)))      # c_out, c_skip, nstd of the launch


def post_rows(Bn, variant):
    """[Bn][4] float64 (c_out, c_skip, nstd as float32 values, flags).  variant 0: utterance 0 re-noised with nstd = 0, utterance 1 FINAL and not
    re-noised (the noise pointer is there: the flag decides), a third one plain; variant 1: utterance 0 neither, utterance 1 re-noised AND final."""
    kinds = {0: [(0.9, 0.2, 0.0, POSTROW_RENOISE), (0.5, 0.6, 1.1, POSTROW_FINAL), (0.8, 0.3, 0.6, 0)],
             1: [(0.6, 0.5, 0.9, 0), (0.75, 0.35, 1.1, POSTROW_RENOISE | POSTROW_FINAL), (0.9, 0.2, 0.4, POSTROW_RENOISE)]}[variant]
    rows = np.asarray([[float(F32(v)) for v in kinds[b % 3][:3]] + [kinds[b % 3][3]] for b in range(Bn)], F64)
    return _ro(rows)


TAIL_VARIANTS = ("full", "bare", "rows0", "rows1")      # launch scalars with xold and noise; without either; the two row tables (xold and noise given)


def tail_post(variant, Bn):
    """-> (rows [Bn][4] as tail_def takes them, with_xold, with_noise, table: the launch passes post_rows)."""
    if variant in ("full", "bare"):
        on = variant == "full"
        rows = np.asarray([list(POST_SCALARS) + [POSTROW_RENOISE if on else 0]] * Bn, F64)
        return rows, on, on, False
    return post_rows(Bn, int(variant[-1])), True, True, True


# ----------------------------------------------------------------------------------------------------------------- definitions

def stack_def(x0, cp, dp, d, weights, mode, dtype, conv=None):
    """NL = len(weights) residual layers of one utterance, DC.block_def chained with skip_old the running sum: x0 [C][T], cp [>= NL C][T], dp, d
    [>= NL C] -> (skip sum [C][T], the last layer's x')."""
    x, skip = x0, None
    for l, (W3, b3, Wo, bo) in enumerate(weights):
        s = slice(l * CH, (l + 1) * CH)
        if mode and W3 is layer_weights(l)[0]:
            x, skip = _block16(l, x, cp[s], dp[s], d[s], skip, mode, dtype, conv)
        else:
            _, _, x, skip = DC.block_def(x, cp[s], dp[s], d[s], W3, b3, Wo, bo, skip, mode, dtype, conv)
    return skip, x


@functools.lru_cache(maxsize=None)
def _rounded_weights(l, mode):
    W3, _, Wo, _ = layer_weights(l)
    return _ro(VC.round16(W3, mode), VC.round16(Wo, mode))


def _block16(l, x, cp, dp, d, skip_old, mode, dtype, conv):
    """DC.block_def's lines for layer_weights(l) in a 16-bit mode, with the weights rounded once per (layer, mode) instead of in every call (rounding
    is most of a call's time; float32 weights round to values both dtypes hold exactly) -> x', skip: the same bits as DC.block_def (CPU test)."""
    _, b3, _, bo = layer_weights(l)
    w3r, wor = _rounded_weights(l, mode)
    u = DC.u_def(x, cp, dp, mode, dtype)
    w3 = np.asarray(w3r, dtype)
    y = (VC.conv_same(u, w3, 1, dtype) if conv is None else conv(u, w3)) + np.asarray(b3, dtype)[:, None]
    x_new, skip, _ = DC.proj_def(DC.stage_z(DC.gate_def(y, dtype), mode, dtype), x, d, wor, bo, skip_old, dtype, 0)
    return x_new, skip


def head_def(skip, NL, Ws, bs, Wp, bp, dtype, div=None):
    """The skip head (Denoiser.forward, model/modules.py:634-637): F = Wp relu(Ws (skip / float32(sqrt(NL))) + bs) + bp, skip [C][T] -> [80][T]."""
    s = np.asarray(skip, dtype) / dtype(F32(np.sqrt(NL)) if div is None else div)
    h = np.maximum(np.asarray(Ws, dtype) @ s + np.asarray(bs, dtype)[:, None], dtype(0))
    return (np.asarray(Wp, dtype) @ h + np.asarray(bp, dtype)[:, None]).astype(dtype)


def tail_def(skip, NL, Ws, bs, Wp, bp, xold, noise, rows, dtype, div=None):
    """The in-kernel tail of a batch: skip [Bn][C][T] -> head_def, then FK.mel_post_def's post-scaling with the per-utterance rows [Bn][4] (launch
    scalars: the same row for everyone; flags bit 0 decides the noise term) -> [Bn][T][80].  xold / noise None: the term is absent.  Where a row is
    FINAL the launch writes it to out_final; that is the caller's to check."""
    Fm = np.stack([head_def(skip[b], NL, Ws, bs, Wp, bp, dtype, div) for b in range(len(skip))])
    Bn, _, T = Fm.shape
    zero = np.zeros((Bn, T, MEL), F32)
    case = {"F": Fm, "x": zero if xold is None else xold, "noise": zero if noise is None else noise}
    return FK.mel_post_def(case, dtype, xold is not None, noise is not None, rows=np.asarray(rows, F64))


# ----------------------------------------------------------------------------------------------------------------- references

def _f43(u, w3):
    return W.conv1d_f43(u, w3)


def _f23(u, w3):
    return W.conv1d_winograd(u, w3)


_CONV32 = {"f43": _f43, "f23": _f23}


def case_inputs(T, Bn=B, fact=False, Tc=None):
    """(x0, cp, dp, d) of a case; fact: cp expanded from fact_case; Tc: the first Tc frames alone (a trimmed utterance's definition)."""
    x0, cp, dp, d = stack_inputs(T, Bn)
    if fact:
        cp = fact_cp(T, Bn)
    if Tc is not None:
        x0, cp = x0[:, :, :Tc], cp[:, :, :Tc]
    return x0, cp, dp, d


@functools.lru_cache(maxsize=None)
def _stack_eval(inst, NL, T, Bn=B, fact=False, Tc=None):
    """-> dict(ref float64 [Bn][C][T], s32 the float32 evaluation, d32, model: fp16x3's |rounded-operand float64 - plain float64|)."""
    x0, cp, dp, d = case_inputs(T, Bn, fact, Tc)
    mode = 3 if inst == "fp16x3" else 0
    ws = stack_weights(NL)
    ref = np.stack([stack_def(x0[b], cp[b], dp[b], d[b], ws, mode, F64)[0] for b in range(Bn)])
    s32 = np.stack([stack_def(x0[b], cp[b], dp[b], d[b], ws, mode, F32, conv=_CONV32.get(inst))[0] for b in range(Bn)])
    assert ref.dtype == F64 and s32.dtype == F32
    out = {"ref": ref, "s32": s32, "d32": VC.dmax(ref, s32), "model": 0.0}
    if mode:
        plain = np.stack([stack_def(x0[b], cp[b], dp[b], d[b], ws, 0, F64)[0] for b in range(Bn)])
        out["plain"], out["model"] = plain, VC.dmax(plain, ref)
    _ro(ref, s32)
    return out


@functools.lru_cache(maxsize=None)
def stack_reference(inst, NL, T, Bn=B, fact=False, Tc=None):
    """The skip sum of an instance ("direct", "f43", "f23", "fp16x3") -> (ref float64 [Bn][C][T or Tc], yard).  yard = max(d32 of the case, d32 of the
    instance at T_MAX, 4 ulps of the output); F(4,3) / F(2,3): the float32 evaluation's conv is the restatement in oracle.winograd_ref and yard is
    floored by the direct form's; fp16x3: the reference is float64 on operands rounded by VC.round16(., 3), d32 the float32 evaluation of the same,
    and yard is floored by the 22-bit operand model |rounded-operand float64 - plain float64|.  No rounding-flip widening."""
    e, top = _stack_eval(inst, NL, T, Bn, fact, Tc), _stack_eval(inst, NL, T_MAX, B, fact)
    yard = max(e["d32"], top["d32"], VC.floor4(e["ref"]), e["model"], top["model"])
    if inst in _CONV32:
        yard = max(yard, stack_reference("direct", NL, T, Bn, fact, Tc)[1])
    return e["ref"], yard


@functools.lru_cache(maxsize=None)
def _tail_eval(inst, NL, T, variant, Bn=B, fact=False, Tc=None):
    e = _stack_eval(inst, NL, T, Bn, fact, Tc)
    xold, noise = post_inputs(T, Bn)
    if Tc is not None:
        xold, noise = xold[:, :Tc], noise[:, :Tc]
    rows, wx, wn, _ = tail_post(variant, Bn)
    tw = tail_weights()
    ev = lambda s, dt: tail_def(s, NL, *tw, xold if wx else None, noise if wn else None, rows, dt)
    ref, o32 = ev(e["ref"], F64), ev(e["s32"], F32)
    assert ref.dtype == F64 and o32.dtype == F32
    return {"ref": _ro(ref), "d32": VC.dmax(ref, o32), "model": VC.dmax(ev(e["plain"], F64), ref) if "plain" in e else 0.0}


@functools.lru_cache(maxsize=None)
def tail_reference(inst, NL, T, variant, Bn=B, fact=False, Tc=None):
    """out [Bn][T][80] = tail_def o stack_def in float64 -> (ref, yard); yard from the float32 evaluation of the WHOLE composition, floored as
    stack_reference floors its own."""
    e, top = _tail_eval(inst, NL, T, variant, Bn, fact, Tc), _tail_eval(inst, NL, T_MAX, variant, B, fact)
    yard = max(e["d32"], top["d32"], VC.floor4(e["ref"]), e["model"], top["model"])
    if inst in _CONV32:
        yard = max(yard, tail_reference("direct", NL, T, variant, Bn, fact, Tc)[1])
    return e["ref"], yard


def tail_on_skip_reference(skip, NL, T, variant):
    """The tail alone on a GIVEN float32 skip sum [Bn][C][T] (the 16-bit instances: their skip sum is anchored bit for bit by the per-layer chain,
    and rounding flips over several layers make a bound on the composition meaningless) -> (ref float64 [Bn][T][80], yard)."""
    Bn = skip.shape[0]
    xold, noise = post_inputs(T, Bn)
    rows, wx, wn, _ = tail_post(variant, Bn)
    tw = tail_weights()
    ev = lambda dt: tail_def(skip, NL, *tw, xold if wx else None, noise if wn else None, rows, dt)
    ref = ev(F64)
    return ref, max(VC.dmax(ref, ev(F32)), VC.floor4(ref))
