"""Inputs, float64 definitions, float32 restatements, yardsticks and shape lists shared by tests/test_quad_kernel_cases_cpu.py and
tests/test_gpu_quad_kernels.py (not a test module): the three Winograd F(4,3) kernels that work on output QUADS, called ALONE through their launch
hooks (cm-tts_amd/csrc/resblock_pair.h) — conv_xlq_kernel (conv_xlq.hip, 27 instances), conv_xlq_pair3_kernel (conv_xlq_pair.hip, 6) and
conv_k5q_kernel (conv_k5q.hip, 3 x the row splits).  What tests/vocoder_kernel_cases.py already has is taken from there: weights, signal, padded,
conv_def, pair_def, dmax, floor4, M, SENTINEL, GARBAGE and the ctypes argument blocks.

Every reference is the float64 DEFINITION on the operands the kernel itself has.  The yardstick is the definition's own float32 error in two
evaluations — the direct sum and the restatement of the form's own F(4,3) products (oracle/winograd_ref.py) — each also at the instance's largest T,
floored by 4 ulps of the output: denoiser_kernel_cases.block_reference(f43=True)'s rule.  Nothing here is computed from a kernel."""
import functools

import numpy as np

from oracle import winograd_ref as W
import text_kernel_cases as TC
import vocoder_kernel_cases as VC
from vocoder_kernel_cases import (B, GARBAGE, M, SENTINEL, SLOPE, ConvXlArgs, PairArgs, conv_def, dmax, floor4, kmajor, lds_of,  # noqa: F401
                                  padded, pair_def, pair_weights, signal, weights)

F32, F64 = np.float32, np.float64

# ----------------------------------------------------------------------------------------------------------------- shapes

XLQ_C, XLQ_K, DILS = (64, 128, 256), (3, 7, 11), (1, 3, 5)
PAIR_C = (64, 128)
K5Q_INSTANCES = ((128, False), (256, False), (256, True))      # (C_in, LayerNorm prologue); 256 output rows
K5Q_SPLITS = (0, 1, 2, 4)                                       # row_split: the launcher's rule, then 1 / 2 / 4 workgroups per tile
LN_EPS = 1e-12


# Output-tile width W of every instance, beside the source line that sets it (cm-tts_amd/csrc/)
def tile_width(kernel, dil=1):
    return {
        "conv_xlq": 64 if dil == 1 else 60,              # conv_xlq.hip:56  constexpr int BN = DIL == 1 ? 64 : 60;
        "conv_xlq_pair": {1: 60, 3: 56, 5: 56}[dil],     # conv_xlq_pair.hip:109  BN = 4 * NQ2;  NQ2 = (4 DIL QPC - 2) / 4 = 15 / 14 / 14
        "conv_k5q": 64,                                  # conv_k5q.hip:40  constexpr int BN = 64;
    }[kernel]


def class_entries(dil):
    """conv_xlq at dilation 3 / 5: entries of a residue class per tile (conv_xlq.hip:57  QPC = BN / (4 * DIL) quads): 20 / 12."""
    return tile_width("conv_xlq", dil) // dil


def reach_of(kernel, k, dil=1):
    """How far the operation reaches to either side of an output: dil (k - 1) / 2; the pair: conv1's dil + conv2's 1."""
    return dil + 1 if kernel == "conv_xlq_pair" else dil * (k - 1) // 2


def t_list(kernel, k, dil=1):
    """{1, 2, 3, reach, W - 1, W, W + 1, 2 W + reach + 1}; W + 2: the residue of T mod 4 around W that those do not hit (W - 1 .. W + 2 are all four: a
    ragged quad of 1, 2 and 3 columns and a whole one behind a full tile); dilation 3 / 5: W + dil + 1, a second tile whose class 0 holds two entries
    and every other class one (W + 1 and W + 2 are the second tiles that hold some classes and not others)."""
    Wt, r = tile_width(kernel, dil), reach_of(kernel, k, dil)
    ts = {1, 2, 3, r, Wt - 1, Wt, Wt + 1, Wt + 2, 2 * Wt + r + 1}
    if dil > 1:
        ts.add(Wt + dil + 1)
    return tuple(sorted(ts))


def t_extra_lds(kernel, dil=1):
    """The Ts that also run with rows of T + 3 floats (vocoder_kernel_cases.t_extra_lds): W and its ragged neighbour whose T + 3 is no multiple of 4.
    At dilation 1 these rows are the only place the scalar epilogue runs on whole quads."""
    Wt = tile_width(kernel, dil)
    return (Wt, Wt - 1 if Wt % 4 == 0 else Wt + 1)


def t_alone(kernel, dil=1):
    return (1, tile_width(kernel, dil) + 1)


# ----------------------------------------------------------------------------------------------------------------- inputs

SPIKE, SPIKE_EVERY = 100.0, 64


@functools.lru_cache(maxsize=None)
def spiky(Cc, T):
    """[B][C][T] float32: N(0, 1) with one sample in 64 scaled by 100.  An F(4,3) input transform's rounding error scales with the largest sample of the
    six-sample window, not with the output: the regime in which a wrong association in the transform shows."""
    rs = np.random.RandomState(800 + 7 * Cc + 13 * T)
    x = rs.standard_normal((B, Cc, T)).astype(F32)
    hit = rs.randint(0, SPIKE_EVERY, x.shape) == 0
    x = np.where(hit, x * F32(SPIKE), x).astype(F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def k5q_input(cin, T):
    """[B][cin][T] float32, per-column mean 0.3 and std 1.5: a LayerNorm input of text_kernel_cases.xres_input's kind."""
    x = (np.random.RandomState(4700 + 3 * cin + 11 * T).standard_normal((B, cin, T)) * 1.5 + 0.3).astype(F32)
    x.setflags(write=False)
    return x


def k5q_weights(cin):
    """(w [256][cin][5], bias [256]); (gamma near 1, small beta) = text_kernel_cases.ln_params()."""
    return weights(256, cin, 5, 0)


# ----------------------------------------------------------------------------------------------------------------- definitions and restatements

def leaky(v, dtype):
    return VC.leaky(v, dtype)


_TAPS_U = {}


def taps_U(w):
    """f43_tap_weights(w) rounded to float32 once, as the packer rounds them; kept per weight array (the cases' weights are cached, read-only arrays)."""
    hit = _TAPS_U.get(id(w))
    if hit is None or hit[0] is not w:
        hit = _TAPS_U[id(w)] = (w, [u.astype(F32) for u in W.f43_tap_weights(w)])
    return hit[1]


def xlq_f43(x, w, b, dil, res=None, y_old=None):
    """conv_def through the F(4,3) form's own products, float32: ((conv1d_f43_taps_dil(leaky(x)) + b) + res) + y_old."""
    y = W.conv1d_f43_taps_dil(leaky(x, F32), w, dil, taps_U(w)) + b[:, None]
    if res is not None:
        y = y + res
    if y_old is not None:
        y = y + y_old
    return y


def k5q_def(x, w, b, ln, relu, dtype, f43=False, ln_cols=None):
    """Conv1d(cin -> 256, k = 5, padding 2) + bias [+ ReLU] of x [cin][T]; ln: on LayerNorm(256 channels, eps 1e-12) of every frame inside [0, T) — the
    conv pads the NORMALISED sequence with zeros.  f43: the conv through conv1d_f43_taps (k = 5: two tap groups, the sixth tap zero).
    ln_cols > T: the WRONG prologue that normalises that many columns of a zero-extended x (a padding column then enters the conv as beta)."""
    h = np.asarray(x, dtype)
    T = h.shape[1]
    wd = np.asarray(w, dtype)
    if ln:
        g, be = TC.ln_params()
        if ln_cols is not None:
            h = np.pad(h, ((0, 0), (0, ln_cols - T)))
        h = np.ascontiguousarray(TC.layer_norm_cols(h, g, be, dtype))
    y = (W.conv1d_f43_taps(h, wd) if f43 else W.conv1d_direct(h, wd, 1))[:, :T] + np.asarray(b, dtype)[:, None]
    return np.maximum(y, dtype(0)) if relu else y


# ----------------------------------------------------------------------------------------------------------------- references

@functools.lru_cache(maxsize=None)
def _xlq_f43_base(Cc, k, dil, T, kind):
    w, b = weights(Cc, Cc, k, 0)
    x = spiky(Cc, T) if kind == "spiky" else signal(Cc, T)
    return np.stack([xlq_f43(x[i], w, b, dil) for i in range(B)])


@functools.lru_cache(maxsize=None)
def _xlq_eval(Cc, k, dil, T, res, accum):
    """-> (ref float64 [B][C][T] — vocoder_kernel_cases' own, from its caches —, d32 of the direct float32 evaluation, d32 of the F(4,3) restatement)."""
    ref, d_dir = VC._conv_eval(Cc, k, 0, dil, T, 0, res, accum)
    v = _xlq_f43_base(Cc, k, dil, T, "plain")
    for on, sig in ((res, 1), (accum, 2)):
        if on:
            v = v + signal(Cc, T, sig)
    return ref, d_dir, dmax(ref, v)


def xlq_reference(Cc, k, dil, T, res, accum, Tmax):
    """One conv on signal(C, T) (residual signal(.., 1), old y signal(.., 2)) -> (ref float64, yard = the largest of the direct and the F(4,3) d32, of
    both at the instance's largest T, and of 4 ulps of the output)."""
    ref, d_dir, d_f43 = _xlq_eval(Cc, k, dil, T, res, accum)
    _, t_dir, t_f43 = _xlq_eval(Cc, k, dil, Tmax, res, accum)
    return ref, max(d_dir, d_f43, t_dir, t_f43, floor4(ref))


def xlq_own(Cc, k, dil, T):
    """The plain launch's float32 restatement of its own products."""
    return _xlq_f43_base(Cc, k, dil, T, "plain")


@functools.lru_cache(maxsize=None)
def xlq_spiky_reference(Cc, k, dil, T):
    """The plain conv on spiky(C, T) -> (x, ref float64, yard = the larger d32 of the two float32 evaluations of THIS case, floored by 4 ulps)."""
    w, b = weights(Cc, Cc, k, 0)
    x = spiky(Cc, T)
    ref = np.stack([conv_def(x[i], w, b, dil, 0, F64) for i in range(B)])
    v32 = np.stack([conv_def(x[i], w, b, dil, 0, F32) for i in range(B)])
    ref.setflags(write=False)
    return x, ref, max(dmax(ref, v32), dmax(ref, _xlq_f43_base(Cc, k, dil, T, "spiky")), floor4(ref))


@functools.lru_cache(maxsize=None)
def _pair_f43_eval(Cc, dil, T):
    ws = pair_weights(Cc, 3, 0)
    x = signal(Cc, T)
    return np.stack([W.pair_f43(x[i], *ws, dil, SLOPE)[0] for i in range(B)])


@functools.lru_cache(maxsize=None)
def _pair_eval(Cc, dil, T, accum):
    e = VC._pair_eval(Cc, 3, 0, dil, T, 0, accum)
    v = _pair_f43_eval(Cc, dil, T)
    if accum:
        v = v + signal(Cc, T, 2)
    return e["ref"], e["d32"], dmax(e["ref"], v)


def pair_reference(Cc, dil, T, accum, Tmax):
    """The k = 3 pair on signal(C, T) (old y signal(.., 2)) -> (pair_def in float64, yard = the larger of the float32 evaluation of the pair and of its
    F(4,3) restatement, of both at the largest T, and of 4 ulps).  fp32 rounds nothing on chip: no widening term."""
    ref, d_dir, d_f43 = _pair_eval(Cc, dil, T, accum)
    _, t_dir, t_f43 = _pair_eval(Cc, dil, Tmax, accum)
    return ref, max(d_dir, d_f43, t_dir, t_f43, floor4(ref))


@functools.lru_cache(maxsize=None)
def _k5q_eval(cin, ln, relu, T):
    w, b = k5q_weights(cin)
    x = k5q_input(cin, T)
    ref = np.stack([k5q_def(x[i], w, b, ln, relu, F64) for i in range(B)])
    v32 = np.stack([k5q_def(x[i], w, b, ln, relu, F32) for i in range(B)])
    own = np.stack([k5q_def(x[i], w, b, ln, relu, F32, f43=True) for i in range(B)])
    for a in (ref, own):
        a.setflags(write=False)
    return ref, own, dmax(ref, v32), dmax(ref, own)


def k5q_reference(cin, ln, relu, T, Tmax):
    """-> (ref float64 [B][256][T], the float32 restatement of the form's own products (LayerNorm in numpy's order), yard)."""
    ref, own, d_dir, d_f43 = _k5q_eval(cin, ln, relu, T)
    _, _, t_dir, t_f43 = _k5q_eval(cin, ln, relu, Tmax)
    return ref, own, max(d_dir, d_f43, t_dir, t_f43, floor4(ref))
