"""Inputs, float64 definitions and argument-block mirrors shared by tests/test_text_kernel_cases_cpu.py and tests/test_gpu_text_kernels.py
(not a test module): the text side's kernels — attention.hip and conv_xres.hip — called alone, and the flip rate of the integer stages
behind them.  Every reference is the definition evaluated in float64; the same function evaluated in float32 is the yardstick `d32` the
kernels' errors are measured in.  Computed once per case and left unchanged."""
import ctypes as C
import functools
import math

import numpy as np
from scipy.special import erf

from oracle import winograd_ref as W
from resample_cases import GARBAGE

# ----------------------------------------------------------------------------------------------------------------- attention.hip


class AttnArgs(C.Structure):
    """struct AttnArgs (cm-tts_amd/csrc/attention.h)."""
    _fields_ = [("qkv", C.c_void_p), ("out", C.c_void_p), ("lens", C.c_void_p), ("bstride", C.c_long), ("obstride", C.c_long),
                ("B", C.c_int), ("H", C.c_int), ("dh", C.c_int), ("L", C.c_int), ("ld", C.c_int), ("scale", C.c_float)]


ATTN_B, ATTN_H, DH = 3, 2, 128
KEY_CHUNK = 64                                   # attention_long_kernel walks the keys in chunks of 64
ATTN_L_SHORT = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192)      # attention_kernel<1..6>; attention_qb_kernel<1..4> up to 128
ATTN_L_LONG = (193, 256, 257, 320, 700)          # attention_long_kernel: one and several 128-query blocks, whole and ragged key chunks
ATTN_L_EXTRA_LD = (33, 129, 257)                 # a second row stride (ld + 8) at these
ATTN_CASES = ("unit", "peaky", "first", "overflow", "flat")
SENTINEL = 12345.0                               # what `out` holds before a launch


def attn_lds(L):
    ld = (L + 3) // 4 * 4
    return (ld, ld + 8) if L in ATTN_L_EXTRA_LD else (ld,)


def attn_lens(L, zero_row=False):
    """[L, about 0.6 L — strictly inside a 32-key tile and, for the long kernel, strictly inside a 64-key chunk with at least one whole
    chunk beyond it — , 1]; zero_row: the last utterance has no valid key at all."""
    mid = max(int(0.6 * L), 1)
    if L > 192:
        c = min(mid // KEY_CHUNK, L // KEY_CHUNK - 2)                    # chunk c + 1 lies wholly inside [0, L)
        off = min(max(mid - c * KEY_CHUNK, 17), 47)
        mid = c * KEY_CHUNK + (33 if off == 32 else off)
        assert mid % 32 and (mid // KEY_CHUNK + 2) * KEY_CHUNK <= L
    elif mid % 32 == 0:
        mid += 1
    return np.asarray([L, mid, 0 if zero_row else 1], np.int64)


def _ramp(n, reverse):
    """0.2 -> 1 over n keys, steep towards the 1 end (0.2 + 0.8 x^4): the keys of the last chunk stand clear of the chunk before."""
    x = np.arange(n) / max(n - 1, 1)
    r = 0.2 + 0.8 * x ** 4
    return r[::-1] if reverse else r


@functools.lru_cache(maxsize=None)
def attn_input(L, ld, case, zero_row=False):
    """(qkv float32 [B][3 H dh][ld], lens int64 [B]) of one launch.

    Queries are N(0, 1) around a per-head mean mu of +-0.5 per channel, so that the mean query of a head, Qbar, is a direction every
    query shares (|mu|^2 = 32: scores against N(0, 1) keys stay ~ N(0, 1.25)).  What must never reach an output is made to dominate if
    it does: the padded key columns [len, L) hold +4 Qbar (their score, ~ 4 |Qbar|^2 / sqrt(dh), beats every valid key of the case) with
    V = +-100 there, and columns [L, ld) of every row hold +-GARBAGE.  All of it finite: the product's QKV launch writes those columns, and
    P = 0 times a non-finite V would be NaN by IEEE.
      unit      Q, K ~ N(0, 1): the regime of the synthetic checkpoints (largest score about 4)
      peaky     Q x 4, K = ramp (n + mu) with the ramp 0.2 -> 1 over the valid keys and the LAST valid key = 2.5 mu: score spread about 25,
                the largest key of most queries in the last valid chunk — the online softmax's alpha takes the earlier chunks down by e^-10 .. e^-20
      first     the same reversed: the maximum in the first chunk, alpha = 1 afterwards
      overflow  unit with Q x 25: scores beyond 89, where expf without the max subtraction is inf
      flat      K = 0: all scores equal, the output is the mean of V over len keys"""
    assert case in ATTN_CASES and ld % 4 == 0 and ld >= L
    rs = np.random.RandomState(1000 * L + ld + 17 * ATTN_CASES.index(case))
    lens = attn_lens(L, zero_row)
    C3 = 3 * ATTN_H * DH
    qkv = np.where(rs.random_sample((ATTN_B, C3, ld)) < 0.5, -GARBAGE, GARBAGE).astype(np.float32)
    for b in range(ATTN_B):
        n = int(min(lens[b], L))
        for h in range(ATTN_H):
            mu = np.where(rs.random_sample(DH) < 0.5, -0.5, 0.5)
            q = rs.standard_normal((DH, L)) + mu[:, None]
            k = rs.standard_normal((DH, L))
            v = rs.standard_normal((DH, L))
            if case in ("peaky", "first"):
                q = q * 4.0
                if n:
                    k[:, :n] = (k[:, :n] + mu[:, None]) * _ramp(n, case == "first")[None, :]
                    k[:, 0 if case == "first" else n - 1] = 2.5 * mu
            elif case == "overflow":
                q = q * 25.0
            elif case == "flat":
                k[:] = 0.0
            q = q.astype(np.float32)
            k[:, n:] = 4.0 * q.astype(np.float64).mean(1, keepdims=True)
            v[:, n:] = np.where(rs.random_sample((DH, L - n)) < 0.5, -100.0, 100.0)
            qkv[b, h * DH:(h + 1) * DH, :L] = q
            qkv[b, (ATTN_H + h) * DH:(ATTN_H + h + 1) * DH, :L] = k
            qkv[b, (2 * ATTN_H + h) * DH:(2 * ATTN_H + h + 1) * DH, :L] = v
    qkv.setflags(write=False)
    lens.setflags(write=False)
    return qkv, lens


def attn_scores(q, k, dtype=np.float64):
    """s[key][query] = (K^T Q) dh^-1/2 over ALL key columns given."""
    return (k.astype(dtype).T @ q.astype(dtype)) * dtype(1.0 / math.sqrt(q.shape[0]))


def attention_def(qkv, lens, L, dtype=np.float64, n_heads=ATTN_H):
    """The definition (model/blocks.py:266-312 -> F.multi_head_attention_forward, no biases) on the kernels' layout: qkv [B][3 H dh][>= L]
    channel-major -> out [B][H dh][L].  Per utterance and head, with len = min(lens[b], L): s = (K^T Q) dh^-1/2 over keys < len, a
    two-pass softmax over the keys, then V P.  Only KEYS are masked: queries len <= i < L are computed like any other.  lens[b] == 0: zeros."""
    Bn, C3 = qkv.shape[:2]
    dh = C3 // (3 * n_heads)
    out = np.zeros((Bn, n_heads * dh, L), dtype)
    for b in range(Bn):
        n = int(min(lens[b], L))
        if n == 0:
            continue
        for h in range(n_heads):
            q = qkv[b, h * dh:(h + 1) * dh, :L]
            k = qkv[b, (n_heads + h) * dh:(n_heads + h + 1) * dh, :n]
            v = qkv[b, (2 * n_heads + h) * dh:(2 * n_heads + h + 1) * dh, :n].astype(dtype)
            s = attn_scores(q, k, dtype)
            p = np.exp(s - s.max(0, keepdims=True))
            p = p / p.sum(0, keepdims=True, dtype=dtype)
            out[b, h * dh:(h + 1) * dh] = v @ p
    return out


@functools.lru_cache(maxsize=None)
def attn_reference(L, ld, case, zero_row=False):
    """(ref float64 [B][H dh][L], d32 = max |float32 evaluation - float64 evaluation|, floor = 4 float32 ulps of the largest |output|)."""
    qkv, lens = attn_input(L, ld, case, zero_row)
    ref = attention_def(qkv, lens, L, np.float64)
    d32 = float(np.abs(attention_def(qkv, lens, L, np.float32).astype(np.float64) - ref).max())
    floor = 4.0 * float(np.spacing(np.float32(np.abs(ref).max())))
    ref.setflags(write=False)
    return ref, d32, floor


# ----------------------------------------------------------------------------------------------------------------- conv_xres.hip

ACT_NONE, ACT_GELU_ERF = 0, 2
INT_MAX = 2 ** 31 - 1


class ConvOut(C.Structure):
    """struct ConvOut (cm-tts_amd/csrc/conv_args.h)."""
    _fields_ = [("Y", C.c_void_p), ("y_zs0", C.c_long), ("y_zs1", C.c_long), ("ldy", C.c_int), ("row_off", C.c_int), ("Tout", C.c_int),
                ("ostride", C.c_int), ("ooff_base", C.c_int), ("ooff_mul", C.c_int), ("bias", C.c_void_p), ("bvec", C.c_void_p),
                ("bvec_zs", C.c_long), ("res", C.c_void_p), ("r_zs0", C.c_long), ("r_zs1", C.c_long), ("ldr", C.c_int),
                ("lens", C.c_void_p), ("alpha", C.c_float), ("act", C.c_int), ("div", C.c_float), ("rmul", C.c_float), ("accum", C.c_int)]


class ConvArgs(C.Structure):
    """struct ConvArgs (cm-tts_amd/csrc/conv_args.h)."""
    _fields_ = [("A", C.c_void_p), ("X", C.c_void_p), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("taps", C.c_int), ("dil", C.c_int),
                ("pad", C.c_int), ("Tin", C.c_int), ("a_ld", C.c_int), ("a_cols", C.c_int), ("a_tap_stride", C.c_long), ("ldx", C.c_int),
                ("zdiv", C.c_int), ("a_zs0", C.c_long), ("a_zs1", C.c_long), ("x_zs0", C.c_long), ("x_zs1", C.c_long),
                ("pre_div", C.c_float), ("pre_slope", C.c_float), ("split", C.c_int), ("out", ConvOut * 2),
                ("x16", C.c_int), ("y16", C.c_int), ("y16_slope", C.c_float), ("small_tiles", C.c_int), ("wfrag_iter", C.c_void_p),
                ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("ln_eps", C.c_float), ("xres_nt", C.c_int), ("ln_lens", C.c_void_p),
                ("ln_skip_tiles", C.c_int), ("w2frag", C.c_void_p), ("part", C.c_void_p), ("part_zs0", C.c_long), ("part_zs1", C.c_long),
                ("part_ld", C.c_int), ("M2", C.c_int), ("text_epi", C.c_int)]


def conv_args(X, Tin, ldx, x_bs, Y, ldy, y_bs, N, M, K, taps, bias):
    """cmtts_api.hip: conv_args() — the argument block every text-side launch starts from (pointers as integers or None)."""
    a = ConvArgs()
    a.X, a.M, a.N, a.K, a.taps, a.dil, a.pad = X, M, N, K, taps, 1, (taps - 1) // 2
    a.Tin, a.a_ld, a.a_cols, a.a_tap_stride, a.ldx = Tin, M, M, K * M, ldx
    a.zdiv, a.x_zs0, a.pre_div, a.pre_slope, a.split = 1, x_bs, 1.0, 1.0, INT_MAX
    for o in a.out:
        o.Y, o.y_zs0, o.ldy, o.Tout, o.ostride, o.bias, o.alpha, o.act, o.div = Y, y_bs, ldy, N, 1, bias, 1.0, ACT_NONE, 1.0
    return a


XRES_B, XRES_K = 2, 256
XRES_N = (1, 31, 33, 95, 97, 130)                # ragged around the 32- and 96-column tiles, ragged pairs and quads
XRES_N_EXTRA_LD = 97                             # one case with rows 8 floats longer: rows do not start where tiles do
LN_EPS = 1e-12
FFN_ALPHA = float(np.float32(9 ** -0.5))          # model/blocks.py:539-546: w_1(x) * kernel_size^-0.5, as the float the launch is given


def xres_lds(N):
    ld = (N + 3) // 4 * 4
    return (ld, ld + 8) if N == XRES_N_EXTRA_LD else (ld,)


def xres_lens(N):
    return np.asarray([N, max(int(0.6 * N), 1)], np.int64)


@functools.lru_cache(maxsize=None)
def xres_weights(M, taps, seed):
    """(w [M][K][taps] float32 in torch's layout, bias [M]); rows differ in their mean: a transpose is not a symmetry."""
    rs = np.random.RandomState(seed)
    w = (rs.standard_normal((M, XRES_K, taps)) / np.sqrt(XRES_K * taps)).astype(np.float32)
    w += (np.arange(M)[:, None, None] * 2e-5).astype(np.float32)
    b = rs.standard_normal(M).astype(np.float32)
    w.setflags(write=False)
    b.setflags(write=False)
    return w, b


@functools.lru_cache(maxsize=None)
def ffn2_weights():
    rs = np.random.RandomState(77)
    w2 = (rs.standard_normal((256, 1024)) / 32.0).astype(np.float32)
    w2.setflags(write=False)
    return w2


@functools.lru_cache(maxsize=None)
def ln_params():
    rs = np.random.RandomState(78)
    g = (1.0 + 0.1 * rs.standard_normal(XRES_K)).astype(np.float32)
    be = (0.1 * rs.standard_normal(XRES_K)).astype(np.float32)
    g.setflags(write=False)
    be.setflags(write=False)
    return g, be


@functools.lru_cache(maxsize=None)
def xres_input(N, ld):
    """x float32 [B][256][ld]: per-column mean 0.3, std 1.5 (LayerNorm input as in test_conv_k5q_kernel_vs_oracle); GARBAGE beyond N."""
    rs = np.random.RandomState(4000 + 10 * N + ld)
    x = (rs.standard_normal((XRES_B, XRES_K, ld)) * 1.5 + 0.3).astype(np.float32)
    x[:, :, N:] = GARBAGE
    x.setflags(write=False)
    return x


def kmajor(w):
    """torch [M][K][taps] -> the packers' k-major [taps][K][M]."""
    return np.ascontiguousarray(np.transpose(w, (2, 1, 0)), np.float32)


def layer_norm_cols(x, g, be, dtype, lens_n=None):
    """LayerNorm over the rows of x [K][N] (model/blocks.py:88-107), columns >= lens_n zero (layernorm_ct_kernel's mask)."""
    x = x.astype(dtype)
    mu = x.mean(0, dtype=dtype)
    var = ((x - mu) ** 2).mean(0, dtype=dtype)
    h = (x - mu) / np.sqrt(var + dtype(LN_EPS)) * g.astype(dtype)[:, None] + be.astype(dtype)[:, None]
    if lens_n is not None:
        h[:, int(lens_n):] = 0
    return h.astype(dtype)


def gelu(x):
    return x * x.dtype.type(0.5) * (x.dtype.type(1.0) + erf(x * x.dtype.type(math.sqrt(0.5))))


CONV_FORMS = {"direct": lambda h, w: W.conv1d_direct(h, w, 1), "f23": lambda h, w: W.conv1d_winograd(h, w, 1), "f43": W.conv1d_f43_taps}


def qkv_def(x, N, dtype, lens_n=None):
    """In-projection of one utterance: W LayerNorm(x) + b -> [768][N]."""
    w, b = xres_weights(768, 1, 11)
    g, be = ln_params()
    h = layer_norm_cols(x[:, :N], g, be, dtype, lens_n)
    return W.conv1d_direct(h, w.astype(dtype), 1) + b.astype(dtype)[:, None]


OUT_ALPHA = 0.75


def outproj_def(x, res, N, dtype, lens_n):
    """Out-projection of one utterance with the block's epilogue: ((W x + b) alpha + res), columns >= lens_n zero -> [256][N]."""
    w, b = xres_weights(256, 1, 12)
    y = (W.conv1d_direct(x[:, :N].astype(dtype), w.astype(dtype), 1) + b.astype(dtype)[:, None]) * dtype(OUT_ALPHA) + res[:, :N].astype(dtype)
    y[:, int(lens_n):] = 0
    return y


def ffn_def(x, N, dtype, form="direct", lens_n=None):
    """The fused FFN launch of one utterance: W2 gelu((conv_k9(LayerNorm(x)) + b) k^-1/2) -> [256][N]; form: the conv as the plain sum
    ("direct") or as the restatement of a Winograd form's own products ("f23": F(2,3) pairs, "f43": F(4,3) quads; oracle/winograd_ref.py)."""
    w, b = xres_weights(1024, 9, 13)
    g, be = ln_params()
    h = layer_norm_cols(x[:, :N], g, be, dtype, lens_n)
    wd = w.astype(dtype)
    c = CONV_FORMS[form](np.ascontiguousarray(h), wd)
    a = gelu(((c + b.astype(dtype)[:, None]) * dtype(FFN_ALPHA)).astype(dtype))
    return ffn2_weights().astype(dtype) @ a


def yardstick(ref64, val32):
    return float(np.abs(val32.astype(np.float64) - ref64).max())


# ----------------------------------------------------------------------------------------------------------------- flip rates

FLIP_B, FLIP_L, FLIP_T = 8, 64, 512              # 4096 frames
FLIP_VARIANTS = ("LJSpeech", "LibriTTS")
VA = "duration_pitch_energy_net.variance_adaptor."


@functools.lru_cache(maxsize=None)
def flip_inputs(variant, B=FLIP_B, L=FLIP_L):
    """(cfg, sd, texts int64 [B][L], lens int64 [B], spk float32 [B][dim] or None): unsearched inputs."""
    from cmtts_amd.config import get_config
    from cmtts_amd.weights import synth_cmtts_state_dict
    cfg = get_config(variant)
    sd = synth_cmtts_state_dict(cfg, seed=31, dur_frames=6.0, dur_spread=0.04)
    rs = np.random.RandomState(7)
    texts = rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)
    spk = rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32) if cfg.multi_speaker else None
    lens = np.maximum((rs.uniform(0.5, 1.0, size=B) * L).astype(np.int64), 1)
    lens[0] = L
    texts[np.arange(L)[None, :] >= lens[:, None]] = 0
    return cfg, sd, texts, lens, spk


@functools.lru_cache(maxsize=None)
def flip_oracle(variant, prec, B=FLIP_B, L=FLIP_L, T=FLIP_T):
    """The oracle's text and frame side in "f32" or "f64" -> the values the flip accounting needs."""
    from oracle import cmtts_oracle as O
    cfg, sd, texts, lens, spk = flip_inputs(variant, B, L)
    with O.precision(prec):
        st = O.duration_pitch_speaker_net(sd, cfg, texts, lens, spk, max_mel_len=T)
    return {k: np.asarray(st[k]) for k in ("log_d", "d_rounded", "e_pred", "e_idx", "f0_denorm", "p_idx", "mel_len")}


def duration_units(log_d):
    """The value durations_from_log rounds, in frames (one bucket = 1; boundaries at the half integers)."""
    return np.exp(np.asarray(log_d, np.float64)) - 1.0


def energy_units(e_pred, bins):
    """The energy predictor's output on a scale where bucket edge i sits at the integer i (piecewise linear between the edges of
    energy_bins, the end buckets continued with their neighbours' widths): bucketize is ceil() of it and one bucket = 1."""
    v, bins = np.asarray(e_pred, np.float64), np.asarray(bins, np.float64)
    n = len(bins)
    u = np.interp(v, bins, np.arange(n, dtype=np.float64))
    u = np.where(v < bins[0], (v - bins[0]) / (bins[1] - bins[0]), u)
    return np.where(v > bins[-1], n - 1 + (v - bins[-1]) / (bins[-1] - bins[-2]), u)


def pitch_units(f0_denorm):
    """The value f0_to_coarse rounds (utils/pitch_tools.py:26-35), restated in float64 exactly as conftest.pitch_margin_mask restates it:
    one bucket = 1, boundaries at the half integers."""
    f0 = np.asarray(f0_denorm).astype(np.float64)
    mel = 1127 * np.log(1 + f0 / 700)
    lo, hi = 1127 * np.log(1 + 50.0 / 700), 1127 * np.log(1 + 1100.0 / 700)
    sc = np.where(mel > 0, (mel - lo) * 254 / (hi - lo) + 1, mel)
    return np.clip(sc, 1, 255)


def half_margin(u):
    """Distance of u from the nearest half integer (durations, pitch)."""
    f = u + 0.5 - np.floor(u + 0.5)
    return np.minimum(f, 1 - f)


def int_margin(u):
    """Distance of u from the nearest integer (energy_units)."""
    return np.abs(u - np.rint(u))


def flip_masks(variant, d_rounded, e_idx, B=FLIP_B, L=FLIP_L, T=FLIP_T):
    """(valid phonemes [B][L], valid frames [B][T]).  Pitch frames count only in utterances whose durations AND energy buckets agree with the
    float64 oracle's: both are upstream of the pitch predictor (a duration moves every later frame, an energy bucket replaces an embedding
    row of its input), so a frame behind one of them compares two different inputs, not two roundings."""
    _, _, _, lens, _ = flip_inputs(variant, B, L)
    ref = flip_oracle(variant, "f64", B, L, T)
    ph = np.arange(L)[None, :] < lens[:, None]
    agree = (((np.asarray(d_rounded) == ref["d_rounded"]) & (np.asarray(e_idx) == ref["e_idx"])) | ~ph).all(1)
    fr = (np.arange(T)[None, :] < np.minimum(ref["mel_len"], T)[:, None]) & agree[:, None]
    return ph, fr


def flip_stats(variant, got, B=FLIP_B, L=FLIP_L, T=FLIP_T):
    """got: dict(log_d, d_rounded, e_pred, e_idx, f0_denorm, p_idx) of one arm (or of the float32 oracle) -> per stage
    {"n": observed disagreements with float64, "of": elements, "rate": expected flip rate = mean |pre-rounding value - float64's| in buckets,
     "max_err": the largest such error, "max_step": the largest disagreement, "off_margin": the largest boundary margin (of the float64
     value) among the disagreeing elements, 0 if none, "margins": every valid element's boundary margin}."""
    _, sd, _, _, _ = flip_inputs(variant, B, L)
    ref = flip_oracle(variant, "f64", B, L, T)
    ph, fr = flip_masks(variant, got["d_rounded"], got["e_idx"], B, L, T)
    bins = sd[VA + "energy_bins"]
    stages = {
        "dur": (duration_units(got["log_d"]), duration_units(ref["log_d"]), got["d_rounded"], ref["d_rounded"], ph, half_margin),
        "energy": (energy_units(got["e_pred"], bins), energy_units(ref["e_pred"], bins), got["e_idx"], ref["e_idx"], ph, int_margin),
        "pitch": (pitch_units(got["f0_denorm"]), pitch_units(ref["f0_denorm"]), got["p_idx"], ref["p_idx"], fr, half_margin),
    }
    out = {}
    for name, (u, u64, idx, idx64, valid, margin) in stages.items():
        err = np.abs(u - u64)[valid]
        step = np.abs(np.asarray(idx, np.float64) - np.asarray(idx64, np.float64))
        diff = (step != 0) & valid
        out[name] = {"n": int(diff.sum()), "of": int(valid.sum()), "rate": float(err.mean()) if err.size else 0.0,
                     "max_err": float(err.max()) if err.size else 0.0, "max_step": float(step[valid].max()) if err.size else 0.0,
                     "off_margin": float(margin(u64)[diff].max()) if diff.any() else 0.0,
                     "margins": margin(u64)[valid]}
    return out
