"""Inputs, float64 definitions, comparison functions and ctypes mirrors shared by tests/test_frame_kernel_cases_cpu.py and
tests/test_gpu_frame_kernels.py (not a test module): the frame-side and small kernels of kernels.hip called ALONE through the launch hooks
of kernel_hooks.hip, and the generic conv kernel (conv_mfma.hip) through cmtts_launch_conv.

Every definition is a plain numpy function that takes a dtype: evaluated in float64 it is the reference, evaluated in float32 it is the
yardstick `d32` the kernel's error is measured in.  A float result passes if max |kernel - float64| <= M x max(d32, 4 ulps of the case's
largest reference magnitude); M = BOUNDS[kernel].  Every comparison the GPU test makes is a function check_*(got, case) here: it returns the
measured ratio (a float with .d = max |kernel - float64| and .d32) or raises AssertionError, so the CPU test can feed it wrong "results".

Inputs are made once per case with a fixed seed, cached and read-only.  Layout rules: [T, ld) of inputs holds finite +-GARBAGE, lengths are
[T, about 0.6 T and no multiple of 16, 1].

BOUNDS: M = twice the worst ratio measured on MI355X, rounded up (docs/HISTORY.md has the same table).  A ratio of a few is a reordered fp32
sum; above 10 it is a finding, not a bound to set — none was measured.  Worst max |kernel - float64| / max(d32, 4 ulps) and its case:
  layernorm_ct 0.64 (T = 1)                      ln_linear<1 | 10 | 11> 0.71 / 0.67 / 0.66 (T = 64 / 16 / 64)
  chan_linear O = 1 | 10 | 11 | 16: 0.81 / 0.92 / 0.62 / 0.69 (T = 17 / 1 / 17 / 65)
  energy head (EE 1 | 2) and energy_embed 0.41 (T = 65, ld = 76, control 1: the prediction; everything behind it is exact)
  pitch_index 2.83 (T = 257, O = 11, stat_ld 1, std_scale 1; r_ws and f0_denorm per utterance)
  pos_embed_add 0.12, pos_embed_add_lr 0.12, embed_tokens 0.12 (of the 4-ulp floor: one fused multiply-add against two roundings)
  dense_small<4> 2.01 (B = 1, K = 255, N = 1), dense_small<16> 0.77 (B = 9, K = 1024, N = 1); stats_mlp 0.56 (256 -> 130 -> 70 -> 2)
  softmax_cols 0.37 (L = 63, overflow)           reduce_partials 0.47 (of the floor; the float32 left-to-right sum bit for bit)
  conv_post and conv_post_v4 2.00 (T = 1023, C = 30, KW = 3; the same bits)
  mel_prep 0.12, mel_post 0.23, mel_post_rows 0.28, diff_embed 0.06
  conv1d_mfma_kernel by configuration: gated 128 x 128 1.58 (N = 129), split 128 x 128 1.06, 64 x 64 / 64-channel chunks 1.00 (zdiv = 8) and
  1.00 (short M), 64 x 64 / five taps per barrier 4.59 (N = 65, Tin < N, GELU), 64 x 64 plain 0.69, 64 x 256 0.56, 32 x 256 4.29 (N = 255, tanh),
  transposed-conv phases 0.38
Integer stages: every duration of every case equals float64's (no step observed, so the project's DUR_MARGIN stands: the pre-rounding value of
the durations kernels is not an output); largest pre-rounding error of the energy value 1.02e-4 buckets (T = 65, control table) and of the
pitch value 1.81e-4 buckets (T = 700): margins 4 x these, below the project's ENERGY_MARGIN 1.3e-3 and FLIP_MARGIN 2e-3."""
import ctypes as C
import functools
import math

import numpy as np

import text_kernel_cases as TC
from text_kernel_cases import conv_args, ConvArgs, SENTINEL, GARBAGE, yardstick  # noqa: F401  (one copy: text_kernel_cases')
from conftest import pitch_margin_mask

FINDING = 10          # a ratio above this is a finding (the ceiling every kernel is held to before and after its M is measured)
BOUNDS = {
    "layernorm_ct": 2, "ln_linear": 2, "chan_linear": 2, "energy_head": 1, "pitch_index": 6,
    "pos_embed_add": 1, "pos_embed_add_lr": 1, "embed_tokens": 1,
    "dense_small": 5, "stats_mlp": 2, "softmax_cols": 1, "reduce_partials": 1, "conv_post": 4,
    "mel_prep": 1, "mel_post": 1, "mel_post_rows": 1, "diff_embed": 1,
    "conv_generic": 10,
}
assert max(BOUNDS.values()) <= FINDING
ISENT = -7777          # what integer outputs hold before a launch
# boundary margins of this module in buckets: 4 x the largest pre-rounding error measured here against float64 (header)
FRAME_ENERGY_MARGIN = 4.1e-4
FRAME_PITCH_MARGIN = 7.3e-4


# the durations kernels do not output their pre-rounding value, so none was measured: the project's DUR_MARGIN (tests/test_gpu_text_kernels.py)
FRAME_DUR_MARGIN = 2.2e-4
# (tests/test_frame_kernel_cases_cpu.py asserts that none of the three exceeds the project's DUR_MARGIN, ENERGY_MARGIN, FLIP_MARGIN)


class Ratio(float):
    """The measured ratio of one comparison, with what it was made of."""
    def __new__(cls, r, d=0.0, d32=0.0):
        self = super().__new__(cls, r)
        self.d, self.d32 = d, d32
        return self


def worst(*rs):
    return max(rs, key=float)


def ratio_check(kernel, got, ref, d32, what=""):
    """max |got - ref| / max(d32, 4 float32 ulps of max |ref|) against BOUNDS[kernel]."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (kernel, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (kernel, what, "non-finite result")
    floor = 4.0 * float(np.spacing(np.float32(np.abs(ref).max() if ref.size else 0.0)))
    d = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    r = Ratio(d / max(d32, floor), d, d32)
    assert r <= BOUNDS[kernel], (kernel, what, f"|d| {d:.3e}, d32 {d32:.3e}, floor {floor:.3e}, ratio {float(r):.2f} > {BOUNDS[kernel]}")
    return r


def exact(kernel, got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (kernel, what, got.shape, want.shape)
    same = (got == want) | ((got != got) & (want != want))
    assert same.all(), (kernel, what, f"{int((~same).sum())} of {same.size} elements differ, first at {tuple(np.argwhere(~same)[0])}")
    return Ratio(0.0)


def same_bits(kernel, a, b, what=""):
    """Two results of kernels that promise the same bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (kernel, what)
    assert a.tobytes() == b.tobytes(), (kernel, what, "bits differ")
    return Ratio(0.0)


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _garbage(rs, shape):
    return np.where(rs.random_sample(shape) < 0.5, -GARBAGE, GARBAGE).astype(np.float32)


def ceil4(n):
    return (n + 3) // 4 * 4


def case_lens(T):
    """[T, about 0.6 T and no multiple of 16, 1]."""
    mid = max(int(0.6 * T), 1)
    if mid % 16 == 0:
        mid += 1
    return np.asarray([T, min(mid, T), 1], np.int64)


def _memo(case, name, fn):
    if name not in case["_memo"]:
        case["_memo"][name] = fn()
    return case["_memo"][name]


# ----------------------------------------------------------------------------------------------------------------- the heads

HEAD_B, HEAD_C = 3, 256
HEAD_T = (1, 15, 16, 17, 63, 64, 65, 130)
HEAD_EXTRA_LD = (17, 65)
HEAD_REGIMES = ("unit", "relu", "offset", "dead")
HEAD_MASKS = ("none", "same", "differ")
LN_O = (1, 10, 11)
CHAN_O = (1, 10, 11, 16)
LN_EPS, LN_EPS_ENC = 1e-12, 1e-5
# the dead column's value: every partial sum of 256 copies of it, in any order, is exact in float32, so the variance of the column is exactly 0
# in the kernels and in both evaluations of the definition
DEAD_VALUE = 1.5


def head_lds(T):
    return (ceil4(T), ceil4(T) + 8) if T in HEAD_EXTRA_LD else (ceil4(T),)


def energy_cases():
    """Every (T, ld, mode) the GPU test runs."""
    return [(T, ld, mode) for T in HEAD_T for ld in head_lds(T) for mode in ENERGY_MODES]


@functools.lru_cache(maxsize=None)
def head_weights(O):
    rs = np.random.RandomState(500 + O)
    W = (rs.standard_normal((O, HEAD_C)) / 16.0).astype(np.float32)
    bias = rs.standard_normal(O).astype(np.float32)
    _ro(W, bias)
    return W, bias


@functools.lru_cache(maxsize=None)
def head_case(T, ld, regime="unit", mask="none", O=1, eps=LN_EPS):
    """x float32 [B][256][ld] in one of the four regimes (unit: N(0, 1); relu: max(N(0, 1), 0), what the heads see in production; offset: per
    column mean 30 and deviation 0.05, where a one-pass variance loses every digit; dead: unit with one column of 256 equal values per
    utterance), LayerNorm parameters, a Linear(256 -> O), and the two length vectors of `mask` (none / same / differ)."""
    assert regime in HEAD_REGIMES and mask in HEAD_MASKS and ld >= T
    rs = np.random.RandomState(9000 + 13 * T + ld + 1000 * HEAD_REGIMES.index(regime))
    x = _garbage(rs, (HEAD_B, HEAD_C, ld))
    v = rs.standard_normal((HEAD_B, HEAD_C, T))
    if regime == "relu":
        v = np.maximum(v, 0)
    elif regime == "offset":
        v = 30.0 + 0.05 * v
    elif regime == "dead":
        v[:, :, T // 2] = DEAD_VALUE
    x[:, :, :T] = v
    g, be = TC.ln_params()
    W, bias = head_weights(O)
    lens = case_lens(T)
    ln_lens = None if mask == "none" else lens
    out_lens = None if mask == "none" else (lens if mask == "same" else np.ascontiguousarray(lens[::-1]))
    _ro(x, lens, out_lens)
    return {"T": T, "ld": ld, "regime": regime, "mask": mask, "O": O, "eps": eps, "x": x, "g": g, "be": be, "W": W, "bias": bias,
            "ln_lens": ln_lens, "out_lens": out_lens, "dead_col": T // 2 if regime == "dead" else None, "_memo": {}}


def _mask_cols(h, lens, axis_t):
    """Positions t >= lens[b] of h become 0 (t on axis `axis_t` of each utterance's slab)."""
    if lens is None:
        return h
    T = h.shape[axis_t + 1]
    keep = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    shape = [h.shape[0]] + [1] * (h.ndim - 1)
    shape[axis_t + 1] = T
    return np.where(keep.reshape(shape), h, 0).astype(h.dtype)


def layernorm_def(x, g, be, eps, dtype, lens=None, one_pass=False):
    """LayerNorm over the 256 channels of x [B][256][T] (two passes: mean, then the mean of the squared deviations; biased); columns >= lens[b] zero.
    one_pass: the WRONG variance E[x^2] - mean^2 (the CPU test's mutant)."""
    x = x.astype(dtype)
    mu = x.mean(1, keepdims=True, dtype=dtype)
    var = ((x * x).mean(1, keepdims=True, dtype=dtype) - mu * mu) if one_pass else ((x - mu) ** 2).mean(1, keepdims=True, dtype=dtype)
    h = ((x - mu) / np.sqrt(var + dtype(eps))).astype(dtype) * g.astype(dtype)[None, :, None] + be.astype(dtype)[None, :, None]
    return _mask_cols(h.astype(dtype), lens, 1)


def ln_linear_def(case, dtype, one_pass=False, masked_keeps_beta=False):
    """Linear(256 -> O)(LayerNorm(x)) -> [B][T][O]: a column masked by ln_lens enters the linear as 0, a position masked by out_lens is 0.
    masked_keeps_beta: the WRONG masked column (beta instead of 0)."""
    c, T = case, case["T"]
    h = layernorm_def(c["x"][:, :, :T], c["g"], c["be"], c["eps"], dtype, None if masked_keeps_beta else c["ln_lens"], one_pass)
    if masked_keeps_beta and c["ln_lens"] is not None:
        keep = np.arange(T)[None, None, :] < c["ln_lens"][:, None, None]
        h = np.where(keep, h, c["be"].astype(dtype)[None, :, None])
    out = np.einsum("bct,oc->bto", h, c["W"].astype(dtype)).astype(dtype) + c["bias"].astype(dtype)
    return _mask_cols(out.astype(dtype), c["out_lens"], 0)


def chan_linear_def(case, dtype):
    """Linear(256 -> O) over the channels of x -> [B][T][O]; positions >= lens[b] are 0 (the kernel takes one length vector: out_lens)."""
    c, T = case, case["T"]
    out = np.einsum("bct,oc->bto", c["x"][:, :, :T].astype(dtype), c["W"].astype(dtype)).astype(dtype) + c["bias"].astype(dtype)
    return _mask_cols(out.astype(dtype), c["out_lens"], 0)


def _head_refs(case, name, fn):
    def make():
        ref = fn(np.float64)
        return ref, yardstick(ref, fn(np.float32))
    return _memo(case, name, make)


def check_layernorm(got, case):
    """got [B][256][T]: by ratio; masked columns exactly 0; the dead column exactly beta."""
    c, T = case, case["T"]
    ref, d32 = _head_refs(c, "ln", lambda dt: layernorm_def(c["x"][:, :, :T], c["g"], c["be"], c["eps"], dt, c["ln_lens"]))
    if c["ln_lens"] is not None:
        for b in range(HEAD_B):
            assert not np.asarray(got)[b][:, int(c["ln_lens"][b]):].any(), ("layernorm_ct", "a masked column is not 0")
    if c["dead_col"] is not None:
        for b in range(HEAD_B):
            if c["ln_lens"] is None or c["dead_col"] < c["ln_lens"][b]:
                exact("layernorm_ct", np.asarray(got)[b][:, c["dead_col"]], c["be"], "the dead column is not beta")
    return ratio_check("layernorm_ct", got, ref, d32, (T, c["ld"], c["regime"], c["mask"]))


def _masked_zero(kernel, got, lens):
    if lens is not None:
        for b in range(len(lens)):
            assert not np.asarray(got)[b][int(lens[b]):].any(), (kernel, "a position masked by out_lens is not exactly 0")


def check_ln_linear(got, case, kernel="ln_linear"):
    """got [B][T][O]."""
    c = case
    ref, d32 = _head_refs(c, "lnl", lambda dt: ln_linear_def(c, dt))
    _masked_zero(kernel, got, c["out_lens"])
    return ratio_check(kernel, got, ref, d32, (c["T"], c["ld"], c["regime"], c["mask"], c["O"]))


def check_chan_linear(got, case):
    c = case
    ref, d32 = _head_refs(c, "chan", lambda dt: chan_linear_def(c, dt))
    _masked_zero("chan_linear", got, c["out_lens"])
    return ratio_check("chan_linear", got, ref, d32, (c["T"], c["ld"], c["regime"], c["mask"], c["O"]))


# ----------------------------------------------------------------------------------------------------------------- the energy epilogue

NBINS = 255
ENERGY_MODES = ("ctl1", "ctl1.3", "table", "target")
E_CONTROL = float(np.float32(1.3))
# at most 1 % of a case may lie within ENERGY_MARGIN of a bucket edge (asserted on the CPU); with 45 elements that is none: the first table drawn
# for (T, ld) = (15, 16) put one scaled prediction of 45 within that margin, so that case draws from another seed
ENERGY_RESEED = {(15, 16): 100000}


@functools.lru_cache(maxsize=None)
def energy_tables():
    """(bins float32 [255] strictly ascending, E float32 [256][256])."""
    rs = np.random.RandomState(321)
    bins = (np.linspace(-2.4, 2.4, NBINS) + rs.uniform(-0.004, 0.004, NBINS)).astype(np.float32)
    assert (np.diff(bins) > 0).all()
    E = rs.standard_normal((NBINS + 1, HEAD_C)).astype(np.float32)
    _ro(bins, E)
    return bins, E


@functools.lru_cache(maxsize=None)
def energy_case(T, ld, mode):
    """The energy predictor's head: head_case(relu, both masks set, O = 1) + xin, 255 bins, the embedding table and — by mode — the scalar
    control 1 or 1.3, a control table, or teacher-forced targets (exactly on bin edges, below the first, above the last, one NaN)."""
    assert mode in ENERGY_MODES
    c = dict(head_case(T, ld, "relu", "same", 1))
    c["_memo"] = {}
    rs = np.random.RandomState(7000 + 10 * T + ld + ENERGY_RESEED.get((T, ld), 0))
    xin = _garbage(rs, (HEAD_B, HEAD_C, ld))
    xin[:, :, :T] = rs.standard_normal((HEAD_B, HEAD_C, T))
    bins, E = energy_tables()
    table = rs.uniform(0.7, 1.4, (HEAD_B, T)).astype(np.float32)
    target = rs.uniform(-3.0, 3.0, (HEAD_B, T)).astype(np.float32)
    flat = target.reshape(-1)
    flat[0::5] = bins[(7 * np.arange(len(flat[0::5])) + 3) % NBINS]      # exactly on an edge
    if flat.size > 1:
        flat[1] = np.nan
    if flat.size > 2:
        flat[2] = bins[0] - np.float32(0.5)
    if flat.size > 3:
        flat[3] = bins[-1] + np.float32(0.5)
    if flat.size > 6:
        flat[6] = bins[-1]
    _ro(xin, table, target)
    c.update(mode=mode, xin=xin, bins=bins, E=E, e_table=table if mode == "table" else None, e_target=target if mode == "target" else None,
             e_control=E_CONTROL if mode == "ctl1.3" else 1.0)
    return c


def bucketize_def(v, bins, side="left"):
    """torch.bucketize(right=False): the first i with bins[i] >= v; NaN sorts last."""
    idx = np.searchsorted(bins, v, side=side).astype(np.int64)
    return np.where(np.isnan(v), len(bins), idx)


def energy_def(case, dtype, side="left"):
    """(pred [B][T], v = what is bucketized [B][T], e_idx [B][T]) in dtype."""
    c = case
    pred = ln_linear_def(c, dtype)[:, :, 0]
    if c["e_target"] is not None:
        v = c["e_target"].astype(dtype)
    elif c["e_table"] is not None:
        v = pred * c["e_table"].astype(dtype)
    else:
        v = pred * dtype(np.float32(c["e_control"]))
    return pred, v, bucketize_def(v, c["bins"].astype(dtype), side)


def check_energy(got, case):
    """got: dict(out [B][T][1], e_idx [B][T], out1 [B][256][ld], e_scaled [B][T], SENTINEL before the launch).  The prediction by ratio; e_scaled
    exactly the kernel's own prediction x control (untouched when the control is 1 or a target is given... with a table always written);
    e_idx exactly the bucket of the kernel's own scaled value; out1 = xin + E[e_idx] bit for bit, 0 in [T, ld); against float64 a bucket may
    differ by one where the float64 value is within FRAME_ENERGY_MARGIN of an edge.  Returns the prediction's ratio; .err_units = the largest
    pre-rounding error in buckets."""
    c, T = case, case["T"]
    pred = np.asarray(got["out"])[:, :, 0]
    r = check_ln_linear(got["out"], c, "energy_head")
    es = np.asarray(got["e_scaled"])
    if c["e_target"] is not None:
        v = c["e_target"]
        exact("energy_head", es, np.full_like(es, SENTINEL), "e_scaled written although a target is given")
    elif c["e_table"] is not None:
        v = pred * c["e_table"]
        exact("energy_head", es, v, "e_scaled is not prediction x table")
    elif c["e_control"] != 1.0:
        v = pred * np.float32(c["e_control"])
        exact("energy_head", es, v, "e_scaled is not prediction x control")
    else:
        v = pred
        exact("energy_head", es, np.full_like(es, SENTINEL), "e_scaled written although the control is 1")
    idx = np.asarray(got["e_idx"])
    exact("energy_head", idx, bucketize_def(v, c["bins"]), "e_idx is not the bucket of the kernel's own value")
    out1 = np.asarray(got["out1"])
    want = c["xin"][:, :, :T] + np.transpose(c["E"][idx], (0, 2, 1))
    same_bits("energy_head", out1[:, :, :T], want.astype(np.float32), "out1 != xin + E[e_idx]")
    assert not out1[:, :, T:].any(), ("energy_head", "out1[:, :, T:ld) is not 0")
    _, v64, idx64 = _memo(c, "e64", lambda: energy_def(c, np.float64))
    r.err_units = 0.0
    if c["e_target"] is None:
        u64 = TC.energy_units(v64, c["bins"])
        r.err_units = float(np.abs(TC.energy_units(v, c["bins"]) - u64).max())
        diff = idx != idx64
        assert (np.abs(idx - idx64) <= 1).all(), ("energy_head", "a bucket is off by more than one")
        assert (TC.int_margin(u64)[diff] < FRAME_ENERGY_MARGIN).all(), ("energy_head", "a bucket differs away from an edge")
    else:
        exact("energy_head", idx, idx64, "teacher-forced buckets")
    return r


# ----------------------------------------------------------------------------------------------------------------- durations

DUR_L = (1, 63, 64, 65, 128, 129, 200)
DUR_CONTROLS = (1.0, 0.5, float(np.float32(1.3)))
DUR_KINDS = ("clear", "spread")


def dur_cases(L):
    """Every (kind, control, table, B) the GPU test runs at L: three scalar controls and their constant tables, a varying table; B = 65 once."""
    return [(kind, ctl, table, B) for B in ((3, 65) if L == 200 else (3,)) for kind in DUR_KINDS
            for ctl, table in [(c, t) for c in DUR_CONTROLS for t in (None, "const")] + [(1.0, "vary")]]


@functools.lru_cache(maxsize=None)
def dur_case(L, kind="spread", control=1.0, table=None, B=3):
    """log_d float32 [B][L], |log_d| <= 6.  clear: float32(log1p(k + 0.25 s)), s in {1, 3}: exp - 1 stands 0.25 from every rounding boundary.
    spread: uniform, with exact zeros and values below log(0.5) (exp - 1 < -0.5: rounds to -1, clamped to 0).  The first 64 phonemes carry
    large durations in both: the carry into the second lane group is large.  table: None (the scalar `control`), "const" (a table holding
    `control`) or "vary" (a factor per phoneme)."""
    assert kind in DUR_KINDS and table in (None, "const", "vary")
    rs = np.random.RandomState(100 * L + B + (7 if kind == "clear" else 0))
    if kind == "clear":
        k = rs.randint(0, 40, (B, L))
        k[:, :64] += 200
        logd = np.log1p(k + 0.25 * rs.choice([1, 3], (B, L))).astype(np.float32)
    else:
        logd = rs.uniform(-6.0, 4.0, (B, L))
        logd[:, :64] = rs.uniform(3.0, 6.0, (B, min(L, 64)))
        for b in range(B):
            logd[b, 5 + b % 3::23] = 0.0
            logd[b, 7 + b % 3::29] = -1.0
            logd[b, 9 + b % 3::31] = -6.0
        logd = logd.astype(np.float32)
    tab = None
    if table == "const":
        tab = np.full((B, L), control, np.float32)
    elif table == "vary":
        tab = rs.uniform(0.5, 1.5, (B, L)).astype(np.float32)
    _ro(logd, tab)
    return {"L": L, "B": B, "kind": kind, "logd": logd, "control": float(np.float32(control)), "table": tab, "_memo": {}}


def durations_def(logd, ctl, dtype, cum_round=np.trunc):
    """(u = exp(log_d) - 1, d_rounded = max(rint(u) x control, 0), cum = cumsum(trunc(d_rounded)), mel_len) — model/modules.py:369-372 with the
    expansion's truncation (docs/HISTORY.md: mel2ph for non-integer d_control).  ctl: the fp32 scalar or table."""
    u = np.exp(logd.astype(dtype)) - dtype(1.0)
    d = np.maximum(np.rint(u) * np.asarray(ctl, np.float32).astype(dtype), 0).astype(dtype)
    cum = np.cumsum(cum_round(d).astype(np.int64), 1)
    return u, d, cum, cum[:, -1].copy()


def dur_ctl(case):
    return case["table"] if case["table"] is not None else np.float32(case["control"])


def check_durations(got, case):
    """got: dict(d_rounded float32 [B][L], cum int32 [B][L], mel_len int64 [B]).  cum == cumsum(trunc(d_rounded)) of the kernel's own d_rounded,
    mel_len == cum[:, -1]; against float64: clear must match exactly, spread may be off by one rounding step where the float64 pre-rounding
    value is within FRAME_DUR_MARGIN of a half integer.  Returns the fraction of such steps."""
    c = case
    d = np.asarray(got["d_rounded"])
    assert np.isfinite(d).all() and (d >= 0).all()
    cum = np.cumsum(np.trunc(d).astype(np.int64), 1)
    exact("durations", np.asarray(got["cum"]).astype(np.int64), cum, "cum != cumsum(trunc(d_rounded))")
    exact("durations", np.asarray(got["mel_len"]).astype(np.int64), cum[:, -1], "mel_len != cum[:, -1]")
    u64, d64, _, _ = _memo(c, "d64", lambda: durations_def(c["logd"], dur_ctl(c), np.float64))
    ctl = np.asarray(dur_ctl(c), np.float32).astype(np.float64)
    ok = d == d64.astype(np.float32)
    if c["kind"] == "clear":
        assert ok.all(), ("durations", "a clear duration differs from float64")
        return Ratio(0.0)
    n64 = np.rint(u64)
    near = TC.half_margin(u64) < FRAME_DUR_MARGIN
    step = np.zeros_like(ok)
    for s in (-1.0, 1.0):
        step |= d == np.maximum((n64 + s) * ctl, 0).astype(np.float32)
    assert (ok | (step & near)).all(), ("durations", "a duration differs from float64 away from a rounding boundary, or by more than one step")
    return Ratio(float((~ok).mean()))


# ----------------------------------------------------------------------------------------------------------------- cumsum_durations, mel2ph

CUM_T = (1, 255, 256, 257)
CUM_L = (1, 64, 200)
CUM_SCALES = {"long": (400, 256, 120, 0), "short": (200, 100, 3, 0)}      # mel_len per utterance: T = 1 lies below the shortest non-empty one,
#                                                                           255 .. 257 between the long ones and above the longest short one


@functools.lru_cache(maxsize=None)
def cumsum_case(L, scale="long"):
    """dur float32 [4][L]: integer durations that sum to CUM_SCALES[scale] with runs of zeros (about half the phonemes), a fraction in
    [0, 0.9] added to each (truncation drops it), negative entries (-0.5, -1.7) on some zeros, one utterance all zeros."""
    rs = np.random.RandomState(40 * L + len(scale))
    tg = CUM_SCALES[scale]
    dur = np.zeros((len(tg), L))
    for b, n in enumerate(tg):
        p = rs.random_sample(L) * (rs.random_sample(L) < 0.5)
        if L >= 8:
            p[L // 4:L // 4 + 3] = 0          # a run of zeros
        if p.sum() == 0:
            p[0] = 1
        dur[b] = rs.multinomial(n, p / p.sum())
    zero = dur == 0
    dur = dur + rs.uniform(0, 0.9, dur.shape)
    neg = zero & (rs.random_sample(dur.shape) < 0.3)
    dur[neg] = rs.choice([-0.5, -1.7], int(neg.sum()))
    dur = dur.astype(np.float32)
    _ro(dur)
    return {"L": L, "B": len(tg), "dur": dur, "mel_len": np.asarray(tg, np.int64), "_memo": {}}


def cumsum_def(dur):
    """LengthRegulator.expand: max(int(d), 0), summed."""
    cum = np.cumsum(np.maximum(np.trunc(dur).astype(np.int64), 0), 1)
    return cum, cum[:, -1].copy()


def mel2ph_def(cum, T):
    """mel2ph[b][t] = 1 + #{l : cum[l] <= t} for t < cum[L - 1], else 0 (utils/tools.py:793-797)."""
    t = np.arange(T)[None, :]
    idx = (np.asarray(cum)[:, None, :] <= t[:, :, None]).sum(-1)
    return np.where(t < np.asarray(cum)[:, -1:], idx + 1, 0).astype(np.int64)


def check_cumsum(got, case):
    cum, ml = cumsum_def(case["dur"])
    exact("cumsum_durations", np.asarray(got["cum"]).astype(np.int64), cum)
    return exact("cumsum_durations", np.asarray(got["mel_len"]).astype(np.int64), ml)


def check_mel2ph(got, case, T):
    cum, _ = cumsum_def(case["dur"])
    return exact("mel2ph", np.asarray(got).astype(np.int64), mel2ph_def(cum, T), T)


def frames_case(T, L, mel_lens, seed=0):
    """(cum int32 [B][L], mel2ph int64 [B][T]) of utterances with the given frame counts (runs of zero durations inside)."""
    rs = np.random.RandomState(seed + 3 * T + L)
    dur = np.zeros((len(mel_lens), L), np.int64)
    for b, n in enumerate(mel_lens):
        p = rs.random_sample(L) * (rs.random_sample(L) < 0.6)
        if p.sum() == 0:
            p[0] = 1
        dur[b] = rs.multinomial(n, p / p.sum())
    cum = np.cumsum(dur, 1)
    return cum.astype(np.int32), mel2ph_def(cum, T)


# ----------------------------------------------------------------------------------------------------------------- pitch_index

PITCH_T = (2, 3, 255, 256, 257, 700)
PITCH_EPS = 1e-9
PITCH_B = 3
PITCH_COMBOS = ((11, 2, 1.3), (11, 1, 1.0), (10, 1, 1.3), (10, 2, 1.0))      # (O, stat_ld, std_scale) the GPU test runs at every T
TINY = float(np.finfo(np.float32).tiny)


@functools.lru_cache(maxsize=None)
def pitch_case(T, O, stat_ld, std_scale):
    """cwt float32 [B][T][O]; O = 11: the uv logit in column 10 (exact 0 and -0: voiced; the smallest positive normal: unvoiced), O = 10: uv_mask
    bytes.  Per-utterance mean / deviation: buckets of utterances 0 and 1 span 1 .. 255, utterance 2 sits above 1100 Hz (the clip at 255)."""
    assert O in (10, 11) and stat_ld in (1, 2)
    rs = np.random.RandomState(60 * T + O + stat_ld)
    cwt = rs.standard_normal((PITCH_B, T, O)).astype(np.float32)
    uv_mask = None
    if O == 11:
        lg = rs.standard_normal((PITCH_B, T)).astype(np.float32)
        lg[:, 0::7] = 0.0
        lg[:, 1::7] = -0.0
        lg[:, 2::7] = TINY
        cwt[:, :, 10] = lg
    else:
        uv_mask = (rs.random_sample((PITCH_B, T)) < 0.3).astype(np.uint8) * rs.randint(1, 255, (PITCH_B, T)).astype(np.uint8)
    mean = np.asarray([6.0, 5.9, 7.8], np.float32)
    std = (np.asarray([0.7, 1.0, 0.1]) / std_scale).astype(np.float32)
    stats = np.ascontiguousarray(np.stack([mean, std], 1)) if stat_ld == 2 else None
    _ro(cwt, uv_mask, mean, std, stats)
    return {"T": T, "O": O, "stat_ld": stat_ld, "std_scale": float(np.float32(std_scale)), "cwt": cwt, "uv_mask": uv_mask, "mean": mean, "std": std,
            "stats": stats, "_memo": {}}


def pitch_def(case, dtype, ddof=1, uv_ge=False):
    """VarianceAdaptor.get_pitch_embedding's cwt branch (oracle/cmtts_oracle.py: cwt_to_pitch_index, f0_to_coarse) -> (r [B][T], f0_denorm, p_idx).
    ddof = 0 (the biased deviation) and uv_ge (logit >= 0 unvoiced) are the CPU test's mutants."""
    c = case
    spec = c["cwt"][:, :, :10].astype(dtype)
    scale = ((np.arange(10, dtype=dtype) + dtype(1) + dtype(2.5)) ** dtype(-2.5)).astype(dtype)
    r = (spec * scale[None, None, :]).sum(-1, dtype=dtype)
    rn = ((r - r.mean(-1, keepdims=True, dtype=dtype)) / r.std(-1, ddof=ddof, keepdims=True, dtype=dtype)).astype(dtype)
    std = c["std"].astype(dtype) * dtype(np.float32(c["std_scale"]))
    f0 = np.exp(rn * std[:, None] + c["mean"].astype(dtype)[:, None]).astype(dtype)
    f0d = np.exp2(np.log2(f0 + dtype(PITCH_EPS)).astype(dtype)).astype(dtype)
    f0d = np.where(unvoiced(c, uv_ge), dtype(0), f0d)
    mel = (dtype(1127) * np.log(dtype(1) + f0d / dtype(700))).astype(dtype)
    lo, hi = 1127 * np.log(1 + 50.0 / 700), 1127 * np.log(1 + 1100.0 / 700)
    mel = np.where(mel > 0, (mel - dtype(lo)) * dtype(254) / dtype(hi - lo) + dtype(1), mel)
    mel = np.clip(mel, dtype(1), dtype(255)).astype(dtype)
    return r, f0d, (mel + dtype(0.5)).astype(np.int64)


def unvoiced(case, uv_ge=False):
    if case["O"] == 11:
        lg = case["cwt"][:, :, 10]
        return (lg >= 0) if uv_ge else (lg > 0)
    return case["uv_mask"] != 0


def check_pitch(got, case):
    """got: dict(r_ws [B][T], f0_denorm [B][T], p_idx [B][T]).  r_ws and f0_denorm by ratio per utterance; unvoiced frames exactly 0 and bucket 1;
    a bucket differs from float64's only by one and only where conftest.pitch_margin_mask puts the float64 value on a boundary.
    .err_units = the largest pre-rounding error in buckets."""
    c = case
    r64, f64, i64 = _memo(c, "p64", lambda: pitch_def(c, np.float64))
    r32, f32, _ = _memo(c, "p32", lambda: pitch_def(c, np.float32))
    f0, idx = np.asarray(got["f0_denorm"]), np.asarray(got["p_idx"])
    uv = unvoiced(c)
    assert not f0[uv].any() and (idx[uv] == 1).all(), ("pitch_index", "an unvoiced frame is not (0, bucket 1)")
    out = Ratio(0.0)
    for b in range(PITCH_B):
        ra = ratio_check("pitch_index", np.asarray(got["r_ws"])[b], r64[b], yardstick(r64[b], r32[b]), (c["T"], b))
        rb = ratio_check("pitch_index", f0[b], f64[b], yardstick(f64[b], f32[b]), (c["T"], b))
        out = worst(out, ra, rb)
    diff = idx != i64
    assert (np.abs(idx - i64) <= 1).all(), ("pitch_index", "a bucket is off by more than one")
    assert not (diff & pitch_margin_mask(f64, FRAME_PITCH_MARGIN)).any(), ("pitch_index", "a bucket differs away from a rounding boundary")
    out.err_units = float(np.abs(TC.pitch_units(f0) - TC.pitch_units(f64)).max())
    return out


# ----------------------------------------------------------------------------------------------------------------- pitch_table_scale

def pitch_table_case(T, L=37, O=11):
    """cwt [B][T][O], mel2ph, cum and a factor table [B][L] for utterances with mel_len = T, > T, 0 and T // 2."""
    rs = np.random.RandomState(5 * T + L)
    mel_lens = (T, T + 37, 0, T // 2)
    cum, _ = frames_case(T + 37, L, mel_lens, 11)
    m2p = mel2ph_def(cum, T)
    cwt = rs.standard_normal((len(mel_lens), T, O)).astype(np.float32)
    ptab = rs.uniform(0.5, 1.5, (len(mel_lens), L)).astype(np.float32)
    return {"T": T, "L": L, "O": O, "B": len(mel_lens), "cwt": cwt, "mel2ph": m2p, "cum": cum, "ptab": ptab}


def pitch_table_def(case):
    """cwt[b][t][:] *= ptab[b][ph - 1]; ph = mel2ph[b][t], a padding frame (ph = 0) takes the last frame's (mel2ph[b][mel_len - 1] when
    0 < mel_len <= T, else 1); clamped to [1, L] (kernels.hip: pitch_table_scale_kernel's comment)."""
    c = case
    out = c["cwt"].copy()
    for b in range(c["B"]):
        ml = int(c["cum"][b, -1])
        last = int(c["mel2ph"][b, ml - 1]) if 0 < ml <= c["T"] else 1
        ph = np.where(c["mel2ph"][b] > 0, c["mel2ph"][b], last)
        ph = np.clip(ph, 1, c["L"])
        out[b] *= c["ptab"][b][ph - 1][:, None]
    return out


def check_pitch_table(got, case):
    return same_bits("pitch_table_scale", np.asarray(got), pitch_table_def(case))


# ----------------------------------------------------------------------------------------------------------------- gathers

GATHER_T = (1, 257)
GATHER_C, GATHER_L, GATHER_LDL, GATHER_NE = 8, 37, 40, 19


@functools.lru_cache(maxsize=None)
def gather_case(T):
    rs = np.random.RandomState(800 + T)
    B = 3
    _, m2p = frames_case(T, GATHER_L, (T, max(int(0.6 * T), 1) if T > 1 else 0, 0), 21)
    out1 = _garbage(rs, (B, GATHER_C, GATHER_LDL))
    out1[:, :, :GATHER_L] = rs.standard_normal((B, GATHER_C, GATHER_L))
    x = rs.standard_normal((B, GATHER_C, T)).astype(np.float32)
    idx = rs.randint(0, GATHER_NE, (B, T)).astype(np.int64)
    E = rs.standard_normal((GATHER_NE, GATHER_C)).astype(np.float32)
    padv = rs.standard_normal(GATHER_C).astype(np.float32)
    _ro(m2p, out1, x, idx, E, padv)
    return {"T": T, "B": B, "mel2ph": m2p, "out1": out1, "x": x, "idx": idx, "E": E, "padv": padv}


def length_regulate_def(case, padv=None):
    c = case
    g = np.take_along_axis(c["out1"], np.maximum(c["mel2ph"] - 1, 0)[:, None, :].repeat(GATHER_C, 1), 2)
    pad = np.zeros(GATHER_C, np.float32) if padv is None else padv
    return np.where(c["mel2ph"][:, None, :] > 0, g, pad[None, :, None]).astype(np.float32)


def check_length_regulate(got, case, with_padv):
    return same_bits("length_regulate", np.asarray(got), length_regulate_def(case, case["padv"] if with_padv else None))


def check_lr_gather_add(got, case):
    want = length_regulate_def(case) + np.transpose(case["E"][case["idx"]], (0, 2, 1))
    return same_bits("lr_gather_add", np.asarray(got), want.astype(np.float32))


def check_gather_add(got, case):
    want = case["x"] + np.transpose(case["E"][case["idx"]], (0, 2, 1))
    return same_bits("gather_add", np.asarray(got), want.astype(np.float32))


# ----------------------------------------------------------------------------------------------------------------- positions

POS_T = (1, 255, 256, 257, 600)          # block_positions gives a thread 1, 2 or 3 positions
POS_C, EMB_C, POS_B = 24, 40, 3          # three channel groups of 8 (pos_embed_add); one full and one ragged group of 32 (embed_tokens)
POS_TAB_ROWS = (0, 100, 700)             # computed branch only / both / table branch only
POS_ALPHA = float(np.float32(1.25))
LR_L, LR_LDL = 50, 52
N_SYM = 60


def pos_omega(Cn):
    half = Cn // 2
    e = np.float32(math.log(10000) / (half - 1))
    return np.exp(np.arange(half, dtype=np.float32) * -e).astype(np.float32)


def pos_embed(pos, Cn):
    """float32 [..., C]: row p = [sin(p w_j) | cos(p w_j)] with the fp32 product p w_j as the argument and the float64 sine / cosine rounded to
    fp32 (kernels.hip: pos_embed; the host-built table follows the same recipe); p = 0 is the zero row."""
    arg = (np.asarray(pos).astype(np.float32)[..., None] * pos_omega(Cn)).astype(np.float32).astype(np.float64)
    pe = np.concatenate([np.sin(arg), np.cos(arg)], -1).astype(np.float32)
    return np.where(np.asarray(pos)[..., None] == 0, np.float32(0), pe)


def pos_table(rows, Cn):
    return np.ascontiguousarray(pos_embed(np.arange(max(rows, 1)), Cn))


def positions_def(flags, skip=True):
    """cumsum(flag) * flag (utils/tools.py:810-822).  skip = False: the WRONG positions that count every frame up to the last flagged one."""
    f = flags.astype(np.int64)
    return np.cumsum(f if skip else np.ones_like(f), 1) * f


@functools.lru_cache(maxsize=None)
def pos_case(T):
    """x [B][C][ld]: channel 0 is exactly 0.0 at T // 3 and -0.0 at T // 2 (false flags in the middle of the frames); lens shorter than the
    flagged span in utterances 1 and 2."""
    rs = np.random.RandomState(1700 + T)
    ld = ceil4(T)
    x = _garbage(rs, (POS_B, POS_C, ld))
    x[:, :, :T] = rs.standard_normal((POS_B, POS_C, T))
    if T >= 3:
        x[:, 0, T // 3] = 0.0
        x[:, 0, T // 2] = -0.0
    lens = case_lens(T)
    _ro(x, lens)
    return {"T": T, "ld": ld, "x": x, "lens": lens, "_memo": {}}


def pos_embed_add_def(case, dtype, masked, skip=True):
    c, T = case, case["T"]
    x = c["x"][:, :, :T]
    pe = pos_embed(positions_def(x[:, 0, :] != 0, skip), POS_C)                      # [B][T][C]
    out = x.astype(dtype) + dtype(np.float32(POS_ALPHA)) * np.transpose(pe, (0, 2, 1)).astype(dtype)
    return _mask_cols(out.astype(dtype), c["lens"] if masked else None, 1)


def check_pos_embed_add(got, case, masked):
    c = case
    ref, d32 = _head_refs(c, ("pea", masked), lambda dt: pos_embed_add_def(c, dt, masked))
    if masked:
        for b in range(POS_B):
            assert not np.asarray(got)[b][:, int(c["lens"][b]):].any(), ("pos_embed_add", "a column beyond lens is not 0")
    return ratio_check("pos_embed_add", got, ref, d32, (c["T"], masked))


@functools.lru_cache(maxsize=None)
def pos_lr_case(T, pad0_zero):
    """src [B][C][ldl] over 50 phonemes (channel 0 of one phoneme in the middle exactly 0), mel2ph with padding frames in utterances 1 and 2,
    padv with padv[0] zero (padding frames take position 0) or non-zero (they go on counting)."""
    rs = np.random.RandomState(2300 + T)
    _, m2p = frames_case(T, LR_L, (T, max(int(0.6 * T), 1) if T > 1 else 0, 0), 31)
    src = _garbage(rs, (POS_B, POS_C, LR_LDL))
    src[:, :, :LR_L] = rs.standard_normal((POS_B, POS_C, LR_L))
    mid = int(m2p[0, T // 2]) - 1          # a phoneme that has frames in the middle of utterance 0
    src[:, 0, max(mid, 0)] = 0.0
    padv = rs.standard_normal(POS_C).astype(np.float32)
    if pad0_zero:
        padv[0] = 0.0
    _ro(m2p, src, padv)
    return {"T": T, "mel2ph": m2p, "src": src, "padv": padv, "_memo": {}}


def pos_embed_add_lr_def(case, dtype, skip=True):
    c = case
    g = np.take_along_axis(c["src"], np.maximum(c["mel2ph"] - 1, 0)[:, None, :].repeat(POS_C, 1), 2)
    x = np.where(c["mel2ph"][:, None, :] > 0, g, c["padv"][None, :, None]).astype(np.float32)
    pe = pos_embed(positions_def(x[:, 0, :] != 0, skip), POS_C)
    return (x.astype(dtype) + dtype(np.float32(POS_ALPHA)) * np.transpose(pe, (0, 2, 1)).astype(dtype)).astype(dtype)


def check_pos_embed_add_lr(got, case):
    c = case
    ref, d32 = _head_refs(c, "pealr", lambda dt: pos_embed_add_lr_def(c, dt))
    return ratio_check("pos_embed_add_lr", got, ref, d32, c["T"])


@functools.lru_cache(maxsize=None)
def embed_case(L):
    """texts int64 [B][L] (a token 0 inside the text of utterance 0; utterance 1 keeps non-zero tokens beyond its length), lens, E [60][40]."""
    rs = np.random.RandomState(2900 + L)
    texts = rs.randint(1, N_SYM, (POS_B, L)).astype(np.int64)
    lens = case_lens(L)
    if L >= 3:
        texts[0, L // 2] = 0
    texts[2, int(lens[2]):] = 0
    E = rs.standard_normal((N_SYM, EMB_C)).astype(np.float32)
    _ro(texts, lens, E)
    return {"L": L, "ld": ceil4(L), "texts": texts, "lens": lens, "E": E, "scale": float(np.float32(math.sqrt(EMB_C))), "_memo": {}}


def embed_tokens_def(case, dtype, skip=True):
    """x[b][c][l] = scale E[tok][c] + PE[position(tok != 0)][c] for l < lens[b], else 0 (model/modules.py:145-151, :94)."""
    c = case
    pe = pos_embed(positions_def(c["texts"] != 0, skip), EMB_C)
    out = dtype(np.float32(c["scale"])) * c["E"][c["texts"]].astype(dtype) + pe.astype(dtype)          # [B][L][C]
    return _mask_cols(np.transpose(out, (0, 2, 1)).astype(dtype), c["lens"], 1)


def check_embed_tokens(got, case):
    c = case
    ref, d32 = _head_refs(c, "emb", lambda dt: embed_tokens_def(c, dt))
    for b in range(POS_B):
        assert not np.asarray(got)[b][:, int(c["lens"][b]):].any(), ("embed_tokens", "a column beyond lens is not 0")
    return ratio_check("embed_tokens", got, ref, d32, c["L"])


# ----------------------------------------------------------------------------------------------------------------- small dense

DENSE_NONE, DENSE_RELU, DENSE_MISH = 0, 1, 2
DENSE_B = (1, 8, 9)
DENSE_N = (1, 63, 64, 65, 130)
DENSE_K = (3, 255, 256, 1024)
DB = 8                                   # kernels.hip: batch rows per workgroup


def dense_slices(B, K, N):
    """k_dense_small's rule: 16 K slices when K >= 512 and fewer than 128 workgroups (ceil(N / 64) x ceil(B / 8)), else 4."""
    return 16 if K >= 512 and -(-N // 64) * -(-B // DB) < 128 else 4


@functools.lru_cache(maxsize=None)
def dense_case(B, K, N, in_ks=1):
    """in [B][K] (element stride in_ks: the gaps hold GARBAGE), Wt [K][N] scaled so that the sums have deviation ~ 8, bias spread over [-25, 25]:
    pre-activations on both sides of Mish's v > 20 branch and down to where log1p(exp(v)) underflows; add [B][N]."""
    rs = np.random.RandomState(K * 7 + N * 3 + B)
    raw = _garbage(rs, (B, K * in_ks))
    x = rs.standard_normal((B, K)).astype(np.float32)
    raw[:, ::in_ks] = x
    Wt = (rs.standard_normal((K, N)) * 8.0 / math.sqrt(K)).astype(np.float32)
    bias = np.linspace(-25.0, 25.0, N).astype(np.float32) if N > 1 else np.asarray([21.0], np.float32)
    add = rs.standard_normal((B, N)).astype(np.float32)
    _ro(raw, x, Wt, bias, add)
    return {"B": B, "K": K, "N": N, "in_ks": in_ks, "raw": raw, "x": x, "Wt": Wt, "bias": bias, "add": add, "_memo": {}}


def mish_def(v, dtype):
    """model/blocks.py:621-623: v tanh(softplus(v)), softplus with torch's threshold 20."""
    sp = np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, dtype(20))))).astype(dtype)
    return (v * np.tanh(sp)).astype(dtype)


def dense_def(case, dtype, act, with_bias, with_add):
    c = case
    v = (c["x"].astype(dtype) @ c["Wt"].astype(dtype)).astype(dtype)
    if with_bias:
        v = v + c["bias"].astype(dtype)
    if act == DENSE_RELU:
        v = np.maximum(v, 0)
    elif act == DENSE_MISH:
        v = mish_def(v, dtype)
    if with_add:
        v = v + c["add"].astype(dtype)
    return v.astype(dtype)


def check_dense(got, case, act, with_bias, with_add):
    c = case
    ref, d32 = _head_refs(c, ("dense", act, with_bias, with_add), lambda dt: dense_def(c, dt, act, with_bias, with_add))
    return ratio_check("dense_small", got, ref, d32, (c["B"], c["K"], c["N"], act, with_bias, with_add))


STATS_SHAPES = ((256, 130, 70, 2), (256, 256, 128, 2))      # (K0, N0, N1, N2): widths that are no multiples of 128, and the model's own
STATS_DECLINED = (8192, 4096, 64, 2)                         # (K0 + N0 + N1 + 3 * 128) floats > 48 KB of LDS
STATS_B = 3


def stats_lds_bytes(K0, N0, N1):
    return (K0 + N0 + N1 + 3 * 128) * 4


@functools.lru_cache(maxsize=None)
def stats_case(shape):
    K0, N0, N1, N2 = shape
    rs = np.random.RandomState(K0 + N0 + N1)
    x = rs.standard_normal((STATS_B, K0)).astype(np.float32)
    Ws = [(rs.standard_normal((k, n)) * 1.5 / math.sqrt(k)).astype(np.float32) for k, n in ((K0, N0), (N0, N1), (N1, N2))]
    bs = [rs.standard_normal(n).astype(np.float32) for n in (N0, N1, N2)]
    _ro(x, *Ws, *bs)
    return {"shape": shape, "x": x, "W": Ws, "b": bs, "_memo": {}}


def stats_def(case, dtype):
    c = case
    h = c["x"].astype(dtype)
    for i in range(3):
        h = (h @ c["W"][i].astype(dtype)).astype(dtype) + c["b"][i].astype(dtype)
        if i < 2:
            h = np.maximum(h, 0)
    return h.astype(dtype)


def check_stats_mlp(got, case):
    c = case
    ref, d32 = _head_refs(c, "stats", lambda dt: stats_def(c, dt))
    return ratio_check("stats_mlp", got, ref, d32, c["shape"])


SOFTMAX_L = (1, 63, 64, 65, 130)
SOFTMAX_H, SOFTMAX_B = 2, 4
SOFTMAX_REGIMES = ("unit", "overflow")


def softmax_lens(L):
    return np.asarray([L, case_lens(L)[1], 1, 0], np.int64)


@functools.lru_cache(maxsize=None)
def softmax_case(L, regime):
    """st [B H][L keys][ld]: column i = one query.  unit: N(0, 1) scores; overflow: x 25 (beyond 89, where expf without the max subtraction is inf).
    Masked key rows hold scores that would win (+400), [L, ld) holds GARBAGE."""
    rs = np.random.RandomState(3100 + L + (1 if regime == "overflow" else 0))
    ld = ceil4(L)
    lens = softmax_lens(L)
    st = _garbage(rs, (SOFTMAX_B * SOFTMAX_H, L, ld))
    st[:, :, :L] = rs.standard_normal((SOFTMAX_B * SOFTMAX_H, L, L)) * (25.0 if regime == "overflow" else 1.0)
    for z in range(SOFTMAX_B * SOFTMAX_H):
        st[z, int(lens[z // SOFTMAX_H]):, :L] = 400.0
    _ro(st, lens)
    return {"L": L, "ld": ld, "regime": regime, "st": st, "lens": lens, "_memo": {}}


def softmax_def(case, dtype):
    c, L = case, case["L"]
    out = np.zeros((SOFTMAX_B * SOFTMAX_H, L, L), dtype)
    for z in range(out.shape[0]):
        n = int(min(c["lens"][z // SOFTMAX_H], L))
        if n:
            s = c["st"][z, :n, :L].astype(dtype)
            p = np.exp(s - s.max(0, keepdims=True))
            out[z, :n] = p / p.sum(0, keepdims=True, dtype=dtype)
    return out


def check_softmax(got, case):
    """got [B H][L][L] (the columns < L of the buffer after the launch): masked keys exactly 0, a len = 0 utterance all zeros."""
    c = case
    ref, d32 = _head_refs(c, "sm", lambda dt: softmax_def(c, dt))
    for z in range(ref.shape[0]):
        assert not np.asarray(got)[z, int(c["lens"][z // SOFTMAX_H]):].any(), ("softmax_cols", "a masked key is not exactly 0")
    return ratio_check("softmax_cols", got, ref, d32, (c["L"], c["regime"]))


REDUCE_NSEG, REDUCE_B = 8, 2
REDUCE_C = (256, 6)
REDUCE_L = (1, 65)


@functools.lru_cache(maxsize=None)
def reduce_case(Cn, L):
    rs = np.random.RandomState(3300 + Cn + L)
    ld = ceil4(L)
    part = _garbage(rs, (REDUCE_B, REDUCE_NSEG, Cn, ld))
    part[..., :L] = rs.standard_normal((REDUCE_B, REDUCE_NSEG, Cn, L))
    bias = rs.standard_normal(Cn).astype(np.float32)
    res = _garbage(rs, (REDUCE_B, Cn, ld))
    res[..., :L] = rs.standard_normal((REDUCE_B, Cn, L))
    lens = np.asarray([L, max(int(0.6 * L), 1)], np.int64)
    _ro(part, bias, res, lens)
    return {"C": Cn, "L": L, "ld": ld, "part": part, "bias": bias, "res": res, "lens": lens, "_memo": {}}


def reduce_def(case, dtype, with_bias, with_res, with_lens):
    """mask(((p_0 + p_1) + ... + p_7) + bias + res), left to right."""
    c, L = case, case["L"]
    v = c["part"][:, 0, :, :L].astype(dtype)
    for s in range(1, REDUCE_NSEG):
        v = v + c["part"][:, s, :, :L].astype(dtype)
    if with_bias:
        v = v + c["bias"].astype(dtype)[None, :, None]
    if with_res:
        v = v + c["res"][..., :L].astype(dtype)
    return _mask_cols(v.astype(dtype), c["lens"] if with_lens else None, 1)


def check_reduce(got, case, with_bias, with_res, with_lens):
    """Only adds, in a stated order: the float32 left-to-right sum exactly, and float64 by ratio."""
    c = case
    same = reduce_def(c, np.float32, with_bias, with_res, with_lens)
    exact("reduce_partials", np.asarray(got), same, (c["C"], c["L"], with_bias, with_res, with_lens))
    ref = reduce_def(c, np.float64, with_bias, with_res, with_lens)
    return ratio_check("reduce_partials", got, ref, yardstick(ref, same), (c["C"], c["L"]))


POST_T = (1, 3, 4, 5, 1023, 1024, 1025, 1029)
POST_C = (32, 30)
POST_KW = (7, 3)
POST_B = 2
POST_DIV, POST_SLOPE = 3.0, 0.01


def post_takes_v4(T, ld, KW, aligned=True):
    """k_conv_post's rule for the 16-byte-load kernel (post_v4 on): KW <= 7, rows 16-byte aligned holding whole float4s up to the last sample's, T >= 4."""
    return KW <= 7 and KW // 2 <= 4 and ld % 4 == 0 and aligned and ld >= ceil4(T) and T >= 4


@functools.lru_cache(maxsize=None)
def post_case(T, Cn, KW, ld):
    rs = np.random.RandomState(3500 + T + Cn + KW + ld)
    x = _garbage(rs, (POST_B, Cn, ld))
    x[..., :T] = rs.standard_normal((POST_B, Cn, T)) * 3.0
    w = (rs.standard_normal((Cn, KW)) / math.sqrt(Cn * KW)).astype(np.float32)
    w[:, KW // 2 + 1:] += np.float32(0.05)          # taps differ in their mean: a mirrored kernel is not a symmetry
    bias = np.asarray([0.1], np.float32)
    _ro(x, w, bias)
    return {"T": T, "C": Cn, "KW": KW, "ld": ld, "x": x, "w": w, "bias": bias, "_memo": {}}


def conv_post_def(case, dtype):
    """tanh(Conv1d(C -> 1, KW, same padding)(leaky_relu(x / 3, 0.01)) + b) (hifigan/models.py:161-163)."""
    c, T, KW = case, case["T"], case["KW"]
    v = c["x"][..., :T].astype(dtype) / dtype(POST_DIV)
    v = np.where(v > 0, v, v * dtype(np.float32(POST_SLOPE))).astype(dtype)
    pad = KW // 2
    vp = np.zeros((POST_B, c["C"], T + 2 * pad), dtype)
    vp[..., pad:pad + T] = v
    acc = np.zeros((POST_B, T), dtype)
    for k in range(KW):
        acc += np.einsum("bct,c->bt", vp[..., k:k + T], c["w"][:, k].astype(dtype))
    return np.tanh(acc + dtype(c["bias"][0])).astype(dtype)


def check_conv_post(got, case):
    c = case
    ref, d32 = _head_refs(c, "post", lambda dt: conv_post_def(c, dt))
    return ratio_check("conv_post", got, ref, d32, (c["T"], c["C"], c["KW"], c["ld"]))


MEL_T = (1, 3, 4, 100)
MEL_M, MEL_B = 80, 3
POSTROW_RENOISE, POSTROW_FINAL = 1, 2


class PostRow(C.Structure):
    """struct PostRow (cm-tts_amd/csrc/persist_args.h)."""
    _fields_ = [("c_out", C.c_float), ("c_skip", C.c_float), ("nstd", C.c_float), ("flags", C.c_uint)]


@functools.lru_cache(maxsize=None)
def mel_case(T):
    rs = np.random.RandomState(3700 + T)
    x = rs.standard_normal((MEL_B, T, MEL_M)).astype(np.float32)
    F = rs.standard_normal((MEL_B, MEL_M, T)).astype(np.float32)
    noise = rs.standard_normal((MEL_B, T, MEL_M)).astype(np.float32)
    scale_b = np.asarray([0.3, 1.7, 0.9], np.float32)
    rows = np.asarray([[0.7, 0.4, 1.1, POSTROW_RENOISE], [0.2, 0.9, 0.6, 0], [0.5, 0.5, 0.8, POSTROW_RENOISE | POSTROW_FINAL]], np.float32)
    tsteps = np.asarray([0.0, 13.5, 947.25], np.float32)
    _ro(x, F, noise, scale_b, rows, tsteps)
    return {"T": T, "x": x, "F": F, "noise": noise, "scale_b": scale_b, "rows": rows, "scale": float(np.float32(0.37)),
            "c": tuple(float(np.float32(v)) for v in (0.7, 0.4, 1.1)), "t": tsteps, "_memo": {}}


def mel_prep_def(case, dtype, per_utt):
    c = case
    s = c["scale_b"].astype(dtype)[:, None, None] if per_utt else dtype(np.float32(c["scale"]))
    return (s * np.transpose(c["x"], (0, 2, 1)).astype(dtype)).astype(dtype)


def mel_post_def(case, dtype, with_xold, with_noise, rows=None):
    """c_out F^T + c_skip xold + noise nstd 0.85 -> [B][T][M]; rows: [B][4] per-utterance (c_out, c_skip, nstd, flags: bit 0 = add the noise term)."""
    c = case
    Ft = np.transpose(c["F"], (0, 2, 1)).astype(dtype)
    if rows is None:
        co, cs, ns = (np.full((MEL_B, 1, 1), np.float32(v)).astype(dtype) for v in c["c"])
        noisy = np.full((MEL_B, 1, 1), with_noise)
    else:
        co, cs, ns = (rows[:, i].astype(dtype)[:, None, None] for i in range(3))
        noisy = ((rows[:, 3].astype(np.int64) & POSTROW_RENOISE) != 0)[:, None, None] & with_noise
    v = co * Ft
    if with_xold:
        v = v + cs * c["x"].astype(dtype)
    return np.where(noisy, v + c["noise"].astype(dtype) * ns * dtype(np.float32(0.85)), v).astype(dtype)


def check_mel_prep(got, case, per_utt):
    c = case
    ref, d32 = _head_refs(c, ("prep", per_utt), lambda dt: mel_prep_def(c, dt, per_utt))
    return ratio_check("mel_prep", got, ref, d32, (c["T"], per_utt))


def check_mel_post(got, case, with_xold, with_noise):
    c = case
    ref, d32 = _head_refs(c, ("post", with_xold, with_noise), lambda dt: mel_post_def(c, dt, with_xold, with_noise))
    return ratio_check("mel_post", got, ref, d32, (c["T"], with_xold, with_noise))


def check_mel_post_rows(got_out, got_final, case, before):
    """Utterances with POSTROW_FINAL land in out_final and leave `out` as it was (`before`), the others the other way round."""
    c = case
    ref, d32 = _head_refs(c, "rows", lambda dt: mel_post_def(c, dt, True, True, c["rows"]))
    final = (c["rows"][:, 3].astype(np.int64) & POSTROW_FINAL) != 0
    r = Ratio(0.0)
    for b in range(MEL_B):
        mine, other = (got_final, got_out) if final[b] else (got_out, got_final)
        exact("mel_post_rows", np.asarray(other)[b], np.full_like(np.asarray(other)[b], before), "the other destination was written")
        r = worst(r, ratio_check("mel_post_rows", np.asarray(mine)[b], ref[b], d32, (c["T"], b)))
    return r


DIFF_C = 128


def diff_embed_def(case, dtype):
    """[sin(t w) | cos(t w)] with the fp32 product as the argument (model/blocks.py:633-640; kernels.hip: float64 sine of the fp32 product)."""
    arg = (case["t"][:, None] * pos_omega(DIFF_C)[None, :]).astype(np.float32).astype(dtype)
    return np.concatenate([np.sin(arg), np.cos(arg)], 1).astype(dtype)


def check_diff_embed(got, case):
    c = case
    ref, d32 = _head_refs(c, "diff", lambda dt: diff_embed_def(c, dt))
    return ratio_check("diff_embed", got, ref, d32)


# ----------------------------------------------------------------------------------------------------------------- conv_mfma.hip

ACT_NONE, ACT_RELU, ACT_GELU_ERF, ACT_TANH = 0, 1, 2, 3
EPI_PLAIN, EPI_GATED = 0, 1
INT_MAX = TC.INT_MAX
CONV_FIELDS = ("M", "N", "K", "taps", "dil", "pad", "Tin", "a_ld", "a_cols", "a_tap_stride", "ldx", "zdiv", "a_zs0", "a_zs1", "x_zs0", "x_zs1",
               "pre_div", "pre_slope", "split")
OUT_FIELDS = ("y_zs0", "y_zs1", "ldy", "row_off", "Tout", "ostride", "ooff_base", "ooff_mul", "bvec_zs", "r_zs0", "r_zs1", "ldr", "alpha", "act",
              "div", "rmul", "accum")
OUT_DEFAULTS = dict(y_zs0=0, y_zs1=0, ldy=0, row_off=0, Tout=0, ostride=1, ooff_base=0, ooff_mul=0, bvec_zs=0, r_zs0=0, r_zs1=0, ldr=0, alpha=1.0,
                    act=ACT_NONE, div=1.0, rmul=0.0, accum=0, Y=None, bias=None, bvec=None, res=None, lens=None)
CONV_CONFIGS = ("gated", "split", "kc64", "tb5", "plain64", "t64x256", "t32x256", "shortm", "convT")
CONV_TILE_N = {"gated": 128, "split": 128, "kc64": 64, "tb5": 64, "plain64": 64, "t64x256": 256, "t32x256": 256, "shortm": 64, "convT": 256}


def conv_config(a, epi, nbatch):
    """cmtts_launch_conv's rule restated: (BM, BN, KC, taps per barrier), or -2 for what it refuses."""
    halo = (a["taps"] - 1) * abs(a["dil"])
    if a["a_ld"] % 4 or a["a_cols"] % 4:
        return -2

    def cfg(*t):
        return -2 if halo > 64 else t
    if epi == EPI_GATED:
        return -2 if a["M"] % 64 else cfg(128, 128, 16, 1)
    if a["M"] > 64:
        if a["split"] != INT_MAX and a["split"] % 128:
            return -2
        big = -(-a["N"] // 128) * -(-a["M"] // 128) * nbatch
        if big < 512 and a["split"] == INT_MAX:
            if a["taps"] == 1 and a["K"] >= 128:
                return cfg(64, 64, 64, 1)
            return cfg(64, 64, 16, 5) if a["taps"] > 1 else cfg(64, 64, 16, 1)
        return cfg(128, 128, 16, 1)
    if a["split"] != INT_MAX:
        return -2
    if a["taps"] == 1 and a["K"] >= 128 and -(-a["N"] // 256) * nbatch < 256:
        return cfg(64, 64, 64, 1)
    return cfg(64, 256, 16, 1) if a["M"] > 32 else cfg(32, 256, 16, 1)


CONV_EXPECT = {"gated": (128, 128, 16, 1), "split": (128, 128, 16, 1), "kc64": (64, 64, 64, 1), "tb5": (64, 64, 16, 5), "plain64": (64, 64, 16, 1),
               "t64x256": (64, 256, 16, 1), "t32x256": (32, 256, 16, 1), "shortm": (64, 64, 64, 1), "convT": (32, 256, 16, 1)}


def _kmajor_weights(rs, taps, K, M, a_ld, nz=1):
    """A[z][tap][k][m] built directly k-major, columns [M, a_ld) GARBAGE; rows differ in their mean (+ m 1e-3: a transpose is not a symmetry)."""
    A = _garbage(rs, (nz, taps, K, a_ld))
    A[..., :M] = rs.standard_normal((nz, taps, K, M)) / math.sqrt(K * taps) + np.arange(M) * 1e-3
    return A


def _xin(rs, shape, T):
    x = _garbage(rs, shape)
    x[..., :T] = rs.standard_normal(shape[:-1] + (T,))
    return x


@functools.lru_cache(maxsize=None)
def conv_case(config, N, variant=0):
    """One launch of the generic kernel.  -> dict(a: the ConvArgs scalars, out: the two ConvOut blocks (buffers by name), bufs: name -> float32 /
    int64 array (the outputs' contents BEFORE the launch), epi, nbatch).  variant 1: Tin = N - 3 < N,
    split: accum = 1 on out[1]."""
    assert config in CONV_CONFIGS
    rs = np.random.RandomState(4100 + 17 * CONV_CONFIGS.index(config) + N + 1000 * variant)
    B = 2
    ld = ceil4(N)
    Tin = max(N - (3 if variant else 0), 1)
    a = dict(N=N, Tin=Tin, dil=1, zdiv=1, a_zs0=0, a_zs1=0, x_zs1=0, pre_div=1.0, pre_slope=1.0, split=INT_MAX, ldx=ld)
    o0, o1 = dict(OUT_DEFAULTS), dict(OUT_DEFAULTS)
    bufs, epi, nbatch = {}, EPI_PLAIN, B

    def shape(M, K, taps, a_ld=None):
        a_ld = a_ld or ceil4(M)
        a.update(M=M, K=K, taps=taps, pad=(taps - 1) * abs(a["dil"]) // 2, a_ld=a_ld, a_cols=a_ld, a_tap_stride=K * a_ld, x_zs0=K * ld)
        bufs["A"] = _kmajor_weights(rs, taps, K, M, a_ld)
        bufs["X"] = _xin(rs, (B, K, ld), Tin)
        bufs["bias"] = rs.standard_normal(M).astype(np.float32)

    def plain_out(o, name, rows):
        bufs[name] = np.full((B, rows, ld), SENTINEL, np.float32)
        o.update(Y=name, y_zs0=rows * ld, ldy=ld, Tout=N, bias="bias")

    if config == "gated":          # the denoiser block's gated conv: 64-row groups [32 gate | 32 filter] -> M / 2 rows
        shape(128, 64, 3)
        epi = EPI_GATED
        plain_out(o0, "Y0", 64)
    elif config == "split":        # the residual / skip projection: out[0] rows 0 .. 127 with residual, per-batch vector and 1 / sqrt(2); out[1] rows 128 .. 255
        shape(256, 128, 1)
        a["split"] = 128
        plain_out(o0, "Y0", 128)
        plain_out(o1, "Y1", 128)
        bufs["R"] = _xin(rs, (B, 128, ld), N)
        bufs["bvec"] = rs.standard_normal((B, 256)).astype(np.float32)
        o0.update(res="R", r_zs0=128 * ld, ldr=ld, bvec="bvec", bvec_zs=256, rmul=float(np.float32(math.sqrt(0.5))))
        o1.update(row_off=128, accum=variant)
        if variant:
            bufs["Y1"] = _xin(rs, (B, 128, ld), ld)
    elif config == "kc64":         # the FFN linear's K segments: zdiv = 8 with the second batch strides
        a.update(zdiv=8)
        shape(96, 128, 1)
        bufs["A"] = _kmajor_weights(rs, 1, 128, 96, 96, 8)
        bufs["X"] = _xin(rs, (B, 8 * 128, ld), Tin)
        a.update(a_zs0=0, a_zs1=128 * 96, x_zs0=8 * 128 * ld, x_zs1=128 * ld)
        bufs["Y0"] = np.full((B, 8, 96, ld), SENTINEL, np.float32)
        o0.update(Y="Y0", y_zs0=8 * 96 * ld, y_zs1=96 * ld, ldy=ld, Tout=N, bias="bias")
        nbatch = B * 8
    elif config == "tb5":          # the FFN conv: nine taps, a ragged last chunk, GELU with k^-1/2, the length mask
        shape(96, 40, 9)
        plain_out(o0, "Y0", 96)
        bufs["lens"] = np.asarray([N, max(int(0.6 * N), 1)], np.int64)
        o0.update(alpha=TC.FFN_ALPHA, act=ACT_GELU_ERF, lens="lens")
    elif config == "plain64":      # the skip head's form: pre_div with ReLU
        shape(256, 80, 1)
        plain_out(o0, "Y0", 256)
        a["pre_div"] = float(np.float32(math.sqrt(20.0)))
        o0.update(act=ACT_RELU)
    elif config == "t64x256":      # a dilated ResBlock conv with its LeakyReLU on load
        a["dil"] = 5
        shape(33, 20, 3, 36)
        plain_out(o0, "Y0", 33)
        a["pre_slope"] = float(np.float32(0.1))
    elif config == "t32x256":
        shape(11, 128, 5, 12)
        plain_out(o0, "Y0", 11)
        o0.update(act=ACT_TANH)
    elif config == "shortm":       # few rows and few columns: division and the length mask
        shape(40, 128, 1)
        plain_out(o0, "Y0", 40)
        bufs["lens"] = np.asarray([max(int(0.6 * N), 1), N], np.int64)
        o0.update(div=3.0, lens="lens")
    else:                          # convT: ConvTranspose1d(32 -> 16, kernel 8, stride 4) as vocoder.hip's four polyphase launches-in-one (z = utterance x phase)
        st, KT, Cin, Cout = 4, 8, 32, 16
        Ti = N - 1                                                     # the launch computes Ti + 1 columns per phase
        assert Ti >= 1 and not variant
        w = (rs.standard_normal((Cin, Cout, KT)) / math.sqrt(Cin * 2) + np.arange(Cout)[None, :, None] * 1e-3).astype(np.float32)
        A = np.zeros((st, KT // st, Cin, Cout), np.float32)            # import.hip: pack_conv_transpose — phase r uses taps k = r + st q
        for r in range(st):
            for q in range(KT // st):
                A[r, q] = w[:, :, r + st * q]
        To = Ti * st
        a.update(M=Cout, K=Cin, taps=KT // st, dil=-1, pad=0, Tin=Ti, a_ld=Cout, a_cols=Cout, a_tap_stride=Cin * Cout, ldx=Ti, zdiv=st, a_zs0=0,
                 a_zs1=(KT // st) * Cin * Cout, x_zs0=Cin * Ti, x_zs1=0, pre_div=3.0, pre_slope=float(np.float32(0.1)))
        bufs.update(A=A, X=rs.standard_normal((B, Cin, Ti)).astype(np.float32), bias=rs.standard_normal(Cout).astype(np.float32), W=w,
                    Y0=np.full((B, Cout, To), SENTINEL, np.float32))
        o0.update(Y="Y0", y_zs0=Cout * To, y_zs1=0, ldy=To, Tout=To, ostride=st, ooff_base=-((KT - st) // 2), ooff_mul=1, bias="bias")
        nbatch = B * st
    if config != "split":
        o1 = dict(o0)
    _ro(*bufs.values())
    return {"config": config, "a": a, "out": (o0, o1), "bufs": bufs, "epi": epi, "nbatch": nbatch, "_memo": {}}


def _act(v, act, dtype):
    if act == ACT_RELU:
        return np.maximum(v, 0)
    if act == ACT_GELU_ERF:
        return TC.gelu(v.astype(dtype))
    if act == ACT_TANH:
        return np.tanh(v)
    return v


def conv_def(case, dtype, swap_gate=False, ignore_row_off=False, phase_shift=0):
    """Y[z][m][t_out] = epilogue(sum_{tap, k} A[z][tap][k][m] pre(X[z][k][n + tap dil - pad])) (conv_args.h), the epilogue in conv_epilogue.h's
    order: + bias, x alpha, activation, + residual + per-batch vector, / div, x rmul, + old Y (accum), length mask; t_out = n ostride +
    ooff_base + (z % zdiv) ooff_mul, stored where 0 <= t_out < Tout and n < N.  Gated: per 64-row group [32 gate | 32 filter] ->
    sigmoid(g) tanh(f) in M / 2 rows.  Addresses are formed on the flat buffers exactly as the kernel forms them.
    -> (name -> flat array in dtype after the launch, name -> bool mask of the written elements).
    swap_gate / ignore_row_off / phase_shift: the CPU test's mutants."""
    c, a, bufs = case, case["a"], case["bufs"]
    M, N, K, taps = a["M"], a["N"], a["K"], a["taps"]
    A, X = bufs["A"].reshape(-1), bufs["X"].reshape(-1)
    ys = {o["Y"]: bufs[o["Y"]].reshape(-1).astype(dtype) for o in c["out"]}
    wr = {k: np.zeros(v.shape, bool) for k, v in ys.items()}
    n = np.arange(N)
    for z in range(c["nbatch"]):
        zq, zr = divmod(z, a["zdiv"])
        a0, x0 = zq * a["a_zs0"] + zr * a["a_zs1"], zq * a["x_zs0"] + zr * a["x_zs1"]
        Xz = X[x0:x0 + (K - 1) * a["ldx"] + a["Tin"]]
        Xz = np.stack([Xz[k * a["ldx"]:k * a["ldx"] + a["Tin"]] for k in range(K)]).astype(dtype)
        Xz = Xz / dtype(np.float32(a["pre_div"])) if a["pre_div"] != 1.0 else Xz
        Xz = np.where(Xz > 0, Xz, Xz * dtype(np.float32(a["pre_slope"]))).astype(dtype)
        acc = np.zeros((M, N), dtype)
        for tap in range(taps):
            At = A[a0 + tap * a["a_tap_stride"]:a0 + tap * a["a_tap_stride"] + K * a["a_ld"]].reshape(K, a["a_ld"])[:, :M].astype(dtype)
            t_in = n + tap * a["dil"] - a["pad"]
            ok = (t_in >= 0) & (t_in < a["Tin"])
            acc += At.T @ np.where(ok[None, :], Xz[:, np.clip(t_in, 0, a["Tin"] - 1)], 0).astype(dtype)
        if c["epi"] == EPI_GATED:
            o = c["out"][0]
            v = (acc + bufs[o["bias"]].astype(dtype)[:, None]).reshape(M // 64, 2, 32, N)
            g, f = (v[:, 1], v[:, 0]) if swap_gate else (v[:, 0], v[:, 1])
            y = ((dtype(1) / (dtype(1) + np.exp(-g))) * np.tanh(f)).reshape(M // 2, N).astype(dtype)
            rows, cols = np.arange(M // 2), n[n < o["Tout"]]
            idx = (zq * o["y_zs0"] + zr * o["y_zs1"] + rows[:, None] * o["ldy"] + cols[None, :])
            ys[o["Y"]][idx] = y[:, :len(cols)]
            wr[o["Y"]][idx] = True
            continue
        for oi, (m_lo, m_hi) in enumerate(((0, min(M, a["split"])), (min(M, a["split"]), M))):
            if m_hi <= m_lo:
                continue
            o = c["out"][oi]
            m = np.arange(m_lo, m_hi)
            v = acc[m_lo:m_hi]
            if o["bias"] is not None:
                v = v + bufs[o["bias"]].astype(dtype)[m, None]
            v = _act(v * dtype(np.float32(o["alpha"])), o["act"], dtype)
            t = n * o["ostride"] + o["ooff_base"] + zr * o["ooff_mul"] + phase_shift
            okt = (t >= 0) & (t < o["Tout"])
            tc = np.clip(t, 0, o["Tout"] - 1)
            if ignore_row_off and o["row_off"]:
                continue          # the mutant's stores land row_off rows further on, beyond this buffer: it keeps what it held
            row = m - o["row_off"]
            if o["res"] is not None:
                R = bufs[o["res"]].reshape(-1)
                v = v + R[zq * o["r_zs0"] + zr * o["r_zs1"] + row[:, None] * o["ldr"] + tc[None, :]].astype(dtype)
            if o["bvec"] is not None:
                v = v + bufs[o["bvec"]].reshape(-1)[zq * o["bvec_zs"] + m].astype(dtype)[:, None]
            if o["div"] != 1.0:
                v = v / dtype(np.float32(o["div"]))
            if o["rmul"] != 0.0:
                v = v * dtype(np.float32(o["rmul"]))
            idx = zq * o["y_zs0"] + zr * o["y_zs1"] + row[:, None] * o["ldy"] + tc[None, :]
            if o["accum"]:
                v = v + ys[o["Y"]][idx]
            if o["lens"] is not None:
                v = np.where((t >= bufs[o["lens"]][zq])[None, :], 0, v)
            ys[o["Y"]][idx[:, okt]] = v[:, okt].astype(dtype)
            wr[o["Y"]][idx[:, okt]] = True
    return ys, wr


def conv_transpose_def(case, dtype):
    """ConvTranspose1d(stride 4, padding (K - stride) / 2)(leaky_relu(x / 3, 0.1)) + b of the convT case, directly -> [B][Cout][Ti 4]."""
    b = case["bufs"]
    x = b["X"].astype(dtype) / dtype(3.0)
    x = np.where(x > 0, x, x * dtype(np.float32(0.1))).astype(dtype)
    w = b["W"].astype(dtype)
    Bn, Cin, Ti = x.shape
    KT, st, p = w.shape[2], 4, 2
    full = np.zeros((Bn, w.shape[1], (Ti - 1) * st + KT), dtype)
    for k in range(KT):
        full[:, :, k:k + (Ti - 1) * st + 1:st] += np.einsum("io,bit->bot", w[:, :, k], x)
    return (full[:, :, p:full.shape[2] - p] + b["bias"].astype(dtype)[None, :, None]).astype(dtype)


def check_conv(got, case):
    """got: name -> float32 array, the output buffers after the launch.  Nothing outside the definition's footprint was written; the written
    elements by ratio against float64 (d32: the definition in float32); convT also against the float64 transposed conv."""
    c = case
    (y64, wr), (y32, _) = _memo(c, "c64", lambda: conv_def(c, np.float64)), _memo(c, "c32", lambda: conv_def(c, np.float32))
    r = Ratio(0.0)
    for name, ref in y64.items():
        g = np.asarray(got[name]).reshape(-1)
        w = wr[name]
        exact("conv_generic", g[~w], c["bufs"][name].reshape(-1)[~w], (c["config"], name, "written outside the launch's footprint"))
        if w.any():
            r = worst(r, ratio_check("conv_generic", g[w], ref[w], yardstick(ref[w], y32[name][w]), (c["config"], c["a"]["N"], name)))
    if c["config"] == "convT":
        ref = conv_transpose_def(c, np.float64)
        assert wr["Y0"].all()
        r = worst(r, ratio_check("conv_generic", np.asarray(got["Y0"]).reshape(ref.shape), ref, yardstick(ref, conv_transpose_def(c, np.float32)), "convT vs transposed conv"))
    return r
