"""Instances, inputs, float64 definitions and yardsticks shared by tests/test_text16_kernel_cases_cpu.py and tests/test_gpu_text16_kernels.py
(not a test module): the opt-in 16-bit text side ("text16") — conv_xt16_kernel (cm-tts_amd/csrc/conv_xt16.hip) and the text_epi branch of
conv1d_mfma16_kernel (conv_mfma16.hip) — called ALONE through cmtts_launch_conv_xt16 / cmtts_launch_conv16.  Every reference is the definition
evaluated in float64 on the operands the kernels themselves have (x and w rounded from their fp32 value to bf16 / fp16; bias, alpha and residual
fp32); the same function evaluated in float32 is the yardstick `d32`.  No intermediate is rounded on chip, so the bound has no widening term.
Nothing here is computed from a kernel.  Computed once per (instance, N, mode) and left unchanged."""
import collections
import functools

import numpy as np

from text_kernel_cases import (ACT_GELU_ERF, ACT_NONE, FFN_ALPHA, GARBAGE, OUT_ALPHA, SENTINEL, ConvArgs, ConvOut, conv_args,  # noqa: F401
                               ffn2_weights, gelu, kmajor, xres_input, xres_lens, xres_weights, yardstick)
from vocoder_kernel_cases import M, dmax, floor4, round16  # noqa: F401

F32, F64 = np.float32, np.float64
ACT_RELU, ACT_TANH = 1, 3                        # enum ConvAct (cm-tts_amd/csrc/conv_args.h)
B = 2
MODES = {1: "bf16", 2: "fp16"}

# The launches text_side.hip makes with text_epi = 1 (qkv: self_attention, out: out_projection, ffn1: ffn_conv, ffn2: ffn_linear, pred3 / pred5:
# the predictors' convs), and `small`, which production does not make and the launcher admits: M = 64 and the ragged M = 48 on launch16<64,128,2,2>,
# where epi_tile_simple's m < M guard and the min(.., M - 1) clamp of its bias and residual loads are live.
Inst = collections.namedtuple("Inst", "K M taps seed alpha act res mask")
INSTANCES = {
    "qkv": Inst(256, 768, 1, 11, 1.0, ACT_NONE, False, False),
    "out": Inst(256, 256, 1, 12, OUT_ALPHA, ACT_NONE, True, True),
    "ffn1": Inst(256, 1024, 9, 13, FFN_ALPHA, ACT_GELU_ERF, False, False),
    "pred3": Inst(256, 256, 3, 14, 1.0, ACT_RELU, False, False),
    "pred5": Inst(256, 256, 5, 15, 1.0, ACT_RELU, False, False),
    "ffn2": Inst(1024, 256, 1, 16, 1.0, ACT_NONE, True, True),
    "small64": Inst(256, 64, 3, 17, 1.0, ACT_RELU, False, False),
    "small48": Inst(256, 48, 3, 18, 1.0, ACT_RELU, False, False),
}
XT16 = ("qkv", "out", "ffn1", "pred3", "pred5")          # K = 256 and M % 128 == 0: cmtts_launch_conv_xt16 takes them; the others it refuses

# Both sides of conv_xt16's 32-column n-tiles and 96-column workgroup tiles and of the chunked kernel's 96- and 128-column tiles
NS = (1, 31, 33, 95, 96, 97, 127, 128, 129, 130, 193)
N_EXTRA_LD = 97                                  # also with rows 8 floats longer: rows do not start where tiles do
N_ALONE = (1, 97)                                # utterance 1 alone, and the launch repeated behind one on inputs 1e4 times larger (bf16)


def round_up(n, q):
    return (n + q - 1) // q * q


def lds_of(N):
    ld = round_up(N, 4)
    return (ld, ld + 8) if N == N_EXTRA_LD else (ld,)


def chunked_tile(Mrows, N):
    """(BM, BN) of the chunked kernel's launch for a text_epi conv that conv_xt16 does not take: cmtts_launch_conv16's rule (conv_mfma16.hip:315-322)."""
    if Mrows > 64 and round_up(N, 96) < round_up(N, 128):
        return 128, 96
    return (128 if Mrows > 64 else 64 if Mrows > 32 else 32), 128


TILE_RULE_SOURCE = "a.text_epi && a.M > 64 && (a.N + 95) / 96 * 96 < (a.N + 127) / 128 * 128"      # the rule's own text in conv_mfma16.hip
N_TILE128 = (97, 127, 128, 193)                  # by the rule: these take launch16<128,128,4,1>, the rest of NS launch16<128,96,4,1>


# ----------------------------------------------------------------------------------------------------------------- inputs

@functools.lru_cache(maxsize=None)
def weights(name):
    """(w [M][K][taps] float32 in torch's layout, bias [M])."""
    I = INSTANCES[name]
    if name == "ffn2":
        w, b = ffn2_weights()[:, :, None], xres_weights(I.M, 1, I.seed)[1]
    else:
        w, b = xres_weights(I.M, I.taps, I.seed)
    assert w.shape == (I.M, I.K, I.taps) and b.shape == (I.M,)
    return w, b


def packer_input(name):
    """kmajor(w) [taps][K][round_up(M, 32)]: the fragment16 packer takes whole 32-row m-tiles; the rows beyond M are zero, as to_fragment16's header says."""
    w, _ = weights(name)
    p = kmajor(w)
    pad = round_up(p.shape[2], 32) - p.shape[2]
    return np.ascontiguousarray(np.pad(p, ((0, 0), (0, 0), (0, pad))))


@functools.lru_cache(maxsize=None)
def x_input(K, N):
    """x float32 [B][K][N], the valid columns alone (every row stride of a case has the same values; what lies around them is GARBAGE, set by the
    caller).  K = 256: text_kernel_cases.xres_input's (mean 0.3, std 1.5); K = 1024: the size of an FFN conv's GELU output."""
    if K == 256:
        x = np.ascontiguousarray(xres_input(N, round_up(N, 4))[:, :, :N])
    else:
        rs = np.random.RandomState(6000 + N)
        x = gelu((rs.standard_normal((B, K, N)) * 1.5).astype(F64)).astype(F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def residual(N):
    """[B][256][N] float32: the other utterance's x halved (text_kernel_cases' out-projection residual)."""
    r = np.ascontiguousarray(x_input(256, N)[::-1]) * F32(0.5)
    r.setflags(write=False)
    return r


def padded(v, ld, rows_around=0, fill=GARBAGE):
    """[Bn][C][N] -> [Bn + 2 rows_around][C][ld] holding `fill` behind the valid columns and in the utterances around."""
    out = np.full((v.shape[0] + 2 * rows_around, v.shape[1], ld), fill, v.dtype)
    out[rows_around:rows_around + v.shape[0], :, :v.shape[2]] = v
    return out


# ----------------------------------------------------------------------------------------------------------------- definition

def conv_taps(xq, wq, dtype, zero_halo=True, beyond=None):
    """sum_{tap, k} wq[m][k][tap] xq[k][n + tap - (taps - 1) / 2] with zeros outside [0, N) -> [M][N].  zero_halo = False (a wrong kernel): the
    columns right of N - 1 hold `beyond` [K][pad] instead of zeros."""
    Mr, K, taps = wq.shape
    N = xq.shape[1]
    pad = (taps - 1) // 2
    xp = np.zeros((K, N + 2 * pad), dtype)
    xp[:, pad:pad + N] = xq
    if not zero_halo and pad:
        xp[:, pad + N:] = beyond
    y = np.zeros((Mr, N), dtype)
    for tau in range(taps):
        y += np.ascontiguousarray(wq[:, :, tau], dtype) @ xp[:, tau:tau + N]
    return y


def activation(v, act):
    if act == ACT_GELU_ERF:
        return gelu(v)
    if act == ACT_RELU:
        return np.maximum(v, v.dtype.type(0))
    assert act == ACT_NONE
    return v


def conv16_def(x, w, b, mode, dtype, alpha=1.0, act=ACT_NONE, res=None, lens_n=None, wrong=None, wq=None):
    """One text16 launch on one utterance, x [K][N] -> [M][N], in epi_tile_simple's order (conv_epilogue.h): ((acc + b) * alpha), the activation,
    + res, columns >= lens_n set to 0; acc = the conv of round16(x) with round16(w), zero padding outside [0, N).
    wrong: one of WRONG — the same launch as a subtly wrong kernel would compute it (tests/test_text16_kernel_cases_cpu.py); wq: round16(w) in
    dtype where the caller has it already (rounding 2.4 M weights is most of a small case's time)."""
    assert wrong is None or wrong in WRONG
    xq = np.asarray(x, dtype)
    if wrong == "operands not rounded":
        wq = np.asarray(w, dtype)
    else:
        xq, wq = round16(xq, mode), round16(np.asarray(w, dtype), mode) if wq is None else wq
    if wrong == "taps reversed":
        wq = wq[:, :, ::-1]
    halo = wrong == "halo not zeroed at the right edge"
    acc = conv_taps(xq, wq, dtype, not halo, round16(np.asarray(GARBAGE, dtype), mode) if halo else None)
    v = acc + np.asarray(b, dtype)[:, None]
    if wrong == "alpha after the activation":
        v = activation(v, act) * dtype(alpha)
    else:
        v = activation((v * dtype(alpha)).astype(dtype), act)
    if res is not None:
        r = np.asarray(res, dtype)
        if wrong == "residual row stride ld + 1":      # row m read at m (ld + 1) of a buffer with rows of ld = N floats: row m shifted by m columns
            flat = np.concatenate([r.ravel(), np.full(r.shape[0], GARBAGE, dtype)])
            r = np.stack([flat[m * (r.shape[1] + 1):m * (r.shape[1] + 1) + r.shape[1]] for m in range(r.shape[0])])
        v = v + r
    if lens_n is not None:
        v = v.copy()
        v[:, int(lens_n) + (1 if wrong == "mask from lens + 1" else 0):] = 0
    return v.astype(dtype)


WRONG = ("operands not rounded", "alpha after the activation", "taps reversed", "mask from lens + 1", "residual row stride ld + 1",
         "halo not zeroed at the right edge")


@functools.lru_cache(maxsize=None)
def rounded_weights(name, mode, dtype):
    wq = round16(np.asarray(weights(name)[0], dtype), mode)
    wq.setflags(write=False)
    return wq


def instance_def(name, N, mode, dtype, wrong=None):
    """The instance's launch on its inputs at N -> [B][M][N]."""
    I = INSTANCES[name]
    w, b = weights(name)
    wq = rounded_weights(name, mode, dtype)
    x, lens = x_input(I.K, N), xres_lens(N)
    res = residual(N) if I.res else None
    return np.stack([conv16_def(x[i], w, b, mode, dtype, I.alpha, I.act, None if res is None else res[i], lens[i] if I.mask else None, wrong, wq)
                     for i in range(B)])


@functools.lru_cache(maxsize=None)
def _eval(name, N, mode):
    ref = instance_def(name, N, mode, F64)
    d32 = dmax(ref, instance_def(name, N, mode, F32))
    ref.setflags(write=False)
    return ref, d32


def reference(name, N, mode):
    """-> (ref float64 [B][M][N], yard = max(d32 of the case, d32 of the instance at its largest N, 4 float32 ulps of the output))."""
    ref, d32 = _eval(name, N, mode)
    return ref, max(d32, _eval(name, max(NS), mode)[1], floor4(ref))


def decode_fragment16(stream, taps, K, Mrows, mode):
    """The fragment16 stream [taps][K/16][M/32][64 lanes][8] of uint16 (weight_pack.cpp: to_fragment16) -> float32 [taps][K][M]: element (lane, j) is
    P[tap][16 g + 8 (lane >> 5) + j][32 mt + (lane & 31)]."""
    u = np.ascontiguousarray(stream).view(np.uint16).reshape(taps, K // 16, Mrows // 32, 64, 8)
    v = (u.astype(np.uint32) << np.uint32(16)).view(F32) if mode == 1 else u.view(np.float16).astype(F32)
    out = np.empty((taps, K, Mrows), F32)
    t, g, mt, l, j = np.meshgrid(*[np.arange(n) for n in u.shape], indexing="ij", sparse=True)
    out[t, 16 * g + 8 * (l >> 5) + j, 32 * mt + (l & 31)] = v
    return out
