"""CPU: what tests/test_gpu_text16_kernels.py measures the 16-bit text side's kernels against (tests/text16_kernel_cases.py) is itself right — the
float64 definitions against an independent restatement, the operand model against the weight packer, the bound against the errors a subtly wrong
kernel makes, and the shape list against cmtts_launch_conv16's tile rule."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cmtts_amd import _lib
import text16_kernel_cases as T16

F32, F64 = np.float32, np.float64


def _torch_restatement(name, N, mode):
    """torch.nn.functional.conv1d in float64 on the rounded operands, then the epilogue as text_side.hip states it (model/blocks.py: w(x) * alpha,
    activation, + residual, * nonpad) — written without text16_kernel_cases' helpers."""
    I = T16.INSTANCES[name]
    w, b = T16.weights(name)
    x = T16.x_input(I.K, N)
    to16 = (lambda t: t.to(torch.bfloat16)) if mode == 1 else (lambda t: t.to(torch.float16))
    xq, wq = to16(torch.from_numpy(np.array(x))).double(), to16(torch.from_numpy(np.array(w))).double()
    y = torch.nn.functional.conv1d(xq, wq, torch.from_numpy(np.array(b)).double(), padding=(I.taps - 1) // 2)
    y = y * float(F32(I.alpha))
    if I.act == T16.ACT_GELU_ERF:
        y = torch.nn.functional.gelu(y)
    elif I.act == T16.ACT_RELU:
        y = torch.relu(y)
    if I.res:
        y = y + torch.from_numpy(np.array(T16.residual(N))).double()
    if I.mask:
        lens = torch.from_numpy(T16.xres_lens(N))
        y = y * (torch.arange(N)[None, :] < lens[:, None])[:, None, :].double()
    return y.numpy()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(T16.INSTANCES))
def test_definitions_equal_an_independent_restatement(name, mode):
    """instance_def in float64 = torch's conv1d in float64 on torch's own bf16 / fp16 roundings of x and w, plus the epilogue, to 1e-12 relative at
    N = 33 and 97; the masked columns are exactly 0 and the yardstick has the size fp32 rounding of a K taps-term sum has."""
    for N in (33, 97):
        ref, yard = T16.reference(name, N, mode)
        want = _torch_restatement(name, N, mode)
        assert ref.dtype == F64 and ref.shape == want.shape == (T16.B, T16.INSTANCES[name].M, N)
        assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max(), (N, float(np.abs(ref - want).max()))
        if T16.INSTANCES[name].mask:
            n1 = int(T16.xres_lens(N)[1])
            assert 0 < n1 < N and not ref[1][:, n1:].any() and ref[1][:, :n1].any() and ref[0].all()
        assert T16.floor4(ref) <= yard < 2e-5, yard
        assert T16._eval(name, N, mode)[1] > 0


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(T16.INSTANCES))
def test_packed_weights_are_the_definitions_operands(name, mode):
    """The fragment16 stream the launchers are given decodes, at its one (tap, k, m) per fragment lane element, to round16(w, mode): the definition's
    operand model is the packer's conversion, bit for bit (rows beyond M: zero)."""
    I = T16.INSTANCES[name]
    p = T16.packer_input(name)
    raw = _lib.internal_pack_weights("fragment16", p, mode)
    assert raw is not None and raw.nbytes == 2 * p.size
    got = T16.decode_fragment16(raw, I.taps, I.K, p.shape[2], mode)
    want = T16.round16(T16.kmajor(T16.weights(name)[0]), mode)
    assert np.array_equal(got[:, :, :I.M].view(np.uint32), want.view(np.uint32))
    assert not got[:, :, I.M:].view(np.uint32).any()
    assert np.array_equal(T16.rounded_weights(name, mode, F64), want.transpose(2, 1, 0).astype(F64))


# (what a subtly wrong kernel does, the instance that has the operand, the factor of M yard the definition must move by: bf16, fp16).
# 100 everywhere but for the unrounded operands in fp16: fp16 keeps 11 significant bits against bf16's 8, so the same omission moves the result by
# 1 / 8 as much, and the fp16 yardstick (whose products are exact in more bits) is 1.9 x the bf16 one.  Measured there: 44.6 x M yard (out), 40.3
# (ffn1), 39.1 (qkv), against 647 / 336 / 501 in bf16 — still four times the bound, kept with 30.
WRONG_KERNELS = [("operands not rounded", "out", 100, 30), ("operands not rounded", "ffn1", 100, 30), ("alpha after the activation", "ffn1", 100, 100),
                 ("taps reversed", "ffn1", 100, 100), ("mask from lens + 1", "out", 100, 100), ("mask from lens + 1", "ffn2", 100, 100),
                 ("residual row stride ld + 1", "out", 100, 100), ("halo not zeroed at the right edge", "ffn1", 100, 100),
                 ("halo not zeroed at the right edge", "pred3", 100, 100)]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("wrong,name,f_bf16,f_fp16", WRONG_KERNELS)
def test_a_wrong_kernel_fails(wrong, name, f_bf16, f_fp16, mode):
    """Each error the whole-model criteria could pass moves the definition at N = 97 far beyond M yard."""
    ref, yard = T16.reference(name, 97, mode)
    bad = T16.instance_def(name, 97, mode, F64, wrong)
    moved = float(np.abs(bad - ref).max())
    assert moved > (f_bf16 if mode == 1 else f_fp16) * T16.M * yard, (wrong, name, moved / (T16.M * yard))


def test_every_wrong_kernel_is_tried():
    assert {w for w, *_ in WRONG_KERNELS} == set(T16.WRONG)


def test_shape_list_reaches_both_tile_widths():
    """cmtts_launch_conv16's rule for the chunked kernel (96-column tiles where they pad less than 128-column ones) sends N = 97, 127, 128 and 193 of
    the list to launch16<128,128,4,1> and the others to launch16<128,96,4,1>, each with whole and ragged tiles; the rule restated here is the text of
    conv_mfma16.hip, so a change of the rule fails this test instead of quietly emptying one arm.  Row strides: round_up(N, 4), and 8 more at N = 97."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "conv_mfma16.hip")).read()
    assert T16.TILE_RULE_SOURCE in src and "return launch16<128, 96, 4, 1>" in src and "return launch16<128, 128, 4, 1>" in src
    for Mrows in (256, 768, 1024):
        got = {N: T16.chunked_tile(Mrows, N) for N in T16.NS}
        assert {N for N, t in got.items() if t == (128, 128)} == set(T16.N_TILE128), got
        assert {N for N, t in got.items() if t == (128, 96)} == set(T16.NS) - set(T16.N_TILE128), got
    for width, Ns in ((128, T16.N_TILE128), (96, set(T16.NS) - set(T16.N_TILE128))):
        assert any(N % width == 0 for N in Ns) and any(N % width for N in Ns) and any(N > width for N in Ns), (width, Ns)
    assert all(T16.chunked_tile(64, N) == (64, 128) and T16.chunked_tile(48, N) == (64, 128) for N in T16.NS)
    assert T16.chunked_tile(32, 97) == (32, 128)
    # conv_xt16: 32-column n-tiles in 96-column workgroup tiles
    assert {31, 33, 95, 96, 97, 193} <= set(T16.NS) and set(T16.N_ALONE) <= set(T16.NS) and T16.N_EXTRA_LD in T16.NS
    for N in T16.NS:
        lds = T16.lds_of(N)
        assert lds[0] == (N + 3) // 4 * 4 and (lds[1:] == (lds[0] + 8,) if N == 97 else len(lds) == 1)
    assert set(T16.XT16) == {n for n, I in T16.INSTANCES.items() if I.K == 256 and I.M % 128 == 0}


def test_inputs():
    """What must never reach an output surrounds what may: GARBAGE behind the valid columns and in the utterances around; fp16 stays in range."""
    x = T16.x_input(256, 97)
    p = T16.padded(x, 108, 1)
    assert p.shape == (4, 256, 108) and np.array_equal(p[1:3, :, :97], x)
    assert (p[0] == T16.GARBAGE).all() and (p[3] == T16.GARBAGE).all() and (p[:, :, 97:] == T16.GARBAGE).all()
    for K in (256, 1024):
        assert np.abs(T16.x_input(K, 193)).max() < 16 and T16.x_input(K, 193).std() > 0.5
    assert C.sizeof(T16.ConvArgs) == 504 and T16.ConvArgs.text_epi.offset == 496 and T16.ConvOut.rmul.offset == 124
