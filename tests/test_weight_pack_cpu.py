"""CPU: the host-side weight packers (cm-tts_amd/csrc/weight_pack.cpp, reached through csrc/internal_hooks.h: cmtts_internal_pack_weights) against
their numpy index expressions (oracle/winograd_ref.py: pack_weights) — BITWISE.  The plain and 16-bit layouts are permutations plus one
round-to-nearest-even; the Winograd layouts are IEEE double expressions written in the same order on both sides and rounded to float32 once.
Shapes: the smallest at which every stride of a layout is taken at least twice; normal float32 weights are all distinct, so a wrong permutation
cannot hide."""
import numpy as np
import pytest

from cmtts_amd import _lib
from oracle import winograd_ref as W

# (layout, taps, K, M, mode)
CASES = [
    ("fragment_order", 3, 16, 64, 0),
    ("fragment_iter_order", 3, 32, 64, 0),
    ("fragment16", 3, 32, 64, 1),
    ("fragment16", 3, 32, 64, 2),
    ("fragment16_split", 3, 32, 64, 0),
    ("fragment16_iter", 3, 64, 64, 1),
    ("fragment16_iter", 3, 64, 64, 2),
    ("wino_fragments", 3, 8, 64, 0),
    ("wino43_fragments", 3, 8, 128, 0),
    ("wino_iter_fragments", 3, 32, 64, 0),
    ("wino_iter_fragments", 7, 32, 64, 0),
    ("wino_iter_fragments", 11, 32, 64, 0),
    ("wino43_xres_fragments", 9, 8, 64, 0),
    ("wino23_xres_fragments", 9, 8, 64, 0),
    ("wino43_iter_fragments", 3, 8, 128, 0),
    ("wino43_iter_fragments", 5, 8, 128, 0),
    ("wino43_iter_fragments", 7, 8, 128, 0),
    ("wino43_iter_fragments", 11, 8, 128, 0),
]


def _weights(taps, K, M, seed=0):
    return np.random.RandomState(1000 * taps + K + M + seed).standard_normal((taps, K, M)).astype(np.float32)


def _packed(layout, p, mode=0):
    raw = _lib.internal_pack_weights(layout, p, mode)
    assert raw is not None, (layout, p.shape)
    return raw.view(np.uint16 if layout.startswith("fragment16") else np.float32)


@pytest.mark.parametrize("layout,taps,K,M,mode", CASES)
def test_packer_equals_numpy_layout_bitwise(layout, taps, K, M, mode):
    p = _weights(taps, K, M)
    got, ref = _packed(layout, p, mode), W.pack_weights(layout, p, mode)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), np.flatnonzero(got != ref)[:8]


def test_fp16x3_low_half_is_fragment16_of_the_residual():
    p = _weights(3, 32, 64)
    got = _packed("fragment16_split", p)
    hi = p.astype(np.float16).astype(np.float32)
    assert np.array_equal(got[:p.size], _packed("fragment16", p, 2))
    assert np.array_equal(got[p.size:], _packed("fragment16", p - hi, 2))


@pytest.mark.parametrize("layout,K,M,pad", [("wino_fragments", 8, 64, W.WINO_PAD_HG * (64 // 32) * 2 * 256),
                                            ("wino43_fragments", 8, 128, W.WINO43_PAD_KS * (128 // 64) * 6 * 256)])
def test_denoiser_layouts_end_in_zero_padding(layout, K, M, pad):
    got = _packed(layout, _weights(3, K, M))
    body = (4 if layout == "wino_fragments" else 6) * K * M
    assert got.size == body + pad
    assert not got[body:].view(np.uint32).any()          # +0.0, every bit
    assert np.count_nonzero(got[:body]) == body


def test_unknown_layout_and_uncovered_shapes_are_refused():
    p = _weights(3, 32, 64)
    assert _lib.internal_pack_weights("no_such_layout", p) is None
    assert _lib.internal_pack_weights("fragment_order", p[:, :12]) is None          # K % 8
    assert _lib.internal_pack_weights("fragment16", p, 3) is None                   # mode
    assert _lib.internal_pack_weights("wino_iter_fragments", _weights(5, 32, 64)) is None
    assert _lib.internal_pack_weights("wino43_iter_fragments", _weights(9, 8, 128)) is None
    assert _lib.internal_pack_weights("wino43_xres_fragments", p) is None           # taps = 9 only
    assert _lib.internal_pack_weights("wino43_fragments", _weights(3, 8, 96)) is None  # M % 64


@pytest.mark.parametrize("layout,taps,K,M,mode", [c for c in CASES if not c[0].startswith("fragment16")])
def test_unpack_inverts_the_layout(layout, taps, K, M, mode):
    """The inverse index map the algebra tests use (tests/test_winograd_tables.py) recovers exactly the values the stream permutes."""
    p = _weights(taps, K, M, seed=1)
    U = W.unpack_weights(layout, _packed(layout, p), taps, K, M)
    assert np.array_equal(U, W.frag_values(layout, p).transpose(0, 2, 1))
