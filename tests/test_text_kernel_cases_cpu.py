"""CPU checks of tests/text_kernel_cases.py: the float64 definitions ARE the reference's operations, the attention cases have the
properties tests/test_gpu_text_kernels.py relies on, and the expected-flip-rate formula predicts an observed count."""
import numpy as np
import pytest

from oracle import cmtts_oracle as O
from oracle import winograd_ref as W
import text_kernel_cases as TC


def test_attention_definition_is_the_oracles():
    """attention_def in float64 == O.multihead_self_attention under O.precision("f64") (identity projections, so that the oracle's q, k, v
    are the inputs) on a ragged two-utterance input, to 1e-12 relative."""
    rs = np.random.RandomState(3)
    B, L, Cc, H = 2, 37, 256, 2
    lens = np.asarray([37, 21], np.int64)
    qkv = rs.standard_normal((B, 3 * Cc, L))
    # the oracle projects x [B][L][C] with in_w [3C][C]: x = the first C channels of a random input, in_w = three random maps; q, k, v for
    # the definition are those projections (float64), out_w = identity
    x = rs.standard_normal((B, L, Cc))
    in_w = rs.standard_normal((3 * Cc, Cc)) / 16.0
    with O.precision("f64"):
        ref = O.multihead_self_attention(x, in_w, np.eye(Cc), np.arange(L)[None, :] >= lens[:, None], H)      # [B][L][C]
    qkv = np.einsum("oc,blc->bol", in_w, x)
    got = TC.attention_def(qkv, lens, L, np.float64, n_heads=H).transpose(0, 2, 1)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # a row without a valid key is all zeros
    assert not TC.attention_def(qkv, np.asarray([0, 5]), L, np.float64, n_heads=H)[0].any()


def _heads(L, ld, case, zero_row=False):
    qkv, lens = TC.attn_input(L, ld, case, zero_row)
    for b in range(TC.ATTN_B):
        for h in range(TC.ATTN_H):
            q = qkv[b, h * TC.DH:(h + 1) * TC.DH, :L]
            k = qkv[b, (TC.ATTN_H + h) * TC.DH:(TC.ATTN_H + h + 1) * TC.DH, :L]
            yield int(min(lens[b], L)), TC.attn_scores(q, k)


def test_attention_lens_fall_inside_tiles():
    for L in TC.ATTN_L_SHORT + TC.ATTN_L_LONG:
        lens = TC.attn_lens(L)
        assert lens[0] == L and lens[2] == 1 and 1 <= lens[1] <= L
        if L > 2:
            assert lens[1] % 32 != 0 and lens[1] < L
        if L > 192:
            assert lens[1] % 64 != 0 and (lens[1] // 64 + 2) * 64 <= L       # a ragged chunk, and a whole chunk of padded keys beyond it
        assert TC.attn_lens(L, zero_row=True)[2] == 0
        for ld in TC.attn_lds(L):
            assert ld % 4 == 0 and ld >= L
    assert TC.attn_lds(33) == (36, 44) and TC.attn_lds(700) == (700,)


@pytest.mark.parametrize("L", [33, 192, 257, 700])
def test_attention_garbage_keys_would_win(L):
    """In every case, a padded key column (+4 Qbar) would have the largest score of its query if it were not masked; V there is +-100 and
    everything is finite."""
    for case in TC.ATTN_CASES:
        qkv, _ = TC.attn_input(L, TC.attn_lds(L)[-1], case)
        assert np.isfinite(qkv).all()
        seen = 0
        for n, s in _heads(L, TC.attn_lds(L)[-1], case):
            if n < L:
                assert (s[n:].min(0) > s[:n].max(0)).all(), (case, n)
                seen += 1
        assert seen == 2 * TC.ATTN_H
        assert (np.abs(qkv[1, 2 * TC.ATTN_H * TC.DH:, int(TC.attn_lens(L)[1]):L]) == 100.0).all()
        assert (np.abs(qkv[:, :, L:]) == TC.GARBAGE).all()


@pytest.mark.parametrize("L", TC.ATTN_L_LONG)
def test_attention_score_regimes(L):
    ld = TC.attn_lds(L)[0]
    top = {c: max(float(s[:n].max()) for n, s in _heads(L, ld, c)) for c in TC.ATTN_CASES}
    assert top["overflow"] > 89.0                      # expf(s) without the max subtraction is inf
    assert top["unit"] < 8.0
    assert top["flat"] == 0.0
    for case, first in (("peaky", False), ("first", True)):
        for n, s in _heads(L, ld, case):
            if n == 1:
                continue
            v = s[:n]
            spread = v.max(0) - v.min(0)
            chunk = v.argmax(0) // TC.KEY_CHUNK
            want = 0 if first else (n - 1) // TC.KEY_CHUNK
            assert ((chunk == want) & (spread > 20.0)).mean() > 0.5, (case, n)


@pytest.mark.parametrize("L", [1, 33, 128, 192, 257, 700])
def test_attention_yardstick(L):
    """d32 > 0 in every case but `flat` (where the floor of 4 ulps takes over), and of the size fp32 attention has."""
    for case in TC.ATTN_CASES:
        ref, d32, floor = TC.attn_reference(L, TC.attn_lds(L)[0], case)
        assert np.isfinite(ref).all() and floor > 0
        if case != "flat" and L > 1:
            assert 0 < d32 < 1e-4, (case, d32)
    ref, _, _ = TC.attn_reference(L, TC.attn_lds(L)[0], "flat", True)
    assert not ref[2].any()                            # lens = 0: zeros
    qkv, lens = TC.attn_input(L, TC.attn_lds(L)[0], "flat")
    v = qkv[1, 2 * TC.ATTN_H * TC.DH:, :int(lens[1])].astype(np.float64)
    ref, _, _ = TC.attn_reference(L, TC.attn_lds(L)[0], "flat")
    assert np.abs(ref[1] - v.mean(1, keepdims=True)).max() < 1e-14


def test_winograd_restatements_equal_the_direct_conv():
    """The float64 F(2,3) / F(4,3) restatements of the k = 9 conv equal conv1d_direct (ragged pairs and quads)."""
    rs = np.random.RandomState(5)
    for N in (1, 31, 33, 130):
        x = rs.standard_normal((64, N))
        w = rs.standard_normal((32, 64, 9)) / 24.0
        ref = W.conv1d_direct(x, w, 1)
        for form in ("f23", "f43"):
            assert np.abs(TC.CONV_FORMS[form](x, w) - ref).max() < 1e-12, (form, N)


def test_xres_definitions():
    """The three launches' definitions: float32 yardsticks of the expected size, masked columns as stated."""
    N, ld = 33, 36
    x = TC.xres_input(N, ld)
    n1 = int(TC.xres_lens(N)[1])
    y = TC.qkv_def(x[1], N, np.float64, n1)
    _, b = TC.xres_weights(768, 1, 11)
    assert np.array_equal(y[:, n1:], np.broadcast_to(b.astype(np.float64)[:, None], (768, N - n1)))      # the projection of 0
    assert 0 < TC.yardstick(y, TC.qkv_def(x[1], N, np.float32, n1)) < 1e-4
    o = TC.outproj_def(x[0], x[1], N, np.float64, n1)
    assert not o[:, n1:].any() and o[:, :n1].any()
    f = TC.ffn_def(x[0], N, np.float64)
    for form in ("direct", "f23", "f43"):
        assert 0 < TC.yardstick(f, TC.ffn_def(x[0], N, np.float32, form)) < 1e-4
    assert np.abs(TC.ffn_def(x[0], N, np.float64, "f43") - f).max() < 1e-12


def test_argument_blocks_match_the_headers():
    """The ctypes mirrors have the C structs' sizes (LP64: conv_args.h / attention.h have no packing pragma)."""
    import ctypes as C
    assert C.sizeof(TC.AttnArgs) == 64
    assert C.sizeof(TC.ConvOut) == 136
    assert C.sizeof(TC.ConvArgs) == 504 and TC.ConvArgs.out.offset == 120 and TC.ConvArgs.w2frag.offset == 456 and TC.ConvArgs.text_epi.offset == 496


def test_unit_scales():
    bins = np.asarray([-1.0, 0.0, 0.5, 2.0])
    v = np.asarray([-3.0, -1.0, -0.5, 0.25, 2.0, 3.5])
    u = TC.energy_units(v, bins)
    assert np.allclose(u, [-2.0, 0.0, 0.5, 1.5, 3.0, 4.0])
    assert np.array_equal(np.ceil(u).clip(0, 4).astype(np.int64), O.bucketize(v, bins))
    assert np.allclose(TC.half_margin(np.asarray([1.5, 2.0, 2.4])), [0.0, 0.5, 0.1])
    from conftest import pitch_margin_mask
    f0 = np.asarray([0.0, 60.0, 220.0, 220.37, 1500.0])
    assert np.array_equal(TC.half_margin(TC.pitch_units(f0)) > 2e-3, pitch_margin_mask(f0, 2e-3))


def test_expected_flip_rate_predicts_the_count():
    """For an error much smaller than a bucket, the probability that an element lands in the other bucket is the mean absolute error of the
    pre-rounding value in buckets — given that the values' fractional parts are spread evenly.  Both on a 64 k-frame run (B = 128 of the flip
    test's utterances) of the float32 oracle against the float64 oracle, LibriTTS pitch frames: the count the formula predicts against the
    observed one within a factor 3 (counts below one compare as one), and the even spread (frames within 2e-3 of a boundary: 4e-3 of all)."""
    B = 128
    st = TC.flip_stats("LibriTTS", TC.flip_oracle("LibriTTS", "f32", B), B)["pitch"]
    expected = st["rate"] * st["of"]
    assert st["of"] > 32000 and st["max_step"] <= 1 and st["max_err"] < 2e-3
    assert max(expected, 1.0) / 3.0 <= max(st["n"], 1) <= 3.0 * max(expected, 1.0), (st["n"], expected)
    near = int((st["margins"] < 2e-3).sum())
    assert 4e-3 * st["of"] / 1.5 <= near <= 4e-3 * st["of"] * 1.5, (near, st["of"])
