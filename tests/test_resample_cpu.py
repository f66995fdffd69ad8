"""cmtts_amd/resample.py, the definition the resampling kernel is tested against: taps, the formula against
scipy.signal.upfirdn, pieces that concatenate to the whole exactly, G.711 on all 65 536 inputs, the saturating cast, and the fp32
yardstick that justifies the GPU test's cap on 1-LSB differences."""
import numpy as np
import pytest

from cmtts_amd import resample as rs
from resample_cases import RATES, filt, reference, waves

EXPECTED = {8000: (160, 441, 47), 16000: (320, 441, 24), 24000: (160, 147, 17), 44100: (2, 1, 17), 48000: (320, 147, 17)}


@pytest.mark.parametrize("rate", RATES)
def test_taps(rate):
    L, M, taps, half, R = filt(rate)
    assert (L, M, R) == EXPECTED[rate] and rs.ratio(22050, rate) == (L, M)
    assert taps.dtype == np.float32 and len(taps) == 2 * half + 1
    assert np.array_equal(taps, taps[::-1])
    tab = rs.phase_table(taps, L)
    assert tab.shape == (L, 2 * R + 1) and tab.dtype == np.float32
    assert np.abs(tab.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-3          # every phase has unit DC gain
    # row p, column d + R is h[p - d L + half]
    for p, d in ((0, 0), (L - 1, -R), (L // 2, R), (1 % L, 1)):
        i = p - d * L + half
        assert tab[p, d + R] == (taps[i] if 0 <= i <= 2 * half else 0)


def test_rates_refused():
    assert rs.ratio(22050, 32000) == (640, 441) and rs.half_width(640, rs.design_taps(640, 441)[1]) == 17      # fits the tap storage
    with pytest.raises(ValueError, match="more than one frame"):
        rs.design_taps(*rs.ratio(22050, 1000))          # 20 / 441: R = 372 > hop
    with pytest.raises(ValueError, match="tap table"):
        rs.design_taps(*rs.ratio(22050, 47999))         # L = 47999
    with pytest.raises(ValueError):
        rs.ratio(22050, 0)


@pytest.mark.parametrize("rate", RATES)
def test_definition_equals_upfirdn(rate):
    from scipy.signal import upfirdn
    L, M, taps, half, _ = filt(rate)
    x = np.random.RandomState(1).standard_normal(3000).astype(np.float32)
    y = rs.resample(x, L, M, taps)
    ref = upfirdn(taps.astype(np.float64), x.astype(np.float64), up=L)[half::M]
    assert len(y) == rs.out_len(3000, L, M) and len(ref) >= len(y)
    assert np.abs(y - ref[: len(y)]).max() <= 1e-12


@pytest.mark.parametrize("rate", RATES)
def test_pieces_concatenate_exactly(rate):
    L, M, taps, half, R = filt(rate)
    n = 1400
    x = np.random.RandomState(2).standard_normal(n).astype(np.float32)
    whole = rs.resample(x, L, M, taps)
    # boundaries that are no multiples of 4 or of the hop; [130, 131) has an empty output range when down-sampling, [131, 131) always;
    # [131, 131 + R - 1) is shorter than R
    cuts = [0, 3, 130, 131, 131, 131 + R - 1, 515, 1023, n]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    plan = rs.plan_segments(pieces, n, L, M, half)
    assert any(m0 == m1 for m0, m1, _, _ in plan) and plan[0][0] == 0 and plan[-1][1] == len(whole)
    got = []
    for (s0, s1), (m0, m1, lo, hi) in zip(pieces, plan):
        assert lo == max(s0 - R, 0) and hi == min(s1 + R, n)
        got.append(rs.resample(x[lo:hi], L, M, taps, m0=m0, m1=m1, origin=lo, n=n))          # only the samples the plan asks for
    assert [p[1] for p in plan[:-1]] == [p[0] for p in plan[1:]]
    assert np.array_equal(np.concatenate(got), whole)
    with pytest.raises(ValueError):                                                           # a piece handed over without its left margin
        (s0, _), (m0, m1, lo, hi) = pieces[-2], plan[-2]
        rs.resample(x[s0:hi], L, M, taps, m0=m0, m1=m1, origin=s0, n=n)


def test_g711_all_inputs():
    s = np.arange(-32768, 32768).astype(np.int16)
    codes = np.arange(256)
    for enc, dec, name in ((rs.lin2ulaw, rs.ulaw2lin, "mulaw"), (rs.lin2alaw, rs.alaw2lin, "alaw")):
        c = enc(s)
        assert c.dtype == np.uint8
        back = dec(c).astype(np.int64)
        assert (np.diff(back) >= 0).all(), name                      # decode(encode(.)) is monotone
        lv = np.unique(dec(codes).astype(np.int64))
        # within the segment's step: the decoded value is a neighbour of the input among the 255 / 256 levels, so the error is less
        # than the gap between the two levels around the input (beyond the top level: the clip, less than the top step again)
        i = np.clip(np.searchsorted(lv, s.astype(np.int64)), 1, len(lv) - 1)
        step = lv[i] - lv[i - 1]
        assert (np.abs(back - s) <= step).all(), name
        again = enc(dec(codes))
        if name == "mulaw":      # 0x7F is mu-law's negative zero: it decodes to 0, which encodes as the positive zero 0xFF
            assert again[0x7F] == 0xFF
            again[0x7F] = 0x7F
        assert np.array_equal(again, codes), name
    try:
        import audioop
    except ImportError:
        return
    raw = s.tobytes()
    assert np.array_equal(np.frombuffer(audioop.lin2ulaw(raw, 2), np.uint8), rs.lin2ulaw(s))
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(raw, 2), np.uint8), rs.lin2alaw(s))


def test_saturating_cast():
    assert rs.to_s16(np.array([1.2, -1.2, 1.0, -1.0])).tolist() == [32767, -32768, 32767, -32768]
    # where the native cast (truncation toward zero through int32, then the low 16 bits) does not overflow: its value
    y = np.concatenate([np.linspace(-1.0, 1.0, 20001)[:-1], [0.99996, -0.99998, 3.05e-5, -3.05e-5, 0.0]]).astype(np.float32)
    native = np.trunc(y.astype(np.float32) * np.float32(32768.0)).astype(np.int64)
    assert native.min() >= -32768 and native.max() <= 32767
    assert np.array_equal(rs.to_s16(y), native.astype(np.int16))
    assert rs.encode(np.array([0.5]), "f32").dtype == np.float32 and rs.encode(np.array([0.5]), "mulaw").dtype == np.uint8
    assert np.array_equal(rs.encode(np.array([2.0, -2.0]), "alaw"), rs.lin2alaw(np.array([32767, -32768])))
    with pytest.raises(ValueError):
        rs.encode(np.zeros(1), "s24")


@pytest.mark.parametrize("rate", RATES)
def test_fp32_yardstick(rate):
    """What plain fp32 costs on the GPU test's own inputs: the sum restated sequentially in float32 (one rounding per product and per
    addition) against the float64 definition, both cast to s16 — at most 1 LSB apart on at most 0.5 % of samples, half the cap the
    GPU test sets as a condition."""
    L, M, taps, half, _ = filt(rate)
    diff = total = 0
    for x, (y, bound) in zip(waves(rate), reference(rate)):
        y32 = np.zeros(len(y), np.float32)
        for m in range(len(y)):
            lo, hi = rs.term_range(m, L, M, half)
            j = np.arange(max(lo, 0), min(hi, len(x) - 1) + 1)
            if len(j):
                y32[m] = np.cumsum(x[j] * taps[m * M - j * L + half], dtype=np.float32)[-1]
        assert (np.abs(y32 - y) <= bound).all()
        d = np.abs(rs.to_s16(y32).astype(np.int64) - rs.to_s16(y))
        assert d.max(initial=0) <= 1
        diff += int(np.count_nonzero(d))
        total += len(d)
    print(f"fp32 yardstick {rate} Hz: {diff} of {total} s16 samples differ by 1 LSB ({100.0 * diff / total:.3f} %)")
    assert diff <= 0.005 * total
