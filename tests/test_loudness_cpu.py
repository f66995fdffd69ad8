"""Loudness measurement, CPU side: the numpy definition (cmtts_amd/loudness.py) against the ITU-R BS.1770-4 coefficient table and the
reference levels, the gates, the edge cases and gain_for; the host-only coefficient entry point (csrc/loudness_coef.cpp) against the
definition; argument validation of the device entry points, which rejects before anything touches the GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import loudness as ld
from loudness_cases import BLOCK, FS, HOP, gate_margin, reference, signal, weighted

# ITU-R BS.1770-4, table 1 and table 2 (48 kHz): b0 b1 b2 a1 a2
BS1770_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
BS1770_HIGHPASS = (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def _sine(fs, seconds=3.0, f=997.0, amp=1.0):
    return (amp * np.sin(2 * np.pi * f * np.arange(int(seconds * fs)) / fs)).astype(np.float32)


def test_k_weighting_is_the_bs1770_table_at_48k():
    s1, s2 = ld.k_weighting(48000)
    np.testing.assert_allclose(s1, BS1770_SHELF, rtol=0, atol=1e-12)
    np.testing.assert_allclose(s2, BS1770_HIGHPASS, rtol=0, atol=1e-12)


@pytest.mark.parametrize("fs", [22050, 24000, 48000])
def test_coefficient_entry_point_matches_the_definition(fs):
    lib = _lib.load()
    out = (C.c_double * 10)()
    assert lib.cmtts_loudness_coefficients(fs, out) == 0
    s1, s2 = ld.k_weighting(fs)
    np.testing.assert_allclose(list(out), list(s1) + list(s2), rtol=0, atol=1e-12)


def test_coefficient_entry_point_rejects():
    lib = _lib.load()
    out = (C.c_double * 10)()
    assert lib.cmtts_loudness_coefficients(22055, out) == -1 and b"multiple of 10" in lib.cmtts_last_error()
    assert lib.cmtts_loudness_coefficients(4000, out) == -1
    assert lib.cmtts_loudness_coefficients(48010, out) == -1
    assert lib.cmtts_loudness_coefficients(48000, None) == -1


def test_reference_levels():
    """A full-scale 997 Hz sine: -3.01 LKFS at 48 kHz (BS.1770's nominal figure); the same definition at 22 050 Hz gives -2.981."""
    L48, nb, ng = ld.integrated_loudness(_sine(48000), 48000)
    assert abs(L48 - (-3.01)) <= 0.01 and nb == ng == 27
    L22, nb, ng = ld.integrated_loudness(_sine(22050), 22050)
    assert abs(L22 - (-2.981)) <= 0.001 and nb == ng == 27


def test_gating():
    """1 s at -20, 1 s at -36, 1 s at -80 dBFS: 27 blocks, 20 pass the absolute gate, 10 pass both; skipping a gate gives another L."""
    y = weighted("gating", np.float64)
    z, l = ld.block_loudness(y, FS)
    assert len(z) == 27 and int((l > ld.ABSOLUTE_GATE).sum()) == 20
    L, nb, ng = reference("gating", len(y))
    assert (nb, ng) == (27, 10)
    assert abs(L - (-23.67)) <= 0.005
    assert abs(ld._lk(float(np.mean(y * y))) - (-27.64)) <= 0.005                   # the mean square of the whole signal: no gate at all
    assert abs(ld._lk(float(np.mean(z[l > ld.ABSOLUTE_GATE]))) - L) > 1.0          # the absolute gate alone
    assert float(np.min(np.abs(l - ld.ABSOLUTE_GATE))) >= 8.9
    assert gate_margin("gating", len(y)) >= 2.39          # 2.398 LU: the block nearest to the relative gate
    assert reference("gating", len(y)) == ld.integrated_loudness(signal("gating"), FS)


def test_edge_cases():
    x = signal("modulated")
    assert ld.integrated_loudness(x[:0], FS) == (-math.inf, 0, 0)
    # one sample: one block [0, 1), y[0] = b0 x[0]
    L1, nb, ng = ld.integrated_loudness(x[:1], FS)
    b0 = ld.k_weighting(FS)[0][0]
    assert (nb, ng) == (1, 1) and abs(L1 - (ld.OFFSET + 20 * math.log10(abs(b0 * float(x[0]))))) < 1e-9
    # just under one block: one block [0, n), the mean over n samples
    y = weighted("modulated", np.float64)
    L, nb, ng = ld.integrated_loudness(x[:BLOCK - 1], FS)
    assert (nb, ng) == (1, 1) and abs(L - (ld.OFFSET + 10 * math.log10(float(np.mean(y[:BLOCK - 1] ** 2))))) < 1e-9
    assert ld.integrated_loudness(x[:BLOCK], FS)[1:] == (1, 1)
    assert ld.integrated_loudness(x[:BLOCK + HOP - 1], FS)[1:] == (1, 1)           # the second block is not wholly inside
    assert ld.integrated_loudness(x[:BLOCK + HOP], FS)[1:] == (2, 2)
    # silence, and a level under the absolute gate
    assert ld.integrated_loudness(np.zeros(FS, np.float32), FS) == (-math.inf, 7, 0)
    assert ld.integrated_loudness(np.zeros(100, np.float32), FS) == (-math.inf, 1, 0)
    assert ld.integrated_loudness(_sine(FS, 1.0, amp=10 ** (-80 / 20)), FS) == (-math.inf, 7, 0)
    with pytest.raises(ValueError):
        ld.integrated_loudness(x[:100], 22055)
    # the float32 evaluation is the same recurrence: close to, and not identical with, the float64 one
    d = abs(ld.integrated_loudness(x, FS, np.float32)[0] - ld.integrated_loudness(x, FS)[0])
    assert 0 < d < 1e-3
    assert ld.sample_peak(x[:0]) == 0.0 and ld.sample_peak(np.array([0.1, -0.7, 0.3], np.float32)) == float(np.float32(0.7))


def test_gain_for():
    assert ld.gain_for(-20.0, 0.1, -23.0) == pytest.approx(10 ** (-3 / 20), rel=1e-15)
    assert ld.gain_for(-30.0, 0.1, -16.0, -1.0) == pytest.approx(10 ** (14 / 20), rel=1e-15)          # peak 0.5: under the ceiling
    assert ld.gain_for(-30.0, 0.5, -16.0, -1.0) == pytest.approx(10 ** (-1 / 20) / 0.5, rel=1e-15)    # the ceiling takes over
    assert ld.gain_for(-30.0, 0.5, -16.0, 6.0) == pytest.approx(10 ** (6 / 20) / 0.5, rel=1e-15)
    assert ld.gain_for(-math.inf, 0.5, -16.0) == 1.0
    assert ld.gain_for(-30.0, 0.5, math.nan) == 1.0
    assert ld.gain_for(-30.0, 0.0, -16.0) == 1.0
    x = signal("modulated")[:1000]
    g = ld.gain_for(-14.0, 0.5, -23.0)
    assert np.array_equal(ld.apply_gain(x, g), np.float32(g) * x) and ld.apply_gain(x, g).dtype == np.float32


def test_argument_validation_without_a_gpu():
    """Null pointers, a bad rate and a short workspace are refused before the pointers are looked at: the addresses below are not memory."""
    lib = _lib.load()
    P = 4096          # a non-null address that is never dereferenced
    rows, n = 2, 3 * FS
    nb = lib.cmtts_loudness_workspace_bytes(rows, n, FS)
    assert nb == 2 * rows * 30 * 4
    assert lib.cmtts_loudness_workspace_bytes(rows, n + 1, FS) == 2 * rows * 31 * 4
    assert lib.cmtts_loudness_workspace_bytes(0, n, FS) == 0 and lib.cmtts_loudness_workspace_bytes(rows, n, 22055) == 0

    def measure(wav=P, rows_c=rows, ld_c=n, nv=P, fs=FS, tgt=None, ceil=-1.0, stats=P, ws=P, wsb=nb):
        return lib.cmtts_loudness_measure(wav, rows_c, ld_c, nv, fs, tgt, ceil, stats, ws, wsb, None)

    bad = {"null wav": measure(wav=None), "null n_valid": measure(nv=None), "null stats": measure(stats=None), "null ws": measure(ws=None),
           "rows 0": measure(rows_c=0), "ld 0": measure(ld_c=0), "fs 22055": measure(fs=22055), "fs 4000": measure(fs=4000),
           "fs 96000": measure(fs=96000), "NaN ceiling": measure(ceil=math.nan), "short workspace": measure(wsb=nb - 1),
           "no workspace": measure(wsb=0)}
    for what, rc in bad.items():
        assert rc == -1, what
    assert b"workspace too small" in lib.cmtts_last_error()
    assert measure(wav=None) == -1 and b"null" in lib.cmtts_last_error()

    def encode(r=P, wav=P, seg=P, out=P, gains=P):
        return lib.cmtts_resample_encode_gain(r, wav, 1, 100, seg, 1, 0, 32768.0, out, 100, gains, None)

    for what, rc in {"null resampler": encode(r=None), "null wav": encode(wav=None), "null table": encode(seg=None),
                     "null out": encode(out=None)}.items():
        assert rc == -1, what
    assert b"cmtts_resample_encode_gain" in lib.cmtts_last_error()
