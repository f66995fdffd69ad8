"""The GE2E speaker encoder without a GPU: the numpy definition (cmtts_amd/ge2e.py) against the reference's own outputs (tests/golden/ge2e.npz,
made by tests/golden/make_golden_ge2e.py), torch on the CPU and closed forms; the W_hh packer; the importer; the Python surface."""
import zlib

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd import ge2e as g2
from cmtts_amd import analysis as an
from cmtts_amd.weights import import_ge2e, synth_ge2e_state_dict
from ge2e_cases import GOLDEN, SLICE_COUNTS, clips, lstm_case, lstm_float32, reference_embeddings, torch_lstm, weights, LSTM_CASES


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---------------------------------------------------------------------------------------------------- slices

def test_partial_slices_and_padded_length_match_the_reference(golden):
    assert tuple(golden["slice_n"].tolist()) == SLICE_COUNTS
    for n, cnt, last, pad in zip(golden["slice_n"], golden["slice_count"], golden["slice_last_start"], golden["slice_pad"]):
        wave, mel = g2.partial_slices(int(n))
        assert (len(mel), mel[-1][0], g2.padded_length(int(n))) == (int(cnt), int(last), int(pad)), n
        assert all(b - a == 160 for a, b in mel) and wave == [(a * 220, b * 220) for a, b in mel]
    # the drop of the last slice flips here
    assert [len(g2.partial_slices(n)[1]) for n in (43999, 44000, 61599, 61600)] == [1, 2, 2, 3]
    assert g2.padded_length(1) == 35200 and g2.padded_length(43999) == 43999 and g2.padded_length(44000) == 52800


# ---------------------------------------------------------------------------------------------------- mel

def test_mel_power_frame_counts():
    rs = np.random.RandomState(1)
    for n, F in ((35200, 160), (35201, 161), (52800, 240), (221, 2), (220, 1), (1, 1)):
        assert g2.mel_power(rs.standard_normal(n).astype(np.float32) * 0.1).shape == (F, 40), n


def test_power_spectrum_against_torch_stft():
    rs = np.random.RandomState(2)
    x = (rs.standard_normal(5000) * 0.3).astype(np.float32)
    s = torch.stft(torch.from_numpy(x).double(), n_fft=551, hop_length=220, window=torch.hann_window(551, periodic=True, dtype=torch.float64),
                   center=True, pad_mode="reflect", return_complex=True)
    want = (s.real ** 2 + s.imag ** 2).numpy().T
    got = g2.power_spectrum(x)
    assert got.shape == want.shape == (23, 276)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * want.max())
    # the float32 arm (the contraction with the windowed table) agrees to float32 accuracy
    np.testing.assert_allclose(g2.power_spectrum(x, np.float32), want, rtol=0, atol=2e-5 * want.max())


def test_basis_closed_form_and_the_host_packer():
    b = g2.mel_basis().astype(np.float64)
    assert b.shape == (40, 276)
    f = an.mel_corners(40, 0.0, 11025.0)
    hz = np.linspace(0.0, 11025.0, 276)
    for i in range(40):
        nz = np.nonzero(b[i])[0]
        assert nz.size and (np.diff(nz) == 1).all() and f[i] < hz[nz[0]] and hz[nz[-1]] < f[i + 2]          # one run inside the triangle's support
        k = int(np.argmax(b[i]))
        assert abs(hz[k] - f[i + 1]) <= (hz[1] - hz[0])                                                       # the peak sits at the centre corner
        # Slaney normalisation: the triangle's area in Hz is 1, so its samples sum to about 1 / bin width
        if nz.size >= 6:
            assert abs(b[i].sum() * (hz[1] - hz[0]) - 1.0) < 0.15
    np.testing.assert_allclose(_lib.internal_ge2e_mel_basis(), g2.mel_basis(), rtol=1e-6, atol=0)


def test_a_pure_tone_lands_in_its_triangle():
    f = an.mel_corners(40, 0.0, 11025.0)
    for tone in (300.0, 1000.0, 4000.0):
        x = np.sin(2 * np.pi * tone * np.arange(8000) / 22050.0).astype(np.float32)
        m = g2.mel_power(x)[5:30].mean(axis=0)
        k = int(np.argmax(m))
        assert f[k] < tone < f[k + 2], (tone, k)


def test_reflect_edge_frame_zero_of_a_ramp():
    x = (np.arange(3000, dtype=np.float32) ** 1.5) / 3000.0 ** 1.5                 # asymmetric: a wrong padding rule shows in frame 0
    fr = g2.frames_of(x.astype(np.float64))
    want0 = np.concatenate([x[275:0:-1], x[:276]]).astype(np.float64)
    assert np.array_equal(fr[0], want0)
    s = 220 * 13 - 275 + np.arange(551)
    assert fr.shape[0] == 14 and np.array_equal(fr[13], x[np.where(s < 3000, s, 2 * 2999 - s)].astype(np.float64))
    spec = np.abs(np.fft.rfft(want0 * g2.hann_window())) ** 2
    np.testing.assert_allclose(g2.power_spectrum(x)[0], spec, rtol=1e-12, atol=1e-18)


# ---------------------------------------------------------------------------------------------------- LSTM

def test_lstm_against_torch_float64_and_the_reference(golden):
    sd = weights()
    m = torch_lstm(40, 3, sd, "float64")
    lin = torch.nn.Linear(256, 256).double()
    lin.load_state_dict({"weight": torch.from_numpy(sd["linear.weight"]).double(), "bias": torch.from_numpy(sd["linear.bias"]).double()})
    for i in range(3):
        x = golden[f"fwd_x{i}"]
        with torch.no_grad():
            _, (h, _) = m(torch.from_numpy(x).double())
            y = torch.relu(lin(h[-1]))
            y = (y / (torch.norm(y, dim=1, keepdim=True) + 1e-5)).numpy()
        np.testing.assert_allclose(g2.lstm(sd, x), h[-1].numpy(), rtol=0, atol=1e-13)
        got = g2.embed_frames(sd, x)
        np.testing.assert_allclose(got, y, rtol=0, atol=1e-13)
        np.testing.assert_allclose(got, golden[f"fwd_y{i}"], rtol=0, atol=2e-6)      # the reference ran in float32


def test_lengths_freeze_the_state():
    x, lens, out, h = lstm_case("l0_lengths")
    assert lens is not None and set(lens) == {160, 1, 159}
    for i in (0, 1, 2, 7):
        o1, h1 = g2.lstm_layer(*[weights()[f"lstm.{p}_l0"] for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")],
                               x[i:i + 1, :lens[i]].astype(np.float64))
        # equal up to the BLAS's summation order, which follows the batch size
        assert np.abs(h1[0] - h[i]).max() < 1e-14 and np.abs(o1[0] - out[i, :lens[i]]).max() < 1e-14 and np.isfinite(out[i]).all()
        assert np.array_equal(out[i, lens[i]:], np.broadcast_to(h[i], out[i, lens[i]:].shape))


@pytest.mark.parametrize("name", ["l0_saturated", "l0_default_scale", "l1_n1_t2"])
def test_cases_behave_as_their_names_say(name):
    x, lens, out, h = lstm_case(name)
    o32, h32 = lstm_float32(name)
    assert np.abs(o32.astype(np.float64) - out).max() < (1e-4 if name == "l0_saturated" else 1e-6)      # large pre-activations carry float32 rounding of their own size
    if name == "l0_saturated":
        assert (np.abs(out) > 0.75).mean() > 0.05          # saturated gates drive |h| towards 1
    if name == "l0_default_scale":
        assert 0.02 < np.abs(out[:, -1]).mean() < 0.2


def test_embed_utterance_against_the_reference(golden):
    assert [zlib.crc32(c.tobytes()) for c in clips()] == golden["utt_crc"].tolist()
    assert [len(g2.partial_slices(c.size)[1]) for c in clips()] == [1, 2, 3]
    for up, key in ((True, "utt_partials"), (False, "utt_whole")):
        got = reference_embeddings(up, "float64")
        np.testing.assert_allclose(got, golden[key], rtol=0, atol=5e-6)              # the reference ran in float32
        if up:
            np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- the packer

@pytest.mark.parametrize("K", [40, 256])
def test_lstm_packer_round_trip_and_gate_grouping(K):
    rs = np.random.RandomState(K)
    w = rs.standard_normal((1024, K)).astype(np.float32)
    frag = _lib.ge2e_pack_lstm(w)
    assert frag.size == -(-K // 16) * 64 * 64 * 4
    assert np.array_equal(g2.unpack_lstm_fragments(frag, K), w)
    # every group of four 16-row MFMA tiles holds i, f, g, o of the same 16 hidden units
    rows = g2.packed_row(np.arange(1024)).reshape(16, 4, 16)
    assert sorted(rows.reshape(-1).tolist()) == list(range(1024))
    for g in range(16):
        for gate in range(4):
            assert rows[g, gate].tolist() == list(range(gate * 256 + 16 * g, gate * 256 + 16 * g + 16))
    # a weight that encodes its own torch row: tile rt of the stream holds the rows the map says
    enc = np.repeat(np.arange(1024, dtype=np.float32)[:, None], K, axis=1)
    s = _lib.ge2e_pack_lstm(enc).reshape(-1, 64, 64, 4)
    for lane in (0, 5, 63):
        assert np.array_equal(s[0, :, lane, 0], g2.packed_row(16 * np.arange(64) + (lane & 15)).astype(np.float32))
    _, b = _lib.ge2e_pack_lstm(w, np.arange(1024, dtype=np.float32), np.zeros(1024, np.float32))
    assert np.array_equal(b, g2.packed_row(np.arange(1024)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------- the Python surface

def test_import_ge2e_reads_dict_npz_and_pt(tmp_path):
    sd = synth_ge2e_state_dict(3)
    a = import_ge2e(sd)
    assert list(a) == [k for k in sd if not k.startswith("similarity")] and all(v.dtype == np.float32 for v in a.values())
    np.savez(tmp_path / "enc.npz", **sd)
    b = import_ge2e(str(tmp_path / "enc.npz"))
    # a checkpoint in the reference's layout, written here: the real encoder.pt is not available
    torch.save({"step": 7, "model_state": {k: torch.from_numpy(v) for k, v in sd.items()}}, tmp_path / "encoder.pt")
    c = import_ge2e(str(tmp_path / "encoder.pt"))
    for k in a:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])
    bad = dict(sd)
    del bad["lstm.bias_hh_l1"]
    with pytest.raises(KeyError, match="bias_hh_l1"):
        import_ge2e(bad)
    bad = dict(sd, **{"lstm.weight_ih_l0": np.zeros((1024, 64), np.float32)})
    with pytest.raises(ValueError, match="weight_ih_l0"):
        import_ge2e(bad)


def test_predefined_embedder_builds_ge2e_on_the_cpu():
    from cmtts_amd import host
    cfg = {"preprocessing": {"audio": {"sampling_rate": 22050}, "stft": {"win_length": 1024}, "speaker_embedder": "GE2E"}}
    emb = host.PreDefinedEmbedder(cfg, weights=weights(), device="cpu")
    assert isinstance(emb.embedder, host.GE2EEncoder) and emb.embedder_type == "GE2E"
    with pytest.raises(ValueError, match="ge2e_speaker_embedder_path"):
        host.PreDefinedEmbedder(cfg, device="cpu")
    with pytest.raises(NotImplementedError):
        host.PreDefinedEmbedder({"preprocessing": dict(cfg["preprocessing"], speaker_embedder="other")}, device="cpu")
    lib = _lib.load()
    assert lib.cmtts_ge2e_create(None) == -1 and lib.cmtts_ge2e_finalize(None) == -1 and b"null" in lib.cmtts_last_error()
    assert lib.cmtts_ge2e_workspace_bytes(0, 160) == 0 and lib.cmtts_ge2e_workspace_bytes(1, 0) == 0 and lib.cmtts_ge2e_workspace_bytes(2, 160) > 2 * 160 * 5120


def test_speaker_width_check():
    from cmtts_amd import host
    from cmtts_amd.config import get_config
    cfg = get_config("VCTK")
    assert cfg.external_speaker_dim == 512
    with pytest.raises(ValueError, match="external_speaker_dim = 512"):
        host._check_speaker_width(cfg, torch.zeros(2, 256), 2)
    host._check_speaker_width(cfg, torch.zeros(2, 512), 2)
    host._check_speaker_width(cfg, None, 2)
    assert set(LSTM_CASES) >= {"l0_saturated", "l0_default_scale", "l0_lengths"}
