"""Golden vectors of the GE2E speaker encoder -> tests/golden/ge2e.npz.

Runs only where the reference tree is available (REF below, read-only); the tests read the .npz and never this script.  It imports the
reference's ge2e_encoder.model.SpeakerEncoder and ge2e_encoder.inference at run time — librosa and webrtcvad are stubbed, they are not
installed and not needed: the one librosa call, audio.wav_to_mel_spectrogram, is replaced by cmtts_amd.ge2e.mel_power — loads the seeded
synthetic weights (cmtts_amd.weights.synth_ge2e_state_dict) through the reference's own load_state_dict, and stores data only:

    seed                         the weights' seed (5.7 MB of weights are regenerated from it, not stored)
    slice_n, slice_count,        compute_partial_slices for the sample counts of tests/ge2e_cases.py: SLICE_COUNTS: how many partials, the
    slice_last_start, slice_pad  last one's first mel frame, and the length embed_utterance pads the waveform to
    fwd_x{i}, fwd_y{i}           SpeakerEncoder.forward on a few [N, T, 40] float32 inputs
    utt_partials, utt_whole      embed_utterance on the clips of tests/ge2e_cases.py: clips() (regenerated from their recipe; utt_crc guards
                                 it), with using_partials True / False: the padding, slicing, mean and norm are the reference's own
"""
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cmtts_amd  # noqa: E402,F401
from cmtts_amd import ge2e as g2  # noqa: E402
from cmtts_amd.weights import synth_ge2e_state_dict  # noqa: E402
import ge2e_cases as cases  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_reference():
    _stub("librosa")
    _stub("webrtcvad")
    sys.path.insert(0, REF)
    from ge2e_encoder import inference, audio
    from ge2e_encoder.model import SpeakerEncoder
    return inference, audio, SpeakerEncoder


def main():
    inference, audio, SpeakerEncoder = import_reference()
    cpu = torch.device("cpu")
    model = SpeakerEncoder(cpu, cpu)
    sd = synth_ge2e_state_dict(cases.SEED)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()
    inference._model, inference._device = model, cpu
    audio.wav_to_mel_spectrogram = lambda wav: g2.mel_power(wav).astype(np.float32)

    out = {"seed": np.asarray(cases.SEED)}
    cnt, last, pad = [], [], []
    for n in cases.SLICE_COUNTS:
        wave_slices, mel_slices = inference.compute_partial_slices(n)
        cnt.append(len(mel_slices))
        last.append(mel_slices[-1].start)
        pad.append(max(n, wave_slices[-1].stop) if wave_slices[-1].stop >= n else n)
    out.update(slice_n=np.asarray(cases.SLICE_COUNTS), slice_count=np.asarray(cnt), slice_last_start=np.asarray(last), slice_pad=np.asarray(pad))

    rs = np.random.RandomState(21)
    for i, (N, T, scale) in enumerate(((3, 160, 1.0), (2, 7, 40.0), (1, 1, 1.0))):
        x = (np.abs(rs.standard_normal((N, T, 40))) * scale).astype(np.float32)
        with torch.no_grad():
            y = model.forward(torch.from_numpy(x)).numpy()
        out[f"fwd_x{i}"], out[f"fwd_y{i}"] = x, y

    clips = cases.clips()
    with torch.no_grad():
        out["utt_partials"] = np.stack([inference.embed_utterance(c) for c in clips])
        out["utt_whole"] = np.stack([inference.embed_utterance(c, using_partials=False) for c in clips])
    out["utt_crc"] = np.asarray([zlib.crc32(c.tobytes()) for c in clips], np.int64)
    np.savez_compressed(cases.GOLDEN, **out)
    print("wrote", cases.GOLDEN, os.path.getsize(cases.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
