#!/usr/bin/env python3
"""Every form the generator's host dispatch (csrc/vocoder.hip) can route a ResBlock or an upsampler to, at toy sizes: one JSON line per
cell with the sha256 of the waveform's bytes.  Two builds of the library (CMTTS_LIB) that print the same lines route every cell the same
way; under `rocprofv3 --kernel-trace` the --no-streams cells also give a deterministic launch list to compare.
  --no-streams          only the branch_streams = 0 cells (one stream: the kernel order is deterministic)"""
import argparse, hashlib, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd
from cmtts_amd import host, _lib
from cmtts_amd.config import HifiGanConfig
from cmtts_amd.weights import synth_hifigan_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--no-streams", action="store_true")
args = ap.parse_args()

lib = _lib.load()
DEV = "cuda:0"
hcfg = HifiGanConfig()
voc = host.Generator(hcfg, DEV).load_state_dict(synth_hifigan_state_dict(hcfg, seed=5))

# (1, 1): every tile is halo; (2, 61): ragged tiles, every launch small; (8, 64): the launch-size gate of the fp32 Winograd forms is false
# at the C = 256 / 128 stages and true at C = 64 / 32 (512 and 1024 column tiles)
SHAPES = [(1, 1), (2, 61), (8, 64)]
W2 = {"voc_wino": 2}
FORMS = {      # precision -> [(internal switches, handle options)]
    "fp32": [({}, {})] + [({**W2, "voc_wino43": k}, {}) for k in (0, 1, 2, 3)] +
            [({**W2, "voc_qpair": 0}, {}), ({**W2, "voc_wino64": 0}, {}), ({**W2, "voc_wino64_k": 3}, {}), ({"voc_wino": 0}, {}),
             ({"voc_pair": 0}, {}), ({"voc_pair": 0, "voc_xl": 0}, {}), ({"voc_upsT": 0}, {}),
             ({}, {"winograd": 0}), ({}, {"batch_invariant": 1}), ({}, {"winograd": 0, "batch_invariant": 1})],
    "fp16x3": [({}, {}), ({"voc_pair3": 0}, {}), ({}, {"ups16": 0})],
}
FORMS["bf16"] = FORMS["fp16"] = [({}, {}), ({"voc_rb16": 0}, {}), ({"voc_rb16": 2}, {}), ({"voc_pair": 0}, {}), ({"voc_pair": 2}, {}),
                                 ({"voc_pair": 0, "voc_xl16": 0}, {}), ({"voc_pairw": 0}, {}), ({"voc_upsT": 0}, {}), ({}, {"ups16": 0})]


def mels(B, T):
    return (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(100 * B + T)) * 1.5 - 4).to(DEV)


def emit(cell, out):
    torch.cuda.synchronize()
    assert out.dtype == torch.int16 or torch.isfinite(out).all(), cell
    print(json.dumps({"cell": cell, "sha256": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}), flush=True)


MEL = {bt: mels(*bt) for bt in SHAPES}
for streams in (0,) if args.no_streams else (0, 1):
    prev_streams = lib.cmtts_set_option(b"branch_streams", streams)
    for prec, forms in FORMS.items():
        voc.set_precision(prec)
        for switches, options in forms:
            prev_sw = {k: _lib.internal_set(k, v) for k, v in switches.items()}
            assert all(p >= 0 for p in prev_sw.values()), (switches, prev_sw)
            prev_opt = {k: voc.set_option(k, v) for k, v in options.items()}
            for bt in SHAPES:
                emit({"B": bt[0], "T": bt[1], "streams": streams, "precision": prec, "switches": switches, "options": options}, voc(MEL[bt]))
            for k, v in prev_opt.items():
                voc.set_option(k, v)
            for k, v in prev_sw.items():
                _lib.internal_set(k, v)
    lib.cmtts_set_option(b"branch_streams", prev_streams)
voc.set_precision("fp32")

# one streamed cell per output type: two windows of Tw = 30 frames (cores of 4) out of B = 2 mels of T = 40
prev_streams = lib.cmtts_set_option(b"branch_streams", 0 if args.no_streams else 1)
B, T, Tw, core, N = 2, 40, 30, 4, 2
mel = mels(B, T)
tab = torch.tensor([(0, 0, 0, 4), (1, 10, 13, 4)], dtype=torch.int32, device=DEV)
nb = lib.cmtts_vocoder_windows_workspace_bytes(voc._h, N, Tw)
ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
pcm = torch.zeros(N, core * hcfg.hop, dtype=torch.int16, device=DEV)
_lib.check(lib.cmtts_vocoder_forward_windows(voc._h, host._ptr(mel), B, T, host._ptr(tab), N, Tw, core, host._ptr(pcm), 32768.0, host._ptr(ws), nb, host._stream()))
emit({"entry": "cmtts_vocoder_forward_windows", "B": B, "T": T, "Tw": Tw, "core": core}, pcm)
wav = torch.zeros(N, core * hcfg.hop, dtype=torch.float32, device=DEV)
_lib.check(lib.cmtts_vocoder_forward_windows_f32(voc._h, host._ptr(mel), B, T, host._ptr(tab), N, Tw, core, 0, host._ptr(wav), host._ptr(ws), nb, host._stream()))
emit({"entry": "cmtts_vocoder_forward_windows_f32", "B": B, "T": T, "Tw": Tw, "core": core}, wav)
lib.cmtts_set_option(b"branch_streams", prev_streams)
