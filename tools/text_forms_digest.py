#!/usr/bin/env python3
"""Every form the text / frame side's host dispatch (csrc/text_side.hip: fft_stack, predictor and the two entry points around them) can route a
stage to, at the smallest shapes that reach it: one JSON line per cell with the sha256 of every tensor duration_pitch_energy_net returns.  Two
builds of the library (CMTTS_LIB) that print the same lines route every cell the same way; under `rocprofv3 --kernel-trace` the --no-streams
cells also give a deterministic launch list to compare.
  --no-streams          only the branch_streams = 0 cells (one stream: the kernel order is deterministic)"""
import argparse, hashlib, json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd
from cmtts_amd import host, _lib
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict, synth_decoder_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--no-streams", action="store_true")
args = ap.parse_args()

lib = _lib.load()
DEV = "cuda:0"

# (1, 1): a single column; (2, 25): ragged lengths, 32-column tiles; (8, 100): cols96 and xres_small both false — the generic kernel behind separate
# LayerNorms; (3, 130): two 96-column tiles; (2, 200): key-chunked attention; (32, 85): 96-column tiles fill the chip, the frame side (T = 6 L) reaches
# conv_xl; (64, 85): the in-projection takes the 32-column instance
SHAPES = [(1, 1), (2, 25), (8, 100), (3, 130), (2, 200), (32, 85), (64, 85)]
SWITCH_SHAPES = [(2, 25), (8, 100), (32, 85)]
FORMS = {      # precision -> [(internal switches, model options)]
    "fp32": [({"attn_fused": 0}, {})] +
            [({"text_xres": k, **w}, {}) for k in (0, 1, 2, 4, 9) for w in ({}, {"ffn_wino": 0})] +
            [({k: 0}, {}) for k in ("ffn_xres", "ffn_fused", "ffn_wino", "xres_small", "pred_xres", "pred_xl", "pred_head", "pred_wino",
                                    "energy_head", "stats_mlp", "cwt_in_phoneme")] +
            [({"ffn_wino": 2}, {}), ({}, {"ffn2_split": 0})],
}
FORMS["bf16"] = FORMS["fp16"] = [({}, {"text16": 0}), ({}, {"text16": 1}), ({"text_xt16": 0}, {"text16": 1})]


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def emit(cell, tensors):
    torch.cuda.synchronize()
    print(json.dumps({"cell": cell, "sha256": {k: sha(v) for k, v in sorted(tensors.items())}}), flush=True)


def inputs(cfg, B, L):
    rs = np.random.RandomState(1000 * B + L)
    lens = np.maximum((rs.uniform(0.4, 1.0, size=B) * L).astype(np.int64), 1)
    lens[0] = L
    texts = rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)
    texts[np.arange(L)[None, :] >= lens[:, None]] = 0
    kw = {}
    if cfg.multi_speaker and cfg.n_speaker > 0:
        kw["speakers"] = torch.from_numpy(rs.randint(0, cfg.n_speaker, size=B).astype(np.int64))
    elif cfg.multi_speaker:
        kw["spker_embeds"] = torch.from_numpy(rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32))
    return torch.from_numpy(texts), torch.from_numpy(lens), kw


def text_frame(model, cfg, B, L):
    """One text-side + frame-side pass at a fixed T = 6 L (no read-back) -> {name: tensor}.  The factor's padding columns [L, Lp) are workspace leftovers."""
    texts, lens, kw = inputs(cfg, B, L)
    out = model.duration_pitch_energy_net(texts=texts, src_lens=lens, max_mel_len=6 * L, **kw)
    t = {k: v for k, v in out.items() if torch.is_tensor(v)}
    t.update({"p." + k: v for k, v in out["p_predictions"].items() if torch.is_tensor(v)})
    f = out["cond_factors"]
    if f is not None:
        t["cond_p1"] = f.p1[..., :L]
        if f.p1t is not None:
            t["cond_p1t"] = f.p1t[:, :, :L, :]
    return t


def with_form(model, switches, options, fn):
    prev_sw = {k: _lib.internal_set(k, v) for k, v in switches.items()}
    assert all(p >= 0 for p in prev_sw.values()), (switches, prev_sw)
    prev_opt = {k: model.set_option(k, v) for k, v in options.items()}
    try:
        fn()
    finally:
        for k, v in prev_opt.items():
            model.set_option(k, v)
        for k, v in prev_sw.items():
            _lib.internal_set(k, v)


MODELS = {}
for variant in ("LJSpeech", "VCTK", "VCTK_table"):
    cfg = get_config(variant)
    sd = synth_cmtts_state_dict(cfg, seed=21)
    if variant == "LJSpeech":
        sd.update(synth_decoder_state_dict(cfg, seed=4))
    MODELS[variant] = (cfg, host.CMTotalTTS(cfg, DEV).load_state_dict(sd))

for streams in (0,) if args.no_streams else (0, 1):
    prev_streams = lib.cmtts_set_option(b"branch_streams", streams)
    # every shape, every variant, default forms
    for variant, (cfg, model) in MODELS.items():
        for B, L in SHAPES:
            emit({"variant": variant, "B": B, "L": L, "streams": streams}, text_frame(model, cfg, B, L))
    # every switch against the default cells above, and the 16-bit text side
    cfg, model = MODELS["VCTK"]
    for prec, forms in FORMS.items():
        model.set_precision(prec)
        for switches, options in forms:
            for B, L in SWITCH_SHAPES:
                cell = {"variant": "VCTK", "B": B, "L": L, "streams": streams, "precision": prec, "switches": switches, "options": options}
                with_form(model, switches, options, lambda: emit(cell, text_frame(model, cfg, B, L)))
    model.set_precision("fp32")
    # one ragged call (pad_lens): groups of L = 32, 64, 128 in one text-side launch sequence, then each group's frame side
    groups = []
    for n, Lg in ((3, 32), (2, 64), (2, 128)):
        texts, lens, kw = inputs(cfg, n, Lg)
        groups.append((texts.to(DEV), lens.to(DEV), kw["spker_embeds"].to(DEV), None, 6 * Lg))
    for tb in host.collate_groups(groups, DEV).batches:
        tws, B_all, L_all, mel_len, spk = host._text_forward_ragged(model, tb, "digest_text")
        t = {"mel_lens": mel_len, "speaker_emb": spk}
        for gi, b0, n, Lg in tb["members"]:
            cond_ct, f = host._frame_forward_sub(model, tws, B_all, L_all, b0, n, 6 * Lg, "digest_frame")
            t.update({f"g{gi}.cond_ct": cond_ct, f"g{gi}.mel2ph": f.mel2ph, f"g{gi}.p_idx": f.p_idx, f"g{gi}.cond_p1": f.p1[..., :Lg]})
        emit({"entry": "cmtts_text_forward_ragged", "groups": [(m[2], m[3]) for m in tb["members"]], "streams": streams}, t)
    # the decoder: the same FFT blocks over frames
    cfg, model = MODELS["LJSpeech"]
    B, T = 2, 61
    rs = np.random.RandomState(61)
    x = rs.standard_normal(size=(B, T, cfg.hidden)).astype(np.float32)
    pad = np.arange(T)[None, :] >= np.asarray([T, 37])[:, None]
    x[pad] = 0
    for switches in ({}, {"attn_fused": 0}, {"text_xres": 0}):
        cell = {"entry": "cmtts_decoder_forward", "B": B, "T": T, "streams": streams, "switches": switches}
        with_form(model, switches, {}, lambda: emit(cell, {"y": model.decoder(torch.from_numpy(x), torch.from_numpy(pad))}))
    lib.cmtts_set_option(b"branch_streams", prev_streams)
