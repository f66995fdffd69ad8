#!/usr/bin/env python3
"""Every route the denoiser and sampler's host dispatch (csrc/denoiser_side.hip: denoiser_core, the conditioner branch, the sampler's step loops,
cmtts_retake, cmtts_sample_ragged) can take, at the smallest shapes that reach it: one JSON line per cell with the sha256 of every returned
mel, the call's status, cmtts_poll_error() and cmtts_internal_sample_rows(); profiled cells add n_launches.  Two builds of the library
(CMTTS_LIB) that print the same lines route every cell the same way; under `rocprofv3 --kernel-trace` the --no-streams cells also give a
deterministic launch list to compare.  The tool stops (exit status 1) at the first cell whose status or error word is not the expected one.
  --no-streams          only the branch_streams = 0 cells (one stream: the kernel order is deterministic)"""
import argparse, ctypes as C, hashlib, json, os, re, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmtts_amd
from cmtts_amd import host, _lib
from cmtts_amd.config import get_config
from cmtts_amd.weights import synth_cmtts_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--no-streams", action="store_true")
args = ap.parse_args()

lib = _lib.load()
DEV = "cuda:0"
E_UNSUPPORTED = -2      # include/cmtts_hip.h: CMTTS_E_UNSUPPORTED

# (1, 1): one frame; (2, 63) / (1, 65): below / above one 64-frame tile; (3, 129): three 32-frame tiles and one frame; (5, 100): the mixed sampler's
# batch; (40, 200): 160 tiles, the default rule takes the persistent stack; (70, 250): 280 tiles, the stack's launch is chunked
SHAPES = [(1, 1), (2, 63), (1, 65), (3, 129), (5, 100), (40, 200), (70, 250)]
SWITCH_SHAPES = [(2, 63), (3, 129), (40, 200)]
# (entry-point setters, internal switches, public options, model options, precision, expected status)
P2 = {"persist": 2}
FORMS = [({"persist": 0}, {}, {}, {}, "fp32", 0), (P2, {}, {}, {}, "fp32", 0), ({"fused": 0}, {}, {}, {}, "fp32", 0)] + \
        [(s, {k: v}, {}, {}, "fp32", 0) for k, vs in (("persist_tail", (0,)), ("persist_wino", (0, 1))) for v in vs for s in ({}, P2)] + \
        [({}, {k: v}, {}, {}, "fp32", 0) for k, vs in (("inproj_fused", (0,)), ("cond_gemm", (0, 2))) for v in vs] + \
        [({}, {}, {k: v}, {}, "fp32", 0) for k, vs in (("step_cache", (0,)), ("resblock_split", (0, 2))) for v in vs] + \
        [({"tile": v}, {}, {}, {}, "fp32", 0) for v in (32, 64)] + \
        [(s, {}, {}, {"winograd": v}, "fp32", 0) for v in (0, 2) for s in ({}, P2)] + \
        [(s, {}, {}, {"batch_invariant": 1, "winograd": 1}, "fp32", 0) for s in ({}, P2, {"fused": 0}, {"persist": 0, "fused": 1})] + \
        [({}, {}, {}, {"batch_invariant": 1, "winograd": 2}, "fp32", E_UNSUPPORTED)] + \
        [({}, {"cond_gemm16": v}, {}, {}, p, 0) for p in ("bf16", "fp16", "fp16x3") for v in (0, 1)]
SETTERS = {"persist": (lib.cmtts_set_persistent_denoiser, -1), "fused": (lib.cmtts_set_fused_resblock, None), "tile": (lib.cmtts_set_resblock_tile, 0)}


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def emit(cell, fn, expect=0, profile=0):
    """Run fn() -> {name: mel}; print the cell's line; stop the tool where the status or the error word is not the expected one."""
    status, mels, line = 0, {}, {"cell": cell}
    if profile:
        _lib.check(lib.cmtts_profile_begin(4096, profile))
    try:
        mels = fn()
    except RuntimeError as e:
        m = re.match(r"libcmtts_hip error (-?\d+):", str(e))
        if not m:
            raise
        status = int(m.group(1))
    torch.cuda.synchronize()
    if profile:
        ms, n = C.c_double(), C.c_int()
        _lib.check(lib.cmtts_profile_end(C.byref(ms), C.byref(n)))
        line["profile_stride"], line["n_launches"] = profile, n.value
    err = lib.cmtts_poll_error()
    line.update(status=status, poll_error=err, sample_rows=_lib.internal_sample_rows(), sha256={k: sha(v) for k, v in sorted(mels.items())})
    print(json.dumps(line), flush=True)
    if status != expect or err != 0:
        sys.exit(1)


class form:
    """Setters, switches, options and a precision for the duration of a block; everything restored on exit."""

    def __init__(self, model, setters={}, switches={}, options={}, model_options={}, precision="fp32"):
        self.model, self.a = model, (setters, switches, options, model_options, precision)

    def __enter__(self):
        setters, switches, options, model_options, precision = self.a
        self.prev_set = {}
        for k, v in setters.items():
            fn, query = SETTERS[k]
            prev = fn(v) if query is None else fn(query)
            if query is not None:
                fn(v)
            self.prev_set[k] = 0 if k == "tile" else prev
        self.prev_sw = {k: _lib.internal_set(k, v) for k, v in switches.items()}
        self.prev_opt = {k: lib.cmtts_set_option(k.encode(), v) for k, v in options.items()}
        assert all(p >= 0 for p in list(self.prev_sw.values()) + list(self.prev_opt.values())), self.a
        self.prev_mo = {k: self.model.set_option(k, v) for k, v in model_options.items()}
        self.model.set_precision(precision)

    def __exit__(self, *exc):
        self.model.set_precision("fp32")
        for k, v in self.prev_mo.items():
            self.model.set_option(k, v)
        for k, v in self.prev_opt.items():
            lib.cmtts_set_option(k.encode(), v)
        for k, v in self.prev_sw.items():
            _lib.internal_set(k, v)
        for k, v in self.prev_set.items():
            SETTERS[k][0](v)


def dense_inputs(cfg, B, T):
    gen = torch.Generator().manual_seed(1000 * B + T)
    x = torch.randn(B, 1, T, cfg.n_mels, generator=gen)
    cond = torch.randn(B, T, cfg.hidden, generator=gen)
    spk = torch.randn(B, cfg.hidden, generator=gen) if cfg.multi_speaker else None
    noise = torch.randn(5, B, 1, T, cfg.n_mels, generator=gen).to(DEV)
    return x, cond, spk, noise


def forward_and_samples(model, B, T, steps, cell, expect=0, profile=0):
    """cmtts_denoiser_forward, then cmtts_sample with every step count of `steps`: one line each."""
    x, cond, spk, noise = dense_inputs(model.config, B, T)
    cond_ct = cond.transpose(1, 2).contiguous().to(DEV)
    spk_d = spk.to(DEV) if spk is not None else None
    emit({"entry": "cmtts_denoiser_forward", **cell}, lambda: {"out": model.net(x, torch.full((B,), 1095.5), cond, spk)}, expect, profile)
    for n in steps:
        emit({"entry": "cmtts_sample", "n": n, **cell}, lambda: {"mel": host.sample_with_cond(model, cond_ct, spk_d, n, noise)}, expect, profile)


def text_inputs(cfg, B, L, seed=0):
    rs = np.random.RandomState(1000 * B + L + seed)
    lens = np.maximum((rs.uniform(0.4, 1.0, size=B) * L).astype(np.int64), 1)
    lens[0] = L
    texts = rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)
    texts[np.arange(L)[None, :] >= lens[:, None]] = 0
    spk = torch.from_numpy(rs.standard_normal(size=(B, cfg.external_speaker_dim)).astype(np.float32))
    return torch.from_numpy(texts), torch.from_numpy(lens), spk


def frame_side(model, B, L, T, seed=0):
    """Conditioning with its factors, as the frame side hands them to the sampler."""
    texts, lens, spk = text_inputs(model.config, B, L, seed)
    return model.duration_pitch_energy_net(None, texts, lens, spker_embeds=spk, max_mel_len=T)


def shard(model, sizes, n_steps, trimmed):
    """[(bucket, n)] -> the groups of a ragged shard for host.sample_ragged"""
    groups = []
    for bucket, n in sizes:
        o = frame_side(model, n, bucket // 4, bucket, seed=bucket)
        noise = torch.randn(n_steps + 1, n, 1, bucket, model.config.n_mels, generator=torch.Generator().manual_seed(bucket + n)).to(DEV)
        groups.append((o["cond_ct"], o["speaker_emb"], noise, o["mel_lens"].tolist() if trimmed else None, o["cond_factors"]))
    return groups


MODELS = {}
for variant, seed, kw in (("LJSpeech", 5, {}), ("VCTK", 5, {}), ("LibriTTS", 12, {"dur_frames": 4.0, "dur_spread": 0.0})):
    cfg = get_config(variant)
    MODELS[variant] = host.CMTotalTTS(cfg, DEV).load_state_dict(synth_cmtts_state_dict(cfg, seed=seed, **kw))
    # The step cache takes a row once the event behind its copy has completed: a call that computes sigma_max's row and asks for it again (the second
    # group of a ragged shard) would route by timing — same bits, another launch list.  Every model gets the row before the first cell.
    x, cond, spk, noise = dense_inputs(cfg, 1, 1)
    host.sample_with_cond(MODELS[variant], cond.transpose(1, 2).contiguous().to(DEV), spk.to(DEV) if spk is not None else None, 1, noise)
    torch.cuda.synchronize()

for streams in (0,) if args.no_streams else (0, 1):
    prev_streams = lib.cmtts_set_option(b"branch_streams", streams)
    # every shape, both variants, default forms
    for variant in ("LJSpeech", "VCTK"):
        for B, T in SHAPES:
            forward_and_samples(MODELS[variant], B, T, (1, 2, 4), {"variant": variant, "B": B, "T": T, "streams": streams})
    # every switch against the default cells above
    model = MODELS["VCTK"]
    for setters, switches, options, model_options, precision, expect in FORMS:
        for B, T in SWITCH_SHAPES:
            cell = {"variant": "VCTK", "B": B, "T": T, "streams": streams, "precision": precision, "setters": setters, "switches": switches,
                    "options": options, "model_options": model_options}
            with form(model, setters, switches, options, model_options, precision):
                forward_and_samples(model, B, T, (2,), cell, expect)
    # the event pairs of cmtts_profile_*: the per-layer routes (every stride-th layer), the three-launch block and the persistent stack
    for stride in (1, 3):
        for (B, T), setters in (((3, 129), {}), ((2, 63), {"fused": 0}), ((40, 200), {})):
            with form(model, setters):
                forward_and_samples(model, B, T, (4,), {"variant": "VCTK", "B": B, "T": T, "streams": streams, "setters": setters}, 0, stride)
    # factored and seeded entries on the frame side's conditioning: with the caller's transposed factor, without it, seeded, and the two switches
    for B, L, T in ((1, 5, 33), (3, 40, 200), (32, 85, 512)):
        o = frame_side(model, B, L, T)
        f = o["cond_factors"]
        f_not = host.CondFactors(f.p1, f.p1_ld, f.L, f.mel2ph, f.p_idx, o["cond_ct"])
        noise = torch.randn(5, B, 1, T, model.config.n_mels, generator=torch.Generator().manual_seed(T)).to(DEV)
        for name, fac, kw, switches in (("p1t", f, {"noise": noise}, {}), ("no_p1t", f_not, {"noise": noise}, {}), ("seeded", f, {"seeds": 7}, {}),
                                        ("seeded_no_p1t", f_not, {"seeds": 7}, {}), ("p1t", f, {"noise": noise}, {"cond_inkernel": 0}),
                                        ("p1t", f, {"noise": noise}, {"cond_factored": 0}), ("seeded", f, {"seeds": 7}, {"cond_inkernel": 0})):
            cell = {"entry": "factored", "case": name, "B": B, "L": L, "T": T, "streams": streams, "switches": switches}
            with form(model, switches=switches):
                emit(cell, lambda: {"mel": host.sample_with_cond(model, o["cond_ct"], o["speaker_emb"], 4, factors=fac, **kw)})
    # cmtts_sample_mixed: utterances that leave, a uniform plan, four sigmas in one evaluation, explicit noise in place of seeds
    for B, T, counts in ((5, 100, [4, 4, 2, 2, 1]), (40, 200, [4] * 12 + [2] * 12 + [1] * 16), (5, 100, [4] * 5)):
        x, cond, spk, noise = dense_inputs(model.config, B, T)
        cond_ct, spk_d = cond.transpose(1, 2).contiguous().to(DEV), spk.to(DEV)
        for kw in ({"seeds": 11}, {"noise": noise}):
            cell = {"entry": "cmtts_sample_mixed", "B": B, "T": T, "counts": counts, "noise": sorted(kw)[0], "streams": streams}
            emit(cell, lambda: {"mel": host.sample_mixed(model, cond_ct, spk_d, counts, **kw)})
    x, cond, spk, noise = dense_inputs(model.config, 4, 100)
    sig = np.asarray([[80.0, 40.0, 10.0, 2.5]], np.float32)
    emit({"entry": "cmtts_sample_mixed", "B": 4, "T": 100, "case": "four sigmas in one evaluation", "streams": streams},
         lambda: {"mel": host.sample_mixed(model, cond.transpose(1, 2).contiguous().to(DEV), spk.to(DEV), [1, 1, 1, 1], seeds=3, sigmas=sig,
                                           renoise_std=np.full((1, 4), -1.0, np.float32))})
    # cmtts_retake: B = 3, T = 200, one span that is not quad-aligned (tests/retake_cases.py: "odd")
    x, cond, spk, noise = dense_inputs(model.config, 3, 200)
    emit({"entry": "cmtts_retake", "B": 3, "T": 200, "spans": [(0, 101, 103)], "streams": streams},
         lambda: {"mel": host.retake(model, noise[0, :, 0], cond.transpose(1, 2).contiguous().to(DEV), spk.to(DEV), [(0, 101, 103)], 5, n_steps=4)})
    # cmtts_sample_ragged: one launch for four groups, trimmed and not; a small group set aside; the group-after-group fallback
    model = MODELS["LibriTTS"]
    for n_steps in (1, 4):
        for trimmed in (False, True):
            for name, sizes, setters, precision in (("one_launch", [(128, 8), (256, 8), (512, 8), (384, 8)], {}, "fp32"),
                                                    ("set_aside", [(1024, 15), (256, 8)], {}, "fp32"),
                                                    ("fallback", [(128, 8), (256, 8)], {"persist": 0}, "fp32"),
                                                    ("fallback", [(128, 8), (256, 8)], {}, "bf16")):
                if name != "one_launch" and (trimmed or n_steps == 1 and name == "fallback"):
                    continue
                groups = shard(model, sizes, n_steps, trimmed)
                cell = {"entry": "cmtts_sample_ragged", "case": name, "groups": sizes, "n": n_steps, "active_frames": trimmed, "setters": setters,
                        "precision": precision, "streams": streams}
                with form(model, setters, precision=precision):
                    emit(cell, lambda: {f"g{i}": m for i, m in enumerate(host.sample_ragged(model, groups, n_steps, tail_frames=16))},
                         profile=1 if name == "one_launch" and not trimmed else 0)
    lib.cmtts_set_option(b"branch_streams", prev_streams)
