"""Python host layer: the reference's call surface over the C ABI (include/cmtts_hip.h).

Mirrors, name for name, the callables the reference's inference path is made of:

    CMTotalTTS / CMDenoiserTTS / DurationPitchSpeakerNet   model/cm_tool/tts_net.py, model/cmtts.py
    KarrasDenoiser.denoise, karras_sample_tts               model/cm_tool/karras_diffusion.py
    Generator (HiFi-GAN), get_vocoder-style loading,
    vocoder_infer                                           hifigan/models.py, utils/model.py
    CMTotalTTSSynthesize.synthesize                         synthesize.py:35-153

PyTorch is plumbing only (device memory, streams, nn.Module container): every operator call goes
to hand-written HIP kernels through ctypes.  There is no eager/PyTorch fallback — a missing
``libcmtts_hip.so`` raises at construction time.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import noise as _noise
from . import retake as _retake
from .config import CMTTSConfig, HifiGanConfig


def _ptr(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, device):
    return torch.as_tensor(t).to(device=device, dtype=torch.float32).contiguous()       # a tensor on `device` passes through; a numpy array is uploaded


def _i64(t, device):
    return t.to(device=device, dtype=torch.int64).contiguous()


def _check_speaker_width(cfg, spk, B):
    """spker_embeds as the speaker_emb dense takes them: [B, external_speaker_dim] (512: DeepSpeaker, 256: GE2E).  The kernel reads
    external_speaker_dim floats per row whatever it is handed, so another width must stop here."""
    if spk is None:
        return
    if spk.dim() < 1 or spk.shape[-1] != cfg.external_speaker_dim or spk.numel() != B * cfg.external_speaker_dim:
        raise ValueError(f"spker_embeds has shape {tuple(spk.shape)}; this model's speaker_emb takes [{B}, {cfg.external_speaker_dim}] "
                         f"(external_speaker_dim = {cfg.external_speaker_dim}: 512 for DeepSpeaker vectors, 256 for GE2E)")


def _resolve_controls(B, L, p_control=1.0, e_control=1.0, d_control=1.0):
    """The three prosody controls of a call over B utterances padded to L phonemes, each a Python number (the scalar path), a [B]
    tensor (one factor per utterance) or a [B, L] tensor (one per phoneme), fp32.  Returns ((p, e, d) scalars, {"p" | "e" | "d":
    fp32 [B, L] CPU table}): a control given as a tensor has scalar 1.0 and a table (a [B] vector broadcast along its row).
    The tables are validated here, before anything launches — ValueError for a wrong type, dtype or shape, a NaN, p <= 0
    (it also scales the uv logit) or d < 0."""
    scal, tabs = [], {}
    for name, v in (("p", p_control), ("e", e_control), ("d", d_control)):
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(v)
        if not isinstance(v, torch.Tensor):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name}_control: a number, a [B] tensor or a [B, L] tensor, not {type(v).__name__}")
            scal.append(float(v))       # the scalar path, as it was: cmtts_set_variance_controls judges the value
            continue
        if v.dtype != torch.float32:
            raise ValueError(f"{name}_control: the table must be float32, not {v.dtype}")
        t = v.detach().to("cpu")
        if t.dim() == 1 and t.shape[0] == B:
            t = t[:, None].expand(B, L)
        elif t.dim() != 2 or tuple(t.shape) != (B, L):
            raise ValueError(f"{name}_control: shape {tuple(v.shape)}, expected [{B}] (per utterance) or [{B}, {L}] (per phoneme)")
        if bool(torch.isnan(t).any()):
            raise ValueError(f"{name}_control: NaN in the table")
        if name == "p" and not bool((t > 0).all()):
            raise ValueError("p_control: every factor must be > 0 (it also scales the uv logit)")
        if name == "d" and not bool((t >= 0).all()):
            raise ValueError("d_control: every factor must be >= 0")
        tabs[name] = t.contiguous()
        scal.append(1.0)
    return tuple(scal), tabs


def _check_no_scalar_with_table(scalars, p_control=None, e_control=None, d_control=None):
    """A table REPLACES the scalar of its control (cmtts_set_control_tables): a per-call table on top of a configured scalar other
    than 1 is refused instead of silently dropping one of the two."""
    for name, sc, v in zip("ped", scalars, (p_control, e_control, d_control)):
        if isinstance(v, (torch.Tensor, np.ndarray)) and not isinstance(sc, (torch.Tensor, np.ndarray)) and float(sc) != 1.0:
            raise ValueError(f"{name}_control: a table replaces the scalar control, which is {sc} here (it must be 1)")


class _InstalledTables:
    """The control tables of one call on the device, installed on the model (cmtts_set_control_tables); clear() in a finally."""

    def __init__(self, model, tabs, L, lo=None, hi=None, present_only=()):
        self.model, self.keep = model, []
        ct = _lib.ControlTablesStruct(ld=int(L))
        for name, t in tabs.items():
            if name in present_only:        # a frame-side rank: the rows come out of the records, only "p installed" matters
                t = t[:1]
            elif lo is not None:
                t = t[lo:hi]
            self.keep.append(t.to(device=model.device, dtype=torch.float32).contiguous())
            setattr(ct, name, _ptr(self.keep[-1]))
        self.active = bool(self.keep)
        if self.active:
            _lib.check(model.lib.cmtts_set_control_tables(model._h, C.byref(ct)))

    def clear(self):
        if self.active:
            self.model.lib.cmtts_set_control_tables(self.model._h, None)
            torch.cuda.current_stream(self.model.device).synchronize()      # the tables must outlive the kernels
            self.active = False


def _resolve_targets(B, L, target_frames=None, segments=None, d_targets=None):
    """The duration targets of a call over B utterances padded to L phonemes (cmtts_set_duration_targets; the definition:
    timing.fit_segments).  target_frames: an integer tensor [B] (frames per utterance), or [B, G] with segments, an integer tensor
    [B, L] that names each phoneme's segment in [-1, G) (-1: in none); a target of -1 leaves its utterance / segment alone.
    Returns None, or (target int32 [B, G] CPU, seg int32 [B, L] CPU or None), validated here, before anything launches — ValueError
    for a wrong type, dtype, shape or range, segments without targets, or targets beside d_targets (absolute durations leave
    nothing to fit)."""
    from .timing import MAX_TARGET
    if target_frames is None:
        if segments is not None:
            raise ValueError("segments: needs target_frames [B, G]")
        return None
    if d_targets is not None:
        raise ValueError("target_frames: not beside d_targets (absolute durations leave nothing to fit)")
    out = []
    for name, v in (("target_frames", target_frames), ("segments", segments)):
        if v is None:
            out.append(None)
            continue
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(v)
        if not isinstance(v, torch.Tensor):
            raise ValueError(f"{name}: an integer tensor, not {type(v).__name__}")
        if v.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name}: the tensor must be int32 or int64, not {v.dtype}")
        out.append(v.detach().to("cpu"))
    tgt, seg = out
    if seg is None:
        if tuple(tgt.shape) != (B,):
            raise ValueError(f"target_frames: shape {tuple(tgt.shape)}, expected [{B}] (with segments: [{B}, G])")
        tgt = tgt[:, None]
    else:
        if tgt.dim() != 2 or tgt.shape[0] != B or tgt.shape[1] < 1:
            raise ValueError(f"target_frames: shape {tuple(tgt.shape)}, expected [{B}, G] beside segments")
        if tuple(seg.shape) != (B, L):
            raise ValueError(f"segments: shape {tuple(seg.shape)}, expected [{B}, {L}]")
        G = int(tgt.shape[1])
        if seg.numel() and (int(seg.min()) < -1 or int(seg.max()) >= G):
            raise ValueError(f"segments: every entry must lie in [-1, {G})")
        seg = seg.to(torch.int32).contiguous()
    if tgt.numel() and (int(tgt.min()) < -1 or int(tgt.max()) > MAX_TARGET):
        raise ValueError(f"target_frames: every target must lie in [0, {MAX_TARGET}], or be -1 (leave alone)")
    return tgt.to(torch.int32).contiguous(), seg


class _InstalledTargets:
    """The duration targets of one call on the device, installed on the model (cmtts_set_duration_targets); clear() in a finally.
    lo / hi: the rows of a rank's slice (text_state_records).  clear() does not synchronise: the launch has captured the pointers,
    the tensors were allocated on the calling stream and the caching allocator hands their memory out again in that stream's order."""

    def __init__(self, model, targets, L, lo=None, hi=None):
        self.model, self.unmet, self.active = model, None, targets is not None
        if not self.active:
            return
        tgt, seg = targets
        if lo is not None:
            tgt, seg = tgt[lo:hi], (None if seg is None else seg[lo:hi])
        dev = model.device
        self.tgt = tgt.to(dev).contiguous()
        self.seg = None if seg is None else seg.to(dev).contiguous()
        self.unmet = torch.zeros(int(tgt.shape[0]), dtype=torch.int32, device=dev)
        dt = _lib.DurationTargetsStruct(seg=_ptr(self.seg), target=_ptr(self.tgt), unmet=_ptr(self.unmet), ld=int(L), n_seg=int(tgt.shape[1]))
        _lib.check(model.lib.cmtts_set_duration_targets(model._h, C.byref(dt)))

    def clear(self):
        if self.active:
            self.model.lib.cmtts_set_duration_targets(self.model._h, None)
            self.active = False

    def raise_unmet(self, first=0):
        """After a read-back has synchronised the stream: ValueError naming the utterances with a segment that could not be met."""
        if self.unmet is not None:
            bad = [(first + b, int(k)) for b, k in enumerate(self.unmet.cpu().tolist()) if k > 0]
            if bad:
                raise ValueError("target_frames: " + ", ".join(f"utterance {b}: {k} segment(s)" for b, k in bad) +
                                 " with a target > 0 hold only phonemes of 0 frames and cannot be met")


def _push_state_dict(lib, setter, handle, sd):
    for name, v in sd.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
        if a.ndim == 0:
            a = a.reshape(1)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        _lib.check(setter(handle, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))


_PG_NOTED = False


def _note_process_group(lib):
    """Once torch.distributed is initialised RCCL's kernels may share the GPU with the persistent denoiser grid, whose
    hand-offs need every workgroup resident: tell the library, which then launches that grid cooperatively (the runtime
    checks residency and fails the launch instead of letting it spin; cmtts_set_option("cooperative_launch", 0|1|2))."""
    global _PG_NOTED
    if not _PG_NOTED and torch.distributed.is_available() and torch.distributed.is_initialized():
        lib.cmtts_set_option(b"process_group", 1)
        _PG_NOTED = True


def _norm_device(device):
    """torch.device with an explicit index ("cuda" -> "cuda:<current>"): tensors report indexed devices, so an
    un-indexed one never compares equal to a buffer's and every workspace lookup would reallocate."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class _Workspace:
    """Caller-owned scratch buffers, cached per size (no allocation on the steady-state path)."""

    def __init__(self):
        self._bufs = {}

    def get(self, key, nbytes, device):
        device = _norm_device(device)
        # one set of buffers per HIP stream: groups running concurrently on different streams must not share scratch
        key = (key, torch.cuda.current_stream(device).cuda_stream)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes or buf.device != device:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf


def get_mask_from_lengths(lengths, max_len=None):
    """utils/tools.py:275-283 — True = padding."""
    if max_len is None:
        max_len = int(lengths.max().item())
    if lengths.is_cuda and lengths.dtype == torch.int64:     # one small launch instead of arange + compare
        lengths = lengths.contiguous()
        mask = torch.empty(lengths.shape[0], int(max_len), dtype=torch.bool, device=lengths.device)
        with torch.cuda.device(lengths.device):
            _lib.check(_lib.load().cmtts_length_mask(_ptr(lengths), _ptr(mask), lengths.shape[0], int(max_len), _stream()))
        return mask
    ids = torch.arange(0, max_len, device=lengths.device).unsqueeze(0)
    return ids >= lengths.unsqueeze(1)


class CondFactors:
    """The phoneme-level factor of the conditioner projections that cmtts_frame_forward_sub returns beside the conditioning
    (include/cmtts_hip.h): with it the sampler expands cp from (p1, mel2ph, p_idx) instead of running the stacked conditioner GEMM
    over the frames.  Bound to ONE conditioning tensor: `matches` refuses a different or since-modified cond_ct (the sampler then
    takes the dense GEMM on whatever it was given)."""
    __slots__ = ("p1", "p1t", "p1_ld", "L", "mel2ph", "p_idx", "_ptr", "_version", "_shape", "_aux")

    def __init__(self, p1, p1_ld, L, mel2ph, p_idx, cond_ct, p1t=None):
        self.p1, self.p1_ld, self.L, self.mel2ph, self.p_idx = p1, int(p1_ld), int(L), mel2ph, p_idx
        self.p1t = p1t          # [B, res_layers, p1_ld, res_channels]: the same factor with the channels contiguous (cmtts_frame_forward_sub_t), or None
        self._ptr, self._version, self._shape = cond_ct.data_ptr(), cond_ct._version, tuple(cond_ct.shape)
        # mel2ph and p_idx are the very tensors the caller received (out["mel2ph"], out["p_predictions"]["p_idx"]) and p1 is reachable too:
        # an in-place edit of any of them after the duration net would change the mel on the factored path only — their
        # version counters are part of the match
        self._aux = (p1._version, mel2ph._version, p_idx._version, None if p1t is None else p1t._version)

    def matches(self, cond_ct):
        return (cond_ct.data_ptr() == self._ptr and cond_ct._version == self._version and tuple(cond_ct.shape) == self._shape and
                (self.p1._version, self.mel2ph._version, self.p_idx._version, None if self.p1t is None else self.p1t._version) == self._aux)


class CMTotalTTS(torch.nn.Module):
    """Drop-in for model/cm_tool/tts_net.py:40-183 (inference side).

    ``load_state_dict`` takes the reference checkpoint's flat state_dict (synthesize.py:79-83) and
    hands every tensor, under its original key and layout, to ``cmtts_set_tensor``.
    """

    def __init__(self, config: CMTTSConfig, device="cuda:0"):
        super().__init__()
        self.config = config
        self.device = _norm_device(device) if torch.cuda.is_available() else torch.device(device)
        self.lib = _lib.load()
        cs = _lib.CMTTSConfigStruct()
        for name, _ in cs._fields_:
            setattr(cs, name, type(getattr(cs, name))(getattr(config, name)))
        self._h = C.c_void_p()
        _lib.check(self.lib.cmtts_create(C.byref(cs), C.byref(self._h)))
        self._ready = False
        self._ws = _Workspace()
        self._cond_factors = True       # the duration net returns the conditioner factors with its conditioning (fp32 models)
        self.duration_pitch_energy_net = DurationPitchSpeakerNet(self)
        self.net = CMDenoiserTTS(self)
        self.decoder = FastspeechDecoder(self)      # usable when the loaded state dict carries decoder.* (else it raises)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:      # C is None during interpreter teardown
            self.lib.cmtts_destroy(h)
            self._h = None

    def load_state_dict(self, state_dict, strict=True):
        """Takes the reference checkpoint's flat state dict.  The tensors are handed to the library under their original
        keys (host side: cmtts_set_tensor copies them); cmtts_finalize re-packs and uploads — at once when a GPU is present,
        otherwise on first use (so that host code which builds the object graph before a device is selected still runs)."""
        _push_state_dict(self.lib, self.lib.cmtts_set_tensor, self._h, state_dict)
        self._pending = True
        if self.device.type == "cuda" and torch.cuda.is_available():
            self._finalize()
        return self

    def _finalize(self):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cmtts_finalize(self._h))
        self._pending = False
        self._ready = True

    def eval(self):
        return self

    def set_precision(self, dtype="fp32"):
        """Operand precision of the denoiser residual blocks: "fp32" (reference), "bf16", "fp16", or "fp16x3" — every
        operand as two fp16 numbers (22 bits), every product as three fp16 MFMAs with fp32 accumulation: fp32-class
        results at a fraction of the fp32 matrix cost (large batches: the persistent stack; others run exact fp32)."""
        mode = {"fp32": 0, "f32": 0, "bf16": 1, "fp16": 2, "f16": 2, "fp16x3": 3}[dtype]
        _lib.check(self.lib.cmtts_set_precision(self._h, mode))
        self._precision_mode = mode
        return self

    def set_option(self, name, value):
        """Per-model numerics option (cmtts_model_set_option): "ffn2_split" 1 (default) | 0 — the FFN linear of the FFT blocks as
        eight K-segment partial GEMMs + one reduction, or as one launch (another fp32 summation order); "text16" 0 (default) | 1 — bf16 / fp16
        models: the in- / out-projections and FFN contractions of the FFT blocks and the variance predictors' convs with 16-bit operands as well (the integer stages — durations, pitch buckets, lengths —
        then depend on the precision mode); "winograd" 1 (default) | 2 | 0 — fp32 models, large batches: the gated k = 3 conv of the persistent
        denoiser stack as a Winograd convolution — 1: F(4,3) (half of the conv's MFMAs; fp32 rounding differences ~8e-6 on a mel; since round 5 / ABI revision 5),
        2: F(2,3) (2/3 of them; ~4e-6) — or (0) in the direct form (bit for bit the per-layer kernels of small batches); "batch_invariant" 0 (default) | 1 —
        fp32 models with "winograd" 1: the per-layer residual blocks of small batches run the persistent stack's F(4,3) form too, so an utterance's mel
        does not depend on what it is batched with (no effect with "winograd" 0 or on 16-bit models; with "winograd" 2 the denoiser calls raise:
        F(2,3) has no per-layer form).  Returns the previous value."""
        prev = self.lib.cmtts_model_set_option(self._h, name.encode() if isinstance(name, str) else name, int(value))
        if prev < 0:
            _lib.check(prev)
        return prev

    def _require(self):
        _note_process_group(self.lib)
        if not self._ready and getattr(self, "_pending", False):
            if not torch.cuda.is_available():
                raise RuntimeError("CMTotalTTS: no GPU — cmtts_amd has no CPU fallback (the weights are loaded, the kernels cannot run)")
            self.device = _norm_device(self.device if self.device.type == "cuda" else "cuda")
            self._finalize()
        if not self._ready:
            raise RuntimeError("CMTotalTTS: load_state_dict() first")

    def to(self, *args, **kwargs):
        """nn.Module.to: the weights live in the library's packed device buffers on the device given at construction;
        moving to that device (what synthesize.py:84 does) is a no-op, anything else is refused rather than ignored."""
        dev = kwargs.get("device", args[0] if args and isinstance(args[0], (str, torch.device, int)) else None)
        if dev is not None and self._ready and torch.cuda.is_available() and _norm_device(dev) != self.device:
            raise RuntimeError(f"CMTotalTTS was built on {self.device}; build another instance for {dev}")
        return self

    def get_segmentation_model(self):
        """tts_net.py:66-73 -> (duration_pitch_energy_net, denoise_fun)."""
        return self.duration_pitch_energy_net, self.net.forward

    def forward(self, x, timesteps, speakers=None, texts=None, src_lens=None, pitch=None, f0=None, uv=None, cwt_spec=None,
                f0_mean=None, f0_std=None, mel_lens=None, e_targets=None, d_targets=None, mel2phs=None, spker_embeds=None,
                p_control=1.0, e_control=1.0, d_control=1.0, **kwargs):
        """tts_net.py:75-183: re-runs the duration net with max_mel_len = x.size(2) (mels=x), then the denoiser.  The
        pitch target is assembled exactly like the reference does (:121-131): only when `pitch` is given, from
        pitch / f0 / uv / cwt_spec / f0_mean / f0_std.  The loss bookkeeping of :166-181 is training-only (not built)."""
        p_targets = None if pitch is None else {"pitch": pitch, "f0": f0, "uv": uv, "cwt_spec": cwt_spec,
                                                "f0_mean": f0_mean, "f0_std": f0_std}
        out = self.duration_pitch_energy_net(speakers=speakers, texts=texts, src_lens=src_lens, mels=x, mel_lens=mel_lens,
                                             p_targets=p_targets, e_targets=e_targets, d_targets=d_targets, mel2phs=mel2phs,
                                             spker_embeds=spker_embeds, p_control=p_control, e_control=e_control,
                                             d_control=d_control)
        return self.net(x, timesteps, out["cond"], out["speaker_emb"], out["mel_masks"])


class DurationPitchSpeakerNet(torch.nn.Module):
    """model/cmtts.py:10-122: the inference branch (targets None, controls 1) and the teacher-forced /
    controlled branches of VarianceAdaptor.forward (model/modules.py:331-412)."""

    def __init__(self, owner: CMTotalTTS):
        super().__init__()
        self.__dict__["_owner"] = owner

    def forward(self, speakers=None, texts=None, src_lens=None, mels=None, mel_lens=None, p_targets=None,
                e_targets=None, d_targets=None, mel2phs=None, spker_embeds=None,
                p_control=1.0, e_control=1.0, d_control=1.0, max_mel_len=None, target_frames=None, segments=None, **kwargs):
        """p_targets = {"cwt_spec" [B,T,10], "f0_mean" [B], "f0_std" [B], "uv" bool [B,T]}, e_targets [B,L],
        d_targets [B,L] as in the reference.  `mel2phs` is accepted and ignored: mel2ph is recomputed from
        d_targets (dur_to_mel2ph), which is what the reference's dataset stores.
        p_control / e_control / d_control: a number, or a float32 tensor [B] (one factor per utterance) or [B, L] (one per phoneme):
        the tables of cmtts_set_control_tables (model/modules.py:270, 326, 369 are elementwise).
        target_frames / segments: duration targets (_resolve_targets; cmtts_set_duration_targets) — each utterance, or each segment of
        it, takes exactly its target's frames (timing.fit_segments on the controlled integer durations; timing.frames_for_seconds
        turns seconds into frames, to within half a frame).  "d_rounded" then holds the fitted integers.  A segment that cannot be
        met (a target > 0 over phonemes of 0 frames) raises ValueError after the mel_len read-back; when mels / max_mel_len fix T
        there is no read-back and the counts come back as "unmet_targets" (int32 [B], device) for the caller to judge."""
        o = self._owner
        if texts is None:
            o._require()
        tshape = tuple(torch.as_tensor(texts).shape)
        if len(tshape) != 2:
            raise ValueError("texts must be [B, L]")
        (p_control, e_control, d_control), tabs = _resolve_controls(tshape[0], tshape[1], p_control, e_control, d_control)
        targets = _resolve_targets(tshape[0], tshape[1], target_frames, segments, d_targets)
        o._require()
        cfg, lib, dev = o.config, o.lib, o.device
        vc, keep = None, []
        if p_control != 1.0 or e_control != 1.0 or p_targets is not None or e_targets is not None or d_targets is not None:
            vc = _lib.VarianceControlsStruct(p_control=float(p_control), e_control=float(e_control))
            if d_targets is not None:
                keep.append(_f32(d_targets, dev)); vc.d_target = _ptr(keep[-1])
            if e_targets is not None:
                keep.append(_f32(e_targets, dev)); vc.e_target = _ptr(keep[-1])
            if p_targets is not None:
                for k in ("cwt_spec", "f0_mean", "f0_std"):
                    keep.append(_f32(p_targets[k], dev)); setattr(vc, k, _ptr(keep[-1]))
                keep.append(p_targets["uv"].to(device=dev, dtype=torch.uint8).contiguous()); vc.uv = _ptr(keep[-1])
                if mels is None and max_mel_len is None:
                    max_mel_len = int(p_targets["cwt_spec"].shape[1])
        texts = _i64(texts, dev)
        src_lens = _i64(src_lens, dev)
        B, L = texts.shape
        table = cfg.multi_speaker and cfg.n_speaker > 0          # preprocess.yaml speaker_embedder "none": nn.Embedding(speakers)
        spk_in = _f32(spker_embeds, dev) if (cfg.multi_speaker and not table and spker_embeds is not None) else None
        if cfg.multi_speaker and not table and spk_in is None:
            raise AssertionError("Speaker embedding should not be None")
        _check_speaker_width(cfg, spk_in, B)
        spk_ids = None
        if table:
            if speakers is None:
                raise AssertionError("speakers (ids into the speaker_emb table) should not be None")
            # what nn.Embedding raises (model/cmtts.py:78), also for ids that already live on the device (the reference's
            # to_device has moved them): one tiny min/max read-back — the text path synchronises for mel_len anyway, and a
            # clamped id would silently synthesise another speaker
            if speakers.numel() and (int(speakers.min()) < 0 or int(speakers.max()) >= cfg.n_speaker):
                raise IndexError("index out of range in self")
            spk_ids = _i64(speakers, dev)
        H = cfg.hidden
        with torch.cuda.device(dev):
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
            log_d, d_rounded, e_pred = f(B, L), f(B, L), f(B, L)
            mel_len = torch.empty(B, dtype=torch.int64, device=dev)
            e_idx = torch.empty(B, L, dtype=torch.int64, device=dev)
            enc_ct = f(B, H, L)
            spk = f(B, H) if cfg.multi_speaker else None
            nb = lib.cmtts_text_workspace_bytes(o._h, B, L)
            tws = o._ws.get("text", nb, dev)
            if vc is not None:
                _lib.check(lib.cmtts_set_variance_controls(o._h, C.byref(vc)))
            inst = fit = None
            try:
                inst = _InstalledTables(o, tabs, L)
                fit = _InstalledTargets(o, targets, L)
                _lib.check(lib.cmtts_text_forward(o._h, _ptr(texts), _ptr(src_lens), _ptr(spk_in), _ptr(spk_ids), B, L, float(d_control),
                                                  _ptr(log_d), _ptr(d_rounded), _ptr(mel_len), _ptr(e_pred), _ptr(e_idx),
                                                  _ptr(enc_ct), _ptr(spk), _ptr(tws), nb, _stream()))
                if mels is not None:
                    T = int(mels.size(2))                       # model/cmtts.py:61-62
                elif max_mel_len is not None:
                    T = int(max_mel_len)
                else:
                    T = int(mel_len.max().item())               # the one host read-back (pad() batch max)
                    fit.raise_unmet()
                O = cfg.cwt_out
                cond_ct = f(B, H, T)
                mel2ph = torch.empty(B, T, dtype=torch.int64, device=dev)
                cwt = f(B, T, O)
                f0 = f(B, T)
                p_idx = torch.empty(B, T, dtype=torch.int64, device=dev)
                stats = f(B, 2)
                nf = lib.cmtts_frame_workspace_bytes(o._h, B, T)
                fws = o._ws.get("frame", nf, dev)
                # fp32 models: the phoneme-level factor of the conditioner projections rides along (CondFactors)
                p1_ld = (L + 3) // 4 * 4
                p1 = f(B, cfg.res_layers * cfg.res_channels, p1_ld) if getattr(o, "_precision_mode", 0) == 0 and o._cond_factors else None
                p1t = None if p1 is None else f(B, cfg.res_layers, p1_ld, cfg.res_channels)      # channels contiguous: what the persistent stack gathers from
                _lib.check(lib.cmtts_frame_forward_sub_t(o._h, _ptr(tws), B, L, 0, B, T, _ptr(cond_ct), _ptr(mel2ph), _ptr(cwt),
                                                         _ptr(f0), _ptr(p_idx), _ptr(stats), _ptr(p1), _ptr(p1t), _ptr(fws), nf, _stream()))
            finally:
                if fit is not None:
                    fit.clear()
                if inst is not None:
                    inst.clear()
                if vc is not None:
                    lib.cmtts_set_variance_controls(o._h, None)              # back to the inference defaults
                    torch.cuda.current_stream(dev).synchronize()             # targets must outlive the kernels
        mel_masks = get_mask_from_lengths(mel_len, T)
        factors = None if p1 is None else CondFactors(p1, p1_ld, L, mel2ph, p_idx, cond_ct, p1t)
        cond_ct._cmtts_factors = factors       # rides along with THIS tensor object: sample_with_cond(cond_ct, ...) finds it (and re-checks it)
        extra = {} if fit.unmet is None else {"unmet_targets": fit.unmet}
        return {
            **extra,
            "cond": cond_ct.transpose(1, 2),               # [B,T,H] view of the channel-major buffer
            "cond_ct": cond_ct,
            "cond_factors": factors,
            "p_targets": p_targets,
            "p_predictions": {"pitch_pred": None, "f0_denorm": f0, "cwt": cwt,
                              "f0_mean": stats[:, 0], "f0_std": stats[:, 1], "p_idx": p_idx},
            "e_predictions": e_pred,
            "e_idx": e_idx,
            "log_d_predictions": log_d,
            "d_rounded": d_rounded,
            "mel_lens": mel_len,
            "mel_masks": mel_masks,
            "mel2ph": mel2ph,
            "src_masks": get_mask_from_lengths(src_lens, L),
            "speaker_emb": spk,
            "src_lens": src_lens,
            "enc_out": enc_ct.transpose(1, 2),
        }


def _as_cond_ct(conditioner, dev):
    """[B,T,H] reference layout -> channel-major [B,H,T]; free when it is a view of a _ct buffer."""
    c = conditioner.to(device=dev, dtype=torch.float32).transpose(1, 2)
    return c if c.is_contiguous() else c.contiguous()


class FastspeechDecoder(torch.nn.Module):
    """model/modules.py:154-165 (FFTBlocks.forward :80-105 with the learnable pos_embed_alpha).  The reference defines
    this module and never instantiates it; it is served here from the same FFT-block kernels as
    the text encoder, over the frame axis, for checkpoints whose state dict carries `decoder.*`
    (cmtts_amd.weights.synth_decoder_state_dict lists the keys).  forward(x [B,T,256], padding_mask [B,T] | None)."""

    def __init__(self, owner: CMTotalTTS):
        super().__init__()
        self.__dict__["_owner"] = owner      # not a registered child: the owner holds this module (no module cycle)

    def forward(self, x, padding_mask=None, attn_mask=None, return_hiddens=False):
        if attn_mask is not None or return_hiddens:
            raise NotImplementedError("FastspeechDecoder: attn_mask / return_hiddens are not used on the inference path")
        o = self._owner
        o._require()
        dev, lib = o.device, o.lib
        x = _f32(x, dev)
        B, T, H = x.shape
        if padding_mask is None:
            padding_mask = x.abs().sum(-1).eq(0)            # modules.py:86
        padding_mask = padding_mask.to(device=dev, dtype=torch.bool)
        lens = (~padding_mask).sum(1).to(torch.int64)
        if not torch.equal(padding_mask, get_mask_from_lengths(lens, T)):
            raise NotImplementedError("FastspeechDecoder: the padding mask must mark a suffix of every row (a length mask)")
        x_ct = transpose_last2(x)
        with torch.cuda.device(dev):
            out_ct = torch.empty(B, H, T, dtype=torch.float32, device=dev)
            nb = lib.cmtts_decoder_workspace_bytes(o._h, B, T)
            ws = o._ws.get("dec", nb, dev)
            _lib.check(lib.cmtts_decoder_forward(o._h, _ptr(x_ct), _ptr(lens), B, T, _ptr(out_ct), _ptr(ws), nb, _stream()))
        return transpose_last2(out_ct)


class CMDenoiserTTS(torch.nn.Module):
    """model/cm_tool/tts_net.py:11-37: forward(x, timesteps, conditioner, speaker_emb, mask)."""

    def __init__(self, owner: CMTotalTTS):
        super().__init__()
        self.__dict__["_owner"] = owner

    def forward(self, x, timesteps, conditioner=None, speaker_emb=None, mask=None):
        o = self._owner
        o._require()
        dev, lib = o.device, o.lib
        x = _f32(x, dev)
        B, one, T, M = x.shape
        assert one == 1 and M == o.config.n_mels
        cond_ct = _as_cond_ct(conditioner, dev)
        t = _f32(timesteps, dev)
        spk = _f32(speaker_emb, dev) if speaker_emb is not None else None
        with torch.cuda.device(dev):
            out = torch.empty_like(x)
            nb = lib.cmtts_denoiser_workspace_bytes(o._h, B, T)
            ws = o._ws.get("den", nb, dev)
            _lib.check(lib.cmtts_denoiser_forward(o._h, _ptr(x), _ptr(t), _ptr(cond_ct), _ptr(spk), B, T, _ptr(out),
                                                  _ptr(ws), nb, _stream()))
        return out


class KarrasDenoiser:
    """model/cm_tool/karras_diffusion.py:35-102,392-407 (inference members only)."""

    def __init__(self, sigma_data=0.5, sigma_max=80.0, sigma_min=0.002, rho=7.0, weight_schedule="karras",
                 distillation=False, loss_norm="lpips", **kw):
        """Same defaults as the reference (karras_diffusion.py:36-45: distillation=False); the synthesize path builds
        it with distillation=True (synthesize.py:59-78 via create_model_and_diffusion_tts)."""
        self.sigma_data, self.sigma_max, self.sigma_min, self.rho = sigma_data, sigma_max, sigma_min, rho
        self.weight_schedule, self.distillation, self.loss_norm = weight_schedule, distillation, loss_norm

    def get_scalings(self, sigma):
        """karras_diffusion.py:81-85 (distillation=False)."""
        c_skip = self.sigma_data ** 2 / (sigma ** 2 + self.sigma_data ** 2)
        c_out = sigma * self.sigma_data / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out, c_in

    def get_scalings_for_boundary_condition(self, sigma):
        c_skip = self.sigma_data ** 2 / ((sigma - self.sigma_min) ** 2 + self.sigma_data ** 2)
        c_out = (sigma - self.sigma_min) * self.sigma_data / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        return c_skip, c_out, c_in

    def denoise(self, model, x_t, sigmas, **model_kwargs):
        """Generic (unfused) form: host-side scalings around any model callable.  The fused
        path used by karras_sample_tts is cmtts_sample."""
        scal = self.get_scalings_for_boundary_condition if self.distillation else self.get_scalings
        c_skip, c_out, c_in = [v[(...,) + (None,) * (x_t.ndim - v.ndim)] for v in scal(sigmas)]
        rescaled_t = 1000 * 0.25 * torch.log(sigmas + 1e-44)
        model_output = model(c_in * x_t, rescaled_t, **model_kwargs)
        return model_output, c_out * model_output + c_skip * x_t


class DummyGenerator:
    """model/cm_tool/random_util.py:17-25."""

    def randn(self, *args, **kwargs):
        return torch.randn(*args, **kwargs)

    def randn_like(self, *args, **kwargs):
        return torch.randn_like(*args, **kwargs)


def _device_seeds(seeds, B, device):
    """`seeds` as int64 [B] on `device`: a tensor / array / sequence of B utterance seeds as it is, ONE int expanded with
    noise.utterance_seeds(int, arange(B))."""
    if isinstance(seeds, (int, np.integer)):
        seeds = _noise.utterance_seeds(int(seeds), np.arange(int(B)))
    if not isinstance(seeds, torch.Tensor):
        seeds = torch.from_numpy(np.ascontiguousarray(_noise._as_u64(seeds).view(np.int64)))
    if seeds.dtype != torch.int64 or tuple(seeds.shape) != (int(B),):
        raise ValueError(f"seeds: expected int64 [{int(B)}], got {seeds.dtype} {tuple(seeds.shape)}")
    return seeds.to(device=device).contiguous()


def seeded_noise(seeds, n_noise, T, n_mels=80, device="cuda:0", first_draw=0, t0=0):
    """The sampler's noise fp32 [n_noise, B, 1, T, n_mels] of the utterances with the int64 seeds [B] (cmtts_noise_fill, one
    launch): draws first_draw .. first_draw + n_noise - 1, frames t0 .. t0 + T - 1.  The value at (seed, draw, frame, mel bin) is
    a pure function of those four numbers (noise.py states it in numpy): a row does not depend on B, on its position or on T."""
    lib = _lib.load()
    dev = _norm_device(device)
    B = int(seeds.shape[0]) if hasattr(seeds, "shape") else len(seeds)
    sd = _device_seeds(seeds, B, dev)
    with torch.cuda.device(dev):
        out = torch.empty(int(n_noise), B, 1, int(T), int(n_mels), dtype=torch.float32, device=dev)
        _lib.check(lib.cmtts_noise_fill(_ptr(sd), B, int(T), int(n_mels), int(first_draw), int(n_noise), int(t0), _ptr(out), _stream()))
    return out


def seeded_noise_groups(groups, n_noise, n_mels=80, device="cuda:0", first_draw=0):
    """seeded_noise for every padded group of a ragged shard in one launch (cmtts_noise_fill_groups).
    groups: [(seeds int64 [B_g], T_g)] -> [noise [n_noise, B_g, 1, T_g, n_mels]]."""
    lib = _lib.load()
    dev = _norm_device(device)
    arr = (_lib.NoiseGroupStruct * len(groups))()
    outs, keep = [], []
    with torch.cuda.device(dev):
        for g, (seeds, T) in zip(arr, groups):
            B = int(seeds.shape[0]) if hasattr(seeds, "shape") else len(seeds)
            sd = _device_seeds(seeds, B, dev)
            out = torch.empty(int(n_noise), B, 1, int(T), int(n_mels), dtype=torch.float32, device=dev)
            g.seeds, g.B, g.T, g.out = sd.data_ptr(), B, int(T), out.data_ptr()
            keep.append(sd)
            outs.append(out)
        if outs:
            _lib.check(lib.cmtts_noise_fill_groups(arr, len(outs), int(n_mels), int(first_draw), int(n_noise), _stream()))
    return outs


class IndivGenerator:
    """model/cm_tool/random_util.py:97-182 ("determ-indiv"): noise that does not depend on the batch size or on the number of
    ranks — sample i of the run has its own stream, whichever batch and rank draws it.  Here sample i's stream is the seeded noise
    of noise.utterance_seeds(seed, [i]) and the k-th randn / randn_like call since set_done_samples is draw k of it (draw 0 is x_T,
    draw 1 + i the re-noise after evaluation i), generated on the device by cmtts_noise_fill.
    A tensor with first dimension n takes the samples done_samples + rank + k * world for k < n, clamped to num_samples - 1.
    Shapes: [n, 1, T, n_mels] or [n, T, n_mels] (the sampler's)."""

    def __init__(self, num_samples, seed=0, rank=None, world=None):
        if rank is None or world is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if on else 0) if rank is None else rank
            world = (dist.get_world_size() if on else 1) if world is None else world
        self.num_samples, self.seed, self.rank, self.world_size = int(num_samples), int(seed), int(rank), int(world)
        self.done_samples = 0
        self.draw = 0

    def get_size_and_indices(self, size):
        """random_util.py:119-129: (the size of one sample's tensor, the global sample index of every row)."""
        return (1, *size[1:]), _noise.indiv_indices(size[0], self.num_samples, self.done_samples, self.rank, self.world_size)

    def seeds_for(self, n):
        """int64 numpy [n]: the utterance seeds of the next n rows."""
        return _noise.utterance_seeds(self.seed, _noise.indiv_indices(n, self.num_samples, self.done_samples, self.rank, self.world_size))

    def randn(self, *size, dtype=torch.float, device="cpu"):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if dtype not in (torch.float, torch.float32):
            raise NotImplementedError("determ-indiv: float32 noise only")
        if len(size) < 3 or any(int(v) != 1 for v in size[1:-2]):
            raise NotImplementedError(f"determ-indiv: shape {tuple(size)}; the seeded noise is defined on [n, 1, T, n_mels] / [n, T, n_mels]")
        if _norm_device(device).type != "cuda":
            raise NotImplementedError("determ-indiv: the noise is generated on the GPU (cmtts_noise_fill); pass device=")
        z = seeded_noise(self.seeds_for(size[0]), 1, size[-2], size[-1], device, first_draw=self.draw)
        self.draw += 1
        return z.reshape(tuple(int(v) for v in size))

    def randn_like(self, tensor):
        return self.randn(*tensor.shape, dtype=tensor.dtype, device=tensor.device)

    def set_done_samples(self, done_samples):
        self.done_samples = int(done_samples)
        self.draw = 0

    def get_seed(self):
        return self.seed

    def set_seed(self, seed):
        self.seed = int(seed)
        self.draw = 0


def get_generator(generator, num_samples=0, seed=0):
    """model/cm_tool/random_util.py:6-14."""
    if generator == "dummy":
        return DummyGenerator()
    if generator == "determ-indiv":
        return IndivGenerator(num_samples, seed)
    if generator == "determ":
        raise NotImplementedError('generator "determ" draws num_samples full tensors from one stream and keeps this rank\'s rows of them '
                                  '(random_util.py:28-94): its cost grows with the run, not with the batch.  "determ-indiv" gives '
                                  "the same independence from batch size and world size per sample")
    raise NotImplementedError(generator)


def check_async_error():
    """Raise if a persistent denoiser launch that has completed reported a neighbour-wait timeout (cmtts_poll_error)."""
    _lib.check(_lib.load().cmtts_poll_error())


def synchronize(device=None):
    """torch.cuda.synchronize + cmtts_poll_error: a failure of any launch completed so far is raised HERE, by the call
    that makes the results host-visible, not by whichever call comes next."""
    torch.cuda.synchronize(device)
    check_async_error()


def _step_counts(n_steps, B, what):
    """None for an int (the uniform call), else the per-utterance step counts as a list of B ints."""
    if isinstance(n_steps, (int, np.integer)):
        return None
    if isinstance(n_steps, torch.Tensor):
        n_steps = n_steps.cpu().tolist()
    counts = [int(v) for v in n_steps]
    if len(counts) != B:
        raise ValueError(f"{what}: n_steps has {len(counts)} entries for a batch of {B}")
    return counts


def _take_rows(v, perm, B):
    """v with its utterance rows in the order perm: a tensor / array whose first dimension is B or a list of B entries; anything else
    (None, a number) as it is."""
    if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == B:
        return v[torch.as_tensor(perm, device=v.device)]
    if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B:
        return v[np.asarray(perm)]
    if isinstance(v, (list, tuple)) and len(v) == B:
        return type(v)(v[int(k)] for k in perm)
    return v


def _text_level_order(counts, B, seeds, what):
    """Per-utterance step counts of a text-level call: every count in {1, 2, 4}; returns (perm, inverse, sorted counts, seeds as a [B] array in the
    caller's order or None) — steps.order's stable permutation into non-increasing counts, applied before the duration net."""
    from . import steps as S
    if any(n not in (1, 2, 4) for n in counts):
        raise ValueError(f"{what}: every step count must be 1, 2 or 4 (synthesize.py:111-147), got {counts}")
    perm = S.order(counts)
    inv = np.argsort(perm, kind="stable")
    if isinstance(seeds, (int, np.integer)):          # one int names utterance b's seed by its position in the CALLER's order
        seeds = _noise.utterance_seeds(int(seeds), np.arange(int(B)))
    return perm, inv, [counts[int(k)] for k in perm], seeds


def sample_mixed(model: CMTotalTTS, cond_ct, speaker_emb, n_steps, noise=None, factors=None, seeds=None, sigmas=None, renoise_std=None,
                 out=None):
    """Per-utterance step counts in one batch (cmtts_sample_mixed; the definition: cmtts_amd/steps.py): utterance b takes n_steps[b]
    evaluations and comes out with the bits of its row in sample_with_cond(n_steps=n_steps[b]) on the same batch, but an utterance
    that has taken its last evaluation leaves — later evaluations run on the rest.  n_steps must be NON-INCREASING in b
    (ValueError otherwise: sort the batch with steps.order first).  sigmas / renoise_std: float32 [max_steps, B] per-utterance
    schedules (entry (i, b) is read where i < n_steps[b]; default: cmtts_schedule(n_steps[b]) per utterance).
    noise: fp32 [n_noise,B,1,T,80] with n_noise = max_steps + 1 (max_steps = 1: 1), or seeds as in sample_with_cond.
    out: a contiguous fp32 [B,T,80] device tensor to write (every row is written exactly once).  Returns mel [B,T,80]."""
    from . import steps as S
    model._require()
    lib, dev, cfg = model.lib, model.device, model.config
    B, H, T = cond_ct.shape
    counts = _step_counts(n_steps, B, "sample_mixed")
    if counts is None:
        raise ValueError("sample_mixed: n_steps must be a sequence (one int: sample_with_cond)")
    if (noise is None) == (seeds is None):
        raise ValueError("sample_mixed: give noise or seeds (one of them)")
    if (sigmas is None) != (renoise_std is None):
        raise ValueError("sample_mixed: give sigmas and renoise_std together")
    S.validate(counts)          # ValueError names steps.order
    NS = counts[0]
    if sigmas is None:
        sig = np.zeros((NS, B), np.float32)
        std = np.zeros((NS, B), np.float32)
        for n in sorted(set(counts)):
            a, d = (C.c_float * n)(), (C.c_float * n)()
            _lib.check(lib.cmtts_schedule(model._h, n, a, d))
            cols = [b for b in range(B) if counts[b] == n]
            sig[:n, cols] = np.asarray(a[:], np.float32)[:, None]
            std[:n, cols] = np.asarray(d[:], np.float32)[:, None]
    else:
        sig = np.ascontiguousarray(np.asarray(sigmas, np.float32))
        std = np.ascontiguousarray(np.asarray(renoise_std, np.float32))
        S.validate(counts, sig, std)
    ns = np.asarray(counts, np.int32)
    plan = _lib.StepPlanStruct(NS, ns.ctypes.data, sig.ctypes.data, std.ctypes.data)
    if seeds is not None:
        seeds = _device_seeds(seeds, B, dev)
    else:
        n_noise = 1 if not (std[np.arange(NS)[:, None] < ns[None, :]] >= 0).any() else NS + 1
        assert noise.shape[0] >= n_noise and tuple(noise.shape[1:]) == (B, 1, T, cfg.n_mels)
    with torch.cuda.device(dev):
        mel = torch.empty(B, T, cfg.n_mels, dtype=torch.float32, device=dev) if out is None else out
        if mel.dtype != torch.float32 or tuple(mel.shape) != (B, T, cfg.n_mels) or not mel.is_contiguous() or mel.device != torch.device(dev):
            raise ValueError(f"sample_mixed: out must be a contiguous float32 [{B}, {T}, {cfg.n_mels}] tensor on {dev}")
        nb = lib.cmtts_sample_mixed_workspace_bytes(model._h, B, T, NS)
        ws = model._ws.get("den_mixed", nb, dev)
        if factors is None:
            factors = getattr(cond_ct, "_cmtts_factors", None)
        f = factors if factors is not None and factors.matches(cond_ct) else None
        _lib.check(lib.cmtts_sample_mixed(model._h, _ptr(seeds), _ptr(noise), _ptr(cond_ct), _ptr(speaker_emb), B, T, C.byref(plan),
                                          _ptr(mel), _ptr(ws), nb, _stream(), _ptr(f.p1 if f else None), _ptr(f.p1t if f else None),
                                          f.p1_ld if f else 0, f.L if f else 0, _ptr(f.mel2ph if f else None), _ptr(f.p_idx if f else None)))
    return mel


def sample_with_cond(model: CMTotalTTS, cond_ct, speaker_emb, n_steps, noise=None, factors=None, seeds=None):
    """T-step consistency sampling on precomputed conditioning (cmtts_sample).
    n_steps: an int, or a sequence of B per-utterance step counts, non-increasing (sample_mixed: cmtts_sample_mixed).
    noise: fp32 [n_noise,B,1,T,80] on device.  factors: the duration net's out["cond_factors"] for THIS cond_ct (default: the ones the
    duration net attached to the tensor object it returned; the conditioner projections are then expanded from them,
    cmtts_sample_factored — an unmodified, same-storage cond_ct only, else the dense GEMM).  Returns mel [B,T,80].
    seeds (in place of noise): int64 [B] utterance seeds, or one int (noise.utterance_seeds(int, arange(B))) — the sampler
    generates the seeded noise itself (cmtts_sample_seeded: no noise tensor for x_T, one launch for the re-noise draws); the mel
    has the bits of noise=seeded_noise(seeds, n_noise, T)."""
    model._require()
    lib, dev, cfg = model.lib, model.device, model.config
    B, H, T = cond_ct.shape
    if _step_counts(n_steps, B, "sample_with_cond") is not None:
        return sample_mixed(model, cond_ct, speaker_emb, n_steps, noise, factors, seeds)
    n_noise = 1 if n_steps == 1 else n_steps + 1
    if (noise is None) == (seeds is None):
        raise ValueError("sample_with_cond: give noise or seeds (one of them)")
    if seeds is not None:
        return _sample_seeded(model, cond_ct, speaker_emb, n_steps, _device_seeds(seeds, B, dev), factors)
    assert noise.shape[0] >= n_noise and tuple(noise.shape[1:]) == (B, 1, T, cfg.n_mels)
    sig = (C.c_float * n_steps)()
    std = (C.c_float * n_steps)()
    _lib.check(lib.cmtts_schedule(model._h, n_steps, sig, std))
    with torch.cuda.device(dev):
        mel = torch.empty(B, T, cfg.n_mels, dtype=torch.float32, device=dev)
        nb = lib.cmtts_denoiser_workspace_bytes(model._h, B, T)
        ws = model._ws.get("den", nb, dev)
        if factors is None:
            factors = getattr(cond_ct, "_cmtts_factors", None)
        if factors is not None and factors.matches(cond_ct):
            _lib.check(lib.cmtts_sample_factored_t(model._h, _ptr(noise), _ptr(cond_ct), _ptr(speaker_emb), B, T, n_steps, sig, std,
                                                   _ptr(mel), _ptr(ws), nb, _stream(), _ptr(factors.p1), _ptr(factors.p1t), factors.p1_ld, factors.L,
                                                   _ptr(factors.mel2ph), _ptr(factors.p_idx)))
        else:
            _lib.check(lib.cmtts_sample(model._h, _ptr(noise), _ptr(cond_ct), _ptr(speaker_emb), B, T, n_steps, sig, std,
                                        _ptr(mel), _ptr(ws), nb, _stream()))
    return mel


def _sample_seeded(model, cond_ct, speaker_emb, n_steps, seeds, factors):
    lib, dev, cfg = model.lib, model.device, model.config
    B, H, T = cond_ct.shape
    sig = (C.c_float * n_steps)()
    std = (C.c_float * n_steps)()
    _lib.check(lib.cmtts_schedule(model._h, n_steps, sig, std))
    with torch.cuda.device(dev):
        mel = torch.empty(B, T, cfg.n_mels, dtype=torch.float32, device=dev)
        nb = lib.cmtts_sample_seeded_workspace_bytes(model._h, B, T, n_steps)
        ws = model._ws.get("den_seeded", nb, dev)
        if factors is None:
            factors = getattr(cond_ct, "_cmtts_factors", None)
        f = factors if factors is not None and factors.matches(cond_ct) else None
        _lib.check(lib.cmtts_sample_seeded(model._h, _ptr(seeds), _ptr(cond_ct), _ptr(speaker_emb), B, T, n_steps, sig, std,
                                           _ptr(mel), _ptr(ws), nb, _stream(), _ptr(f.p1 if f else None), _ptr(f.p1t if f else None),
                                           f.p1_ld if f else 0, f.L if f else 0, _ptr(f.mel2ph if f else None), _ptr(f.p_idx if f else None)))
    return mel


def _draw_sampler_noise(gen, B, T, n_mels, draws, device):
    """The sampler's noise from a generator: x0 = randn, then randn_like(x0) per further draw; an IndivGenerator gives the same
    bits in one fill."""
    if isinstance(gen, IndivGenerator):
        noise = seeded_noise(gen.seeds_for(B), draws, T, n_mels, device, first_draw=gen.draw)
        gen.draw += draws
        return noise
    x0 = gen.randn(B, 1, T, n_mels, device=device)
    return torch.stack([x0] + [gen.randn_like(x0) for _ in range(draws - 1)], 0).float()


def sample_ragged(model: CMTotalTTS, groups, n_steps, tail_frames=0):
    """cmtts_sample_ragged: T-step consistency sampling of a RAGGED shard — every group a padded (B, T) batch with its own
    conditioning, results those of sample_with_cond on that batch — with the residual layers of ALL groups in one persistent
    launch per evaluation (buckets too small to fill the chip fill it together).
    groups: iterable of (cond_ct [B,H,T], speaker_emb [B,H] | None, noise [n_noise,B,1,T,80], active_frames | None[, CondFactors | None]);
    active_frames = host sequence of B ints (mel_len): the utterance is then only computed as far as those frames (+ tail_frames
    + the sampler's receptive field) need — they come out bit-identical to the untrimmed run in the direct and F(2,3) forms of the
    stack and within fp32 rounding of it (<= 1.5e-5: include/cmtts_hip.h, tests/conftest.py WINO_TRIM_TOL; ~2e-6 typical) in the default F(4,3) form, whose frame quads round every output from all
    six inputs of the quad; frames beyond the computed range are zeros.
    Returns the list of mels [B,T,80]."""
    if not isinstance(n_steps, (int, np.integer)):
        raise NotImplementedError("sample_ragged: per-utterance step counts are not supported on a ragged shard (one int; "
                                  "sample_with_cond takes a sequence on a padded batch)")
    model._require()
    lib, dev, cfg = model.lib, model.device, model.config
    n_noise = 1 if n_steps == 1 else n_steps + 1
    sig = (C.c_float * n_steps)()
    std = (C.c_float * n_steps)()
    _lib.check(lib.cmtts_schedule(model._h, n_steps, sig, std))
    groups = list(groups)
    arr = (_lib.SampleGroupStruct * len(groups))()
    mels, keep = [], []
    with torch.cuda.device(dev):
        for gi, grp in enumerate(groups):
            cond_ct, spk, noise, active = grp[:4]
            factors = grp[4] if len(grp) > 4 else None
            B, H, T = cond_ct.shape
            assert noise.shape[0] >= n_noise and tuple(noise.shape[1:]) == (B, 1, T, cfg.n_mels)
            mel = torch.empty(B, T, cfg.n_mels, dtype=torch.float32, device=dev)
            nb = lib.cmtts_denoiser_workspace_bytes(model._h, B, T)
            ws = model._ws.get(("den_ragged", gi), nb, dev)
            g = arr[gi]
            g.noise, g.cond_ct, g.speaker_emb = noise.data_ptr(), cond_ct.data_ptr(), (spk.data_ptr() if spk is not None else None)
            g.B, g.T, g.mel, g.ws, g.ws_bytes = B, T, mel.data_ptr(), ws.data_ptr(), nb
            if active is not None:
                act = (C.c_int64 * B)(*[int(v) for v in active])
                keep.append(act)
                g.active_frames = C.cast(act, C.c_void_p).value
            if factors is not None and factors.matches(cond_ct):
                g.cond_p1, g.p1_ld, g.L = factors.p1.data_ptr(), factors.p1_ld, factors.L
                g.mel2ph, g.p_idx = factors.mel2ph.data_ptr(), factors.p_idx.data_ptr()
                keep.append(factors)
            mels.append(mel)
            keep += [cond_ct, spk, noise, ws]
        _lib.check(lib.cmtts_sample_ragged(model._h, arr, len(groups), n_steps, sig, std, int(tail_frames), _stream()))
    return mels


def karras_sample_tts(diffusion, model, shape, steps=2, clip_denoised=False, progress=False, callback=None,
                      model_kwargs=None, device=None, sigma_min=0.002, sigma_max=80, rho=7.0, sampler="onestep",
                      generator=None, ts=None, **unused):
    """karras_diffusion.py:480-577.  "onestep" and "multistep" with steps=2, ts=(0,)*T+(1,) (what
    synthesize.py selects) run fused in cmtts_sample; "heun", "dpm", "euler", "ancestral", "our_multistep", any
    other multistep `ts` schedule, and everything under a diffusion with distillation=False (get_scalings instead of
    the boundary-condition scalings) run the reference's loops host-side around the denoiser kernels (s_churn,
    s_tmin, s_tmax, s_noise, T as keywords).  The duration net runs once (bit-identical to the reference's
    per-evaluation re-run) with max_mel_len = shape[2]."""
    if generator is None:
        generator = DummyGenerator()
    B, one, T, M = shape
    ode = sampler in ("heun", "dpm", "euler", "ancestral", "our_multistep", "progdist")
    distilled = getattr(diffusion, "distillation", False)
    # cmtts_schedule / cmtts_sample take sigma_min, sigma_max, sigma_data and rho from the model's config; a caller
    # whose arguments or diffusion object say otherwise gets the reference's host-side loop, which honours them
    cfg = model.config
    same = lambda a, b: abs(float(a) - float(b)) <= 1e-6 * max(abs(float(a)), abs(float(b)), 1e-30)
    if not (same(sigma_min, cfg.sigma_min) and same(sigma_max, cfg.sigma_max) and
            same(getattr(diffusion, "sigma_min", cfg.sigma_min), cfg.sigma_min) and
            same(getattr(diffusion, "sigma_max", cfg.sigma_max), cfg.sigma_max) and
            same(getattr(diffusion, "sigma_data", cfg.sigma_data), cfg.sigma_data) and
            same(getattr(diffusion, "rho", cfg.rho), cfg.rho)):
        distilled_fusable = False
    else:
        distilled_fusable = distilled
    if sampler == "onestep":
        n_steps = 1
        ode = not distilled_fusable    # cmtts_sample fuses the boundary-condition scalings (and the config's sigmas) only
    elif sampler == "multistep":
        fused = distilled_fusable and steps == 2 and ts is not None and tuple(ts[:-1]) == (0,) * (len(ts) - 1) and ts[-1] == 1
        n_steps = len(ts) - 1 if fused else 0
        ode = not fused                # any other `ts` schedule: the reference's loop, host-side
    elif not ode:
        raise KeyError(sampler)          # the reference's dispatch table has no other entry (karras_diffusion.py:536-545)
    dev = model.device
    kw = dict(model_kwargs or {})
    out = model.duration_pitch_energy_net(kw.get("speakers"), kw["texts"], kw["src_lens"],
                                          spker_embeds=kw.get("spker_embeds"), max_mel_len=T)
    if ode:
        # the reference's other loops (karras_diffusion.py:538-577), host-side around the denoiser kernels
        sigmas = get_sigmas_karras(steps + 1 if sampler == "progdist" else steps, sigma_min, sigma_max, rho)     # karras_diffusion.py:529-532
        x_T = _f32(generator.randn(*shape, device=dev), dev) * sigma_max
        dist = make_distiller(diffusion, model, out_cond(out), out["speaker_emb"])
        fn = {"heun": sample_heun, "dpm": sample_dpm, "euler": sample_euler, "ancestral": sample_euler_ancestral,
              "our_multistep": our_multistep, "onestep": sample_onestep, "multistep": stochastic_iterative_sampler,
              "progdist": sample_progdist}[sampler]
        args = {}
        if sampler in ("heun", "dpm"):
            args = {k: unused[k] for k in ("s_churn", "s_tmin", "s_tmax", "s_noise") if k in unused}
        elif sampler == "our_multistep":
            args = {"T": unused.get("T", 4)}
        elif sampler == "multistep":
            args = dict(ts=ts, t_min=sigma_min, t_max=sigma_max, rho=diffusion.rho, steps=steps)
        return fn(dist, x_T, sigmas, generator, **args)[:, 0]
    draws = [generator.randn(*shape, device=dev)]
    for _ in range(n_steps if n_steps > 1 else 0):
        draws.append(generator.randn_like(draws[0]))
    noise = torch.stack([_f32(d, dev) for d in draws], 0)
    return sample_with_cond(model, out["cond_ct"], out["speaker_emb"], n_steps, noise, factors=out.get("cond_factors"))


def out_cond(out):
    """[B,T,H] view of the duration net's channel-major conditioning (what CMDenoiserTTS.forward takes)."""
    return out["cond_ct"].transpose(1, 2)


def get_sigmas_karras(n, sigma_min, sigma_max, rho=7.0, device="cpu"):
    """karras_diffusion.py:580-586 (fp32, trailing 0).  Kept on the host: the loops branch on its values."""
    ramp = torch.linspace(0, 1, n)
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return torch.cat([(hi + ramp * (lo - hi)) ** rho, torch.zeros(1)])


def to_d(x, sigma, denoised):
    """karras_diffusion.py:589-591."""
    return (x - denoised) / float(sigma)


def get_ancestral_step(sigma_from, sigma_to):
    """karras_diffusion.py:594-601."""
    sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


def sample_euler(denoiser, x, sigmas, generator=None, **kw):
    """karras_diffusion.py:743-771."""
    s_in = x.new_ones([x.shape[0]])
    for i in range(len(sigmas) - 1):
        d = to_d(x, sigmas[i], denoiser(x, float(sigmas[i]) * s_in))
        x = x + d * float(sigmas[i + 1] - sigmas[i])
    return x


def sample_euler_ancestral(denoiser, x, sigmas, generator, **kw):
    """karras_diffusion.py:605-632."""
    s_in = x.new_ones([x.shape[0]])
    for i in range(len(sigmas) - 1):
        denoised = denoiser(x, float(sigmas[i]) * s_in)
        sigma_down, sigma_up = get_ancestral_step(sigmas[i], sigmas[i + 1])
        d = to_d(x, sigmas[i], denoised)
        x = x + d * float(sigma_down - sigmas[i])
        x = x + generator.randn_like(x) * float(sigma_up)
    return x


def _churn(x, sigmas, i, generator, s_churn, s_tmin, s_tmax, s_noise):
    gamma = min(s_churn / (len(sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sigmas[i] <= s_tmax else 0.0
    eps = generator.randn_like(x) * s_noise          # drawn every iteration, like the reference
    sigma_hat = sigmas[i] * (gamma + 1)
    if gamma > 0:
        x = x + eps * float((sigma_hat ** 2 - sigmas[i] ** 2) ** 0.5)
    return x, sigma_hat


def sample_progdist(denoiser, x, sigmas, generator=None, **kw):
    """karras_diffusion.py:856-888: Euler steps over the schedule WITHOUT its trailing zero (the progressive-distillation teacher's
    sampler; `steps + 1` sigmas are requested for it, :529-530)."""
    s_in = x.new_ones([x.shape[0]])
    sigmas = sigmas[:-1]
    for i in range(len(sigmas) - 1):
        d = to_d(x, sigmas[i], denoiser(x, float(sigmas[i]) * s_in))
        x = x + d * float(sigmas[i + 1] - sigmas[i])
    return x


def sample_heun(denoiser, x, sigmas, generator, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, **kw):
    """karras_diffusion.py:693-739 (Algorithm 2 of Karras et al. 2022)."""
    s_in = x.new_ones([x.shape[0]])
    for i in range(len(sigmas) - 1):
        x, sigma_hat = _churn(x, sigmas, i, generator, s_churn, s_tmin, s_tmax, s_noise)
        d = to_d(x, sigma_hat, denoiser(x, float(sigma_hat) * s_in))
        dt = float(sigmas[i + 1] - sigma_hat)
        if sigmas[i + 1] == 0:
            x = x + d * dt
        else:
            x_2 = x + d * dt
            d_2 = to_d(x_2, sigmas[i + 1], denoiser(x_2, float(sigmas[i + 1]) * s_in))
            x = x + (d + d_2) / 2 * dt
    return x


def sample_dpm(denoiser, x, sigmas, generator, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, **kw):
    """karras_diffusion.py:775-820 (midpoint on a rho=3 schedule)."""
    s_in = x.new_ones([x.shape[0]])
    for i in range(len(sigmas) - 1):
        x, sigma_hat = _churn(x, sigmas, i, generator, s_churn, s_tmin, s_tmax, s_noise)
        d = to_d(x, sigma_hat, denoiser(x, float(sigma_hat) * s_in))
        sigma_mid = ((sigma_hat ** (1 / 3) + sigmas[i + 1] ** (1 / 3)) / 2) ** 3
        x_2 = x + d * float(sigma_mid - sigma_hat)
        d_2 = to_d(x_2, sigma_mid, denoiser(x_2, float(sigma_mid) * s_in))
        x = x + d_2 * float(sigmas[i + 1] - sigma_hat)
    return x


def sample_onestep(distiller, x, sigmas, generator=None, **kw):
    """karras_diffusion.py:801-811 on the generic (unfused) denoise callable."""
    return distiller(x, sigmas[0] * x.new_ones([x.shape[0]]))


def our_multistep(distiller, x, sigmas, generator=None, T=4, **kw):
    """karras_diffusion.py:814-826: T evaluations at sigma_max without re-noising."""
    s_in = x.new_ones([x.shape[0]])
    for _ in range(T):
        x = distiller(x, sigmas[0] * s_in)
    return x


def stochastic_iterative_sampler(distiller, x, sigmas, generator, ts, t_min=0.002, t_max=80.0, rho=7.0, steps=40, **kw):
    """karras_diffusion.py:830-854, any `ts` schedule, on the generic denoise callable (SURVEY.md §8f item 3:
    host-side loops around the same denoiser kernels; the fused cmtts_sample covers synthesize.py's cases)."""
    t_max_rho, t_min_rho = t_max ** (1 / rho), t_min ** (1 / rho)
    s_in = x.new_ones([x.shape[0]])
    for i in range(len(ts) - 1):
        t = (t_max_rho + ts[i] / (steps - 1) * (t_min_rho - t_max_rho)) ** rho
        x0 = distiller(x, t * s_in)
        next_t = (t_max_rho + ts[i + 1] / (steps - 1) * (t_min_rho - t_max_rho)) ** rho
        next_t = float(np.clip(next_t, t_min, t_max))
        x = x0 + generator.randn_like(x) * np.sqrt(next_t ** 2 - t_min ** 2) * 0.85
    return x


def make_distiller(diffusion: "KarrasDenoiser", model: CMTotalTTS, cond, speaker_emb):
    """denoiser(x_t, sigma) closure of karras_sample_tts (karras_diffusion.py:561-566) over precomputed
    conditioning: KarrasDenoiser.denoise around CMDenoiserTTS.forward."""
    def distiller(x_t, sigma):
        return diffusion.denoise(lambda xx, tt: model.net(xx, tt, cond, speaker_emb), x_t, sigma)[1]
    return distiller


class Generator(torch.nn.Module):
    """hifigan/models.py:112-174 — HiFi-GAN V1 generator; forward(x [B,80,T]) -> [B,1,256*T]."""

    def __init__(self, h: HifiGanConfig = HifiGanConfig(), device="cuda:0"):
        super().__init__()
        self.h = h
        self.device = _norm_device(device) if torch.cuda.is_available() else torch.device(device)
        self.lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self.lib.cmtts_vocoder_create(C.byref(self._h)))
        self._ready = False
        self._ws = _Workspace()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:
            self.lib.cmtts_vocoder_destroy(h)
            self._h = None

    def load_state_dict(self, state_dict, strict=True):
        """Accepts plain weights or weight_g/weight_v pairs (folded like remove_weight_norm)."""
        from .weights import fold_weight_norm
        sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in state_dict.items()}
        if any(k.endswith("weight_g") for k in sd):
            sd = fold_weight_norm(sd)
        _push_state_dict(self.lib, self.lib.cmtts_vocoder_set_tensor, self._h, sd)
        self._pending = True
        if self.device.type == "cuda" and torch.cuda.is_available():
            self._finalize()
        return self

    def _finalize(self):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cmtts_vocoder_finalize(self._h))
        self._pending = False
        self._ready = True

    def remove_weight_norm(self):
        return self

    def set_precision(self, dtype="fp32"):
        """Operand precision of the ResBlock convs: "fp32" (reference), "bf16", "fp16", or "fp16x3" (operands as hi + lo fp16
        pairs, three fp16 MFMAs per product, fp32 accumulate: fp32-class results, activations stay fp32 in HBM)."""
        mode = {"fp32": 0, "f32": 0, "bf16": 1, "fp16": 2, "f16": 2, "fp16x3": 3}[dtype]
        _lib.check(self.lib.cmtts_vocoder_set_precision(self._h, mode))
        return self

    def set_option(self, name, value):
        """Per-vocoder numerics option (cmtts_vocoder_set_option): "ups16" 1 (default) | 0 — in the 16-bit modes the upsamplers
        take 16-bit operands too, or stay fp32.  Returns the previous value.  "winograd" 1 (default) | 0 — fp32 generator, large batches: the ResBlock convs of the C >= 128 stages as Winograd
        convolutions (4 / 10 / 15 products per output pair instead of 6 / 14 / 22; <= 1.2e-6 on the waveform) or in the direct form.  "batch_invariant"
        0 (default) | 1 — fp32 generator: the large-launch forms at every launch size, so a row's waveform does not depend on the batch."""
        prev = self.lib.cmtts_vocoder_set_option(self._h, name.encode() if isinstance(name, str) else name, int(value))
        if prev < 0:
            _lib.check(prev)
        return prev

    def eval(self):
        return self

    def _require(self):
        if not self._ready and getattr(self, "_pending", False):
            if not torch.cuda.is_available():
                raise RuntimeError("Generator: no GPU — cmtts_amd has no CPU fallback (the weights are loaded, the kernels cannot run)")
            self.device = _norm_device(self.device if self.device.type == "cuda" else "cuda")
            self._finalize()
        if not self._ready:
            raise RuntimeError("Generator: load_state_dict() first")

    def forward(self, x):
        self._require()
        dev = self.device
        x = _f32(x, dev)
        B, M, T = x.shape
        with torch.cuda.device(dev):
            wav = torch.empty(B, 1, T * self.h.hop, dtype=torch.float32, device=dev)
            nb = self.lib.cmtts_vocoder_workspace_bytes(self._h, B, T)
            ws = self._ws.get("voc", nb, dev)
            _lib.check(self.lib.cmtts_vocoder_forward(self._h, _ptr(x), B, T, _ptr(wav), _ptr(ws), nb, _stream()))
        return wav


def vocoder_infer_device(mels, vocoder, max_wav_value=32768.0):
    """The device half of vocoder_infer (utils/model.py:187-198): mels [B,80,T] -> int16 PCM [B, T*hop] still on the GPU
    (what shard.allgather_pcm collates across ranks before anything crosses PCIe)."""
    wavs = vocoder(mels).squeeze(1)
    pcm = torch.empty(wavs.shape, dtype=torch.int16, device=wavs.device)
    with torch.cuda.device(wavs.device):
        _lib.check(vocoder.lib.cmtts_wav_to_int16(_ptr(wavs), _ptr(pcm), wavs.numel(), float(max_wav_value), _stream()))
    return pcm


class _Resampler:
    """One (L, M) resampler of a vocoder: the float32 taps of cmtts_amd.resample.design_taps handed to cmtts_resampler_create."""

    def __init__(self, lib, device, L, M, identity=False):
        from . import resample as rs
        self.lib, self.L, self.M = lib, L, M
        # identity (L = M = 1 only): the single tap 1.0 — y = x, what a gain at the native rate rides on without filtering anything
        self.taps, self.half = (np.ones(1, np.float32), 0) if identity else rs.design_taps(L, M)
        self.R = rs.half_width(L, self.half)
        self._h = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(lib.cmtts_resampler_create(L, M, self.taps.ctypes.data_as(C.c_void_p), self.half, C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:
            self.lib.cmtts_resampler_destroy(h)
            self._h = None

    def out_len(self, n):
        return -(-int(n) * self.L // self.M)


def _output_format(vocoder, sample_rate, encoding, force=False):
    """None for the native format (the vocoder's rate, "s16": the existing path, wrap included), else (resampler, encoding code,
    torch dtype).  The filter of a rate is designed once per vocoder (cmtts_amd.resample.design_taps).  force: the float path for the
    native format too — what a gain rides on; at the native rate it is the L = M = 1 resampler with the single tap 1.0, which filters
    nothing (the output is the encoding of fl32(g x); "s16" then saturates)."""
    from . import resample as rs
    if encoding not in rs.ENCODINGS:
        raise ValueError(f"encoding {encoding!r}: expected one of {sorted(rs.ENCODINGS)}")
    native = rs.NATIVE_RATE
    rate = native if sample_rate is None else int(sample_rate)
    if rate == native and encoding == "s16" and not force:
        return None
    L, M = rs.ratio(native, rate)
    cache = vocoder.__dict__.setdefault("_resamplers", {})
    key = (L, M, "identity") if force and rate == native else (L, M)
    if key not in cache:
        cache[key] = _Resampler(vocoder.lib, vocoder.device, L, M, identity=len(key) == 3)
    dtype = {"f32": torch.float32, "s16": torch.int16, "mulaw": torch.uint8, "alaw": torch.uint8}[encoding]
    return cache[key], rs.ENCODINGS[encoding], dtype


def _resample_encode(lib, rsm, wav, seg_tab, enc, dtype, max_wav_value, out_ld, gains=None):
    """cmtts_resample_encode on the current stream: wav fp32 [rows, ld] (device), seg_tab int32 [N, 5] (pinned host or device).
    gains: fp32 [rows] (device), one per source row — cmtts_resample_encode_gain."""
    N = seg_tab.shape[0]
    out = torch.empty(N, out_ld, dtype=dtype, device=wav.device)
    if gains is None:
        _lib.check(lib.cmtts_resample_encode(rsm._h, _ptr(wav), wav.shape[0], wav.shape[1], _ptr(seg_tab), N, enc, float(max_wav_value),
                                             _ptr(out), out_ld, _stream()))
    else:
        assert gains.dtype == torch.float32 and gains.is_contiguous() and gains.numel() == wav.shape[0]
        _lib.check(lib.cmtts_resample_encode_gain(rsm._h, _ptr(wav), wav.shape[0], wav.shape[1], _ptr(seg_tab), N, enc,
                                                  float(max_wav_value), _ptr(out), out_ld, _ptr(gains), _stream()))
    return out


# ----------------------------------------------------------------------------- loudness and output gain

def _per_utterance(what, value, B):
    """A number or [B] values -> float64 numpy [B]."""
    v = np.asarray(value.detach().cpu().numpy() if torch.is_tensor(value) else value, dtype=np.float64)
    if v.ndim == 0:
        return np.full(B, float(v))
    if v.shape != (B,):
        raise ValueError(f"{what}: expected a number or {B} values, got shape {tuple(v.shape)}")
    return v


def _linear_gains(what, gain_db, B, device):
    """gain_db (a number or [B]) -> fp32 [B] linear gains on the device: 10^(gain_db / 20) in float64, rounded once."""
    g = _per_utterance(what, gain_db, B)
    if not np.isfinite(g).all():
        raise ValueError(f"{what}: gain_db must be finite")
    return torch.from_numpy((10.0 ** (g / 20.0)).astype(np.float32)).to(device)


def _measure_loudness(vocoder, wavs, lens, target=None, peak_ceiling_db=-1.0):
    """cmtts_loudness_measure on the current stream: wavs fp32 [B, n] (device), lens valid samples per row, target None or float64 [B]
    (NaN: measure only) -> stats fp32 [B, 4] on the device (L, sample peak, linear gain, gated blocks).  No synchronisation."""
    from . import resample as rs
    lib, dev = vocoder.lib, wavs.device
    B, n = wavs.shape
    n_valid = torch.tensor([int(v) for v in lens], dtype=torch.int32).to(dev)
    tgt = None if target is None else torch.from_numpy(np.asarray(target, np.float32)).to(dev)
    stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
    nb = lib.cmtts_loudness_workspace_bytes(B, n, rs.NATIVE_RATE)
    ws = vocoder._ws.get("loudness", max(nb, 1), dev)
    _lib.check(lib.cmtts_loudness_measure(_ptr(wavs), B, n, _ptr(n_valid), rs.NATIVE_RATE, None if tgt is None else _ptr(tgt),
                                          float(peak_ceiling_db), _ptr(stats), _ptr(ws), nb, _stream()))
    return stats


def _clip_lengths(lengths, B, n):
    return [n] * B if lengths is None else [min(max(int(v), 0), n) for v in lengths]


def _append_stats(stats, st, gains):
    """One dict per utterance from the device stats [B, 4]; gains: the fixed gains applied instead of the measured ones, or None."""
    st = st.cpu().numpy()
    g = st[:, 2] if gains is None else gains.cpu().numpy()
    for b, (L, pk, _, nblk) in enumerate(st):
        stats.append({"lufs": float(L), "peak": float(pk), "gain_db": 20.0 * math.log10(float(g[b])), "blocks": int(nblk)})


def vocoder_loudness(mels, vocoder, lengths=None):
    """Integrated loudness (ITU-R BS.1770; the definition: cmtts_amd.loudness) of what vocoder_infer would deliver, measured on the
    device: mels [B,80,T] -> float32 numpy [B, 4] = (L in LKFS, sample peak, 1.0, gated blocks) per utterance; `lengths` counts
    samples as vocoder_infer's.  It only measures — the generator, then cmtts_loudness_measure: the way to calibrate a voice once and
    pass a fixed gain_db afterwards (a stream cannot know its integrated loudness before it ends)."""
    wavs = vocoder(mels).squeeze(1)
    B, n = wavs.shape
    with torch.cuda.device(wavs.device):
        stats = _measure_loudness(vocoder, wavs, _clip_lengths(lengths, B, n))
    out = stats.cpu().numpy()
    check_async_error()
    return out


def vocoder_infer(mels, vocoder, model_config=None, preprocess_config=None, lengths=None, max_wav_value=32768.0,
                  sample_rate=None, encoding="s16", loudness=None, peak_ceiling_db=-1.0, gain_db=None, stats=None):
    """utils/model.py:187-205: mels [B,80,T] -> list of int16 numpy arrays trimmed to `lengths`.
    sample_rate / encoding: another output rate (8000, 16000, 24000, 32000, 44100, 48000) and / or "f32", "s16",
    "mulaw", "alaw" — resampled and encoded on the device by one cmtts_resample_encode after the unchanged generator; `lengths` still
    counts SOURCE samples, row b comes back with ceil(lengths[b] * L / M) samples of dtype float32 / int16 / uint8, and "s16" saturates.
    The defaults (None or the native 22 050 Hz, "s16") are the reference's cast, wrap included.
    loudness / gain_db (give one, not both): a target in LUFS resp. a fixed gain in dB, a number or [B] values.
    loudness measures every utterance's integrated loudness (BS.1770, over its `lengths` samples) on the device after the generator and
    scales it to the target, with the SAMPLE peak kept at or under peak_ceiling_db dBFS (no true-peak oversampling: a resampled wave can
    still overshoot between samples, which the saturating encoders absorb); NaN leaves that utterance alone.  Either one takes the
    float path for every format — the gain is one fp32 multiplication per source sample in cmtts_resample_encode_gain's staging, the
    native rate runs the L = M = 1 resampler with the single tap 1.0 (no filtering: the encoding of fl32(g x)) and "s16" saturates.  stats: a list that receives one dict per utterance: "lufs" (before
    the gain; -inf for silence), "peak", "gain_db" (passing these as gain_db reproduces the output bit for bit), "blocks"."""
    if preprocess_config is not None:
        max_wav_value = preprocess_config["preprocessing"]["audio"]["max_wav_value"]
    if loudness is not None and gain_db is not None:
        raise ValueError("vocoder_infer: give loudness (a target in LUFS) or gain_db (a fixed gain), not both")
    if stats is not None and not isinstance(stats, list):
        raise ValueError("vocoder_infer: stats must be a list")
    leveled = loudness is not None or gain_db is not None
    fmt = _output_format(vocoder, sample_rate, encoding, force=leveled)
    if fmt is not None:
        rsm, enc, dtype = fmt
        wavs = vocoder(mels).squeeze(1)
        B, n = wavs.shape
        lens = _clip_lengths(lengths, B, n)
        tab = torch.tensor([(b, 0, 0, rsm.out_len(lens[b]), lens[b]) for b in range(B)], dtype=torch.int32).pin_memory()
        with torch.cuda.device(wavs.device):
            gains = st = None
            if loudness is not None:
                target = _per_utterance("vocoder_infer: loudness", loudness, B)
                st = _measure_loudness(vocoder, wavs, lens, target, peak_ceiling_db)
                gains = st[:, 2].contiguous()
            elif gain_db is not None:
                gains = _linear_gains("vocoder_infer: gain_db", gain_db, B, wavs.device)
            if stats is not None and st is None:
                st = _measure_loudness(vocoder, wavs, lens)
            out = _resample_encode(vocoder.lib, rsm, wavs, tab, enc, dtype, max_wav_value, max(rsm.out_len(n), 1), gains)
        arr = out.cpu().numpy()          # synchronises: the pinned table is free again
        check_async_error()
        if stats is not None:
            _append_stats(stats, st, None if gain_db is None else gains)
        return [arr[b, : rsm.out_len(lens[b])] for b in range(B)]
    if stats is not None:          # the native format, measured but not scaled: vocoder_infer_device's two calls around the measurement
        wavs = vocoder(mels).squeeze(1)
        pcm = torch.empty(wavs.shape, dtype=torch.int16, device=wavs.device)
        with torch.cuda.device(wavs.device):
            st = _measure_loudness(vocoder, wavs, _clip_lengths(lengths, *wavs.shape))
            _lib.check(vocoder.lib.cmtts_wav_to_int16(_ptr(wavs), _ptr(pcm), wavs.numel(), float(max_wav_value), _stream()))
        _append_stats(stats, st, None)
    else:
        pcm = vocoder_infer_device(mels, vocoder, max_wav_value)
    out = [w for w in pcm.cpu().numpy()]
    check_async_error()          # the D2H copy synchronised: a timeout in the launches that produced `mels` is raised here
    if lengths is not None:
        out = [w[: int(lengths[i])] for i, w in enumerate(out)]
    return out


# ----------------------------------------------------------------------------- streamed PCM (DESIGN.md §3 "Streaming")

STREAM_CHUNK_FRAMES = (32, 64, 128, 256)


def vocoder_halo_frames(hcfg: HifiGanConfig = None):
    """Receptive radius of the generator in mel frames (config.HifiGanConfig.halo_frames; 13 for V1)."""
    return (hcfg if hcfg is not None else HifiGanConfig()).halo_frames


class StreamRound:
    """One round of a stream plan: every window Tw mel frames wide, chunk rows of `core` frames, windows = [(utterance, window
    start, core offset in the window, core length)] — the int32 [N][4] table of cmtts_vocoder_forward_windows."""
    __slots__ = ("Tw", "core", "windows")

    def __init__(self, Tw, core, windows):
        self.Tw, self.core, self.windows = Tw, core, windows

    def __repr__(self):
        return f"StreamRound(Tw={self.Tw}, core={self.core}, windows={self.windows})"


def plan_stream_windows(T, mel_lens, chunk_frames=STREAM_CHUNK_FRAMES, halo=13):
    """Windows of a streamed vocoding of a padded mel [B, 80, T] whose utterances hold mel_lens[b] frames.  Round r vocodes the next
    chunk_frames[r] frames (the last entry repeats; at most the longest remainder) of every utterance not finished yet, in windows Tw = core + 2 halo wide that all lie
    inside [0, T): a window starts `halo` frames before its core unless that would cross 0 or T, where it shifts inwards (the whole-mel
    run sees zero padding at every layer only at the tensor's ends; zero mel frames are not the same, conv_pre's bias makes them non-zero)
    and its core offset grows.  When core + 2 halo >= T the round is one whole-tensor window per utterance (Tw = core = T) holding
    everything left.  Cores tile [0, mel_lens[b]) exactly; an utterance's last core may be short.  Zero-length utterances get no window.
    Returns [StreamRound]."""
    T, halo = int(T), int(halo)
    lens = [int(n) for n in mel_lens]
    chunks = [int(c) for c in chunk_frames]
    if T <= 0 or halo < 0 or not chunks or min(chunks) <= 0:
        raise ValueError(f"plan_stream_windows: T = {T}, halo = {halo}, chunk_frames = {chunks}")
    if any(n < 0 or n > T for n in lens):
        raise ValueError(f"plan_stream_windows: mel_lens {lens} outside [0, {T}]")
    pos = [0] * len(lens)
    live = [b for b, n in enumerate(lens) if n > 0]
    rounds = []
    while live:
        # no wider than the longest remainder: a final round of short cores does not pay for a full-width window
        c = min(chunks[min(len(rounds), len(chunks) - 1)], max(lens[b] - pos[b] for b in live))
        wins = []
        if c + 2 * halo >= T:
            Tw = core = T
            for b in live:
                wins.append((b, 0, pos[b], lens[b] - pos[b]))
        else:
            Tw, core = c + 2 * halo, c
            for b in live:
                cs = pos[b]
                start = min(max(cs - halo, 0), T - Tw)
                wins.append((b, start, cs - start, min(c, lens[b] - cs)))
        for b, start, off, n in wins:
            pos[b] = start + off + n
        rounds.append(StreamRound(Tw, core, wins))
        live = [b for b in live if pos[b] < lens[b]]
    return rounds


def vocoder_infer_stream(mels, vocoder, lengths=None, chunk_frames=STREAM_CHUNK_FRAMES, max_wav_value=32768.0,
                         sample_rate=None, encoding="s16", gain_db=None, loudness=None):
    """vocoder_infer, streamed: mels [B,80,T] -> a generator of (utterance, sample_offset, pcm int16 numpy, is_last), round by round
    (plan_stream_windows; lengths = mel FRAMES per utterance, default T — vocoder_infer's `lengths` count samples).  Concatenated per
    utterance the chunks are vocoder_infer(mels, lengths=mel_len * hop)'s output: bitwise with the direct fp32 form ("winograd" 0),
    within the conv forms' rounding otherwise.  Round r + 1 is enqueued on the current stream before round r's chunks are
    handed back; each round's int16 rows go to pinned host memory on a copy stream, so that copy overlaps the next round's generator.
    sample_rate / encoding (vocoder_infer): the windows reach one frame further (halo H + 1), each round's last layer
    writes fp32 rows with one frame of margin (cmtts_vocoder_forward_windows_f32) and one cmtts_resample_encode turns the round's cores
    into chunks of the output format; offsets then count OUTPUT samples, an utterance's chunks concatenate to
    ceil(mel_len * hop * L / M) samples and are bitwise vocoder_infer(..., sample_rate, encoding)'s under the same condition.
    gain_db (vocoder_infer): a fixed gain per utterance, a number or [B] values — each round gathers the utterance
    gains to its window rows on the device and the gain rides on the round's cmtts_resample_encode_gain (the float path for the native
    format too); one multiplication per source sample, so the chunks stay bitwise vocoder_infer(..., gain_db=...)'s.  A loudness
    TARGET is not available on a stream (ValueError): measure with vocoder_loudness and pass gain_db."""
    if loudness is not None:
        raise ValueError("vocoder_infer_stream: integrated loudness needs the whole utterance, which a stream does not have when its "
                         "first chunk leaves: calibrate the voice with vocoder_loudness and pass gain_db")
    vocoder._require()
    lib, dev = vocoder.lib, vocoder.device
    fmt = _output_format(vocoder, sample_rate, encoding, force=gain_db is not None)
    x = _f32(mels, dev)
    B, M, T = x.shape
    gains = None if gain_db is None else _linear_gains("vocoder_infer_stream: gain_db", gain_db, B, dev)
    lens = [T] * B if lengths is None else [int(n) for n in lengths]
    if len(lens) != B:
        raise ValueError(f"vocoder_infer_stream: {len(lens)} lengths for {B} mels")
    halo = lib.cmtts_vocoder_halo_frames(vocoder._h)
    if halo < 0:
        _lib.check(halo)
    hop = vocoder.h.hop
    if fmt is not None and fmt[0].R > hop:
        raise ValueError(f"vocoder_infer_stream: the filter's half-width {fmt[0].R} exceeds one frame ({hop} samples)")
    # the resampler needs R <= hop samples beyond a core on each side: one more frame of halo, one frame of margin in the float rows
    rounds = plan_stream_windows(T, lens, chunk_frames, halo if fmt is None else halo + 1)
    if not rounds:
        return
    with torch.cuda.device(dev):
        comp = torch.cuda.current_stream(dev)
        copy = torch.cuda.Stream(dev)
        nb = max(lib.cmtts_vocoder_windows_workspace_bytes(vocoder._h, len(r.windows), r.Tw) for r in rounds)
        ws = vocoder._ws.get("voc_stream", nb, dev)

        def enqueue(r):
            N = len(r.windows)
            tab = torch.tensor(r.windows, dtype=torch.int32).pin_memory()      # read in place by the call: kept until `done`
            if fmt is None:
                pcm = torch.empty(N, r.core * hop, dtype=torch.int16, device=dev)
                _lib.check(lib.cmtts_vocoder_forward_windows(vocoder._h, _ptr(x), B, T, _ptr(tab), N, r.Tw, r.core, _ptr(pcm),
                                                             float(max_wav_value), _ptr(ws), nb, _stream()))
            else:
                rsm, enc, dtype = fmt
                rows = torch.empty(N, (r.core + 2) * hop, dtype=torch.float32, device=dev)
                _lib.check(lib.cmtts_vocoder_forward_windows_f32(vocoder._h, _ptr(x), B, T, _ptr(tab), N, r.Tw, r.core, 1, _ptr(rows),
                                                                 _ptr(ws), nb, _stream()))
                # row n starts at frame max(core start - 1, window start); the outputs of the core [f0, f0 + cl) come from the absolute m
                segs = [(n, max(start + off - 1, start) * hop, rsm.out_len((start + off) * hop), rsm.out_len((start + off + cl) * hop),
                         lens[b] * hop) for n, (b, start, off, cl) in enumerate(r.windows)]
                seg_tab = torch.tensor(segs, dtype=torch.int32).pin_memory()
                row_gains = None if gains is None else gains[torch.tensor([w[0] for w in r.windows], device=dev)]
                pcm = _resample_encode(lib, rsm, rows, seg_tab, enc, dtype, max_wav_value, max(m1 - m0 for _, _, m0, m1, _ in segs),
                                       row_gains)
                tab = (tab, seg_tab, segs)
            ready = torch.cuda.Event()
            ready.record(comp)
            host = torch.empty(pcm.shape, dtype=pcm.dtype, pin_memory=True)
            with torch.cuda.stream(copy):
                copy.wait_event(ready)
                host.copy_(pcm, non_blocking=True)
                pcm.record_stream(copy)
                done = torch.cuda.Event()
                done.record(copy)
            return r, tab, host, done

        pending = [enqueue(rounds[0])]
        try:
            for i in range(len(rounds)):
                if i + 1 < len(rounds):
                    pending.append(enqueue(rounds[i + 1]))
                r, _tab, host, done = pending[0]
                done.synchronize()
                check_async_error()          # the round's launches completed: a failure reported by them is raised here
                pending.pop(0)
                arr = host.numpy()
                for n, (b, start, off, cl) in enumerate(r.windows):
                    f0 = start + off
                    if fmt is None:
                        yield b, f0 * hop, arr[n, : cl * hop].copy(), f0 + cl >= lens[b]
                    else:
                        m0, m1 = _tab[2][n][2:4]
                        yield b, m0, arr[n, : m1 - m0].copy(), f0 + cl >= lens[b]
        finally:
            # a consumer that stops early: the pinned tables of rounds still in flight are read by their calls' copies
            for p in pending:
                p[3].synchronize()


def phoneme_marks(out, T=None, sample_rate=None, vocoder=None):
    """Where each phoneme lies in the delivered audio: int32 [B, L, 4] on the device = start frame, end frame, start sample, end
    sample (cmtts_phoneme_marks; the definition: timing.phoneme_marks).  out: what DurationPitchSpeakerNet.forward returned (its
    "d_rounded" and "src_lens").  T: clip the frames to a mel cut at T frames (default: none).  sample_rate: the output rate the
    audio is delivered at (vocoder_infer / vocoder_infer_stream's); None = the native rate, up = down = 1.  vocoder: supplies the hop
    (default: the V1 generator's 256)."""
    from . import resample as _resample
    d, src = out["d_rounded"], out["src_lens"]
    hop = vocoder.h.hop if vocoder is not None else _resample.HOP
    up, down = (1, 1) if sample_rate is None else _resample.ratio(_resample.NATIVE_RATE, sample_rate)      # as _output_format
    T = 0 if T is None else int(T)
    if T < 0:
        raise ValueError(f"phoneme_marks: T = {T}")
    B, L = d.shape
    lib = _lib.load()
    with torch.cuda.device(d.device):
        marks = torch.empty(B, L, 4, dtype=torch.int32, device=d.device)
        _lib.check(lib.cmtts_phoneme_marks(_ptr(d), _ptr(src), B, L, T, int(hop), int(up), int(down), _ptr(marks), _stream()))
    return marks


# ----------------------------------------------------------------------------- re-taking spans

def retake(model: CMTotalTTS, mel, cond_ct, speaker_emb, spans, seeds, n_steps=4, ts=None, steps=40, windowed=True):
    """A new take of some frames of utterances that are already synthesized (cmtts_retake; the definition: retake.retake_reference).
    mel [B,T,80]: the utterances as they are; spans: [(b, lo, hi)] half-open frame intervals to sample again; cond_ct [B,hidden,T],
    speaker_emb: the conditioning the new take is drawn under; seeds: as in sample_with_cond (int64 [B] or one int) — a new seed
    gives a new take.  Returns mel [B,T,80]: every frame outside the spans has the bits of `mel`, the frames inside are sampled
    by the masked consistency sampler (the known frames are put back after every evaluation, so the take joins them).
    n_steps evaluations on cmtts_schedule(n_steps); ts / steps give the general decreasing schedule of stochastic_iterative_sampler
    instead (len(ts) - 1 evaluations).  windowed=True samples every cluster of spans on a window that reaches res_layers frames
    beyond it (retake.plan_retake_windows) — the cost is the spans plus halos, not the utterances; windowed=False runs one
    whole-utterance window per utterance with spans: the yardstick (the same bits in the direct conv form with the model option
    "batch_invariant" set, within the conv forms' rounding otherwise).
    Where spans come from: phoneme_marks(out)[b, l, 0:2] are the frames of phoneme l, and out["mel2ph"][b] == l + 1 marks the same
    frames; a word is the union of its phonemes' intervals.  A changed prosody for the span (control tables of
    DurationPitchSpeakerNet.forward, another speaker vector) gives a new cond_ct; pass segments= / target_frames= to that call so
    that the span, and with it cond_ct, keeps its frame count — a retake does not change T."""
    model._require()
    lib, dev, cfg = model.lib, model.device, model.config
    mel = _f32(mel, dev)
    B, T, M = mel.shape
    if M != cfg.n_mels or tuple(cond_ct.shape) != (B, cfg.hidden, T):
        raise ValueError(f"retake: mel {tuple(mel.shape)} and cond_ct {tuple(cond_ct.shape)} do not fit [B,T,{cfg.n_mels}] / [B,{cfg.hidden},T]")
    spans = [(int(b), int(lo), int(hi)) for b, lo, hi in spans]
    mask = _retake.regen_mask(spans, B, T)
    if ts is None:
        sig = (C.c_float * n_steps)()
        std = (C.c_float * n_steps)()
        _lib.check(lib.cmtts_schedule(model._h, n_steps, sig, std))
    else:
        sg, sd_ = _retake.schedule_from_ts(ts, steps, cfg.sigma_min, cfg.sigma_max, cfg.rho)
        n_steps = len(sg)
        sig = (C.c_float * n_steps)(*sg.tolist())
        std = (C.c_float * n_steps)(*sd_.tolist())
    Tw, wins = _retake.plan_retake_windows(spans, T, cfg.res_layers) if windowed else _retake.whole_windows(spans, T)
    tab = np.ascontiguousarray(np.asarray(wins, np.int32).reshape(-1, 4))
    N = tab.shape[0]
    cond_ct = _f32(cond_ct, dev)
    spk = None if speaker_emb is None else _f32(speaker_emb, dev)
    seeds = _device_seeds(seeds, B, dev)
    with torch.cuda.device(dev):
        regen = torch.from_numpy(mask.astype(np.uint8)).to(dev)
        out = torch.empty_like(mel)
        nb = lib.cmtts_retake_workspace_bytes(model._h, N, Tw)
        ws = model._ws.get("retake", nb, dev)
        _lib.check(lib.cmtts_retake(model._h, _ptr(mel), _ptr(regen), _ptr(cond_ct), _ptr(spk), _ptr(seeds), B, T, C.c_void_p(tab.ctypes.data),
                                    N, Tw, n_steps, sig, std, _ptr(out), _ptr(ws), nb, _stream()))
    return out


def retake_pcm(mel_new, vocoder, pcm_old, spans, lengths=None, max_wav_value=32768.0, sample_rate=None, encoding="s16", gain_db=None):
    """The audio of a retake without vocoding the utterances again: mel_new [B,80,T] (vocoder_infer's layout) is the mel after
    retake(..., spans), pcm_old what vocoder_infer returned for the mel before it (a list of int16 arrays, or int16 [B, T * hop]).
    Only the output frames retake.retake_pcm_range names — [lo - H, hi + H), H = the generator's receptive radius — are vocoded, in
    windows that reach H frames beyond them (cmtts_vocoder_forward_windows, one call), and their int16 samples are spliced into a
    copy of pcm_old.  Returns a list of int16 arrays like vocoder_infer's: every sample outside those frames has the bits of pcm_old,
    and the whole equals vocoder_infer(mel_new, lengths=lengths) — bitwise in the direct conv form, within one LSB otherwise.
    lengths: samples per utterance as in vocoder_infer (default: pcm_old's).  The native rate as int16 only."""
    if sample_rate is not None or encoding != "s16" or gain_db is not None:
        raise ValueError("retake_pcm: the native rate as int16 only (sample_rate, encoding and gain_db are not available here)")
    vocoder._require()
    lib, dev = vocoder.lib, vocoder.device
    x = _f32(mel_new, dev)
    B, M, T = x.shape
    hop = vocoder.h.hop
    H = lib.cmtts_vocoder_halo_frames(vocoder._h)
    if H < 0:
        _lib.check(H)
    old = [np.asarray(w.cpu() if hasattr(w, "cpu") else w) for w in pcm_old]
    if len(old) != B or any(w.dtype != np.int16 or w.ndim != 1 for w in old):
        raise ValueError(f"retake_pcm: pcm_old must hold {B} int16 rows")
    lens = [len(w) for w in old] if lengths is None else [int(n) for n in lengths]
    if len(lens) != B or any(n > len(w) or n < 0 or n > T * hop for n, w in zip(lens, old)):
        raise ValueError("retake_pcm: lengths do not fit pcm_old / the mel")
    out = [w[:n].copy() for w, n in zip(old, lens)]
    per = {}
    for b, lo, hi in spans:
        if not 0 <= int(b) < B:
            raise ValueError(f"retake_pcm: span ({b}, {lo}, {hi}): utterance out of range")
        per.setdefault(int(b), []).append(_retake.retake_pcm_range(lo, hi, H, T))
    cores = []          # (b, first frame, end): the frame ranges of one utterance merged where they touch
    for b in sorted(per):
        for lo, hi in sorted(per[b]):
            if cores and cores[-1][0] == b and lo <= cores[-1][2]:
                cores[-1][2] = max(cores[-1][2], hi)
            else:
                cores.append([b, lo, hi])
    if not cores:
        return out
    core = max(hi - lo for _, lo, hi in cores)
    if core + 2 * H >= T:
        Tw = core = T
        wins = [(b, 0, lo, hi - lo) for b, lo, hi in cores]
    else:
        Tw = core + 2 * H
        wins = []
        for b, lo, hi in cores:
            start = min(max(lo - H, 0), T - Tw)
            wins.append((b, start, lo - start, hi - lo))
    N = len(wins)
    with torch.cuda.device(dev):
        tab = torch.tensor(wins, dtype=torch.int32).pin_memory()      # read in place by the call: kept until the copy below has synchronised
        pcm = torch.empty(N, core * hop, dtype=torch.int16, device=dev)
        nb = lib.cmtts_vocoder_windows_workspace_bytes(vocoder._h, N, Tw)
        ws = vocoder._ws.get("voc_stream", nb, dev)
        _lib.check(lib.cmtts_vocoder_forward_windows(vocoder._h, _ptr(x), B, T, _ptr(tab), N, Tw, core, _ptr(pcm), float(max_wav_value),
                                                     _ptr(ws), nb, _stream()))
        arr = pcm.cpu().numpy()
    check_async_error()
    for n, (b, lo, hi) in enumerate(cores):
        s0, s1 = lo * hop, min(hi * hop, lens[b])
        if s1 > s0:
            out[b][s0:s1] = arr[n, : s1 - s0]
    return out


def synthesize_stream(model: CMTotalTTS, vocoder, texts, src_lens, spker_embeds=None, speakers=None, n_steps=4, noise=None,
                      chunk_frames=STREAM_CHUNK_FRAMES, generator=None, max_wav_value=32768.0,
                      p_control=1.0, e_control=1.0, d_control=1.0, seeds=None, sample_rate=None, encoding="s16",
                      target_frames=None, segments=None, on_marks=None, gain_db=None, loudness=None):
    """Text -> streamed PCM: the duration net and the T-step sampler exactly as CMTotalTTSSynthesize.synthesize runs them (noise
    [n_noise, B, 1, T, 80] drawn as x0 = randn, then randn_like(x0) per further step, unless given), then vocoder_infer_stream on
    the mels trimmed to their predicted lengths.  Yields (utterance, sample_offset, pcm int16 numpy, is_last).
    p_control / e_control / d_control: numbers, [B] or [B, L] float32 tensors (DurationPitchSpeakerNet.forward).
    seeds: int64 [B] utterance seeds or one int — seeded noise generated by the sampler (sample_with_cond), in place of noise / generator.
    sample_rate / encoding: the output format (vocoder_infer_stream); offsets then count output samples.
    target_frames / segments: duration targets (DurationPitchSpeakerNet.forward): utterance b's chunks then concatenate to exactly
    out_len(target * hop) samples.
    on_marks: a callable that receives phoneme_marks(...) as int32 numpy [B, L, 4] once, before the first chunk is handed out, in the
    stream's own output rate — the scale of the chunk offsets.  What the generator yields does not change.
    gain_db: a fixed gain per utterance (vocoder_infer_stream); loudness= is refused as it is there."""
    if loudness is not None:
        raise ValueError("synthesize_stream: integrated loudness needs the whole utterance, which a stream does not have when its "
                         "first chunk leaves: calibrate the voice with vocoder_loudness and pass gain_db")
    if seeds is not None and noise is not None:
        raise ValueError("synthesize_stream: give noise or seeds, not both")
    if on_marks is not None and not callable(on_marks):
        raise ValueError("synthesize_stream: on_marks must be callable")
    B0 = int(torch.as_tensor(texts).shape[0])
    counts = _step_counts(n_steps, B0, "synthesize_stream")
    perm = inv = None
    if counts is not None:
        # per-utterance step counts: the batch is sorted by step count at the text level (steps.order), sampled in one cmtts_sample_mixed call
        # and handed out in the caller's order; given noise rows move with their utterances
        perm, inv, n_steps, seeds = _text_level_order(counts, B0, seeds, "synthesize_stream")
        texts, src_lens, spker_embeds, speakers, p_control, e_control, d_control, target_frames, segments, seeds = (
            _take_rows(v, perm, B0) for v in (texts, src_lens, spker_embeds, speakers, p_control, e_control, d_control, target_frames,
                                              segments, seeds))
    out = model.duration_pitch_energy_net(speakers=speakers, texts=texts, src_lens=src_lens, spker_embeds=spker_embeds,
                                          p_control=p_control, e_control=e_control, d_control=d_control,
                                          target_frames=target_frames, segments=segments)
    B, T, _ = out["cond"].shape
    cfg = model.config
    if counts is None and n_steps not in (1, 2, 4):
        raise ValueError("n_steps must be 1, 2 or 4 (synthesize.py:111-147)")
    most = n_steps if counts is None else n_steps[0]
    draws = 1 if most == 1 else most + 1
    if noise is None and seeds is None:      # drawn in the caller's order
        noise = _draw_sampler_noise(generator or DummyGenerator(), B, T, cfg.n_mels, draws, model.device)
    if noise is not None and perm is not None:
        noise = noise[:, torch.as_tensor(perm, device=noise.device)].contiguous()
    mel = sample_with_cond(model, out["cond_ct"], out["speaker_emb"], n_steps, noise, factors=out.get("cond_factors"), seeds=seeds)
    mel_lens = out["mel_lens"].cpu().tolist()
    marks = phoneme_marks(out, sample_rate=sample_rate, vocoder=vocoder) if on_marks is not None else None
    if inv is not None:
        back = torch.as_tensor(inv, device=mel.device)
        mel = mel[back].contiguous()
        mel_lens = [mel_lens[int(k)] for k in inv]
        marks = marks[back] if marks is not None else None
    if on_marks is not None:
        on_marks(marks.cpu().numpy())
    yield from vocoder_infer_stream(mel.transpose(1, 2), vocoder, mel_lens, chunk_frames, max_wav_value, sample_rate=sample_rate,
                                    encoding=encoding, gain_db=gain_db)


def synth_samples(args, targets, predictions, vocoder, model_config, preprocess_config, path, diffusion=None):
    """utils/tools.py:566-607 (same argument list), the part that is on the inference path: mel -> vocoder_infer -> one int16
    .wav per utterance at the dataset's sampling rate (22 050 Hz), written to <path>/<args.restore_step>/ under the
    reference's names: "<basename>_<speaker_id><tag>.wav" for a multi-speaker model in single mode, "<basename><tag>.wav"
    otherwise (tag = "_teacher_forced" when args.teacher_forced).  `targets` is the synthesize batch (ids first),
    `predictions` the out_put list of CMTotalTTSSynthesize.synthesize (mel [B,T,80] in slot 0, mel_lens in slot 11).  The
    mel-spectrogram PNGs of :573-594 are matplotlib host work and are not produced.  Returns the paths written."""
    import os
    from scipy.io import wavfile
    multi_speaker = model_config["multi_speaker"]
    tag = "_teacher_forced" if getattr(args, "teacher_forced", False) else ""
    basenames = targets[0]
    mel_predictions = predictions[0].transpose(1, 2)            # [B,80,T]
    lengths = predictions[11] * preprocess_config["preprocessing"]["stft"]["hop_length"]
    wav_predictions = vocoder_infer(mel_predictions, vocoder, model_config, preprocess_config, lengths=lengths.tolist())
    sampling_rate = preprocess_config["preprocessing"]["audio"]["sampling_rate"]
    out_dir = os.path.join(path, str(getattr(args, "restore_step", "")))
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for wav, basename in zip(wav_predictions, basenames):
        single = multi_speaker and getattr(args, "mode", None) == "single"
        name = "{}_{}{}.wav".format(basename, args.speaker_id, tag) if single else "{}{}.wav".format(basename, tag)
        out = os.path.join(out_dir, name)
        wavfile.write(out, sampling_rate, wav)
        written.append(out)
    return written


def transpose_last2(x):
    """[B,R,C] -> [B,C,R] on the HIP transpose kernel (cmtts_transpose)."""
    x = x.contiguous()
    B, R, Cn = x.shape
    out = torch.empty(B, Cn, R, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().cmtts_transpose(_ptr(x), _ptr(out), B, R, Cn, _stream()))
    return out


class StreamPipelinedSynthesizer:
    """Throughput mode for a stream of batches: the phoneme/frame-level conditioning of batch i+1 (many small,
    latency-bound launches that cannot fill 256 CUs) runs on a second HIP stream underneath the MFMA-bound
    sampler of batch i.  Same kernels, same results per batch; only the issue order across batches changes."""

    def __init__(self, model: CMTotalTTS, n_steps=4):
        self.model, self.n_steps = model, n_steps
        self.side = torch.cuda.Stream(device=model.device)
        self.ready = None          # (event, out_dict) of the batch whose conditioning is already computed
        self._keep = []

    def prepare(self, texts, src_lens, spker_embeds=None, max_mel_len=None):
        main = torch.cuda.current_stream(self.model.device)
        self.side.wait_stream(main)                       # inputs / workspaces written on main are visible
        with torch.cuda.stream(self.side):
            out = self.model.duration_pitch_energy_net(None, texts, src_lens, spker_embeds=spker_embeds,
                                                       max_mel_len=max_mel_len)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.ready = (ev, out)

    def sample_and_prepare_next(self, noise, next_batch):
        """Sample the prepared batch on the current stream while `next_batch` = (texts, src_lens, spk,
        max_mel_len) is conditioned on the side stream.  Returns (mel, mel_lens) of the prepared batch."""
        ev, out = self.ready
        torch.cuda.current_stream(self.model.device).wait_event(ev)
        f = out.get("cond_factors")
        for v in (out["cond_ct"], out["speaker_emb"]) + ((f.p1, f.p1t, f.mel2ph, f.p_idx) if f is not None else ()):
            if v is not None:
                v.record_stream(torch.cuda.current_stream(self.model.device))
        self._keep = [out]
        if next_batch is not None:
            self.prepare(*next_batch)
        mel = sample_with_cond(self.model, out["cond_ct"], out["speaker_emb"], self.n_steps, noise, factors=out.get("cond_factors"))
        return mel, out["mel_lens"]


ATTN_SHORT_MAX = 192        # attention.hip: all keys in registers up to here, key-chunked online softmax above (not bitwise the same)


class CollatedShard:
    """A ragged shard's bucket groups collated for ONE phoneme-level call per attention class (cmtts_text_forward_ragged): the
    host-side counterpart of the reference's collate_fn padding (dataset.py), done once per shard.  `batches`: list of dicts with
    texts [Bt,Lt], src_lens [Bt], pad_lens [Bt] (each utterance's own group's padded phoneme count), spk [Bt,D] | None and
    `members` = [(group index, b0, n, Lg)]; `groups` keeps (noise, bucket) per group."""

    def __init__(self, groups, device):
        # a group may carry a sixth element: speakers int64 [n] (models whose speaker_emb is an nn.Embedding table, model/cmtts.py:77-78)
        self.groups = [(g[3], int(g[4])) for g in groups]
        self.n = [int(g[0].shape[0]) for g in groups]
        classes = {}
        for i, g in enumerate(groups):
            classes.setdefault(int(g[0].shape[1]) > ATTN_SHORT_MAX, []).append(i)      # groups that take the same attention kernel alone and batched
        self.batches = []
        for _, idx in sorted(classes.items()):
            Lt = max(int(groups[i][0].shape[1]) for i in idx)
            Bt = sum(int(groups[i][0].shape[0]) for i in idx)
            texts = torch.zeros(Bt, Lt, dtype=torch.int64, device=device)
            has_spk = groups[idx[0]][2] is not None
            has_ids = len(groups[idx[0]]) > 5 and groups[idx[0]][5] is not None
            src, pad, spk, ids, members, b0 = [], [], [], [], [], 0
            for i in idx:
                tx, ln, sp = groups[i][0], groups[i][1], groups[i][2]
                if has_ids:
                    ids.append(groups[i][5].to(device=device, dtype=torch.int64))
                n, Lg = tx.shape
                texts[b0:b0 + n, :Lg] = tx.to(device)
                src.append(ln.to(device=device, dtype=torch.int64))
                pad.append(torch.full((n,), Lg, dtype=torch.int64, device=device))
                if has_spk:
                    spk.append(sp.to(device=device, dtype=torch.float32))
                members.append((i, b0, n, Lg))
                b0 += n
            self.batches.append({"texts": texts, "src_lens": torch.cat(src), "pad_lens": torch.cat(pad),
                                 "spk": torch.cat(spk) if has_spk else None, "speakers": torch.cat(ids) if has_ids else None,
                                 "members": members})


def collate_groups(groups, device):
    """groups: [(texts [n,Lg], src_lens [n], spker_embeds [n,D] | None, noise, bucket)] -> CollatedShard."""
    return CollatedShard(list(groups), _norm_device(device))


def _text_forward_ragged(model, tb, key):
    """One cmtts_text_forward_ragged call for a collated text batch.  Returns (text workspace, B, L, mel_len [B], speaker_emb [B,H] | None)."""
    lib, dev, cfg = model.lib, model.device, model.config
    texts, src, pad, spk_in = tb["texts"], tb["src_lens"], tb["pad_lens"], tb["spk"]
    B, L = texts.shape
    table = cfg.multi_speaker and cfg.n_speaker > 0
    ids = tb.get("speakers") if table else None
    if table:
        if ids is None:
            raise AssertionError("speakers (ids into the speaker_emb table) should not be None")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= cfg.n_speaker):
            raise IndexError("index out of range in self")
        spk_in = None
    elif cfg.multi_speaker and spk_in is None:
        raise AssertionError("Speaker embedding should not be None")
    with torch.cuda.device(dev):
        mel_len = torch.empty(B, dtype=torch.int64, device=dev)
        spk = torch.empty(B, cfg.hidden, dtype=torch.float32, device=dev) if cfg.multi_speaker else None
        nb = lib.cmtts_text_workspace_bytes(model._h, B, L)
        tws = model._ws.get(key, nb, dev)
        _lib.check(lib.cmtts_text_forward_ragged(model._h, _ptr(texts), _ptr(src), _ptr(pad), _ptr(spk_in), _ptr(ids), B, L, 1.0,
                                                 None, None, _ptr(mel_len), None, None, None, _ptr(spk), _ptr(tws), nb, _stream()))
    return tws, B, L, mel_len, spk


def _frame_forward_sub(model, tws, B_all, L_all, b0, n, T, key, want_factors=True):
    """cmtts_frame_forward_sub for utterances [b0, b0 + n) of a text workspace -> (cond_ct, CondFactors | None)."""
    lib, dev, cfg = model.lib, model.device, model.config
    with torch.cuda.device(dev):
        f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        cond_ct = f(n, cfg.hidden, T)
        mel2ph = torch.empty(n, T, dtype=torch.int64, device=dev)
        p_idx = torch.empty(n, T, dtype=torch.int64, device=dev)
        p1_ld = (L_all + 3) // 4 * 4
        p1 = f(n, cfg.res_layers * cfg.res_channels, p1_ld) if want_factors and getattr(model, "_precision_mode", 0) == 0 and model._cond_factors else None
        nf = lib.cmtts_frame_workspace_bytes(model._h, n, T)
        fws = model._ws.get(key, nf, dev)
        _lib.check(lib.cmtts_frame_forward_sub(model._h, _ptr(tws), B_all, L_all, b0, n, T, _ptr(cond_ct), _ptr(mel2ph), None, None,
                                               _ptr(p_idx), None, _ptr(p1), _ptr(fws), nf, _stream()))
    factors = None if p1 is None else CondFactors(p1, p1_ld, L_all, mel2ph, p_idx, cond_ct)
    cond_ct._cmtts_factors = factors
    return cond_ct, factors


class BucketedSynthesizer:
    """BASELINE.json configs[3] on one rank: a shard of ragged utterances dealt into static frame buckets
    (cmtts_amd.shard.frame_bucket).  A bucket group alone cannot fill 256 CUs.  mode "ragged" (default): the text side of every
    group runs on its own HIP stream (short launches that overlap), then ONE cmtts_sample_ragged call runs the residual layers of
    all groups in one persistent launch per evaluation, each utterance trimmed to the frames its mel_len (+ tail_frames) needs
    — the one host read-back of the shard (the reference's length regulator reads back per phoneme, model/modules.py:439-441).
    mode "streams": every group end to end on its own stream (round 2).  Either way each group's valid frames are those of
    running the group alone."""

    def __init__(self, model: CMTotalTTS, n_steps=4, n_streams=4, persistent=None, mode="ragged", tail_frames=16, trim=True, batch_text=None):
        """persistent: denoiser mode while the groups run in "streams" mode (cmtts_set_persistent_denoiser; None = leave the
        process setting alone).  tail_frames: frames beyond mel_len that must be exact in the padded mel (16 covers HiFi-GAN's
        receptive field; the frames beyond the computed range are zeros instead of denoised padding).  trim=False computes
        every padded frame (bit-identical to the per-group launches everywhere)."""
        self.model, self.n_steps, self.persistent, self.mode = model, n_steps, persistent, mode
        self.tail_frames, self.trim = int(tail_frames), bool(trim)
        self.streams = [torch.cuda.Stream(device=model.device) for _ in range(n_streams)]
        # round 4, mode "ragged": the phoneme-level half of ALL groups in one cmtts_text_forward_ragged call (one launch sequence for the
        # shard instead of one per group), then each group's frame-level half on its own stream; False = one text side per group (round 3)
        # None = automatic: batched once a process group exists (measured on MI355X, configs[3] shard: with RCCL loaded the one-call text side
        # runs the shard at 860-870 k frames/s against 824-834 k for one text side per group on four streams; without RCCL 870-880 k against
        # 877-881 k) — a CollatedShard passed to run() is always batched
        if batch_text is None:
            batch_text = torch.distributed.is_available() and torch.distributed.is_initialized()
        self.batch_text = bool(batch_text)

    def _early_groups(self, sizes):
        """sizes: [(n, bucket)] -> indices of the small groups that run end to end on their own stream (see run())."""
        early = set()
        cap = torch.cuda.get_device_properties(self.model.device).multi_processor_count
        tiles = [n * ((bucket + 63) // 64) for n, bucket in sizes]
        order = sorted(range(len(sizes)), key=lambda i: tiles[i])
        rest, gone = sum(tiles), 0
        for i in order:
            if rest <= cap or gone + tiles[i] > 64:
                break
            early.add(i); rest -= tiles[i]; gone += tiles[i]
        if not (rest * 0.92 <= cap):       # would not fit one round even after trimming: let the library decide
            early = set()
        return early

    def _run_batched(self, coll):
        """mode "ragged", fp32: one phoneme-level call per attention class for the whole shard, the frame-level halves per group on
        the streams, set-aside candidates sampled end to end on theirs, ONE cmtts_sample_ragged for the rest."""
        model, lib, dev = self.model, self.model.lib, self.model.device
        main = torch.cuda.current_stream(dev)
        ng = len(coll.groups)
        early = self._early_groups([(coll.n[i], coll.groups[i][1]) for i in range(ng)]) if self.trim else set()
        conds, lens, done, late_events = [None] * ng, [None] * ng, {}, []
        text_done = []
        for k, tb in enumerate(coll.batches):          # the library's branch streams stay ON here: one call, nothing to compete with
            tws, Bt, Lt, mel_len, spk = _text_forward_ragged(model, tb, ("text_ragged", k))
            ev = torch.cuda.Event()
            ev.record(main)
            text_done.append((tb, tws, Bt, Lt, mel_len, spk, ev))
        prev_branch = lib.cmtts_set_option(b"branch_streams", 0)       # the groups overlap across the streams from here on
        try:
            order = []
            for tb, tws, Bt, Lt, mel_len, spk, ev in text_done:
                for (i, b0, n, Lg) in tb["members"]:
                    order.append((i not in early, i, b0, n, tws, Bt, Lt, mel_len, spk, ev))
            for _, i, b0, n, tws, Bt, Lt, mel_len, spk, ev in sorted(order, key=lambda t: t[:2]):      # the early groups are queued first
                noise, bucket = coll.groups[i]
                st = self.streams[i % len(self.streams)]
                st.wait_event(ev)
                with torch.cuda.stream(st):
                    cond_ct, factors = _frame_forward_sub(model, tws, Bt, Lt, b0, n, bucket, ("frame_ragged", i))
                    spk_i = None if spk is None else spk[b0:b0 + n]
                    lens[i] = mel_len[b0:b0 + n]
                    if i in early:
                        prev_p = lib.cmtts_set_persistent_denoiser(0)
                        try:
                            done[i] = (sample_with_cond(model, cond_ct, spk_i, self.n_steps, noise, factors=factors), lens[i])
                        finally:
                            lib.cmtts_set_persistent_denoiser(prev_p)
                    else:
                        e2 = torch.cuda.Event()
                        e2.record(st)
                        late_events.append(e2)
                    conds[i] = (cond_ct, spk_i, factors)
        finally:
            lib.cmtts_set_option(b"branch_streams", prev_branch)
        for e2 in late_events:
            main.wait_event(e2)
        late = [i for i in range(ng) if i not in early]
        active = [None] * len(late)
        if self.trim and late:      # one device -> host copy for the whole shard
            flat = torch.cat([lens[i] for i in late]).cpu().tolist()
            k = 0
            for gi, i in enumerate(late):
                active[gi] = flat[k:k + coll.n[i]]
                k += coll.n[i]
        mels = sample_ragged(model, [(conds[i][0], conds[i][1], coll.groups[i][0], a, conds[i][2]) for i, a in zip(late, active)],
                             self.n_steps, self.tail_frames) if late else []
        for i, mel in zip(late, mels):
            done[i] = (mel, lens[i])
        for st in self.streams:
            main.wait_stream(st)
        return [done[i] for i in range(ng)]

    def run(self, groups):
        """groups: iterable of (texts, src_lens, spker_embeds | None, noise [n_steps+1,n,1,bucket,80], bucket), or the CollatedShard
        collate_groups() made of them (collation = input preparation, once per shard).
        Returns [(mel [n,bucket,80], mel_lens [n])] in the same order."""
        dev = self.model.device
        if not isinstance(groups, CollatedShard):
            groups = list(groups)
        table = self.model.config.multi_speaker and self.model.config.n_speaker > 0
        no_ids = table and not isinstance(groups, CollatedShard) and any(len(g) < 6 or g[5] is None for g in groups)
        if self.mode == "ragged" and (self.batch_text or isinstance(groups, CollatedShard)) and getattr(self.model, "_precision_mode", 0) == 0 and not no_ids:
            return self._run_batched(groups if isinstance(groups, CollatedShard) else collate_groups(groups, dev))
        if isinstance(groups, CollatedShard):
            raise ValueError("a CollatedShard needs mode='ragged' with batch_text on an fp32 model")
        main = torch.cuda.current_stream(dev)
        out = []
        lib = self.model.lib
        prev = lib.cmtts_set_persistent_denoiser(self.persistent) if self.persistent is not None and (self.mode != "ragged" or getattr(self.model, "_precision_mode", 0) != 0) else None
        # the groups already overlap across streams; the library's own side streams (independent branches of one group)
        # would only add streams competing for the few hardware queues HIP maps them onto (25 -> 31-39 ms measured)
        prev_branch = lib.cmtts_set_option(b"branch_streams", 0)
        groups = list(groups)
        mode = self.mode
        if mode == "ragged" and getattr(self.model, "_precision_mode", 0) != 0:
            mode = "streams"      # the one-launch form is the fp32 persistent kernel's: 16-bit models keep one stream per bucket group
        # "ragged": a shard whose padded tiles exceed the CU count needs a second round of the persistent launch unless a few SMALL
        # groups are left out (cmtts_sample_ragged sets them aside itself once the lengths are known).  When the padded sizes already
        # say so, those groups run END TO END on their own stream right away — their sampler (per-layer kernels) then overlaps the
        # text side of the large groups instead of following it.  The guess only moves work between streams: results are per group.
        early = set()
        if mode == "ragged" and self.trim:
            cap = torch.cuda.get_device_properties(dev).multi_processor_count
            tiles = [int(g[0].shape[0]) * ((int(g[4]) + 63) // 64) for g in groups]
            order = sorted(range(len(groups)), key=lambda i: tiles[i])
            rest, gone = sum(tiles), 0
            for i in order:
                if rest <= cap or gone + tiles[i] > 64:
                    break
                early.add(i); rest -= tiles[i]; gone += tiles[i]
            if not (rest * 0.92 <= cap):       # would not fit one round even after trimming: let the library decide
                early = set()
        try:
            conds = []
            done = {}
            late_events = []
            for i in sorted(range(len(groups)), key=lambda i: i not in early):      # the early groups are queued first
                texts, src_lens, spk, noise, bucket = groups[i][:5]
                ids = groups[i][5] if len(groups[i]) > 5 else None
                st = self.streams[i % len(self.streams)]
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    o = self.model.duration_pitch_energy_net(ids, texts, src_lens, spker_embeds=spk, max_mel_len=bucket)
                    if mode != "ragged" or i in early:
                        prev_p = lib.cmtts_set_persistent_denoiser(0) if i in early else None
                        mel = sample_with_cond(self.model, o["cond_ct"], o["speaker_emb"], self.n_steps, noise, factors=o.get("cond_factors"))
                        if prev_p is not None:
                            lib.cmtts_set_persistent_denoiser(prev_p)
                        done[i] = (mel, o["mel_lens"])
                    if i not in early:      # main waits for THIS group's text side, whatever else shares its stream
                        ev = torch.cuda.Event()
                        ev.record(st)
                        late_events.append(ev)
                conds.append((i, o))
            conds = [o for _, o in sorted(conds, key=lambda t: t[0])]
            if mode != "ragged":
                out = [done[i] for i in range(len(groups))]
        finally:
            lib.cmtts_set_option(b"branch_streams", prev_branch)
            if prev is not None:
                lib.cmtts_set_persistent_denoiser(prev)
        # every late group's text side is ordered before main by ITS OWN event: with more groups than streams a late group can
        # share an early group's stream, whose full join only happens after the persistent launches are queued (below)
        for ev in late_events:
            main.wait_event(ev)
        early_streams = {id(self.streams[i % len(self.streams)]) for i in early}
        for st in self.streams:
            if id(st) not in early_streams:
                main.wait_stream(st)
        if mode == "ragged":
            late = [i for i in range(len(groups)) if i not in early]
            lens = [conds[i]["mel_lens"] for i in late]
            active = [None] * len(late)
            if self.trim and late:      # one device -> host copy for the whole shard
                flat = torch.cat(lens).cpu().tolist()
                k = 0
                for gi, l in enumerate(lens):
                    active[gi] = flat[k:k + l.numel()]
                    k += l.numel()
            mels = sample_ragged(self.model, [(conds[i]["cond_ct"], conds[i]["speaker_emb"], groups[i][3], a, conds[i].get("cond_factors"))
                                              for i, a in zip(late, active)],
                                 self.n_steps, self.tail_frames) if late else []
            for i, mel, l in zip(late, mels, lens):
                done[i] = (mel, l)
            out = [done[i] for i in range(len(groups))]
        for st in self.streams:
            if id(st) in early_streams:
                main.wait_stream(st)
        return out


class CMTotalTTSSynthesize:
    """synthesize.py:35-153 with the reference's constructor: CMTotalTTSSynthesize(model_path, model_step_num, args,
    preprocess_config, model_config, train_config, p_control, e_control, d_control).  The checkpoint
    <model_path>/CMDenoiserTTS/model{step:06d}.pt is read with torch.load and handed to CMTotalTTS.load_state_dict
    (cmtts_set_tensor + cmtts_finalize).  `from_model` keeps the model-object form (the reference reloads the checkpoint
    for every batch, :203-206; a serving host builds the model once)."""

    def __init__(self, model_path, model_step_num, args, preprocess_config, model_config, train_config,
                 p_control=1.0, e_control=1.0, d_control=1.0, device=None, generator=None, n_speaker=None):
        import os.path as osp
        self.device = _norm_device(device if device is not None else "cuda") if torch.cuda.is_available() else torch.device("cpu")
        self.CMDenoiserTTS_path = osp.join(model_path, "CMDenoiserTTS", "model{:06d}.pt".format(int(model_step_num)))
        self.args = args
        self.train_config = train_config
        self.model, self.diffusion = self.load_cm_model(args, preprocess_config, model_config, train_config, n_speaker=n_speaker)
        self.duration_pitch_energy_net, self.denoise_net = self.model.get_segmentation_model()
        self.p_control, self.e_control, self.d_control = p_control, e_control, d_control
        self.generator = generator

    @classmethod
    def from_model(cls, model: CMTotalTTS, T=1, generator=None, p_control=1.0, e_control=1.0, d_control=1.0):
        """A synthesizer around an already loaded model (no checkpoint I/O); T = sampling steps (args.T)."""
        import argparse
        self = cls.__new__(cls)
        cfg = model.config
        self.device = model.device
        self.CMDenoiserTTS_path = None
        self.args = argparse.Namespace(T=int(T))
        self.train_config = {"cm": {"sigma_min": cfg.sigma_min, "sigma_max": cfg.sigma_max}}
        self.model = model
        self.diffusion = KarrasDenoiser(sigma_data=cfg.sigma_data, sigma_max=cfg.sigma_max, sigma_min=cfg.sigma_min,
                                        rho=cfg.rho, distillation=True)
        self.duration_pitch_energy_net, self.denoise_net = model.get_segmentation_model()
        self.p_control, self.e_control, self.d_control = p_control, e_control, d_control
        self.generator = generator
        return self

    def load_cm_model(self, args, preprocess_config, model_config, train_config, n_speaker=None):
        """synthesize.py:59-86: distillation from cm.training_mode, model + diffusion from the `cm` block
        (script_util.py:56-76: sigma_min / sigma_max / sigma_data / rho, weight_schedule, loss_norm), torch.load of the
        checkpoint -> load_state_dict -> to(device) -> eval()."""
        from .config import config_from_reference
        cm = train_config["cm"]
        mode = cm["training_mode"]
        if mode == "progdist":
            distillation = False
        elif "consistency" in mode:
            distillation = True
        else:
            raise ValueError(f"unknown training mode {mode}")
        cfg = config_from_reference(preprocess_config, model_config, train_config, n_speaker=n_speaker)
        model = CMTotalTTS(cfg, self.device)
        diffusion = KarrasDenoiser(sigma_data=cfg.sigma_data, sigma_max=cfg.sigma_max, sigma_min=cfg.sigma_min, rho=cfg.rho,
                                   weight_schedule=cm.get("weight_schedule", "karras"), distillation=distillation,
                                   loss_norm=cm.get("loss_norm", "lpips"))
        state = torch.load(self.CMDenoiserTTS_path, map_location="cpu")
        model.load_state_dict(state)
        model.to(self.device)
        model.eval()
        return model, diffusion

    def synthesize(self, batch, p_control=None, e_control=None, d_control=None, seeds=None, target_frames=None, segments=None, n_steps=None):
        """batch = (ids, raw_texts, speakers, texts, src_lens, max_src_len, spker_embeds) after to_device (:88-153).
        The controls given at construction apply (numbers, or float32 [B] / [B, L] tensors); a control given here replaces the
        constructor's for this call — a table on top of a constructor scalar other than 1 is a ValueError.
        seeds: int64 [B] utterance seeds or one int — the sampler generates the seeded noise itself (sample_with_cond) and the
        generator is not drawn from.  A "determ-indiv" generator (get_generator) without `seeds` does the same with its own seeds.
        target_frames / segments: duration targets (DurationPitchSpeakerNet.forward) — out_put[11] are then the fitted lengths.
        n_steps: None = args.T; an int replaces it for this call; a sequence of B step counts (each 1, 2 or 4, any order) samples the
        batch in ONE mixed call (cmtts_sample_mixed): the batch is sorted by step count at the text level (steps.order), every
        utterance comes back at the caller's position with the bits of its row in the uniform call at its count, and noise drawn
        from the generator is drawn in the caller's order."""
        B0 = int(torch.as_tensor(batch[3]).shape[0])
        counts = None if n_steps is None else _step_counts(n_steps, B0, "synthesize")
        perm = inv = None
        if counts is not None:
            perm, inv, counts, seeds = _text_level_order(counts, B0, seeds, "synthesize")
            p_control = self.p_control if p_control is None else p_control
            e_control = self.e_control if e_control is None else e_control
            d_control = self.d_control if d_control is None else d_control
            batch = list(batch)
            batch[2], batch[3], batch[4], batch[-1], p_control, e_control, d_control, target_frames, segments, seeds = (
                _take_rows(v, perm, B0) for v in (batch[2], batch[3], batch[4], batch[-1], p_control, e_control, d_control, target_frames,
                                                  segments, seeds))
        kw = {"speakers": batch[2], "texts": batch[3], "src_lens": batch[4], "spker_embeds": batch[-1]}
        if target_frames is not None or segments is not None:
            kw["target_frames"], kw["segments"] = target_frames, segments
        _check_no_scalar_with_table((self.p_control, self.e_control, self.d_control), p_control, e_control, d_control)
        for name, own, given in (("p_control", self.p_control, p_control), ("e_control", self.e_control, e_control),
                                 ("d_control", self.d_control, d_control)):
            v = own if given is None else given
            if isinstance(v, (torch.Tensor, np.ndarray)) or v != 1.0:      # the defaults leave the call as it was
                kw[name] = v
        tshape = tuple(torch.as_tensor(kw["texts"]).shape)
        _resolve_controls(tshape[0], tshape[-1], kw.get("p_control", 1.0), kw.get("e_control", 1.0), kw.get("d_control", 1.0))
        _resolve_targets(tshape[0], tshape[-1], target_frames, segments)
        out_dict = self.duration_pitch_energy_net(**kw)
        B, T, _ = out_dict["cond"].shape
        cfg = self.model.config
        steps = int(self.args.T) if n_steps is None else (counts[0] if counts is not None else int(n_steps))
        if steps == 1:
            n_steps, draws = 1, 1
        elif steps in (2, 4):
            n_steps, draws = steps, steps + 1
        else:
            raise ValueError("T must be 1, 2 or 4 (synthesize.py:111-147)")
        cm = self.train_config["cm"]
        fusable = getattr(self.diffusion, "distillation", False) and \
            abs(float(cm.get("sigma_max", cfg.sigma_max)) - cfg.sigma_max) < 1e-6 * cfg.sigma_max and \
            abs(float(cm.get("sigma_min", cfg.sigma_min)) - cfg.sigma_min) < 1e-6 * cfg.sigma_min
        gen = self.generator or DummyGenerator()
        if seeds is not None and not fusable:
            raise NotImplementedError("seeds: the fused sampler only (a distilled model with the config's sigmas)")
        if counts is not None and not fusable:
            raise NotImplementedError("n_steps per utterance: the fused sampler only (a distilled model with the config's sigmas)")
        if target_frames is not None and not fusable:      # the host-side loops re-run the duration net from the reference's argument list
            raise NotImplementedError("target_frames: the fused sampler only (a distilled model with the config's sigmas)")
        if not fusable:      # e.g. a progdist teacher: the reference's sampler loops, host-side (karras_sample_tts routes)
            sample = karras_sample_tts(self.diffusion, self.model, (B, 1, T, cfg.n_mels), steps=2, model_kwargs=kw,
                                       device=self.device, sigma_min=float(cm.get("sigma_min", cfg.sigma_min)),
                                       sigma_max=float(cm.get("sigma_max", cfg.sigma_max)),
                                       sampler="onestep" if steps == 1 else "multistep",
                                       ts=None if steps == 1 else (0,) * steps + (1,), generator=gen)
        else:                # the duration net ran once above; the reference's in-sampler re-runs are bit-identical
            noise = None
            from_gen = False
            if seeds is None and isinstance(gen, IndivGenerator) and gen.draw == 0:
                seeds = gen.seeds_for(B)          # the sampler makes draws 0 .. draws - 1 itself
                from_gen = True
                gen.draw += draws
            elif seeds is None:
                noise = _draw_sampler_noise(gen, B, T, cfg.n_mels, draws, self.model.device)
            if perm is not None and seeds is None:      # drawn in the caller's order: the rows move with their utterances
                noise = noise[:, torch.as_tensor(perm, device=noise.device)].contiguous()
            elif perm is not None and from_gen:
                seeds = _take_rows(np.asarray(seeds), perm, B)
            sample = sample_with_cond(self.model, out_dict["cond_ct"], out_dict["speaker_emb"], counts if counts is not None else n_steps, noise,
                                      factors=out_dict.get("cond_factors"), seeds=seeds)
        out_put = [None] * 12
        out_put[0] = sample
        out_put[10] = kw["src_lens"]
        out_put[11] = out_dict["mel_lens"]
        if inv is not None:      # back to the caller's order
            out_put[0] = sample[torch.as_tensor(inv, device=sample.device)].contiguous()
            out_put[10], out_put[11] = _take_rows(out_put[10], inv, B), _take_rows(out_put[11], inv, B)
        return out_put


def get_vocoder(config, device, root="."):
    """utils/model.py:155-184: config["vocoder"] = {"model": "HiFi-GAN", "speaker": "LJSpeech" | "universal"} ->
    hifigan/config.json + hifigan/generator_<speaker>.pth.tar (ckpt["generator"], weight-norm pairs folded like
    remove_weight_norm) under `root` (the reference resolves them against the working directory).  MelGAN comes from
    torch.hub (network) in the reference and is not part of this path."""
    import json
    import os
    name, speaker = config["vocoder"]["model"], config["vocoder"]["speaker"]
    if name != "HiFi-GAN":
        raise NotImplementedError(f"vocoder {name!r}: only HiFi-GAN is on the hot path (MelGAN needs torch.hub)")
    if speaker not in ("LJSpeech", "universal"):
        raise ValueError(f"unknown vocoder speaker {speaker!r}")
    with open(os.path.join(root, "hifigan", "config.json")) as f:
        hc = json.load(f)
    h = HifiGanConfig(num_mels=hc.get("num_mels", 80), upsample_rates=tuple(hc["upsample_rates"]),
                      upsample_kernel_sizes=tuple(hc["upsample_kernel_sizes"]),
                      upsample_initial_channel=hc["upsample_initial_channel"],
                      resblock_kernel_sizes=tuple(hc["resblock_kernel_sizes"]),
                      resblock_dilation_sizes=tuple(tuple(d) for d in hc["resblock_dilation_sizes"]))
    if h != HifiGanConfig():
        raise NotImplementedError("the vocoder kernels are specialised for hifigan/config.json (V1 generator)")
    ckpt = torch.load(os.path.join(root, "hifigan", f"generator_{speaker}.pth.tar"), map_location="cpu")
    vocoder = Generator(h, device)
    vocoder.load_state_dict(ckpt["generator"])
    vocoder.eval()
    vocoder.remove_weight_norm()
    return vocoder


# ---- speaker embeddings from reference audio (csrc/speaker_encoder.hip; definition: cmtts_amd/speaker.py)

class SpeakerEncoder:
    """The DeepSpeaker ResCNN on the device (deepspeaker/embedding.py: build_model): cmtts_spkenc_* behind one handle."""

    def __init__(self, weights, device="cuda:0"):
        from .weights import import_deepspeaker
        self.device = _norm_device(device) if torch.cuda.is_available() else torch.device(device)
        self.lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self.lib.cmtts_spkenc_create(C.byref(self._h)))
        self._ws = _Workspace()
        self._ready = False
        _push_state_dict(self.lib, self.lib.cmtts_spkenc_set_tensor, self._h, import_deepspeaker(weights))
        if self.device.type == "cuda" and torch.cuda.is_available():
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cmtts_spkenc_finalize(self._h))
            self._ready = True

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:
            self.lib.cmtts_spkenc_destroy(h)
            self._h = None

    def _require(self):
        if not self._ready:
            raise RuntimeError("SpeakerEncoder: no GPU — cmtts_amd has no CPU fallback (the weights are loaded, the kernels cannot run)")


def get_speaker_encoder(weights, device="cuda:0"):
    """deepspeaker/embedding.py: build_model — `weights`: a dict of the ResCNN's tensors under their Keras names, an .npz of them, or the
    reference's .h5 checkpoint (weights.import_deepspeaker)."""
    return SpeakerEncoder(weights, device)


def _speaker_windows_bound(n, sample_rate):
    """The most windows windows="all" can give a row of n samples."""
    from . import speaker as sp
    frame_len, frame_step, _ = sp.frame_geometry(sample_rate, 1024)
    F = sp.num_frames(n, frame_len, frame_step)
    return max(1, min(sp.MAX_WINDOWS, len(sp.window_offsets(F, "all"))))


def speaker_features(enc: SpeakerEncoder, wavs, lengths=None, sample_rate=22050, win_length=1024, windows="center"):
    """cmtts_spkenc_features: float audio [B, n] -> (windows fp32 [W, 160, 64] on the device, info int32 [B, 4] on the HOST = (first, last,
    frames, windows) per row).  Reading info back synchronises the stream."""
    from . import resample as rs
    enc._require()
    if int(sample_rate) != rs.NATIVE_RATE:
        raise ValueError(f"speaker_embedding: the audio must be at the model's sample rate {rs.NATIVE_RATE} Hz, not {sample_rate}")
    dev = enc.device
    if isinstance(wavs, (list, tuple)):
        rows = [torch.as_tensor(np.asarray(w, np.float32)).reshape(-1) for w in wavs]
        if lengths is None:
            lengths = [r.numel() for r in rows]
        ld = max(1, max(r.numel() for r in rows))
        wavs = torch.zeros(len(rows), ld, dtype=torch.float32)
        for i, r in enumerate(rows):
            wavs[i, :r.numel()] = r
    wavs = torch.as_tensor(wavs)
    if wavs.dim() == 1:
        wavs = wavs[None]
    if not wavs.dtype.is_floating_point:
        raise ValueError("speaker_embedding: float audio expected")
    wavs = _f32(wavs, dev)
    B, n = wavs.shape
    lens = _clip_lengths(lengths, B, n)
    offsets = None
    if isinstance(windows, str):
        if windows not in ("center", "all"):
            raise ValueError(f"windows = {windows!r}: expected 'center', 'all' or integer offsets")
        mode = 0 if windows == "center" else 1
    else:
        mode = 2
        offs = [int(windows)] * B if np.ndim(windows) == 0 else [int(v) for v in windows]
        if len(offs) != B or min(offs) < 0:
            raise ValueError("windows: one non-negative frame offset per row")
    max_w = max(_speaker_windows_bound(v, sample_rate) for v in lens) if mode == 1 else 1
    with torch.cuda.device(dev):
        n_valid = torch.tensor(lens, dtype=torch.int32).to(dev)
        if mode == 2:
            offsets = torch.tensor(offs, dtype=torch.int32).to(dev)
        win = torch.empty(B * max_w, 160, 64, dtype=torch.float32, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev)
        _lib.check(enc.lib.cmtts_spkenc_features(enc._h, _ptr(wavs), B, n, _ptr(n_valid), int(sample_rate), int(win_length), mode,
                                                 _ptr(offsets), max_w, _ptr(win), _ptr(info), _stream()))
        info = info.cpu().numpy()
    if mode == 2:
        from . import speaker as sp
        for b in range(B):
            if info[b, 2] and offs[b] > max(int(info[b, 2]) - sp.NUM_FRAMES, 0):
                raise ValueError(f"window offset {offs[b]} of row {b} outside [0, {max(int(info[b, 2]) - sp.NUM_FRAMES, 0)}]")
    return win[:int(info[:, 3].sum())], info


def speaker_forward(enc: SpeakerEncoder, windows, row_map, rows):
    """cmtts_spkenc_forward: windows fp32 [W, 160, 64] (device), row_map int [W] -> embeddings fp32 [rows, 512] (device)."""
    enc._require()
    dev = enc.device
    windows = _f32(windows, dev)
    W = int(windows.shape[0])
    with torch.cuda.device(dev):
        rm = torch.as_tensor(np.asarray(row_map, np.int32).reshape(-1)).to(dev) if not isinstance(row_map, torch.Tensor) else row_map.to(dev, torch.int32)
        if rm.numel() != W:
            raise ValueError("speaker_forward: one row_map entry per window")
        if W == 0:
            rm = torch.zeros(1, dtype=torch.int32, device=dev)
        emb = torch.empty(int(rows), 512, dtype=torch.float32, device=dev)
        nb = enc.lib.cmtts_spkenc_workspace_bytes(max(W, 1), 1, 1)
        ws = enc._ws.get("spkenc", nb, dev)
        _lib.check(enc.lib.cmtts_spkenc_forward(enc._h, _ptr(windows) if W else None, W, _ptr(rm), int(rows), _ptr(emb), _ptr(ws), nb, _stream()))
    return emb


def speaker_embedding(enc: SpeakerEncoder, wavs, lengths=None, sample_rate=22050, win_length=1024, windows="center"):
    """deepspeaker/embedding.py: predict_embedding for a batch — float audio [B, n] (or a list of 1-D arrays) at the model's sample rate ->
    a DEVICE tensor [B, 512] of unit-norm DeepSpeaker vectors, accepted unchanged as spker_embeds= by synthesize, synthesize_stream,
    synthesize_sharded and text_state_records.  windows: "center" (one 160-frame window from the middle of the trimmed utterance; the
    reference draws its offset at random), "all" (every window at hop 80, embeddings averaged), or integer frame offsets (one, or one per row).
    A row the trim keeps nothing of — silence, constant magnitude — raises ValueError naming the rows (the reference raises IndexError)."""
    win, info = speaker_features(enc, wavs, lengths, sample_rate, win_length, windows)
    bad = [b for b in range(info.shape[0]) if info[b, 2] == 0]
    if bad:
        raise ValueError(f"speaker_embedding: nothing left of rows {bad} after the silence trim (silent or constant-magnitude audio)")
    row_map = np.repeat(np.arange(info.shape[0], dtype=np.int32), info[:, 3])
    return speaker_forward(enc, win, row_map, info.shape[0])


# ---- GE2E speaker embeddings from reference audio (csrc/ge2e.hip; definition: cmtts_amd/ge2e.py)

class GE2EEncoder:
    """The GE2E LSTM encoder on the device (ge2e_encoder/inference.py: load_model): cmtts_ge2e_* behind one handle."""

    def __init__(self, weights, device="cuda:0"):
        from .weights import import_ge2e
        self.device = _norm_device(device) if torch.cuda.is_available() else torch.device(device)
        self.lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self.lib.cmtts_ge2e_create(C.byref(self._h)))
        self._ws = _Workspace()
        self._ready = False
        _push_state_dict(self.lib, self.lib.cmtts_ge2e_set_tensor, self._h, import_ge2e(weights))
        if self.device.type == "cuda" and torch.cuda.is_available():
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cmtts_ge2e_finalize(self._h))
            self._ready = True

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:
            self.lib.cmtts_ge2e_destroy(h)
            self._h = None

    def _require(self):
        if not self._ready:
            raise RuntimeError("GE2EEncoder: no GPU — cmtts_amd has no CPU fallback (the weights are loaded, the kernels cannot run)")


def get_ge2e_encoder(weights, device="cuda:0"):
    """ge2e_encoder/inference.py: load_model — `weights`: a dict of the encoder's tensors under torch's names, an .npz of them, or the
    reference's encoder.pt (weights.import_ge2e)."""
    return GE2EEncoder(weights, device)


def ge2e_features(enc: GE2EEncoder, wavs, lengths=None, sample_rate=22050, using_partials=True):
    """cmtts_ge2e_features: float audio [B, n] (or a list of rows) at 22 050 Hz -> (windows fp32 [W, T, 40] on the device — the rows' partials,
    T = 160, or with using_partials=False each row's whole power mel padded to the longest —, win_lens int32 [W] on the device, info int32
    [B, 4] on the HOST = (samples, padded samples, frames, windows) per row).  Reading info back synchronises the stream."""
    from . import ge2e as g2
    enc._require()
    if int(sample_rate) != g2.SAMPLE_RATE:
        raise ValueError(f"ge2e_embedding: the audio must be at {g2.SAMPLE_RATE} Hz, the one sample rate the GE2E front end is defined at, not {sample_rate}")
    dev = enc.device
    if isinstance(wavs, (list, tuple)):
        rows = [torch.as_tensor(np.asarray(w, np.float32)).reshape(-1) for w in wavs]
        if lengths is None:
            lengths = [r.numel() for r in rows]
        wavs = torch.zeros(len(rows), max(1, max(r.numel() for r in rows)), dtype=torch.float32)
        for i, r in enumerate(rows):
            wavs[i, :r.numel()] = r
    wavs = torch.as_tensor(wavs)
    if wavs.dim() == 1:
        wavs = wavs[None]
    if not wavs.dtype.is_floating_point:
        raise ValueError("ge2e_embedding: float audio expected")
    wavs = _f32(wavs, dev)
    B, n = wavs.shape
    lens = _clip_lengths(lengths, B, n)
    if using_partials:
        mode, T, max_w = 1, g2.PARTIAL_FRAMES, max(len(g2.partial_slices(v)[1]) for v in lens)
    else:
        mode, T, max_w = 0, max(1, max(g2.frame_count(v) for v in lens)), 1
    with torch.cuda.device(dev):
        n_valid = torch.tensor(lens, dtype=torch.int32).to(dev)
        win = torch.empty(B * max_w, T, g2.N_MELS, dtype=torch.float32, device=dev)
        wl = torch.empty(B * max_w, dtype=torch.int32, device=dev)
        info = torch.empty(B, 4, dtype=torch.int32, device=dev)
        _lib.check(enc.lib.cmtts_ge2e_features(enc._h, _ptr(wavs), B, n, _ptr(n_valid), int(sample_rate), mode, max_w, T, _ptr(win), _ptr(wl),
                                               _ptr(info), _stream()))
        info = info.cpu().numpy()
    W = int(info[:, 3].sum())
    return win[:W], wl[:W], info


def ge2e_forward(enc: GE2EEncoder, windows, row_map=None, rows=None, lengths=None):
    """cmtts_ge2e_forward: windows fp32 [W, T, 40] (device), lengths int [W] or None, row_map int [W] (host) -> embeddings fp32 [rows, 256]
    (device): per row the normalised mean of its windows' embeddings; row_map None: the W window embeddings themselves."""
    enc._require()
    dev = enc.device
    windows = _f32(windows, dev)
    W, T = int(windows.shape[0]), int(windows.shape[1])
    rm = None
    if row_map is not None:
        rm = np.ascontiguousarray(np.asarray(row_map.cpu() if isinstance(row_map, torch.Tensor) else row_map, np.int32).reshape(-1))
        if rm.size != W:
            raise ValueError("ge2e_forward: one row_map entry per window")
    rows = W if rows is None else int(rows)
    with torch.cuda.device(dev):
        ln = None
        if lengths is not None:
            ln = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
            if ln.numel() != W:
                raise ValueError("ge2e_forward: one length per window")
        emb = torch.empty(rows, 256, dtype=torch.float32, device=dev)
        nb = enc.lib.cmtts_ge2e_workspace_bytes(max(W, 1), max(T, 1))
        ws = enc._ws.get("ge2e", nb, dev)
        _lib.check(enc.lib.cmtts_ge2e_forward(enc._h, _ptr(windows) if W else None, W, max(T, 1), _ptr(ln), None if rm is None else rm.ctypes.data,
                                              rows, _ptr(emb), _ptr(ws), nb, _stream()))
    return emb


def ge2e_embedding(enc: GE2EEncoder, wavs, lengths=None, sample_rate=22050, using_partials=True):
    """ge2e_encoder/inference.py: embed_utterance for a batch — float audio [B, n] (or a list of 1-D arrays) at 22 050 Hz, as the reference
    hands it over: RAW (preprocess_wav — volume normalisation, webrtcvad trim — is not applied on this path, speaker_embedder.py:51) -> a
    DEVICE tensor [B, 256] of unit-norm GE2E vectors, accepted unchanged as spker_embeds= by a model whose external_speaker_dim is 256.
    using_partials=False: each row's whole spectrogram through the network once."""
    win, wl, info = ge2e_features(enc, wavs, lengths, sample_rate, using_partials)
    bad = [b for b in range(info.shape[0]) if info[b, 3] == 0]
    if bad:
        raise ValueError(f"ge2e_embedding: rows {bad} hold no samples")
    if not using_partials:
        return ge2e_forward(enc, win, None, None, wl)
    return ge2e_forward(enc, win, np.repeat(np.arange(info.shape[0], dtype=np.int32), info[:, 3]), info.shape[0])


# ---- recorded speech in (csrc/mel_analysis.hip; definition: cmtts_amd/analysis.py)

class Analyzer:
    """The log-mel / energy analysis on the device (preprocessor/preprocessor.py:44-52: TacotronSTFT): cmtts_analysis_* behind one handle."""

    def __init__(self, preprocess_config=None, device="cuda:0"):
        from . import analysis as an
        from . import resample as rs
        pp = (preprocess_config or {}).get("preprocessing", {})
        stft, mel = pp.get("stft", {}), pp.get("mel", {})
        self.sample_rate = int(pp.get("audio", {}).get("sampling_rate", an.SAMPLE_RATE))
        an.check_geometry(stft.get("filter_length", an.N_FFT), stft.get("hop_length", an.HOP), stft.get("win_length", an.N_FFT),
                          mel.get("n_mel_channels", an.N_MELS))
        if self.sample_rate != rs.NATIVE_RATE:
            raise ValueError(f"get_analyzer: the audio must be at the model's sample rate {rs.NATIVE_RATE} Hz, not {self.sample_rate}")
        self.fmin = float(mel.get("mel_fmin", an.FMIN) or 0.0)
        self.fmax = float(mel.get("mel_fmax", an.FMAX) or self.sample_rate / 2.0)
        self.hop = an.HOP
        self.device = _norm_device(device) if torch.cuda.is_available() else torch.device(device)
        self.lib = _lib.load()
        self._h = C.c_void_p()
        self._ws = _Workspace()
        self._ready = False
        if self.device.type == "cuda" and torch.cuda.is_available():
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cmtts_analysis_create(self.sample_rate, an.N_FFT, an.HOP, an.N_FFT, an.N_MELS, self.fmin, self.fmax, C.byref(self._h)))
            self._ready = True

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:
            self.lib.cmtts_analysis_destroy(h)
            self._h = None

    def _require(self):
        if not self._ready:
            raise RuntimeError("Analyzer: no GPU — cmtts_amd has no CPU fallback (analysis.py is the definition the kernels are tested against)")


def get_analyzer(preprocess_config=None, device="cuda:0"):
    """The analysis the model's features were made with (preprocessor/preprocessor.py:44-52): `preprocess_config` is the preprocess YAML dict
    (default: 22050 Hz, 1024 / 256 / 1024, 80 channels over 0-8000 Hz).  Another STFT geometry or sample rate raises ValueError."""
    return Analyzer(preprocess_config, device)


def _audio_rows(wavs, lengths, what):
    """float or int16 audio as one [B, n] tensor (host or device) and the host-known lengths."""
    if isinstance(wavs, (list, tuple)):
        rows = [torch.as_tensor(np.asarray(w.cpu() if hasattr(w, "cpu") else w)).reshape(-1) for w in wavs]
        if not rows or any(r.dtype != rows[0].dtype for r in rows):
            raise ValueError(f"{what}: the rows must share one dtype")
        if lengths is None:
            lengths = [r.numel() for r in rows]
        wavs = torch.zeros(len(rows), max(1, max(r.numel() for r in rows)), dtype=rows[0].dtype)
        for i, r in enumerate(rows):
            wavs[i, :r.numel()] = r
    wavs = torch.as_tensor(wavs)
    if wavs.dim() == 1:
        wavs = wavs[None]
    if wavs.dim() != 2 or not (wavs.dtype == torch.int16 or wavs.dtype.is_floating_point):
        raise ValueError(f"{what}: float or int16 audio [B, n] expected, not {wavs.dtype} {tuple(wavs.shape)}")
    B, n = wavs.shape
    lens = [n] * B if lengths is None else [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if len(lens) != B or any(v < 0 or v > n for v in lens):
        raise ValueError(f"{what}: one length in [0, {n}] per row")
    return wavs, lens


def mel_from_audio(an: Analyzer, wavs, lengths=None, pad="reference", layout="tc"):
    """Audio.tools.get_mel_from_wav for a batch (cmtts_mel_analysis, one launch): wavs float in [-1, 1] or int16, [B, n] or a list of 1-D rows at
    22050 Hz; lengths: samples per row (default: all).  pad="reference": the framing the acoustic model's mels were made with (1 + n // 256
    frames, n > 512); pad="vocoder": frame f covers samples [256 f, 256 f + 256) (n // 256 frames, n > 384) — the framing for copy synthesis.
    Returns device tensors {"mel": [B, T, 80] (layout="tc", what retake takes) or [B, 80, T] ("ct", what vocoder_infer takes), "mel_lens":
    int64 [B], "energy": fp32 [B, T]} with T the longest row's frame count and zeros beyond a row's frames.  A row at or below the minimum
    length raises ValueError before anything is launched."""
    from . import analysis as A
    wavs, lens = _audio_rows(wavs, lengths, "mel_from_audio")
    if layout not in ("tc", "ct"):
        raise ValueError(f"layout = {layout!r}: expected 'tc' or 'ct'")
    short = [b for b, v in enumerate(lens) if A.frame_count(v, pad) == 0]
    if short:
        raise ValueError(f"mel_from_audio: rows {short} have {A.min_samples(pad)} samples or fewer: too short for pad={pad!r}")
    an._require()
    dev, lib = an.device, an.lib
    B, n = wavs.shape
    T = max(A.frame_count(v, pad) for v in lens)
    i16 = wavs.dtype == torch.int16
    wavs = wavs.to(dev).contiguous() if i16 else _f32(wavs, dev)
    with torch.cuda.device(dev):
        n_valid = torch.tensor(lens, dtype=torch.int32).to(dev)
        mel = torch.empty((B, T, A.N_MELS) if layout == "tc" else (B, A.N_MELS, T), dtype=torch.float32, device=dev)
        energy = torch.empty(B, T, dtype=torch.float32, device=dev)
        frames = torch.empty(B, dtype=torch.int32, device=dev)
        nb = lib.cmtts_analysis_workspace_bytes(B, T)
        ws = an._ws.get("analysis", nb, dev)
        _lib.check(lib.cmtts_mel_analysis(an._h, _ptr(wavs), int(i16), B, n, _ptr(n_valid), 0 if pad == "reference" else 1, T,
                                          0 if layout == "tc" else 1, _ptr(mel), _ptr(energy), _ptr(frames), _ptr(ws), nb, _stream()))
    return {"mel": mel, "mel_lens": frames.to(torch.int64), "energy": energy}


def energy_targets(an: Analyzer, energy, d_targets, mean, std):
    """preprocessor/preprocessor.py:296-305 and its normalisation (cmtts_phoneme_energy, one launch): energy [B, T] from mel_from_audio,
    d_targets int [B, L] (an aligner's durations) -> fp32 [B, L] on the device, accepted unchanged as e_targets= by
    DurationPitchSpeakerNet.forward.  mean, std: stats.json "energy"[2:4]."""
    if np.ndim(energy) != 2 or np.ndim(d_targets) != 2 or energy.shape[0] != d_targets.shape[0]:
        raise ValueError(f"energy_targets: energy {tuple(np.shape(energy))} and d_targets {tuple(np.shape(d_targets))} do not fit [B, T] / [B, L]")
    if not float(std) > 0.0 or math.isnan(float(mean)):
        raise ValueError("energy_targets: std must be positive, mean a number")
    an._require()
    dev = an.device
    energy = _f32(energy, dev)
    d = torch.as_tensor(d_targets).to(device=dev, dtype=torch.int32).contiguous()
    (B, T), L = energy.shape, d.shape[1]
    with torch.cuda.device(dev):
        out = torch.empty(B, L, dtype=torch.float32, device=dev)
        _lib.check(an.lib.cmtts_phoneme_energy(_ptr(energy), B, T, _ptr(d), L, float(mean), float(std), _ptr(out), _stream()))
    return out


def retake_recording_pcm(mel_new, vocoder, pcm_rec, spans, xfade_frames=1):
    """A retake joined into a RECORDING: mel_new [B,80,T] (vocoder_infer's layout) is the recording's mel after retake(..., spans), pcm_rec
    the recording itself (a list of int16 rows, or int16 [B, n]; n <= T * hop).  Spans of one utterance whose fades would touch are merged;
    per merged span only the frames [lo - X, hi + X), X = xfade_frames, are vocoded (cmtts_vocoder_forward_windows_f32 with margin X, in
    windows that reach the generator's receptive radius beyond them), crossfaded on the device (cmtts_pcm_crossfade; the definition:
    analysis.crossfade_splice) and spliced into a copy of the recording.  Returns a list of int16 arrays: the samples of frames [lo, hi) are
    the vocoded audio, the X frames on either side fade linearly between the recording and it — no fade on a side the utterance's start or
    end clips — and every other sample has the recording's bits.  retake_pcm is the counterpart for audio that vocoder_infer made."""
    vocoder._require()
    lib, dev = vocoder.lib, vocoder.device
    x = _f32(mel_new, dev)
    B, M, T = x.shape
    hop, X = vocoder.h.hop, int(xfade_frames)
    if X < 0:
        raise ValueError("retake_recording_pcm: xfade_frames must be >= 0")
    H = lib.cmtts_vocoder_halo_frames(vocoder._h)
    if H < 0:
        _lib.check(H)
    rec = [np.asarray(w.cpu() if hasattr(w, "cpu") else w) for w in pcm_rec]
    if len(rec) != B or any(w.dtype != np.int16 or w.ndim != 1 or len(w) > T * hop for w in rec):
        raise ValueError(f"retake_recording_pcm: pcm_rec must hold {B} int16 rows of at most {T * hop} samples")
    out = [w.copy() for w in rec]
    per = {}
    for b, lo, hi in spans:
        b, lo, hi = int(b), int(lo), int(hi)
        if not 0 <= b < B or not (0 <= lo < hi <= T and (hi - 1) * hop < len(rec[b])):
            raise ValueError(f"retake_recording_pcm: span ({b}, {lo}, {hi}) outside the utterances")
        per.setdefault(b, []).append((lo, hi))
    cores = []          # [b, lo, hi]: the spans of one utterance merged where their fades touch
    for b in sorted(per):
        for lo, hi in sorted(per[b]):
            if cores and cores[-1][0] == b and lo - X <= cores[-1][2] + X:
                cores[-1][2] = max(cores[-1][2], hi)
            else:
                cores.append([b, lo, hi])
    if not cores:
        return out
    core = max(hi - lo for _, lo, hi in cores)
    Tw = core + 2 * X + 2 * H
    if Tw >= T:
        Tw = T
    row = (core + 2 * X) * hop
    wins, tab = [], []
    rec_rows = np.zeros((len(cores), row), np.int16)
    for i, (b, lo, hi) in enumerate(cores):
        start = min(max(lo - X - H, 0), T - Tw)
        wins.append((b, start, lo - start, hi - lo))
        lead, trail, n = min(X, lo), min(X, T - hi), len(rec[b])
        tab.append((lead, hi - lo, trail, (1 if X > 0 and lo - X >= 0 else 0) | (2 if X > 0 and (hi + X) * hop <= n else 0)))
        s0, s1 = (lo - lead) * hop, min((hi + trail) * hop, n)
        rec_rows[i, :s1 - s0] = rec[b][s0:s1]
    N = len(wins)
    with torch.cuda.device(dev):
        wtab = torch.tensor(wins, dtype=torch.int32).pin_memory()      # read in place by the call: kept until the copy below has synchronised
        ftab = torch.tensor(tab, dtype=torch.int32).to(dev)
        rrows = torch.from_numpy(rec_rows).to(dev)
        wav_rows = torch.empty(N, row, dtype=torch.float32, device=dev)
        pcm = torch.empty(N, row, dtype=torch.int16, device=dev)
        nb = lib.cmtts_vocoder_windows_workspace_bytes(vocoder._h, N, Tw)
        ws = vocoder._ws.get("voc_stream", nb, dev)
        _lib.check(lib.cmtts_vocoder_forward_windows_f32(vocoder._h, _ptr(x), B, T, _ptr(wtab), N, Tw, core, X, _ptr(wav_rows), _ptr(ws), nb, _stream()))
        _lib.check(lib.cmtts_pcm_crossfade(_ptr(wav_rows), _ptr(rrows), _ptr(ftab), N, core, X, hop, _ptr(pcm), _stream()))
        arr = pcm.cpu().numpy()
    check_async_error()
    for i, (b, lo, hi) in enumerate(cores):
        lead, trail = tab[i][0], tab[i][2]
        s0, s1 = (lo - lead) * hop, min((hi + trail) * hop, len(rec[b]))
        out[b][s0:s1] = arr[i, :s1 - s0]
    return out


# ---- alignment of a recording to its phonemes (csrc/align.hip; definition: cmtts_amd/align.py)

_ALIGN_WS = _Workspace()
_ALIGN_KEEP = {}        # per device: the host tables of the latest call, read by its copies on the stream


def _align_lengths(what, lens, B, side):
    lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
    if len(lens) != B or any(v < 1 or v > side for v in lens):
        raise ValueError(f"{what}: one length in [1, {side}] per row expected, not {lens}")
    return lens


def _align_mel(what, mel):
    from . import align as A
    shape = tuple(torch.as_tensor(mel).shape) if not hasattr(mel, "shape") else tuple(mel.shape)
    if len(shape) != 3 or shape[2] != A.N_MELS or shape[0] < 1 or not 1 <= shape[1] <= A.MAX_SIDE:
        raise ValueError(f"{what} must be [B, T, {A.N_MELS}] with 1 <= T <= {A.MAX_SIDE}, not {shape}")
    return shape


def dtw_align(mel_syn, syn_lens, d_syn, mel_rec, rec_lens, normalise=True, device=None):
    """Dynamic time warping of a rendering against a recording (cmtts_align_cost, cmtts_align_dtw, cmtts_align_durations; the definition:
    align.py).  mel_syn [B, Ts, 80]: the model's rendering, syn_lens [B] its frames, d_syn int [B, L] its frames per phoneme (sum = syn_lens);
    mel_rec [B, Tr, 80]: the recording's log-mel (mel_from_audio), rec_lens [B].  Returns device tensors {"d_targets": int64 [B, L], the
    recording's frames per phoneme (sum = rec_lens; accepted unchanged as d_targets= and by energy_targets), "phoneme_cost": fp32 [B, L], the
    mean match cost of a phoneme's frames (0 for none), "row": int32 [B, Tr], the rendering frame each recording frame was matched to,
    "cost": fp32 [B], the path's total over its number of points}.  Lengths and shapes that do not fit, more than 4096 frames a side or
    durations that do not sum to syn_lens raise ValueError before a device is asked for."""
    B, Ts, _ = _align_mel("dtw_align: mel_syn", mel_syn)
    Br, Tr, _ = _align_mel("dtw_align: mel_rec", mel_rec)
    if Br != B:
        raise ValueError(f"dtw_align: {B} renderings and {Br} recordings")
    xl = _align_lengths("dtw_align: syn_lens", syn_lens, B, Ts)
    yl = _align_lengths("dtw_align: rec_lens", rec_lens, B, Tr)
    d_host = np.asarray(d_syn.cpu() if hasattr(d_syn, "cpu") else d_syn)
    if d_host.ndim != 2 or d_host.shape[0] != B or d_host.shape[1] < 1 or not np.array_equal(d_host, np.rint(d_host)):
        raise ValueError(f"dtw_align: d_syn must hold integers [B, L], not {d_host.dtype} {d_host.shape}")
    d_host = np.ascontiguousarray(d_host.astype(np.int32))
    if (d_host < 0).any() or d_host.sum(axis=1).tolist() != xl:
        raise ValueError(f"dtw_align: d_syn must be non-negative and sum to syn_lens {xl}, not {d_host.sum(axis=1).tolist()}")
    L = d_host.shape[1]
    if device is None:
        device = next((t.device for t in (mel_syn, mel_rec) if isinstance(t, torch.Tensor) and t.is_cuda), "cuda:0")
    if not torch.cuda.is_available():
        raise RuntimeError("dtw_align: no GPU — cmtts_amd has no CPU fallback (align.py is the definition the kernels are tested against)")
    dev, lib = _norm_device(device), _lib.load()
    x, y = _f32(mel_syn, dev), _f32(mel_rec, dev)
    xl_h, yl_h = np.asarray(xl, np.int32), np.asarray(yl, np.int32)
    _ALIGN_KEEP[dev] = (xl_h, yl_h, d_host)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    with torch.cuda.device(dev):
        d_dev = torch.from_numpy(d_host).to(dev)
        cost = torch.empty(B, Ts, Tr, dtype=torch.float32, device=dev)
        row = torch.zeros(B, Tr, dtype=torch.int32, device=dev)
        total = torch.empty(B, dtype=torch.float32, device=dev)
        n = torch.empty(B, dtype=torch.int32, device=dev)
        d_rec = torch.empty(B, L, dtype=torch.int32, device=dev)
        pc = torch.empty(B, L, dtype=torch.float32, device=dev)
        nb = lib.cmtts_align_workspace_bytes(B, Ts, Tr)
        ws = _ALIGN_WS.get("align", nb, dev)
        _lib.check(lib.cmtts_align_cost(_ptr(x), hp(xl_h), Ts, _ptr(y), hp(yl_h), Tr, B, x.shape[2], int(bool(normalise)), _ptr(cost), _ptr(ws), nb,
                                        _stream()))
        _lib.check(lib.cmtts_align_dtw(_ptr(cost), hp(xl_h), hp(yl_h), B, Ts, Tr, _ptr(row), _ptr(total), _ptr(n), _ptr(ws), nb, _stream()))
        _lib.check(lib.cmtts_align_durations(_ptr(row), _ptr(cost), _ptr(d_dev), hp(d_host), hp(xl_h), hp(yl_h), B, Ts, Tr, L, _ptr(d_rec), _ptr(pc),
                                             _ptr(ws), nb, _stream()))
        return {"d_targets": d_rec.to(torch.int64), "phoneme_cost": pc, "row": row, "cost": total / n.to(torch.float32)}


def align_recording(model: CMTotalTTS, texts, src_lens, mel_rec, rec_lens, spker_embeds=None, speakers=None, n_steps=4, seeds=None):
    """Forced alignment of a recording to its text without a second model: the text and frame side run with every control at 1, the sampler
    renders the phonemes in the given voice (sample_with_cond; `seeds` as there — seeded noise makes the call reproducible, without them the
    noise is drawn from torch's generator), and dtw_align carries the rendering's phoneme boundaries (d_rounded) over to the recording's
    frames.  mel_rec [B, Tr, 80], rec_lens [B]: mel_from_audio's "mel" and "mel_lens".  Returns dtw_align's dict plus "mel_syn" [B, Ts, 80] and
    "d_syn" int32 [B, L].  Limits: a phoneme rendered with 0 frames gets 0 frames; silence the text does not name goes to the
    first or last phoneme.  Shapes that do not fit raise ValueError before a device is asked for."""
    tshape = tuple(torch.as_tensor(texts).shape)
    if len(tshape) != 2:
        raise ValueError("align_recording: texts must be [B, L]")
    B, Tr, _ = _align_mel("align_recording: mel_rec", mel_rec)
    if B != tshape[0]:
        raise ValueError(f"align_recording: {tshape[0]} texts and {B} recordings")
    _align_lengths("align_recording: rec_lens", rec_lens, B, Tr)
    _align_lengths("align_recording: src_lens", src_lens, B, tshape[1])
    if isinstance(n_steps, (list, tuple, np.ndarray, torch.Tensor)) or int(n_steps) < 1:
        raise ValueError("align_recording: n_steps must be one positive int")
    from . import align as A
    model._require()
    out = model.duration_pitch_energy_net(speakers, texts, src_lens, spker_embeds=spker_embeds)
    lens = out["mel_lens"].cpu().tolist()
    T = out["cond_ct"].shape[2]
    if min(lens) < 1 or T > A.MAX_SIDE:
        raise ValueError(f"align_recording: the renderings have {lens} frames; each needs 1 .. {A.MAX_SIDE}")
    if seeds is None:
        n_noise = 1 if n_steps == 1 else n_steps + 1
        noise = torch.randn(n_noise, B, 1, T, model.config.n_mels, dtype=torch.float32, device=model.device)
        mel_syn = sample_with_cond(model, out["cond_ct"], out["speaker_emb"], int(n_steps), noise)
    else:
        mel_syn = sample_with_cond(model, out["cond_ct"], out["speaker_emb"], int(n_steps), seeds=seeds)
    d_syn = out["d_rounded"].to(torch.int32)
    res = dtw_align(mel_syn, lens, d_syn, mel_rec, rec_lens, device=model.device)
    res["mel_syn"], res["d_syn"] = mel_syn, d_syn
    return res


# ---- pitch of a recording (csrc/pitch.hip; definition: cmtts_amd/pitch.py)

class PitchTracker:
    """F0 tracking and the CWT pitch targets on the device (utils/pitch_tools.py:81-118, preprocessor/preprocessor.py:408-414): cmtts_pitch_*
    behind one handle."""

    def __init__(self, preprocess_config=None, device="cuda:0"):
        from . import pitch as P
        from . import resample as rs
        pp = (preprocess_config or {}).get("preprocessing", {})
        pitch = pp.get("pitch", {})
        if pitch.get("pitch_type", "cwt") != "cwt":
            raise ValueError(f"get_pitch_tracker: pitch_type {pitch.get('pitch_type')!r}: only 'cwt' targets are made")
        if pitch.get("pitch_norm", "log") != "log":
            raise ValueError(f"get_pitch_tracker: pitch_norm {pitch.get('pitch_norm')!r}: only 'log' is supported")
        self.sample_rate = int(pp.get("audio", {}).get("sampling_rate", P.SAMPLE_RATE))
        if self.sample_rate != rs.NATIVE_RATE:
            raise ValueError(f"get_pitch_tracker: the audio must be at the model's sample rate {rs.NATIVE_RATE} Hz, not {self.sample_rate}")
        self.geometry = P.Geometry(self.sample_rate, int(pp.get("stft", {}).get("hop_length", P.HOP)), P.FLOOR_HZ, P.CEILING_HZ)
        self.hop, self.lags = self.geometry.hop, self.geometry.LMAX + 2
        self.device = _norm_device(device) if torch.cuda.is_available() else torch.device(device)
        self.lib = _lib.load()
        self._h = C.c_void_p()
        self._ws = _Workspace()
        self._ready = False
        if self.device.type == "cuda" and torch.cuda.is_available():
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cmtts_pitch_create(self.sample_rate, self.hop, P.FLOOR_HZ, P.CEILING_HZ, C.byref(self._h)))
            self._ready = True

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and C is not None:
            self.lib.cmtts_pitch_destroy(h)
            self._h = None

    def _require(self):
        if not self._ready:
            raise RuntimeError("PitchTracker: no GPU — cmtts_amd has no CPU fallback (pitch.py is the definition the kernels are tested against)")

    def _workspace(self, B, T):
        nb = self.lib.cmtts_pitch_workspace_bytes(B, T)
        return self._ws.get("pitch", nb, self.device), nb


def get_pitch_tracker(preprocess_config=None, device="cuda:0"):
    """The pitch analysis the model's pitch targets are made with: `preprocess_config` is the preprocess YAML dict (default: 22050 Hz, hop 256,
    pitch_type "cwt", pitch_norm "log"; floor 80 Hz and ceiling 750 Hz are the reference's constants).  Another pitch_type, pitch_norm or
    sample rate raises ValueError."""
    return PitchTracker(preprocess_config, device)


def _pitch_frames(pt, lens, what):
    from . import pitch as P
    T = max(pt.geometry.frame_count(v) for v in lens)
    if T > P.MAX_FRAMES:
        raise ValueError(f"{what}: {T} frames; at most {P.MAX_FRAMES} per row")
    return T


def pitch_nacf(pt: PitchTracker, wavs, lengths=None):
    """The normalised autocorrelation of every frame (cmtts_pitch_nacf, one launch): wavs float in [-1, 1] or int16, [B, n] or a list of 1-D rows at
    22050 Hz; lengths: samples per row (default: all).  Returns device tensors {"r": fp32 [B, T, LMAX + 2], "pk": fp32 [B, T], "frames":
    int32 [B]} with T = 1 + n // 256 of the longest row: frame f is centred on sample 256 f, as mel frame f of mel_from_audio(pad="reference")."""
    wavs, lens = _audio_rows(wavs, lengths, "pitch_nacf")
    T = _pitch_frames(pt, lens, "pitch_nacf")
    pt._require()
    dev, lib = pt.device, pt.lib
    B, n = wavs.shape
    i16 = wavs.dtype == torch.int16
    wavs = wavs.to(dev).contiguous() if i16 else _f32(wavs, dev)
    with torch.cuda.device(dev):
        n_valid = torch.tensor(lens, dtype=torch.int32).to(dev)
        r = torch.empty(B, T, pt.lags, dtype=torch.float32, device=dev)
        pk = torch.empty(B, T, dtype=torch.float32, device=dev)
        frames = torch.empty(B, dtype=torch.int32, device=dev)
        ws, nb = pt._workspace(B, T)
        _lib.check(lib.cmtts_pitch_nacf(pt._h, _ptr(wavs), int(i16), B, n, _ptr(n_valid), T, _ptr(r), _ptr(pk), _ptr(frames), _ptr(ws), nb, _stream()))
    return {"r": r, "pk": pk, "frames": frames}


def pitch_track(pt: PitchTracker, r, pk, frames):
    """The tracker's path on ANY fp32 r [B, T, LMAX + 2], pk [B, T], frames int [B] (cmtts_pitch_track, two launches) -> {"lag": int32 [B, T]
    (0 = unvoiced), "f0": fp32 [B, T]}: the bits of pitch.track for every input."""
    shape = tuple(np.shape(r))
    if len(shape) != 3 or shape[2] != pt.lags or shape[0] < 1 or shape[1] < 1 or tuple(np.shape(pk)) != shape[:2] or tuple(np.shape(frames)) != shape[:1]:
        raise ValueError(f"pitch_track: r [B, T, {pt.lags}], pk [B, T] and frames [B] expected, not {shape}, {tuple(np.shape(pk))}, {tuple(np.shape(frames))}")
    from . import pitch as P
    if shape[1] > P.MAX_FRAMES:
        raise ValueError(f"pitch_track: at most {P.MAX_FRAMES} frames per row")
    pt._require()
    dev, lib = pt.device, pt.lib
    B, T, _ = shape
    r, pk = _f32(r, dev), _f32(pk, dev)
    frames = torch.as_tensor(frames).to(device=dev, dtype=torch.int32).contiguous()
    with torch.cuda.device(dev):
        lag = torch.empty(B, T, dtype=torch.int32, device=dev)
        f0 = torch.empty(B, T, dtype=torch.float32, device=dev)
        ws, nb = pt._workspace(B, T)
        _lib.check(lib.cmtts_pitch_track(pt._h, _ptr(r), _ptr(pk), _ptr(frames), B, T, _ptr(lag), _ptr(f0), _ptr(ws), nb, _stream()))
    return {"lag": lag, "f0": f0}


def pitch_from_audio(pt: PitchTracker, wavs, lengths=None):
    """utils/pitch_tools.py:81-118 for a batch, per request and on the device (pitch_nacf, pitch_track): returns device tensors {"f0": fp32 [B, T]
    in Hz, 0 where unvoiced, "uv": bool [B, T], "lag": int32 [B, T], "frames": int32 [B]}; zeros (uv False) at and beyond a row's frames."""
    a = pitch_nacf(pt, wavs, lengths)
    t = pitch_track(pt, a["r"], a["pk"], a["frames"])
    T = t["f0"].shape[1]
    inside = torch.arange(T, device=pt.device)[None, :] < a["frames"][:, None]
    return {"f0": t["f0"], "uv": (t["f0"] == 0) & inside, "lag": t["lag"], "frames": a["frames"]}


def pitch_targets_from_f0(pt: PitchTracker, f0, frames, check=True):
    """preprocessor/preprocessor.py:408-414 for a batch (cmtts_pitch_targets, one launch), on a contour that came from pitch_from_audio or from
    elsewhere — a flattened question, a transposed melody: f0 [B, T] in Hz with 0 where unvoiced, frames int [B], 3 <= T <= 4096.  Returns
    the dict DurationPitchSpeakerNet.forward takes as p_targets= — {"cwt_spec": fp32 [B, T, 10], "f0_mean": fp32 [B], "f0_std": fp32 [B],
    "uv": bool [B, T]} — plus "f0" and "status" (int32 [B]: 0 fine, 1 no voiced frame, 2 a constant contour, 3 fewer than 3 frames; the
    reference drops such clips, preprocessor.py:310, 314).  check=True copies the B status ints once and raises ValueError naming the rows
    whose status is not 0; check=False returns them and synchronises nothing."""
    shape = tuple(np.shape(f0))
    from . import pitch as P
    if len(shape) != 2 or shape[0] < 1 or not 3 <= shape[1] <= P.MAX_FRAMES or tuple(np.shape(frames)) != shape[:1]:
        raise ValueError(f"pitch_targets_from_f0: f0 [B, T] with 3 <= T <= {P.MAX_FRAMES} and frames [B] expected, not {shape}, {tuple(np.shape(frames))}")
    pt._require()
    dev, lib = pt.device, pt.lib
    B, T = shape
    f0 = _f32(f0, dev)
    frames = torch.as_tensor(frames).to(device=dev, dtype=torch.int32).contiguous()
    with torch.cuda.device(dev):
        cwt = torch.empty(B, T, P.CWT_SCALES, dtype=torch.float32, device=dev)
        mean = torch.empty(B, dtype=torch.float32, device=dev)
        std = torch.empty(B, dtype=torch.float32, device=dev)
        uv = torch.empty(B, T, dtype=torch.uint8, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        ws, nb = pt._workspace(B, T)
        _lib.check(lib.cmtts_pitch_targets(pt._h, _ptr(f0), _ptr(frames), B, T, _ptr(cwt), _ptr(mean), _ptr(std), _ptr(uv), _ptr(status), _ptr(ws), nb,
                                           _stream()))
    if check:
        bad = {b: s for b, s in enumerate(status.cpu().tolist()) if s != 0}
        if bad:
            why = {1: "no voiced frame", 2: "a constant contour", 3: "fewer than 3 frames"}
            raise ValueError("pitch_targets: no CWT targets for rows " + ", ".join(f"{b} ({why.get(s, s)})" for b, s in bad.items()))
    return {"cwt_spec": cwt, "f0_mean": mean, "f0_std": std, "uv": uv.view(torch.bool), "f0": f0, "status": status}


def pitch_targets(pt: PitchTracker, wavs, lengths=None, check=True):
    """The pitch targets of recordings: pitch_from_audio, then pitch_targets_from_f0 (four launches in all).  Rows shorter than 3 frames
    (512 samples) raise ValueError before a device is asked for."""
    wavs, lens = _audio_rows(wavs, lengths, "pitch_targets")
    short = [b for b, v in enumerate(lens) if pt.geometry.frame_count(v) < 3]
    if short:
        raise ValueError(f"pitch_targets: rows {short} have fewer than 3 frames ({2 * pt.hop} samples)")
    _pitch_frames(pt, lens, "pitch_targets")
    p = pitch_from_audio(pt, wavs, lens)
    return pitch_targets_from_f0(pt, p["f0"], p["frames"], check=check)


# ---- objective metrics of a rendering against its recording (csrc/metrics.hip; definition: cmtts_amd/metrics.py)

_METRIC_WS = _Workspace()
_METRIC_TABLES = {}      # (device, n_cep) -> the DCT table on that device
_METRIC_KEEP = {}        # per device: the host lengths of the latest call, read by the DTW's copies on the stream


def _metric_table(lib, dev, n_cep):
    key = (str(dev), n_cep)
    if key not in _METRIC_TABLES:
        from . import metrics as M
        tab = np.empty((M.N_MELS, n_cep), np.float32)
        _lib.check(lib.cmtts_metric_dct_table(M.N_MELS, n_cep, C.c_void_p(tab.ctypes.data)))
        _METRIC_TABLES[key] = torch.from_numpy(tab).to(dev)
    return _METRIC_TABLES[key]


def _metric_lengths(what, lens, B, side, lo=1):
    lens = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
    if len(lens) != B or any(v < lo or v > side for v in lens):
        raise ValueError(f"{what}: one length in [{lo}, {side}] per row expected, not {lens}")
    return lens


def _metric_device(device, *tensors):
    if device is None:
        device = next((t.device for t in tensors if isinstance(t, torch.Tensor) and t.is_cuda), "cuda:0")
    if not torch.cuda.is_available():
        raise RuntimeError("metrics: no GPU — cmtts_amd has no CPU fallback (metrics.py is the definition the kernels are tested against)")
    return _norm_device(device)


def mel_cepstra(mel, lens, n_cep=20, device=None):
    """The cepstra the metrics are made of (cmtts_metric_cepstra, one launch): mel [B, T, 80] natural-log mel (mel_from_audio, or the model's
    rendering), lens [B] frames per row (0 .. T) -> fp32 [B, T, n_cep] on the device, the orthonormal DCT-II over the mel channels; rows at
    and beyond a row's frames are zeros.  The table is made once per device and n_cep.  These are NOT WORLD / SPTK mel-cepstra (metrics.py)."""
    from . import metrics as M
    B, T, _ = _align_mel("mel_cepstra: mel", mel)
    n_cep = int(n_cep)
    if not 1 <= n_cep <= M.N_MELS:
        raise ValueError(f"mel_cepstra: 1 <= n_cep <= {M.N_MELS}, not {n_cep}")
    lens = _metric_lengths("mel_cepstra: lens", lens, B, T, lo=0)
    dev, lib = _metric_device(device, mel), _lib.load()
    x = _f32(mel, dev)
    with torch.cuda.device(dev):
        ld = torch.tensor(lens, dtype=torch.int32).to(dev)
        out = torch.zeros(B, T, n_cep, dtype=torch.float32, device=dev)
        _lib.check(lib.cmtts_metric_cepstra(_ptr(x), _ptr(ld), _ptr(_metric_table(lib, dev, n_cep)), B, T, M.N_MELS, n_cep, _ptr(out), _stream()))
    return out


def score_pairs(mel_syn, syn_lens, mel_rec, rec_lens, f0_syn=None, f0_rec=None, align="dtw", mcd_coefs=(1, 13), ssim_coefs=20, data_range=None,
                emb_syn=None, emb_rec=None, device=None):
    """How close B renderings are to the recordings they were made from (cmtts_metric_*, cmtts_align_dtw; the definition: metrics.py, which says
    where this differs from the reference's all_metrics.py).  mel_syn [B, Ts, 80], syn_lens [B]; mel_rec [B, Tr, 80], rec_lens [B] (mel_from_audio);
    f0_syn [B, Ts], f0_rec [B, Tr] in Hz with 0 = unvoiced (pitch_from_audio), both or neither.  align="dtw": the exact DTW of align.py on the
    cepstral cost; "frame": frame i against frame i.  mcd_coefs (k_lo, k_hi): the cepstra of the distortion (c0 excluded by default);
    ssim_coefs: the first C cepstra make the images; data_range: the SSIM's L (default: max - min over the pairs of this call, taken on the
    device).  Returns device tensors [B]: "mcd" (dB, of this project's cepstra), "ssim", "path_len", "row" int32 [B, Tr] (the rendering frame
    per recording frame); with F0 "ffe", "gpe", "vde", "f0_rmse_cents", "f0_mae_cents", "f0_corr" (NaN where undefined) and "counts" int32
    [B, 4] = (n, n_vv, n_gpe, n_vde); with emb_syn, emb_rec [B, D] "speaker_cos" (all_metrics.py:562-602).  Nothing is copied to the host.
    Shapes and lengths that do not fit raise ValueError before a device is asked for."""
    from . import metrics as M
    B, Ts, _ = _align_mel("score_pairs: mel_syn", mel_syn)
    Br, Tr, _ = _align_mel("score_pairs: mel_rec", mel_rec)
    if Br != B:
        raise ValueError(f"score_pairs: {B} renderings and {Br} recordings")
    if B > 65535:
        raise ValueError("score_pairs: at most 65535 pairs per call")
    xl = _metric_lengths("score_pairs: syn_lens", syn_lens, B, Ts)
    yl = _metric_lengths("score_pairs: rec_lens", rec_lens, B, Tr)
    if align not in ("dtw", "frame"):
        raise ValueError(f"score_pairs: align = {align!r}: expected 'dtw' or 'frame'")
    if (f0_syn is None) != (f0_rec is None):
        raise ValueError("score_pairs: f0_syn and f0_rec go together")
    if f0_syn is not None and (tuple(f0_syn.shape) != (B, Ts) or tuple(f0_rec.shape) != (B, Tr)):
        raise ValueError(f"score_pairs: f0_syn [{B}, {Ts}] and f0_rec [{B}, {Tr}] expected, not {tuple(f0_syn.shape)}, {tuple(f0_rec.shape)}")
    if (emb_syn is None) != (emb_rec is None):
        raise ValueError("score_pairs: emb_syn and emb_rec go together")
    if emb_syn is not None and (len(emb_syn.shape) != 2 or tuple(emb_syn.shape) != tuple(emb_rec.shape) or emb_syn.shape[0] != B):
        raise ValueError(f"score_pairs: emb_syn and emb_rec must both be [{B}, D], not {tuple(emb_syn.shape)}, {tuple(emb_rec.shape)}")
    k_lo, k_hi = (int(v) for v in mcd_coefs)
    C_img = int(ssim_coefs)
    if not 0 <= k_lo <= k_hi < M.N_MELS or not 1 <= C_img <= M.N_MELS:
        raise ValueError(f"score_pairs: mcd_coefs {mcd_coefs} must lie in 0 .. {M.N_MELS - 1} and ssim_coefs {ssim_coefs} in 1 .. {M.N_MELS}")
    if data_range is not None and not float(data_range) > 0.0:
        raise ValueError("score_pairs: data_range must be positive")
    n_cep = max(k_hi + 1, C_img)
    dev, lib = _metric_device(device, mel_syn, mel_rec), _lib.load()
    x, y = _f32(mel_syn, dev), _f32(mel_rec, dev)
    xl_h, yl_h = np.asarray(xl, np.int32), np.asarray(yl, np.int32)
    _METRIC_KEEP[dev] = (xl_h, yl_h)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    with torch.cuda.device(dev):
        st = _stream()
        tab = _metric_table(lib, dev, n_cep)
        xl_d, yl_d = torch.from_numpy(xl_h).to(dev), torch.from_numpy(yl_h).to(dev)
        cx = torch.zeros(B, Ts, n_cep, dtype=torch.float32, device=dev)
        cy = torch.zeros(B, Tr, n_cep, dtype=torch.float32, device=dev)
        _lib.check(lib.cmtts_metric_cepstra(_ptr(x), _ptr(xl_d), _ptr(tab), B, Ts, M.N_MELS, n_cep, _ptr(cx), st))
        _lib.check(lib.cmtts_metric_cepstra(_ptr(y), _ptr(yl_d), _ptr(tab), B, Tr, M.N_MELS, n_cep, _ptr(cy), st))
        cost = torch.empty(B, Ts, Tr, dtype=torch.float32, device=dev)
        _lib.check(lib.cmtts_metric_cost(_ptr(cx), _ptr(xl_d), Ts, _ptr(cy), _ptr(yl_d), Tr, B, n_cep, k_lo, k_hi, _ptr(cost), st))
        total = torch.empty(B, dtype=torch.float32, device=dev)
        n = torch.empty(B, dtype=torch.int32, device=dev)
        if align == "dtw":
            row = torch.zeros(B, Tr, dtype=torch.int32, device=dev)
            nb = lib.cmtts_align_workspace_bytes(B, Ts, Tr)
            ws = _ALIGN_WS.get("align", nb, dev)
            _lib.check(lib.cmtts_align_dtw(_ptr(cost), hp(xl_h), hp(yl_h), B, Ts, Tr, _ptr(row), _ptr(total), _ptr(n), _ptr(ws), nb, st))
            row_arg = _ptr(row)
        else:
            _lib.check(lib.cmtts_metric_diagonal(_ptr(cost), _ptr(xl_d), _ptr(yl_d), B, Ts, Tr, _ptr(total), _ptr(n), st))
            j = torch.arange(Tr, dtype=torch.int32, device=dev)[None, :]
            row = torch.where(j < yl_d[:, None], torch.minimum(j, xl_d[:, None] - 1), torch.zeros_like(j))
            row_arg = None
        out = {"mcd": (total.double() * M.MCD_CONST / n.double()).float(), "row": row, "path_len": n}
        u = torch.empty(B, Tr, C_img, dtype=torch.float32, device=dev)
        v = torch.empty(B, Tr, C_img, dtype=torch.float32, device=dev)
        mm = torch.empty(B, 2, dtype=torch.float32, device=dev)
        _lib.check(lib.cmtts_metric_ssim_prepare(_ptr(cx), _ptr(xl_d), Ts, _ptr(cy), _ptr(yl_d), Tr, row_arg, B, n_cep, C_img, _ptr(u), _ptr(v),
                                                 _ptr(mm), st))
        if data_range is None:
            rng = (mm[:, 1].max() - mm[:, 0].min()).reshape(1)
        else:
            rng = torch.full((1,), float(data_range), dtype=torch.float32, device=dev)
        ssim = torch.empty(B, dtype=torch.float32, device=dev)
        nb = lib.cmtts_metric_workspace_bytes(B, Tr, C_img)
        ws = _METRIC_WS.get("ssim", nb, dev)
        _lib.check(lib.cmtts_metric_ssim(_ptr(u), _ptr(v), _ptr(yl_d), B, Tr, C_img, _ptr(rng), _ptr(ssim), _ptr(ws), nb, st))
        out["ssim"], out["data_range"] = ssim, rng
        if f0_syn is not None:
            fs, fr = _f32(f0_syn, dev), _f32(f0_rec, dev)
            counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
            vals = torch.empty(B, 3, dtype=torch.float32, device=dev)
            _lib.check(lib.cmtts_metric_f0(_ptr(fs), _ptr(xl_d), Ts, _ptr(fr), _ptr(yl_d), Tr, row_arg, B, _ptr(counts), _ptr(vals), st))
            c = counts.double()
            out["counts"] = counts
            out["ffe"], out["gpe"], out["vde"] = ((c[:, 2] + c[:, 3]) / c[:, 0]).float(), (c[:, 2] / c[:, 1]).float(), (c[:, 3] / c[:, 0]).float()
            out["f0_rmse_cents"], out["f0_mae_cents"], out["f0_corr"] = vals[:, 0], vals[:, 1], vals[:, 2]
        if emb_syn is not None:
            out["speaker_cos"] = torch.nn.functional.cosine_similarity(_f32(emb_syn, dev), _f32(emb_rec, dev), dim=1)
    return out


def score_audio(an: Analyzer, pt: PitchTracker, wav_syn, wav_rec, lengths_syn=None, lengths_rec=None, **kw):
    """score_pairs on two batches of audio at 22050 Hz (float in [-1, 1] or int16, [B, n] or lists of rows): mel_from_audio(pad="reference") and
    pitch_from_audio for both sides, everything on the device.  The two analyses must agree on every row's frame count (they do at hop 256:
    1 + n // 256); otherwise ValueError.  **kw: score_pairs' align, mcd_coefs, ssim_coefs, data_range, emb_syn, emb_rec."""
    from . import analysis as A
    sides = []
    for what, wav, lengths in (("wav_syn", wav_syn, lengths_syn), ("wav_rec", wav_rec, lengths_rec)):
        wav, lens = _audio_rows(wav, lengths, f"score_audio: {what}")
        mel_frames = [A.frame_count(v, "reference") for v in lens]
        f0_frames = [pt.geometry.frame_count(v) for v in lens]
        if mel_frames != f0_frames:
            raise ValueError(f"score_audio: {what}: the mel analysis gives {mel_frames} frames and the pitch analysis {f0_frames}")
        sides.append((wav, lens, mel_frames))
    if len(sides[0][1]) != len(sides[1][1]):
        raise ValueError(f"score_audio: {len(sides[0][1])} renderings and {len(sides[1][1])} recordings")
    feats = []
    for wav, lens, frames in sides:
        m = mel_from_audio(an, wav, lens, pad="reference")
        p = pitch_from_audio(pt, wav, lens)
        feats.append((m["mel"], frames, p["f0"]))
    (ms, ls, fs), (mr, lr, fr) = feats
    return score_pairs(ms, ls, mr, lr, f0_syn=fs, f0_rec=fr, device=an.device, **kw)


class PreDefinedEmbedder(torch.nn.Module):
    """model/speaker_embedder.py:11-42 — forward(audio) -> numpy (1, 512) for "DeepSpeaker", (1, 256) for "GE2E".  config: the preprocess YAML
    dict.  DeepSpeaker: the ResCNN's weights come from `weights` (default: the reference's checkpoint path, which needs h5py; see
    weights.import_deepspeaker).  GE2E: the LSTM encoder's from `weights` or config["preprocessing"]["ge2e_speaker_embedder_path"]
    (weights.import_ge2e); the audio goes in raw, as in the reference (speaker_embedder.py:51)."""

    _DEEPSPEAKER_CKPT = "./deepspeaker/pretrained_models/ResCNN_triplet_training_checkpoint_265.h5"

    def __init__(self, config, weights=None, device="cuda:0"):
        super().__init__()
        self.sampling_rate = config["preprocessing"]["audio"]["sampling_rate"]
        self.win_length = config["preprocessing"]["stft"]["win_length"]
        self.embedder_type = config["preprocessing"]["speaker_embedder"]
        if self.embedder_type == "DeepSpeaker":
            self.embedder = get_speaker_encoder(self._DEEPSPEAKER_CKPT if weights is None else weights, device)
        elif self.embedder_type == "GE2E":
            if weights is None:
                weights = config["preprocessing"].get("ge2e_speaker_embedder_path")
            if weights is None:
                raise ValueError('PreDefinedEmbedder: "GE2E" needs weights= or preprocessing.ge2e_speaker_embedder_path')
            self.embedder = get_ge2e_encoder(weights, device)
        else:
            raise NotImplementedError(f"speaker embedder {self.embedder_type!r}")

    def forward(self, audio):
        audio = np.asarray(audio.detach().cpu() if isinstance(audio, torch.Tensor) else audio, np.float32).reshape(1, -1)
        if self.embedder_type == "GE2E":
            return ge2e_embedding(self.embedder, audio, None, self.sampling_rate).cpu().numpy()
        return speaker_embedding(self.embedder, audio, None, self.sampling_rate, self.win_length).cpu().numpy()


# ---- a batch that starts from TEXT, sharded over the ranks of a process group by predicted mel length (shard.two_phase): the text
# side of each rank's slice, its per-utterance state packed into records (cmtts_text_state_pack), the lengths agreed, the records moved
# to the ranks the plan gives them, unpacked into one text workspace per bucket (cmtts_text_state_unpack) and the frame side + sampler
# of every bucket group run there (one cmtts_sample_ragged call for the rank's groups, like BucketedSynthesizer).

def utterance_noise(seed, index, n_noise, T, n_mels, device):
    """The sampler's noise [n_noise, 1, T, n_mels] of ONE utterance, drawn from a generator seeded by (seed, global utterance index):
    an utterance gets the same noise whatever the world size and whichever rank computes it."""
    g = torch.Generator(device=device)
    g.manual_seed((int(seed) * 1000003 + int(index)) % (1 << 63))
    return torch.randn(n_noise, 1, int(T), int(n_mels), generator=g, device=device)


def text_state_records(model: CMTotalTTS, texts, src_lens, lo, hi, spker_embeds=None, speakers=None, d_control=1.0,
                       e_control=1.0, p_control=1.0, target_frames=None, segments=None):
    """Text side of utterances [lo, hi) of a batch padded to L_all = texts.shape[1] phonemes (the reference's batch padding,
    cmtts_text_forward), packed into text-state records.  Returns (records uint8 [hi - lo, R], mel_len int64 [hi - lo]) on the
    model's device.  d_control / e_control / p_control: numbers, or float32 tensors [B] / [B, L_all] over the WHOLE batch (global
    utterance index): rows [lo, hi) are the tables of this call; with a p_control table the records carry its rows (layout
    revision 2) for the frame side.  A scalar e_control / p_control other than 1 is set with cmtts_set_variance_controls by the
    caller around both phases (synthesize_sharded), not here.
    target_frames / segments: duration targets over the WHOLE batch ([B] / [B, G] and [B, L_all], global utterance index), rows
    [lo, hi) taken here; the records carry the fitted cum, so the frame side needs nothing more.  A segment that cannot be met
    raises ValueError (one read-back of hi - lo counters)."""
    o = model
    L = int(texts.shape[1])
    (p_s, e_s, d_control), tabs = _resolve_controls(int(texts.shape[0]), L, p_control, e_control, d_control)
    targets = _resolve_targets(int(texts.shape[0]), L, target_frames, segments)
    if p_s != 1.0 or e_s != 1.0:
        raise ValueError("text_state_records: scalar p_control / e_control are variance controls of both phases "
                         "(cmtts_set_variance_controls around them, as synthesize_sharded does); pass tables or 1.0 here")
    o._require()
    cfg, lib, dev = o.config, o.lib, o.device
    n = hi - lo
    if n <= 0:
        inst = _InstalledTables(o, tabs, L, present_only=tuple(tabs))
        try:
            R = lib.cmtts_text_state_record_bytes(o._h, L)
        finally:
            inst.clear()
        return torch.empty(0, R, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    tx = _i64(texts[lo:hi], dev)
    sl = _i64(src_lens[lo:hi], dev)
    table = cfg.multi_speaker and cfg.n_speaker > 0
    spk_in = _f32(spker_embeds[lo:hi], dev) if (cfg.multi_speaker and not table) else None
    ids = _i64(speakers[lo:hi], dev) if table else None
    if cfg.multi_speaker and not table and spker_embeds is None:
        raise AssertionError("Speaker embedding should not be None")
    _check_speaker_width(cfg, spk_in, hi - lo)
    if table:
        if speakers is None:
            raise AssertionError("speakers (ids into the speaker_emb table) should not be None")
        if int(ids.min()) < 0 or int(ids.max()) >= cfg.n_speaker:
            raise IndexError("index out of range in self")
    with torch.cuda.device(dev):
        mel_len = torch.empty(n, dtype=torch.int64, device=dev)
        nb = lib.cmtts_text_workspace_bytes(o._h, n, L)
        tws = o._ws.get("text_sharded", nb, dev)
        inst = fit = None
        try:
            inst = _InstalledTables(o, tabs, L, lo, hi)      # this rank's utterances, selected by global index
            fit = _InstalledTargets(o, targets, L, lo, hi)
            R = lib.cmtts_text_state_record_bytes(o._h, L)
            _lib.check(lib.cmtts_text_forward(o._h, _ptr(tx), _ptr(sl), _ptr(spk_in), _ptr(ids), n, L, float(d_control),
                                              None, None, _ptr(mel_len), None, None, None, None, _ptr(tws), nb, _stream()))
            rows = torch.arange(n, dtype=torch.int32, device=dev)
            gidx = torch.arange(lo, hi, dtype=torch.int64, device=dev)
            records = torch.empty(n, R, dtype=torch.uint8, device=dev)
            _lib.check(lib.cmtts_text_state_pack(o._h, _ptr(tws), n, L, _ptr(rows), n, _ptr(gidx), _ptr(sl), _ptr(records), _stream()))
            fit.raise_unmet(lo)
        finally:
            if fit is not None:
                fit.clear()
            if inst is not None:
                inst.clear()
    return records, mel_len


def frame_side_from_records(model: CMTotalTTS, groups, L_all, n_steps=4, seed=0, tail_frames=16, details=None, p_control=1.0, seeds=None):
    """groups: [(bucket, records uint8 [n, R], utterance ids [n], planned lengths [n])] (shard.two_phase).  Every group's records are
    unpacked into a text workspace of its own, its frame side runs with T = bucket, and ONE cmtts_sample_ragged call samples all
    groups (each utterance trimmed to its planned length + tail_frames) with utterance_noise(seed, id).  Returns [(mel [n, bucket, 80],
    mel_len int64 [n])]; `details` (a list) receives one {"mel2ph", "p_idx", "cwt", "ids"} per group.
    p_control: what the text side was given (a number, or a float32 tensor [B] / [B, L_all] over the whole batch).  A table's rows
    arrive in the records (layout revision 2); here it only says that they do — every rank must agree on that, record sizes depend
    on it.  A number other than 1 is the caller's cmtts_set_variance_controls around both phases (synthesize_sharded).
    seeds: int64 numpy / CPU tensor indexed by GLOBAL utterance id — seeded noise (one cmtts_noise_fill_groups launch for all
    groups) in place of utterance_noise(seed, id)."""
    from . import shard
    cfg, lib, dev = model.config, model.lib, model.device
    p_tab = None
    if isinstance(p_control, (torch.Tensor, np.ndarray)):
        pt = torch.as_tensor(p_control)
        if pt.dim() not in (1, 2) or (pt.dim() == 2 and int(pt.shape[1]) != int(L_all)):
            raise ValueError(f"p_control: shape {tuple(pt.shape)}, expected [B] or [B, {int(L_all)}]")
        _, tabs = _resolve_controls(int(pt.shape[0]), int(L_all), p_control)
        p_tab = {"p": tabs["p"]}
    n_noise = 1 if n_steps == 1 else n_steps + 1
    lay = shard.text_state_layout(cfg.hidden, cfg.cwt_hidden, L_all, with_p=p_tab is not None)
    p1_ld = (L_all + 3) // 4 * 4
    use_p1 = getattr(model, "_precision_mode", 0) == 0 and model._cond_factors
    inst = _InstalledTables(model, p_tab or {}, L_all, present_only=("p",))
    try:
        return _frame_side_from_records(model, groups, L_all, n_steps, seed, tail_frames, details, lay, p1_ld, use_p1, n_noise, seeds)
    finally:
        inst.clear()


def _frame_side_from_records(model, groups, L_all, n_steps, seed, tail_frames, details, lay, p1_ld, use_p1, n_noise, seeds=None):
    from . import shard
    cfg, lib, dev = model.config, model.lib, model.device
    sample_groups, lens = [], []
    with torch.cuda.device(dev):
        seeded = None
        if seeds is not None:
            sv = seeds.cpu().numpy() if isinstance(seeds, torch.Tensor) else np.asarray(seeds)
            seeded = seeded_noise_groups([(sv[[int(i) for i in ids]], int(bucket)) for bucket, _, ids, _ in groups], n_noise, cfg.n_mels, dev)
        f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        for k, (bucket, rec, ids, planned) in enumerate(groups):
            n, T = len(ids), int(bucket)
            rec = rec.to(dev).contiguous()
            nb = lib.cmtts_text_workspace_bytes(model._h, n, L_all)
            tws = model._ws.get(("text_unpacked", k), nb, dev)
            _lib.check(lib.cmtts_text_state_unpack(model._h, _ptr(rec), n, L_all, _ptr(tws), nb, _stream()))
            cond_ct = f(n, cfg.hidden, T)
            mel2ph = torch.empty(n, T, dtype=torch.int64, device=dev)
            p_idx = torch.empty(n, T, dtype=torch.int64, device=dev)
            p1 = f(n, cfg.res_layers * cfg.res_channels, p1_ld) if use_p1 else None
            p1t = None if p1 is None else f(n, cfg.res_layers, p1_ld, cfg.res_channels)
            nf = lib.cmtts_frame_workspace_bytes(model._h, n, T)
            fws = model._ws.get(("frame_unpacked", k), nf, dev)
            cwt = f(n, T, cfg.cwt_out) if details is not None else None
            _lib.check(lib.cmtts_frame_forward_sub_t(model._h, _ptr(tws), n, L_all, 0, n, T, _ptr(cond_ct), _ptr(mel2ph), _ptr(cwt), None,
                                                     _ptr(p_idx), None, _ptr(p1), _ptr(p1t), _ptr(fws), nf, _stream()))
            factors = None if p1 is None else CondFactors(p1, p1_ld, L_all, mel2ph, p_idx, cond_ct, p1t)
            spk = shard.text_state_region(rec, lay, "spk") if cfg.multi_speaker else None
            noise = seeded[k] if seeded is not None else torch.stack([utterance_noise(seed, i, n_noise, T, cfg.n_mels, dev) for i in ids], 1)
            sample_groups.append((cond_ct, spk, noise, [int(t) for t in planned], factors))
            lens.append(torch.tensor([int(t) for t in planned], dtype=torch.int64, device=dev))
            if details is not None:
                details.append({"mel2ph": mel2ph, "p_idx": p_idx, "cwt": cwt, "ids": list(ids)})
        mels = sample_ragged(model, sample_groups, n_steps, tail_frames)
    return list(zip(mels, lens))


def synthesize_sharded(model: CMTotalTTS, texts, src_lens, spker_embeds=None, speakers=None, n_steps=4, group=None, seed=0,
                       buckets=None, vocoder=None, d_control=1.0, p_control=1.0, e_control=1.0, tail_frames=16, max_wav_value=32768.0,
                       seeds=None, target_frames=None, segments=None):
    """A batch of texts (synthesize.py batch mode: texts int64 [B, L], src_lens [B], the same on every rank) over the ranks of
    `group` (torch.distributed; none initialised = one rank): text side of this rank's slice (shard.shard_range), lengths agreed,
    text-state records moved to the ranks of the agreed plan_shards(mel_len) (shard.two_phase), frame side and sampler per bucket,
    the mels of every rank all-gathered once.  An utterance longer than the largest bucket is truncated to it and reported.
    Noise is drawn per utterance from (seed, global index) (utterance_noise): results do not depend on the world size.
    seeds: int64 [B] utterance seeds by GLOBAL utterance (the same on every rank), or one int (noise.utterance_seeds(int, arange(B))):
    seeded noise instead (seeded_noise_groups, one launch per rank) — an utterance's noise then follows its seed, not its position.
    Returns {"mels": [mel [len_i, 80]] in input order (every rank), "mel_len": the predicted lengths, "truncated": indices,
    "plan": the plan; with `vocoder`: "wavs": [int16 [len_i * 256]] (shard.allgather_pcm per bucket)}.
    d_control / p_control / e_control: numbers, or float32 tensors [B] (per utterance) / [B, L] (per phoneme, L = texts.shape[1])
    indexed by GLOBAL utterance: every rank passes the same tables, each takes the rows of its own utterances for the text
    side, and the pitch rows travel inside the text-state records to the rank that runs the utterance's frame side.
    target_frames / segments: duration targets by GLOBAL utterance ([B] / [B, G] and [B, L]; DurationPitchSpeakerNet.forward): each
    rank fits the rows of its own slice, and the fitted lengths are what the ranks agree the plan on."""
    from . import shard
    if not isinstance(n_steps, (int, np.integer)):
        raise NotImplementedError("synthesize_sharded: per-utterance step counts are not supported on the sharded path (one int; "
                                  "CMTotalTTSSynthesize.synthesize and synthesize_stream take a sequence)")
    if buckets is None:
        buckets = shard.FRAME_BUCKETS
    texts = torch.as_tensor(texts)
    src_lens = torch.as_tensor(src_lens)
    L_all = int(src_lens.max())                       # the reference's batch padding: the longest utterance of the batch
    n_items = int(texts.shape[0])
    if seeds is not None:
        seeds = _device_seeds(seeds, n_items, "cpu").numpy()
    (p_control, e_control, d_control), tabs = _resolve_controls(n_items, int(texts.shape[1]), p_control, e_control, d_control)
    tabs = {k: t[:, :L_all].contiguous() for k, t in tabs.items()}      # the tables are as wide as `texts` and cut with it
    targets = _resolve_targets(n_items, int(texts.shape[1]), target_frames, segments)
    tf_arg = None if targets is None else (targets[0] if targets[1] is not None else targets[0][:, 0])
    seg_arg = None if targets is None or targets[1] is None else targets[1][:, :L_all].contiguous()
    texts = texts[:, :L_all]
    d_arg, e_arg, p_arg = tabs.get("d", d_control), tabs.get("e", 1.0), tabs.get("p", 1.0)
    model._require()
    _note_process_group(model.lib)
    vc = None
    if p_control != 1.0 or e_control != 1.0:
        vc = _lib.VarianceControlsStruct(p_control=float(p_control), e_control=float(e_control))
        _lib.check(model.lib.cmtts_set_variance_controls(model._h, C.byref(vc)))
    try:
        res = shard.two_phase(
            n_items,
            lambda lo, hi: text_state_records(model, texts, src_lens, lo, hi, spker_embeds, speakers, d_arg, e_arg, p_arg,
                                              target_frames=tf_arg, segments=seg_arg),
            lambda groups: frame_side_from_records(model, groups, L_all, n_steps, seed, tail_frames, p_control=p_arg, seeds=seeds),
            group=group, buckets=buckets)
        if vocoder is not None:
            wavs = [None] * n_items
            for b, (mel, mel_len) in sorted(res["local"].items()):
                pcm = vocoder_infer_device(mel.transpose(1, 2).contiguous(), vocoder, max_wav_value)
                hop = pcm.shape[1] // mel.shape[1]
                all_pcm, all_len = shard.allgather_pcm(pcm, mel_len * hop, group)
                for row, i in enumerate(i for r in res["plan"][b] for i in r):
                    if i >= 0:
                        wavs[i] = all_pcm[row, :int(all_len[row])]
            res["wavs"] = wavs
    finally:
        if vc is not None:
            model.lib.cmtts_set_variance_controls(model._h, None)
            torch.cuda.current_stream(model.device).synchronize()
    check_async_error()
    return res
