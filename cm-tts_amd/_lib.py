"""Binding of libcmtts_hip.so (the C ABI in include/cmtts_hip.h): ctypes by default; cffi in ABI mode
(BASELINE.json north_star: "a thin C-ABI cffi layer"; declarations parsed from the header itself) with ``CMTTS_FFI=cffi`` —
``cffi`` is not installed in this image, so ctypes is what runs here and what the tests exercise, and the
cffi adapter stays opt-in until it has run somewhere; both bind the same symbols with the same signatures behind the same call sites.
There is NO compute fallback: if the shared library is missing or a symbol is absent the import of the compute path
fails loudly.
"""
import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CMTTS_LIB") or os.path.join(_HERE, "libcmtts_hip.so")     # CMTTS_LIB: an experimental build of the same ABI (tools/)


class CMTTSConfigStruct(C.Structure):
    """struct cmtts_config (include/cmtts_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "n_symbols", "hidden", "enc_layers", "enc_heads", "ffn_kernel",
        "pred_filter", "pred_layers", "pred_kernel", "dur_layers", "dur_kernel", "cwt_hidden",
        "pitch_bins", "energy_bins", "use_uv", "multi_speaker", "external_speaker_dim", "n_speaker",
        "n_mels", "res_layers", "res_channels")] + [(n, C.c_float) for n in (
            "cwt_std_scale", "pitch_norm_eps", "sigma_min", "sigma_max", "sigma_data", "rho")]


class VarianceControlsStruct(C.Structure):
    """struct cmtts_variance_controls (include/cmtts_hip.h): device pointers as void*."""
    _fields_ = [("p_control", C.c_float), ("e_control", C.c_float), ("d_target", C.c_void_p), ("e_target", C.c_void_p),
                ("cwt_spec", C.c_void_p), ("f0_mean", C.c_void_p), ("f0_std", C.c_void_p), ("uv", C.c_void_p)]


class ControlTablesStruct(C.Structure):
    """struct cmtts_control_tables (include/cmtts_hip.h): fp32 [B, ld] device pointers as void*."""
    _fields_ = [("d", C.c_void_p), ("e", C.c_void_p), ("p", C.c_void_p), ("ld", C.c_int)]


class DurationTargetsStruct(C.Structure):
    """struct cmtts_duration_targets (include/cmtts_hip.h): int32 device pointers as void*."""
    _fields_ = [("seg", C.c_void_p), ("target", C.c_void_p), ("unmet", C.c_void_p), ("ld", C.c_int), ("n_seg", C.c_int)]


class SampleGroupStruct(C.Structure):
    """struct cmtts_sample_group (include/cmtts_hip.h)."""
    _fields_ = [("noise", C.c_void_p), ("cond_ct", C.c_void_p), ("speaker_emb", C.c_void_p), ("B", C.c_int32), ("T", C.c_int32),
                ("active_frames", C.c_void_p), ("mel", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t),
                ("cond_p1", C.c_void_p), ("p1_ld", C.c_int32), ("L", C.c_int32), ("mel2ph", C.c_void_p), ("p_idx", C.c_void_p)]


class StepPlanStruct(C.Structure):
    """struct cmtts_step_plan (include/cmtts_hip.h): HOST arrays as void*."""
    _fields_ = [("max_steps", C.c_int32), ("n_steps", C.c_void_p), ("sigmas", C.c_void_p), ("renoise_std", C.c_void_p)]


class NoiseGroupStruct(C.Structure):
    """struct cmtts_noise_group (include/cmtts_hip.h)."""
    _fields_ = [("seeds", C.c_void_p), ("B", C.c_int32), ("T", C.c_int32), ("out", C.c_void_p)]


_vp, _i, _f, _sz, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64

# name -> (restype, argtypes); must list every symbol include/cmtts_hip.h declares
SIGNATURES = {
    "cmtts_last_error": (C.c_char_p, []),
    "cmtts_version": (C.c_char_p, []),
    "cmtts_abi_version": (_i, []),
    "cmtts_create": (_i, [C.POINTER(CMTTSConfigStruct), C.POINTER(_vp)]),
    "cmtts_set_tensor": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i]),
    "cmtts_finalize": (_i, [_vp]),
    "cmtts_destroy": (None, [_vp]),
    "cmtts_text_workspace_bytes": (_sz, [_vp, _i, _i]),
    "cmtts_text_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_text_forward_ragged": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_set_variance_controls": (_i, [_vp, C.POINTER(VarianceControlsStruct)]),
    "cmtts_set_control_tables": (_i, [_vp, C.POINTER(ControlTablesStruct)]),
    "cmtts_set_duration_targets": (_i, [_vp, C.POINTER(DurationTargetsStruct)]),
    "cmtts_phoneme_marks": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "cmtts_frame_workspace_bytes": (_sz, [_vp, _i, _i]),
    "cmtts_frame_forward": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_frame_forward_sub": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_frame_forward_sub_t": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_text_state_record_bytes": (_sz, [_vp, _i]),
    "cmtts_text_state_pack": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "cmtts_text_state_unpack": (_i, [_vp, _vp, _i, _i, _vp, _sz, _vp]),
    "cmtts_length_regulate": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "cmtts_denoiser_workspace_bytes": (_sz, [_vp, _i, _i]),
    "cmtts_denoiser_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "cmtts_schedule": (_i, [_vp, _i, C.POINTER(_f), C.POINTER(_f)]),
    "cmtts_sample": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _vp, _sz, _vp]),
    "cmtts_sample_factored": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _vp, _sz, _vp, _vp, _i, _i, _vp, _vp]),
    "cmtts_sample_factored_t": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _vp, _sz, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "cmtts_noise_fill": (_i, [_vp, _i, _i, _i, _i, _i, _i64, _vp, _vp]),
    "cmtts_noise_fill_groups": (_i, [C.POINTER(NoiseGroupStruct), _i, _i, _i, _i, _vp]),
    "cmtts_sample_seeded_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "cmtts_sample_seeded": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _vp, _sz, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "cmtts_sample_mixed_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "cmtts_sample_mixed": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, C.POINTER(StepPlanStruct), _vp, _vp, _sz, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "cmtts_retake_workspace_bytes": (_sz, [_vp, _i, _i]),
    "cmtts_retake": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, C.POINTER(_f), C.POINTER(_f), _vp, _vp, _sz, _vp]),
    "cmtts_sample_ragged": (_i, [_vp, C.POINTER(SampleGroupStruct), _i, _i, C.POINTER(_f), C.POINTER(_f), _i, _vp]),
    "cmtts_vocoder_create": (_i, [C.POINTER(_vp)]),
    "cmtts_vocoder_set_tensor": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i]),
    "cmtts_vocoder_finalize": (_i, [_vp]),
    "cmtts_vocoder_destroy": (None, [_vp]),
    "cmtts_vocoder_workspace_bytes": (_sz, [_vp, _i, _i]),
    "cmtts_vocoder_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "cmtts_wav_to_int16": (_i, [_vp, _vp, _i64, _f, _vp]),
    "cmtts_vocoder_halo_frames": (_i, [_vp]),
    "cmtts_vocoder_windows_workspace_bytes": (_sz, [_vp, _i, _i]),
    "cmtts_vocoder_forward_windows": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _f, _vp, _sz, _vp]),
    "cmtts_resampler_create": (_i, [_i, _i, _vp, _i, C.POINTER(_vp)]),
    "cmtts_resampler_destroy": (None, [_vp]),
    "cmtts_resampler_half_width": (_i, [_vp]),
    "cmtts_resample_encode": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _f, _vp, _i64, _vp]),
    "cmtts_vocoder_forward_windows_f32": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cmtts_loudness_coefficients": (_i, [_i, C.POINTER(C.c_double)]),
    "cmtts_loudness_workspace_bytes": (_i64, [_i, _i64, _i]),
    "cmtts_loudness_measure": (_i, [_vp, _i, _i64, _vp, _i, _vp, _f, _vp, _vp, _sz, _vp]),
    "cmtts_resample_encode_gain": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _f, _vp, _i64, _vp, _vp]),
    "cmtts_spkenc_create": (_i, [C.POINTER(_vp)]),
    "cmtts_spkenc_set_tensor": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i]),
    "cmtts_spkenc_finalize": (_i, [_vp]),
    "cmtts_spkenc_destroy": (None, [_vp]),
    "cmtts_spkenc_workspace_bytes": (_sz, [_i, _i64, _i]),
    "cmtts_spkenc_features": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cmtts_spkenc_forward": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "cmtts_ge2e_create": (_i, [C.POINTER(_vp)]),
    "cmtts_ge2e_set_tensor": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i]),
    "cmtts_ge2e_finalize": (_i, [_vp]),
    "cmtts_ge2e_destroy": (None, [_vp]),
    "cmtts_ge2e_workspace_bytes": (_sz, [_i, _i]),
    "cmtts_ge2e_features": (_i, [_vp, _vp, _i, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "cmtts_ge2e_forward": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "cmtts_mel_basis": (_i, [_i, _i, _i, C.c_double, C.c_double, _vp]),
    "cmtts_analysis_create": (_i, [_i, _i, _i, _i, _i, C.c_double, C.c_double, C.POINTER(_vp)]),
    "cmtts_analysis_destroy": (None, [_vp]),
    "cmtts_analysis_workspace_bytes": (_sz, [_i, _i]),
    "cmtts_mel_analysis": (_i, [_vp, _vp, _i, _i, _i64, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_phoneme_energy": (_i, [_vp, _i, _i, _vp, _i, C.c_double, C.c_double, _vp, _vp]),
    "cmtts_pcm_crossfade": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "cmtts_align_workspace_bytes": (_sz, [_i, _i, _i]),
    "cmtts_align_cost": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cmtts_align_dtw": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_align_durations": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_pitch_tables": (_i, [_i, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "cmtts_pitch_create": (_i, [_i, _i, C.c_double, C.c_double, C.POINTER(_vp)]),
    "cmtts_pitch_destroy": (None, [_vp]),
    "cmtts_pitch_workspace_bytes": (_sz, [_i, _i]),
    "cmtts_pitch_nacf": (_i, [_vp, _vp, _i, _i, _i64, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_pitch_track": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_pitch_targets": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_metric_dct_table": (_i, [_i, _i, _vp]),
    "cmtts_metric_workspace_bytes": (_sz, [_i, _i, _i]),
    "cmtts_metric_cepstra": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "cmtts_metric_cost": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cmtts_metric_diagonal": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "cmtts_metric_f0": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "cmtts_metric_ssim_prepare": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "cmtts_metric_ssim": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_profile_begin": (_i, [_i, _i]),
    "cmtts_set_fused_resblock": (_i, [_i]),
    "cmtts_set_persistent_denoiser": (_i, [_i]),
    "cmtts_poll_error": (_i, []),
    "cmtts_set_option": (_i, [C.c_char_p, _i]),
    "cmtts_model_set_option": (_i, [_vp, C.c_char_p, _i]),
    "cmtts_vocoder_set_option": (_i, [_vp, C.c_char_p, _i]),
    "cmtts_set_resblock_tile": (_i, [_i]),
    "cmtts_set_precision": (_i, [_vp, _i]),
    "cmtts_vocoder_set_precision": (_i, [_vp, _i]),
    "cmtts_set_debug_stamps": (_i, [_vp]),
    "cmtts_profile_end": (_i, [C.POINTER(C.c_double), C.POINTER(_i)]),
    "cmtts_decoder_workspace_bytes": (_sz, [_vp, _i, _i]),
    "cmtts_decoder_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "cmtts_length_mask": (_i, [_vp, _vp, _i, _i, _vp]),
    "cmtts_comm_unique_id": (_i, [_vp]),
    "cmtts_comm_init_rank": (_i, [C.POINTER(_vp), _i, _i, _vp]),
    "cmtts_comm_destroy": (_i, [_vp]),
    "cmtts_allgather_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "cmtts_allgather_mels": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_allgather_pcm_workspace_bytes": (_sz, [_i, _i, _i64]),
    "cmtts_allgather_pcm": (_i, [_vp, _i, _vp, _vp, _i, _i64, _vp, _vp, _vp, _sz, _vp]),
    "cmtts_exchange_records": (_i, [_vp, _i, _vp, C.POINTER(_i64), _vp, C.POINTER(_i64), _sz, _vp]),
    "cmtts_transpose": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "cmtts_pack_conv_weight": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_i)]),
    "cmtts_free_device": (None, [_vp]),
    "cmtts_conv1d": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
}

ABI_VERSION = 8         # include/cmtts_hip.h: CMTTS_ABI_VERSION
_lib = None
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "cmtts_hip.h")


def cdef_from_header(path=HEADER_PATH):
    """The header as cffi.FFI.cdef() takes it: comments, preprocessor lines and the extern "C" wrapper removed."""
    import re
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lines = [ln for ln in text.splitlines() if not ln.lstrip().startswith("#")]
    text = "\n".join(lines)
    text = text.replace('extern "C" {', "")
    text = re.sub(r"^\}\s*$", "", text, flags=re.M)          # the closing brace of extern "C" (struct bodies end in "} name;")
    return text


def address_of(arg):
    """Integer address of whatever the call sites pass for a pointer parameter: None, an int, a ctypes pointer value
    (c_void_p, cast), byref(obj), a ctypes array / structure, or an object with data_ptr()."""
    if arg is None:
        return 0
    if isinstance(arg, int):
        return arg
    if isinstance(arg, C.c_void_p):
        return arg.value or 0
    if hasattr(arg, "_obj"):                       # byref(x)
        return C.addressof(arg._obj)
    if isinstance(arg, (C.Array, C.Structure)):
        return C.addressof(arg)
    if isinstance(arg, C._Pointer):
        return C.cast(arg, C.c_void_p).value or 0
    if hasattr(arg, "data_ptr"):
        return int(arg.data_ptr())
    raise TypeError(f"cannot take the address of {type(arg).__name__}")


class _CffiLib:
    """libcmtts_hip.so through cffi (ABI mode: ffi.dlopen, no compiler), callable exactly like the ctypes object: pointer
    parameters accept what address_of() understands, `const char*` parameters take bytes, `const char*` results come back
    as bytes."""

    def __init__(self, path):
        import cffi
        self.ffi = cffi.FFI()
        self.ffi.cdef(cdef_from_header())
        self._c = self.ffi.dlopen(path)
        for name, (res, args) in SIGNATURES.items():
            setattr(self, name, self._wrap(name, res, args))

    def _wrap(self, name, res, args):
        ffi, fn = self.ffi, getattr(self._c, name)          # AttributeError if the .so lacks the symbol
        ctypes_ = ffi.typeof(fn).args
        assert len(ctypes_) == len(args), name

        def call(*a):
            conv = []
            for v, ct, at in zip(a, ctypes_, args):
                if at is C.c_char_p:
                    conv.append(ffi.NULL if v is None else v)
                elif ct.kind == "pointer":
                    conv.append(ffi.cast(ct, address_of(v)))
                else:
                    conv.append(v.value if hasattr(v, "value") else v)
            r = fn(*conv)
            if res is C.c_char_p:
                return None if r == ffi.NULL else ffi.string(r)
            return None if res is None else int(r)
        call.__name__ = name
        return call


def _load_ctypes():
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks the symbol
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """dlopen libcmtts_hip.so and bind every entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C cm-tts_amd/csrc). "
            "cmtts_amd has no CPU or PyTorch fallback.")
    # PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64 and must bring them in FIRST: the library then binds to
    # that HIP runtime (same SONAME) and shares torch's device context and streams.  Loaded the other way round, the
    # process ends up with /opt/rocm's runtime under torch and "no ROCm-capable device is detected".
    import torch  # noqa: F401
    # ctypes is the default binding: it is the one every test in this image exercises.  The cffi ABI-mode binding is opt-in
    # (CMTTS_FFI=cffi) until a CI leg with cffi installed has run tests/test_cabi.py and a GPU smoke through it.
    want = os.environ.get("CMTTS_FFI", "ctypes")
    if want == "cffi":
        import cffi  # noqa: F401  (ImportError: the caller asked for a binding this environment does not have)
        lib = _CffiLib(LIB_PATH)
    elif want == "ctypes":
        lib = _load_ctypes()
    else:
        raise RuntimeError(f"CMTTS_FFI={want!r}: expected 'ctypes' or 'cffi'")
    got = lib.cmtts_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} implements ABI revision {got}, this binding was written for {ABI_VERSION} "
                           "(include/cmtts_hip.h: CMTTS_ABI_VERSION): rebuild the library")
    _lib = lib
    # measurement hook (tools/, A/B runs of bench.py): CMTTS_INTERNAL="persist_wino=1,voc_wino=0" flips csrc/internal_hooks.h switches at load.
    # These switches change numerics, so a stray variable must not reach a production process: it is honoured only together with
    # CMTTS_INTERNAL_ENABLE=1, every entry is validated, an unknown name is an error, and what was applied is logged.
    spec = os.environ.get("CMTTS_INTERNAL", "")
    if spec:
        if os.environ.get("CMTTS_INTERNAL_ENABLE") != "1":
            print(f"cmtts_amd: ignoring CMTTS_INTERNAL={spec!r} (measurement hook: set CMTTS_INTERNAL_ENABLE=1 to apply it)", file=sys.stderr)
        else:
            for kv in filter(None, (e.strip() for e in spec.split(","))):
                k, sep, v = kv.partition("=")
                try:
                    val = int(v)
                except ValueError:
                    val = None
                if not sep or not k.strip() or val is None:
                    raise RuntimeError(f"CMTTS_INTERNAL: malformed entry {kv!r} (expected name=integer[,name=integer...])")
                if internal_set(k.strip(), val) < 0:
                    raise RuntimeError(f"CMTTS_INTERNAL: unknown switch {k.strip()!r} (csrc/internal_hooks.h)")
                print(f"cmtts_amd: CMTTS_INTERNAL applied {k.strip()}={val}", file=sys.stderr)
    return lib


_internal = None


def internal_set(name, value):
    """csrc/internal_hooks.h: flip one of the A/B switches between a fused kernel and the path it replaces (bitwise equal
    pairs; tests/ and tools/ only — not part of the C ABI, hence bound here and not in SIGNATURES).  Returns the previous value."""
    global _internal
    load()
    if _internal is None:
        _internal = C.CDLL(LIB_PATH).cmtts_internal_set
        _internal.restype, _internal.argtypes = _i, [C.c_char_p, _i]
    return _internal(name if isinstance(name, bytes) else name.encode(), int(value))


_noise_bits = None


def internal_noise_bits(seeds, B, T, M, first_draw, n_draws, t0, bits, stream):
    """csrc/internal_hooks.h: cmtts_internal_noise_bits — the raw Philox blocks of the seeded noise (tests only; pointers as
    integers or c_void_p).  Returns the status."""
    global _noise_bits
    load()
    if _noise_bits is None:
        _noise_bits = C.CDLL(LIB_PATH).cmtts_internal_noise_bits
        _noise_bits.restype, _noise_bits.argtypes = _i, [_vp, _i, _i, _i, _i, _i, _i64, _vp, _vp]
    return _noise_bits(seeds, int(B), int(T), int(M), int(first_draw), int(n_draws), int(t0), bits, stream)


_retake_step = None


def internal_retake_step(x0, known, regen, seeds, windows, N, Tw, M, T, draw, scale, mode, out, stream):
    """csrc/internal_hooks.h: cmtts_internal_retake_step — the masked sampler's step kernel alone on the caller's device buffers (tests
    only; pointers as integers, c_void_p or None).  Returns the status."""
    global _retake_step
    load()
    if _retake_step is None:
        _retake_step = C.CDLL(LIB_PATH).cmtts_internal_retake_step
        _retake_step.restype, _retake_step.argtypes = _i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp, _vp]
    return _retake_step(x0, known, regen, seeds, windows, int(N), int(Tw), int(M), int(T), int(draw), float(scale), int(mode), out, stream)


_sample_rows = None


def internal_sample_rows():
    """csrc/internal_hooks.h: cmtts_internal_sample_rows — the utterance-evaluations launched by the last sampler call (tests only)."""
    global _sample_rows
    load()
    if _sample_rows is None:
        _sample_rows = C.CDLL(LIB_PATH).cmtts_internal_sample_rows
        _sample_rows.restype, _sample_rows.argtypes = C.c_long, []
    return int(_sample_rows())


_duration_fit = None


def internal_duration_fit(d_rounded, cum, mel_len, src_lens, seg, target, unmet, B, L, n_seg, stream):
    """csrc/internal_hooks.h: cmtts_internal_duration_fit — the fit kernel alone on the caller's device buffers (tools/ and tests only;
    pointers as integers or None).  Returns the status."""
    global _duration_fit
    load()
    if _duration_fit is None:
        _duration_fit = C.CDLL(LIB_PATH).cmtts_internal_duration_fit
        _duration_fit.restype, _duration_fit.argtypes = _i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]
    return _duration_fit(d_rounded, cum, mel_len, src_lens, seg, target, unmet, int(B), int(L), int(n_seg), stream)


_eval_scalings = None


def internal_eval_scalings(sigma, sigma_min, sigma_data):
    """csrc/internal_hooks.h: cmtts_internal_eval_scalings — the sampler's fp32 scalings of one evaluation, computed on the host (tests only; no
    GPU).  Returns a float32 array (c_in, c_out, c_skip, 250 log(sigma))."""
    global _eval_scalings
    import numpy as np
    load()
    if _eval_scalings is None:
        _eval_scalings = C.CDLL(LIB_PATH).cmtts_internal_eval_scalings
        _eval_scalings.restype, _eval_scalings.argtypes = None, [C.c_float, C.c_float, C.c_float, _vp]
    out = np.empty(4, np.float32)
    _eval_scalings(float(sigma), float(sigma_min), float(sigma_data), out.ctypes.data)
    return out


_pack_weights = None


def internal_pack_weights(layout, kmajor, mode=0):
    """csrc/internal_hooks.h: cmtts_internal_pack_weights — one of the host-side weight packers (csrc/weight_pack.h) on a float32 numpy array
    kmajor [taps][K][M] (tests only; host memory, no GPU).  Returns the packed stream as a uint8 array, or None for an unknown layout or a
    shape the packer does not cover."""
    global _pack_weights
    import numpy as np
    load()
    if _pack_weights is None:
        _pack_weights = C.CDLL(LIB_PATH).cmtts_internal_pack_weights
        _pack_weights.restype, _pack_weights.argtypes = _i, [C.c_char_p, _vp, _i, _i, _i, _i, _vp, _sz, C.POINTER(_sz)]
    w = np.ascontiguousarray(kmajor, np.float32)
    taps, K, M = w.shape
    need = _sz(0)
    if _pack_weights(layout.encode(), w.ctypes.data, taps, K, M, int(mode), None, 0, C.byref(need)) != 0:
        return None
    out = np.empty(need.value, np.uint8)
    if _pack_weights(layout.encode(), w.ctypes.data, taps, K, M, int(mode), out.ctypes.data, out.nbytes, C.byref(need)) != 0:
        return None
    return out


_spk_hooks = None


def _spk():
    global _spk_hooks
    load()
    if _spk_hooks is None:
        lib = C.CDLL(LIB_PATH)
        pack, conv, fbank = lib.cmtts_internal_spkenc_pack, lib.cmtts_internal_spkenc_conv, lib.cmtts_internal_spkenc_fbank
        pack.restype, pack.argtypes = _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, C.POINTER(_sz)]
        conv.restype, conv.argtypes = _i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]
        fbank.restype, fbank.argtypes = _i, [_vp, _i, _i64, _i, _i, _i, _vp, _i, _vp, _vp, _vp]
        _spk_hooks = (pack, conv, fbank)
    return _spk_hooks


def internal_spkenc_pack(kernel, bias=None, bn=None):
    """csrc/internal_hooks.h: cmtts_internal_spkenc_pack — the speaker encoder's Conv2D packer with its BatchNorm fold on a Keras kernel
    (kh, kw, cin, cout), bias [cout] or None, bn [4, cout] (gamma, beta, moving mean, moving variance) or None (tests only; host memory, no
    GPU).  Returns (fragment stream, folded bias) as float32 arrays."""
    import numpy as np
    pack = _spk()[0]
    k = np.ascontiguousarray(kernel, np.float32)
    kh, kw, cin, cout = k.shape
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    n = None if bn is None else np.ascontiguousarray(bn, np.float32)
    need = _sz(0)
    if pack(k.ctypes.data, kh * kw, cin, cout, None, None, None, 0, None, C.byref(need)) != 0:
        raise ValueError("cmtts_internal_spkenc_pack: shape not covered")
    frag, bout = np.empty(need.value, np.float32), np.empty(cout, np.float32)
    rc = pack(k.ctypes.data, kh * kw, cin, cout, None if b is None else b.ctypes.data, None if n is None else n.ctypes.data, frag.ctypes.data,
              frag.size, bout.ctypes.data, C.byref(need))
    if rc != 0:
        raise ValueError("cmtts_internal_spkenc_pack failed")
    return frag, bout


def internal_spkenc_conv(x, frag, bias, res, B, H, W, cin, cout, ks, stride, y, stream):
    """csrc/internal_hooks.h: cmtts_internal_spkenc_conv — the speaker encoder's Conv2D kernel alone on the caller's device buffers (tests and
    tools only; pointers as integers, c_void_p or None).  Returns the status."""
    return _spk()[1](x, frag, bias, res, int(B), int(H), int(W), int(cin), int(cout), int(ks), int(stride), y, stream)


def internal_spkenc_fbank(wav, rows, ld, fs, win_length, mode, offsets, max_windows, windows, info, stream):
    """csrc/internal_hooks.h: cmtts_internal_spkenc_fbank — the fbank kernel alone on kept spans the caller wrote into info (tests only)."""
    return _spk()[2](wav, int(rows), int(ld), int(fs), int(win_length), int(mode), offsets, int(max_windows), windows, info, stream)


_ge2e_hooks = None


def _ge2e():
    global _ge2e_hooks
    load()
    if _ge2e_hooks is None:
        lib = C.CDLL(LIB_PATH)
        mel, layer, tail = lib.cmtts_internal_ge2e_mel, lib.cmtts_internal_ge2e_layer, lib.cmtts_internal_ge2e_tail
        basis = lib.cmtts_internal_ge2e_mel_basis
        mel.restype, mel.argtypes = _i, [_vp, _i, _i64, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]
        layer.restype, layer.argtypes = _i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]
        tail.restype, tail.argtypes = _i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]
        basis.restype, basis.argtypes = _i, [_vp]
        _ge2e_hooks = (mel, layer, tail, basis)
    return _ge2e_hooks


def internal_ge2e_mel(wav, rows, ld, n_valid, mode, max_windows, T, windows, win_lens, info, stream):
    """csrc/internal_hooks.h: cmtts_internal_ge2e_mel — the GE2E front end alone (tests and tools only; pointers as integers or None)."""
    return _ge2e()[0](wav, int(rows), int(ld), n_valid, int(mode), int(max_windows), int(T), windows, win_lens, info, stream)


def internal_ge2e_layer(x, N, T, K, wih, whh, bias, lens, tile, pre, hseq, hlast, stream):
    """csrc/internal_hooks.h: cmtts_internal_ge2e_layer — one LSTM layer (projection GEMM + recurrence) on the caller's device buffers."""
    return _ge2e()[1](x, int(N), int(T), int(K), wih, whh, bias, lens, int(tile), pre, hseq, hlast, stream)


def internal_ge2e_tail(hlast, W, lin_t, lin_b, emb_w, row_map, rows, emb, stream):
    """csrc/internal_hooks.h: cmtts_internal_ge2e_tail — Linear + ReLU + norm per window and the row means on the caller's device buffers."""
    return _ge2e()[2](hlast, int(W), lin_t, lin_b, emb_w, row_map, int(rows), emb, stream)


def internal_ge2e_mel_basis():
    """csrc/internal_hooks.h: cmtts_internal_ge2e_mel_basis — csrc/mel_basis.cpp at n_fft = 551: float32 [40, 276] (host only)."""
    import numpy as np
    out = np.empty((40, 276), np.float32)
    if _ge2e()[3](out.ctypes.data) != 0:
        raise ValueError("cmtts_internal_ge2e_mel_basis failed")
    return out


def ge2e_pack_lstm(w, bias_ih=None, bias_hh=None):
    """The lstm_fragments stream (csrc/weight_pack.h: to_lstm_fragments) of a torch LSTM matrix [1024, K] as a float32 array, and — with the two
    biases — their sum in packed row order (tests and tools only; host memory)."""
    import numpy as np
    from . import ge2e
    w = np.asarray(w, np.float32)
    raw = internal_pack_weights("lstm_fragments", np.ascontiguousarray(w.T)[None])
    if raw is None:
        raise ValueError("lstm_fragments: shape not covered")
    frag = raw.view(np.float32)
    if bias_ih is None:
        return frag
    b = (np.asarray(bias_ih, np.float32) + np.asarray(bias_hh, np.float32))[ge2e.packed_row(np.arange(1024))]
    return frag, np.ascontiguousarray(b, np.float32)


def backend():
    """"cffi" or "ctypes": which binding load() picked."""
    return "cffi" if isinstance(load(), _CffiLib) else "ctypes"


def check(rc):
    if rc != 0:
        msg = load().cmtts_last_error()
        raise RuntimeError(f"libcmtts_hip error {rc}: {msg.decode() if msg else '?'}")
