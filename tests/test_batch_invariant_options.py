"""CPU checks of the batch-invariance switches (no compute calls): cmtts_model_set_option / cmtts_vocoder_set_option "batch_invariant"
take 0 or 1 and refuse anything else, the process-wide table does not know them, and the ABI revision says they exist."""
import ctypes as C
import os

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from cmtts_amd.config import get_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_revision_8():
    lib = _lib.load()
    assert lib.cmtts_abi_version() == 8 and _lib.ABI_VERSION == 8


def test_model_option_values():
    from cmtts_amd import host
    model = host.CMTotalTTS(get_config("VCTK"), "cpu")          # cmtts_create only: options live on the handle
    assert model.set_option("batch_invariant", 1) == 0          # default 0
    lib = model.lib
    for bad in (2, -1, 7):
        assert lib.cmtts_model_set_option(model._h, b"batch_invariant", bad) == 1     # refused: the previous value comes back, unchanged
    assert model.set_option("batch_invariant", 0) == 1
    assert model.set_option("batch_invariant", 0) == 0
    # a per-model option, not a process-wide one (tests/test_cabi.py pins that table)
    assert lib.cmtts_set_option(b"batch_invariant", 1) == -1


def test_vocoder_option_values():
    lib = _lib.load()
    v = C.c_void_p()
    assert lib.cmtts_vocoder_create(C.byref(v)) == 0
    try:
        assert lib.cmtts_vocoder_set_option(v, b"batch_invariant", 1) == 0
        for bad in (2, -1):
            assert lib.cmtts_vocoder_set_option(v, b"batch_invariant", bad) == 1
        assert lib.cmtts_vocoder_set_option(v, b"batch_invariant", 0) == 1
        assert lib.cmtts_vocoder_set_option(v, b"batch_invariant", 0) == 0
    finally:
        lib.cmtts_vocoder_destroy(v)


def test_options_documented():
    text = open(os.path.join(ROOT, "include", "cmtts_hip.h")).read()
    assert 'cmtts_model_set_option(m, "batch_invariant"' in text and 'cmtts_vocoder_set_option(v, "batch_invariant"' in text
