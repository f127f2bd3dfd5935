"""CPU: the host side of session audio (tts_ar_session_enable_audio / tts_ar_session_audio): the two symbols are exported, declared and bound, a host-only
context refuses both with TTS_ERR_HIP, and the additions leave the API version at 8."""
import ctypes as C

import numpy as np

SYMBOLS = ["tts_ar_session_enable_audio", "tts_ar_session_audio"]
ERR_ARG, ERR_HIP = -1, -4


def test_the_two_symbols_are_exported_declared_and_bound(pkg):
    L = pkg.lib()
    declared = set(pkg.header_symbols())
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert getattr(L, name).argtypes is not None, name
    for m in ("enable_audio", "audio"):
        assert callable(getattr(pkg.Engine, "ar_session_" + m)), m


def test_host_only_context_refuses_both(pkg):
    eng = pkg.Engine(-1)
    try:
        buf, last = np.zeros(256, np.float32), np.zeros(1, np.int32)
        for _ in range(2):
            assert eng.L.tts_ar_session_enable_audio(eng.h, 8) == ERR_HIP
            assert b"host-only" in eng.L.tts_last_error(eng.h)
            assert eng.L.tts_ar_session_audio(eng.h, 0, buf.ctypes.data_as(C.c_void_p), 256, last.ctypes.data_as(C.c_void_p)) == ERR_HIP
        assert eng.L.tts_ar_session_enable_audio(None, 8) == ERR_ARG
        assert eng.L.tts_ar_session_audio(None, 0, None, 0, None) == ERR_ARG
    finally:
        eng.close()


def test_the_api_version_is_still_8(pkg):
    assert pkg.lib().tts_version() == 8
