"""CPU: the host side of in-flight batching (tts_ar_session_*): the exported symbols, the allocator's first-fit rule, and the behaviour of every session
call on a host-only context (no device: nothing may crash, nothing may pretend to work)."""
import ctypes as C

import numpy as np
import pytest

SYMBOLS = ["tts_ar_session_open", "tts_ar_session_admit", "tts_ar_session_room", "tts_ar_session_step", "tts_ar_session_finished", "tts_ar_session_collect",
           "tts_ar_session_logits", "tts_ar_session_cancel", "tts_ar_session_close", "tts_ar_session_recaptures", "tts_host_session_first_fit"]
ERR_ARG, ERR_HIP, ERR_STATE = -1, -4, -5


def test_the_eleven_symbols_are_exported_declared_and_bound(pkg):
    L = pkg.lib()
    declared = set(pkg.header_symbols())
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert getattr(L, name).argtypes is not None, name
    for m in ("open", "admit", "room", "step", "finished", "collect", "logits", "cancel", "close", "recaptures"):
        assert callable(getattr(pkg.Engine, "ar_session_" + m)), m


def first_fit(busy, n):
    for i in range(len(busy) - n + 1):
        if not any(busy[i:i + n]):
            return i
    return -1


def test_first_fit_against_the_python_loop(pkg):
    rs = np.random.RandomState(5)
    for _ in range(400):
        n_slots = int(rs.randint(1, 41))
        busy = (rs.rand(n_slots) < rs.choice([0.1, 0.4, 0.7])).astype(np.uint8)
        n = int(rs.randint(1, n_slots + 1))
        assert pkg.host_session_first_fit(busy, n) == first_fit(list(busy), n), (list(busy), n)


def test_first_fit_edges(pkg):
    ff = pkg.host_session_first_fit
    assert ff(np.zeros(20, np.uint8), 20) == 0              # n_cand = n_slots, all free
    assert ff(np.array([0] * 19 + [1], np.uint8), 20) == -1  # n_cand = n_slots, one taken
    assert ff(np.ones(20, np.uint8), 1) == -1               # a full map
    assert ff(np.array([1, 0, 0, 1, 1, 0, 0, 0], np.uint8), 3) == 5   # a run that ends at the last slot
    assert ff(np.array([1, 0, 0, 1, 1, 0, 0, 0], np.uint8), 4) == -1
    assert ff(np.array([0, 1, 0, 0, 1, 0, 0], np.uint8), 2) == 2      # the LOWEST run, not the best fit
    assert ff(np.array([7, 0, 255], np.uint8), 1) == 1                # any nonzero byte is taken
    L = pkg.lib()
    assert L.tts_host_session_first_fit(None, 4, 1) == -1
    one = np.zeros(4, np.uint8)
    assert L.tts_host_session_first_fit(one.ctypes.data_as(C.c_void_p), 0, 1) == -1
    assert L.tts_host_session_first_fit(one.ctypes.data_as(C.c_void_p), 4, 0) == -1
    assert L.tts_host_session_first_fit(one.ctypes.data_as(C.c_void_p), 4, 5) == -1


def _calls(L, h):
    tok = np.array([255, 14, 0], np.int32)
    voice = np.zeros(1024, np.float32)
    codes, rows, steps, stopped = np.zeros(502, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    logits, ids = np.zeros(8194, np.float32), np.zeros(4, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return {
        "open": lambda: L.tts_ar_session_open(h, 4, 2, 16, 8, 3),
        "admit": lambda: L.tts_ar_session_admit(h, p(tok), 3, p(voice), 1, 7, None),
        "room": lambda: L.tts_ar_session_room(h),
        "step": lambda: L.tts_ar_session_step(h),
        "finished": lambda: L.tts_ar_session_finished(h, p(ids), 4),
        "collect": lambda: L.tts_ar_session_collect(h, 0, p(codes), p(rows), None, p(steps), p(stopped)),
        "logits": lambda: L.tts_ar_session_logits(h, 0, p(logits)),
        "cancel": lambda: L.tts_ar_session_cancel(h, 0),
        "close": lambda: L.tts_ar_session_close(h),
        "recaptures": lambda: L.tts_ar_session_recaptures(h),
    }


def test_host_only_context_refuses_every_session_call(pkg):
    eng = pkg.Engine(-1)
    try:
        for _ in range(2):  # a refused call leaves nothing behind: the second round answers the same
            for name, call in _calls(eng.L, eng.h).items():
                assert call() in (ERR_HIP, ERR_STATE), name
        assert b"host-only" in eng.L.tts_last_error(eng.h)
        with pytest.raises(pkg.TtsError):
            eng.ar_session_open(4, 2, 16, 8)
        # the host-only stages still work afterwards
        eng.seed(3)
        assert 0.0 <= eng.rng_uniform() < 1.0
    finally:
        eng.close()


def test_null_context_is_a_bad_argument(pkg):
    for name, call in _calls(pkg.lib(), None).items():
        assert call() == ERR_ARG, name
