"""CPU: per-request sampler controls and step limit of a session (tts_ar_request, tts_ar_request_init, tts_ar_session_admit_ex, TTS_AR_ROW_CONTROLS): the
symbols, the descriptor's checks through the host probe (the very predicate tts_set_option applies to each control), the calls on a host-only and on a null
context, and the sharpness of the control sets tests/test_ar_session_controls_gpu.py admits: on the known logits of that test every set must change the
sampled sequence, or the GPU test would pass with the controls silently ignored."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

V = 8194
OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_LIMIT = 0, -1, -4, -5, -6
SYMBOLS = ["tts_ar_request_init", "tts_ar_session_admit_ex", "tts_host_ar_request_check"]
OPTION_OF = dict(temperature="ar_temperature", top_k="ar_top_k", top_p="ar_top_p", penalty="ar_repetition_penalty", scope="ar_penalty_scope")

# ---- the control sets of the GPU test (shared with it) ----
SESSION = dict(temperature=0.9, top_k=50, top_p=0.8, penalty=2.0, scope=0)    # what the session pins: NOT the context defaults (temperature 0.8)
CONTROLS_B = dict(temperature=1.3, top_k=5, top_p=0.5, penalty=1.2, scope=0)
CONTROLS_C = dict(scope=1, penalty=3.0, top_k=100)                            # the largest top-k the lists serve: pf_min 114
CONTROLS_D = dict(scope=1, top_k=200)                                         # above TTS_PF_TOPK_MAX: the full-row path
HOT_FIXED = [1, 31, 32, 33, 8191, 8192, 8193]


def full(controls):
    """A control dict with the missing keys taken from the session's set, as ar_session_admit(controls=...) does."""
    return dict(SESSION, **controls)


def crafted_bias():
    """The bias of the `crafted` fixture of tests/test_sampler_controls_gpu.py: 60 hot ids from U(4, 6), the rest N(0, 1); (bias, hot)."""
    rs = np.random.RandomState(31)
    bias = rs.randn(V)
    hot = np.unique(np.concatenate([HOT_FIXED, rs.randint(2, 8190, 53)]))
    bias[hot] = rs.uniform(4, 6, len(hot))
    return bias.astype(np.float32), hot


def literal_sequence(pkg, row, uniforms, controls):
    """The codes of one candidate whose every logits row is `row`: the literal formulation (tts_host_sample_row_ex mode 1) over `uniforms`. Iteration 0 is
    penalised with the prompt-shaped ids {1, 8192}; afterwards scope 0 penalises the id fed last, scope 1 every id fed so far plus 1 and 8192."""
    c = full(controls)
    kw = dict(temperature=c["temperature"], top_k=c["top_k"], top_p=c["top_p"], penalty=c["penalty"])
    hist, out = [1, 8192], []
    for i, u in enumerate(uniforms):
        ids = hist if (i == 0 or c["scope"] == 1) else [out[-1]]
        out.append(pkg.host_sample_row_ex(row, ids, u, mode=1, **kw))
        hist.append(out[-1])
    return np.array(out, np.int32)


def test_the_symbols_are_exported_declared_and_bound(pkg):
    L = pkg.lib()
    declared = set(pkg.header_symbols())
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
        assert getattr(L, name).argtypes is not None, name
    hdr = open(pkg.HEADER).read()
    assert "typedef struct tts_ar_request" in hdr and "TTS_AR_ROW_CONTROLS" in hdr
    assert pkg.AR_ROW_CONTROLS not in (pkg.AR_MASK_STOP, pkg.AR_RETIRE) and pkg.AR_ROW_CONTROLS & (pkg.AR_MASK_STOP | pkg.AR_RETIRE) == 0
    assert "TTS_AR_ROW_CONTROLS = %d" % pkg.AR_ROW_CONTROLS in hdr
    assert callable(pkg.Engine.ar_request) and callable(pkg.host_ar_request_check)
    import inspect
    assert "row_controls" in inspect.signature(pkg.Engine.ar_session_open).parameters
    assert {"controls", "max_steps"} <= set(inspect.signature(pkg.Engine.ar_session_admit).parameters)


def test_header_with_the_descriptor_is_plain_c_and_the_layouts_agree(pkg, tmp_path):
    """The header compiles as C99 (-pedantic -Werror); the struct's size and offsets as C sees them are the ctypes binding's; the host probe is reachable from C."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "req.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include <stdint.h>
#include "tortoise_mi355x.h"
int main(void) {
  tts_ar_request r;
  r.struct_size = (uint32_t)sizeof r; r.n_cand = 2; r.seed = 5u; r.max_steps = 0; r.stop_at = NULL;
  r.temperature = 0.8; r.top_k = 50; r.top_p = 0.8; r.repetition_penalty = 2.0; r.penalty_scope = 0;
  printf("%d %d %d %d %d %d\n", (int)sizeof r, (int)offsetof(tts_ar_request, n_cand), (int)offsetof(tts_ar_request, stop_at), (int)offsetof(tts_ar_request, temperature),
         (int)offsetof(tts_ar_request, penalty_scope), (int)TTS_AR_ROW_CONTROLS);
  printf("%d ", tts_host_ar_request_check(&r, 4, 8));
  r.top_k = 2.5;
  printf("%d ", tts_host_ar_request_check(&r, 4, 8));
  r.top_k = 50; r.n_cand = 5;
  printf("%d\n", tts_host_ar_request_check(&r, 4, 8));
  return 0;
}
''')
    exe = tmp_path / "req"
    inc = os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "include")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-ltortoise_mi355x",
                    "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    R = pkg.ArRequest
    assert [int(x) for x in out[0].split()] == [C.sizeof(R), R.n_cand.offset, R.stop_at.offset, R.temperature.offset, R.penalty_scope.offset, pkg.AR_ROW_CONTROLS]
    assert [int(x) for x in out[1].split()] == [OK, ERR_ARG, ERR_LIMIT]


BAD = [("temperature", 0.0), ("temperature", -0.5), ("temperature", float("nan")), ("temperature", float("inf")), ("top_k", 0), ("top_k", 8195), ("top_k", 2.5),
       ("top_p", 0.0), ("top_p", 1.0000001), ("penalty", 0.999), ("scope", 2)]
EDGE = [("temperature", 1e-30), ("temperature", 3e38), ("top_k", 1), ("top_k", 8194), ("top_p", 1e-30), ("top_p", 1.0), ("penalty", 1.0), ("penalty", 3e38),
        ("scope", 0), ("scope", 1)]


def test_descriptor_checks_are_those_of_set_option(pkg):
    """Every control value: the host probe answers TTS_OK exactly where tts_set_option accepts the value under the option's key, and TTS_ERR_ARG where it refuses."""
    check = pkg.host_ar_request_check
    assert check(4, 8) == OK
    eng = pkg.Engine(-1)
    try:
        for key, value in BAD + EDGE:
            accepted = eng.L.tts_set_option(eng.h, OPTION_OF[key].encode(), float(value)) == OK
            assert accepted == ((key, value) in EDGE), (key, value)
            assert check(4, 8, **{key: value}) == (OK if accepted else ERR_ARG), (key, value)
        # a grid beyond the listed values: the two must never disagree
        rs = np.random.RandomState(3)
        grid = {"temperature": [-1, 0, 1e-46, 1e-45, 0.5, 1e39, -np.inf], "top_k": [-3, 0.5, 1, 7, 100, 101, 8194, 8194.5, 1e9, np.nan],
                "top_p": [-0.1, 0, 1e-46, 0.2, 1, 1.5, np.nan], "penalty": [0, 0.5, 1, 1.0000001, 1e39, np.inf, np.nan], "scope": [-1, 0, 0.5, 1, 2, np.nan]}
        for key, values in grid.items():
            for value in list(values) + list(rs.uniform(-2, 3, 8)):
                accepted = eng.L.tts_set_option(eng.h, OPTION_OF[key].encode(), float(value)) == OK
                assert check(4, 8, **{key: value}) == (OK if accepted else ERR_ARG), (key, value)
    finally:
        eng.close()


def test_descriptor_checks_of_the_other_fields(pkg):
    check = pkg.host_ar_request_check
    assert check(4, 8, req_max_steps=-1) == ERR_ARG
    assert check(4, 8, req_max_steps=9) == ERR_LIMIT
    for ms in (0, 1, 8):
        assert check(4, 8, req_max_steps=ms) == OK, ms
    assert check(4, 8, n_cand=5) == ERR_LIMIT
    assert check(4, 8, n_cand=4) == OK
    assert check(4, 8, n_cand=0) == ERR_ARG
    size = C.sizeof(pkg.ArRequest)
    assert check(4, 8, struct_size=size - 1) == ERR_ARG and check(4, 8, struct_size=0) == ERR_ARG
    assert check(4, 8, struct_size=size) == OK and check(4, 8, struct_size=size + 64) == OK   # a caller built against a longer, later struct
    L = pkg.lib()
    assert L.tts_host_ar_request_check(None, 4, 8) == ERR_ARG
    req = pkg.ArRequest(size, 1, 0, 0, None, 0.8, 50, 0.8, 2.0, 0)
    assert L.tts_host_ar_request_check(C.byref(req), 0, 8) == ERR_ARG and L.tts_host_ar_request_check(C.byref(req), 4, 0) == ERR_ARG
    stop = np.array([3, 0], np.int32)   # a candidate that would stop before its first code: tts_ar_session_admit's rule
    req = pkg.ArRequest(size, 2, 0, 0, stop.ctypes.data, 0.8, 50, 0.8, 2.0, 0)
    assert L.tts_host_ar_request_check(C.byref(req), 4, 8) == ERR_ARG


def _calls(pkg, L, h):
    tok = np.array([255, 14, 0], np.int32)
    voice = np.zeros(1024, np.float32)
    req = pkg.ArRequest(C.sizeof(pkg.ArRequest), 1, 7, 0, None, 0.8, 50, 0.8, 2.0, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return {"open_rows": lambda: L.tts_ar_session_open(h, 4, 2, 16, 8, 3 | pkg.AR_ROW_CONTROLS), "request_init": lambda: L.tts_ar_request_init(h, C.byref(req)),
            "admit_ex": lambda: L.tts_ar_session_admit_ex(h, p(tok), 3, p(voice), C.byref(req))}


def test_host_only_context_refuses_and_null_context_is_a_bad_argument(pkg):
    eng = pkg.Engine(-1)
    try:
        for _ in range(2):
            for name, call in _calls(pkg, eng.L, eng.h).items():
                assert call() == ERR_HIP, name
        assert b"host-only" in eng.L.tts_last_error(eng.h)
        with pytest.raises(pkg.TtsError):
            eng.ar_request()
    finally:
        eng.close()
    for name, call in _calls(pkg, pkg.lib(), None).items():
        assert call() == ERR_ARG, name


N_UNIFORMS = 24   # the GPU test's session steps


def test_the_gpu_tests_control_sets_are_sharp(pkg):
    """On the crafted row (every logits row of the GPU test's literal comparison) and over the same uniforms, each non-default control set gives another
    sequence than the session's set: a request whose controls were ignored could not pass the GPU test by coincidence. Each single control of B is sharp as
    well where the others are the session's, and so is the session's temperature against the context default."""
    bias, hot = crafted_bias()
    assert len(hot) == 60
    row = bias.copy()
    row[8193] = -1e30
    rs = np.random.RandomState(77)
    sets = dict(B=CONTROLS_B, C=CONTROLS_C, D=CONTROLS_D, default_temperature=dict(temperature=0.8))
    sets.update({"B_" + k: {k: v} for k, v in CONTROLS_B.items() if v != SESSION[k]})
    sets.update(C_scope=dict(scope=1), C_penalty_under_scope1=dict(scope=1, penalty=3.0))
    differs = {name: 0 for name in sets}
    n_streams = 4
    for _ in range(n_streams):
        u = rs.uniform(0, 1, N_UNIFORMS).astype(np.float32)
        base = literal_sequence(pkg, row, u, SESSION)
        assert (base >= 0).all()
        for name, c in sets.items():
            seq = literal_sequence(pkg, row, u, c)
            assert (seq >= 0).all(), name
            differs[name] += int((seq != base).any())
    # the sets the GPU test admits: in every stream; one control of a set alone: in at least one
    assert all(differs[name] == n_streams for name in ("B", "C", "D", "default_temperature")), differs
    assert all(n >= 1 for n in differs.values()), differs
    u = rs.uniform(0, 1, N_UNIFORMS).astype(np.float32)
    assert (literal_sequence(pkg, row, u, CONTROLS_C) != literal_sequence(pkg, row, u, CONTROLS_D)).any()
