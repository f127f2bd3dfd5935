"""No GPU: the diffusion session's surface (tts_diff_session_*): header and exports, the packed-row probe against a restatement of Layout::build's rule, the
request descriptor's checks and their agreement with tts_set_option, the struct_size rule, and a host-only context."""
import ctypes as C

import numpy as np
import pytest

OK, ERR_ARG, ERR_HIP, ERR_STATE, ERR_LIMIT = 0, -1, -4, -5, -6
NEW = ["tts_diff_request_init", "tts_diff_session_open", "tts_diff_session_admit", "tts_diff_session_room", "tts_diff_session_step",
       "tts_diff_session_finished", "tts_diff_session_collect", "tts_diff_session_cancel", "tts_diff_session_close", "tts_diff_session_captures",
       "tts_host_diff_packed_rows", "tts_host_diff_request_check"]


def test_header_declares_and_library_exports(pkg):
    declared = pkg.header_symbols()
    L = pkg.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
    assert "typedef struct tts_diff_request" in open(pkg.HEADER).read()


def test_version_stays_8(pkg):
    assert pkg.lib().tts_version() == 8


def frames(L):
    return L * 4 * 24000 // 22050


def packed_rows(rows):
    """Layout::build's rule restated: sequences start on multiples of 8 from row 8, a guard row follows each, the total is padded to 128; a request brings its
    conditioned sequences and one unconditioned copy of each."""
    r = 8
    for L in list(rows) + list(rows):
        r = (r + frames(L) + 1 + 7) // 8 * 8
    return (r + 127) // 128 * 128


# rows 2 -> T = 8 (T % 8 == 0), rows 9 / 11 -> T = 39 / 47 (T % 8 == 7), rows 1, the shapes of the GPU tests, a pair that crosses 128 rows only together, the longest
ROW_LISTS = [[1], [2], [9], [11], [2, 9], [43, 17], [61], [30], [12], [14], [13, 13], [210], [500], [500] * 16, [1] * 7, [1] * 8]


@pytest.mark.parametrize("rows", ROW_LISTS, ids=lambda r: "x".join(map(str, r[:4])) + ("" if len(r) <= 4 else "_n%d" % len(r)))
def test_packed_rows_probe(pkg, rows):
    assert frames(2) % 8 == 0 and frames(9) % 8 == 7 and frames(11) % 8 == 7 and frames(1) == 4
    assert pkg.host_diff_packed_rows(rows) == packed_rows(rows)


def test_packed_rows_probe_refuses(pkg):
    L = pkg.lib()
    assert L.tts_host_diff_packed_rows(None, 1) == ERR_ARG
    for bad in ([0], [501], [5, -1]):
        a = np.array(bad, np.int32)
        assert L.tts_host_diff_packed_rows(a.ctypes.data_as(C.c_void_p), len(a)) == ERR_ARG
    a = np.array([5], np.int32)
    assert L.tts_host_diff_packed_rows(a.ctypes.data_as(C.c_void_p), 0) == ERR_ARG


def check(pkg, max_rows=4096, **kw):
    return pkg.host_diff_request_check(max_rows, **kw)


def test_request_check_accepts_and_refuses(pkg):
    lat = np.random.RandomState(0).randn(5, 1024).astype(np.float32)
    assert check(pkg, latents=[lat]) == OK
    assert check(pkg, latents=[lat, lat[:2]], n_steps=2, sampler=1, ddim_eta=1.0, cond_free_k=0.0, voice=np.zeros(2048, np.float32)) == OK
    # null pointers
    assert pkg.lib().tts_host_diff_request_check(None, 4096) == ERR_ARG
    assert check(pkg, latents=[lat], null_latents=True) == ERR_ARG
    assert check(pkg, latents=[lat], null_rows=True) == ERR_ARG
    # n_cand, rows, n_steps
    assert check(pkg, latents=[lat], n_cand=0) == ERR_ARG
    assert check(pkg, latents=[lat], rows=[0]) == ERR_ARG
    assert check(pkg, latents=[lat], rows=[501]) == ERR_ARG
    assert check(pkg, latents=[lat], n_steps=1) == ERR_ARG
    # non-finite values
    bad = lat.copy()
    bad[3, 7] = np.nan
    assert check(pkg, latents=[bad]) == ERR_ARG
    bad[3, 7] = np.inf
    assert check(pkg, latents=[lat, bad]) == ERR_ARG
    v = np.zeros(2048, np.float32)
    v[2047] = -np.inf
    assert check(pkg, latents=[lat], voice=v) == ERR_ARG
    # room: the probe's own count decides
    need = pkg.host_diff_packed_rows([5])
    assert check(pkg, max_rows=need, latents=[lat]) == OK
    assert check(pkg, max_rows=need - 1, latents=[lat]) == ERR_LIMIT
    assert pkg.lib().tts_host_diff_request_check(C.byref(pkg.DiffRequest()), 0) == ERR_ARG


CONTROL_VALUES = {"diff_sampler": [0, 1, 2, -1, 0.5, float("nan")], "ddim_eta": [0, 0.5, 1, 1.0001, -1e-9, float("nan"), float("inf")],
                  "cond_free_k": [0, 1, 2, 7.5, -0.1, float("nan"), float("inf"), 1e39]}


@pytest.mark.parametrize("key", sorted(CONTROL_VALUES))
def test_controls_agree_with_set_option(pkg, key):
    """One predicate: a request's control is accepted exactly when tts_set_option accepts the value (sampler is an int32 field: integral values only)."""
    L = pkg.lib()
    h = L.tts_create(-1)
    lat = np.zeros((3, 1024), np.float32)
    field = {"diff_sampler": "sampler", "ddim_eta": "ddim_eta", "cond_free_k": "cond_free_k"}[key]
    try:
        for v in CONTROL_VALUES[key]:
            if key == "diff_sampler" and (v != v or v != int(v)):
                continue
            want = L.tts_set_option(h, key.encode(), float(v))
            assert want in (OK, ERR_ARG)
            assert check(pkg, latents=[lat], **{field: v}) == want, (key, v)
    finally:
        L.tts_destroy(h)


def test_struct_size_rule(pkg):
    lat = np.zeros((3, 1024), np.float32)
    size = C.sizeof(pkg.DiffRequest)
    assert check(pkg, latents=[lat], struct_size=size) == OK
    assert check(pkg, latents=[lat], struct_size=size + 16) == OK  # a caller whose header declares a longer struct: this version reads its own fields
    assert check(pkg, latents=[lat], struct_size=size - 1) == ERR_ARG
    assert check(pkg, latents=[lat], struct_size=0) == ERR_ARG


def test_host_only_context_refuses_every_session_call(pkg):
    L = pkg.lib()
    h = L.tts_create(-1)
    try:
        req = pkg.DiffRequest()
        req.struct_size = C.sizeof(pkg.DiffRequest)
        ids = np.zeros(4, np.int32)
        mel = np.zeros(400, np.float32)
        vp = C.c_void_p
        assert L.tts_diff_session_open(h, 1024, 4) == ERR_HIP
        assert L.tts_diff_request_init(h, C.byref(req)) == ERR_HIP
        assert L.tts_diff_session_admit(h, C.byref(req)) == ERR_HIP
        assert L.tts_diff_session_room(h) == ERR_HIP
        assert L.tts_diff_session_step(h) == ERR_HIP
        assert L.tts_diff_session_finished(h, ids.ctypes.data_as(vp), 4) == ERR_HIP
        assert L.tts_diff_session_collect(h, 0, mel.ctypes.data_as(vp)) == ERR_HIP
        assert L.tts_diff_session_cancel(h, 0) == ERR_HIP
        assert L.tts_diff_session_captures(h) == ERR_HIP
        assert L.tts_diff_session_close(h) == ERR_HIP
    finally:
        L.tts_destroy(h)
