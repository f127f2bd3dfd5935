"""GPU: session audio (tts_ar_session_enable_audio / tts_ar_session_audio). Every one-candidate request of an audio session streams HiFi-GAN audio while the
batch decodes. The contract is the session's and the stream's at once: codes, rows, steps and stop status are those of the request run alone
(tts_seed + tts_ar_set_stop_schedule + tts_autoregressive); the latents that collect returns are that run's bit for bit (31 rows or more: the incremental
latent pass runs the multi-row kernels, as the lone pass does); the concatenated audio is bit for bit tts_hifigan_decode of those latents; and none of it
depends on the stride, the slot or the rest of the batch.

The only tolerance is the short utterance's (fewer than 31 rows: the lone run ends on the exact-f32 GEMV pass, which sums in another order): rel_err < 1e-4,
the bound tests/test_hifigan_stream_gpu.py::test_stream_latents_of_a_short_utterance holds the stream to.

Shapes: 2 GPT-2 layers (small_models). 8 slots; prompts of 9, 60 and 131 ids (1 + 131 prompt rows + the mel rows: the visible keys cross the 128-key LDS
chunk of the attention kernel while the request decodes); 200-code requests under stride 96 for passes of more than 128 packed rows (two GEMM row blocks)
and more than 64 rows per item (several attention blocks per item, items at different n_past)."""
import ctypes as C

import numpy as np
import pytest

from test_ar_session_gpu import other_voice, prompt
from test_hifigan_cpu import hifigan_model  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -5


def req(n_text, n_cand, seed, stop_at, at=0, voice_k=0):
    return dict(tokens=prompt(n_text, 300 + seed), n_cand=n_cand, seed=seed, stop_at=stop_at, at=at, voice_k=voice_k)


def voice_of(r, voice):
    return other_voice(voice, r["voice_k"]) if r["voice_k"] else voice


@pytest.fixture(scope="module")
def eng(pkg, small_models, hifigan_model):
    e = pkg.Engine(0)
    e.load(ar=small_models + "/ggml-model.bin")
    e.load_hifigan(hifigan_model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lone(eng, voice):
    """(codes, rows, latents, steps, stopped) of a request run alone, once per request and flag set"""
    memo = {}

    def run(r, max_steps, retire=True):
        key = (r["tokens"].tobytes(), r["n_cand"], r["seed"], tuple(r["stop_at"] or ()), r["voice_k"], max_steps, retire)
        if key not in memo:
            eng.set_stop_schedule(r["stop_at"])
            try:
                eng.seed(r["seed"])
                codes, rows, lats, steps = eng.autoregressive(r["tokens"], voice_of(r, voice), r["n_cand"], max_steps, mask_stop=True, retire=retire)
                memo[key] = (codes, rows, lats, steps, eng.ar_stop_status(r["n_cand"]))
            finally:
                eng.set_stop_schedule(None)
        return memo[key]
    return run


def run_session(eng, pkg, reqs, voice, stride, shape, retire=True, cancel=None, after=None):
    """Admits reqs[k] once `at` steps have run, drains every one-candidate request after every step, collects a request in the step that reports it finished.
    cancel = (k, step): request k is cancelled once `step` steps have run. after: requests admitted one by one once everything before them has been
    collected (slot reuse). Returns {k: dict(got = collect's tuple, drains = [(samples, is_last, still running)], audio)}."""
    eng.ar_session_open(*shape, mask_stop=True, retire=retire)
    eng.ar_session_enable_audio(stride)
    out, rid_of, cancelled = {}, {}, {}
    pending = sorted(range(len(reqs)), key=lambda k: reqs[k]["at"])
    later = list(after or [])
    drains = {k: [] for k in range(len(reqs) + len(later))}
    all_reqs = list(reqs) + later
    step = 0

    def drain(k, running):
        a, last = eng.ar_session_audio(rid_of[k])
        assert len(a) % 256 == 0, (k, len(a))
        drains[k].append((a, last, running))

    try:
        while pending or rid_of or later:
            assert step < 400
            if not pending and not rid_of:
                all_k = len(all_reqs) - len(later)
                r = later.pop(0)
                rid_of[all_k] = eng.ar_session_admit(r["tokens"], voice_of(r, voice), r["n_cand"], r["seed"], r["stop_at"])
            while pending and reqs[pending[0]]["at"] <= step:
                k = pending.pop(0)
                r = reqs[k]
                rid_of[k] = eng.ar_session_admit(r["tokens"], voice_of(r, voice), r["n_cand"], r["seed"], r["stop_at"])
            if cancel and cancel[1] == step and cancel[0] in rid_of:
                k = cancel[0]
                eng.ar_session_cancel(rid_of[k])
                cancelled[k] = rid_of.pop(k)
            eng.ar_session_step()
            step += 1
            finished = eng.ar_session_finished()
            for k in sorted(rid_of):
                r = all_reqs[k]
                done = rid_of[k] in finished
                if r["n_cand"] == 1:
                    drain(k, not done)
                elif step == 1 or done:  # several candidates are re-ranked: admitted and run as before, without audio
                    with pytest.raises(pkg.TtsError, match=r"cannot stream\) \(status -1\)"):
                        eng.ar_session_audio(rid_of[k])
                if done:
                    out[k] = dict(got=eng.ar_session_collect(rid_of[k]), step=step)
                    del rid_of[k]
        recaptures = eng.ar_session_recaptures()
        for k, rid in cancelled.items():
            with pytest.raises(pkg.TtsError, match=r"no request %d \(status -1\)" % rid):
                eng.ar_session_audio(rid)
    finally:
        eng.ar_session_close()
    for k in out:
        out[k]["drains"] = drains[k]
        out[k]["audio"] = np.concatenate([d[0] for d in drains[k]]) if drains[k] else None
    return out, recaptures


def assert_request(eng, res, ref, r, voice, what, exact_latents=True):
    (c, rows, l, s, st), (ca, ra, la, sa, sta) = res["got"], ref
    assert (c == ca).all(), (what, "codes")
    assert (rows == ra).all() and s == sa and (st == sta).all(), (what, rows, ra, s, sa, st, sta)
    assert len(l) == len(la) and all(a.shape == b.shape for a, b in zip(l, la)), what
    if exact_latents:
        for b in range(len(la)):
            assert l[b].tobytes() == la[b].tobytes(), (what, "latents", b, float(np.abs(l[b] - la[b]).max()))
    if r["n_cand"] == 1:
        want = eng.hifigan_decode([l[0]], voice_of(r, voice))[0]
        assert res["audio"].tobytes() == want.tobytes(), (what, "audio", len(res["audio"]), len(want))
        assert [d[1] for d in res["drains"]] == [False] * (len(res["drains"]) - 1) + [True], (what, "is_last")


SHAPE = (8, 2, 131, 80)
STAGGERED = [
    req(9, 1, 41, [34]),
    req(60, 1, 42, [45], at=3, voice_k=1),
    req(131, 1, 43, [70], at=7, voice_k=2),
    req(16, 2, 44, None),
]


@pytest.fixture(scope="module")
def staggered(eng, pkg, voice, tmp_path_factory):
    """the staggered session at a stride, once per stride: (results, recaptures, the context's RNG state before, after)"""
    memo = {}

    def run(stride):
        if stride not in memo:
            d = tmp_path_factory.mktemp("rng%d" % stride)
            eng.seed(999)
            eng.rng_save_state(str(d / "a.txt"))
            out, recaptures = run_session(eng, pkg, STAGGERED, voice, stride, SHAPE)
            eng.rng_save_state(str(d / "b.txt"))
            memo[stride] = (out, recaptures, (d / "a.txt").read_text(), (d / "b.txt").read_text())
        return memo[stride]
    return run


def test_staggered_session(eng, pkg, voice, lone, staggered):
    out, recaptures, rng0, rng1 = staggered(8)
    assert sorted(out) == [0, 1, 2, 3]
    for k, r in enumerate(STAGGERED):
        assert_request(eng, out[k], lone(r, SHAPE[3]), r, voice, k)
    assert all(int(out[k]["got"][1][0]) >= 31 for k in range(3))
    assert any(len(a) > 0 and running for a, _, running in out[2]["drains"]), "the 70-code request delivered nothing while it was running"
    print("frames per drain:", {k: [len(d[0]) // 256 for d in out[k]["drains"] if len(d[0])] for k in range(3)})
    assert recaptures == 0
    assert rng0 == rng1


def test_stride_independence(staggered):
    runs = {stride: staggered(stride)[0] for stride in (1, 8, 64)}
    for k in range(3):
        for stride in (1, 64):
            assert runs[stride][k]["audio"].tobytes() == runs[8][k]["audio"].tobytes(), (k, stride, "audio")
            assert runs[stride][k]["got"][2][0].tobytes() == runs[8][k]["got"][2][0].tobytes(), (k, stride, "latents")
            assert runs[stride][k]["step"] == runs[8][k]["step"]
    for k in (0, 1):  # finished before the clock's first tick at 64: everything arrives on the finishing step
        filled = [i for i, d in enumerate(runs[64][k]["drains"]) if len(d[0])]
        assert filled == [len(runs[64][k]["drains"]) - 1], (k, filled)
    # the 70-code request: the shorter the stride, the more often it delivers
    assert sum(len(d[0]) > 0 for d in runs[1][2]["drains"]) > sum(len(d[0]) > 0 for d in runs[8][2]["drains"]) > sum(len(d[0]) > 0 for d in runs[64][2]["drains"])


def test_tile_boundaries(eng, pkg, voice, lone):
    reqs = [req(16, 1, 51, None), req(41, 1, 52, None, at=5, voice_k=1)]
    out, recaptures = run_session(eng, pkg, reqs, voice, 96, (2, 1, 41, 200), retire=False)
    for k, r in enumerate(reqs):
        assert int(out[k]["got"][1][0]) > 200
        assert_request(eng, out[k], lone(r, 200, retire=False), r, voice, k)
    assert recaptures == 0


def test_short_utterance(eng, pkg, voice, lone):
    r = req(16, 1, 61, None)
    out, _ = run_session(eng, pkg, [r], voice, 6, (2, 1, 16, 12), retire=False)
    ref = lone(r, 12, retire=False)
    rows = int(ref[1][0])
    assert rows < 31
    assert_request(eng, out[0], ref, r, voice, "short", exact_latents=False)
    rel = np.abs(out[0]["got"][2][0] - ref[2][0]).max() / np.abs(ref[2][0]).max()
    print("short utterance (%d rows, drains of %s frames): rel_err %.2e" % (rows, [len(d[0]) // 256 for d in out[0]["drains"]], rel))
    assert rel < 1e-4


def test_slot_reuse(eng, pkg, voice, lone):
    first, second = req(60, 1, 71, [44]), req(9, 1, 72, [33], voice_k=2)
    out, _ = run_session(eng, pkg, [first], voice, 8, (1, 1, 60, 50), after=[second])  # one slot: the second request can only take the first one's
    assert_request(eng, out[0], lone(first, 50), first, voice, "first")
    assert_request(eng, out[1], lone(second, 50), second, voice, "second, in the slot the first one left")


def test_cancel_mid_stream(eng, pkg, voice, lone):
    reqs = [req(16, 1, 81, [40]), req(41, 1, 82, [60], voice_k=1), req(9, 1, 83, [36], at=2)]
    out, _ = run_session(eng, pkg, reqs, voice, 4, (4, 1, 41, 64), cancel=(1, 30))
    assert sorted(out) == [0, 2]
    for k in (0, 2):
        assert_request(eng, out[k], lone(reqs[k], 64), reqs[k], voice, k)


def test_statuses(pkg, eng, voice, small_models):
    L, h = eng.L, eng.h
    last = np.zeros(1, np.int32)
    buf = np.zeros(256, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    err = lambda e: e.L.tts_last_error(e.h).decode()  # noqa: E731
    assert L.tts_ar_session_enable_audio(h, 8) == ERR_STATE and "tts_ar_session_open not called" in err(eng)
    assert L.tts_ar_session_audio(h, 0, p(buf), 256, p(last)) == ERR_STATE and "tts_ar_session_open not called" in err(eng)
    eng.ar_session_open(4, 2, 16, 8, mask_stop=True, retire=True)
    try:
        assert L.tts_ar_session_audio(h, 0, p(buf), 256, p(last)) == ERR_STATE and "tts_ar_session_enable_audio not called" in err(eng)
        assert L.tts_ar_session_enable_audio(h, 0) == ERR_ARG and L.tts_ar_session_enable_audio(h, -3) == ERR_ARG
        rid = eng.ar_session_admit(prompt(9, 1), voice, 1, 1, [3])
        assert L.tts_ar_session_enable_audio(h, 8) == ERR_STATE and "admitted" in err(eng)
        assert L.tts_ar_session_audio(h, rid, p(buf), 256, p(last)) == ERR_STATE  # the session has no audio: the request is served as before
        while eng.ar_session_step():
            pass
        eng.ar_session_collect(rid)
    finally:
        eng.ar_session_close()
    eng.ar_session_open(4, 2, 16, 8, mask_stop=True, retire=True)
    try:
        eng.ar_session_enable_audio(2)
        eng.ar_session_enable_audio(3)  # before the first admit: the later call holds
        rid = eng.ar_session_admit(prompt(9, 1), voice, 1, 1, [3])
        two = eng.ar_session_admit(prompt(9, 2), voice, 2, 2, [3, 3])
        assert L.tts_ar_session_audio(h, 7, p(buf), 256, p(last)) == ERR_ARG and "no request 7" in err(eng)
        assert L.tts_ar_session_audio(h, two, p(buf), 256, p(last)) == ERR_ARG and "cannot stream" in err(eng)
        assert L.tts_ar_session_audio(h, rid, p(buf), -1, p(last)) == ERR_ARG
        assert L.tts_ar_session_audio(h, rid, None, 256, p(last)) == ERR_ARG
        assert L.tts_ar_session_audio(h, rid, p(buf), 256, None) == ERR_ARG
        assert L.tts_ar_session_audio(h, rid, None, 0, p(last)) == 0 and last[0] == 0  # nothing asked for, nothing drained
        while eng.ar_session_step():
            pass
        assert L.tts_ar_session_audio(h, rid, p(buf), 255, p(last)) == 0 and last[0] == 0  # less than a frame of room: the audio waits
        total = 0
        while not last[0]:
            n = L.tts_ar_session_audio(h, rid, p(buf), 256, p(last))
            assert n == 256
            total += n
        codes, rows, lats, steps, stopped = eng.ar_session_collect(rid)
        assert total == 256 * eng.frames(int(rows[0]))
        assert L.tts_ar_session_audio(h, rid, p(buf), 256, p(last)) == ERR_ARG and "no request" in err(eng)  # collected
        eng.ar_session_cancel(two)
    finally:
        eng.ar_session_close()
    # refusals of the context's state
    bare = pkg.Engine(0)
    try:
        bare.load(ar=small_models + "/ggml-model.bin")
        bare.ar_session_open(4, 2, 16, 8)
        assert bare.L.tts_ar_session_enable_audio(bare.h, 8) == ERR_STATE and "tts_load_hifigan not called" in err(bare)
        bare.ar_session_close()
    finally:
        bare.close()
    eng.set_option("ggml_lut", 1)
    try:
        eng.ar_session_open(4, 2, 16, 8)
        eng.set_option("ggml_lut", 0)  # the session pinned the option when it was opened
        assert L.tts_ar_session_enable_audio(h, 8) == ERR_STATE and "ggml_lut" in err(eng)
    finally:
        eng.set_option("ggml_lut", 0)
        eng.ar_session_close()
