"""GPU: in-flight batching of the autoregressive stage (tts_ar_session_*). Requests join a running batch at any step and leave at any step; the contract is
that of every batching feature here: each request's bits are those of that request run alone (tts_seed + tts_ar_set_stop_schedule + tts_autoregressive).
Nothing below has a tolerance: every comparison is bit for bit against the single-request path, which this feature does not change.

Shapes: 20 slots = two tiles of 16 rows, the second partly empty; one request of 16 candidates sits in slots 3 .. 18 and straddles the tile boundary; prompts of
9, 16, 41 and 131 ids (131 + 2 rows: a prompt pass of several 16-row tiles with a ragged last one); 24 steps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SLOTS, MAX_CAND, MAX_TEXT, S = 20, 16, 131, 24
ERR_STATE, ERR_LIMIT = -5, -6


def prompt(n, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([[255], rs.randint(1, 250, n - 2), [0]]).astype(np.int32)


def other_voice(voice, k=1):
    return np.ascontiguousarray(np.roll(voice, 17 * k)[::-1] * np.float32(0.5 + 0.25 * k))


def req(n_text, n_cand, seed, stop_at, at=0, hold=0, voice_k=0):
    return dict(tokens=prompt(n_text, 100 + seed), n_cand=n_cand, seed=seed, stop_at=list(stop_at), at=at, hold=hold, voice_k=voice_k)


def voice_of(r, voice):
    return other_voice(voice, r["voice_k"]) if r["voice_k"] else voice


def run_session(eng, reqs, voice, want_latents=True, on_step=None, flags=dict(mask_stop=True, retire=True), shape=(N_SLOTS, MAX_CAND, MAX_TEXT, S), close=True):
    """Admits reqs[k] once `at` session steps have run, collects a finished request `hold` steps after it was first reported. Returns {k: collect's tuple}."""
    eng.ar_session_open(*shape, **flags)
    out, rid_of, seen = {}, {}, {}
    pending = sorted(range(len(reqs)), key=lambda k: reqs[k]["at"])
    step = 0
    while pending or rid_of:
        assert step < 200
        for rid in eng.ar_session_finished():
            k = next(k for k, r in rid_of.items() if r == rid)
            seen.setdefault(k, step)
            if step >= seen[k] + reqs[k]["hold"]:
                out[k] = eng.ar_session_collect(rid, want_latents=want_latents)
                del rid_of[k]
        while pending and reqs[pending[0]]["at"] <= step:
            k = pending.pop(0)
            r = reqs[k]
            rid_of[k] = eng.ar_session_admit(r["tokens"], voice_of(r, voice), r["n_cand"], r["seed"], r["stop_at"])
        live = eng.ar_session_step()
        step += 1
        if on_step:
            on_step(step, rid_of, live)
    assert eng.ar_session_room() == shape[0] and eng.ar_session_finished() == []
    if close:
        eng.ar_session_close()
    return out


def alone(eng, r, voice, want_latents=True, max_steps=S):
    eng.set_stop_schedule(r["stop_at"])
    try:
        eng.seed(r["seed"])
        codes, rows, lats, steps = eng.autoregressive(r["tokens"], voice_of(r, voice), r["n_cand"], max_steps, mask_stop=True, retire=True, want_latents=want_latents)
        return codes, rows, lats, steps, eng.ar_stop_status(r["n_cand"])
    finally:
        eng.set_stop_schedule(None)


def assert_same(got, ref, what, latents=True):
    (c, r, l, s, st), (ca, ra, la, sa, sta) = got, ref
    assert (c == ca).all(), (what, "codes")
    assert (r == ra).all() and s == sa and (st == sta).all(), (what, r, ra, s, sa, st, sta)
    if latents:
        assert len(l) == len(la)
        for b in range(len(la)):
            assert l[b].shape == la[b].shape and (l[b] == la[b]).all(), (what, "latents", b)


# admitted at session steps 0, 0, 3 and 7; they end at different steps, B and D run to max_steps (a stop_at beyond it never fires)
FOUR = [
    req(9, 3, 11, [2, 4, 3]),                                                                    # slots 0 .. 2, collected before step 7
    req(131, 16, 12, [5, 9, 30, 12, 7, 30, 3, 18, 11, 30, 6, 14, 22, 8, 30, 10]),                # slots 3 .. 18: straddles the tile boundary
    req(16, 1, 13, [15], at=3),                                                                  # slot 19
    req(41, 2, 14, [6, 40], at=7, voice_k=1),                                                    # slots 0 .. 1 again, another voice
]


@pytest.mark.parametrize("mode", ["f32", "fp16", "fp8", "ggml_lut", "scope1", "host_topk"])
def test_each_request_equals_itself_alone(pkg, mid_models, voice, mode):
    eng = pkg.Engine(0)
    try:
        if mode in ("fp16", "fp8"):
            eng.set_option("ar_weights", 1 if mode == "fp16" else 2)
        if mode == "ggml_lut":
            eng.set_option("ggml_lut", 1)
        if mode == "scope1":
            eng.set_option("ar_penalty_scope", 1)
        if mode == "host_topk":
            eng.set_option("device_topk", 0)
        eng.load(ar=mid_models + "/ggml-model.bin")
        lat = mode in ("f32", "scope1")  # the latents are compared where the latent pass is the f32 one
        got = run_session(eng, FOUR, voice, want_latents=lat)
        assert sorted(got) == [0, 1, 2, 3]
        assert got[1][3] == S and got[3][3] == S and 0 in got[1][4] and 1 in got[1][4]  # B was cut at max_steps, some of its candidates stopped
        for k, r in enumerate(FOUR):
            assert_same(got[k], alone(eng, r, voice, want_latents=lat), (mode, k), latents=lat)
    finally:
        eng.close()


def test_per_step_logits_of_a_late_request(engine, mid_models, voice):
    """The request admitted at step 7: its rows of every session step's logits against tts_ar_begin + tts_ar_prefill + tts_ar_step of its prompt alone, fed the codes
    the session produced: a wrong position id or context length shows here even where the sampler would happen to agree."""
    engine.load(ar=mid_models + "/ggml-model.bin")
    d = FOUR[3]
    rows = []

    def on_step(step, rid_of, live):
        if 3 in rid_of and rid_of[3] not in engine.ar_session_finished():
            rows.append(engine.ar_session_logits(rid_of[3]))

    got = run_session(engine, FOUR, voice, want_latents=False, on_step=on_step)
    codes, steps = got[3][0], got[3][3]
    assert steps == S and len(rows) == S - 2  # S iterations: one at admission, S - 1 steps; the last step's logits finish the request
    engine.ar_begin(d["tokens"], voice_of(d, voice), d["n_cand"], S)
    engine.ar_prefill()
    for i in range(S - 2):
        fed = np.array([codes[b, 1 + i] if i <= d["stop_at"][b] else 8193 for b in range(d["n_cand"])], np.int32)
        ref = engine.ar_step(fed, i)
        assert np.isfinite(ref).all() and (rows[i] == ref).all(), (i, np.abs(rows[i] - ref).max())


def test_slot_reuse_and_parking(pkg, mid_models, voice):
    """Slot reuse: after a collect, a request with a SHORTER prompt and another voice takes the same slots. Parking: a finished request is collected only after five
    more steps and one more admission into the neighbouring slots. Penalty scope 1, so that a stale history bit would show as well as a stale K/V row."""
    eng = pkg.Engine(0)
    try:
        eng.set_option("ar_penalty_scope", 1)
        eng.load(ar=mid_models + "/ggml-model.bin")
        reqs = [
            req(41, 3, 21, [3, 2, 4]),                          # slots 0 .. 2, finished after 4 steps, collected at once
            req(16, 2, 22, [3, 5], hold=5),                     # slots 3 .. 4, finished after 5 steps, parked for 5 more
            req(131, 2, 23, [20, 30]),                          # slots 5 .. 6: keeps the session stepping
            req(9, 3, 24, [6, 30, 8], at=6, voice_k=2),         # slots 0 .. 2 again: shorter prompt, another voice
            req(16, 1, 25, [9], at=7, voice_k=1),               # slot 7
        ]
        got = run_session(eng, reqs, voice)
        for k, r in enumerate(reqs):
            assert_same(got[k], alone(eng, r, voice), k)
    finally:
        eng.close()


def test_first_fit_slots_room_and_refusal(engine, pkg, mid_models, voice):
    engine.load(ar=mid_models + "/ggml-model.bin")
    engine.ar_session_open(N_SLOTS, MAX_CAND, MAX_TEXT, S, mask_stop=True, retire=True)
    try:
        assert engine.ar_session_room() == N_SLOTS
        a = engine.ar_session_admit(prompt(9, 1), voice, 3, 1, [1, 1, 1])     # finishes with its first step
        b = engine.ar_session_admit(prompt(16, 2), voice, 16, 2, [30] * 16)
        c = engine.ar_session_admit(prompt(9, 3), voice, 1, 3, [30])
        assert (a, b, c) == (0, 1, 2) and engine.ar_session_room() == 0 and engine.ar_session_finished() == []
        assert engine.ar_session_step() == 2 and engine.ar_session_finished() == [a]
        p4 = prompt(9, 4)
        for n_cand in (1, 3):  # the map is full: a finished request keeps its slots until it is collected
            rc = engine.L.tts_ar_session_admit(engine.h, p4.ctypes.data, 9, voice.ctypes.data, n_cand, 4, None)
            assert rc == ERR_LIMIT and b"free slots" in engine.L.tts_last_error(engine.h)
            assert engine.ar_session_room() == 0 and engine.ar_session_finished() == [a]
        # argument checks: refused before any device work, nothing changes
        bad = prompt(9, 4)
        bad[3] = 256
        nan_voice = voice.copy()
        nan_voice[100] = np.nan
        for tok, v, n_cand, stop_at, status in ((bad, voice, 1, None, -1), (prompt(9, 4), nan_voice, 1, None, -1), (prompt(9, 4), voice, 0, None, -1),
                                                (prompt(9, 4), voice, 1, [0], -1), (prompt(MAX_TEXT + 1, 4), voice, 1, None, ERR_LIMIT),
                                                (prompt(9, 4), voice, MAX_CAND + 1, None, ERR_LIMIT)):
            sa = None if stop_at is None else np.array(stop_at, np.int32)
            rc = engine.L.tts_ar_session_admit(engine.h, tok.ctypes.data, len(tok), v.ctypes.data, n_cand, 4, None if sa is None else sa.ctypes.data)
            assert rc == status, (n_cand, stop_at, rc)
        with pytest.raises(pkg.TtsError, match="still running"):
            engine.ar_session_collect(b, want_latents=False)
        codes, rows, _, steps, stopped = engine.ar_session_collect(a, want_latents=False)
        assert steps == 2 and (stopped == 1).all() and (codes[:, 2] == 8193).all()
        assert engine.ar_session_room() == 3 and engine.ar_session_finished() == []
        d = engine.ar_session_admit(prompt(9, 4), voice, 3, 4, None)          # the same admit succeeds now, into slots 0 .. 2
        assert d == 3 and engine.ar_session_room() == 0
        engine.ar_session_cancel(b)
        assert engine.ar_session_room() == 16
        for args in ((0, 1, 16, 8), (4, 5, 16, 8), (4, 0, 16, 8), (4, 2, 0, 8), (4, 2, 16, 0)):
            assert engine.L.tts_ar_session_open(engine.h, *args, 3) == -1, args
        for args in ((4, 2, 405, 8), (4, 2, 16, 501), (4, 2, 405, 501), (5000, 2, 16, 8)):
            assert engine.L.tts_ar_session_open(engine.h, *args, 3) == ERR_LIMIT, args
        assert engine.L.tts_ar_session_open(engine.h, 4, 2, 16, 8, 4) == -1    # unknown flag
        assert engine.ar_session_room() == 16                                  # a refused open leaves the open session as it is
        # the largest shape the limits allow (404 + 2 + 500 + 1 = 907 of 1024 positions) opens, and replaces the open session
        assert engine.L.tts_ar_session_open(engine.h, 4, 2, 404, 500, 3) == 0
        assert engine.ar_session_room() == 4 and engine.ar_session_finished() == []
    finally:
        engine.ar_session_close()


def test_a_strict_session(engine, pkg, mid_models, voice):
    """flags 0: these weights never sample 8193, so no request can end. One that reaches max_steps fails alone (collect: TTS_ERR_LIMIT), a second one keeps running
    untouched and is cancelled."""
    engine.load(ar=mid_models + "/ggml-model.bin")
    engine.ar_session_open(8, 4, 41, 6)
    try:
        p = engine.ar_session_admit(prompt(16, 5), voice, 2, 5)
        for _ in range(3):
            assert engine.ar_session_step() == 1
        q = engine.ar_session_admit(prompt(41, 6), voice, 3, 6)
        assert engine.ar_session_step() == 2 and engine.ar_session_finished() == []
        assert engine.ar_session_step() == 1 and engine.ar_session_finished() == [p]   # p: 6 iterations, no stop token
        with pytest.raises(pkg.TtsError, match="no stop token within 6 steps"):
            engine.ar_session_collect(p)
        assert engine.ar_session_finished() == [] and engine.ar_session_room() == 3     # slots 0 .. 1 are free again, q holds 2 .. 4, 5 .. 7 were never taken
        assert engine.L.tts_ar_session_cancel(engine.h, p) == -1 and b"no request" in engine.L.tts_last_error(engine.h)
        ql = engine.ar_session_logits(q)
        assert np.isfinite(ql).all()
        assert engine.ar_session_step() == 1
        with pytest.raises(pkg.TtsError, match="still running"):
            engine.ar_session_collect(q)
        engine.ar_session_cancel(q)
        assert engine.ar_session_room() == 8 and engine.ar_session_step() == 0
    finally:
        engine.ar_session_close()


def test_no_recapture_context_rng_options_and_afterwards(engine, pkg, mid_models, voice, tmp_path):
    engine.load(ar=mid_models + "/ggml-model.bin")
    r0 = req(16, 2, 31, [5, 9])
    before = alone(engine, r0, voice)
    reqs = [req(9, 2, 32, [4, 6]), req(41, 3, 33, [3, 30, 12]), req(16, 2, 34, [7, 5], at=5)]
    engine.seed(999)
    engine.rng_save_state(str(tmp_path / "rng0.txt"))

    def on_step(step, rid_of, live):
        if step == 2:  # the session read its options when it was opened: these reach no session call
            engine.set_option("ar_top_k", 3)
            engine.set_option("ar_temperature", 3.0)
            engine.set_option("ar_penalty_scope", 1)
            engine.set_option("device_topk", 0)
            with pytest.raises(pkg.TtsError, match="a session is open"):
                engine.autoregressive(r0["tokens"], voice, 2, S, mask_stop=True, retire=True)
            with pytest.raises(pkg.TtsError, match="a session is open"):
                engine.ar_begin(r0["tokens"], voice, 2, S)

    try:
        got = run_session(engine, reqs, voice, on_step=on_step, close=False)   # three admissions, three collects
        assert engine.ar_session_recaptures() == 0
        engine.ar_session_close()
    finally:
        engine.set_option("ar_top_k", 50)
        engine.set_option("ar_temperature", 0.8)
        engine.set_option("ar_penalty_scope", 0)
        engine.set_option("device_topk", 1)
    engine.rng_save_state(str(tmp_path / "rng1.txt"))
    assert (tmp_path / "rng0.txt").read_text() == (tmp_path / "rng1.txt").read_text()
    for k, r in enumerate(reqs):
        assert_same(got[k], alone(engine, r, voice), k)
    assert_same(alone(engine, r0, voice), before, "after the session")
    with pytest.raises(pkg.TtsError, match="tts_ar_session_open not called"):
        engine.ar_session_step()
    # a second session of the same shape, one request: the first session left nothing behind
    engine.ar_session_open(N_SLOTS, MAX_CAND, MAX_TEXT, S, mask_stop=True, retire=True)
    try:
        rid = engine.ar_session_admit(reqs[0]["tokens"], voice, 2, 32, [4, 6])
        captures = []
        while engine.ar_session_step():
            captures.append(engine.ar_session_recaptures())
        assert captures and set(captures) == {0}
        assert_same(engine.ar_session_collect(rid), got[0], "second session")
    finally:
        engine.ar_session_close()
