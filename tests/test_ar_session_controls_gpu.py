"""GPU: per-request sampler controls and step limit in a session (tts_ar_session_admit_ex, TTS_AR_ROW_CONTROLS; ar.hip: sample_prefilter_rows_kernel and the
per-row control table). The contract is that of every batching feature here: each request's bits are those of the request alone, where alone means
tts_set_option of the request's five controls + tts_seed(seed) + tts_ar_set_stop_schedule + tts_autoregressive with the request's max_steps and the session's
flags. Nothing below has a tolerance: every comparison is bit for bit.

Shapes: 20 slots = two tiles of 16 rows, the second partly empty; 24 session steps. The session is opened under options that are not the context defaults
(temperature 0.9) and the context is put back to its defaults right after, so a request that took `what tts_set_option holds now` would show. The mixed
session's requests (control sets: tests/test_ar_session_controls_cpu.py, which also shows that each set changes the sampled sequence):
  A  3 candidates, the session's own controls, step 0, slots 0 .. 2; max_steps 6, so that it leaves before step 7 with the stop schedule off as well
  B  16 candidates in slots 3 .. 18, across the tile boundary, step 0: temperature 1.3, top_k 5, top_p 0.5, penalty 1.2, scope 0
  C  1 candidate, step 3, slot 19: scope 1, penalty 3.0, top_k 100 (the largest top-k the lists serve: pf_min 114)
  D  2 candidates, step 7, the slots A has left (a stale table row or history row shows here): scope 1, top_k 200 (above TTS_PF_TOPK_MAX: its rows, and only
     its rows, take the full-row path), max_steps 10 while the others run to 24, another voice"""
import numpy as np
import pytest

from test_ar_session_controls_cpu import CONTROLS_B, CONTROLS_C, CONTROLS_D, OPTION_OF, SESSION, crafted_bias, full, literal_sequence
from test_ar_session_gpu import MAX_CAND, MAX_TEXT, N_SLOTS, S, assert_same, other_voice, prompt
from test_hifigan_cpu import hifigan_model  # noqa: F401
from test_sampler_controls_gpu import crafted  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_STATE = -5
DEFAULTS = dict(temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, scope=0)


def set_controls(eng, c):
    for k, v in full(c).items():
        eng.set_option(OPTION_OF[k], v)


def req(n_text, n_cand, seed, stop_at, at=0, voice_k=0, controls=None, max_steps=None):
    return dict(tokens=prompt(n_text, 100 + seed), n_cand=n_cand, seed=seed, stop_at=list(stop_at), at=at, voice_k=voice_k, controls=controls, max_steps=max_steps)


def voice_of(r, voice):
    return other_voice(voice, r["voice_k"]) if r["voice_k"] else voice


MIXED = [
    req(9, 3, 11, [2, 4, 3], controls={}, max_steps=6),
    req(131, 16, 12, [5, 9, 30, 12, 7, 30, 3, 18, 11, 30, 6, 14, 22, 8, 30, 10], controls=CONTROLS_B),
    req(16, 1, 13, [15], at=3, controls=CONTROLS_C),
    req(41, 2, 14, [6, 40], at=7, voice_k=1, controls=CONTROLS_D, max_steps=10),
]


def admit(eng, r, voice):
    kw = {}
    if r["controls"] is not None:
        kw["controls"] = r["controls"]
    if r["max_steps"] is not None:
        kw["max_steps"] = r["max_steps"]
    return eng.ar_session_admit(r["tokens"], voice_of(r, voice), r["n_cand"], r["seed"], r["stop_at"], **kw)


def run_session(eng, reqs, voice, mask=True, rows=True, want_latents=True, on_step=None, shape=(N_SLOTS, MAX_CAND, MAX_TEXT, S), audio=0):
    """Opens a session under SESSION's controls, puts the context back to its defaults, admits reqs[k] once `at` steps have run and collects every request when
    it is first reported finished. Returns ({k: collect's tuple}, recaptures, fallbacks, {k: audio})."""
    set_controls(eng, SESSION)
    try:
        eng.ar_session_open(*shape, mask_stop=mask, retire=True, row_controls=rows)
    finally:
        set_controls(eng, DEFAULTS)
    try:
        if audio:
            eng.ar_session_enable_audio(audio)
        out, rid_of, pcm = {}, {}, {k: [] for k in range(len(reqs))}
        pending = sorted(range(len(reqs)), key=lambda k: reqs[k]["at"])
        step = 0
        while pending or rid_of:
            assert step < 100
            for rid in eng.ar_session_finished():
                k = next(k for k, r in rid_of.items() if r == rid)
                if audio:
                    a, last = eng.ar_session_audio(rid)
                    pcm[k].append(a)
                out[k] = eng.ar_session_collect(rid, want_latents=want_latents)
                del rid_of[k]
            while pending and reqs[pending[0]]["at"] <= step:
                k = pending.pop(0)
                rid_of[k] = admit(eng, reqs[k], voice)
            eng.ar_session_step()
            step += 1
            if audio:
                for k, rid in rid_of.items():
                    pcm[k].append(eng.ar_session_audio(rid)[0])
            if on_step:
                on_step(step)
        assert eng.ar_session_room() == shape[0]
        return out, eng.ar_session_recaptures(), eng.topk_fallbacks(), {k: np.concatenate(v) if v else None for k, v in pcm.items()}
    finally:
        eng.ar_session_close()


def alone(eng, r, voice, mask=True, want_latents=True, controls=None):
    """The request alone: its controls as context options, its seed, its stop schedule, tts_autoregressive with its max_steps. (collect's tuple, fallbacks)"""
    set_controls(eng, (r["controls"] or {}) if controls is None else controls)
    eng.set_stop_schedule(r["stop_at"])
    try:
        eng.seed(r["seed"])
        codes, rows, lats, steps = eng.autoregressive(r["tokens"], voice_of(r, voice), r["n_cand"], r["max_steps"] or S, mask_stop=mask, retire=True, want_latents=want_latents)
        return (codes, rows, lats, steps, eng.ar_stop_status(r["n_cand"])), eng.topk_fallbacks()
    finally:
        eng.set_stop_schedule(None)
        set_controls(eng, DEFAULTS)


def d_fallbacks(r, mask):
    """What a top_k 200 request adds to tts_ar_topk_fallbacks: every live candidate fetches its full row in every step after the prompt's. Without the mask
    no schedule applies and every candidate samples iterations 1 .. max_steps - 1. With it candidate b stops at iteration stop_at[b] and is retired, so it
    samples iterations 1 .. min(stop_at[b], max_steps - 1): D's candidate 0 (stop_at 6) six times, its candidate 1 (stop_at 40, max_steps 10) nine times."""
    limit = r["max_steps"] or S
    return sum(min(stop, limit - 1) if mask else limit - 1 for stop in r["stop_at"])


@pytest.mark.parametrize("mask", [True, False], ids=["mask_stop", "no_mask"])
@pytest.mark.parametrize("mode", ["f32", "fp16", "host_topk"])
def test_each_request_of_the_mixed_session_equals_itself_alone(pkg, mid_models, voice, mode, mask):
    eng = pkg.Engine(0)
    try:
        if mode == "fp16":
            eng.set_option("ar_weights", 1)
        if mode == "host_topk":
            eng.set_option("device_topk", 0)
        eng.load(ar=mid_models + "/ggml-model.bin")
        lat = mode == "f32"  # the latents are compared where the latent pass is the f32 one
        got, recaptures, fallbacks, _ = run_session(eng, MIXED, voice, mask=mask, want_latents=lat)
        assert sorted(got) == [0, 1, 2, 3] and recaptures == 0
        want_fb = 0
        for k, r in enumerate(MIXED):
            ref, fb = alone(eng, r, voice, mask=mask, want_latents=lat)
            assert_same(got[k], ref, (mode, mask, k), latents=lat)
            want_fb += fb
            if k == 3 and mode != "host_topk":  # D: one per candidate and step sampled from a device row (the first code comes from the prompt pass on the host)
                assert fb == d_fallbacks(r, mask), fb
            if k == 1:  # the main assertion is not vacuous: B under the session's controls is another request
                other, _ = alone(eng, r, voice, mask=mask, want_latents=False, controls=SESSION)
                assert (other[0] != ref[0]).any()
        assert got[1][3] == S and got[3][3] == 10 and got[0][3] <= 6   # B is cut at the session's max_steps, D at its own
        if not mask:  # no schedule: every request runs to its limit
            assert got[0][3] == 6 and got[2][3] == S
        assert fallbacks == want_fb, (fallbacks, want_fb)
        if mode == "host_topk":
            assert fallbacks == 0
    finally:
        eng.close()


def test_codes_are_the_literal_formulation_on_known_logits(pkg, engine, crafted, voice):  # noqa: F811
    """On the crafted head every logits row is the bias exactly: the codes of B, C and D are a Python loop over tts_host_sample_row_ex (mode 1) with the request's
    own uniforms, controls and history. The schedules never fire, so every candidate samples every step."""
    path, bias, _ = crafted
    assert (bias == crafted_bias()[0]).all()
    engine.load(ar=path)
    row = bias.copy()
    row[8193] = -1e30
    reqs = [dict(r, stop_at=[40] * r["n_cand"]) for r in MIXED]
    reqs[0]["stop_at"] = MIXED[0]["stop_at"]
    got, recaptures, _, _ = run_session(engine, reqs, voice, want_latents=False)
    assert recaptures == 0
    for k in (1, 2, 3):
        r = reqs[k]
        steps = r["max_steps"] or S
        assert got[k][3] == steps
        engine.seed(r["seed"])
        u = np.array([[(engine.rng_uniform(), engine.rng_uniform())[1] for _ in range(r["n_cand"])] for _ in range(steps)], np.float32)
        for b in range(r["n_cand"]):
            want = literal_sequence(pkg, row, u[:, b], r["controls"])
            assert (got[k][0][b, 1:1 + steps] == want).all(), (k, b, got[k][0][b, 1:1 + steps], want)


def test_uniform_then_rows_sessions_keep_their_graphs_and_options_set_mid_session_change_nothing(pkg, mid_models, voice):
    """One context: a uniform session, a rows session, then both again. Each captures its step once (the rows graph has a slot of its own, so the uniform
    session opened later finds its graph: tts_ar_session_recaptures counts from the session's first step and stays 0 through every admission), the second run of
    each returns the first run's bits, and tts_set_option of every control in the middle of a session reaches no request."""
    eng = pkg.Engine(0)
    try:
        eng.load(ar=mid_models + "/ggml-model.bin")
        uniform = [dict(r, controls=None, max_steps=None) for r in MIXED]   # the unchanged tts_ar_session_admit path

        def on_step(step):
            if step == 2:
                set_controls(eng, dict(temperature=3.0, top_k=3, top_p=0.3, penalty=1.5, scope=1))

        runs = []
        for rows, reqs in ((False, uniform), (True, MIXED), (False, uniform), (True, MIXED)):
            got, recaptures, fallbacks, _ = run_session(eng, reqs, voice, rows=rows, want_latents=False, on_step=on_step)
            assert recaptures == 0, (rows, recaptures)
            runs.append(got)
            if not rows:  # a uniform list-served session contributes what it does today: the sum of its requests' alone counts, none under top_k 50
                want_fb = sum(alone(eng, dict(r, controls=SESSION), voice, want_latents=False)[1] for r in uniform)
                assert fallbacks == want_fb == 0, (fallbacks, want_fb)
        for k in range(4):
            assert_same(runs[2][k], runs[0][k], ("uniform again", k), latents=False)
            assert_same(runs[3][k], runs[1][k], ("rows again", k), latents=False)
            ref, _ = alone(eng, dict(uniform[k], controls=SESSION), voice, want_latents=False)
            assert_same(runs[0][k], ref, ("uniform", k), latents=False)
            ref, _ = alone(eng, MIXED[k], voice, want_latents=False)
            assert_same(runs[1][k], ref, ("rows", k), latents=False)
    finally:
        eng.close()


def test_session_audio_under_row_controls(pkg, small_models, hifigan_model, voice):  # noqa: F811
    """A rows session with audio and two one-candidate requests under different controls: each one's audio is tts_hifigan_decode of its collected latents and
    its codes are those of its alone run."""
    eng = pkg.Engine(0)
    try:
        eng.load(ar=small_models + "/ggml-model.bin")
        eng.load_hifigan(hifigan_model)
        reqs = [req(16, 1, 41, [40], controls=CONTROLS_B), req(41, 1, 42, [33], at=2, voice_k=1, controls=CONTROLS_C)]
        shape = (4, 2, 41, 36)
        got, recaptures, _, pcm = run_session(eng, reqs, voice, audio=8, shape=shape)
        assert recaptures == 0
        for k, r in enumerate(reqs):
            codes, rows, lats, steps, stopped = got[k]
            assert rows[0] >= 31   # the incremental pass and the lone pass then run the same kernels: the latents are compared bit for bit as well
            want = eng.hifigan_decode([lats[0]], voice_of(r, voice))[0]
            assert pcm[k].shape == want.shape and (pcm[k] == want).all(), k
            set_controls(eng, r["controls"])
            eng.set_stop_schedule(r["stop_at"])
            try:
                eng.seed(r["seed"])
                ca, ra, la, sa = eng.autoregressive(r["tokens"], voice_of(r, voice), 1, shape[3], mask_stop=True, retire=True)
                assert_same(got[k], (ca, ra, la, sa, eng.ar_stop_status(1)), ("audio", k))
            finally:
                eng.set_stop_schedule(None)
                set_controls(eng, DEFAULTS)
    finally:
        eng.close()


def test_without_the_flag(pkg, mid_models, voice):
    """A session opened without TTS_AR_ROW_CONTROLS: differing controls are refused with TTS_ERR_STATE and the session stays usable; tts_ar_session_admit_ex with the
    session's controls is tts_ar_session_admit bit for bit; a per-request max_steps works there too."""
    eng = pkg.Engine(0)
    try:
        eng.load(ar=mid_models + "/ggml-model.bin")
        base = MIXED[3]
        reqs = [dict(base, controls=None, max_steps=None, at=0), dict(base, controls={}, max_steps=None, at=0), dict(base, controls=None, max_steps=5, at=1),
                dict(base, controls=dict(temperature=SESSION["temperature"]), max_steps=None, at=1)]
        refused = []

        def on_step(step):
            if step == 1:
                with pytest.raises(pkg.TtsError, match=r"differ from the session's.*\(status -5\)"):
                    admit(eng, dict(base, controls=dict(top_k=49)), voice)
                refused.append(eng.ar_session_room())

        got, recaptures, fallbacks, _ = run_session(eng, reqs, voice, rows=False, on_step=on_step, shape=(8, 2, MAX_TEXT, S))
        assert recaptures == 0 and refused == [4]   # the two requests of step 0 hold four of the eight slots; the refused one took none
        assert_same(got[1], got[0], "admit_ex with the session's controls")
        assert_same(got[3], got[0], "admit_ex with the session's controls spelled out")
        ref, fb = alone(eng, dict(base, controls=SESSION, max_steps=None), voice)
        assert_same(got[0], ref, "uniform")
        ref, fb5 = alone(eng, dict(base, controls=SESSION, max_steps=5), voice)
        assert_same(got[2], ref, "max_steps 5")
        assert got[2][3] == 5
        assert fallbacks == 3 * fb + fb5 == 0, (fallbacks, fb, fb5)   # the uniform list-served session's counter: the sum of the alone runs', none under top_k 50
    finally:
        eng.close()


@pytest.mark.parametrize("left", ["B", "C", "D"])
def test_slots_a_differing_request_has_left_hold_nothing_of_it(pkg, engine, crafted, voice, left):  # noqa: F811
    """A request under the session's controls takes the slots a differing request has left, once after that request was cancelled mid-run and once after it
    finished by itself and was collected: both times it equals itself alone, and it adds nothing to the fallback counter. A table row that kept the leaver's
    entry would show: scope 1 (C) penalises the whole history on the device and the last id again on the host; top_k 5 (B) keeps too short a list; top_k 200
    (D) writes no list, so every step would fetch the full row. On the crafted head (every logits row is the known bias, as in the CPU file's sharpness check)
    so that a wrong penalty or keep bound changes the sampled ids. With the rows left unwritten at an admission under the session's controls, cases C and D fail
    (other codes; 30 fallbacks too many); case B's shorter list happens to serve these ids and is kept for the pattern."""
    path, _, _ = crafted
    engine.load(ar=path)
    controls = dict(B=CONTROLS_B, C=CONTROLS_C, D=CONTROLS_D)[left]
    never = [40, 40]
    leaver = req(16, 2, 21, never, controls=controls)
    plain = req(9, 2, 22, never)                       # tts_ar_session_admit
    spelled = req(41, 2, 23, never, controls={})       # tts_ar_session_admit_ex with the session's controls
    shape = (2, 2, 41, 16)                             # two slots: every request sits in slots 0 .. 1
    set_controls(engine, SESSION)
    try:
        engine.ar_session_open(*shape, mask_stop=True, retire=True, row_controls=True)
    finally:
        set_controls(engine, DEFAULTS)
    try:
        def to_the_end(r):
            rid = admit(engine, r, voice)
            for _ in range(shape[3]):
                if engine.ar_session_step() == 0:
                    break
            assert engine.ar_session_finished() == [rid]
            return engine.ar_session_collect(rid, want_latents=False)

        rid = admit(engine, leaver, voice)
        for _ in range(5):
            engine.ar_session_step()
        engine.ar_session_cancel(rid)                  # mid-run: nothing but the book is released
        fb0 = engine.topk_fallbacks()
        assert fb0 == (2 * 5 if left == "D" else 0)
        got_plain = to_the_end(plain)
        assert engine.topk_fallbacks() == fb0
        to_the_end(dict(leaver, max_steps=6))          # the leaver again: this time it finishes by itself, is parked and collected
        fb1 = engine.topk_fallbacks()
        assert fb1 - fb0 == (2 * 5 if left == "D" else 0)
        got_spelled = to_the_end(spelled)
        assert engine.topk_fallbacks() == fb1 and engine.ar_session_recaptures() == 0
    finally:
        engine.ar_session_close()
    for r, got in ((plain, got_plain), (spelled, got_spelled)):
        ref, fb = alone(engine, dict(r, max_steps=shape[3]), voice, want_latents=False)
        assert fb == 0 and got[3] == shape[3]
        assert_same(got, ref, (left, r["seed"]), latents=False)
