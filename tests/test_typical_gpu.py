"""GPU: locally typical sampling through the decode step (option "ar_typical_mass"; ar.hip: typical_members, sample_prefilter_typical_kernel and the typical
branch of sample_prefilter_rows_kernel) against the host sampler fed the same rows (tts_ar_step + tts_sample), against the literal formulation
(tts_host_sample_row_typical mode 1) on heads whose logits are known exactly, through the driver, and in both kinds of session. Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import DEFAULT_TOKENS
from test_ar_session_gpu import assert_same, prompt
from test_sampler_controls_gpu import crafted  # noqa: F401
from test_typical_cpu import DEFAULTS, V, np_distance, penalise

pytestmark = pytest.mark.gpu

ERR_STATE = -5
OPTION_OF = dict(temperature="ar_temperature", top_k="ar_top_k", top_p="ar_top_p", penalty="ar_repetition_penalty", scope="ar_penalty_scope",
                 typical_mass="ar_typical_mass")
OFF = dict(temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, scope=0, typical_mass=0.0)


def set_controls(eng, **kw):
    for k, v in dict(OFF, **kw).items():
        eng.set_option(OPTION_OF[k], v)


@pytest.fixture
def controls(engine):
    try:
        yield lambda **kw: set_controls(engine, **kw)
    finally:
        set_controls(engine)
        engine.set_option("device_topk", 1)
        engine.set_stop_schedule(None)


def head_with_bias(small_models, bias, path):
    """small_models' AR weights with lm_head.1.weight = 0: every logits row IS `bias` (the construction of test_sampler_controls_gpu.py's `crafted`)."""
    from tortoise_cpp_amd import synth_weights as SW
    t = SW.read_ggml(small_models + "/ggml-model.bin")
    t["inference_model.lm_head.1.weight"][:] = 0
    t["inference_model.lm_head.1.bias"][:] = bias
    w = SW.GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return path


@pytest.fixture(scope="module")
def gauss3(small_models, tmp_path_factory):
    """(path, bias): a Gaussian head scaled by 3, whose typical sets have 15 members at mass 0.05 (fewer than top-k 50) and 58 at mass 0.2 (fewer than the keep
    window's 64)."""
    bias = (np.random.RandomState(8).randn(V) * 3).astype(np.float32)
    return head_with_bias(small_models, bias, str(tmp_path_factory.mktemp("typical") / "ar_gauss3.bin")), bias


def prompt_ids(toks, B):
    return np.tile(np.array([1] * (len(toks) + 1) + [8192], np.int32), (B, 1))


def _pad(hist):
    n = max(len(h) for h in hist)
    return np.array([sorted(h) + [min(h)] * (n - len(h)) for h in hist], np.int32)


def stepwise(engine, toks, voice, B, S, seed, mask, scope, fused):
    """The decode loop with the stepwise ABI. fused(i): tts_ar_step_sample; otherwise tts_ar_step + tts_sample fed the ids the scope names (scope 0: the ids
    of the last input; scope 1: the accumulated history). Returns (ids [S, B], the next uniform, fallbacks)."""
    engine.seed(seed)
    engine.ar_begin(toks, voice, B, S)
    lg = engine.ar_prefill()
    if mask:
        lg[:, 8193] = -1e30
    hist = [{1, 8192} for _ in range(B)]
    s = engine.sample(lg, prompt_ids(toks, B))
    out, fb = [s], 0
    for i in range(S - 1):
        for b in range(B):
            hist[b].add(int(s[b]))
        if fused(i):
            s = engine.ar_step_sample(s, i, mask_stop=mask)
            fb += engine.topk_fallbacks()
        else:
            lg = engine.ar_step(s, i)
            if mask:
                lg[:, 8193] = -1e30
            s = engine.sample(lg, _pad(hist) if scope else s.reshape(B, 1))
        out.append(s)
    return np.stack(out), engine.rng_uniform(), fb


@pytest.mark.parametrize("scope", [0, 1])
@pytest.mark.parametrize("mask", [False, True], ids=["no_mask", "mask_stop"])
@pytest.mark.parametrize("mass", [0.9, 0.2, 0.05])
@pytest.mark.parametrize("B", [1, 3, 17])
def test_fused_step_is_step_then_sample(engine, controls, small_models, voice, B, mass, mask, scope):
    """tts_ar_step_sample returns the ids and leaves the RNG position of tts_ar_step + tts_sample, also when the two forms alternate; on continuous logits no
    list needs its full row."""
    engine.load(ar=small_models + "/ggml-model.bin")
    controls(typical_mass=mass, scope=scope)
    toks, S, seed = DEFAULT_TOKENS, 24, 300 + B
    want, u_want, _ = stepwise(engine, toks, voice, B, S, seed, mask, scope, lambda i: False)
    got, u_got, fb = stepwise(engine, toks, voice, B, S, seed, mask, scope, lambda i: True)
    assert (got == want).all() and u_got == u_want, np.argwhere(got != want)[:4]
    assert fb == 0
    mixed, u_mixed, _ = stepwise(engine, toks, voice, B, S, seed, mask, scope, lambda i: i % 3 != 1)
    assert (mixed == want).all() and u_mixed == u_want


def literal_loop(pkg, row, u, scope, mass, **kw):
    hist, out = [1, 8192], []
    for i, x in enumerate(u):
        ids = hist if (i == 0 or scope == 1) else [out[-1]]
        out.append(pkg.host_sample_row_typical(row, ids, x, typical_mass=mass, mode=1, **kw))
        hist.append(out[-1])
    return np.array(out, np.int32)


def engine_uniforms(engine, seed, S, B):
    engine.seed(seed)
    return np.array([[(engine.rng_uniform(), engine.rng_uniform())[1] for _ in range(B)] for _ in range(S)])


@pytest.mark.parametrize("mask", [False, True], ids=["no_mask", "mask_stop"])
@pytest.mark.parametrize("scope,mass", [(0, 0.9), (1, 0.9), (0, 0.2), (1, 0.05)])
def test_crafted_head_sequence_is_the_literal_loop(pkg, engine, controls, crafted, voice, scope, mass, mask):  # noqa: F811
    """On the crafted head every logits row is the bias exactly: the whole sequence is a Python loop over the literal probe with the engine's uniforms. It is
    not the mass-0 sequence, and at mass 0.9 the row's argmax (which the typical set drops) is never sampled."""
    path, bias, hot = crafted
    engine.load(ar=path)
    toks, B, S, seed = DEFAULT_TOKENS, 3, 32, 4712
    row = bias.copy()
    if mask:
        row[8193] = -1e30
    u = engine_uniforms(engine, seed, S, B)
    want = np.stack([literal_loop(pkg, row, u[:, b], scope, mass, **DEFAULTS) for b in range(B)], 1)
    controls(typical_mass=mass, scope=scope)
    got, _, fb = stepwise(engine, toks, voice, B, S, seed, mask, scope, lambda i: True)
    assert (got == want).all(), np.argwhere(got != want)[:4]
    print("crafted head, scope %d mass %g mask %d: %d of %d rows fell back" % (scope, mass, mask, fb, (S - 1) * B))
    off = np.stack([literal_loop(pkg, row, u[:, b], scope, 0.0, **DEFAULTS) for b in range(B)], 1)
    assert (off != want).any()
    if mass == 0.9:
        assert int(np.argmax(row)) not in set(got.ravel().tolist()) and int(np.argmax(row)) in set(off.ravel().tolist())


@pytest.mark.parametrize("mass,lo,hi", [(0.05, 8, 30), (0.2, 50, 63)])
def test_sets_below_the_keep_window_come_as_whole_set_lists(pkg, engine, controls, gauss3, voice, mass, lo, hi):
    """The Gaussian head scaled by 3: the typical set has fewer members than the keep window's lower bound (64), at mass 0.05 fewer than top-k 50. The device
    hands the whole set over (header flag) and the host tail accepts it: the literal's ids with no fallback."""
    path, bias = gauss3
    engine.load(ar=path)
    toks, B, S, seed = DEFAULT_TOKENS, 3, 24, 99
    u = engine_uniforms(engine, seed, S, B)
    want = np.stack([literal_loop(pkg, bias, u[:, b], 0, mass, **DEFAULTS) for b in range(B)], 1)
    sizes = [int(pkg.host_typical_keep(penalise(bias, [int(t)], 2.0), mass).sum()) for t in want[:-1].ravel()]
    assert lo <= min(sizes) and max(sizes) <= hi, (min(sizes), max(sizes))
    controls(typical_mass=mass)
    got, _, fb = stepwise(engine, toks, voice, B, S, seed, False, 0, lambda i: True)
    assert (got == want).all() and fb == 0, (np.argwhere(got != want)[:4], fb)


def test_adversarial_masses_on_the_crafted_head(pkg, engine, controls, crafted, voice):  # noqa: F811
    """The two floats either side of a cumulative mass c_j of the row the step sees (the bias with the fed id penalised), for several prefixes j: the ids are the
    literal's whether the device decided the set or handed the row back."""
    path, bias, hot = crafted
    engine.load(ar=path)
    toks, B = DEFAULT_TOKENS, 3
    fed = np.array([int(hot[3]), 77, int(np.argmax(bias))], np.int32)
    engine.ar_begin(toks, voice, B, 4)
    engine.ar_prefill()
    fb_total = n = 0
    for b0 in range(B):
        pen = penalise(bias, [int(fed[b0])], 2.0)
        x = pen.astype(np.float64)
        lnp = (x - x.max()) - np.log(np.exp(x - x.max()).sum())
        c = np.cumsum(np.exp(lnp)[np.argsort(np_distance(pen), kind="stable")])
        for j in (0, 15, 63, 64, 128, 3000):
            lo = np.float32(c[j])
            if float(lo) > c[j]:
                lo = np.nextafter(lo, np.float32(0))
            for m in (lo, np.nextafter(lo, np.float32(1))):
                controls(typical_mass=float(m))
                u = engine_uniforms(engine, 1000 + n, 1, B)[0]
                engine.seed(1000 + n)
                got = engine.ar_step_sample(fed, 0)
                fb_total += engine.topk_fallbacks()
                want = [pkg.host_sample_row_typical(bias, [int(fed[b])], u[b], typical_mass=float(m), mode=1, **DEFAULTS) for b in range(B)]
                assert list(got) == want, (b0, j, float(m), got, want)
                n += B
    print("adversarial masses: %d of %d rows fell back to the full row" % (fb_total, n))


def _driver_pair(pkg, engine, toks, voice, B, S, seed, **flags):
    res = []
    for on in (1, 0):
        engine.set_option("device_topk", on)
        engine.seed(seed)
        try:
            codes, rows, lats, steps = engine.autoregressive(toks, voice, B, S, **flags)
        except pkg.TtsError as e:
            res.append(("err", str(e)))
            continue
        res.append((codes, rows, lats, steps, engine.rng_uniform(), engine.ar_stop_status(B), engine.topk_fallbacks()))
    engine.set_option("device_topk", 1)
    return res


def _same(res):
    failed = [isinstance(r[0], str) for r in res]
    if any(failed):
        assert all(failed), res
        return False
    a, b = res
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[3] == b[3] and a[4] == b[4] and (a[5] == b[5]).all()
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    return True


@pytest.mark.parametrize("scope,mass", [(0, 0.9), (1, 0.2)])
@pytest.mark.parametrize("flags", ["mask_stop", "retire", "strict"])
def test_driver_device_topk_on_off(pkg, engine, controls, small_models, crafted, voice, flags, scope, mass):  # noqa: F811
    """tts_autoregressive with the typical set decided on the device and with full rows on the host: same codes, rows, latents, steps, RNG state, stop status."""
    toks = DEFAULT_TOKENS
    if flags == "strict":
        engine.load(ar=crafted[0])
        controls(typical_mass=mass, scope=scope)
        _same(_driver_pair(pkg, engine, toks, voice, 1, 200, 61))
        return
    engine.load(ar=small_models + "/ggml-model.bin")
    controls(typical_mass=mass, scope=scope)
    if flags == "retire":
        engine.set_stop_schedule([5, 30, 7, 12, 9, 15])
        res = _driver_pair(pkg, engine, toks, voice, 6, 30, 62, mask_stop=True, retire=True)
    else:
        res = _driver_pair(pkg, engine, toks, voice, 16, 30, 63, mask_stop=True)
        assert res[0][3] == 30
    assert _same(res)
    assert res[0][6] == 0, res[0][6]


def test_top_k_200_takes_the_full_row_path(pkg, engine, controls, small_models, voice):
    engine.load(ar=small_models + "/ggml-model.bin")
    controls(typical_mass=0.5, top_k=200)
    B, S = 3, 10
    res = _driver_pair(pkg, engine, DEFAULT_TOKENS, voice, B, S, 64, mask_stop=True)
    assert _same(res)
    assert res[0][6] == B * (S - 1)


def test_multi_prompt_groups_equal_each_prompt_alone(engine, controls, small_models, voice):
    engine.load(ar=small_models + "/ggml-model.bin")
    controls(typical_mass=0.2)
    prompts = [DEFAULT_TOKENS, np.concatenate([DEFAULT_TOKENS[:-1], DEFAULT_TOKENS[1:-1], DEFAULT_TOKENS[-1:]]).astype(np.int32)]
    n_cand, S, seed = [2, 1], 24, 65
    c0 = [0, 2, 3]
    engine.seed(seed)
    codes, rows, lats, steps = engine.autoregressive_multi(prompts, voice, n_cand, S, mask_stop=True)
    try:
        for g, p in enumerate(prompts):
            engine.set_option("rng_shard_offset", c0[g])
            engine.set_option("rng_shard_total", 3)
            engine.seed(seed)
            ca, ra, la, sa = engine.autoregressive(p, voice, n_cand[g], S, mask_stop=True)
            assert (codes[g] == ca).all() and (rows[g] == ra).all() and sa == steps
            for x, y in zip(lats[g], la):
                assert np.array_equal(x, y)
    finally:
        engine.set_option("rng_shard_offset", 0)
        engine.set_option("rng_shard_total", 0)


# ---- sessions ----
SHAPE = (20, 16, 41, 20)   # slots (two tiles, the second partly empty), max_cand, max_text, max_steps


def sreq(n_text, n_cand, seed, stop_at, at=0, controls=None):
    return dict(tokens=prompt(n_text, 100 + seed), n_cand=n_cand, seed=seed, stop_at=list(stop_at), at=at, controls=controls)


def run_session(eng, reqs, voice, session_controls, rows, want_latents=True):
    """Opens a session under session_controls, puts the context back to OFF, admits reqs[k] once `at` steps have run, collects every request when it is first
    reported finished. ({k: collect's tuple}, recaptures, fallbacks)"""
    set_controls(eng, **session_controls)
    try:
        eng.ar_session_open(*SHAPE, mask_stop=True, retire=True, row_controls=rows)
    finally:
        set_controls(eng)
    try:
        out, rid_of = {}, {}
        pending = sorted(range(len(reqs)), key=lambda k: reqs[k]["at"])
        step = 0
        while pending or rid_of:
            assert step < 100
            for rid in eng.ar_session_finished():
                k = next(k for k, r in rid_of.items() if r == rid)
                out[k] = eng.ar_session_collect(rid, want_latents=want_latents)
                del rid_of[k]
            while pending and reqs[pending[0]]["at"] <= step:
                k = pending.pop(0)
                r = reqs[k]
                kw = {} if r["controls"] is None else dict(controls=r["controls"])
                rid_of[k] = eng.ar_session_admit(r["tokens"], voice, r["n_cand"], r["seed"], r["stop_at"], **kw)
            eng.ar_session_step()
            step += 1
        return out, eng.ar_session_recaptures(), eng.topk_fallbacks()
    finally:
        eng.ar_session_close()


def alone(eng, r, voice, ctl, want_latents=True):
    set_controls(eng, **ctl)
    eng.set_stop_schedule(r["stop_at"])
    try:
        eng.seed(r["seed"])
        codes, rows, lats, steps = eng.autoregressive(r["tokens"], voice, r["n_cand"], SHAPE[3], mask_stop=True, retire=True, want_latents=want_latents)
        return codes, rows, lats, steps, eng.ar_stop_status(r["n_cand"])
    finally:
        eng.set_stop_schedule(None)
        set_controls(eng)


def test_uniform_session_with_the_mass_pinned(engine, small_models, voice):
    engine.load(ar=small_models + "/ggml-model.bin")
    pinned = dict(typical_mass=0.2, temperature=0.9)
    reqs = [sreq(9, 3, 11, [4, 9, 20]), sreq(41, 16, 12, [5, 9, 20, 12, 7, 20, 3, 18, 11, 20, 6, 14, 20, 8, 20, 10]), sreq(16, 1, 13, [15], at=3)]
    got, recaptures, _ = run_session(engine, reqs, voice, pinned, rows=False)
    assert recaptures == 0
    for k, r in enumerate(reqs):
        assert_same(got[k], alone(engine, r, voice, pinned), ("uniform", k))
    assert (alone(engine, reqs[0], voice, dict(temperature=0.9), want_latents=False)[0] != got[0][0]).any()


@pytest.mark.parametrize("weights", ["f32", "fp16"])
def test_rows_session_with_masses_side_by_side(pkg, small_models, voice, weights):
    """TTS_AR_ROW_CONTROLS: requests of mass 0, 0.2 and 0.9 (scope 0 and 1) beside each other in one launch, each the request alone; no re-capture."""
    eng = pkg.Engine(0)
    try:
        if weights == "fp16":
            eng.set_option("ar_weights", 1)
        eng.load(ar=small_models + "/ggml-model.bin")
        lat = weights == "f32"
        reqs = [sreq(9, 3, 11, [4, 9, 20], controls=dict(typical_mass=0.0)),
                sreq(41, 14, 12, [5, 9, 20, 12, 7, 20, 3, 18, 11, 20, 6, 14, 20, 8], controls=dict(typical_mass=0.2)),   # slots 3 .. 16: across the tile boundary
                sreq(16, 2, 13, [15, 20], at=2, controls=dict(typical_mass=0.9, scope=1)),
                sreq(16, 1, 14, [20], at=3, controls=dict(typical_mass=0.05, top_k=20))]
        session = dict(temperature=0.9)
        got, recaptures, _ = run_session(eng, reqs, voice, session, rows=True, want_latents=lat)
        assert recaptures == 0 and sorted(got) == [0, 1, 2, 3]
        for k, r in enumerate(reqs):
            assert_same(got[k], alone(eng, r, voice, dict(session, **r["controls"]), want_latents=lat), (weights, k), latents=lat)
        other = alone(eng, reqs[1], voice, session, want_latents=False)
        assert (other[0] != got[1][0]).any()
    finally:
        eng.close()


def test_a_differing_mass_needs_the_flag_and_an_old_size_descriptor_runs_under_the_sessions_mass(pkg, engine, small_models, voice):
    engine.load(ar=small_models + "/ggml-model.bin")
    pinned = dict(typical_mass=0.2)
    r = sreq(16, 2, 31, [7, 20])
    set_controls(engine, **pinned)
    try:
        engine.ar_session_open(*SHAPE, mask_stop=True, retire=True)
    finally:
        set_controls(engine)
    try:
        with pytest.raises(pkg.TtsError, match="status %d" % ERR_STATE):
            engine.ar_session_admit(r["tokens"], voice, 2, r["seed"], r["stop_at"], controls=dict(typical_mass=0.5))
        assert engine.ar_session_room() == SHAPE[0]
        assert engine.ar_request().typical_mass == float(np.float32(0.2))   # tts_ar_request_init: the pinned mass
        # a caller built before the field existed: struct_size 64, the bytes behind it are not the library's to read
        req = pkg.ArRequest()
        req.struct_size = pkg.AR_REQUEST_SIZE_V0
        req.typical_mass = 0.77
        engine._ck(engine.L.tts_ar_request_init(engine.h, C.byref(req)))
        assert req.typical_mass == 0.77 and req.top_k == 50
        req.n_cand, req.seed = 2, r["seed"]
        stop = np.array(r["stop_at"], np.int32)
        req.stop_at = stop.ctypes.data
        tok = np.ascontiguousarray(r["tokens"], np.int32)
        rid = engine._ck(engine.L.tts_ar_session_admit_ex(engine.h, tok.ctypes.data_as(C.c_void_p), len(tok), voice.ctypes.data_as(C.c_void_p), C.byref(req)))
        engine._session_cand[rid] = 2
        while engine.ar_session_step():
            pass
        got = engine.ar_session_collect(rid)
    finally:
        engine.ar_session_close()
    assert_same(got, alone(engine, r, voice, pinned), "old-size descriptor")


def test_switching_on_and_off(pkg, engine, controls, crafted, voice):  # noqa: F811
    """The mass is part of the step graphs' signature: after on -> off the outputs are a fresh context's bit for bit, and after off -> on (and between two
    masses) no stale graph is replayed. On the crafted head, where each mass gives another sequence."""
    path = crafted[0]
    engine.load(ar=path)
    toks, B, S = DEFAULT_TOKENS, 4, 16

    def run(eng, seed):
        eng.seed(seed)
        codes = eng.autoregressive(toks, voice, B, S, mask_stop=True, want_latents=False)[0]
        seq, u, _ = stepwise(eng, toks, voice, B, S, seed + 1, False, 0, lambda i: True)
        return codes, seq, u

    off0 = run(engine, 70)
    controls(typical_mass=0.9)
    on9 = run(engine, 70)
    controls(typical_mass=0.2)
    on2 = run(engine, 70)
    controls()
    off1 = run(engine, 70)
    fresh = pkg.Engine(0)
    try:
        fresh.load(ar=path)
        ref_off = run(fresh, 70)
        set_controls(fresh, typical_mass=0.2)
        ref_on2 = run(fresh, 70)
        set_controls(fresh, typical_mass=0.9)
        ref_on9 = run(fresh, 70)
    finally:
        fresh.close()
    for got, ref in ((off0, ref_off), (off1, ref_off), (on9, ref_on9), (on2, ref_on2)):
        assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and got[2] == ref[2]
    assert (on9[1] != off0[1]).any() and (on2[1] != on9[1]).any()
