"""GPU: the autoregressive sampler's controls through the decode step — penalty scope 1 (the history bitmap and the penalising prefilter of ar.hip), the keep
window that follows ar_top_k, the step graphs' signature — against the host sampler fed the same history (tts_ar_step + tts_sample) and against the literal
formulation (tts_host_sample_row_ex mode 1) on a head whose logits are known exactly."""
import numpy as np
import pytest

from conftest import DEFAULT_TOKENS
from test_sampler_controls_cpu import DEFAULTS, OPTION_OF, V

pytestmark = pytest.mark.gpu

HOT_FIXED = [1, 31, 32, 33, 8191, 8192, 8193]  # bitmap word edges (bit 31 | bit 0 of the next word), the last word (8192, 8193: bits 0 and 1 of word 256)


def set_controls(eng, temperature=0.8, top_k=50, top_p=0.8, penalty=2.0, scope=0):
    for k, v in dict(temperature=temperature, top_k=top_k, top_p=top_p, penalty=penalty).items():
        eng.set_option(OPTION_OF[k], v)
    eng.set_option("ar_penalty_scope", scope)


@pytest.fixture
def controls(engine):
    """set(...) changes the engine's sampler controls; the defaults are restored afterwards whatever happens"""
    try:
        yield lambda **kw: set_controls(engine, **kw)
    finally:
        set_controls(engine)
        engine.set_option("device_topk", 1)
        engine.set_stop_schedule(None)


@pytest.fixture(scope="module")
def crafted(pkg, small_models, tmp_path_factory):
    """(path, bias): small_models' AR weights with lm_head.1.weight = 0, so every logits row IS the bias: 60 hot ids from U(4, 6) (among them HOT_FIXED), the rest
    N(0, 1). Penalised by 2 the hot ids (2 .. 3) interleave with the cold maximum (about 3.7)."""
    from tortoise_cpp_amd import synth_weights as SW
    t = SW.read_ggml(small_models + "/ggml-model.bin")
    rs = np.random.RandomState(31)
    bias = rs.randn(V)
    hot = np.unique(np.concatenate([HOT_FIXED, rs.randint(2, 8190, 53)]))
    bias[hot] = rs.uniform(4, 6, len(hot))
    bias = bias.astype(np.float32)
    t["inference_model.lm_head.1.weight"][:] = 0
    t["inference_model.lm_head.1.bias"][:] = bias
    path = str(tmp_path_factory.mktemp("sampler_controls") / "ar_hot.bin")
    w = SW.GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return path, bias, hot


def _pad(hist):
    n = max(len(h) for h in hist)
    return np.array([sorted(h) + [min(h)] * (n - len(h)) for h in hist], np.int32)  # repeated ids are penalised once


def stepwise(engine, toks, voice, B, S, seed, mask, fused, twice_at=-1):
    """The decode loop with the stepwise ABI under penalty scope 1. fused(i): tts_ar_step_sample (history kept and applied on the device); otherwise tts_ar_step +
    tts_sample fed the accumulated history [1, 8192, every id fed so far]. twice_at: that step is fed twice (the first time through tts_ar_step)."""
    engine.seed(seed)
    engine.ar_begin(toks, voice, B, S)
    lg = engine.ar_prefill()
    if mask:
        lg[:, 8193] = -1e30
    hist = [{1, 8192} for _ in range(B)]
    s = engine.sample(lg, _pad(hist))
    out, fb = [s], 0
    for i in range(S - 1):
        for b in range(B):
            hist[b].add(int(s[b]))
        if i == twice_at:
            engine.ar_step(s, i)
        if fused(i):
            s = engine.ar_step_sample(s, i, mask_stop=mask)
            fb += engine.topk_fallbacks()
        else:
            lg = engine.ar_step(s, i)
            if mask:
                lg[:, 8193] = -1e30
            s = engine.sample(lg, _pad(hist))
        out.append(s)
    return np.stack(out), engine.rng_uniform(), fb


@pytest.mark.parametrize("B,mask", [(1, True), (3, False), (16, True), (16, False), (17, True), (17, False), (3, True), (1, False)])
def test_scope1_step_sample_is_step_then_sample_with_the_history(engine, controls, small_models, crafted, voice, B, mask):
    """Penalty scope 1: tts_ar_step_sample returns the ids and leaves the RNG position of tts_ar_step + tts_sample fed the accumulated history — over 40 steps, also
    when the two forms alternate (the device set is then extended by both step graphs) and when one step is fed twice. Continuous logits (B = 16, 17: two tiles
    of the decode kernels) and the crafted head, where penalised hot ids sit at the list's threshold."""
    engine.load(ar=crafted[0] if B <= 3 else small_models + "/ggml-model.bin")
    controls(scope=1)
    toks, S, seed = DEFAULT_TOKENS, 40, 900 + B
    want, u_want, _ = stepwise(engine, toks, voice, B, S, seed, mask, lambda i: False)
    got, u_got, fb = stepwise(engine, toks, voice, B, S, seed, mask, lambda i: True)
    assert (got == want).all() and u_got == u_want, np.argwhere(got != want)[:4]
    assert fb == 0  # no ties in either head: every list decided
    mixed, u_mixed, _ = stepwise(engine, toks, voice, B, S, seed, mask, lambda i: i % 3 != 1)
    assert (mixed == want).all() and u_mixed == u_want
    twice, u_twice, _ = stepwise(engine, toks, voice, B, S, seed, mask, lambda i: i % 2 == 0, twice_at=7)
    assert (twice == want).all() and u_twice == u_want
    if mask:
        assert (got != 8193).all()


@pytest.mark.parametrize("mask", [False, True])
def test_scope1_sequence_is_the_literal_formulation_on_known_logits(pkg, engine, controls, crafted, voice, mask):
    """On the crafted head every logits row is the bias exactly, so the whole scope-1 sequence is a Python loop over the literal formulation with the engine's
    uniforms and the growing history; scope 0 gives another sequence (it repeats hot ids that scope 1 has pushed below the cold logits)."""
    path, bias, hot = crafted
    engine.load(ar=path)
    toks, B, S, seed = DEFAULT_TOKENS, 3, 40, 4711
    row = bias.copy()
    if mask:
        row[8193] = -1e30
    engine.seed(seed)
    u = np.array([[(engine.rng_uniform(), engine.rng_uniform())[1] for _ in range(B)] for _ in range(S)])
    want = np.empty((S, B), np.int32)
    for b in range(B):
        hist = [1, 8192]
        for i in range(S):
            want[i, b] = pkg.host_sample_row_ex(row, hist, u[i, b], mode=1, **DEFAULTS)
            hist.append(int(want[i, b]))
    controls(scope=1)
    got, _, fb = stepwise(engine, toks, voice, B, S, seed, mask, lambda i: True)
    assert (got == want).all() and fb == 0
    if not mask:
        assert set(HOT_FIXED) <= set(hot.tolist())
    controls(scope=0)
    engine.seed(seed)
    engine.ar_begin(toks, voice, B, S)
    lg = engine.ar_prefill()
    if mask:
        lg[:, 8193] = -1e30
    assert (lg == row[None]).all()
    s = engine.sample(lg, np.tile(np.array([1] * (len(toks) + 1) + [8192], np.int32), (B, 1)))
    ref0 = [s]
    for i in range(S - 1):
        s = engine.ar_step_sample(s, i, mask_stop=mask)
        ref0.append(s)
    ref0 = np.stack(ref0)
    assert (ref0 != got).any()  # the history is used
    hot_set = set(hot.tolist())
    assert any(np.bincount(ref0[:, b][np.isin(ref0[:, b], list(hot_set))], minlength=1).max() >= 2 for b in range(B))  # scope 0 repeats a hot id


PARAM_SETS = [dict(temperature=1.0, top_k=80, top_p=0.9, penalty=1.3, scope=1), dict(temperature=0.5, top_k=100, top_p=1.0, penalty=2.0, scope=1),
              dict(temperature=1.7, top_k=20, top_p=0.8, penalty=2.0, scope=0)]


def _driver_pair(pkg, engine, toks, voice, B, S, seed, **flags):
    res = []
    for on in (1, 0):
        engine.set_option("device_topk", on)
        engine.seed(seed)
        try:
            codes, rows, lats, steps = engine.autoregressive(toks, voice, B, S, **flags)
        except pkg.TtsError as e:  # strict mode may run out of steps: then both forms must
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


@pytest.mark.parametrize("params", PARAM_SETS, ids=lambda p: "t%g-k%d-p%g-r%g-s%d" % (p["temperature"], p["top_k"], p["top_p"], p["penalty"], p["scope"]))
@pytest.mark.parametrize("flags", ["mask_stop", "retire", "strict"])
def test_driver_device_topk_on_off_with_controls(pkg, engine, controls, small_models, crafted, voice, params, flags):
    """tts_autoregressive with the sampler's top-k on the device (lists; penalised lists under scope 1) and with full rows: same codes, rows, latents, steps, RNG
    position and stop status, and no list ever needs its full row on continuous logits for top-k <= 100 (the keep window follows top-k)."""
    toks = DEFAULT_TOKENS
    if flags == "strict":  # one candidate on the crafted head: the stop token is one of the hot ids, the loop ends when it is sampled
        engine.load(ar=crafted[0])
        controls(**params)
        res = _driver_pair(pkg, engine, toks, voice, 1, 200, 61)
        if _same(res):
            assert res[0][6] == 0
        return
    engine.load(ar=small_models + "/ggml-model.bin")
    controls(**params)
    if flags == "retire":
        B, S = 6, 30
        engine.set_stop_schedule([5, 30, 7, 12, 9, 15])
        res = _driver_pair(pkg, engine, toks, voice, B, S, 62, mask_stop=True, retire=True)
    else:
        B, S = 16, 30
        res = _driver_pair(pkg, engine, toks, voice, B, S, 63, mask_stop=True)
        assert res[0][3] == S
    assert _same(res)
    assert res[0][6] == 0, res[0][6]


@pytest.mark.parametrize("scope", [0, 1])
def test_top_k_above_100_samples_every_candidate_from_its_full_row(pkg, engine, controls, small_models, voice, scope):
    engine.load(ar=small_models + "/ggml-model.bin")
    controls(top_k=101, scope=scope)
    B, S = 3, 10
    res = _driver_pair(pkg, engine, DEFAULT_TOKENS, voice, B, S, 64, mask_stop=True)
    assert _same(res)
    assert res[0][6] == B * (S - 1)  # every sampled step after the prompt's: no 128-entry list serves this top-k


def test_multi_prompt_groups_equal_each_prompt_alone_under_scope1(engine, controls, small_models, voice):
    """Two prompts of different length, three candidates in all, penalty scope 1: every group is the prompt run alone with its RNG shard (a candidate's ids do not
    depend on the rest of the batch, the history least of all), and a second begin starts from a fresh history (the same call twice gives the same codes)."""
    engine.load(ar=small_models + "/ggml-model.bin")
    controls(temperature=1.0, top_k=80, top_p=0.9, penalty=1.3, scope=1)
    prompts = [DEFAULT_TOKENS, np.concatenate([DEFAULT_TOKENS[:-1], DEFAULT_TOKENS[1:-1], DEFAULT_TOKENS[-1:]]).astype(np.int32)]
    n_cand, S, seed = [2, 1], 30, 65
    c0 = [0, 2, 3]
    runs = []
    for _ in range(2):
        engine.seed(seed)
        runs.append(engine.autoregressive_multi(prompts, voice, n_cand, S, mask_stop=True))
    assert all((a == b).all() for a, b in zip(runs[0][0], runs[1][0]))
    codes, rows, lats, steps = runs[0]
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


def test_defaults_after_option_changes_equal_a_fresh_context(pkg, engine, controls, small_models, voice):
    """Every control is part of the step graphs' signature: after runs with other values (scope 1, another keep window, another penalty) the defaults give the ids of
    a context that never saw them, through the driver and through the stepwise form."""
    path = small_models + "/ggml-model.bin"
    engine.load(ar=path)
    toks, B, S = DEFAULT_TOKENS, 4, 16
    for params in PARAM_SETS + [dict(top_k=101, scope=1), dict(penalty=1.5, scope=1)]:
        controls(**params)
        engine.seed(1)
        engine.autoregressive(toks, voice, B, 6, mask_stop=True, want_latents=False)
        s = np.arange(B, dtype=np.int32) + 40
        engine.ar_begin(toks, voice, B, 4)
        engine.ar_prefill()
        engine.ar_step(s, 0)
        engine.ar_step_sample(s, 1)
    controls()
    fresh = pkg.Engine(0)
    try:
        fresh.load(ar=path)
        out = []
        for eng in (engine, fresh):
            eng.seed(66)
            codes, rows, lats, steps = eng.autoregressive(toks, voice, B, S, mask_stop=True, want_latents=False)
            eng.seed(67)
            eng.ar_begin(toks, voice, B, S)
            lg = eng.ar_prefill()
            s = eng.sample(lg, np.tile(np.array([1] * (len(toks) + 1) + [8192], np.int32), (B, 1)))
            seq = [s]
            for i in range(S - 1):
                s = eng.ar_step_sample(s, i)
                seq.append(s)
            out.append((codes, np.stack(seq), eng.rng_uniform(), eng.topk_fallbacks()))
        assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all() and out[0][2] == out[1][2] and out[0][3] == out[1][3] == 0
    finally:
        fresh.close()
