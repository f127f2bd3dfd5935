"""GPU: the device sampler (option ar_sampler = 1; csrc/ar.hip: sample_device_kernel) against the rule of tests/sample_device_ref.py on planted rows, its
bit identities, and tts_autoregressive on it against a host-driven loop of tts_ar_step + tts_sample_device: every ar_sync_steps, sharded, beside the host sampler."""
import numpy as np
import pytest

import sample_device_ref as R
from conftest import DEFAULT_TOKENS as TOKS
from test_hifigan_cpu import hifigan_model  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = R.SEED
DEFAULTS = dict(ar_temperature=0.8, ar_top_k=50, ar_top_p=0.8, ar_penalty_scope=0, ar_sampler=0, ar_sync_steps=1, rng_shard_offset=0, rng_shard_total=0)


@pytest.fixture
def eng(engine):
    """the shared engine, seeded; its options are the defaults again afterwards whatever happens"""
    engine.seed(SEED)
    yield engine
    for k, v in DEFAULTS.items():
        engine.set_option(k, v)


def options(eng, **kw):
    for k, v in kw.items():
        eng.set_option(k, v)


def check(got, ref, what):
    want, decided, near = ref
    assert got == want if decided else got in near, (what, got, want, near)


@pytest.mark.parametrize("case", range(len(R.planted_cases())))
def test_planted_rows_against_the_reference(pkg, eng, case):
    n, top_k, top_p, temperature, _, mask = R.planted_cases()[case]
    rows, ids = R.planted_inputs(case)
    options(eng, ar_top_k=top_k, ar_top_p=top_p, ar_temperature=temperature)
    for it in range(R.ITERATIONS):
        got = eng.sample_device(rows, ids, it, mask_stop=mask)
        for b in range(n):
            check(got[b], R.sample_ref(rows[b], ids[b], pkg.host_ar_uniform(SEED, b, it), temperature, top_k, top_p, 2.0, mask), (it, b, R.KINDS[(b + case) % 6]))


def test_an_all_equal_row_is_refused_and_nothing_is_written(eng):
    rows = np.stack([R.planted_inputs(0)[0][0], np.full(R.V, 0.25, np.float32)])
    out = np.full(2, -7, np.int32)
    rc = eng.L.tts_sample_device(eng.h, rows.ctypes.data, 2, np.array([1, 1], np.int32).ctypes.data, 1, 0, 0, 0, out.ctypes.data)
    assert rc == -6 and (out == -7).all(), (rc, out)  # TTS_ERR_LIMIT


def test_bit_identities_of_the_kernel(eng):
    rows, ids = (a[:4] for a in R.planted_inputs(8))
    whole = eng.sample_device(rows, ids, 3)
    assert (eng.sample_device(rows, ids, 3) == whole).all()  # two runs
    for b in range(4):  # a row alone, at its place in the batch
        assert eng.sample_device(rows[b:b + 1], ids[b:b + 1], 3, first_candidate=b)[0] == whole[b]
    halves = [eng.sample_device(rows[c:c + 2], ids[c:c + 2], 3, first_candidate=c) for c in (0, 2)]
    assert (np.concatenate(halves) == whole).all()
    assert len({int(eng.sample_device(rows[:1], ids[:1], it)[0]) for it in range(16)}) > 1  # the iteration moves the draw


def host_loop(pkg, eng, voice, B, S, scope, mask):
    """tts_ar_step (full logits) + tts_sample_device under tts_autoregressive's penalty ids: [1 ... 1, 8192], then the token fed (scope 0) or the history;
    scope 0: every draw against the reference"""
    eng.ar_begin(TOKS, voice, B, S)
    hist = [[1, 8192] for _ in range(B)]
    ids = np.tile(np.array([1] * (len(TOKS) + 1) + [8192], np.int32), (B, 1))
    out = []
    for it in range(S):
        lg = eng.ar_prefill() if it == 0 else eng.ar_step(out[-1], it - 1)
        out.append(eng.sample_device(lg, ids, it, mask_stop=mask))
        for b in range(B):
            if not scope:
                check(out[-1][b], R.sample_ref(lg[b], ids[b], pkg.host_ar_uniform(SEED, b, it), mask_stop=mask), (it, b))
            hist[b].append(int(out[-1][b]))
        ids = np.array([h + [1] * (S + 2 - len(h)) for h in hist], np.int32) if scope else out[-1][:, None]
    return np.stack(out, 1)  # [B, S]


@pytest.mark.parametrize("scope,mask", [(0, True), (1, True), (0, False)])
def test_autoregressive_is_the_host_driven_loop(pkg, eng, small_models, voice, scope, mask):
    B, S = 3, 14
    eng.load(ar=small_models + "/ggml-model.bin")
    options(eng, ar_sampler=1, ar_penalty_scope=scope)
    want = host_loop(pkg, eng, voice, B, S, scope, mask)
    codes = eng.autoregressive(TOKS, voice, B, S, mask_stop=mask, retire=not mask)[0]
    for b in range(B):
        n = S if 8193 not in want[b] else list(want[b]).index(8193)  # a sequence freezes at its first stop token
        assert (codes[b, 1:1 + n] == want[b, :n]).all(), (b, codes[b, :S + 2], want[b])


@pytest.fixture(scope="module")
def stop_model(small_models, tmp_path_factory):
    """small_models' AR weights with the stop token's bias raised by 7.5 to the rows' usual maximum (the head's logits: standard deviation 2.6, maxima near 9,
    the stop token's own about 1): it is drawn every few steps"""
    from tortoise_cpp_amd import synth_weights as SW
    t = SW.read_ggml(small_models + "/ggml-model.bin")
    t["inference_model.lm_head.1.bias"][8193] += 7.5
    path = str(tmp_path_factory.mktemp("sample_device") / "ar_stop.bin")
    w = SW.GgmlWriter(path)
    for name, arr in t.items():
        w.add(name, arr)
    w.close()
    return path


@pytest.mark.parametrize("groups,retire", [(1, False), (1, True), (2, True)])
def test_sync_steps_change_nothing(eng, stop_model, voice, groups, retire):
    """ar_sync_steps 1, 4 and 7 (neither divides the run): codes, rows, latents, steps and the stop status are identical; under TTS_AR_RETIRE candidates end at
    different steps, and steps enqueued behind the end are discarded. (Strict mode needs the mask to end at max_steps.)"""
    eng.load(ar=stop_model)
    res = {}
    for N in (1, 4, 7):
        options(eng, ar_sampler=1, ar_sync_steps=N)
        codes, rows, lats, steps = eng.autoregressive_multi([TOKS, TOKS[:9]][:groups], voice, 4, 30, mask_stop=not retire, retire=retire)
        stopped = eng.ar_stop_status(4 * groups)
        assert not retire or (0 < stopped.sum() and len(set(np.concatenate(rows))) > 1), (stopped, rows)  # the ended flag was at work
        res[N] = [a.tobytes() for a in codes + rows + sum(lats, [])] + [steps, stopped.tobytes()]
    assert res[4] == res[1] and res[7] == res[1]


def test_shards_the_generator_and_the_host_sampler_beside_it(pkg, eng, small_models, voice, tmp_path):
    B, S = 4, 12
    eng.load(ar=small_models + "/ggml-model.bin")
    options(eng, ar_sampler=1, ar_sync_steps=4)
    eng.rng_save_state(str(tmp_path / "before"))
    whole = eng.autoregressive(TOKS, voice, B, S, mask_stop=True)[0]
    eng.rng_save_state(str(tmp_path / "after"))
    assert open(tmp_path / "before").read() == open(tmp_path / "after").read()  # the context's mt19937 was never touched
    eng.set_option("ar_sampler", 0)
    host = eng.autoregressive(TOKS, voice, B, S, mask_stop=True)[0]
    fresh = pkg.Engine(0)  # ... and the host sampler goes on as on a fresh context with the same seed
    fresh.load(ar=small_models + "/ggml-model.bin")
    fresh.seed(SEED)
    assert (fresh.autoregressive(TOKS, voice, B, S, mask_stop=True)[0] == host).all()
    fresh.close()
    options(eng, ar_sampler=1, rng_shard_total=B)
    for off in (0, 2):  # two shards of 2 reproduce the call of 4
        eng.set_option("rng_shard_offset", off)
        assert (eng.autoregressive(TOKS, voice, 2, S, mask_stop=True)[0] == whole[off:off + 2]).all()


def test_sessions_and_streaming_are_refused(pkg, eng, small_models, hifigan_model, voice):
    eng.load(ar=small_models + "/ggml-model.bin")
    eng.load_hifigan(hifigan_model)
    eng.set_option("ar_sampler", 1)
    for call in (lambda: eng.ar_session_open(4, 2, 16, 8), lambda: eng.hifigan_stream(TOKS, voice, 8, pkg.AR_MASK_STOP, 4)):
        with pytest.raises(pkg.TtsError, match=r"host sampler.*status -5"):
            call()
    eng.set_option("ar_sampler", 0)
    eng.ar_session_open(4, 2, 16, 8)
    eng.ar_session_close()
    assert eng.hifigan_stream(TOKS, voice, 8, pkg.AR_MASK_STOP, 4)[4] == 8
