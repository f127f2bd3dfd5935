"""GPU: tts_ar_score_codes through the C ABI on the small synthetic AR weights (2 layers) and DEFAULT_TOKENS, candidates of 5, 12 and 40 codes
(tests/ar_score_ref.py: 6 and 6 + 13 rows run the latent pass's GEMV path, 3 x 41 its MFMA path).

  TRAIN mode   the hidden rows are tts_ar_latents' own, bit for bit, so the gate is the kernel's operand-derived bound (ar_score_ref.Ref) around the float64
               head applied to engine.ar_latents(...) of the same padded codes.
  DECODE mode  against float64 log-softmax of the oracle's prefill() / step() fed the same codes: 2 x 1e-4 x max |oracle logit| (the decode-logit gate of
               tests/test_ar_gpu.py, once for the logit and once for lse). The TRAIN-mode scores of the same input lie far outside that gate: the position quirk
               is pinned from both sides (the condition on the oracle alone: tests/test_ar_score_cpu.py).
  round trip   what a greedy sampler drew is what the scorer calls greedy. The sampler is made greedy with ar_top_k = 1 AND ar_repetition_penalty = 1: at the
               default 2 the penalised id of the last input can lose a maximum it holds, which is the sampler's rule and not the scorer's.
Measured on an MI355X (profiles/ar_score.txt): TRAIN at most 0.0016 of the bound; DECODE worst distance 1.6e-04 against a gate of 2.7e-03; TRAIN mode on the DECODE oracle 2.5 nats away."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ar_score_ref as R
from conftest import DEFAULT_TOKENS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, HIP, STATE, LIMIT = -1, -4, -5, -6
KEYS = ("logp", "stop_logp", "lse")


@pytest.fixture(scope="module")
def eng(pkg, small_models):
    e = pkg.Engine(0)
    e.load(ar=small_models + "/ggml-model.bin")
    yield e
    e.close()


@pytest.fixture(scope="module")
def decode_oracle(oracle, small_models, voice):
    """float32 logits [3][41][8194] of the oracle's decode steps on the candidates: computed once, shared, never written to"""
    l = R.oracle_decode_logits(oracle, small_models + "/ggml-model.bin", DEFAULT_TOKENS, voice, R.candidates())
    l.setflags(write=False)
    return l


def _targets(c):
    return np.concatenate([c, [8193]]).astype(np.int32)


@pytest.mark.parametrize("take", (1, 2, 3), ids=("6-rows-gemv", "26-rows-gemv", "123-rows-mfma"))
def test_train_mode_is_the_float64_head_on_the_engines_own_latents(eng, oracle, small_models, voice, take):
    cands = R.candidates()[:take]
    got = eng.ar_score_codes(DEFAULT_TOKENS, voice, cands, "train")
    n_rows = max(len(c) for c in cands) + 1
    eng.ar_begin(DEFAULT_TOKENS, voice, len(cands), 1)
    eng.ar_prefill()
    lat = eng.ar_latents(R.padded502(cands), n_rows)
    W, b = R.head(oracle.Model(small_models + "/ggml-model.bin"))
    worst = 0.0
    for i, c in enumerate(cands):
        n = len(c)
        ref = R.Ref(lat[i, :n + 1], W, b, _targets(c), 8194)
        ratios = ref.ratios({k: got[i][k] for k in KEYS})
        worst = max(worst, max(ratios.values()))
        assert max(ratios.values()) <= 1.0, (i, ratios)
        fails = ref.argmax_failures(got[i]["greedy"])
        assert not fails, fails[:3]
        assert 1.0 - ref.decided.mean() <= R.MAX_LEFT_OUT
    print("train mode, %d candidates: at most %.4f of the kernel's bound" % (take, worst))


def test_decode_mode_is_what_the_sampler_saw_and_train_mode_is_not(eng, voice, decode_oracle):
    cands = R.candidates()
    gate = 2.0 * R.DECODE_GATE * float(np.abs(decode_oracle).max())
    lp = R.log_softmax64(decode_oracle)
    dec, trn = eng.ar_score_codes(DEFAULT_TOKENS, voice, cands, "decode"), eng.ar_score_codes(DEFAULT_TOKENS, voice, cands, "train")
    worst, apart = 0.0, np.inf
    for i, c in enumerate(cands):
        n, t = len(c), _targets(c)
        rows = np.arange(n + 1)
        want = {"logp": lp[i, rows, t], "stop_logp": lp[i, :n + 1, 8193], "lse": R.direct64(decode_oracle[i, :n + 1].astype(np.float64))}
        for k in KEYS:
            worst = max(worst, float(np.abs(dec[i][k] - want[k]).max()))
        # the quirk from the other side: behind row 0 (position 0 in both modes) the latent pass's positions give other scores
        apart = min(apart, float(np.abs(trn[i]["logp"][1:] - want["logp"][1:]).max()))
        assert np.array_equal(dec[i]["logp"][:1], trn[i]["logp"][:1])
        top2 = np.sort(decode_oracle[i, :n + 1].astype(np.float64), axis=1)[:, -2:]
        sure = top2[:, 1] - top2[:, 0] > 2.0 * gate
        assert np.array_equal(dec[i]["greedy"][sure], decode_oracle[i, :n + 1].argmax(1)[sure])
    print("decode mode: worst distance from the oracle %.3e (gate %.3e); train mode on the same input: %.3e" % (worst, gate, apart))
    assert worst <= gate
    assert apart > gate


def test_greedy_round_trip(eng, voice, decode_oracle, oracle, small_models):
    saved = {"ar_top_k": 50, "ar_repetition_penalty": 2.0}
    try:
        eng.set_option("ar_top_k", 1)
        eng.set_option("ar_repetition_penalty", 1.0)
        eng.seed(11)
        codes, _, _, steps = eng.autoregressive(DEFAULT_TOKENS, voice, 1, 12, mask_stop=True, want_latents=False)
    finally:
        for k, v in saved.items():
            eng.set_option(k, v)
    c = codes[0, 1:13]
    assert (c < 8192).all()
    got = eng.ar_score_codes(DEFAULT_TOKENS, voice, [c], "decode")[0]
    ol = R.oracle_decode_logits(oracle, small_models + "/ggml-model.bin", DEFAULT_TOKENS, voice, [c])[0, :12, :8193].astype(np.float64)  # the stop column ignored
    gate = 2.0 * R.DECODE_GATE * float(np.abs(ol).max())
    top2 = np.sort(ol, axis=1)[:, -2:]
    sure = top2[:, 1] - top2[:, 0] > 2.0 * gate
    assert sure.sum() >= 6, "the margin leaves too little to compare"
    assert np.array_equal(got["greedy"][:12][sure], c[sure])


def test_identities_generator_and_neighbouring_calls(eng, voice):
    cands = R.candidates()
    eng.seed(5)
    want_u = [eng.rng_uniform() for _ in range(3)]
    eng.seed(9)
    before = eng.autoregressive(DEFAULT_TOKENS, voice, 2, 6, mask_stop=True)
    eng.ar_begin(DEFAULT_TOKENS, voice, 1, 1)
    eng.ar_prefill()
    lat_before = eng.ar_latents(R.padded502(cands[2:]), 41)
    eng.seed(5)
    three = eng.ar_score_codes(DEFAULT_TOKENS, voice, cands, "decode")
    assert [eng.rng_uniform() for _ in range(3)] == want_u, "the generator was touched"
    alone = eng.ar_score_codes(DEFAULT_TOKENS, voice, cands[2:], "decode")[0]  # 41 rows: the MFMA path, as the batch of three
    again = eng.ar_score_codes(DEFAULT_TOKENS, voice, cands, "decode")
    for k in KEYS + ("greedy",):
        assert np.array_equal(alone[k].view(np.uint32), three[2][k].view(np.uint32)), "a candidate's %s depends on its batch" % k
        for a, b in zip(three, again):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "two calls differ in %s" % k
    eng.seed(9)
    after = eng.autoregressive(DEFAULT_TOKENS, voice, 2, 6, mask_stop=True)
    assert np.array_equal(before[0], after[0]) and all(np.array_equal(a, b) for a, b in zip(before[2], after[2]))
    eng.ar_begin(DEFAULT_TOKENS, voice, 1, 1)
    eng.ar_prefill()
    assert np.array_equal(eng.ar_latents(R.padded502(cands[2:]), 41), lat_before)


def test_refusals_leave_the_outputs_alone(eng, voice):
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    toks, v = np.ascontiguousarray(DEFAULT_TOKENS, np.int32), np.ascontiguousarray(voice, np.float32)
    codes, n = np.full((2, 8), 7, np.int32), np.array([8, 3], np.int32)
    outs = [np.full((2, 9), 7, dt) for dt in (np.float32, np.float32, np.int32, np.float32)]

    def call(codes=codes, n=n, n_cand=2, stride=8, positions=0, toks=toks, n_text=len(toks)):
        return eng.L.tts_ar_score_codes(eng.h, p(toks), n_text, p(v), p(codes), p(n), n_cand, stride, positions, *[p(o) for o in outs])
    bad = codes.copy()
    bad[1, 2] = 8192
    early = codes.copy()
    early[1, 5] = 9999  # past the candidate's 3 codes: not read
    assert call(codes=bad) == ARG and call(n=np.array([8, 0], np.int32)) == ARG and call(n=np.array([9, 3], np.int32)) == ARG
    assert call(n_cand=0) == ARG and call(n_text=0) == ARG and call(positions=2) == ARG and call(positions=-1) == ARG
    assert call(n_cand=65, codes=np.zeros((65, 8), np.int32), n=np.full(65, 8, np.int32)) == LIMIT
    assert call(codes=np.zeros((1, 501), np.int32), n=np.array([501], np.int32), n_cand=1, stride=501) == LIMIT
    long_text = np.full(600, 5, np.int32)  # 1 + 600 + 500 + 1 positions
    big = np.zeros((1, 500), np.int32)
    assert eng.L.tts_ar_score_codes(eng.h, p(long_text), 600, p(v), p(big), p(np.array([500], np.int32)), 1, 500, 0, *[p(np.full(501, 7, o.dtype)) for o in outs]) == LIMIT
    eng.ar_session_open(2, 1, 16, 4)
    try:
        assert call() == STATE
    finally:
        eng.ar_session_close()
    assert all((o == 7).all() for o in outs), "a refused call wrote an output"
    assert call(codes=early) == 0
    assert (outs[0][1, 4:] == 7).all() and (outs[0][0] != 7).all() and (outs[3][1, :4] != 7).all() and (outs[3][1, 4:] == 7).all(), "entries past n + 1 are left alone"


def _clip(n, seed, rate=22050):
    g = np.random.default_rng(seed)
    t = np.arange(n) / rate
    return (0.3 * np.sin(2 * np.pi * (180 + 40 * seed) * t) + 0.05 * g.standard_normal(n)).astype(np.float32)


def test_scores_of_a_recordings_codes_and_the_cli_line(pkg, small_models, voice, tmp_path):
    import shutil
    import dvae_ref as D
    d = tmp_path / "models"
    d.mkdir()
    os.symlink(os.path.join(small_models, "ggml-model.bin"), d / "ggml-model.bin")
    shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    clips = [_clip(int(0.6 * 22050), 1), _clip(int(0.3 * 16000), 2, 16000)]
    rates = [22050, 16000]
    paths = []
    for i, (c, r) in enumerate(zip(clips, rates)):
        paths.append(str(tmp_path / ("c%d.wav" % i)))
        assert pkg.lib().tts_write_wav(paths[-1].encode(), c, len(c), r) == 0
    msg = "hello there world"
    e = pkg.Engine(0)
    e.load(ar=str(d / "ggml-model.bin"))
    e.tokenizer_load(str(d / "tokenizer.json"))
    e.load_dvae(D.model("mid")[0])
    codes = e.dvae_codes_audio(clips, rates)
    got = e.ar_score_codes(e.tokenize(msg), voice, codes, "train")
    e.close()
    assert all(len(g["logp"]) == len(c) + 1 and np.isfinite(g["logp"]).all() and (g["logp"] < 0).all() for g, c in zip(got, codes))
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    r = subprocess.run([exe, "--models", str(d), "--voice", os.path.join(ROOT, "models", "mol.bin"), "--message", msg, "--dvae", D.model("mid")[0],
                        "--score-audio", ",".join(paths)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("score: ")]
    assert len(lines) == 2
    for l, path, g, c in zip(lines, paths, got, codes):
        total = 0.0
        for x in g["logp"]:
            total += float(x)
        nll = -total / (len(c) + 1)
        hits = int((g["greedy"] == np.concatenate([c, [8193]])).sum())
        assert l[1] == path and int(l[2]) == len(c)
        assert l[3] == "%.9g" % total and l[4] == "%.9g" % nll and l[6] == "%.9g" % float(g["stop_logp"][-1]) and l[7] == "%.9g" % (hits / (len(c) + 1))
        assert abs(float(l[5]) - np.exp(nll)) <= 1e-8 * np.exp(nll)
