"""GPU: several prompts in one autoregressive pass (tts_ar_begin_multi / tts_autoregressive_multi) and the CLI's --split-text. A batch of G prompt groups
runs its decode steps in lock-step; only the context length differs per row. Every row must see exactly the numbers of its prompt run alone: the decode step
is batch-invariant bit for bit (tests/test_properties_gpu.py), and the per-row context offset must not change that."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import DEFAULT_TOKENS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prompt(n, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([[255], rs.randint(1, 250, n - 2), [0]]).astype(np.int32) if n > 2 else rs.randint(1, 250, n).astype(np.int32)


def step_tokens(i, B):
    return ((np.arange(B) * 131 + i * 37 + 5) % 8192).astype(np.int32)


@pytest.mark.parametrize("mode", ["f32", "fp16", "fp8", "ggml_lut"])
def test_step_logits_bit_identical_to_each_prompt_alone(pkg, mid_models, voice, mode):
    lens, n_cand, steps = [16, 66, 131, 404], [3, 1, 16, 2], 12
    prompts = [prompt(n, 10 + g) for g, n in enumerate(lens)]
    B = sum(n_cand)
    c0 = np.concatenate([[0], np.cumsum(n_cand)])
    eng = pkg.Engine(0)
    try:
        if mode in ("fp16", "fp8"):
            eng.set_option("ar_weights", 1 if mode == "fp16" else 2)
        if mode == "ggml_lut":
            eng.set_option("ggml_lut", 1)
        eng.load(ar=mid_models + "/ggml-model.bin")
        eng.ar_begin_multi(prompts, voice, n_cand, steps)
        multi = [eng.ar_prefill()]
        for i in range(steps):
            multi.append(eng.ar_step(step_tokens(i, B), i))
        multi = np.stack(multi)  # [steps + 1, B, 8194]
        assert np.isfinite(multi).all()
        lat_multi = None
        if mode == "f32":  # the latent pass: every candidate against its own prompt
            codes = np.full((B, 502), 83, np.int32)
            codes[:, 0] = 8192
            codes[:, 1:41] = (np.arange(40)[None] * 7 + 3 + np.arange(B)[:, None] * 11) % 8192
            lat_multi = eng.ar_latents(codes, 24)
        for g in range(len(lens)):
            eng.ar_begin(prompts[g], voice, n_cand[g], steps)
            alone = [eng.ar_prefill()]
            for i in range(steps):
                alone.append(eng.ar_step(step_tokens(i, B)[c0[g]:c0[g + 1]], i))
            alone = np.stack(alone)
            got = multi[:, c0[g]:c0[g + 1]]
            assert (got == alone).all(), (mode, g, np.abs(got - alone).max())
            if lat_multi is not None:
                la = eng.ar_latents(codes[c0[g]:c0[g + 1]], 24)
                assert (lat_multi[c0[g]:c0[g + 1]] == la).all(), (g, np.abs(lat_multi[c0[g]:c0[g + 1]] - la).max())
        # the step state of the batch is left as it was: a single-prompt begin afterwards is the single-prompt path again
        eng.ar_begin(DEFAULT_TOKENS, voice, 2, 4)
        assert np.isfinite(eng.ar_prefill()).all()
    finally:
        eng.close()


def _alone(eng, prompts, voice, n_cand, S, seed, stop_at=None, **kw):
    """each group as a single-prompt tts_autoregressive with the RNG shard of its candidates"""
    B, out = sum(n_cand), []
    c0 = np.concatenate([[0], np.cumsum(n_cand)])
    try:
        for g, p in enumerate(prompts):
            eng.set_option("rng_shard_offset", int(c0[g]))
            eng.set_option("rng_shard_total", B)
            if stop_at is not None:
                eng.set_stop_schedule(stop_at[c0[g]:c0[g + 1]])
            eng.seed(seed)
            codes, rows, lats, steps = eng.autoregressive(p, voice, n_cand[g], S, **kw)
            out.append((codes, rows, lats, steps, eng.ar_stop_status(n_cand[g])))
    finally:
        eng.set_option("rng_shard_offset", 0)
        eng.set_option("rng_shard_total", 0)
        eng.set_stop_schedule(None)
    return out


@pytest.mark.parametrize("retire", [False, True])
def test_driver_equals_each_prompt_alone(engine, pkg, mid_models, voice, retire):
    engine.load(ar=mid_models + "/ggml-model.bin")
    prompts = [prompt(16, 1), prompt(41, 2), prompt(9, 3)]
    n_cand, S, seed = [2, 3, 1], 20, 77
    B = sum(n_cand)
    stop_at = [5, 20, 7, 12, 9, 15] if retire else None  # candidates of different groups end at different steps (group 0 runs to max_steps)
    kw = dict(mask_stop=True, retire=retire)
    if retire:
        engine.set_stop_schedule(stop_at)
    try:
        engine.seed(seed)
        codes, rows, lats, steps = engine.autoregressive_multi(prompts, voice, n_cand, S, **kw)
        stopped = engine.ar_stop_status(B)
    finally:
        engine.set_stop_schedule(None)
    alone = _alone(engine, prompts, voice, n_cand, S, seed, stop_at, **kw)
    c0 = np.concatenate([[0], np.cumsum(n_cand)])
    assert steps == max(a[3] for a in alone)
    for g, (ca, ra, la, _, sa) in enumerate(alone):
        assert (codes[g] == ca).all() and (rows[g] == ra).all(), g
        assert (stopped[c0[g]:c0[g + 1]] == sa).all(), g
        for k in range(n_cand[g]):
            err = float(np.abs(lats[g][k] - la[k]).max() / np.abs(la[k]).max())
            assert lats[g][k].shape == la[k].shape and err <= 1e-4, (g, k, err)
    if retire:
        assert len(set(int(r) for rg in rows for r in rg)) > 2  # a ragged batch across groups


def test_one_prompt_is_the_existing_path(engine, pkg, small_models, voice, tmp_path):
    engine.load(ar=small_models + "/ggml-model.bin")
    engine.seed(5)
    ca, ra, la, sa = engine.autoregressive(DEFAULT_TOKENS, voice, 3, 16, mask_stop=True)
    engine.rng_save_state(str(tmp_path / "a.txt"))
    engine.seed(5)
    cb, rb, lb, sb = engine.autoregressive_multi([DEFAULT_TOKENS], voice, [3], 16, mask_stop=True)
    engine.rng_save_state(str(tmp_path / "b.txt"))
    assert sa == sb and (ca == cb[0]).all() and (ra == rb[0]).all()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(la, lb[0]))
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes()


def test_errors_leave_the_engine_usable(engine, pkg, small_models, voice):
    engine.load(ar=small_models + "/ggml-model.bin")
    ok = [prompt(12, 4), prompt(20, 5)]

    def expect(status, fn):
        with pytest.raises(pkg.TtsError, match="status %d" % status):
            fn()
        engine.seed(1)  # a valid call still works
        codes, rows, lats, steps = engine.autoregressive_multi(ok, voice, [1, 2], 4, mask_stop=True)
        assert steps == 4 and codes[1].shape == (2, 502)

    expect(-6, lambda: engine.autoregressive_multi([prompt(405, 6), ok[0]], voice, [1, 1], 4, mask_stop=True))  # a prompt of 405 ids
    expect(-6, lambda: engine.ar_begin_multi([prompt(404, 7), ok[0]], voice, [1, 1], 607))  # 404 + 2 + 607 + 1 positions: beyond the 608 mel / 1024 context
    expect(-1, lambda: engine.autoregressive_multi([], voice, [], 4, mask_stop=True))  # G = 0
    expect(-1, lambda: engine.autoregressive_multi(ok, voice, [1, 0], 4, mask_stop=True))  # n_cand = 0
    bad = ok[1].copy()
    bad[3] = 256
    expect(-1, lambda: engine.autoregressive_multi([ok[0], bad], voice, [1, 1], 4, mask_stop=True))  # a text id >= 256
    engine.set_stop_schedule([2, 3])
    try:
        expect(-1, lambda: engine.autoregressive_multi(ok, voice, [1, 2], 4, mask_stop=True, retire=True))  # schedule of 2 for 3 candidates
    finally:
        engine.set_stop_schedule(None)


def _cli(small_models, tmp_path, message, out, extra):
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    d = tmp_path / "models"
    if not d.exists():
        d.mkdir()
        for f in ("ggml-model.bin", "ggml-diffusion-model.bin", "ggml-vocoder-model.bin"):
            os.symlink(os.path.join(small_models, f), d / f)
        shutil.copy(os.path.join(ROOT, "models", "tokenizer.json"), d / "tokenizer.json")
    r = subprocess.run([exe, "--models", str(d), "--message", message, "--voice", os.path.join(ROOT, "models", "mol.bin"), "--seed", "3", "--codes", "24",
                        "--steps", "4", "--output", str(out)] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_split_text(pkg, small_models, tmp_path):
    short = "this is a test message."
    _cli(small_models, tmp_path, short, tmp_path / "plain.wav", [])
    _cli(small_models, tmp_path, short, tmp_path / "split.wav", ["--split-text", "200"])
    assert (tmp_path / "plain.wav").read_bytes() == (tmp_path / "split.wav").read_bytes()
    sentences = ["the quick brown fox jumps over the lazy dog number %s." % w for w in
                 ("one", "two", "three", "four", "five", "six", "seven", "eight", "nine", "ten", "eleven", "twelve", "thirteen", "fourteen", "fifteen",
                           "sixteen")]
    long_msg = " ".join(sentences)
    out = [tmp_path / "long1.wav", tmp_path / "long2.wav"]
    logs = [_cli(small_models, tmp_path, long_msg, o, ["--split-text", "200"]) for o in out]
    raw = out[0].read_bytes()
    assert raw == out[1].read_bytes()  # same seed, same bytes
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and int.from_bytes(raw[24:28], "little") == 24000
    frames = [int(l.split()[-3]) for l in logs[0].splitlines() if l.startswith("chunk ")]
    assert len(frames) >= 3, logs[0]
    n = (len(raw) - 44) // 4
    assert n == sum(pkg.lib().tts_vocoder_samples(t) for t in frames), (n, frames)
    # refused with several devices
    exe = os.path.join(ROOT, "tortoise.cpp_amd", "tortoise")
    r = subprocess.run([exe, "--message", long_msg, "--split-text", "200", "--devices", "2", "--output", str(tmp_path / "x.wav")], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--split-text" in r.stderr
